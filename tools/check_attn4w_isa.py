"""Safety check of attention4w.hip's asm-owned AGPR block.  The kernel keeps its O^T accumulators, Q and V^T fragments in AGPRs
that are NAMED in inline asm: the register allocator knows them only as clobbers, so a compiler-generated v_accvgpr_* (an AGPR
used as VGPR spill space) or any scratch access inside attn4w_kernel would silently corrupt them.  This compiles the file to
assembly with the library's flags and fails when either appears.      python tools/check_attn4w_isa.py [extra hipcc flags]

The row-resident kernels (mlp320w / qkv320w / qkv640w / geglu640w) depend on more than that: their generated streams wait with
counted vmcnt / lgkmcnt, so the ORDER of every memory, LDS, MFMA and wait instruction the compiler emits around the streams is
part of their correctness.  `skeleton()` extracts that order; to show that an edit of those files left it alone:
    python tools/check_attn4w_isa.py --compare OLD_TREE NEW_TREE [FILE:KERNEL ...]
(without FILE:KERNEL pairs, e.g. attention8.hip:attn8_kernel, the row-resident kernels are compared).  With --from=MNEMONIC in
front of the trees the ordered sequences are compared from the kernel's first MNEMONIC on (--from=s_barrier: an edit of the
prologue's scalar code, e.g. a kernel argument that went; see compare()).  Instantiations are paired
by demangled name; the OLD_TREE halves a kernel of DROPPED_ARG lost are reported as removed, any other instantiation that only one
tree has fails the comparison."""
import collections
import functools
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "instancediffusion_amd", "csrc", "attention4w.hip")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form".split()


ROW_KERNELS = [("mlp_fused.hip", "mlp320w_kernel"), ("mlp_fused.hip", "mlp320_kernel"), ("qkv_fused.hip", "qkv320w_kernel"),
               ("qkv640_fused.hip", "qkv640w_kernel"), ("geglu_fused.hip", "geglu640w_kernel")]
ORDERED = ("global_", "buffer_", "flat_", "scratch_", "ds_", "s_load", "s_barrier", "v_mfma", "v_accvgpr")
# kernels that lost a trailing template argument: the OLD_TREE instantiations with this value of it pair with the new ones
DROPPED_ARG = {}
# ... and the kernels bound by the descriptor and the COUNTED class counts only: every wait in them is the compiler's own (no
# inline-asm LDS-DMA, no hand-counted vmcnt), so a differing order is printed but does not fail the comparison
UNORDERED = ("gemm_kernel", "gemm_kernel_dma", "splitk_reduce_kernel")
COUNTED = ("v_mfma", "ds_", "global_", "s_barrier", "s_waitcnt")
# compare(start=...): the classes that may neither come nor go when the code in front of `start` (scalar loads, their waits) moves
COUNTED_FROM = ("v_mfma", "ds_", "global_", "buffer_", "scratch_", "s_barrier")
DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


@functools.lru_cache(maxsize=None)
def listing(src, extra=()):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "a.s")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       cwd=os.path.dirname(src), stderr=subprocess.DEVNULL)
        return open(out).read()


def bodies(txt, kernel):
    """[(mangled name, text from the kernel's label to its s_endpgm)], one per instantiation"""
    return re.findall(r"\n(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)\n\ts_endpgm", txt, flags=re.S)


def skeleton(src, kernel, extra=()):
    """per instantiation (keyed by its demangled name, without the return type and the argument list): seq = the ordered memory / LDS / MFMA / AGPR mnemonics and every s_waitcnt
    WITH its operands; mnemonics = the multiset of all instructions; desc = the kernel descriptor's register and segment sizes"""
    txt = listing(src, tuple(extra))
    found = bodies(txt, kernel)
    plain = subprocess.run(["c++filt"], input="\n".join(n for n, _ in found), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    out = {}
    for (name, body), dem in zip(found, plain):
        key = re.search(r"\b" + kernel + r"(<.*>)?(?=\()", dem)
        if not key:                                  # another kernel whose name merely contains this one's
            continue
        seq, mnem = [], collections.Counter()
        for line in body.split("\n"):
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            m = t.split()[0]
            mnem[m] += 1
            if m == "s_waitcnt":
                seq.append(" ".join(t.split()))
            elif m.startswith(ORDERED):
                seq.append(m)
        blk = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S).group(1)
        desc = {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", blk).group(1)) for k in DESCRIPTOR}
        out[key.group(0)] = dict(seq=seq, mnemonics=mnem, desc=desc)
    return out


def compare(old_tree, new_tree, kernels=ROW_KERNELS, start=None):
    """0 when every kernel of `kernels` [(file, kernel)] in new_tree has the ordered sequence (UNORDERED kernels: the COUNTED class
    counts) and the descriptor of old_tree's, and no instantiation came or went but the halves a DROPPED_ARG kernel lost;
    prints the instructions added / removed where the mnemonic multisets differ (address arithmetic may; nothing else should).
    start: compare the ordered sequences from the first occurrence of this mnemonic on, and let s_waitcnt come and go (COUNTED_FROM)"""
    bad = False
    counted = COUNTED_FROM if start else COUNTED
    tail = lambda seq: seq[seq.index(start):] if start in seq else seq
    for f, kernel in kernels:
        a, b = (skeleton(os.path.join(t, "instancediffusion_amd", "csrc", f), kernel) for t in (old_tree, new_tree))
        if kernel in DROPPED_ARG:
            a = {re.sub(", " + DROPPED_ARG[kernel] + ">$", ">", k): v for k, v in a.items()}
        for k in sorted(set(a) - set(b)):
            expected = kernel in DROPPED_ARG and re.search(", (true|false)>$", k)       # the other value of the dropped argument
            print(f"{k}: removed" if expected else f"{k}: MISSING from {new_tree}")
            bad |= not expected
        for k in sorted(set(b) - set(a)):
            print(f"{k}: NEW, no instantiation of {old_tree} to compare with")
        bad |= bool(set(b) - set(a)) or not b
        for k in sorted(set(a) & set(b)):
            same_seq, same_desc = tail(a[k]["seq"]) == tail(b[k]["seq"]), a[k]["desc"] == b[k]["desc"]
            add, rem = b[k]["mnemonics"] - a[k]["mnemonics"], a[k]["mnemonics"] - b[k]["mnemonics"]
            same_cls = not any(m.startswith(counted) for m in (*add, *rem))
            print(f"{k}: {len(tail(b[k]['seq']))} ordered entries {'same' if same_seq else 'DIFFER'}; descriptor {b[k]['desc']} "
                  f"{'same' if same_desc else 'DIFFERS from ' + str(a[k]['desc'])}; {sum(b[k]['mnemonics'].values())} instructions"
                  f" added {dict(add)} removed {dict(rem)}")
            bad |= not (same_desc and same_cls and (same_seq or kernel in UNORDERED))
    return 1 if bad else 0


def check(extra=(), src=SRC, kernel="attn4w_kernel"):
    """src / kernel: the same scan for another file with asm-owned AGPRs (mlp_fused.hip's mlp320w_kernel)"""
    report = {}
    for name, body in bodies(listing(src, tuple(extra)), kernel):
        in_asm, stray, scratch, mfma = False, [], 0, 0
        for line in body.split("\n"):
            t = line.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
            elif t.startswith(";;#ASMEND"):
                in_asm = False
            elif t.startswith("v_accvgpr") and not in_asm:
                stray.append(t)
            elif t.startswith("scratch_"):
                scratch += 1
            elif t.startswith("v_mfma"):
                mfma += 1
        report[name] = dict(stray_accvgpr=stray, scratch_ops=scratch, mfma=mfma)
    return report


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"]:
        start = sys.argv.pop(2)[len("--from="):] if sys.argv[2].startswith("--from=") else None
        pairs = [tuple(a.split(":", 1)) for a in sys.argv[4:]] or ROW_KERNELS
        sys.exit(compare(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]), pairs, start))
    rep = check(sys.argv[1:])
    bad = False
    for k, v in rep.items():
        print(k, "stray v_accvgpr:", len(v["stray_accvgpr"]), "scratch ops:", v["scratch_ops"], "mfma:", v["mfma"])
        bad |= bool(v["stray_accvgpr"]) or v["scratch_ops"] > 0
    if not rep:
        print("no attn4w kernel found")
        bad = True
    sys.exit(1 if bad else 0)
