"""The scheduler shared by the generators of the row kernels' instruction streams (gen_qkvw_stream.py, gen_qkv640w_stream.py,
gen_gegluw_stream.py -> instancediffusion_amd/csrc/*_stream.inc; gen_mlpw_stream.py, the first of the family, keeps its own
scheduling loop and uses the `Stream` counter, `header` and `finish` of this module).

A stream is ONE wave's program for one pipeline step: every statement becomes an `asm volatile` primitive of csrc/mw_prims.h, so
the order written here is the order issued.  The rules:
  * the step's MFMAs are the backbone; "gap g" is the room behind MFMA g (a 32 x 32 x 16 MFMA occupies the matrix pipe for 32
    cycles: ~4-6 other instructions issue under it for free)
  * LDS operations -- reads AND writes -- retire in order through one counter: `Stream` numbers them, and a consumer waits with
    the exact s_waitcnt lgkmcnt(N) that lets every younger operation stay in flight
  * a W fragment read is issued LA gaps ahead of its MFMA, a constant read of the epilogue min(LA, 2) gaps ahead of the gap of
    its first use, never more than 13 outstanding (the counter has 4 bits)
  * the LDS-DMA pieces of the next W chunk go in front of the first MFMA (PRE_DMA of them) and one per gap behind it; the
    epilogue of the previous work item is spread over the gaps behind the pieces, at most MAXV statements per gap, the rest
    trails the last MFMA
An epilogue is a list of (kind, code, needs, defines): kind 'r' a hoistable LDS read, 'l' an LDS operation that stays in place
(a write, or the read-back of a staging image), 's' any other statement; `needs` names the reads it consumes.

`Gen` is what a generator script is made of besides its epilogues: the options <PREFIX>_LA / _PRE_DMA / _MAXV (and the timing
experiments _NO_EPI / _NO_DMA = 1: wrong results) from the environment, the declaration of a stream function, and the file.
`mf_items640` / `dma_pieces640` / `XLOAD640` are the MFMA backbone, the LDS-DMA pieces and the next-tile fetch of the K = 640
kernels (csrc/mw_row.h Row640: one 32 x 32 fragment, 40 k-steps on two accumulators, ten K-tiles per chunk).
"""
import os
import sys


class Stream:
    """statements in issue order; LDS operations (reads AND writes) are counted: a wait for read r is lgkmcnt(issued - seq(r) - 1)"""

    def __init__(self):
        self.lines, self.issued, self.done, self.seq = [], 0, 0, {}

    def lds(self, code, name=None):
        self.lines.append("  " + code)
        if name:
            self.seq[name] = self.issued
        self.issued += 1

    def wait(self, name):
        s = self.seq[name]
        if s < self.done:
            return
        n = self.issued - s - 1
        assert 0 <= n <= 15, (name, n)
        self.lines.append(f"  mw_wait_lgkm<{n}>();")
        self.done = s + 1

    def stmt(self, code, needs=()):
        for r in needs:
            self.wait(r)
        self.lines.append("  " + code)


ARGS = "f32x16 (&accC)[2], f32x16 (&accN)[2], const {ctx}& c"     # accC: the item in its epilogue, accN: the one in its MFMAs


def schedule(decl, mfs, pieces, items, la, pre_dma, maxv, top=None, xload=None):
    """One stream as the text of a __device__ function.
    decl: the function's declaration; mfs: [(MFMA statement, read name, read statement)]; pieces: the LDS-DMA statements;
    items: the epilogue (module docstring); top: the statement that opens the step (wait + barrier) or None; xload: the next
    tile's row fetch (last step of a tile) or None."""
    st = Stream()
    st.lines.append(decl + " {")
    if top:
        st.lines.append("  " + top)
    ngap = len(mfs)
    pre, rest = pieces[:pre_dma], pieces[pre_dma:]
    # epilogue statements over the gaps behind the DMA pieces
    vgaps = list(range(min(len(rest), ngap), ngap))
    per_gap = {g: [] for g in range(ngap + 1)}
    n_under = min(len(items), maxv * len(vgaps))
    for k in range(n_under):
        per_gap[vgaps[k * len(vgaps) // n_under]].append(items[k])
    for k in range(n_under, len(items)):
        per_gap[ngap].append(items[k])
    hoist = []                              # (need gap, order, code, name, gaps ahead)
    for g, (_, rn, rc) in enumerate(mfs):
        hoist.append((g, 1, rc, rn, la))
    for g in range(ngap + 1):
        for kind, code, needs, defs in per_gap[g]:
            if kind == "r":
                hoist.append((g, 0, code, defs, min(la, 2)))
    hoist.sort(key=lambda h: (h[0], h[1]))
    hp = [0]

    def issue_upto(gap):
        while hp[0] < len(hoist):
            need, _, code, rn, ahead = hoist[hp[0]]
            if need - ahead > gap or st.issued - st.done >= 13:
                break
            st.lds(code, rn)
            hp[0] += 1

    def force(rn):                          # a consumer is about to wait for rn: it must have been issued
        while rn not in st.seq:
            _, _, code, r2, _ = hoist[hp[0]]
            st.lds(code, r2)
            hp[0] += 1

    def emit(kind, ecode, needs, defs):
        if kind == "r":
            return
        for r in needs:
            force(r)
        if kind == "l":
            for r in needs:
                st.wait(r)
            st.lds(ecode, defs)
        else:
            st.stmt(ecode, needs)

    if xload:
        st.lines.append("  " + xload)
    issue_upto(0)
    for s in pre:
        st.lines.append("  " + s)
    for g in range(ngap):
        code, rn, _ = mfs[g]
        issue_upto(g)
        force(rn)
        st.stmt(code, [rn])
        issue_upto(g + 1)
        if g < len(rest):
            st.lines.append("  " + rest[g])
        for it in per_gap[g]:
            emit(*it)
    for s in rest[ngap:]:
        st.lines.append("  " + s)
    for it in per_gap[ngap]:
        emit(*it)
    assert hp[0] == len(hoist), (decl, hp[0], len(hoist))
    st.lines.append("}")
    return "\n".join(st.lines)


def header(script, la, pre_dma, maxv=None):
    tail = f", <= {maxv} epilogue statements per gap." if maxv is not None else "."
    return [f"// GENERATED by tools/{script} -- do not edit; see that script for the schedule rules.",
            f"// LA = {la} gaps of LDS-read lookahead, {pre_dma} LDS-DMA pieces in front of the first MFMA{tail}", ""]


def finish(parts, out):
    """write the .inc; `-o FILE` writes a variant elsewhere, `--check` exits 1 when the checked-in file is stale"""
    txt = "\n\n".join(parts) + "\n"
    if "-o" in sys.argv:
        open(sys.argv[sys.argv.index("-o") + 1], "w").write(txt)
        return
    if "--check" in sys.argv:
        cur = open(out).read() if os.path.exists(out) else ""
        sys.exit(0 if cur == txt else 1)
    open(out, "w").write(txt)
    print("wrote", out, len(txt.split("\n")), "lines")


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def csrc(name):
    return os.path.join(ROOT, "instancediffusion_amd", "csrc", name)


class Gen:
    def __init__(self, script, out, prefix, ctx, la, pre_dma, maxv, tmpl="int DT, int VMC", top="mw_wait_vm_barrier<VMC>();", xload=None):
        env = os.environ
        self.script, self.out, self.ctx, self.tmpl, self.top, self.xload = script, csrc(out), ctx, tmpl, top, xload
        self.LA, self.PRE_DMA, self.MAXV = (int(env.get(f"{prefix}_{k}", d)) for k, d in (("LA", la), ("PRE_DMA", pre_dma), ("MAXV", maxv)))
        self.NO_EPI, self.NO_DMA = env.get(f"{prefix}_NO_EPI") == "1", env.get(f"{prefix}_NO_DMA") == "1"
        self.parts = header(script, self.LA, self.PRE_DMA, self.MAXV)

    def add(self, name, mfs, pieces, items, top=True, xload=False):
        """one stream: the MFMAs `mfs` with their `pieces`, the epilogue `items` of the work item before"""
        decl = f"template <{self.tmpl}> __device__ __forceinline__ void {name}({ARGS.format(ctx=self.ctx)})"
        self.parts.append(schedule(decl, mfs, [] if self.NO_DMA else pieces, [] if self.NO_EPI else items, self.LA, self.PRE_DMA, self.MAXV,
                                   top=self.top if top else None, xload=self.xload if xload else None))

    def finish(self):
        finish(self.parts, self.out)


def mf_items640(fn="mw_mf1"):
    """fn: mw_mf1 (a lane owns a token) or mw_mf1t (operands swapped: a lane owns a W row)"""
    out = []
    for ks in range(40):
        name = f"w_{ks}"
        first = "true" if ks < 2 else "false"
        out.append((f"{fn}<DT, {ks}, {first}>(accN[{ks & 1}], {name});", name,
                    f"const u32x4 {name} = mw_lds128<{(ks >> 2) * 4096}>(c.w1a[{ks & 3}]);"))
    return out


def dma_pieces640():
    return [f"mw_dma<{kt * 4096}, {kt * 128}>(c.w1dst, c.w1_vj, c.wb);" for kt in range(10)]


XLOAD640 = ("if (c.has_next) { mw_static_for<40>([&](auto kc) { mw_load_x2<decltype(kc)::value, decltype(kc)::value>(c.xnext); }); "
            "asm volatile(\"global_load_dwordx2 a[160:161], %0, off\" ::\"v\"(c.snext) : \"memory\"); }")
