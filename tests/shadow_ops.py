"""A recording judge around any ops object (``HipOps`` on the GPU, ``EmulOps`` on the CPU): ``ShadowOps(inner, dt)`` is handed to an
engine as ``ops=`` and holds EVERY launch the engine issues to the fp64 reference of that op, with the arguments exactly as the
engine built them -- views, strides, aliasing, keyword combinations.  Needs no GPU and no HIP library to import;
tests/test_shadow_ops_refs.py proves it on the CPU, tests/test_engine_launches_gpu.py applies it to the kernels.

One call of a judged op (``JUDGED``):
  1. snapshot: every tensor argument is copied; of every tensor the op may write the WHOLE underlying storage is copied, and the
     snapshots of tensors that share such a storage are views into that copy (``out`` may alias ``res`` / ``x``);
  2. the inner op runs with the original arguments, the judge synchronises, the return value is handed back unchanged;
  3. the project's fp64 reference of the op (tests/gemm_conv_cases.py, attention_cases.py, row_kernel_cases.py, small_kernel_cases.py --
     none shares code with tests/emul_ops.py) is evaluated on the snapshots, on the device the inner ops live on;
  4. the result is judged with the bound that reference's own module defines; 0 elements may lie outside, a NaN is outside;
  5. stray writes: every element of a written storage outside the views the op was handed is bit-identical to the snapshot, and so is
     every input that is not an output (and ``out`` itself when ``conv_up2x`` / ``conv3x3_skip`` decline the launch);
  6. one record per launch (``records``, ``line``): index, op, shapes, strides, flags, engine buffer roles, err/bound, elements outside.
A launch that fails raises ``LaunchOutside`` carrying its record (``strict=False``: it is only recorded).

Every other attribute is the inner object's.  Callables among them -- ``empty``, ``zeros``, the static helpers, the sampler step ops that
their own GPU tests pin bit for bit -- are counted by name in ``passed``: a test compares that set with an explicit allow-list, so a
new op cannot slip past unjudged.

ROW SAMPLING.  A launch with at most ``row_cap`` (1024) output rows -- GEMM rows, output pixels, attention queries -- is judged whole.
A larger one is judged on exactly ``row_cap`` rows: its first 64 and last 64; for a conv every pixel of the first and last image row
and column of the first and last sample (when those are at most 512); one seeded row of every batch entry; a seeded sample of the
rest.  Normalisations and the other bandwidth ops are always judged whole, and so are the stray-write checks.

THE CONV REFERENCE ON SAMPLED PIXELS.  ``conv_rows_ref`` gathers the nine taps of the sampled output pixels and multiplies in fp64;
tests/test_shadow_ops_refs.py proves it equal to ``gemm_conv_cases.conv3x3_ref`` (1e-13 relative) for stride 1 and 2, up 0 and 1,
pad_lo 0 and 1.  ``conv_up2x_rows_ref`` is the four 2x2 phase convolutions straight from ``pack_conv_up2x``'s images in the same form.

STATISTICS BY-PRODUCTS.  ``out_stats``: ``gemm_conv_cases.out_stats_excess`` (<= 1).  ``ln_stats_out`` and ``row_stats``:
``small_kernel_cases.row_stats_ref`` of the rows; the mean within the fp32 bar (1e-5 of max|a|) and rstd within 1e-4 relative (the
LN_STATS_TOL of tests/test_gemm_big_walk_gpu.py).  ``gn_partial``: ``gemm_conv_cases.gn_partial_errors`` of the STORED output within
(2e-5 chunk standard deviations, 2e-4 relative M2), the GN_PARTIAL_TOL of the same module.  The q | k | v launches the row-resident
kernel takes (its launch counter moves) get the 2^-16 rstd |mu| |c| of tests/row_kernel_cases.py on top of ``gemm_ref``'s slack.
"""
from __future__ import annotations

import torch

from tests import attention_cases as AC
from tests import gemm_conv_cases as K
from tests import row_kernel_cases as RK
from tests import small_kernel_cases as SK

ROW_CAP = 1024
LN_STATS_TOL = 1e-4
GN_PARTIAL_TOL = (2e-5, 2e-4)
F32_BAR = 1e-5

JUDGED = ("gemm", "conv3x3", "conv3x3_down", "conv3x3_skip", "conv_up2x", "attention", "attention_causal", "attention_qkv", "softmax_rows",
          "mlp_geglu", "groupnorm", "layernorm", "row_stats", "layernorm_patch2", "dwconv7x7", "seg_in_conv", "scaleu_concat",
          "timestep_embedding", "unifusion_embed", "conv_in", "clip_embed", "clip_patchify", "cast16", "pointwise_nchw", "vae_posterior")
# what an engine forward may call beside the judged ops: allocation and the static helpers
HELPERS = frozenset({"empty", "zeros", "gn_partial_shape", "mlp_supported", "mlp_pack", "proj_row_takes"})


class LaunchOutside(AssertionError):
    def __init__(self, record, line):
        super().__init__(line)
        self.record = record
        self.index = record["index"]


# ---- storage, bits, masks ----------------------------------------------------------------------------------------------------------
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _flat(t):
    """The whole storage under ``t`` as a flat tensor of t's dtype."""
    st = t.untyped_storage()
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(st, 0, (st.nbytes() // t.element_size(),), (1,))


def _bits(t):
    return t.view(_INT[t.element_size()]) if t.dtype != torch.bool else t


def _same_bits(a, b):
    return bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


def _view_index(t):
    """Storage element indices the view ``t`` covers (flat int64 on t's device), or a (lo, hi) range for a contiguous view."""
    off = t.storage_offset()
    if t.is_contiguous():
        return (off, off + t.numel())
    idx = torch.full((1,) * t.dim(), off, dtype=torch.int64, device=t.device)
    for d, (n, s) in enumerate(zip(t.shape, t.stride())):
        shape = [1] * t.dim()
        shape[d] = n
        idx = idx + (torch.arange(n, device=t.device, dtype=torch.int64) * s).view(shape)
    return idx.reshape(-1)


def sample_rows(total, cap, seed, batch_rows=0, border=None):
    """Sorted int64 row indices of a launch with ``total`` output rows (module docstring), or None: judge every row."""
    if total <= cap:
        return None
    rows = set(range(64)) | set(range(total - 64, total))
    if border is not None and len(border) <= 512:
        rows |= set(border)
    g = torch.Generator().manual_seed(7919 + seed)
    if batch_rows and total // batch_rows <= cap - len(rows):
        nb = total // batch_rows
        pick = torch.randint(0, batch_rows, (nb,), generator=g)
        rows |= {b * batch_rows + int(pick[b]) for b in range(nb)}
    for r in torch.randperm(total, generator=g).tolist():
        if len(rows) >= cap:
            break
        rows.add(r)
    return torch.tensor(sorted(rows), dtype=torch.int64)


def conv_border_rows(B, Ho, Wo):
    """Flat output-pixel indices of the first and last image row and column of the first and last sample."""
    out = set()
    for b in {0, B - 1}:
        base = b * Ho * Wo
        for x in range(Wo):
            out.add(base + x)
            out.add(base + (Ho - 1) * Wo + x)
        for y in range(Ho):
            out.add(base + y * Wo)
            out.add(base + y * Wo + Wo - 1)
    return out


# ---- references on sampled rows -----------------------------------------------------------------------------------------------------
def unpack_geglu(t, period):
    """The inverse of ``engine.pack_geglu`` on the leading dimension: period-P image [P/2 value | P/2 gate] -> [value rows | gate rows]."""
    h, n2 = period // 2, t.shape[0]
    blk = t.reshape(n2 // period, 2, h, *t.shape[1:])
    return torch.cat([blk[:, 0].reshape(n2 // 2, *t.shape[1:]), blk[:, 1].reshape(n2 // 2, *t.shape[1:])], 0)


def _gather_taps(x, b, oy, ox, offsets, stride, up, pad_lo):
    """x [B, H, W, Cin]; for the output pixels (b, oy, ox) the taps at (dy, dx) in ``offsets``: pixel (oy*stride + dy - pad_lo, ..) of the
    (nearest-x2 upsampled when ``up``) image, zero outside -> [n, len(offsets) * Cin] in x's dtype."""
    _, H, W_, Cin = x.shape
    Hu, Wu = H << up, W_ << up
    cols = []
    for dy, dx in offsets:
        iy, ix = oy * stride + dy - pad_lo, ox * stride + dx - pad_lo
        ok = (iy >= 0) & (iy < Hu) & (ix >= 0) & (ix < Wu)
        v = x[b, (iy.clamp(0, Hu - 1) >> up), (ix.clamp(0, Wu - 1) >> up)]
        cols.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


def _pixel_index(rows, Ho, Wo):
    return rows // (Ho * Wo), rows % (Ho * Wo) // Wo, rows % Wo


TAPS3 = [(ky, kx) for ky in range(3) for kx in range(3)]


def conv_rows_ref(x, w, rows, *, bias=None, rowbias=None, res=None, stride=1, up=0, pad_lo=1, cd=torch.float64):
    """``gemm_conv_cases.conv3x3_ref`` on the output pixels ``rows`` (flat (b, oy, ox) indices, on x's device) as a gather of their taps
    and one fp64 matmul: -> (want, slack) [len(rows), Cout]."""
    B, H, W_, Cin = x.shape
    Ho, Wo = K.conv_out_hw(H, W_, stride, up, pad_lo)
    b, oy, ox = _pixel_index(rows, Ho, Wo)
    a = _gather_taps(x, b, oy, ox, TAPS3, stride, up, pad_lo)
    y = a.to(cd) @ w.to(cd).t()
    mag = a.double().abs() @ w.double().abs().t()
    if bias is not None:
        y = y + bias.to(cd)
    if rowbias is not None:
        y = y + rowbias.to(cd)[b]
    if res is not None:
        y = y + res.to(cd)[b, oy, ox]
    return y, 9 * Cin * K.EPS32 * mag


def conv_up2x_rows_ref(x, wf, rows, bias=None, cd=torch.float64):
    """Nearest-x2 + 3x3 pad-1 conv as the four 2x2 phase convolutions of ``engine.pack_conv_up2x``'s images wf [4, Cout, 4*Cin]: output
    pixel (2y + py, 2x + px) reads source pixels (y - 1 + py + ty, x - 1 + px + tx) against wf[py*2 + px][:, (ty*2 + tx)*Cin + ci].
    -> (want, slack) [len(rows), Cout], slack = 4 Cin 2^-24 |x| |wf|."""
    B, H, W_, Cin = x.shape
    Cout = wf.shape[1]
    b, oy, ox = _pixel_index(rows, 2 * H, 2 * W_)
    want = torch.zeros(rows.numel(), Cout, dtype=cd, device=x.device)
    slack = torch.zeros(rows.numel(), Cout, dtype=torch.float64, device=x.device)
    for py in range(2):
        for px in range(2):
            m = ((oy & 1) == py) & ((ox & 1) == px)
            if not bool(m.any()):
                continue
            y0, x0 = (oy[m] >> 1) - 1 + py, (ox[m] >> 1) - 1 + px
            a = _gather_taps(x, b[m], y0, x0, [(0, 0), (0, 1), (1, 0), (1, 1)], 1, 0, 0)
            wp = wf[py * 2 + px]
            want[m] = a.to(cd) @ wp.to(cd).t()
            slack[m] = 4 * Cin * K.EPS32 * (a.double().abs() @ wp.double().abs().t())
    if bias is not None:
        want = want + bias.to(cd)
    return want, slack


def layernorm_patch2_fast(x, gamma, beta, eps):
    """``small_kernel_cases.layernorm_patch2_ref`` without the Python loops (proved equal in tests/test_shadow_ops_refs.py)."""
    B, H, W_, C = x.shape
    y = SK.layernorm_ref(x, gamma, beta, eps)
    return y.reshape(B, H // 2, 2, W_ // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W_ // 2), 4 * C)


def seg_in_conv_fast(segs, w, bias):
    """``small_kernel_cases.seg_in_conv_ref`` without the Python loops (proved equal in tests/test_shadow_ops_refs.py)."""
    B, _, S, _ = segs.shape
    y = torch.nn.functional.conv2d(segs.double(), w.double(), bias.double(), padding=1)
    P = S // 4
    return y.reshape(B, 3, P, 4, P, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * P * P, 48)


def gn_stats_from_partial(partial, HW, C):
    """(mean, variance) [B, 32] fp64 of the (mean, M2) chunk partials [B, nch, 32, 2] a conv leaves (equal counts per chunk)."""
    nch = partial.shape[1]
    n = (HW // nch) * (C // 32)
    pm, pq = partial[..., 0].double(), partial[..., 1].double()
    mu = pm.mean(1)
    return mu, (pq.sum(1) + n * (pm - mu[:, None]).pow(2).sum(1)) / (n * nch)


def _outside(got, want, slack, dt, f32out=False):
    """``gemm_conv_cases.outside`` (it judges on the CPU) of a reference that was evaluated on the device."""
    return K.outside(got, want.cpu(), slack.cpu(), dt, f32out)


def _pick(t, b):
    return t[b] if (t is not None and t.dim() == 3) else t


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
class ShadowOps:
    def __init__(self, inner, dt, row_cap=ROW_CAP, strict=True, engine=None):
        self.__dict__.update(inner=inner, judge_dt=dt, row_cap=row_cap, strict=strict, engine=engine, records=[], passed=set(),
                             returned={})

    def __getattr__(self, name):
        inner = self.__dict__["inner"]
        attr = getattr(inner, name)                          # AttributeError when the inner ops lack it: hasattr stays true to inner
        if name in JUDGED:
            return lambda *a, **k: self._run(name, attr, a, k)
        if callable(attr) and not name.startswith("_"):
            def counted(*a, **k):
                self.passed.add(name)
                return attr(*a, **k)
            return counted
        return attr

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------------
    def _sync(self):
        if self.inner.device.type == "cuda":
            torch.cuda.synchronize()

    def _roles(self, tensors):
        eng = self.engine
        if eng is None:
            return {}
        by_ptr = {}
        for (role, _, _), buf in eng._bufs.items():
            by_ptr.setdefault(buf.untyped_storage().data_ptr(), role)
        return {n: by_ptr.get(t.untyped_storage().data_ptr(), "-") for n, t in tensors.items()}

    @staticmethod
    def line(r):
        parts = " ".join(f"{p['part']}: err/bound {p['ratio']:.3g} outside {p['outside']} rows {p['rows']}/{p['total']}" for p in r["parts"])
        args = " ".join(f"{n}{list(s)}/{list(st)}@{r['roles'].get(n, '-')}" for n, (s, st) in r["args"].items())
        return (f"launch {r['index']} {r['op']} [{r['flags']}] {args} | {parts} | stray {r['stray']} inputs_modified {r['inputs_modified']}"
                f"{' | ' + r['note'] if r['note'] else ''}")

    def summary(self):
        """{op: dict(launches, worst, rows, total)} of the judged launches so far."""
        out = {}
        for r in self.records:
            s = out.setdefault(r["op"], dict(launches=0, worst=0.0, rows=0, total=0, outside=0))
            s["launches"] += 1
            for p in r["parts"]:
                s["worst"] = max(s["worst"], p["ratio"])
                s["outside"] += p["outside"]
            if r["parts"]:
                s["rows"] += r["parts"][0]["rows"]
                s["total"] += r["parts"][0]["total"]
        return out

    def print_summary(self, what):
        for op, s in sorted(self.summary().items()):
            print(f"[launches] {what} {op}: {s['launches']} judged, worst err/bound {s['worst']:.3f}, outside {s['outside']}, "
                  f"rows {s['rows']}/{s['total']}")
        print(f"[launches] {what}: passed through unjudged: {sorted(self.passed)}")

    def failures(self):
        return [r for r in self.records if not r["ok"]]

    # ---- one launch --------------------------------------------------------------------------------------------------------------
    def _run(self, name, fn, args, kw):
        index = len(self.records)
        plan = getattr(self, "_plan_" + name)(*args, **kw)
        tensors = {n: t for n, t in plan["tensors"].items() if t is not None}
        writes = {n: v for n, v in plan["writes"].items() if v is not None}        # name -> the view the op may write
        # 1. snapshot
        stores = {}                                                                # storage ptr -> [flat live, flat snapshot, tensor]
        for n in writes:
            t = tensors[n]
            p = t.untyped_storage().data_ptr()
            if p not in stores:
                live = _flat(t)
                stores[p] = [live, live.clone()]
        snap = {}
        for n, t in tensors.items():
            p = t.untyped_storage().data_ptr()
            if p in stores and stores[p][0].dtype == t.dtype:
                snap[n] = torch.as_strided(stores[p][1], t.shape, t.stride(), t.storage_offset())
            else:
                snap[n] = t.clone()
        pre = plan.get("pre")
        state = pre() if pre else None
        # 2. launch
        ret = fn(*args, **kw)
        self._sync()
        self.returned.setdefault(name, []).append(ret if isinstance(ret, bool) else None)
        declined = ret is False and name in ("conv_up2x", "conv3x3_skip")
        # 3./4. reference and judgement
        parts, note = [], ""
        if not declined:
            with torch.no_grad():
                parts = plan["judge"](snap, tensors, index, state) or []
        else:
            note = "launch declined"
        # 5. stray writes, inputs
        stray = 0
        for p, (live, old) in stores.items():
            changed = _bits(live) != _bits(old)
            if not declined:
                for n, view in writes.items():
                    if tensors[n].untyped_storage().data_ptr() == p:
                        idx = _view_index(view)
                        if isinstance(idx, tuple):
                            changed[idx[0]:idx[1]] = False
                        else:
                            changed[idx] = False
            stray += int(changed.sum())
        modified = [n for n, t in tensors.items()
                    if t.untyped_storage().data_ptr() not in stores and not _same_bits(t, snap[n])]
        ok = stray == 0 and not modified and all(p["outside"] == 0 for p in parts)
        rec = dict(index=index, op=name, flags=plan.get("flags", ""), args={n: (tuple(t.shape), tuple(t.stride())) for n, t in tensors.items()},
                   roles=self._roles(tensors), parts=parts, stray=stray, inputs_modified=modified, ok=ok, note=note)
        self.records.append(rec)
        if not ok and self.strict:
            raise LaunchOutside(rec, self.line(rec))
        return ret

    def _part(self, part, bad, ratio, rows, total):
        return dict(part=part, outside=int(bad), ratio=float(ratio), rows=int(rows), total=int(total))

    def _f32out(self, out):
        return out.dtype == torch.float32 and self.inner.dtype != torch.float32

    # ---- GEMM --------------------------------------------------------------------------------------------------------------------
    def _qkv_row_launches(self):
        lib = getattr(self.inner, "lib", None)
        if lib is None:
            return None
        from instancediffusion_amd import _lib
        return lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES)

    def _plan_gemm(self, a, w, out, *, bias=None, rowbias=None, rows_per_batch=0, res=None, gate=None, act=None, geglu=False,
                   geglu_period=64, ln_row=None, ln_col=None, out_stats=None, out_stats_eps=1e-5, ln_eps=1e-5, ln_stats_out=None,
                   vt_out=None):
        M = a.shape[-2]
        T = dict(a=a, w=w, out=out, bias=bias, rowbias=rowbias, res=res, gate=gate, out_stats=out_stats, ln_stats_out=ln_stats_out,
                 vt_out=vt_out)
        if ln_row is not None:
            T["ln_row.stats"], T["ln_row.c"] = ln_row
        if ln_col is not None:
            T["ln_col.stats"], T["ln_col.c"], T["ln_col.d"] = ln_col
        flags = "+".join(k for k, v in {"bias": bias, "rowbias": rowbias, "res": res, "gate": gate, act: act, f"geglu{geglu_period}": geglu or None,
                                            "ln_row": ln_row, "ln_col": ln_col, "out_stats": out_stats, "ln_stats_out": ln_stats_out, "vt_out": vt_out,
                                            "f32out": self._f32out(out) or None, "batched": out.dim() == 3 or None}.items()
                         if v is not None)
        dt = self.judge_dt

        def judge(S, L, index, qkv_before):
            batched = L["out"].dim() == 3
            Bt = L["out"].shape[0] if batched else 1
            total = Bt * M
            sel = sample_rows(total, self.row_cap, index, batch_rows=M if batched else rows_per_batch)
            dev = S["a"].device
            split16 = qkv_before is not None and vt_out is not None and self._qkv_row_launches() != qkv_before
            wants, slacks, gots, got_vt, got_os, got_ls, a_rows = [], [], [], [], [], [], []
            wk, bk = S["w"], S.get("bias")
            for b in range(Bt):
                if sel is None:
                    m = torch.arange(M, device=dev)
                else:
                    m = (sel[(sel >= b * M) & (sel < (b + 1) * M)] - b * M).to(dev)
                    if m.numel() == 0:
                        continue
                ab, wb = _pick(S["a"], b)[m], _pick(wk, b)
                kwr = dict(act=act, geglu=geglu, ln_eps=ln_eps)
                bias_b = bk
                if geglu:
                    wb = unpack_geglu(wb, geglu_period)
                    bias_b = None if bk is None else unpack_geglu(bk, geglu_period)
                kwr["bias"] = bias_b
                if rowbias is not None:
                    kwr["rowbias"], kwr["rows_per_batch"] = S["rowbias"][m // rows_per_batch], 1
                if res is not None:
                    kwr["res"], kwr["gate"] = _pick(S["res"], b)[m], S.get("gate")
                if ln_row is not None:
                    st, c = S.get("ln_row.stats"), S["ln_row.c"]
                    if st is not None:
                        st = (st[b] if (batched and st.dim() == 3) else st.reshape(-1, 2))[m]
                    kwr["ln_row"] = (st, unpack_geglu(c, geglu_period) if geglu else c)
                if ln_col is not None:
                    kwr["ln_col"] = (_pick(S["ln_col.stats"], b), S["ln_col.c"].reshape(-1)[m], S["ln_col.d"].reshape(-1)[m])
                want, slack = K.gemm_ref(ab, wb, **kwr)
                if split16 and kwr["ln_row"][0] is not None:
                    slack = slack + RK.SPLIT16 * RK.mean_term(kwr["ln_row"][0], kwr["ln_row"][1]).to(slack.device)
                wants.append(want)
                slacks.append(slack)
                a_rows.append(ab)
                gots.append(_pick(L["out"], b)[m])
                if vt_out is not None:
                    got_vt.append(L["vt_out"][:, m].t())
                if out_stats is not None:
                    got_os.append(L["out_stats"].reshape(Bt, M, 2)[b][m])
                if ln_stats_out is not None:
                    got_ls.append(L["ln_stats_out"].reshape(Bt, M, 2)[b][m])
            want, slack, got = torch.cat(wants), torch.cat(slacks), torch.cat(gots)
            n = want.shape[0]
            n_out = L["out"].shape[-1]
            f32 = self._f32out(L["out"])
            parts = [self._part("out", *_outside(got, want[:, :n_out], slack[:, :n_out], dt, f32), n, total)]
            if vt_out is not None:
                parts.append(self._part("vt_out", *_outside(torch.cat(got_vt), want[:, n_out:], slack[:, n_out:], dt), n, total))
            if out_stats is not None:
                e_mu, e_rs = K.out_stats_excess(torch.cat(got_os), want.cpu(), slack.cpu(), dt, eps=out_stats_eps)
                parts.append(self._part("out_stats", int(not e_mu <= 1.0) + int(not e_rs <= 1.0), max(e_mu, e_rs), n, total))
            if ln_stats_out is not None:
                parts.append(self._stats_part("ln_stats_out", torch.cat(got_ls), torch.cat(a_rows), ln_eps, n, total))
            return parts
        return dict(tensors=T, writes=dict(out=out, out_stats=out_stats, ln_stats_out=ln_stats_out,
                                           vt_out=None if vt_out is None else vt_out[:, :M]),
                    judge=judge, flags=flags, pre=self._qkv_row_launches)

    def _stats_part(self, part, got, x_rows, eps, n, total):
        mu, rstd = SK.row_stats_ref(x_rows, eps)
        g = got.double().reshape(-1, 2).to(mu.device)
        e_mu = (g[:, 0] - mu).abs() / (F32_BAR * x_rows.double().abs().max().clamp_min(1e-30))
        e_rs = (g[:, 1] / rstd - 1).abs() / LN_STATS_TOL
        e = torch.cat([e_mu, e_rs])
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        return self._part(part, int((e > 1).sum()), float(e.max()), n, total)

    # ---- fused MLP ---------------------------------------------------------------------------------------------------------------
    def _plan_mlp_geglu(self, x, stats, w1, cd, w2p, b2, out, *, gate=None):
        from instancediffusion_amd.ops import HipOps
        T = dict(x=x, stats=stats, w1=w1, cd=cd, w2p=w2p, b2=b2, out=out, gate=gate)

        def judge(S, L, index, _):
            M, C = S["x"].shape
            sel = sample_rows(M, self.row_cap, index)
            m = torch.arange(M) if sel is None else sel
            cpu = lambda t: t.detach().cpu()
            cdm = cpu(S["cd"]).reshape(-1, 128)
            c1, d1 = unpack_geglu(cdm[:, :64].reshape(-1), 32), unpack_geglu(cdm[:, 64:].reshape(-1), 32)
            perm = torch.tensor(HipOps.MLP_W2_PERM)
            w2 = cpu(S["w2p"]).reshape(C, 4 * C // 16, 16).index_select(2, perm).reshape(C, 4 * C)
            g = None if gate is None else float(cpu(S["gate"]).reshape(-1)[0])
            md = m.to(S["x"].device)
            want, slack = RK.mlp_ref(cpu(S["x"][md]), cpu(S["stats"].reshape(-1, 2)[md]), unpack_geglu(cpu(S["w1"]), 32), c1, d1, w2,
                                     cpu(S["b2"]), g, self.judge_dt)
            return [self._part("out", *_outside(L["out"][md], want, slack, self.judge_dt), m.numel(), M)]
        return dict(tensors=T, writes=dict(out=out), judge=judge, flags="gate" if gate is not None else "")

    # ---- convs -------------------------------------------------------------------------------------------------------------------
    def _gn_part(self, part_live, out_live, total):
        e_mean, e_m2 = K.gn_partial_errors(part_live, out_live)
        bad = int(not e_mean < GN_PARTIAL_TOL[0]) + int(not e_m2 < GN_PARTIAL_TOL[1])
        return self._part("gn_partial", bad, max(e_mean / GN_PARTIAL_TOL[0], e_m2 / GN_PARTIAL_TOL[1]), total, total)

    def _conv_rows(self, B, Ho, Wo, index, dev):
        total = B * Ho * Wo
        sel = sample_rows(total, self.row_cap, index, batch_rows=Ho * Wo, border=conv_border_rows(B, Ho, Wo))
        return (torch.arange(total, device=dev) if sel is None else sel.to(dev)), total

    def _plan_conv(self, x, w, out, bias, rowbias, res, stride, up, pad_lo, n_valid, gn_partial):
        T = dict(x=x, w=w, out=out, bias=bias, rowbias=rowbias, res=res, gn_partial=gn_partial)
        flags = "+".join(k for k, v in dict(bias=bias, rowbias=rowbias, res=res, stride2=stride == 2 or None, up=up or None,
                                            pad_lo0=pad_lo == 0 or None, nchw=n_valid or None, gn_partial=gn_partial).items() if v is not None)

        def judge(S, L, index, _):
            B, H, W_, _ = S["x"].shape
            Ho, Wo = K.conv_out_hw(H, W_, stride, up, pad_lo)
            rows, total = self._conv_rows(B, Ho, Wo, index, S["x"].device)
            want, slack = conv_rows_ref(S["x"], S["w"], rows, bias=S.get("bias"), rowbias=S.get("rowbias"), res=S.get("res"), stride=stride,
                                        up=up, pad_lo=pad_lo)
            b, oy, ox = _pixel_index(rows, Ho, Wo)
            if n_valid:
                got, want, slack = L["out"][b, :, oy, ox], want[:, :n_valid], slack[:, :n_valid]
            else:
                got = L["out"][b, oy, ox]
            parts = [self._part("out", *_outside(got, want, slack, self.judge_dt, bool(n_valid) and self._f32out(L["out"])), rows.numel(), total)]
            if gn_partial is not None:
                parts.append(self._gn_part(L["gn_partial"], L["out"], total))
            return parts
        return dict(tensors=T, writes=dict(out=out, gn_partial=gn_partial), judge=judge, flags=flags)

    def _plan_conv3x3(self, x, w, out, *, bias=None, rowbias=None, res=None, stride=1, upsample=0, n_valid=0, gn_partial=None):
        return self._plan_conv(x, w, out, bias, rowbias, res, stride, upsample, 1, n_valid, gn_partial)

    def _plan_conv3x3_down(self, x, w, out, *, bias=None, res=None, gn_partial=None):
        return self._plan_conv(x, w, out, bias, None, res, 2, 0, 0, 0, gn_partial)

    def _plan_conv3x3_skip(self, g2, w_packed, x, out, *, bias=None, gn_partial=None):
        T = dict(g2=g2, w_packed=w_packed, x=x, out=out, bias=bias, gn_partial=gn_partial)

        def judge(S, L, index, _):
            B, H, W_, C2 = S["g2"].shape
            rows, total = self._conv_rows(B, H, W_, index, S["x"].device)
            wc, ws = S["w_packed"][:, :9 * C2], S["w_packed"][:, 9 * C2:]
            want, slack = conv_rows_ref(S["g2"], wc, rows, bias=S.get("bias"))
            b, oy, ox = _pixel_index(rows, H, W_)
            want2, slack2 = K.gemm_ref(S["x"][b, oy, ox], ws)
            parts = [self._part("out", *_outside(L["out"][b, oy, ox], want + want2, slack + slack2, self.judge_dt), rows.numel(), total)]
            if gn_partial is not None:
                parts.append(self._gn_part(L["gn_partial"], L["out"], total))
            return parts
        return dict(tensors=T, writes=dict(out=out, gn_partial=gn_partial), judge=judge,
                    flags="bias" + ("+gn_partial" if gn_partial is not None else ""))

    def _plan_conv_up2x(self, x, wf, out, *, bias=None):
        T = dict(x=x, wf=wf, out=out, bias=bias)

        def judge(S, L, index, _):
            B, H, W_, _ = S["x"].shape
            rows, total = self._conv_rows(B, 2 * H, 2 * W_, index, S["x"].device)
            want, slack = conv_up2x_rows_ref(S["x"], S["wf"], rows, S.get("bias"))
            b, oy, ox = _pixel_index(rows, 2 * H, 2 * W_)
            return [self._part("out", *_outside(L["out"][b, oy, ox], want, slack, self.judge_dt), rows.numel(), total)]
        return dict(tensors=T, writes=dict(out=out), judge=judge, flags="bias" if bias is not None else "")

    # ---- attention ---------------------------------------------------------------------------------------------------------------
    def _plan_attention(self, q, k0, vt0, n0, out, heads, *, k1=None, vt1=None, n1=0, qbits=None, kbits0=None, kbits1=None):
        T = dict(q=q, k0=k0, vt0=vt0, out=out, k1=k1, vt1=vt1, qbits=qbits, kbits0=kbits0, kbits1=kbits1)

        def judge(S, L, index, _):
            B, Nq, C = S["q"].shape
            per = max(1, self.row_cap // B)
            sel = sample_rows(Nq, per, index) if B * Nq > self.row_cap else None
            c = dict(H=heads, n0=n0, n1=n1, dt=self.judge_dt, q=S["q"], nq=Nq, d=C // heads, k0=S["k0"], vt0=S["vt0"], k1=S.get("k1"),
                     vt1=S.get("vt1"), qbits=S.get("qbits"), kbits0=S.get("kbits0"), kbits1=S.get("kbits1"))
            dev = S["q"].device
            want, bound = AC.attention_ref(c, qsel=sel, device=dev)
            got = L["out"] if sel is None else L["out"][:, sel.to(dev)]
            n = Nq if sel is None else sel.numel()
            return [self._part("out", *AC.outside(got, want, bound), B * n, B * Nq)]
        flags = "+".join(k for k, v in dict(seg1=n1 or None, mask=qbits).items() if v is not None)
        return dict(tensors=T, writes=dict(out=out), judge=judge, flags=f"n0={n0} n1={n1} {flags}")

    def _plan_qkv_attention(self, qkv, out, heads, T_, causal):
        B = out.shape[0] // T_

        def judge(S, L, index, _):
            c = dict(B=B, T=T_, H=heads, qkv=S["qkv"], causal=causal, dt=self.judge_dt)
            want, bound = AC.qkv_attention_ref(c, device=S["qkv"].device)
            return [self._part("out", *AC.outside(L["out"][:B * T_], want, bound), B * T_, B * T_)]
        return dict(tensors=dict(qkv=qkv, out=out), writes=dict(out=out[:B * T_]), judge=judge, flags=f"T={T_}")

    def _plan_attention_causal(self, qkv, out, heads, T):
        return self._plan_qkv_attention(qkv, out, heads, T, True)

    def _plan_attention_qkv(self, qkv, out, heads, T):
        return self._plan_qkv_attention(qkv, out, heads, T, False)

    def _plan_softmax_rows(self, s_f32, out, scale):
        def judge(S, L, index, _):
            n = S["s_f32"].shape[-1]
            want, bound = AC.softmax_rows_ref(S["s_f32"].reshape(-1, n), scale, self.judge_dt)
            rows = want.shape[0]
            return [self._part("out", *AC.outside(L["out"].reshape(-1, n), want, bound), rows, rows)]
        return dict(tensors=dict(s_f32=s_f32, out=out), writes=dict(out=out), judge=judge)

    # ---- the bandwidth kernels: judged whole, within one rounding ------------------------------------------------------------------
    def _rounding_part(self, got, want, rows):
        """``small_kernel_cases.within_one_rounding`` as (elements outside, largest error / bound)."""
        share = SK.within_one_rounding(got, want, self.judge_dt)
        w = want.detach().double().cpu()
        g = got.detach().double().cpu().reshape(w.shape)
        bound = SK.U[self.judge_dt] * w.abs() + 1e-5 * w.abs().max()
        ratio = ((g - w).abs() / bound.clamp_min(1e-300))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        return self._part("out", round(share * w.numel()), float(ratio.max()) if w.numel() else 0.0, rows, rows)

    def _f32_part(self, part, got, want, rows):
        w = want.detach().double().cpu()
        g = got.detach().double().cpu().reshape(w.shape)
        bar = F32_BAR * w.abs().max().clamp_min(1e-30)
        err = (g - w).abs()
        return self._part(part, int((~(err <= bar)).sum()), float(torch.nan_to_num(err / bar, nan=float("inf")).max()), rows, rows)

    def _exact_part(self, part, got, want, rows):
        bad = _bits(got.contiguous()) != _bits(want.to(got.device).contiguous())
        bad &= ~((got == 0) & (want.to(got.device) == 0))
        return self._part(part, int(bad.sum()), float("inf") if bool(bad.any()) else 0.0, rows, rows)

    def _plan_groupnorm(self, x, out, gamma, beta, eps, silu, partial=None):
        def judge(S, L, index, _):
            B, C = S["x"].shape[0], S["x"].shape[-1]
            x3 = S["x"].reshape(B, -1, C)
            stats = None if partial is None else gn_stats_from_partial(S["partial"], x3.shape[1], C)
            want = SK.groupnorm_ref(x3, S["gamma"], S["beta"], eps, silu, stats=stats)
            return [self._rounding_part(L["out"], want, B * x3.shape[1])]
        return dict(tensors=dict(x=x, out=out, gamma=gamma, beta=beta, partial=partial), writes=dict(out=out), judge=judge,
                    flags=("silu" if silu else "") + ("+partial" if partial is not None else ""))

    def _plan_layernorm(self, x, out, gamma, beta, eps=1e-5):
        def judge(S, L, index, _):
            return [self._rounding_part(L["out"], SK.layernorm_ref(S["x"], S["gamma"], S["beta"], eps), S["x"].shape[0])]
        return dict(tensors=dict(x=x, out=out, gamma=gamma, beta=beta), writes=dict(out=out), judge=judge)

    def _plan_row_stats(self, x, stats, eps=1e-5):
        def judge(S, L, index, _):
            return [self._stats_part("stats", L["stats"], S["x"], eps, S["x"].shape[0], S["x"].shape[0])]
        return dict(tensors=dict(x=x, stats=stats), writes=dict(stats=stats), judge=judge)

    def _plan_layernorm_patch2(self, x, out, gamma, beta, eps):
        C4 = 4 * x.shape[-1]

        def judge(S, L, index, _):
            want = layernorm_patch2_fast(S["x"], S["gamma"], S["beta"], eps)
            return [self._rounding_part(L["out"][:, :C4], want, want.shape[0])]
        return dict(tensors=dict(x=x, out=out, gamma=gamma, beta=beta), writes=dict(out=out[:, :C4]), judge=judge)

    def _plan_dwconv7x7(self, x, w_tap_major, bias, out):
        def judge(S, L, index, _):
            want = SK.dwconv7x7_ref(S["x"].cpu(), S["w"].cpu(), S["bias"].cpu())
            return [self._rounding_part(L["out"], want, want.numel() // want.shape[-1])]
        return dict(tensors=dict(x=x, w=w_tap_major, bias=bias, out=out), writes=dict(out=out), judge=judge)

    def _plan_seg_in_conv(self, segs, w, bias, out):
        def judge(S, L, index, _):
            want = seg_in_conv_fast(S["segs"].cpu(), S["w"].cpu(), S["bias"].cpu())
            return [self._rounding_part(L["out"][:, :48], want, want.shape[0])]
        return dict(tensors=dict(segs=segs, w=w, bias=bias, out=out), writes=dict(out=out[:, :48]), judge=judge)

    def _plan_scaleu_concat(self, h, skip, out, hscale, sm1):
        def judge(S, L, index, _):
            s = float(S["sm1"].reshape(-1)[0].double().cpu() + 1.0)
            want = SK.scaleu_ref(S["h"].cpu(), S["skip"].cpu(), S["hscale"].cpu(), s)
            return [self._rounding_part(L["out"], want, want.numel() // want.shape[-1])]
        return dict(tensors=dict(h=h, skip=skip, out=out, hscale=hscale, sm1=sm1), writes=dict(out=out), judge=judge)

    def _plan_timestep_embedding(self, t_f32, out):
        def judge(S, L, index, _):
            return [self._rounding_part(L["out"], SK.timestep_embedding_ref(S["t"].cpu(), L["out"].shape[1]), L["out"].shape[0])]
        return dict(tensors=dict(t=t_f32, out=out), writes=dict(out=out), judge=judge)

    def _plan_unifusion_embed(self, text, loc, tmask, lmask, null_text, null_loc, freqs, out):
        names = ("text", "loc", "tmask", "lmask", "null_text", "null_loc", "freqs")

        def judge(S, L, index, _):
            want = SK.unifusion_embed_ref(*(S[n].cpu() for n in names))
            return [self._rounding_part(L["out"], want, want.shape[0])]
        return dict(tensors=dict(zip(names, (text, loc, tmask, lmask, null_text, null_loc, freqs)), out=out), writes=dict(out=out), judge=judge)

    def _plan_conv_in(self, x_nchw, w, bias, out):
        def judge(S, L, index, _):
            want = SK.conv_in_ref(S["x"].cpu(), S["w"].cpu(), S["bias"].cpu())
            return [self._rounding_part(L["out"], want, want.numel() // want.shape[-1])]
        return dict(tensors=dict(x=x_nchw, w=w, bias=bias, out=out), writes=dict(out=out), judge=judge)

    # ---- bit for bit: one rounding of an exactly representable value ------------------------------------------------------------------
    def _plan_cast16(self, x_f32, out):
        def judge(S, L, index, _):
            return [self._exact_part("out", L["out"], S["x"].to(L["out"].dtype).reshape(L["out"].shape), L["out"].numel())]
        return dict(tensors=dict(x=x_f32, out=out), writes=dict(out=out), judge=judge)

    def _plan_clip_embed(self, ids_i32, tok_emb, pos_emb, out):
        B, T_ = ids_i32.shape

        def judge(S, L, index, _):
            ids = S["ids"].long().clamp(0, S["tok"].shape[0] - 1)
            want = (S["tok"].float()[ids] + S["pos"].float()[:T_][None]).to(L["out"].dtype).reshape(B * T_, -1)
            return [self._exact_part("out", L["out"][:B * T_], want, B * T_)]
        return dict(tensors=dict(ids=ids_i32, tok=tok_emb, pos=pos_emb, out=out), writes=dict(out=out[:B * T_]), judge=judge)

    def _plan_clip_patchify(self, pixels, patch, cls_row, x, patch_size):
        from tests.clip_vision_cases import patchify_ref
        B, _, S_, _ = pixels.shape
        G, k = S_ // patch_size, 3 * patch_size * patch_size
        cls_view = x.view(-1, x.shape[-1])[0:B * (G * G + 1):G * G + 1]

        def judge(S, L, index, _):
            want = torch.zeros((B * G * G, L["patch"].shape[1]), dtype=L["patch"].dtype, device=L["patch"].device)
            want[:, :k] = patchify_ref(S["pixels"], patch_size).to(want.dtype)
            got_cls = L["x"].view(-1, L["x"].shape[-1])[0:B * (G * G + 1):G * G + 1]
            return [self._exact_part("patch", L["patch"][:B * G * G], want, B * G * G),
                    self._exact_part("cls", got_cls, S["cls_row"].reshape(1, -1).expand(B, -1), B)]
        return dict(tensors=dict(pixels=pixels, patch=patch, cls_row=cls_row, x=x), writes=dict(patch=patch[:B * G * G], x=cls_view), judge=judge)

    # ---- fp32 ops: the project's fp32 bar ----------------------------------------------------------------------------------------
    def _plan_pointwise_nchw(self, x, w, bias, out, in_scale=1.0):
        def judge(S, L, index, _):
            xs = S["x"].double().cpu().flatten(2) * float(torch.tensor(in_scale, dtype=torch.float32))
            want = torch.einsum("oc,bcp->bop", S["w"].double().cpu(), xs)
            if bias is not None:
                want = want + S["bias"].double().cpu().view(1, -1, 1)
            return [self._f32_part("out", L["out"], want.reshape(L["out"].shape), want.shape[0] * want.shape[2])]
        return dict(tensors=dict(x=x, w=w, bias=bias, out=out), writes=dict(out=out), judge=judge)

    def _plan_vae_posterior(self, h, w, bias, noise, scale, z, moments=None):
        def judge(S, L, index, _):
            m = torch.einsum("oc,bchw->bohw", S["w"].double().cpu(), S["h"].double().cpu())
            if bias is not None:
                m = m + S["bias"].double().cpu().view(1, -1, 1, 1)
            E = m.shape[1] // 2
            mean, logvar = m[:, :E], m[:, E:].clamp(-30.0, 20.0)
            want = (mean + (torch.exp(0.5 * logvar) * S["noise"].double().cpu() if noise is not None else 0)) * scale
            rows = want.shape[0] * want.shape[2] * want.shape[3]
            parts = [self._f32_part("z", L["z"], want, rows)]
            if moments is not None:
                parts.append(self._f32_part("moments", L["moments"], torch.cat([mean, logvar], 1), rows))
            return parts
        return dict(tensors=dict(h=h, w=w, bias=bias, noise=noise, z=z, moments=moments), writes=dict(z=z, moments=moments), judge=judge,
                    flags="+".join(k for k, v in dict(bias=bias, noise=noise, moments=moments).items() if v is not None))
