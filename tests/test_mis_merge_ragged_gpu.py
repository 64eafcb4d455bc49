"""``idf_mis_merge_ragged`` on a real MI355X, bit for bit (fp32 kernel, independent of the 16-bit element type): mode 0 against a
sequential fp32 torch loop (s = s + lat[k], then / count), mode 1 against the slicing loop, both against ``idf_mis_merge`` when
all counts are equal; guard elements behind ``out``, a spare NaN unit behind ``lat``; the scalar path (odd shape, base pointers
off by one float).  The argument checks and the wrapper's offset validation need no GPU and carry no ``gpu`` mark."""
import pytest
import torch

from tests.emul_ops_layouts import merge_ragged_expr

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def _boxes(U, H, W, seed):
    """Random boxes inside the frame, plus the three special ones: empty, full frame, and one overlapping its neighbour."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.stack([torch.randint(0, H, (U,), generator=g), torch.randint(0, W, (U,), generator=g)], 1)
    ext = torch.stack([torch.randint(0, H, (U,), generator=g), torch.randint(0, W, (U,), generator=g)], 1)
    hi = torch.minimum(lo + ext, torch.tensor([H, W]))
    b = torch.cat([lo, hi], 1).to(torch.int32)
    if U > 1:
        b[1] = torch.tensor([0, 0, H, W])                       # full frame
    if U > 2:
        b[2] = torch.tensor([H // 2, W // 2, H // 2, W])        # empty
    if U > 3:
        b[3] = torch.tensor([1, 1, H, W - 1])                   # overlaps the full-frame one before it
    return b


def _run(ops, counts, C, H, W, mode, seed, misalign=False):
    """One launch with guards: a NaN unit behind lat[U-1], NaN elements behind out, optionally both bases off by one float."""
    U, B = sum(counts), len(counts)
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(U, C, H, W, generator=g)
    boxes = _boxes(U, H, W, seed + 1) if mode == 1 else None
    chw, shift, guard = C * H * W, (1 if misalign else 0), 64
    lat_buf = torch.full((shift + (U + 1) * chw,), float("nan"), device="cuda")
    lat_d = lat_buf[shift:shift + U * chw].view(U, C, H, W)
    lat_d.copy_(lat)
    out_buf = torch.full((shift + B * chw + guard,), float("nan"), device="cuda")
    out_d = out_buf[shift:shift + B * chw].view(B, C, H, W)
    assert (lat_d.data_ptr() % 16 != 0) == misalign and (out_d.data_ptr() % 16 != 0) == misalign
    ops.mis_merge_ragged(lat_d, _offsets(counts), None if boxes is None else boxes.cuda(), out_d, mode)
    torch.cuda.synchronize()
    want = merge_ragged_expr(lat, _offsets(counts), boxes, mode)
    got = out_d.cpu()
    assert not torch.isnan(got).any(), "the spare NaN unit behind lat was read"
    assert torch.equal(got, want), (counts, (C, H, W), mode, float((got - want).abs().max()))
    assert torch.isnan(out_buf[shift + B * chw:]).all() and torch.isnan(out_buf[:shift]).all(), "wrote outside out"


MIXED33 = [1 + (7 * i) % 9 for i in range(33)]


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("counts,chw,misalign", [
    ([1], (4, 16, 16), False),
    ([1, 4, 2], (4, 16, 16), False),
    ([31], (4, 16, 16), False),
    (MIXED33, (4, 16, 16), False),
    ([1, 4, 2], (3, 5, 7), False),                  # C*H*W = 105: scalar accesses
    ([1, 4, 2], (4, 16, 16), True),                 # base pointers off by one float: scalar accesses
    ([2, 3], (4, 5, 7), False),                     # C*H*W % 4 == 0 with W % 4 != 0: vectors that cross latent rows
    ([1, 4, 2], (4, 64, 64), False),                # the product's latent size, more than one block per image
], ids=["b1u1", "c142", "c31", "b33", "odd", "misaligned", "rowcross", "64x64"])
def test_against_the_sequential_loops(ops, counts, chw, misalign, mode):
    _run(ops, counts, *chw, mode, seed=300 + len(counts), misalign=misalign)


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n1,B", [(1, 1), (4, 2), (9, 5)])
def test_equal_counts_equal_mis_merge(ops, n1, B, mode):
    g = torch.Generator().manual_seed(41 + n1)
    lat = torch.randn(n1, B, 4, 16, 16, generator=g).cuda()
    boxes = _boxes(max(n1 - 1, 1), 16, 16, 43)[:n1 - 1].reshape(-1, 4)
    want = ops.mis_merge(lat, boxes.cuda() if n1 > 1 else torch.zeros(1, 4, dtype=torch.int32, device="cuda"),
                         ops.empty((B, 4, 16, 16), torch.float32), mode)
    # the same units image after image; every image's unit j >= 1 carries instance j's box, its global unit's entry is ignored
    lat_r = lat.permute(1, 0, 2, 3, 4).reshape(n1 * B, 4, 16, 16).contiguous()
    boxes_r = torch.cat([torch.full((1, 4), 7, dtype=torch.int32), boxes], 0).repeat(B, 1).contiguous()
    got = ops.mis_merge_ragged(lat_r, _offsets([n1] * B), boxes_r.cuda(), ops.empty((B, 4, 16, 16), torch.float32), mode)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_argument_errors_return_before_any_launch():
    """Fake, never dereferenced pointers: every IDF_E_ARG case (no GPU needed)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    lat, off, box, out = 0x10000, 0x20000, 0x30000, 0x40000

    def call(lat=lat, off=off, box=box, out=out, B=2, U=5, C=4, H=16, W=16, mode=0):
        return lib.idf_mis_merge_ragged(lat, off, box, out, B, U, C, H, W, mode, None)
    assert call(lat=None) == -1 and call(off=None) == -1 and call(out=None) == -1
    assert call(B=0) == -1 and call(B=-3) == -1 and call(U=1) == -1
    assert call(C=0) == -1 and call(H=0) == -1 and call(W=-1) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(mode=1, box=None) == -1


def test_wrapper_rejects_bad_offset_lists():
    from instancediffusion_amd.ops import HipOps
    chk = HipOps.check_unit_offsets
    assert chk([0, 1, 5, 7], 3, 7) == [0, 1, 5, 7] and chk(torch.tensor([0, 2]), 1, 2) == [0, 2]
    for bad in ([1, 2, 7], [0, 2, 2, 7], [0, 5, 3, 7], [0, 1, 5, 6], [0, 1, 5, 8], [0, 7], [0, 1, 2, 3, 7], []):
        with pytest.raises(ValueError):
            chk(bad, 3, 7)
