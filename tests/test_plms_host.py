"""CPU only: the expressions of tests/plms_cases.py against the CPU oracle's ``_p_sample_plms`` (bit for bit over the five steps of
S = 5), the wrong variants the shared pools must tell apart from the right expressions (with the count of elements each changes),
and ``EmulOps``'s three PLMS ops.  tests/test_plms_kernels_gpu.py holds the HIP kernels to the same expressions on the same pools."""
import numpy as np
import pytest
import torch

from tests import plms_cases as pc


# ---- oracle agreement ------------------------------------------------------------------------------------------------
def test_tensor_sqrt_equals_the_correctly_rounded_root_at_every_index_of_the_schedule():
    """The oracle takes the scalar roots with ``Tensor.sqrt``, the expressions (and the launcher) with the correctly rounded fp32 root.
    At the five indices of S = 5 the two agree -- an assertion on every index, not a filter.  (At S = 50 they do not: indices 6, 7,
    44 and 45 are one ulp apart, which is why the chain runs at S = 5.)"""
    from oracle import ref_cpu
    _, a, a_prev = ref_cpu._schedule(pc.S)
    assert a.dtype == np.float32 and a_prev.dtype == np.float32 and len(a) == pc.S
    for index in range(pc.S):
        a_t, a_p = torch.tensor(a[index]), torch.tensor(a_prev[index])
        want = pc._roots(a[index], a_prev[index])
        got = (float(a_t.sqrt()), float(a_p.sqrt()), float((1.0 - a_p).sqrt()))
        assert got == tuple(float(v) for v in want), index
        assert float(torch.sqrt(1.0 - a_t)) == pc.scalars(index)[2], index
        assert pc.scalars(index)[:2] == (float(a[index]), float(a_prev[index]))


def test_torch_divides_by_the_history_weights_as_ieee_does():
    """(...) / 12 and / 24 on the CPU are correctly rounded divisions, not products with a rounded reciprocal: the kernels divide."""
    v = torch.cat([pc.pool(n)["x"] for n in pc.NS])
    for d in (2, 12, 24):
        assert torch.equal(v / d, torch.from_numpy(v.numpy() / np.float32(d))), d
    assert not torch.equal(v / 12, v * torch.tensor(1.0 / 12.0, dtype=torch.float32))


class _TableModel:
    """A model for ``ref_cpu._p_sample_plms``: returns prepared eps tensors in call order (cond, then uncond, per evaluation)."""

    def __init__(self, table, shape):
        self.it = iter([e.view(shape) for pair in table for e in pair])
        self.calls = 0

    def __call__(self, inp):
        self.calls += 1
        return next(self.it)


def test_the_chain_of_expressions_equals_the_oracle_over_the_five_steps():
    """Modes 0 and 1 in the first step, then 2, 3, 4 and 4 again, with the history rotation of plms.py:109-111."""
    from oracle import ref_cpu
    x, table = pc.chain_table()
    shape = (1, 1, 1, pc.CHAIN_N)
    want = pc.chain_want()
    _, a, a_prev = ref_cpu._schedule(pc.S)
    model = _TableModel(table, shape)
    inp = dict(x=x.view(shape).clone(), context=None)
    uc = torch.zeros(1)
    old: list = []
    t = torch.zeros(1, dtype=torch.long)
    for i in range(pc.S):
        img, e_t = ref_cpu._p_sample_plms(model, inp, t, pc.S - i - 1, a, a_prev, uc, pc.GUIDANCE, old, t)
        inp["x"] = img
        old.append(e_t)
        if len(old) >= 4:
            old.pop(0)
        assert torch.equal(img.view(-1), want[i]), i
    assert model.calls == 2 * pc.CHAIN_CALLS
    assert all(torch.isfinite(w).all() for w in want)


def test_expected_values_are_finite():
    """No NaN or inf among the expected values: ``torch.equal`` on them is a comparison of every element."""
    for n in pc.NS:
        assert all(torch.isfinite(pc.want_cfg(n, g)).all() for g in (7.5, 1.0, 0.0))
        assert all(torch.isfinite(pc.want_plms(n, m, i)).all() for m in pc.MODES for i in pc.STEP_INDICES)
        p = pc.pool(n)
        assert all((p[k] == 0).sum() == 2 and float(p[k].abs().max()) == float(np.float32(1e18)) for k in pc.POOL_NAMES)


# ---- mutation checks -------------------------------------------------------------------------------------------------
def _changed(a, b):
    return int((a != b).sum())


PLMS_MUTANTS = [   # (name, wrong expression, the modes in which it can differ)
    ("contracted_plms", pc.contracted_plms, pc.MODES),
    ("history slots swapped", pc.plms_swapped_history, [3, 4]),
    ("mode off by one", pc.plms_mode_off_by_one, pc.MODES),
    ("sqrt(1 - a_t) for sqrt(1 - a_prev)", pc.plms_dir_from_a_t, pc.MODES),
]


def test_contracted_cfg_changes_every_pool():
    for n in pc.NS:
        p = pc.pool(n)
        k = _changed(pc.contracted_cfg(p["ec"], p["eu"], pc.GUIDANCE), pc.want_cfg(n, pc.GUIDANCE))
        print(f"[mutants] contracted_cfg n = {n}: {k} of {n} elements change")
        assert k > 0, n


@pytest.mark.parametrize("name,wrong,modes", PLMS_MUTANTS, ids=[m[0].split()[0] for m in PLMS_MUTANTS])
def test_plms_mutants_change_every_pool(name, wrong, modes):
    """At every n, every mode the mutant touches and every scalar triple."""
    for n in pc.NS:
        p = pc.pool(n)
        counts = {}
        for mode in modes:
            for index in pc.STEP_INDICES:
                got = wrong(p["x"], p["ec"], pc.history(p), p["en"], mode, *pc.scalars(index))
                counts[(mode, index)] = _changed(got, pc.want_plms(n, mode, index))
        print(f"[mutants] {name} n = {n}: per mode {[sum(counts[(m, i)] for i in pc.STEP_INDICES) for m in modes]} of {3 * n} change "
              f"(least in one case: {min(counts.values())})")
        assert min(counts.values()) > 0, (n, counts)


def test_contracted_chain_ends_elsewhere():
    x, table = pc.chain_table()
    got = pc.chain(pc.contracted_cfg, pc.contracted_plms, x, table)
    k = [_changed(g, w) for g, w in zip(got, pc.chain_want())]
    print(f"[mutants] contracted chain: {k} of {pc.CHAIN_N} elements differ after steps 1..5")
    assert min(k) > 0


MERGE_MUTANTS = [  # (name, wrong expression, mode, least n_inst at which it can differ, needs H != W)
    ("H and W swapped in the pixel decomposition", pc.merge_hw_swapped, 1, 1, True),
    ("boxes applied as [1]:[3] on dim 2", pc.merge_box_axes_swapped, 1, 1, False),
    ("the earlier instance wins", pc.merge_earlier_wins, 1, 3, False),
    ("divisor n_inst", pc.merge_divisor_n_inst, 0, 1, False),
]


@pytest.mark.parametrize("name,wrong,mode,least,rect", MERGE_MUTANTS, ids=["hw", "axes", "order", "divisor"])
def test_merge_mutants_change_every_case(name, wrong, mode, least, rect):
    """At every shape and instance count at which the mutant is another function at all (H == W hides a swapped decomposition, one
    instance has no order)."""
    seen = 0
    for shape in pc.MERGE_SHAPES:
        if rect and shape[2] == shape[3]:
            continue
        for n_inst in pc.MERGE_N_INST:
            if n_inst < least:
                continue
            lat, boxes = pc.merge_lat(n_inst, shape), pc.merge_boxes_for(n_inst, *shape[2:])
            k = _changed(wrong(lat, boxes, mode), pc.mis_merge_expr(lat, boxes, mode))
            print(f"[mutants] {name} {shape} n_inst = {n_inst}: {k} of {lat[0].numel()} elements change")
            assert k > 0, (shape, n_inst)
            seen += 1
    assert seen >= 4


def test_merge_boxes_hold_the_edge_cases():
    for _, _, H, W in pc.MERGE_SHAPES:
        b = pc.merge_boxes(H, W).tolist()
        assert int(pc.merge_boxes(H, W).min()) >= 0
        assert b[2][0] == b[2][2] and b[3][0] > b[3][2]                                   # empty, inverted
        assert (b[4][2] - b[4][0], b[4][3] - b[4][1]) == (1, 1)                           # one pixel
        assert b[5][2] > H and b[5][3] > W and b[6][2:] == [H, W] and b[7] == [0, 0, H, W]
        assert max(b[0][0], b[1][0]) < min(b[0][2], b[1][2]) and max(b[0][1], b[1][1]) < min(b[0][3], b[1][3])   # 0 and 1 overlap
        assert sorted(pc.merge_boxes_for(8, H, W).tolist()) == sorted(b)


# ---- the emulated ops ------------------------------------------------------------------------------------------------
def test_emulated_ops_give_the_expressions():
    from tests.emul_ops import EmulOps
    ops = EmulOps(torch.float32)
    n = 257
    p = pc.pool(n)
    assert torch.equal(ops.cfg_combine(p["ec"], p["eu"], pc.GUIDANCE, torch.empty(n)), pc.want_cfg(n, pc.GUIDANCE))
    for mode in pc.MODES:
        for index in pc.STEP_INDICES:
            got = ops.plms_update(p["x"], p["ec"], pc.history(p), p["en"], mode, *pc.scalars(index), torch.empty(n))
            assert torch.equal(got, pc.want_plms(n, mode, index)), (mode, index)
    shape = pc.MERGE_SHAPES[0]
    lat, boxes = pc.merge_lat(3, shape), pc.merge_boxes_for(3, *shape[2:])
    for mode in (0, 1):
        assert torch.equal(ops.mis_merge(lat, boxes, torch.empty(shape), mode), pc.mis_merge_expr(lat, boxes, mode))


# ---- which GPU test catches which mutant -------------------------------------------------------------------------------
MUTANTS = {                                                 # wrong kernel -> the test of tests/test_plms_kernels_gpu.py that rejects it
    "contracted_cfg": "test_cfg_combine_is_bit_identical at guidance 7.5, every n; test_five_step_chain_through_hipops",
    "contracted_plms": "test_plms_update_is_bit_identical, every mode, n and scalar triple; test_five_step_chain_through_hipops",
    "history slots swapped": "test_plms_update_is_bit_identical, modes 3 and 4",
    "mode off by one": "test_plms_update_is_bit_identical, every mode; test_unread_operands_are_not_read (a NaN operand is read)",
    "sqrt(1 - a_t) for sqrt(1 - a_prev)": "test_plms_update_is_bit_identical, every mode and scalar triple",
    "H and W swapped in the pixel decomposition": "test_mis_merge_is_bit_identical mode 1 at (2, 3, 5, 7) and (1, 4, 24, 40)",
    "boxes applied as [1]:[3] on dim 2": "test_mis_merge_is_bit_identical mode 1, n_inst >= 1, every shape",
    "the earlier instance wins": "test_mis_merge_is_bit_identical mode 1, n_inst 3 and 8 (the overlapping boxes 0 and 1)",
    "divisor n_inst": "test_mis_merge_is_bit_identical mode 0, n_inst >= 1, and its fp64 bound",
}


def test_every_mutant_names_its_gpu_test():
    import os
    names = ["contracted_cfg"] + [m[0] for m in PLMS_MUTANTS] + [m[0] for m in MERGE_MUTANTS]
    assert sorted(names) == sorted(MUTANTS) and len(MUTANTS) == 9
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_plms_kernels_gpu.py")).read()
    for name, where in MUTANTS.items():
        tests = [w for w in where.replace(";", " ").replace(",", " ").split() if w.startswith("test_")]
        assert tests and all(f"def {t}(" in src for t in tests), name
