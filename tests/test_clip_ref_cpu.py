"""tests/clip_ref.py pinned on the CPU — the float32 emulations of the two documented summation orders of the
gradient-clipping kernels stay within the derived bound of float64 on the very inputs tests/test_clip_gpu.py uses,
and differ bit for bit from a plain ascending float32 sum there (so a kernel summing in another order cannot pass
the GPU tests) — plus what needs no GPU of the feature itself: optim.ClipNorm's validation, the trainers' refusal of
a clip= that is no ClipNorm, and the argument validation of the three new entry points (no launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import clip_ref as C
import head_ref64 as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the emulations
def test_wave_and_block_sum_shapes_and_exact_values():
    """Integers: any order is exact, so the tree and the wave chain must give the plain sum."""
    rng = np.random.default_rng(0)
    v = rng.integers(0, 1000, 1024).astype(F32)
    assert C.wave_sum(v[:64]) == v[:64].sum(dtype=np.float64)
    assert C.block_sum(v) == v.sum(dtype=np.float64)
    assert C.block_sum(v.reshape(1, 1024)).shape == (1,)


@pytest.mark.parametrize("i", range(len(C.SLAB_COUNTS)))
def test_partials_layout_per_form(i):
    """1300 columns: 2 blocks of 1024, 6 of 256, 21 of 64; the partials cover every column exactly once (their float64
    sum is the float64 sum of squares to float32 accuracy) and the last block is the partial one."""
    nslab = C.SLAB_COUNTS[i]
    _, g = C.case(i)
    p = C.block_partials(g, nslab)
    assert p.shape == (C.nblk(C.N, nslab),) and p.size == {1: 2, 17: 6, 65: 21}[nslab]
    want = float((g.astype(np.float64) ** 2).sum())
    assert abs(float(p.astype(np.float64).sum()) - want) <= C.gamma(23) * want
    cols = C.cols_per_block(nslab)
    tail = g[(p.size - 1) * cols:]
    assert 0 < tail.size < cols
    assert abs(float(p[-1]) - float((tail.astype(np.float64) ** 2).sum())) <= C.gamma(23) * float(p[-1])


def test_bound_is_the_documented_figure():
    assert C.chain_length(21) == 44 and C.chain_length(1024) == 44 and C.chain_length(1025) == 45
    assert C.chain_length(6000) == 49           # K5 client at B = 4096: a few thousand partials
    assert math.isclose(C.norm_bound(21), 1.37e-6, rel_tol=0.01)
    assert C.norm_bound(21, ref_terms=2600) > C.norm_bound(21)


@pytest.mark.parametrize("g", range(len(C.GROUPS)))
def test_emulation_within_the_derived_bound_of_float64(g):
    ids = C.GROUPS[g]
    parts, norm, coef = C.group_case(g)
    assert parts.size == sum(C.nblk(C.N, C.SLAB_COUNTS[i]) for i in ids) and coef == 1.0
    want = C.norm64([C.case(i)[1] for i in ids])
    assert np.isfinite(norm) and want > 1e3
    assert abs(float(norm) - want) <= C.norm_bound(parts.size, ref_terms=C.N * len(ids)) * want


@pytest.mark.parametrize("g", range(len(C.GROUPS)))
def test_emulation_differs_from_a_plain_ascending_sum(g):
    ids = C.GROUPS[g]
    parts, _, _ = C.group_case(g)
    total = C.group_total(parts)
    plain = C.plain_ascending_sumsq([C.case(i)[1] for i in ids])
    assert total.dtype == F32 and plain.dtype == F32
    assert C.ulps(total, plain) >= 1, "the documented order and a plain ascending sum agree: the inputs pin nothing"
    # ... and so do the partials of a form's blocks against an ascending sum of the block's squares
    for i in ids:
        _, gr = C.case(i)
        cols = C.cols_per_block(C.SLAB_COUNTS[i])
        asc = np.array([C.plain_ascending_sumsq([gr[b:b + cols]]) for b in range(0, C.N, cols)], dtype=F32)
        assert R.differ_share(C.block_partials(gr, C.SLAB_COUNTS[i]), asc) >= 0.5


def test_coef_edges_of_the_emulation():
    assert C.norm_coef(F32(0.0), 1.0) == (0.0, 1.0)
    norm, coef = C.norm_coef(F32(np.inf), 1.0)
    assert np.isinf(norm) and coef == 0.0
    norm, coef = C.norm_coef(F32(np.nan), 1.0)
    assert np.isnan(norm) and np.isnan(coef)
    assert C.norm_coef(F32(4.0), np.inf)[1] == 1.0
    assert C.norm_coef(F32(16.0), 1.0)[1] == F32(F32(1.0) / F32(F32(4.0) + F32(1e-6)))
    assert C.coef64(4.0, 1.0) == 1.0 / (4.0 + 1e-6) and C.coef64(0.5, 1.0) == 1.0


# ------------------------------------------------------------------------------------------------ ClipNorm
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), -float("inf"), None, "1.0", True])
def test_clipnorm_rejects(bad):
    from splitcnn import optim
    with pytest.raises(ValueError, match="max_norm"):
        optim.ClipNorm(bad, device="cpu")


def test_clipnorm_holds_a_device_scalar_and_updates_in_place():
    from splitcnn import optim
    c = optim.ClipNorm(2.5, device="cpu")
    assert c.value.dtype == torch.float32 and c.value.shape == (1,) and c.value.item() == 2.5 and c.max_norm == 2.5
    ptr = c.value.data_ptr()
    c.set_max_norm(0.75)
    assert c.value.data_ptr() == ptr and c.value.item() == 0.75 and c.max_norm == 0.75
    c.set_max_norm(float("inf"))
    assert math.isinf(c.value.item())
    for bad in (0.0, float("nan"), -3.0):
        with pytest.raises(ValueError, match="max_norm"):
            c.set_max_norm(bad)
    assert math.isinf(c.value.item()), "a refused value must not reach the device"
    assert c.to("cpu") is c and c.value.data_ptr() == ptr
    assert optim.ClipNorm(float("inf"), device="cpu").max_norm == float("inf")
    assert optim.ClipNorm(np.float32(3.0), device="cpu").max_norm == 3.0 and "3.0" in repr(optim.ClipNorm(3, "cpu"))


@pytest.mark.parametrize("bad", [1.0, "1.0", {"max_norm": 1.0}])
def test_trainers_reject_a_clip_that_is_no_clipnorm(bad):
    """Before anything touches a device: the check runs on a machine without a GPU."""
    from splitcnn.engine import SplitTrainer
    from splitcnn.wide import WideTrainer
    for T in (SplitTrainer, WideTrainer):
        with pytest.raises(TypeError, match="ClipNorm"):
            T(clip=bad)


def test_dist_refusal_mentions_clip():
    from splitcnn import dist

    class Stage:
        optim = schedule = None
        clip = object()
    with pytest.raises(ValueError, match="only the default optimizer.*clip="):
        dist._default_optimizer_only("Hub", Stage())


# ------------------------------------------------------------------------------------------------ C ABI validation
P, I = ctypes.c_void_p, ctypes.c_int


def _arr(ctype, vals):
    return ctypes.cast((ctype * 8)(*vals), P)


def _fake(k, base=0x1000):
    """k non-null values standing in for device pointers: validation must fail before anything reads them."""
    return _arr(P, [base * (i + 1) for i in range(k)])


def _calls(lib, nseg, group, ngroup, partials, nslab=None):
    """The three entries on `nseg` fake segments; returns their statuses."""
    nslab = _arr(I, nslab or [1] * nseg)
    n = _arr(I, [C.N] * nseg)
    grp = _arr(I, group)
    f = lambda b: _fake(max(nseg, 1), b)  # noqa: E731
    mx = P(0x7000)
    return (
        lib.slk_reduce_sqnorm_multi(f(0x1000), f(0x2000), nslab, n, grp, nseg, partials, ngroup, None, 0, 0.0, None, 0,
                                    None, None),
        lib.slk_sgdm_clip_multi(f(0x1000), f(0x2000), f(0x3000), nslab, n, grp, nseg, partials, f(0x5000), ngroup, mx,
                                P(0x8000), 1, P(0x9000), 0.9, 0.0, 0.0, 0, None),
        lib.slk_adamw_clip_multi(f(0x1000), f(0x2000), f(0x3000), f(0x4000), nslab, n, grp, nseg, partials, f(0x5000),
                                 ngroup, mx, P(0x8000), 1, P(0x9000), 0.9, 0.999, 1e-8, 0.0, 1, None),
    )


def test_argument_validation_without_gpu():
    """Null partials, more than SGD_MAXSEG (4) segments and bad group ids: hipErrorInvalidValue (1) from all three
    entries, before any launch (this machine has no GPU: a launch would return another error)."""
    from splitcnn import _lib
    lib = _lib.load()
    bad = (1, 1, 1)
    assert _calls(lib, 1, [0], 1, None) == bad                       # no partials array
    assert _calls(lib, 1, [0], 1, _arr(P, [None])) == bad            # the group's partials pointer is null
    assert _calls(lib, 5, [0] * 5, 1, _fake(1, 0x6000)) == bad       # more than 4 segments
    assert _calls(lib, 0, [], 1, _fake(1, 0x6000)) == bad            # no segment
    for group, ngroup in (([1], 1), ([0, 2], 3), ([1, 0], 2), ([0, -1], 2), ([0, 1], 1), ([0, 0], 2), ([0, 1], 5)):
        assert _calls(lib, len(group), group, ngroup, _fake(4, 0x6000)) == bad, (group, ngroup)
    assert _calls(lib, 1, [0], 1, _fake(1, 0x6000), nslab=[0]) == bad   # a segment needs at least one slab
    # in place (grad == slabs) is for ONE slab only
    same = _fake(1, 0x1000)
    assert lib.slk_reduce_sqnorm_multi(same, same, _arr(I, [2]), _arr(I, [C.N]), _arr(I, [0]), 1, _fake(1, 0x6000), 1,
                                       None, 0, 0.0, None, 0, None, None) == 1
    # a missing threshold
    assert lib.slk_sgdm_clip_multi(_fake(1), _fake(1, 0x2000), _fake(1, 0x3000), _arr(I, [1]), _arr(I, [C.N]),
                                   _arr(I, [0]), 1, _fake(1, 0x6000), _fake(1, 0x5000), 1, None, P(0x8000), 1, P(0x9000),
                                   0.0, 0.0, 0.0, 0, None) == 1
    # empty segments are valid and launch nothing
    assert lib.slk_reduce_sqnorm_multi(_fake(1), _fake(1, 0x2000), _arr(I, [1]), _arr(I, [0]), _arr(I, [0]), 1,
                                       _fake(1, 0x6000), 1, None, 0, 0.0, None, 0, None, None) == 0
    assert lib.slk_reduce_sqnorm_nblk(1300, 1) == 2 and lib.slk_reduce_sqnorm_nblk(1300, 17) == 6
    assert lib.slk_reduce_sqnorm_nblk(1300, 65) == 21 and lib.slk_reduce_sqnorm_nblk(0, 5) == 0
    for n, k in ((1300, 1), (1300, 16), (1300, 17), (1300, 64), (1300, 65), (1024, 3), (1025, 3), (64, 200)):
        assert lib.slk_reduce_sqnorm_nblk(n, k) == C.nblk(n, k)
