"""Pins tests/layerwise_ref.py on the CPU: the float32 emulation of the layer-wise partials, totals and ratios stays
inside the derived bounds of the float64 closed form on the op tests' inputs, and three plausible but wrong recipes
leave those bounds there, so the GPU tests that use the reference can tell them apart."""
import numpy as np
import pytest

import clip_ref as C
import layerwise_ref as L

F32 = np.float32
EPS32 = np.finfo(np.float32).eps
LARS = dict(momentum=0.9, nesterov=True, weight_decay=5e-4, trust_coef=1e-3, eps=1e-8)
LAMB = dict(b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-6)), wd=float(F32(0.01)))


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("nw", L.NW_CASES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_lars_emulation_is_within_the_bounds_of_float64(i, nw):
    g, p, nslab = C.case(i)[1], L.params_case(i), C.SLAB_COUNTS[i]
    parts = L.partials(g, p, nslab, nw)
    assert parts.shape == (C.nblk(L.N, nslab), 4)
    tot = L.totals(parts)
    nb, rb = L.norm_bound(parts.shape[0], ref_terms=L.N), L.lars_ratio_bound(parts.shape[0], ref_terms=L.N)
    for (s, is_bias), (kx, kp) in zip(L.tensors(L.N, nw), ((0, 1), (2, 3))):
        wn, gn, r = L.lars_ratio32(tot[kx], tot[kp], 1e-3, 5e-4, 1e-8)
        wn64, gn64 = L.norm64(p[s]), L.norm64(g[s])
        assert rel(wn, wn64) <= nb and rel(gn, gn64) <= nb, (i, nw, is_bias)
        r64 = L.lars_ratio64(wn64, gn64, float(F32(1e-3)), float(F32(5e-4)), float(F32(1e-8)))
        assert rel(r, r64) <= rb, (i, nw, is_bias, float(r), r64)
    if nw == L.N:
        assert tot[2] == 0 and tot[3] == 0, "no bias: its partials are zeros"


def test_a_straddling_block_feeds_both_tensors_and_a_nan_stays_in_its_own():
    g, p = np.array(C.case(0)[1]), np.array(L.params_case(0))
    parts = L.partials(g, p, 1, 1100)
    assert (parts[1] > 0).all() and parts[0, 2] == 0 and parts[0, 3] == 0   # block 1 holds columns 1024 .. 1299
    g[10] = np.nan
    bad = L.partials(g, p, 1, 1100)
    assert np.isnan(bad[0, 0]) and np.array_equal(bad[:, 1:], parts[:, 1:]) and bad[1, 0] == parts[1, 0]
    assert L.lars_ratio32(np.nan, 1.0, 1e-3, 0, 1e-8)[2] == 1 and L.lars_ratio64(1.0, float("nan"), 1e-3, 0, 1e-8) == 1
    assert L.lars_ratio32(0.0, 1.0, 1e-3, 0, 1e-8)[2] == 1 and L.lamb_ratio32(1.0, 0.0)[2] == 1
    assert L.lamb_ratio64(0.0, 1.0) == 1.0 and L.lamb_ratio64(2.0, 4.0) == 0.5


@pytest.mark.parametrize("nw", L.NW_CASES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_lamb_emulation_is_within_the_bounds_of_float64(i, nw):
    """u formed in float32 (numpy, one rounding per operation: the worst case the bound covers) against float64."""
    g, p, m0, nslab = C.case(i)[1], L.params_case(i), L.state_case(i), C.SLAB_COUNTS[i]
    v0 = (np.asarray(m0) ** 2).astype(F32)
    b1, b2, eps, wd = (F32(LAMB[k]) for k in ("b1", "b2", "eps", "wd"))
    step = 2
    m1 = (m0 + (F32(1) - b1) * (g - m0)).astype(F32)
    v1 = ((v0 * b2).astype(F32) + ((g * g).astype(F32) * (F32(1) - b2)).astype(F32)).astype(F32)
    bc2s, rbc1 = F32(np.sqrt(1.0 - float(b2) ** (step + 1))), F32(1.0 / (1.0 - float(b1) ** (step + 1)))
    denom = ((np.sqrt(v1).astype(F32) / bc2s).astype(F32) + eps).astype(F32)
    u32 = (((m1 / denom).astype(F32) * rbc1).astype(F32) + (wd * p).astype(F32)).astype(F32)
    u64, e_u = L.lamb_u_error(g, m0, v0, p, step, LAMB["b1"], LAMB["b2"], LAMB["eps"], LAMB["wd"])
    assert (np.abs(u32 - u64) <= e_u).all(), np.max(np.abs(u32 - u64) / e_u)
    tot = L.totals(L.partials(u32, p, nslab, nw))
    npart = C.nblk(L.N, nslab)
    for (s, is_bias), (kx, kp) in zip(L.tensors(L.N, nw), ((0, 1), (2, 3))):
        wn, un, r = L.lamb_ratio32(tot[kx], tot[kp])
        ub = L.lamb_unorm_bound(npart, u64[s], e_u[s], ref_terms=L.N)
        assert ub < 1e-5
        assert rel(un, L.norm64(u64[s])) <= ub
        assert rel(r, L.lamb_ratio64(L.norm64(p[s]), L.norm64(u64[s]))) <= L.lamb_ratio_bound(npart, ub, ref_terms=L.N)


@pytest.mark.parametrize("variant", ["decayed_norm", "bias_in_weight", "ratio_after_momentum"])
def test_wrong_recipes_leave_the_bound(variant):
    """The ratio from the decayed gradient's norm, the bias summed into the weight's norms, and the ratio applied
    after the momentum: each differs from the recipe by more than the bounds allow, at the op tests' sizes."""
    i, nw, step = 1, 1100, 1
    g, p, buf = C.case(i)[1], L.params_case(i), L.state_case(i)
    kw = dict(exclude_bias=False, **LARS)
    p1, b1, rows = L.lars_step64(p, g, buf, step, 0.1, nw, **kw)
    p2, b2, wrong = L.lars_step64(p, g, buf, step, 0.1, nw, variant=variant, **kw)
    rb = L.lars_ratio_bound(C.nblk(L.N, C.SLAB_COUNTS[i]), ref_terms=L.N)
    p64 = np.asarray(p, dtype=np.float64)
    assert within(p1, p1, p64)
    if variant == "ratio_after_momentum":     # the same ratios in the wrong place: the update leaves `within`
        assert [r[2] for r in rows] == [r[2] for r in wrong]
        assert not within(p2, p1, p64) and not within(b2, b1, np.asarray(buf, dtype=np.float64))
    else:                                     # a wrong norm: the weight's ratio leaves its bound
        assert rel(wrong[0][2], rows[0][2]) > 3 * rb, (wrong[0], rows[0], rb)


def test_excluded_bias_and_zero_tensors_take_ratio_one():
    g, p, buf = C.case(0)[1], np.array(L.params_case(0)), L.state_case(0)
    _, _, rows = L.lars_step64(p, g, buf, 0, 0.1, 1100, exclude_bias=True, **LARS)
    assert rows[1][2] == 1.0 and rows[0][2] != 1.0 and rows[1][0] > 0
    p[:1100] = 0
    newp, _, rows = L.lars_step64(p, g, buf, 0, 0.1, 1100, exclude_bias=False, **LARS)
    assert rows[0] == (0.0, L.norm64(g[:1100]), 1.0) and rows[1][2] != 1.0
    sgd = -0.1 * (1 + 0.9) * np.asarray(g[:1100], dtype=np.float64)     # first step, Nesterov, p = 0: no decay term
    assert np.allclose(newp[:1100], sgd, rtol=1e-15, atol=0)
    q, _, _, rows = L.lamb_step64(p, g, np.zeros(L.N), np.zeros(L.N), 0, 1e-3, 1100)
    assert rows[0][0] == 0.0 and rows[0][2] == 1.0 and rows[1][2] == 1.0 and np.isfinite(q).all()


def test_zero_gradient_keeps_the_parameters_finite():
    p, z = L.params_case(2), np.zeros(L.N)
    newp, _, rows = L.lars_step64(p, z, z, 0, 0.1, 1100, **LARS)
    assert all(r[2] == 1.0 for r in rows) and np.isfinite(newp).all()
    newp, _, _, rows = L.lamb_step64(p, z, z, z, 0, 1e-3, 1100, weight_decay=0.0)
    assert all(r[2] == 1.0 for r in rows) and np.array_equal(newp, np.asarray(p, dtype=np.float64))
