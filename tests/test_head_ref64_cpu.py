"""CPU pins of tests/head_ref64.py: the float64 references equal the oracles' (oracle/split_step.py,
oracle/wide_step.py), the integer generators reach the boundaries they are meant to discriminate (shares printed and
asserted, floor 1 %), the three float32 reduction emulations differ from each other, from the earlier wording of
include/slk.h and from the rounded float64 sum in at least 25 % of the columns wherever they should, and the crafted
cross-entropy rows break a float32 cross-entropy that skips the max-subtraction while the float64 reference stays
finite."""
import numpy as np
import pytest
import torch

import head_ref64 as R
from oracle import split_step as S
from oracle import wide_step as WO

SLAB_COUNTS = [1, 7, 8, 9, 16, 17, 33, 64, 65, 200]


def _np(t):
    return t.double().cpu().numpy()


# ----------------------------------------------------------------------------- references == the oracles
def test_conv1_refs_equal_oracle():
    x, W1, b1 = R.conv1_real_case(3, 11)
    act = R.conv1_relu(x, W1, b1)
    want = S.client_forward(_np(x), _np(W1), _np(b1))
    np.testing.assert_allclose(_np(act), want, rtol=0, atol=1e-12)
    g = torch.randn(act.shape, generator=torch.Generator().manual_seed(5)).double()
    dW, db = S.client_backward(_np(x), want, _np(g))
    per = R.conv1_wgrad_per_sample(x, act, g)
    np.testing.assert_allclose(_np(per.sum(0)), np.concatenate([dW.reshape(-1), db]), rtol=0, atol=1e-10)
    slabs = R.conv1_wgrad_slabs(x, act, g)
    assert slabs.shape == (3, 320)
    np.testing.assert_allclose(_np(slabs.sum(0)), _np(per.sum(0)), rtol=0, atol=1e-10)


def test_fc_refs_equal_oracle():
    gen = torch.Generator().manual_seed(3)
    B = 70
    pooled = torch.randn((B, R.P_SAMPLE), generator=gen).double().clamp_min(0.0)
    W3 = (torch.randn((10, R.P_SAMPLE), generator=gen) * 0.01).double()
    b3 = torch.randn((10,), generator=gen).double()
    y = torch.randint(0, 10, (B,), generator=gen).numpy()
    logits = R.fc_fwd(pooled, W3, b3)
    np.testing.assert_allclose(_np(logits), _np(pooled) @ _np(W3).T + _np(b3), rtol=0, atol=1e-10)
    loss, loss_i, dl = S.cross_entropy(_np(logits), y)
    l64, d64, _ = R.xent64(_np(logits), y, grad_scale=1.0 / B)
    np.testing.assert_allclose(l64, loss_i, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d64, dl, rtol=0, atol=1e-15)
    dlt = torch.from_numpy(dl)
    np.testing.assert_allclose(_np(R.fc_dgrad(dlt, W3)), dl @ _np(W3), rtol=0, atol=1e-12)
    slabs = R.fc_wgrad_slabs(dlt, pooled)
    assert slabs.shape == (R.fc_wgrad_nslab(B), 92170) and R.fc_wgrad_per(B) == 35
    np.testing.assert_allclose(_np(slabs.sum(0)), np.concatenate([(dl.T @ _np(pooled)).reshape(-1), dl.sum(0)]),
                               rtol=0, atol=1e-10)


@pytest.mark.parametrize("B,per,nslab", [(1, 1, 1), (7, 7, 1), (8, 8, 1), (9, 9, 1), (64, 64, 1), (65, 33, 2),
                                          (130, 44, 3), (4096, 64, 64), (5000, 79, 64)])
def test_fc_wgrad_slice_formula(B, per, nslab):
    assert (R.fc_wgrad_per(B), R.fc_wgrad_nslab(B)) == (per, nslab)


def test_conv1_ranges():
    for B in (1, 5, 127, 128, 129, 300):
        r = R.conv1_ranges(B)
        assert len(r) == min(B, 128) and r[0][0] == 0 and r[-1][1] == B
        assert all(a[1] == b[0] for a, b in zip(r, r[1:])) and max(hi - lo for lo, hi in r) <= 3
    assert {hi - lo for lo, hi in R.conv1_ranges(129)} == {1, 2} and {hi - lo for lo, hi in R.conv1_ranges(300)} == {2, 3}


def test_head_ref_equals_wide_oracle():
    gen = torch.Generator().manual_seed(9)
    B = 5
    cut = torch.randn((B, R.CUT_F), generator=gen).double().clamp_min(0.0)
    Wf = (torch.randn((10, R.CUT_F), generator=gen) * 0.01).double()
    bf = torch.randn((10,), generator=gen).double()
    y = torch.randint(0, 10, (B,), generator=gen).numpy()
    keep = WO.dropout_keep(7, 3, B)
    s = WO.server_step({"fc.weight": _np(Wf), "fc.bias": _np(bf)}, _np(cut).reshape(B, 256, 8, 8), y, keep, bf=False)
    kt = torch.from_numpy(keep)
    logits = R.head_fwd(cut, Wf, bf, kt, 1.0 / 0.75)
    np.testing.assert_allclose(_np(logits), s["logits"], rtol=0, atol=1e-10)
    l64, d64, _ = R.xent64(s["logits"], y, grad_scale=1.0 / B)
    np.testing.assert_allclose(l64, s["loss_i"], rtol=0, atol=1e-12)
    dcut, slabs = R.head_bwd(cut, Wf, torch.from_numpy(s["dlogits"]), kt, 1.0 / 0.75)
    np.testing.assert_allclose(_np(dcut), s["dcut"].reshape(B, -1), rtol=0, atol=1e-12)
    want = np.concatenate([s["grads"]["fc.weight"].reshape(-1), s["grads"]["fc.bias"]])
    np.testing.assert_allclose(_np(slabs.sum(0)), want, rtol=0, atol=1e-10)


def test_c8_order_and_keep_bytes():
    flat = torch.arange(2 * R.CUT_F, dtype=torch.float64).reshape(2, R.CUT_F)
    c8 = R.c8_of_flat(flat)
    assert torch.equal(R.flat_of_c8(c8), flat)
    plane, pix, k = 5, 37, 6                                  # include/slk.h, slk_wide_fc_shadow's formula
    assert c8[1, (plane * 64 + pix) * 8 + k] == flat[1, (plane * 8 + k) * 64 + pix]
    keep = WO.dropout_keep(7, 3, 2, p=0.5)
    kb = R.keep_bytes(keep)
    assert kb.shape == (2, 2048) and kb.dtype == np.uint8
    assert ((kb[1, plane * 64 + pix] >> k) & 1) == int(keep[1, (plane * 8 + k) * 64 + pix])
    bits = np.unpackbits(kb[:, :, None], axis=2, bitorder="little").reshape(2, R.CUT_F)
    assert np.array_equal(_np(R.flat_of_c8(torch.from_numpy(bits.astype(np.float64)))) > 0, keep)


# ----------------------------------------------------------------------------- the generators discriminate
def test_conv1_integer_case_reaches_the_relu_boundary(capsys):
    x, W1, b1 = R.conv1_int_case(130, 1)      # 128 ranges, two of them with two samples
    pre = R.conv1_pre(x, W1, b1)
    assert float(R.conv1_abs_bound(x, W1, b1).max()) < 2 ** 24
    z = pre == 0
    share, last_pair, last_row = (float(v.double().mean()) for v in (z, z[:, :, 25, 24:], z[:, :, 25, :]))
    with capsys.disabled():
        print(f"\nconv1 integer case: pre-activation == 0 in {100 * share:.2f} % of the outputs, "
              f"{100 * last_pair:.2f} % of the last pixel pairs, {100 * last_row:.2f} % of the last rows")
    assert min(share, last_pair, last_row) >= 0.01
    # the boundary matters: a gradient placed exactly there is what `>=` would let through
    g = R.cut_grad_int(130, 2)
    a = R.conv1_wgrad_slabs(x, torch.where(pre > 0, pre, torch.zeros_like(pre)), g)
    for m in ("ge", "drop_last_pair", "shift_tap", "drop_last_sample"):
        assert not torch.equal(a, R.conv1_wgrad_slabs(x, R.conv1_relu(x, W1, b1), g, mutate=m)), m


def test_head_integer_case_drops_nonzero_values(capsys):
    cut, Wf, bf = R.head_int_case(17, 4)
    keep = R.keep_mask(7, 3, 17, 0.5)
    dropped_nonzero = float((_np(cut)[~keep] != 0).mean())
    kept = float(keep.mean())
    with capsys.disabled():
        print(f"\nK5 head integer case at p = 0.5: {100 * dropped_nonzero:.2f} % of the dropped features hold a nonzero "
              f"cut value; {100 * kept:.2f} % of the features are kept")
    assert dropped_nonzero >= 0.01 and 0.45 <= kept <= 0.55
    kt = torch.from_numpy(keep)
    assert float(R.head_fwd(cut.abs(), Wf.abs(), bf.abs(), kt, 2.0).max()) < 2 ** 24
    # masks that a wrong index would draw differ from the right one
    assert (R.keep_mask(7, 3, 8, 0.5, b0=262140) != R.keep_mask(7, 3, 8, 0.5, b0=0)).mean() > 0.25
    c8_mask = _np(R.c8_of_flat(torch.from_numpy(keep.astype(np.float64)))) > 0
    assert (c8_mask != keep).mean() > 0.25


def test_fc_integer_case_bounds():
    pooled, W3, b3 = R.fc_int_case(17, 5)
    assert float(R.fc_fwd(pooled, W3.abs(), b3.abs()).max()) < 2 ** 24
    ks = R.onehot_features(40)
    assert {0, 9215, 1151, 1152, 8064, 9215 - 1151, 63, 64}.issubset(set(ks)) and len(set(ks)) >= 20
    p = R.onehot_rows(33, R.P_SAMPLE, R.onehot_features(33))
    assert torch.equal(p.sum(1), torch.ones(33, dtype=torch.float64))


# ----------------------------------------------------------------------------- reduction emulations
def test_reduction_emulations_differ(capsys):
    n = 1300
    lines = []
    for nslab in SLAB_COUNTS:
        s = R.reduce_case(nslab, n, 100 + nslab)
        prior = R.reduce_case(1, n, 7)[0]
        asc, p4, p16 = R.reduce_ascending(s), R.reduce_partials(s, 4), R.reduce_partials(s, 16)
        f64 = s.astype(np.float64).sum(0).astype(np.float32)
        doc = R.reduce_emulated(s)
        d = dict(a4=R.differ_share(asc, p4), a16=R.differ_share(asc, p16), p416=R.differ_share(p4, p16),
                 f64=R.differ_share(doc, f64))
        form = R.reduce_form(nslab)
        if form > 1:
            d["prior"] = R.differ_share(R.reduce_partials(s, form, prior), R.reduce_partials_prior_last(s, form, prior))
        lines.append(f"nslab {nslab:3d} (form {form:2d}): " + "  ".join(f"{k} {100 * v:.0f} %" for k, v in d.items()))
        if nslab == 1:
            assert d["a4"] == d["a16"] == d["f64"] == 0.0
            continue
        assert d["a4"] >= 0.25 and d["f64"] >= 0.25, (nslab, d)
        if nslab <= 16:       # 16 partials of at most one slab each: the ascending chain itself
            assert d["a16"] == 0.0
        if nslab >= 33:
            assert d["a16"] >= 0.25 and d["p416"] >= 0.25, (nslab, d)
        if form > 1:
            assert d["prior"] >= 0.25, (nslab, d)
        # with a prior the ascending form adds it LAST (prior + g)
        assert np.array_equal(R.reduce_ascending(s, prior), prior + asc)
    with capsys.disabled():
        print("\nbitwise-different columns of the float32 reduction forms (n = 1300):\n  " + "\n  ".join(lines))


def test_exact_values_stay_exact():
    for n in (1, 63, 64, 255, 256, 257, 1000, 4099):
        v = R.exact_values(n, n)
        assert (v < 8).all() and (v * 1024 == np.round(v * 1024)).all() and v.sum() * 1024 < 2 ** 24
        assert np.float32(v.sum()) == v.sum()


# ----------------------------------------------------------------------------- crafted cross-entropy rows
def test_crafted_rows_break_a_naive_cross_entropy():
    names, z, y = R.xent_cases(finite_only=False)
    assert (z.astype(np.float32).astype(np.float64) == z).all()
    loss64, d64, p64 = R.xent64(z, y)
    finite_row = np.isfinite(z).all(axis=1)
    assert np.isfinite(loss64).all() and np.isfinite(d64).all() and (loss64 >= 0).all()
    assert np.abs(d64.sum(axis=1)).max() < 1e-12
    naive = xent = R.xent32_naive(np.where(np.isfinite(z), z, -1e38), y)
    caught = set()
    for i, nm in enumerate(names):
        row = nm.split("/")[0]
        wrong = not np.isfinite(naive[i]) or abs(float(naive[i]) - loss64[i]) > R.loss_bound(z[i:i + 1], loss64[i:i + 1])[0]
        if wrong:
            caught.add(row)
        if row in R.NAIVE_BREAKS:
            assert wrong, f"{nm}: a cross-entropy without the max-subtraction passes ({xent[i]} vs {loss64[i]})"
    assert caught >= set(R.NAIVE_BREAKS)
    # labels at the maximum, at the minimum and in between, in every row with distinct logits
    for r in ("down_from_100", "1e4_unit_gaps", "one_200_above"):
        ys = [int(y[i]) for i, nm in enumerate(names) if nm.startswith(r + "/")]
        zs = next(z[i] for i, nm in enumerate(names) if nm.startswith(r + "/"))
        assert zs[ys[0]] == zs.max() and zs[ys[1]] == zs.min() and zs.min() < zs[ys[2]] < zs.max()
    assert finite_row.sum() == 27 and len(names) == 33
    # a wrong z[y] (the neighbouring class) misses the loss bound on every row with distinct logits
    for i, nm in enumerate(names):
        if nm.split("/")[0] in ("down_from_100", "down_from_-100", "1e4_unit_gaps", "-1e4_unit_gaps"):
            other = R.xent64(z[i:i + 1], [(y[i] + 1) % 10])[0][0]
            assert abs(other - loss64[i]) > R.loss_bound(z[i:i + 1], loss64[i:i + 1])[0]


def test_gradsum_bound_is_the_row_sum_of_grad_bound():
    """gradsum_bound = sum_j of grad_bound's relative term (sum_j p_j = 1) + ten roundings: never below the issue's
    10 * 2^-23 and never above the per-element bounds added up."""
    names, z, y = R.xent_cases()
    _, _, p64 = R.xent64(z, y)
    gs, gb = R.gradsum_bound(z), R.grad_bound(z, p64)
    assert (gs >= 10 * 2.0 ** -23).all() and (gs <= gb.sum(axis=1) + 10 * 2.0 ** -23).all()
    i = names.index("zeros/max")
    assert gs[i] < 2e-6
    # a float32 emulation of the kernels' expression needs the first term: lse rounds at ulp(1e4) = 2^-10
    f = np.float32
    j = names.index("1e4_unit_gaps/max")
    zz = z[j].astype(f)
    m = zz.max()
    lse = f(m + np.log(np.exp(zz - m, dtype=f).sum(dtype=f), dtype=f))
    s = float(np.exp(zz - lse, dtype=f).astype(np.float64).sum() - 1.0)
    assert 10 * 2.0 ** -23 < abs(s) <= gs[j]
