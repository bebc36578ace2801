"""The cut-noise rule without a GPU: the tables of splitcnn.privacy against their closed forms, the law of the draws
(tests/cut_noise_ref.py's numpy restatement and privacy.noise_draws, which must agree), the slicing property, and
that the wrong variants a kernel could compute are visible on the device tests' rows."""
import math
import statistics

import numpy as np
import pytest

import cut_noise_ref as R

LAW_KEYS = [(0, 0), (5, 1), (0xDEADBEEF, 0x80000003)]   # (seed, t)
LAW_ROWS = 64


def tables(kind):
    from splitcnn import privacy
    if kind == "hand":
        return R.hand_table()
    t64, tail = privacy.noise_tables(kind)
    return t64.astype(np.float32), float(np.float32(tail))


def test_tables_are_the_nearest_float32_to_their_closed_forms():
    from splitcnn import privacy
    lap, tail = privacy.noise_tables("laplace")
    assert lap.dtype == np.float64 and lap.shape == (1024,) and tail == math.log(2.0)
    want = np.array([-math.log1p(-(k + 0.5) / 2048.0) for k in range(1024)])
    assert np.array_equal(lap.astype(np.float32), want.astype(np.float32))
    assert 0 < lap[0] and lap[-1] < math.log(2.0) and (np.diff(lap) > 0).all()
    gau, gtail = privacy.noise_tables("gaussian")
    assert gau.dtype == np.float64 and gau.shape == (1024,) and gtail == 0.0
    nd = statistics.NormalDist()
    indep = np.array([nd.inv_cdf(0.5 + (k + 0.5) / 2048.0) for k in range(1024)])   # half-normal quantile
    assert np.abs(gau - indep).max() <= 1e-12 * indep.max()
    # the nearest float32: the bisection's own value rounds, and the independent one rounds to the same or to a
    # neighbour only where it sits within its 1e-12 of a rounding boundary
    g32, i32 = gau.astype(np.float32), indep.astype(np.float32)
    differ = g32 != i32
    assert differ.sum() <= 2
    for k in np.flatnonzero(differ):
        mid = 0.5 * (float(g32[k]) + float(i32[k]))
        assert abs(gau[k] - mid) <= 1e-12 * indep.max()
    assert (np.diff(gau) > 0).all()
    # the deviations the README states
    assert abs(gau[-1] - 3.487) < 5e-4 and abs((gau ** 2).mean() - 0.99936) < 5e-6
    with pytest.raises(ValueError, match="kind"):
        privacy.noise_tables("cauchy")


def test_host_twin_is_the_reference():
    from splitcnn import privacy
    for seed, t in LAW_KEYS:
        rows = [0, 1, 7, 2 ** 31 + 5]
        neg, k, G = privacy.noise_draws(rows, t, seed)
        wneg, wk, wG = R.draws(rows, t, seed)
        assert np.array_equal(neg.astype(bool), wneg) and np.array_equal(k, wk) and np.array_equal(G, wG)
    assert R.clz32(np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 65536], dtype=np.uint64)).tolist() == [32, 31, 0, 0, 15]


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_the_law_of_the_draws(kind):
    """64 rows x 16,384 draws per key at unit scale: pooled mean, second moment and (Laplace) tail mass within 5
    standard errors of the law's own moments, every per-element mean over the rows within 6, lag-1 correlation
    within 5. The moments come from the table and the geometric law by enumeration (cut_noise_ref.law_moments)."""
    table, tail = tables(kind)
    m2, m4, _ = R.law_moments(table, tail)
    if kind == "laplace":
        assert abs(m2 - 2.0) < 1e-6 and abs(m4 - 24.0) < 1e-3      # Laplace(1): E x^2 = 2, E x^4 = 24
    else:
        assert abs(m2 - 0.99936) < 5e-6
    N = LAW_ROWS * R.SAMPLE
    for seed, t in LAW_KEYS:
        x = R.noise(np.arange(LAW_ROWS), t, seed, table, tail, 1.0)[0].astype(np.float64)
        z_mean = x.mean() / math.sqrt(m2 / N)
        z_m2 = ((x ** 2).mean() - m2) / math.sqrt((m4 - m2 ** 2) / N)
        z_el = np.abs(x.mean(axis=0)).max() / math.sqrt(m2 / LAW_ROWS)
        z_lag = (x[:, :-1] * x[:, 1:]).mean() / m2 * math.sqrt(LAW_ROWS * (R.SAMPLE - 1))
        print(f"{kind} seed {seed} t {t}: mean {z_mean:+.2f} second moment {z_m2:+.2f} per-element {z_el:.2f} "
              f"lag-1 {z_lag:+.2f} standard errors")
        assert abs(z_mean) <= 5 and abs(z_m2) <= 5 and z_el <= 6 and abs(z_lag) <= 5
        if kind == "laplace":
            p = 2.0 ** -10     # |x| > 10 ln 2 exactly when G >= 10: the table stays inside (0, ln 2)
            z_tail = ((np.abs(x) > 10 * math.log(2.0)).mean() - p) / math.sqrt(p * (1 - p) / N)
            print(f"  tail mass beyond 10 ln 2: {z_tail:+.2f} standard errors")
            assert abs(z_tail) <= 5
        neg, k, _ = R.draws(np.arange(LAW_ROWS), t, seed)
        assert abs(neg.mean() - 0.5) <= 5 * 0.5 / math.sqrt(N)
        assert np.bincount(k.ravel(), minlength=1024).min() > 0


def test_a_slice_with_its_row0_is_the_rows_of_the_whole():
    bits = R.sample_bits()
    table, tail = tables("laplace")
    kw = dict(table=table, tail=tail, scale=0.5, clip=R.CLIP, seed=5, t=1)
    whole, wstats = R.apply(bits, row0=0, **kw)
    part, pstats = R.apply(bits[2:7], row0=2, **kw)
    wrong, _ = R.apply(bits[2:7], row0=0, **kw)
    assert R.same_bits(part, whole[2:7]) and R.same_f32(pstats, wstats[2:7])
    assert not R.same_bits(wrong, whole[2:7])


def test_the_sample_rows_are_what_their_names_say():
    names = [n for n, _ in R.samples()]
    bits = R.sample_bits()
    x = R.to_f32(bits).astype(np.float64)
    norm, coef = R.clip_stats(R.to_f32(bits), R.CLIP)
    i = names.index
    assert norm[i("all_zero")] == 0 and coef[i("all_zero")] == 1
    for n in ("relu_0", "relu_1", "relu_2"):
        r = x[i(n)]
        assert (r >= 0).all() and 0.4 < (r == 0).mean() < 0.6 and not (bits[i(n)] == 0x8000).any()
    exact = np.sqrt((x[i("under_clip")] ** 2).sum()), np.sqrt((x[i("over_clip")] ** 2).sum())
    assert R.CLIP * (1 - 2e-3) < exact[0] < R.CLIP < exact[1] < R.CLIP * (1 + 2e-3)
    assert coef[i("under_clip")] == 1 and coef[i("over_clip")] < 1
    assert (bits[i("signed_neg_zero")] == 0x8000).sum() > 2000 and (x[i("signed_neg_zero")] < 0).any()
    assert np.isinf(norm[i("bf16_max")]) and coef[i("bf16_max")] == 0
    assert np.isnan(norm[i("has_nan")]) and np.isnan(coef[i("has_nan")])
    assert np.isinf(norm[i("has_inf")]) and coef[i("has_inf")] == 0
    # the float32 norm of the reference is inside its own float64 bound
    ok = R.norm_bound_applies(bits)
    assert ok.sum() >= 8
    n64 = np.sqrt((x[ok] ** 2).sum(axis=1))
    assert (np.abs(norm[ok].astype(np.float64) - n64) <= R.norm_bound(n64)).all()
    # IEEE, no special case
    y, _ = R.apply(bits, clip=R.CLIP)
    assert R.is_nan_bits(y[i("has_nan")]).all()
    assert R.is_nan_bits(y[i("has_inf")]).sum() == 1 and not (y[i("has_inf")] & 0x7FFF)[np.arange(R.SAMPLE) != 4321].any()
    assert not (y[i("bf16_max")] & 0x7FFF).any() and y[i("bf16_max")][5] == 0x8000
    y, stats = R.apply(bits)
    assert stats is None and np.array_equal(y[~R.is_nan_bits(bits)], bits[~R.is_nan_bits(bits)])


@pytest.mark.parametrize("variant", ["k_low", "G_from_r", "fma", "noise_before_clip"])
def test_wrong_variants_are_visible(variant):
    """A kernel that took k from r's low bits, G from r, contracted scale * a + c into one fma, or added the noise in
    front of the clip gives other bits on the device tests' rows."""
    bits = R.sample_bits()
    seen = 0
    for law in ("laplace", "gaussian", "hand"):
        if variant == "G_from_r" and law == "gaussian":
            continue   # tail = 0: G does not enter
        table, tail = tables(law)
        for seed, t, row0 in R.KEYS:
            kw = dict(table=table, tail=tail, scale=R.SCALES[law], clip=R.CLIP, seed=seed, t=t, row0=row0)
            want, _ = R.apply(bits, **kw)
            got, _ = R.apply(bits, variant=variant, **kw)
            differ = (got != want) & ~R.is_nan_bits(want)
            # a contraction moves a float32 result by one ulp, which bf16 shows only next to a rounding boundary
            # (about 2^-16 of the elements): it is visible on the set as a whole, the others under every key
            assert differ.any() or variant == "fma", (law, seed, t, row0)
            seen += int(differ.sum())
    print(f"{variant}: {seen} elements differ")
    assert seen > 0
