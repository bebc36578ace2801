"""MixUp / Beta(alpha) mixing on the CPU: loss.beta_quantiles and the two table constructions, the blend rule's
identities and the wrong variants it must be told apart from (on the GPU tests' own table and pixels), the host twin
loss.mix_draws against tests/mixup_ref.py and loss.cutmix_draws, and the loaders' refusals."""
import numpy as np
import pytest

import cutmix_ref as M
import mixup_ref as R
from splitcnn import loss as L

ALPHAS = (0.1, 0.2, 0.5, 0.8, 1.0, 2.0, 8.0, 32.0)
U = (np.arange(1024) + 0.5) / 1024


# ------------------------------------------------------------------------------------ the quantiles and the tables
def test_beta_quantiles_closed_forms():
    for alpha, want in ((1.0, U), (0.5, np.sin(np.pi * U / 2) ** 2), (2.0, 0.5 - np.sin(np.arcsin(1 - 2 * U) / 3))):
        q = L.beta_quantiles(alpha)
        assert q.dtype == np.float64 and q.shape == (1024,)
        assert np.abs(q - want).max() <= 1e-12, alpha
    assert np.array_equal(L.beta_quantiles(1.0, n=1024), L.beta_quantiles(1.0))
    q5 = L.beta_quantiles(2.0, n=5)
    assert q5.shape == (5,) and q5[2] == 0.5 and np.abs(q5 - (0.5 - np.sin(np.arcsin(1 - 2 * (np.arange(5) + 0.5) / 5) / 3))).max() <= 1e-12


@pytest.mark.parametrize("alpha", ALPHAS)
def test_beta_quantiles_symmetric_monotone_and_inverse(alpha):
    q = L.beta_quantiles(alpha)
    assert np.array_equal(q[512:], (1.0 - q[:512])[::-1]), "q(1 - u) = 1 - q(u), by construction"
    assert (q >= 0).all() and (q <= 1).all() and (q[:512] > 0).all() and (q[:512] < 0.5).all()
    assert (np.diff(q[:512]) > 0).all() and (np.diff(q) >= 0).all()
    # it inverts the distribution function: a midpoint-rule integral of the density up to q_k returns u_k (in t = x^alpha
    # the integrand x^(alpha-1) (1-x)^(alpha-1) dx = (1 - t^(1/alpha))^(alpha-1) dt / alpha is bounded for alpha <= 1)
    import math
    logb = 2 * math.lgamma(alpha) - math.lgamma(2 * alpha)
    for k in (0, 100, 511):
        n = 200000
        if alpha <= 1:
            t = (np.arange(n) + 0.5) / n * q[k] ** alpha
            val = np.sum((1 - t ** (1 / alpha)) ** (alpha - 1)) * (q[k] ** alpha / n) / alpha
        else:
            x = (np.arange(n) + 0.5) / n * q[k]
            val = np.sum((x * (1 - x)) ** (alpha - 1)) * (q[k] / n)
        assert abs(val / math.exp(logb) - U[k]) <= 1e-6 * max(U[k], 1e-3), (alpha, k)


def test_beta_quantiles_against_scipy():
    sp = pytest.importorskip("scipy.special")
    for alpha in ALPHAS:
        want = sp.betaincinv(alpha, alpha, U)
        assert np.abs(L.beta_quantiles(alpha) / want - 1).max() <= 1e-10, alpha


@pytest.mark.parametrize("bad", (0.0, 0.09, 32.5, -1.0, float("nan"), float("inf")))
def test_alpha_bounds(bad):
    with pytest.raises(ValueError, match=r"\[0\.1, 32\]"):
        L.beta_quantiles(bad)
    for make in (lambda a: L.CutMix(alpha=a), lambda a: L.MixUp(alpha=a), lambda a: L.Mix(cutmix_alpha=a),
                 lambda a: L.Mix(mixup_alpha=a)):
        with pytest.raises(ValueError, match="alpha"):
            make(bad)


def test_mix_classes():
    assert L.CutMix() == L.CutMix(1.0, 0, 1.0) and L.CutMix().alpha == 1.0
    m = L.MixUp()
    assert (m.alpha, m.prob, m.seed) == (1.0, 1.0, 0) and L.MixUp(0.4).alpha == 0.4
    x = L.Mix()
    assert (x.cutmix_alpha, x.mixup_alpha, x.prob, x.switch, x.seed) == (1.0, 1.0, 1.0, 0.5, 0)
    L.beta_quantiles(0.1), L.beta_quantiles(32)
    for bad in (-0.1, 1.5, float("nan")):
        for make in (lambda p: L.MixUp(prob=p), lambda p: L.Mix(prob=p), lambda p: L.Mix(switch=p)):
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                make(bad)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_table_constructions(alpha):
    q = L.beta_quantiles(alpha)
    lam, cut = L.lam_table(alpha), L.cut_table(alpha)
    assert lam.dtype == np.float32 and lam.shape == (1024,) and np.array_equal(lam, q.astype(np.float32))
    assert (lam >= 0).all() and (lam <= 1).all()
    assert cut.dtype == np.uint32 and cut.shape == (1024,)
    import math
    want = [min(math.floor(math.sqrt(1.0 - float(v)) * 4294967296.0), 4294967295) for v in q]
    assert cut.tolist() == want
    assert (np.diff(cut.astype(np.int64)) <= 0).all(), "the side ratio falls as lam rises"
    if alpha <= 0.2:
        assert lam[-1] == 1.0 and cut[0] == 4294967295, "the extreme entries saturate, which is legal"
    # side = (entry * H) >> 32 lies in [0, H)
    for H in (28, 32):
        side = (cut.astype(np.uint64) * np.uint64(H)) >> np.uint64(32)
        assert side.max() <= H - 1


def test_mix_tables_refuses_other_types():
    with pytest.raises(TypeError, match="CutMix.*MixUp.*Mix"):
        L.mix_tables(0.5, "cpu")
    assert L.mix_tables(L.CutMix(), "cpu") == (None, None) and L.mix_tables(None, "cpu") == (None, None)
    ct, lt = L.mix_tables(L.Mix(0.5, 0.4), "cpu")
    assert ct.dtype.is_floating_point is False and ct.element_size() == 4 and tuple(ct.shape) == (1024,)
    assert np.array_equal(ct.numpy().view(np.uint32), L.cut_table(0.5)) and np.array_equal(lt.numpy(), L.lam_table(0.4))
    ct, lt = L.mix_tables(L.CutMix(alpha=0.5), "cpu")
    assert lt is None and np.array_equal(ct.numpy().view(np.uint32), L.cut_table(0.5))
    ct, lt = L.mix_tables(L.MixUp(0.4), "cpu")
    assert ct is None and np.array_equal(lt.numpy(), L.lam_table(0.4))


# ------------------------------------------------------------------------------------ the blend rule
def test_blend_identities_on_every_pixel_pair():
    """wb = 0 returns sample i's ToTensor value bit for bit and wb = 1 sample i2's; a denormal wb adds at most a
    denormal to it, which Normalize's subtraction of a normal mean absorbs: the image is bit for bit the plain one."""
    pa, pb = R.all_pairs()
    fa, fb = pa.astype(np.float32) / np.float32(255), pb.astype(np.float32) / np.float32(255)
    assert np.array_equal(R.blend(pa, pb, np.float32(0)).view(np.uint32), fa.view(np.uint32))
    assert np.array_equal(R.blend(pa, pb, np.float32(1)).view(np.uint32), fb.view(np.uint32))
    for sh in R.SHAPES.values():
        for mean, std in zip(sh["mean"], sh["std"]):
            plain_a, plain_b = R.normalize(fa, (mean,), (std,)), R.normalize(fb, (mean,), (std,))
            for wb in (np.float32(0), R.DENORMAL, np.float32(1.4e-45)):
                got = R.normalize(R.blend(pa, pb, wb), (mean,), (std,))
                assert np.array_equal(got.view(np.uint32), plain_a.view(np.uint32)), (wb, mean)
            got = R.normalize(R.blend(pa, pb, np.float32(1)), (mean,), (std,))
            assert np.array_equal(got.view(np.uint32), plain_b.view(np.uint32))
    mid = R.blend(pa, pb, np.float32(0.5))
    assert (mid >= np.minimum(fa, fb)).all() and (mid <= np.maximum(fa, fb)).all()


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_wrong_variants_differ_on_the_gpu_tests_own_inputs(name):
    """The GPU comparison can see an fma, the lerp form and a blend after Normalize: on the hand-made table and the
    very samples case (b) runs, each variant differs from the rule in some pixel of a sample drawing 1/3, 0.2 and 0.9
    (and an fma differs nowhere at 0.5, which is why 0.5 alone would not do)."""
    sh = R.SHAPES[name]
    C, H, W = sh["shape"]
    img, _ = R.dataset(name)
    table = R.hand_table()
    for v in R.HAND_VALUES:
        assert (table.view(np.uint32) == np.float32(v).view(np.uint32)).sum() == 128
    d = R.draws(H, W, 4, lam_table=table)
    idx, idx2 = R.pick_blend(d, 4)
    seen = {"contracted": set(), "lerp": set(), "after": set()}
    fma_at_half = 0
    for i, i2 in zip(idx[:R.B], idx2[:R.B]):
        wb = d["wb"][i]
        pa = R.shown(img[i], M.crop_one(int(i), 0, 0, 4, True), 4)
        pb = R.shown(img[i2], M.crop_one(int(i2), 0, 0, 4, True), 4)
        rule = R.normalize(R.blend(pa, pb, wb), sh["mean"], sh["std"]).view(np.uint32)
        for key, other in (("contracted", R.normalize(R.blend_contracted(pa, pb, wb), sh["mean"], sh["std"])),
                           ("lerp", R.normalize(R.blend_lerp(pa, pb, wb), sh["mean"], sh["std"])),
                           ("after", R.blend_after_normalize(pa, pb, wb, sh["mean"], sh["std"]))):
            if not np.array_equal(rule, other.view(np.uint32)):
                seen[key].add(int(wb.view(np.uint32)))
            if key == "contracted" and wb == 0.5:
                fma_at_half += int((rule != other.view(np.uint32)).sum())
    telling = set(R.HAND_VALUES[[2, 3, 5]].view(np.uint32).tolist())
    for key, got in seen.items():
        assert telling <= got, (key, got)
    assert fma_at_half == 0


def test_wrong_variants_rates_on_every_pixel_pair():
    pa, pb = R.all_pairs()
    for wb in (np.float32(1) / np.float32(3), np.float32(0.2), np.float32(0.9)):
        rule = R.blend(pa, pb, wb).view(np.uint32)
        assert 0.05 < (R.blend_contracted(pa, pb, wb).view(np.uint32) != rule).mean() < 0.3
        assert (R.blend_lerp(pa, pb, wb).view(np.uint32) != rule).mean() > 0.05
    assert np.array_equal(R.blend_contracted(pa, pb, np.float32(0.5)).view(np.uint32), R.blend(pa, pb, np.float32(0.5)).view(np.uint32))


# ------------------------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("H,W", [(32, 32), (28, 28)])
@pytest.mark.parametrize("seed,epoch", [(0, 0), (7, 3), (0xFFFFFFFF, 0xFFFFFFFF)])
def test_host_twin_equals_the_reference(H, W, seed, epoch):
    idx = np.concatenate([np.arange(300), [49999, 59999, 2 ** 31 - 1]])
    ct, lt = L.cut_table(0.5), L.lam_table(0.4)
    for prob, switch, tabs in ((1.0, 0.5, (ct, lt)), (0.5, 0.5, (ct, lt)), (0.5, 0.25, (ct, lt)), (1.0, 0.0, (ct, lt)),
                               (1.0, 1.0, (ct, lt)), (0.5, 0.5, (ct, None)), (0.5, 0.5, (None, lt)), (0.0, 0.5, (ct, lt))):
        apply, cut, k, y1, y2, x1, x2, wb = L.mix_draws(idx, epoch, seed, H, W, prob, switch, *tabs)
        assert apply.dtype == bool and cut.dtype == bool and wb.dtype == np.float32
        assert all(v.dtype == np.int64 for v in (k, y1, y2, x1, x2))
        want = [R.draw_one(int(i), epoch, seed, H, W, prob, switch, *tabs) for i in idx]
        mode = np.where(apply & cut, "cut", np.where(apply, "blend", "plain"))
        assert mode.tolist() == [w[0] for w in want]
        assert k.tolist() == [w[1] for w in want] and 0 <= k.min() and k.max() <= 1023
        is_cut = mode == "cut"
        for got, j in ((y1, 2), (y2, 3), (x1, 4), (x2, 5)):
            assert got[is_cut].tolist() == [w[j] for w in want if w[0] == "cut"]
        assert np.array_equal(wb.view(np.uint32), np.array([w[7] for w in want], dtype=np.float32).view(np.uint32))
        # apply, cy, cx are slk_image_batch_mix's: the same samples are picked, and the box centres agree
        a0, by1, by2, bx1, bx2, _ = L.cutmix_draws(idx, epoch, seed, H, W, prob)
        assert np.array_equal(apply, a0)
        if tabs[1] is None:
            assert cut.all()
        if tabs[0] is None:
            assert not cut.any() and (y2 == y1).all() and (x2 == x1).all()
    with pytest.raises(ValueError):
        L.mix_draws(idx, 0, 0, H, W)


def test_host_twin_centres_are_cutmix_draws_centres():
    """With only a cut table, apply, cy and cx equal slk_image_batch_mix's: on 2048 indices, wherever both boxes are
    unclipped in a direction their midpoints coincide (a box is [c - half, c + half))."""
    idx = np.arange(2048)
    for H, W in ((32, 32), (28, 28)):
        apply, cut, k, y1, y2, x1, x2, wb = L.mix_draws(idx, 0, 0, H, W, 0.5, 0.5, L.cut_table(1.0), None)
        a0, by1, by2, bx1, bx2, _ = L.cutmix_draws(idx, 0, 0, H, W, 0.5)
        assert np.array_equal(apply, a0) and 900 < apply.sum() < 1150
        for lo, hi, blo, bhi, D in ((y1, y2, by1, by2, H), (x1, x2, bx1, bx2, W)):
            free = (lo > 0) & (hi < D) & (blo > 0) & (bhi < D)
            assert free.sum() > 300 and np.array_equal((lo + hi)[free], (blo + bhi)[free])
        # the side is the table's: Beta(1, 1) through the quantile table has the law of the integer trick
        assert abs(wb[apply].mean() - L.cutmix_draws(idx, 0, 0, H, W, 0.5)[5][apply].mean()) < 0.03


# ------------------------------------------------------------------------------------ the loaders and ops refuse
class _Set:
    images = np.zeros((4, 3, 32, 32), dtype=np.uint8)
    labels = np.zeros(4, dtype=np.uint8)

    def __len__(self):
        return 4


def test_loaders_refuse_other_mix_types():
    from splitcnn.cifar import CifarLoader
    from splitcnn.mnist import DeviceLoader
    for Loader in (CifarLoader, DeviceLoader):
        for bad in (0.5, "mixup", L.SoftCrossEntropy(0.1), L.MixUp):
            with pytest.raises(TypeError, match=r"CutMix, splitcnn\.loss\.MixUp, splitcnn\.loss\.Mix or None"):
                Loader(_Set(), device="cpu", mix=bad)


def test_ops_refuse_cpu_tensors_and_bad_tables():
    import torch
    from splitcnn import ops
    img, lbl = torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    ids = torch.zeros(2, dtype=torch.int64)
    kw = dict(mean=(0.5,) * 3, std=(0.25,) * 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_batch_blend(img, lbl, ids, ids, lam_table=torch.zeros(1024), **kw)
    with pytest.raises(ValueError, match="cut_table, lam_table or both"):
        ops.image_batch_blend(img, lbl, ids, ids, **kw)
