"""WideTrainer(dp=privacy.DPSGD(...)) at B = 8, eager and as a captured graph: bit for bit the plain trainer where nothing
clips, bit for bit the hand-composed sequence through ops where the median norm clips, and the noise row against the
host twin under tests/test_dpsgd_gpu.py's bound. The difference of two reduced gradients, and the gradient the optimizer
wrote, add what float32 sums of n rows in whatever order can lose: n 2^-24 sum |rows| each, the textbook worst case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NOISE_RTOL = 3.5 * 2.0 ** -23     # derived in tests/test_dpsgd_gpu.py
B = 8


def make(gpu, graph, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, **kw)


@pytest.fixture(scope="module")
def batches(gpu):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(42)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(4)]


def run(tr, batches, n):
    for x, y in batches[:n]:
        tr.step(x, y)
    torch.cuda.synchronize()
    return tr.client.params.clone(), tr.server.params.clone(), [v for _, v in tr.loss_log.flush()]


@pytest.fixture(scope="module")
def median_norm(gpu, batches):
    from splitcnn.privacy import DPSGD
    tr = make(gpu, False, dp=DPSGD(float("inf"), 0.0))
    tr.step(*batches[0])
    return float(tr.dp_stats()[:, 0].median())   # torch's median of 8 is the 4th smallest: 3 norms lie below it


@pytest.mark.parametrize("graph", (False, True))
def test_no_clip_no_noise_is_the_plain_trainer(gpu, batches, graph):
    from splitcnn.privacy import DPSGD
    plain = run(make(gpu, graph), batches, 2)
    tr = make(gpu, graph, dp=DPSGD(float("inf"), 0.0))
    got = run(tr, batches, 2)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[2] == plain[2]
    assert (tr.dp_stats()[:, 1] == 1).all() and (tr.dp_stats()[:, 0] > 0).all()


@pytest.mark.parametrize("graph", (False, True))
def test_clipped_step_is_the_hand_composed_sequence(gpu, batches, median_norm, graph):
    from splitcnn import _lib, ops
    from splitcnn.privacy import DPSGD
    x, y = batches[0]
    tr = make(gpu, graph, dp=DPSGD(median_norm, 0.0))
    got = run(tr, batches, 1)
    stats = tr.dp_stats()
    assert 0 < int((stats[:, 1] < 1).sum()) < B and (stats[:, 1] <= 1).all()
    c, s = (ref := make(gpu, False)).client, ref.server
    dcut = s.step_request(c.forward(x), y)[0]
    c.backward_slabs(dcut)                                          # leaves dp2 and da1m of the unscaled dcut
    work = ops.wide_grad_sqnorm(x, c._da1m, c._a1, c._dp2, c._code2, c._p2, dcut, c._code3)
    want = ops.dp_coef(work, float(B), torch.full((1,), median_norm, device=gpu))
    _lib.call("slk_cut_scale_rows", dcut.data_ptr(), B, want.data_ptr(), dcut.data_ptr(),
              torch.cuda.current_stream(gpu).cuda_stream)
    c.backward_step(dcut)
    torch.cuda.synchronize()
    assert torch.equal(stats.view(torch.int32), want.cpu().view(torch.int32))
    assert torch.equal(got[0], c.params) and torch.equal(got[1], s.params)


@pytest.mark.parametrize("graph", (False, True))
def test_noise_row_follows_the_counter_and_the_setters(gpu, batches, median_norm, graph):
    from splitcnn import ops
    from splitcnn.privacy import DPSGD
    from splitcnn.wide import client_backward_slab_shapes
    f = np.float32
    sigma, C = 1.25, median_norm
    tr = make(gpu, graph, dp=DPSGD(C, sigma, seed=5))
    c = tr.client
    for k, (x, y) in enumerate(batches):
        if k == 2:
            sigma *= 2
            c.dp.set_noise_multiplier(sigma)
        if k == 3:
            C *= 3
            c.dp.set_max_grad_norm(C)
        tr.step(x, y)
        torch.cuda.synchronize()
        assert int(c.step_ctr.item()) == k + 1                       # the step read the counter before this tick
        std = float(f(f(sigma) * f(C)) * f(1.0 / B))
        for name, (lo, hi, _), (ns, w) in zip(("s1_dp", "s2_dp", "s3_dp"), c.PAIRS, client_backward_slab_shapes(B)):
            sl = c._b(name, (ns + 1, w), torch.float32)
            want = std * c.dp.noise_draws(np.arange(lo, hi), k)
            assert (np.abs(sl[-1].double().cpu().numpy() - want) <= NOISE_RTOL * np.abs(want)).all() and np.abs(want).max() > 0
            g_all, g_wo, g_opt = (t.double().cpu().numpy() for t in (ops.reduce_slabs(sl), ops.reduce_slabs(sl[:-1]),
                                                                     c.grads[lo:hi]))
            slack = 2 * sl.shape[0] * 2.0 ** -24 * sl.abs().sum(dim=0).double().cpu().numpy()
            assert (np.abs((g_all - g_wo) - want) <= NOISE_RTOL * np.abs(want) + slack).all()
            assert (np.abs(g_opt - g_all) <= slack).all()            # the optimizer summed the noise row too


def test_refused_combinations(gpu):
    from splitcnn import dist, optim, privacy
    from splitcnn.wide import WideClientStage
    dp = privacy.DPSGD(1.0, 1.0)
    for kw in (dict(leak_loss=privacy.DcorLoss(0.1)), dict(clip=optim.ClipNorm(1.0)), dict(optim=optim.LAMB())):
        with pytest.raises(ValueError, match="dp="):
            make(gpu, False, dp=dp, **kw)
    with pytest.raises(RuntimeError, match="no training step"):
        make(gpu, False, dp=dp).dp_stats()
    stage = WideClientStage(device=gpu, dp=dp)
    stage.forward(torch.zeros(2, 3, 32, 32, device=gpu))
    with pytest.raises(ValueError, match="accumulate"):
        stage.backward_grads(torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu), accumulate=True)
    with pytest.raises(ValueError, match="DP-SGD"):
        dist.WideHub(stage, 0, 2)
