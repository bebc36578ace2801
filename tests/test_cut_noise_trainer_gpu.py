"""wide.WideTrainer(cut_noise=privacy.CutNoise(...)), B = 8, three steps: the fused step — eager and as a captured graph —
is bit for bit the hand-written sequence of stage calls (client.forward, CutNoise.apply under the client's counter,
server.step_request, CutNoise.scale_rows, client.backward_step); the noise differs from step to step and is the host
reference's; optimizer_state() carries the counters; scale = 0 without a clip is the plain trainer; with Fp8Cut the
order is noise, then codec; evaluation clips and adds nothing; cut_stats() is the reference's."""
import numpy as np
import pytest
import torch

import cut_noise_ref as R

pytestmark = pytest.mark.gpu

B, SEED, STEPS = 8, 9, 3
SCALE, CLIP = 0.3, 20.0   # the norms of the cut at initialisation are about 32: this bound binds on every row
CUT = (B, 32, 8, 8, 8)


def _batches(gpu, n=2):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(23)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def _noise(kind="laplace", scale=SCALE, clip=CLIP):
    from splitcnn.privacy import CutNoise
    return CutNoise(kind, scale=scale, clip=clip, seed=SEED)


def _trainer(gpu, graph, noise, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_noise=noise, **kw)


def _state(c, s):
    return [t.clone() for t in (c.params, c.m, c.v, c.step_ctr, c.grads, s.params, s.m, s.v, s.step_ctr, s.grads)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _losses(log):
    torch.cuda.synchronize()
    return [l for _, l in log.flush()]


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(t.shape[0], -1)


def _i16(t):
    return t.view(torch.int16)


def _hand(gpu, noise, codec=None):
    """STEPS hand-written steps on the same batch; the plain step where noise is None."""
    from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
    x, y = _batches(gpu)[0]
    a, b = init_wide_models(seed=0)
    c, s = WideClientStage(a, device=gpu), WideServerStage(b, device=gpu, seed=0)
    wire, states = [], []
    for k in range(STEPS):
        assert int(c.step_ctr.item()) == k and int(s.step_ctr.item()) == k
        cut = c.forward(x)
        raw = cut.clone()
        stats = torch.zeros(B, 2, device=gpu)
        if noise is not None:
            cut = noise.apply(cut, torch.empty_like(cut), c.step_ctr, row0=0,
                              stats=stats if noise.clip_value is not None else None)
        cut_n = cut.clone()
        if codec is not None:
            cut = codec.roundtrip(cut, torch.empty_like(cut), "fwd")
        dcut, _ = s.step_request(cut, y)
        if codec is not None:
            codec.roundtrip(dcut, dcut, "bwd")
        if noise is not None and noise.clip_value is not None:
            noise.scale_rows(dcut, stats, dcut)
        c.backward_step(dcut)
        wire.append((raw, cut_n, cut.clone(), dcut.clone(), stats.clone()))
        states.append(_state(c, s))
    return {"states": states, "losses": _losses(s.loss_log), "wire": wire}


@pytest.fixture(scope="module")
def hand(gpu):
    from splitcnn.codec import Fp8Cut
    return {"noise": _hand(gpu, _noise()), "plain": _hand(gpu, None), "codec": _hand(gpu, _noise(), Fp8Cut()),
            "gauss_noclip": _hand(gpu, _noise("gaussian", 0.2, None))}


@pytest.mark.parametrize("graph", [False, True])
def test_fused_step_is_the_hand_written_sequence(gpu, hand, graph):
    tr = _trainer(gpu, graph, _noise())
    want = hand["noise"]
    x, y = _batches(gpu)[0]
    with pytest.raises(RuntimeError, match="no training step"):
        tr.cut_stats()
    for k in range(STEPS):
        tr.step(x, y)
        _, cut_n, _, dcut, stats = want["wire"][k]
        assert torch.equal(_i16(tr.server._b("cut_n", CUT, torch.bfloat16)), _i16(cut_n))
        assert torch.equal(_i16(tr.server._b("dcut", CUT, torch.bfloat16)), _i16(dcut))
        assert torch.equal(tr.cut_stats(), stats.cpu())
        assert _same(_state(tr.client, tr.server), want["states"][k])
    assert _losses(tr.loss_log) == want["losses"]


def test_the_noise_is_the_references_and_differs_from_step_to_step(hand):
    """Every step's noised cut is the host reference's under the client's counter k (row0 = 0), not any other
    step's; cut_stats' pairs are the reference's."""
    from splitcnn import privacy
    t64, tail = privacy.noise_tables("laplace")
    table = t64.astype(np.float32)
    w = hand["noise"]["wire"]
    for k in range(STEPS):
        raw, cut_n, _, _, stats = w[k]
        want, wstats = R.apply(_bits(raw), table, np.float32(tail), np.float32(SCALE), np.float32(CLIP), SEED, k, 0)
        assert R.same_bits(_bits(cut_n), want) and R.same_f32(stats.cpu().numpy(), wstats)
        other, _ = R.apply(_bits(raw), table, np.float32(tail), np.float32(SCALE), np.float32(CLIP), SEED, k + 1, 0)
        assert not np.array_equal(other, want)
    coef = w[0][4][:, 1].cpu().numpy()
    assert (coef < 1).any()   # the clip binds at this bound: scale_rows is not the identity here


def test_negative_control_the_noise_moves_the_client_gradient(hand):
    gn, gp = hand["noise"]["states"][0][4], hand["plain"]["states"][0][4]
    assert (gn - gp).abs().max() > 1e-6 * gp.abs().max()
    assert not torch.equal(hand["noise"]["states"][0][0], hand["plain"]["states"][0][0])


@pytest.mark.parametrize("graph", [False, True])
def test_no_clip_has_no_backward_launch_and_matches(gpu, hand, graph):
    tr = _trainer(gpu, graph, _noise("gaussian", 0.2, None))
    x, y = _batches(gpu)[0]
    for k in range(STEPS):
        tr.step(x, y)
        assert _same(_state(tr.client, tr.server), hand["gauss_noclip"]["states"][k])
    with pytest.raises(RuntimeError, match="clip=None"):
        tr.cut_stats()
    with pytest.raises(RuntimeError, match="cut_noise"):
        _trainer(gpu, False, None).cut_stats()


def test_optimizer_state_reproduces_the_run(gpu, hand):
    x, y = _batches(gpu)[0]
    one = _trainer(gpu, True, _noise())
    one.step(x, y)
    state = {k: v.clone() for k, v in one.optimizer_state().items()}
    params = (one.client.params.clone(), one.server.params.clone())
    fresh = _trainer(gpu, True, _noise())
    fresh.client.params.copy_(params[0])
    fresh.server.params.copy_(params[1])
    fresh._state_written()
    fresh.load_optimizer_state(state)
    for k in (1, 2):
        one.step(x, y)
        fresh.step(x, y)
        assert _same(_state(one.client, one.server), hand["noise"]["states"][k])
        assert _same(_state(fresh.client, fresh.server), _state(one.client, one.server))


@pytest.mark.parametrize("graph", [False, True])
def test_scale_zero_without_a_clip_is_the_plain_trainer(gpu, hand, graph):
    tr = _trainer(gpu, graph, _noise("laplace", 0.0, None))
    x, y = _batches(gpu)[0]
    for k in range(STEPS):
        tr.step(x, y)
        assert _same(_state(tr.client, tr.server), hand["plain"]["states"][k])
    assert _losses(tr.loss_log) == hand["plain"]["losses"]


@pytest.mark.parametrize("graph", [False, True])
def test_with_a_codec_the_order_is_noise_then_codec(gpu, hand, graph):
    from splitcnn.codec import Fp8Cut
    tr = _trainer(gpu, graph, _noise(), cut_codec=Fp8Cut())
    x, y = _batches(gpu)[0]
    want = hand["codec"]
    for k in range(STEPS):
        tr.step(x, y)
        _, cut_n, cut_q, dcut, _ = want["wire"][k]
        assert torch.equal(_i16(tr.server._b("cut_n", CUT, torch.bfloat16)), _i16(cut_n))
        assert torch.equal(_i16(tr.server._b("cut_q", CUT, torch.bfloat16)), _i16(cut_q))
        assert torch.equal(_i16(tr.server._b("dcut", CUT, torch.bfloat16)), _i16(dcut))
        assert _same(_state(tr.client, tr.server), want["states"][k])
    assert not _same(want["states"][0][:1], hand["noise"]["states"][0][:1])


@pytest.mark.parametrize("graph", [False, True])
def test_evaluation_clips_and_adds_no_noise(gpu, graph):
    (x0, y0), (x1, y1) = _batches(gpu)
    tr, two = _trainer(gpu, graph, _noise()), _trainer(gpu, graph, _noise())
    quiet = _trainer(gpu, graph, _noise(scale=0.0))
    tr.step(x0, y0)
    two.step(x0, y0)
    for dst, src in ((quiet.client, tr.client), (quiet.server, tr.server)):
        dst.params.copy_(src.params)
    quiet._state_written()
    before = _state(tr.client, tr.server)
    stats = tr.cut_stats()
    p, l = (t.clone() for t in tr.eval_batch(x1, y1))
    logits = tr.server.eval_logits.clone()
    pq, lq = quiet.eval_batch(x1, y1)
    assert torch.equal(p, pq) and torch.equal(l, lq) and torch.equal(logits, quiet.server.eval_logits)
    pp, lg = tr.predict(x1, return_logits=True)
    ppq, lgq = quiet.predict(x1, return_logits=True)
    assert torch.equal(pp, ppq) and torch.equal(lg, lgq)
    # the clip is applied: the cut the head read is the reference's clip of the evaluation cut, nothing added
    want, _ = R.apply(_bits(tr.eval_cut), clip=np.float32(CLIP))
    assert R.same_bits(_bits(tr.server._b("eval_cut_n", CUT, torch.bfloat16)), want)
    assert not np.array_equal(want, _bits(tr.eval_cut))
    # a pure function of the weights: again, the same bits; no training state and no training stats moved
    p2, l2 = tr.eval_batch(x1, y1)
    assert torch.equal(p2, p) and torch.equal(l2, l)
    assert _same(_state(tr.client, tr.server), before) and torch.equal(tr.cut_stats(), stats)
    tr.step(x1, y1)
    two.step(x1, y1)
    assert _same(_state(tr.client, tr.server), _state(two.client, two.server))


def test_evaluation_on_averaged_weights_clips_too(gpu):
    from splitcnn.optim import EMA
    (x0, y0), (x1, y1) = _batches(gpu)
    tr = _trainer(gpu, True, _noise(), ema=EMA(0.9))
    tr.step(x0, y0)
    p, l = (t.clone() for t in tr.eval_batch(x1, y1, weights="ema"))
    want, _ = R.apply(_bits(tr.eval_cut), clip=np.float32(CLIP))
    assert R.same_bits(_bits(tr.server._b("eval_cut_n", CUT, torch.bfloat16)), want)
    p2, l2 = tr.eval_batch(x1, y1, weights="ema")
    assert torch.equal(p, p2) and torch.equal(l, l2)


def test_refusals(gpu):
    from splitcnn.wide import WideTrainer
    with pytest.raises(TypeError, match="CutNoise"):
        WideTrainer(device=gpu, cut_noise=0.5)
