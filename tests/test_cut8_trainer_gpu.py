"""wide.WideTrainer(cut_codec=codec.Fp8Cut(...)), B = 8, two steps: the fused step — eager and as a captured graph — is
bit for bit the hand-composed one whose cut and cut gradient are quantised on the host by tests/cut8_ref.py (the
wire's arithmetic); evaluation quantises the cut the same way and touches no training state; a direction set to None
stays dense; the codec combines with optim=, ema= and loss=."""
import numpy as np
import pytest
import torch

import cut8_ref as R

pytestmark = pytest.mark.gpu

B = 8
FORMATS = [("e4m3", "e5m2"), ("e4m3", None), (None, "e5m2")]


def _batches(gpu, n=2):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(23)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def _quantise(t, fmt):
    """What the other side of the wire receives for t, by the host reference (t itself where the direction is dense)."""
    if fmt is None:
        return t
    return R.roundtrip(t.cpu(), fmt).to(t.device)


def _trainer(gpu, fwd, bwd, graph, **kw):
    from splitcnn.codec import Fp8Cut
    from splitcnn.wide import WideTrainer, init_wide_models
    codec = Fp8Cut(fwd=fwd, bwd=bwd) if (fwd or bwd) else None
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=codec, **kw)


def _state(c, s):
    return [t.clone() for t in (c.params, c.m, c.v, c.step_ctr, c.grads, s.params, s.m, s.v, s.step_ctr, s.grads)]


def _losses(log):
    torch.cuda.synchronize()
    return [l for _, l in log.flush()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def hand(gpu):
    """The hand-composed two steps per (fwd, bwd), computed once: client.forward, the reference's quantisation of the
    cut on the host, server.step_request on that, the reference's quantisation of dcut, client.backward_step."""
    from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
    out = {}
    for fwd, bwd in FORMATS + [(None, None)]:
        a, b = init_wide_models(seed=0)
        c, s = WideClientStage(a, device=gpu), WideServerStage(b, device=gpu, seed=0)
        wire = []
        for x, y in _batches(gpu):
            cut = c.forward(x)
            cut_q = _quantise(cut, fwd)
            dcut, _ = s.step_request(cut_q, y)
            dcut_q = _quantise(dcut.clone(), bwd)
            c.backward_step(dcut_q)
            wire.append((cut.clone(), cut_q.clone(), dcut_q.clone()))
        out[fwd, bwd] = {"state": _state(c, s), "losses": _losses(s.loss_log), "wire": wire}
    return out


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fwd,bwd", FORMATS)
def test_fused_step_is_the_hand_composed_step(gpu, hand, fwd, bwd, graph):
    tr = _trainer(gpu, fwd, bwd, graph)
    want = hand[fwd, bwd]
    for k, (x, y) in enumerate(_batches(gpu)):
        tr.step(x, y)
        cut, cut_q, dcut_q = want["wire"][k]
        # what the head read and what the client back-propagated, where the step left them
        assert torch.equal(tr.client._b("cut", (B, 32, 8, 8, 8), torch.bfloat16).view(torch.int16), cut.view(torch.int16))
        if fwd is not None:
            got = tr.server._b("cut_q", (B, 32, 8, 8, 8), torch.bfloat16)
            assert torch.equal(got.view(torch.int16), cut_q.view(torch.int16))
        got = tr.server._b("dcut", (B, 32, 8, 8, 8), torch.bfloat16)
        assert torch.equal(got.view(torch.int16), dcut_q.view(torch.int16))
    assert _same(_state(tr.client, tr.server), want["state"])
    assert _losses(tr.loss_log) == want["losses"]
    # and the codec is not a no-op: the plain step ends elsewhere
    plain = hand[None, None]
    assert not torch.equal(want["state"][0], plain["state"][0]) and not torch.equal(want["state"][5], plain["state"][5])


def test_a_dense_direction_keeps_its_bits(gpu, hand):
    """bwd=None: the gradient the client saw is the server's own dcut; fwd=None: the head read the client's own cut."""
    plain_cut, _, _ = hand[None, None]["wire"][0]
    cut, cut_q, _ = hand[None, "e5m2"]["wire"][0]
    assert torch.equal(cut_q.view(torch.int16), cut.view(torch.int16)) and torch.equal(cut, plain_cut)
    tr = _trainer(gpu, "e4m3", None, False)
    x, y = _batches(gpu)[0]
    calls = []
    real = tr.cut_codec.roundtrip
    tr.cut_codec.roundtrip = lambda t, out, d: (calls.append(d), real(t, out, d))[1]
    tr.step(x, y)
    tr.eval_batch(x, y)
    assert calls == ["fwd", "fwd"]      # one launch in the step, one in the evaluation, none for the dense gradient
    none = _trainer(gpu, None, None, False)
    assert none.cut_codec is None
    none.step(x, y)
    assert _same(_state(none.client, none.server)[:4], [t for t in _plain_first_step(gpu, x, y)])


def _plain_first_step(gpu, x, y):
    from splitcnn.wide import WideTrainer, init_wide_models
    tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False)
    tr.step(x, y)
    return _state(tr.client, tr.server)[:4]


@pytest.mark.parametrize("graph", [False, True])
def test_evaluation_quantises_the_cut_and_touches_nothing(gpu, graph):
    from splitcnn.metrics import EvalMetrics
    (x0, y0), (x1, y1) = _batches(gpu)
    tr = _trainer(gpu, "e4m3", "e5m2", graph)
    two = _trainer(gpu, "e4m3", "e5m2", graph)
    tr.step(x0, y0)
    two.step(x0, y0)
    before = _state(tr.client, tr.server)
    # expected: server.evaluate on the host-quantised cut of the same weights
    cut = tr.client.forward(x1, tag="ref")
    m = EvalMetrics(gpu)
    pred, loss_i = tr.server.evaluate(_quantise(cut, "e4m3"), y1, metrics=m)
    want_pred, want_loss, want_logits = pred.clone(), loss_i.clone(), tr.server.eval_logits.clone()
    want = m.result()
    tr.server.evaluate(cut, y1)
    assert not torch.equal(tr.server.eval_logits, want_logits)   # the quantisation is visible in the logits
    p, l = tr.eval_batch(x1, y1)
    assert torch.equal(p, want_pred) and torch.equal(l, want_loss) and torch.equal(tr.server.eval_logits, want_logits)
    assert torch.equal(tr.eval_cut.view(torch.int16), cut.view(torch.int16))   # eval_cut stays the client's own cut
    p2, lg = tr.predict(x1, return_logits=True)
    assert torch.equal(p2, want_pred) and torch.equal(lg, want_logits)
    res = tr.evaluate([(x1, y1)])
    assert (res.n, res.correct, res.loss) == (want.n, want.correct, want.loss)
    assert np.array_equal(res.confusion, want.confusion)
    assert _same(_state(tr.client, tr.server), before)
    # step, evaluate, step == step, step
    tr.step(x1, y1)
    two.step(x1, y1)
    assert _same(_state(tr.client, tr.server), _state(two.client, two.server))
    assert _losses(tr.loss_log) == _losses(two.loss_log)


def test_combines_with_optim_ema_and_loss(gpu):
    from splitcnn import optim
    from splitcnn.loss import SoftCrossEntropy
    kw = dict(optim=optim.Adam(1e-3, weight_decay=0.01), ema=optim.EMA(0.99, device=gpu),
              loss=SoftCrossEntropy(label_smoothing=0.1))
    from splitcnn.wide import WideTrainer, init_wide_models
    keys = set(WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, **kw).optimizer_state())
    trs = [_trainer(gpu, "e4m3", "e5m2", graph, **kw) for graph in (False, True)]
    for x, y in _batches(gpu):
        for tr in trs:
            tr.step(x, y)
    a, b = trs
    assert set(a.optimizer_state()) == keys and "client.ema" in keys
    assert _same(_state(a.client, a.server) + [a.client.ema, a.server.ema],
                 _state(b.client, b.server) + [b.client.ema, b.server.ema])
    la, lb = _losses(a.loss_log), _losses(b.loss_log)
    assert la == lb and len(la) == 2 and all(np.isfinite(la))
    x, y = _batches(gpu)[0]
    pe, _ = a.eval_batch(x, y, weights="ema")
    pg, _ = b.eval_batch(x, y, weights="ema")
    assert torch.equal(pe, pg)
    a.server.check_labels()


def test_refuses_a_foreign_codec(gpu):
    from splitcnn.wide import WideTrainer
    with pytest.raises(TypeError, match="Fp8Cut"):
        WideTrainer(device=gpu, graph=False, cut_codec="e4m3")
