"""wide.WideTrainer(cut_codec=codec.Fp8Cut(rounding=...)), B = 8: the fused step with a stochastically rounded cut
gradient (and with both directions stochastic) — eager and as a captured graph — is bit for bit the hand-composed one
whose wire tensors are rounded on the host by tests/cut8_sr_ref.py under the stage counters; consecutive steps use
different words; optimizer_state() carries the counters; evaluation rounds to nearest; the default rounding is
Fp8Cut()'s step."""
import pytest
import torch

import cut8_ref as R
import cut8_sr_ref as S

pytestmark = pytest.mark.gpu

B, SEED = 8, 9
ROUNDINGS = [{"bwd": "stochastic"}, "stochastic"]
CUT = (B, 32, 8, 8, 8)


def _batches(gpu, n=2):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(23)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def _codec(rounding):
    from splitcnn.codec import Fp8Cut
    return Fp8Cut("e4m3", "e5m2", rounding=rounding, seed=SEED)


def _trainer(gpu, rounding, graph, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=_codec(rounding), **kw)


def _state(c, s):
    return [t.clone() for t in (c.params, c.m, c.v, c.step_ctr, c.grads, s.params, s.m, s.v, s.step_ctr, s.grads)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _losses(log):
    torch.cuda.synchronize()
    return [l for _, l in log.flush()]


def _host(t, q, direction, counter):
    """What the other side of the wire receives for t (the whole batch, row0 = 0), by the host reference."""
    fmt = q.format(direction)
    if q.rounding_of(direction) == "stochastic":
        return S.roundtrip(t.cpu(), fmt, q.seed, counter, 0).to(t.device)
    return R.roundtrip(t.cpu(), fmt).to(t.device)


def _key(r):
    return repr(r)


@pytest.fixture(scope="module")
def hand(gpu):
    """Two hand-composed steps on the SAME batch per rounding: client.forward, the reference's rounding of the cut
    under the client's counter, server.step_request, the reference's rounding of dcut under the server's counter of
    this step (read before step_request ticks it), client.backward_step."""
    from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
    out = {}
    x, y = _batches(gpu)[0]
    for rounding in ROUNDINGS + ["nearest"]:
        q = _codec(rounding)
        a, b = init_wide_models(seed=0)
        c, s = WideClientStage(a, device=gpu), WideServerStage(b, device=gpu, seed=0)
        wire, states = [], []
        for k in range(2):
            assert int(c.step_ctr.item()) == k and int(s.step_ctr.item()) == k
            cut_q = _host(c.forward(x), q, "fwd", k)
            dcut, _ = s.step_request(cut_q, y)
            raw = dcut.clone()
            dcut_q = _host(raw, q, "bwd", k)
            c.backward_step(dcut_q)
            wire.append((cut_q.clone(), raw, dcut_q.clone()))
            states.append(_state(c, s))
        out[_key(rounding)] = {"states": states, "losses": _losses(s.loss_log), "wire": wire}
    return out


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("rounding", ROUNDINGS, ids=["bwd", "both"])
def test_fused_step_is_the_hand_composed_step(gpu, hand, rounding, graph):
    tr = _trainer(gpu, rounding, graph)
    want = hand[_key(rounding)]
    x, y = _batches(gpu)[0]
    for k in range(2):
        tr.step(x, y)
        cut_q, _, dcut_q = want["wire"][k]
        assert torch.equal(tr.server._b("cut_q", CUT, torch.bfloat16).view(torch.int16), cut_q.view(torch.int16))
        assert torch.equal(tr.server._b("dcut", CUT, torch.bfloat16).view(torch.int16), dcut_q.view(torch.int16))
        assert _same(_state(tr.client, tr.server), want["states"][k])
    assert _losses(tr.loss_log) == want["losses"]
    # stochastic rounding is visible: the nearest codec's step ends elsewhere
    assert not torch.equal(want["states"][0][0], hand[_key("nearest")]["states"][0][0])


def test_consecutive_steps_use_different_words(hand):
    """Same batch twice: the second step's wire gradient is the reference at counter 1, not 0."""
    q = _codec({"bwd": "stochastic"})
    w = hand[_key({"bwd": "stochastic"})]["wire"]
    raw = w[1][1]
    at0, at1 = _host(raw, q, "bwd", 0), _host(raw, q, "bwd", 1)
    assert torch.equal(w[1][2].view(torch.int16), at1.view(torch.int16))
    assert not torch.equal(at0.view(torch.int16), at1.view(torch.int16))


@pytest.mark.parametrize("rounding", ROUNDINGS, ids=["bwd", "both"])
def test_optimizer_state_reproduces_the_next_step(gpu, hand, rounding):
    x, y = _batches(gpu)[0]
    one = _trainer(gpu, rounding, True)
    one.step(x, y)
    state = {k: v.clone() for k, v in one.optimizer_state().items()}
    params = (one.client.params.clone(), one.server.params.clone())
    fresh = _trainer(gpu, rounding, True)
    fresh.client.params.copy_(params[0])
    fresh.server.params.copy_(params[1])
    fresh._state_written()
    fresh.load_optimizer_state(state)
    one.step(x, y)
    fresh.step(x, y)
    assert _same(_state(one.client, one.server), hand[_key(rounding)]["states"][1])
    got, want = _state(fresh.client, fresh.server), _state(one.client, one.server)
    assert _same(got, want)


@pytest.mark.parametrize("graph", [False, True])
def test_evaluation_rounds_to_nearest(gpu, graph):
    (x0, y0), (x1, y1) = _batches(gpu)
    tr, two = _trainer(gpu, "stochastic", graph), _trainer(gpu, "stochastic", graph)
    near = _trainer(gpu, "nearest", graph)
    tr.step(x0, y0)
    two.step(x0, y0)
    for dst, src in ((near.client, tr.client), (near.server, tr.server)):
        dst.params.copy_(src.params)
    near._state_written()
    before = _state(tr.client, tr.server)
    p, l = (t.clone() for t in tr.eval_batch(x1, y1))
    logits = tr.server.eval_logits.clone()
    pn, ln = near.eval_batch(x1, y1)
    assert torch.equal(p, pn) and torch.equal(l, ln) and torch.equal(logits, near.server.eval_logits)
    pp, lg = tr.predict(x1, return_logits=True)
    ppn, lgn = near.predict(x1, return_logits=True)
    assert torch.equal(pp, ppn) and torch.equal(lg, lgn)
    ra, rb = tr.evaluate([(x1, y1)]), near.evaluate([(x1, y1)])
    assert (ra.n, ra.correct, ra.loss) == (rb.n, rb.correct, rb.loss)
    # a pure function of the weights: again, the same bits; and no training state moved
    p2, l2 = tr.eval_batch(x1, y1)
    assert torch.equal(p2, p) and torch.equal(l2, l)
    assert _same(_state(tr.client, tr.server), before)
    # step, evaluate, step == step, step
    tr.step(x1, y1)
    two.step(x1, y1)
    assert _same(_state(tr.client, tr.server), _state(two.client, two.server))
    assert _losses(tr.loss_log) == _losses(two.loss_log)


@pytest.mark.parametrize("graph", [False, True])
def test_default_rounding_is_the_nearest_codecs_step(gpu, hand, graph):
    from splitcnn.codec import Fp8Cut
    from splitcnn.wide import WideTrainer, init_wide_models
    x, y = _batches(gpu)[0]
    plain = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=Fp8Cut())
    named = _trainer(gpu, "nearest", graph)
    for k in range(2):
        plain.step(x, y)
        named.step(x, y)
        assert _same(_state(plain.client, plain.server), _state(named.client, named.server))
        assert _same(_state(plain.client, plain.server), hand[_key("nearest")]["states"][k])
