"""wide.WideTrainer(cut_codec=codec.MxCut(...)), B = 8, one and three steps: the fused step — eager and as a captured
graph — is bit for bit the hand-composed one on the stages (client.forward, MxCut.roundtrip, server.step_request,
roundtrip in place, client.backward_step; the kernel itself is held to the host reference in test_cutmx_gpu.py);
evaluation and prediction quantise the cut the same way on live and averaged weights and touch no training state; the
codec combines with cut_noise= and with optim= + clip= + loss=; the step's launches are the default step's plus the two
slk_cutmx_roundtrip launches at the documented places."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, STEPS = 8, 3
CUT = (B, 32, 8, 8, 8)
FORMATS = [("e2m1", "e4m3"), ("e2m1", None), (None, "e2m1")]


def _batches(gpu, n=STEPS):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(23)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def _codec(fwd, bwd):
    from splitcnn.codec import MxCut
    return MxCut(fwd=fwd, bwd=bwd) if (fwd or bwd) else None


def _trainer(gpu, fwd, bwd, graph, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=_codec(fwd, bwd), **kw)


def _state(c, s):
    return [t.clone() for t in (c.params, c.m, c.v, c.step_ctr, c.grads, s.params, s.m, s.v, s.step_ctr, s.grads)]


def _losses(log):
    torch.cuda.synchronize()
    return [l for _, l in log.flush()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _i16(t):
    return t.view(torch.int16)


def _stages(gpu, optim=None, clip=None, loss=None, ema=None):
    """The two stages as WideTrainer builds them."""
    from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
    a, b = init_wide_models(seed=0)
    c = WideClientStage(a, gpu, optim=optim, clip=clip, ema=ema)
    s = WideServerStage(b, gpu, seed=0, optim=c.optim, schedule=c.schedule, clip=c.clip, loss=loss, ema=c.ema_cfg)
    return c, s


def _hand(gpu, fwd, bwd, noise=None, **kw):
    """STEPS hand-composed steps: per step the state after it and what crossed the wire."""
    q = _codec(fwd, bwd)
    c, s = _stages(gpu, **kw)
    wire, states = [], []
    for x, y in _batches(gpu):
        cut = c.forward(x)
        raw = cut.clone()
        stats = torch.zeros(B, 2, device=gpu)
        if noise is not None:
            cut = noise.apply(cut, torch.empty_like(cut), c.step_ctr, row0=0, stats=stats)
        if fwd is not None:
            cut = q.roundtrip(cut, torch.empty_like(cut), "fwd")
        dcut, _ = s.step_request(cut, y)
        if bwd is not None:
            q.roundtrip(dcut, dcut, "bwd")
        if noise is not None:
            noise.scale_rows(dcut, stats, dcut)
        c.backward_step(dcut)
        wire.append((raw, cut.clone(), dcut.clone()))
        states.append(_state(c, s))
    return {"states": states, "losses": _losses(s.loss_log), "wire": wire}


@pytest.fixture(scope="module")
def hand(gpu):
    return {fb: _hand(gpu, *fb) for fb in FORMATS + [(None, None)]}


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fwd,bwd", FORMATS)
def test_fused_step_is_the_hand_composed_step(gpu, hand, fwd, bwd, graph):
    tr = _trainer(gpu, fwd, bwd, graph)
    want = hand[fwd, bwd]
    for k, (x, y) in enumerate(_batches(gpu)):
        tr.step(x, y)
        raw, cut_q, dcut_q = want["wire"][k]
        assert torch.equal(_i16(tr.client._b("cut", CUT, torch.bfloat16)), _i16(raw))
        if fwd is not None:   # what the head read
            assert torch.equal(_i16(tr.server._b("cut_q", CUT, torch.bfloat16)), _i16(cut_q))
            assert not torch.equal(_i16(cut_q), _i16(raw))
        # what the client back-propagated, where the step left it
        assert torch.equal(_i16(tr.server._b("dcut", CUT, torch.bfloat16)), _i16(dcut_q))
        assert _same(_state(tr.client, tr.server), want["states"][k]), k   # after one step, and after three
    assert _losses(tr.loss_log) == want["losses"] and len(want["losses"]) == STEPS
    # the codec is not a no-op, and a dense direction keeps its bits
    plain = hand[None, None]
    assert not torch.equal(want["states"][0][0], plain["states"][0][0])
    if fwd is None:
        assert torch.equal(_i16(want["wire"][0][1]), _i16(plain["wire"][0][1]))
        assert not torch.equal(_i16(want["wire"][0][2]), _i16(plain["wire"][0][2]))
    if bwd is None:
        assert torch.equal(want["states"][0][5], hand["e2m1", "e4m3"]["states"][0][5])   # the same head step


@pytest.mark.parametrize("graph", [False, True])
def test_evaluation_quantises_the_cut_and_touches_nothing(gpu, graph):
    from splitcnn import optim
    from splitcnn.metrics import EvalMetrics
    (x0, y0), (x1, y1), _ = _batches(gpu)
    tr = _trainer(gpu, "e2m1", "e4m3", graph, ema=optim.EMA(0.5, device=gpu))
    two = _trainer(gpu, "e2m1", "e4m3", graph, ema=optim.EMA(0.5, device=gpu))
    tr.step(x0, y0)
    two.step(x0, y0)
    before = _state(tr.client, tr.server) + [tr.client.ema.clone(), tr.server.ema.clone()]
    q = tr.cut_codec
    logits = {}
    for weights in ("live", "ema"):
        ema = weights == "ema"
        cut = tr.client.forward(x1, tag="ref", ema=ema).clone()
        m = EvalMetrics(gpu)
        pred, loss_i = tr.server.evaluate(q.roundtrip(cut, torch.empty_like(cut), "fwd"), y1, metrics=m, ema=ema)
        want_pred, want_loss, want_logits = pred.clone(), loss_i.clone(), tr.server.eval_logits.clone()
        want = m.result()
        tr.server.evaluate(cut, y1, ema=ema)
        assert not torch.equal(tr.server.eval_logits, want_logits)   # the quantisation is visible in the logits
        p, l = tr.eval_batch(x1, y1, weights=weights)
        assert torch.equal(p, want_pred) and torch.equal(l, want_loss) and torch.equal(tr.server.eval_logits, want_logits)
        assert torch.equal(_i16(tr.eval_cut), _i16(cut))             # eval_cut stays the client's own cut
        p2, lg = tr.predict(x1, return_logits=True, weights=weights)
        assert torch.equal(p2, want_pred) and torch.equal(lg, want_logits)
        res = tr.evaluate([(x1, y1)], weights=weights)
        assert (res.n, res.correct, res.loss) == (want.n, want.correct, want.loss)
        assert np.array_equal(res.confusion, want.confusion)
        logits[weights] = want_logits
    assert not torch.equal(logits["live"], logits["ema"])
    assert _same(_state(tr.client, tr.server) + [tr.client.ema, tr.server.ema], before)
    # step, evaluate, step == step, step
    tr.step(x1, y1)
    two.step(x1, y1)
    assert _same(_state(tr.client, tr.server), _state(two.client, two.server))
    assert _losses(tr.loss_log) == _losses(two.loss_log)


def _noise():
    from splitcnn.privacy import CutNoise
    return CutNoise("laplace", scale=0.3, clip=20.0, seed=9)   # the cut's norms are about 32: the bound binds


@pytest.mark.parametrize("graph", [False, True])
def test_combines_with_cut_noise_and_a_clip(gpu, graph):
    """noise, then the forward format, the head, the backward format in place, the clip's scale_rows, the client."""
    want = _hand(gpu, "e2m1", "e4m3", noise=_noise())
    tr = _trainer(gpu, "e2m1", "e4m3", graph, cut_noise=_noise())
    for k, (x, y) in enumerate(_batches(gpu)):
        tr.step(x, y)
        _, cut_q, dcut_q = want["wire"][k]
        assert torch.equal(_i16(tr.server._b("cut_q", CUT, torch.bfloat16)), _i16(cut_q))
        assert torch.equal(_i16(tr.server._b("dcut", CUT, torch.bfloat16)), _i16(dcut_q))
        assert _same(_state(tr.client, tr.server), want["states"][k])
    assert _losses(tr.loss_log) == want["losses"]
    assert (tr.cut_stats()[:, 1] < 1).any()


@pytest.mark.parametrize("graph", [False, True])
def test_combines_with_optim_clip_and_loss(gpu, graph):
    from splitcnn import optim
    from splitcnn.loss import SoftCrossEntropy
    kw = lambda: dict(optim=optim.Adam(2e-3, weight_decay=0.01), clip=optim.ClipNorm(1.0, device=gpu),  # noqa: E731
                      loss=SoftCrossEntropy(label_smoothing=0.1))
    want = _hand(gpu, "e2m1", "e4m3", **kw())
    tr = _trainer(gpu, "e2m1", "e4m3", graph, **kw())
    for k, (x, y) in enumerate(_batches(gpu)):
        tr.step(x, y)
        assert _same(_state(tr.client, tr.server), want["states"][k])
    la = _losses(tr.loss_log)
    assert la == want["losses"] and len(la) == STEPS and all(np.isfinite(la))
    tr.server.check_labels()


def _record(fn):
    """The names and by-value arguments of every _lib.call inside fn()."""
    import ctypes
    from splitcnn import _lib
    real, out = _lib.call, []

    def call(name, *args):
        types = _lib._SIGS[name]
        out.append([name] + [None if a is None else "p" if t is ctypes.c_void_p else a for t, a in zip(types, args)])
        real(name, *args)
    _lib.call = call
    try:
        fn()
    finally:
        _lib.call = real
    return out


@pytest.mark.parametrize("fwd,bwd", FORMATS)
def test_step_launches_are_the_default_steps_plus_the_roundtrips(gpu, fwd, bwd):
    x, y = _batches(gpu, 1)[0]
    plain, tr = _trainer(gpu, None, None, False), _trainer(gpu, fwd, bwd, False)
    for t in (plain, tr):
        t.step(x, y)    # the first step allocates lazily
    base = _record(lambda: plain.step(x, y))
    got = _record(lambda: tr.step(x, y))
    torch.cuda.synchronize()
    mx = [r for r in got if r[0].startswith("slk_cutmx")]
    fmt = {"e2m1": 0, "e4m3": 1}
    assert mx == [["slk_cutmx_roundtrip", "p", B, fmt[f], "p", "p"] for f in (fwd, bwd) if f is not None]
    rest = [r for r in got if not r[0].startswith("slk_cutmx")]
    assert [r[0] for r in rest] == [r[0] for r in base] and rest == base
    names = [r[0] for r in got]
    head = next(i for i, n in enumerate(names) if n.startswith("slk_wide_head"))
    if fwd is not None:      # after the client's forward, right before the head
        assert names[head - 1] == "slk_cutmx_roundtrip" and got[head - 1][3] == fmt[fwd]
        assert all(n.startswith("slk_wide_conv") or n.startswith("slk_wide_relu") for n in names[:head - 1])
    if bwd is not None:      # after the head, before the client's first backward launch
        first_bwd = next(i for i, n in enumerate(names) if i > head and n.startswith("slk_wide_conv"))
        later = [i for i, r in enumerate(got) if i > head and r[0] == "slk_cutmx_roundtrip"]
        assert len(later) == 1 and later[0] < first_bwd and got[later[0]][3] == fmt[bwd]
        assert got[later[0]][1] == got[later[0]][4] == "p"   # in place: x and out are both pointers (the dcut buffer)


def test_refuses_a_foreign_codec(gpu):
    from splitcnn.wide import WideTrainer
    with pytest.raises(TypeError, match="MxCut"):
        WideTrainer(device=gpu, graph=False, cut_codec="e2m1")
    with pytest.raises(TypeError, match="MxCut"):
        WideTrainer(device=gpu, graph=False, cut_codec=object())
