"""wide.WideTrainer(cut_codec=codec.TopKCut(...)), B = 8, three steps: the fused step — eager and as a captured graph —
is bit for bit the hand-composed one on the stages (client.forward, TopKCut.roundtrip, server.step_request, roundtrip
in place, client.backward_step: straight through; the kernel itself is held to the reference in test_cuttopk_gpu.py);
evaluation and prediction sparsify the cut and touch no training state; the codec combines with cut_noise= and
optim= + clip=; the step's launches are the default step's plus the roundtrips; the hub refuses the codec."""
import pytest
import torch

from test_cutmx_trainer_gpu import B, CUT, _batches, _i16, _losses, _noise, _record, _same, _stages, _state

pytestmark = pytest.mark.gpu

KS = [(2048, None), (None, 1024), (1024, 1024)]


def _codec(fwd, bwd):
    from splitcnn.codec import TopKCut
    return TopKCut(fwd=fwd, bwd=bwd)


def _trainer(gpu, fwd, bwd, graph, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=_codec(fwd, bwd), **kw)


def _hand(gpu, fwd, bwd, noise=None, **kw):
    """Three hand-composed steps: per step the state after it and what crossed the wire."""
    q = _codec(fwd, bwd)
    c, s = _stages(gpu, **kw)
    wire, states = [], []
    for x, y in _batches(gpu):
        cut = raw = c.forward(x)
        stats = torch.zeros(B, 2, device=gpu)
        if noise is not None:
            cut = noise.apply(cut, torch.empty_like(cut), c.step_ctr, row0=0, stats=stats)
        if fwd is not None:
            cut = q.roundtrip(cut, torch.empty_like(cut), "fwd")
            assert int((cut.view(B, -1) != 0).sum(1).max()) <= fwd and not torch.equal(_i16(cut), _i16(raw))
        dcut, _ = s.step_request(cut, y)
        if bwd is not None:
            q.roundtrip(dcut, dcut, "bwd")
            assert int((dcut.view(B, -1) != 0).sum(1).max()) <= bwd
        if noise is not None:
            noise.scale_rows(dcut, stats, dcut)
        c.backward_step(dcut)
        wire.append((cut.clone(), dcut.clone()))
        states.append(_state(c, s))
    return {"states": states, "losses": _losses(s.loss_log), "wire": wire}


def _check(tr, want, gpu):
    for k, (x, y) in enumerate(_batches(gpu)):
        tr.step(x, y)
        cut_q, dcut_q = want["wire"][k]
        if tr.cut_codec.fwd is not None:   # what the head read
            assert torch.equal(_i16(tr.server._b("cut_q", CUT, torch.bfloat16)), _i16(cut_q))
        assert torch.equal(_i16(tr.server._b("dcut", CUT, torch.bfloat16)), _i16(dcut_q))
        assert _same(_state(tr.client, tr.server), want["states"][k]), k
    assert _losses(tr.loss_log) == want["losses"] and len(want["losses"]) == 3


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fwd,bwd", KS)
def test_fused_step_is_the_hand_composed_step(gpu, fwd, bwd, graph):
    _check(_trainer(gpu, fwd, bwd, graph), _hand(gpu, fwd, bwd), gpu)


@pytest.mark.parametrize("graph", [False, True])
def test_combines_with_cut_noise_optim_and_clip(gpu, graph):
    from splitcnn import optim
    kw = lambda: dict(optim=optim.Adam(2e-3, weight_decay=0.01), clip=optim.ClipNorm(1.0, device=gpu))  # noqa: E731
    _check(_trainer(gpu, 1024, 1024, graph, cut_noise=_noise(), **kw()), _hand(gpu, 1024, 1024, noise=_noise(), **kw()), gpu)


@pytest.mark.parametrize("graph", [False, True])
def test_evaluation_sparsifies_the_cut_and_touches_nothing(gpu, graph):
    (x0, y0), (x1, y1), _ = _batches(gpu)
    tr, two = _trainer(gpu, 1024, 1024, graph), _trainer(gpu, 1024, 1024, graph)
    tr.step(x0, y0)
    two.step(x0, y0)
    before = _state(tr.client, tr.server)
    cut = tr.client.forward(x1, tag="ref").clone()
    pred, loss_i = tr.server.evaluate(tr.cut_codec.roundtrip(cut, torch.empty_like(cut), "fwd"), y1)
    want = pred.clone(), loss_i.clone(), tr.server.eval_logits.clone()
    tr.server.evaluate(cut, y1)
    assert not torch.equal(tr.server.eval_logits, want[2])   # the sparsification is visible in the logits
    p, l = tr.eval_batch(x1, y1)
    assert torch.equal(p, want[0]) and torch.equal(l, want[1]) and torch.equal(tr.server.eval_logits, want[2])
    assert torch.equal(_i16(tr.eval_cut), _i16(cut))           # eval_cut stays the client's own cut
    p2, lg = tr.predict(x1, return_logits=True)
    assert torch.equal(p2, want[0]) and torch.equal(lg, want[2])
    assert _same(_state(tr.client, tr.server), before)
    tr.step(x1, y1)    # step, evaluate, step == step, step
    two.step(x1, y1)
    assert _same(_state(tr.client, tr.server), _state(two.client, two.server))
    assert _losses(tr.loss_log) == _losses(two.loss_log)


@pytest.mark.parametrize("fwd,bwd", KS)
def test_step_launches_are_the_default_steps_plus_the_roundtrips(gpu, fwd, bwd):
    from splitcnn.wide import WideTrainer, init_wide_models
    x, y = _batches(gpu, 1)[0]
    plain, tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False), _trainer(gpu, fwd, bwd, False)
    for t in (plain, tr):
        t.step(x, y)    # the first step allocates lazily
    base, got = _record(lambda: plain.step(x, y)), _record(lambda: tr.step(x, y))
    torch.cuda.synchronize()
    assert [r for r in got if not r[0].startswith("slk_cuttopk")] == base
    assert [r for r in got if r[0].startswith("slk_cuttopk")] == [
        ["slk_cuttopk_roundtrip", "p", B, k, "p", "p"] for k in (fwd, bwd) if k is not None]
    names = [r[0] for r in got]
    head = next(i for i, n in enumerate(names) if n.startswith("slk_wide_head"))
    assert (names[head - 1] == "slk_cuttopk_roundtrip") == (fwd is not None)   # right before the head
    later = [i for i, n in enumerate(names) if i > head and n == "slk_cuttopk_roundtrip"]
    first_bwd = next(i for i, n in enumerate(names) if i > head and n.startswith("slk_wide_conv"))
    assert len(later) == (bwd is not None) and all(i < first_bwd for i in later)   # before the client's backward


def test_the_hub_and_foreign_objects_are_refused(gpu):
    from splitcnn import dist
    from splitcnn.wide import WideClientStage, WideTrainer, init_wide_models
    stage = WideClientStage(init_wide_models(seed=0)[0], gpu)
    with pytest.raises(ValueError, match="the top-k cut codec has no hub form yet"):
        dist.WideHub(stage, 0, 2, codec=_codec(1024, None))
    with pytest.raises(TypeError, match="TopKCut"):
        WideTrainer(device=gpu, graph=False, cut_codec=2048)
