"""optim.EMA wired into engine.SplitTrainer (K2) and wide.WideTrainer (K5), B = 8: every step's averaged blocks are the
float64 closed form of tests/ema_ref.py stepped from the device's own values, within the derived bound (a bitwise copy
before `start`); training with ema= is bitwise training without it, under every recipe; graph replays equal eager steps
bit for bit with the averaged blocks included, batch sizes alternate on one trainer and set_decay reaches a captured
graph; evaluation on the averaged weights touches nothing, equals the live evaluation before `start` and afterwards the
live prediction of a fresh trainer loaded from ema_state_dict(); saved state resumes bit for bit; and every path that
cannot keep the average refuses it."""
import numpy as np
import pytest
import torch

import ema_ref as R
from splitcnn import optim

pytestmark = pytest.mark.gpu

B = 8
WHICH = ["k2", "k5"]
RECIPES = ["k2", "k2-lars", "k2-clip", "k5", "k5-lamb", "k5-clip"]


def make(recipe, gpu, ema=None, seed=None, plain_default=False, **kw):
    """A trainer under `recipe`. "k2" / "k5" with ema= are the default recipe plus the average; without ema= "k2" is
    the equivalent explicit optim.SGD(0.01) (plain_default: the by-value default), "k5" the default Adam."""
    which, _, extra = recipe.partition("-")
    if extra == "clip":
        kw["clip"] = optim.ClipNorm(0.5, device=gpu)
    if which == "k2":
        from splitcnn.data import init_models
        from splitcnn.engine import SplitTrainer
        cfg = {"": None if (ema is not None or plain_default) else optim.SGD(0.01),
               "lars": optim.LARS(0.05, momentum=0.9, nesterov=True, weight_decay=5e-4),
               "clip": optim.SGD(0.05, momentum=0.9, weight_decay=5e-4)}[extra]
        return SplitTrainer(*init_models(seed=3 if seed is None else seed), device=gpu, optim=cfg, ema=ema, **kw)
    from splitcnn.wide import WideTrainer, init_wide_models
    cfg = {"": None, "lamb": optim.LAMB(1e-3), "clip": optim.Adam(1e-3, weight_decay=0.01)}[extra]
    return WideTrainer(*init_wide_models(seed=0 if seed is None else seed), device=gpu, optim=cfg, ema=ema, **kw)


def batches(which, gpu, sizes):
    if which.startswith("k2"):
        from splitcnn.data import SyntheticMNIST
        data = SyntheticMNIST(7)
    else:
        from splitcnn.wide import SyntheticCIFAR
        data = SyntheticCIFAR(9)
    return [tuple(t.to(gpu) for t in data.batch(b)) for b in sizes]


def train_state(tr):
    """What training writes, without the averaged blocks (the loss log is compared through losses())."""
    c, s = tr.client, tr.server
    out = [c.params, s.params, c.grads, s.grads]
    out += [t for k, t in sorted(tr._optim_state().items()) if not k.endswith(".ema")]
    return [t.clone() for t in out]


def state(tr):
    return train_state(tr) + [tr.client.ema.clone(), tr.server.ema.clone()]


def losses(tr):
    torch.cuda.synchronize()
    return [l for _, l in tr.loss_log.flush()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _np(t):
    return t.detach().cpu().numpy()


def counters(tr):
    return [int(st.step_ctr.item()) for st in (tr.client, tr.server)]


# ------------------------------------------------------------------ the rule, per step
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_every_step_is_the_closed_form(gpu, which, graph):
    cfg = optim.EMA(0.99, warmup=True, start=2, device=gpu)
    tr = make(which, gpu, ema=cfg, graph=graph)
    stages = (tr.client, tr.server)
    for st in stages:
        assert torch.equal(st.ema, st.params) and st.ema.data_ptr() != st.params.data_ptr()
    for k, (x, y) in enumerate(batches(which, gpu, [B] * 6)):
        before = [_np(st.ema).copy() for st in stages]
        p_before = [_np(st.params).copy() for st in stages]
        assert counters(tr) == [k, k]
        tr.step(x, y)
        torch.cuda.synchronize()
        for st, e0, p0 in zip(stages, before, p_before):
            p, e = _np(st.params), _np(st.ema)
            assert not np.array_equal(p, p0), "the parameters did not move"
            if k < 2:
                assert e.tobytes() == p.tobytes(), (type(st).__name__, k)
            else:
                assert R.within(e, e0, p, k, 2, 0.99, True), (type(st).__name__, k)
                assert not np.array_equal(e, e0) and not np.array_equal(e, p)
                wrong = R.step64(e0, p, k, 2, 0.99, True, variant="n_is_t")
                assert (np.abs(e - wrong) > R.bound(e0, p, k, 2, 0.99, True)).any(), "n = t is told apart"
    assert counters(tr) == [6, 6]


@pytest.mark.parametrize("which", WHICH)
def test_separate_and_flat_gradient_paths_keep_the_average(gpu, which):
    """The stepping paths the fused trainers do not take — K2 step() on each stage with its own counter, K5
    finish_step() / step_from_grads() — launch the update between their optimizer launch and their tick."""
    cfg = optim.EMA(0.9, warmup=True, start=1, device=gpu)
    if which == "k2":
        from splitcnn.data import init_models
        from splitcnn.engine import ClientStage, ServerStage
        a, b = init_models(seed=3)
        c, s = ClientStage(a, device=gpu, ema=cfg), ServerStage(b, device=gpu, ema=cfg)
        c.emit_amax = True
    else:
        from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
        a, b = init_wide_models(seed=0)
        c, s = WideClientStage(a, device=gpu, ema=cfg), WideServerStage(b, device=gpu, ema=cfg)
    assert c.step_ctr is not s.step_ctr
    for k, (x, y) in enumerate(batches(which, gpu, [B] * 3)):
        before = [(_np(st.ema).copy(), _np(st.params).copy()) for st in (c, s)]
        if which == "k2":
            act = c.forward(x)
            cut_grad, loss_i = s.compute(act, y, 1.0 / B, act_amax=c._act_amax)
            s.step()
            c.backward(cut_grad)
            c.step()
        else:
            dcut = s.accumulate(c.forward(x), y, 1.0 / B, 0, 0, 1)
            s.finish_step(1)
            c.backward_grads(dcut)
            c.step_from_grads()
        torch.cuda.synchronize()
        assert [int(st.step_ctr.item()) for st in (c, s)] == [k + 1, k + 1]
        for st, (e0, p0) in zip((c, s), before):
            p, e = _np(st.params), _np(st.ema)
            assert not np.array_equal(p, p0)
            if k < 1:
                assert e.tobytes() == p.tobytes()
            else:
                assert R.within(e, e0, p, k, 1, 0.9, True) and not np.array_equal(e, e0), (type(st).__name__, k)
    # the slab paths of the stages alone: backward_step / step_request tick their own counters
    x, y = batches(which, gpu, [B])[0]
    before = [_np(st.ema).copy() for st in (c, s)]
    if which == "k2":
        cut_grad, _ = s.step_request(c.forward(x), y, act_amax=c._act_amax)
    else:
        cut_grad, _ = s.step_request(c.forward(x), y)
    c.backward_step(cut_grad)
    torch.cuda.synchronize()
    assert [int(st.step_ctr.item()) for st in (c, s)] == [4, 4]
    for st, e0 in zip((c, s), before):
        assert R.within(_np(st.ema), e0, _np(st.params), 3, 1, 0.9, True), type(st).__name__
        assert not np.array_equal(_np(st.ema), e0)


# ------------------------------------------------------------------ training is unchanged
@pytest.mark.parametrize("recipe", RECIPES)
def test_training_with_ema_is_bitwise_training_without(gpu, recipe):
    bs = batches(recipe, gpu, [B] * 6)
    res = []
    for ema in (None, optim.EMA(0.9, start=1, device=gpu)):
        tr = make(recipe, gpu, ema=ema)
        for x, y in bs:
            tr.step(x, y)
        torch.cuda.synchronize()
        pred, logits = tr.predict(bs[0][0], return_logits=True)   # live evaluation does not move with ema= on
        res.append((train_state(tr), losses(tr), counters(tr), pred, logits, set(tr.optimizer_state())))
        if ema is not None:
            assert not torch.equal(tr.client.ema, tr.client.params) and not torch.equal(tr.server.ema, tr.server.params)
    (s0, l0, c0, p0, g0, k0), (s1, l1, c1, p1, g1, k1) = res
    assert same(s0, s1) and l0 == l1 and len(l0) == 6 and c0 == c1 == [6, 6]
    assert torch.equal(p0, p1) and torch.equal(g0, g1)
    assert k1 == k0 | {"client.ema", "server.ema"} and not any(k.endswith(".ema") for k in k0)


def test_k2_ema_alone_selects_the_configured_default(gpu):
    """ema= without optim= runs the configured kernels at optim.SGD(0.01); a trainer with neither keeps the by-value
    default and owns no block and no counter."""
    tr = make("k2", gpu, ema=optim.EMA(device=gpu))
    assert isinstance(tr.client.optim, optim.SGD) and tr.client.optim.lr == 0.01 and tr.client.optim.momentum == 0.0
    assert tr.client.step_ctr is tr.server.step_ctr and tr.client.ema_cfg is tr.server.ema_cfg
    plain = make("k2", gpu, plain_default=True)
    assert plain.client.optim is None and plain.client.ema is None and plain.server.ema is None
    assert plain.optimizer_state() == {}


# ------------------------------------------------------------------ graphs, batch sizes, set_decay
@pytest.mark.parametrize("which", WHICH)
def test_graph_replays_equal_eager_steps_with_alternating_batch_sizes(gpu, which):
    bs = batches(which, gpu, [8, 5, 8, 5, 8, 5])
    res = []
    for graph in (False, True):
        tr = make(which, gpu, ema=optim.EMA(0.9, start=1, device=gpu), graph=graph)
        for x, y in bs:
            tr.step(x, y)
        torch.cuda.synchronize()
        res.append((state(tr), losses(tr)))
        if graph:
            assert sorted(k for k in tr._graphs if isinstance(k, int)) == [5, 8]
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@pytest.mark.parametrize("which", WHICH)
def test_set_decay_reaches_a_captured_graph(gpu, which):
    cfg = optim.EMA(0.99, warmup=False, device=gpu)
    tr = make(which, gpu, ema=cfg, graph=True)
    bs = batches(which, gpu, [B] * 4)
    tr.step(*bs[0])
    tr.step(*bs[1])
    n_graphs = len(tr._graphs)
    for k, decay in ((2, 0.99), (3, 0.5)):
        cfg.set_decay(decay)
        before = [_np(st.ema).copy() for st in (tr.client, tr.server)]
        tr.step(*bs[k])
        torch.cuda.synchronize()
        for st, e0 in zip((tr.client, tr.server), before):
            assert R.within(_np(st.ema), e0, _np(st.params), k, 0, decay, False), (type(st).__name__, decay)
            assert not R.within(_np(st.ema), e0, _np(st.params), k, 0, 1.49 - decay, False)
    assert len(tr._graphs) == n_graphs, "no recapture"


# ------------------------------------------------------------------ evaluation on the average
@pytest.mark.parametrize("which", WHICH)
def test_step_evaluate_on_ema_step_equals_step_step(gpu, which):
    bs = batches(which, gpu, [B] * 3)
    res = []
    for evaluate in (False, True):
        tr = make(which, gpu, ema=optim.EMA(0.9, device=gpu))
        tr.step(*bs[0])
        if evaluate:
            tr.evaluate([bs[2]], weights="ema")
            tr.eval_batch(*bs[2], weights="ema")
            tr.predict(bs[2][0], weights="ema")
            tr.evaluate([bs[2]])
        tr.step(*bs[1])
        res.append((state(tr), losses(tr), tr.global_step))
    assert same(res[0][0], res[1][0]) and res[0][1:] == res[1][1:]


@pytest.mark.parametrize("which", WHICH)
def test_evaluation_before_start_is_the_live_evaluation(gpu, which):
    tr = make(which, gpu, ema=optim.EMA(0.9, start=10, device=gpu))
    bs = batches(which, gpu, [B] * 3)
    tr.step(*bs[0])
    tr.step(*bs[1])
    out = {}
    for w in ("live", "ema"):
        r = tr.evaluate([bs[2], bs[0]], weights=w)
        pred, loss_i = tr.eval_batch(*bs[2], weights=w)
        out[w] = (r.loss, r.n, r.correct, r.confusion.copy(), pred.clone(), loss_i.clone(), tr.server.eval_logits.clone(),
                  tr.predict(bs[2][0], return_logits=True, weights=w))
    a, b = out["live"], out["ema"]
    assert a[:3] == b[:3] and a[1] == 2 * B and np.array_equal(a[3], b[3])
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])
    assert torch.equal(a[7][0], b[7][0]) and torch.equal(a[7][1], b[7][1]) and torch.equal(a[6], a[7][1])
    assert list(tr._eval_graphs) == [B, (B, "ema")] and tr._eval_graphs[B]["graph"] is not tr._eval_graphs[B, "ema"]["graph"]


@pytest.mark.parametrize("which", WHICH)
def test_prediction_on_ema_is_a_fresh_trainer_loaded_from_ema_state_dict(gpu, which):
    """After `start` the averaged pass is bitwise the live pass of a fresh trainer whose modules hold
    ema_state_dict() — on K5 this needs the bf16 shadows rebuilt inside the pass to be current. Twice, with a training
    step in between, through predict (eager) and through eval_batch (the pass's graph)."""
    tr = make(which, gpu, ema=optim.EMA(0.5, warmup=False, device=gpu))
    bs = batches(which, gpu, [B] * 5)
    x, y = bs[4]
    for x_, y_ in bs[:3]:
        tr.step(x_, y_)
    seen = []
    for extra in (None, bs[3]):
        if extra is not None:
            tr.step(*extra)
        sd = tr.ema_state_dict()
        for name, st in (("client", tr.client), ("server", tr.server)):
            own = st.model.state_dict()
            assert list(sd[name]) == list(own) and all(sd[name][k].shape == own[k].shape for k in own)
            assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd[name].values())
            flat = torch.cat([sd[name][k].reshape(-1) for k in st.TENSORS])
            assert torch.equal(flat, st.ema.cpu()) and not torch.equal(flat, st.params.cpu())
        fresh = make(which, gpu, plain_default=True, seed=11, graph=False)
        fresh.client.model.load_state_dict(sd["client"])
        fresh.server.model.load_state_dict(sd["server"])
        fresh._state_written()
        want_pred, want_logits = fresh.predict(x, return_logits=True)
        pred, logits = tr.predict(x, return_logits=True, weights="ema")
        assert torch.equal(logits, want_logits) and torch.equal(pred, want_pred)
        gpred, gloss = tr.eval_batch(x, y, weights="ema")        # the captured pass replays on the current average
        fpred, floss = fresh.eval_batch(x, y)
        assert torch.equal(tr.server.eval_logits, want_logits) and torch.equal(gpred, fpred) and torch.equal(gloss, floss)
        live = tr.predict(x, return_logits=True)[1]
        assert not torch.equal(live, logits)
        seen.append(logits)
    assert not torch.equal(seen[0], seen[1])
    assert list(tr._eval_graphs) == [(B, "ema")]


# ------------------------------------------------------------------ state
@pytest.mark.parametrize("which", WHICH)
def test_resume_is_bit_for_bit_with_the_averaged_blocks(gpu, which):
    bs = batches(which, gpu, [B] * 6)
    mk = lambda seed=None: make(which, gpu, ema=optim.EMA(0.9, start=1, device=gpu), seed=seed)  # noqa: E731
    straight = mk()
    for x, y in bs:
        straight.step(x, y)
    first = mk()
    for x, y in bs[:3]:
        first.step(x, y)
    torch.cuda.synchronize()
    saved = ({k: v.cpu().clone() for k, v in first.client.model.state_dict().items()},
             {k: v.cpu().clone() for k, v in first.server.model.state_dict().items()}, first.optimizer_state())
    own = ("momentum_buffer", "step") if which == "k2" else ("exp_avg", "exp_avg_sq", "step")
    assert set(saved[2]) == {f"{s}.{k}" for s in ("client", "server") for k in own + ("ema",)}
    assert torch.equal(saved[2]["server.ema"], first.server.ema.cpu())
    second = mk(seed=5)
    second.client.model.load_state_dict(saved[0])
    second.server.model.load_state_dict(saved[1])
    second.load_optimizer_state(saved[2])
    for x, y in bs[3:]:
        second.step(x, y)
    assert same(state(straight), state(second))
    assert losses(straight)[3:] == losses(second)
    without = make(which, gpu)
    with pytest.raises(ValueError, match="expected keys"):
        without.load_optimizer_state(saved[2])


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("which", WHICH)
def test_trainer_refusals(gpu, which):
    tr = make(which, gpu, plain_default=True)
    x, y = batches(which, gpu, [B])[0]
    with pytest.raises(RuntimeError, match="ema="):
        tr.evaluate([(x, y)], weights="ema")
    with pytest.raises(RuntimeError, match="ema="):
        tr.eval_batch(x, y, weights="ema")
    with pytest.raises(RuntimeError, match="ema="):
        tr.predict(x, weights="ema")
    with pytest.raises(RuntimeError, match="ema="):
        tr.ema_state_dict()
    for has in (tr, make(which, gpu, ema=optim.EMA(device=gpu))):
        for bad in ("EMA", "averaged", ""):
            with pytest.raises(ValueError, match="weights"):
                has.evaluate([(x, y)], weights=bad)
            with pytest.raises(ValueError, match="weights"):
                has.eval_batch(x, y, weights=bad)
            with pytest.raises(ValueError, match="weights"):
                has.predict(x, weights=bad)
    assert tr._eval_graphs == {}
    with pytest.raises(TypeError, match="ema"):
        make(which, gpu, ema=0.999)


def test_dist_ushaped_and_federated_paths_refuse_a_stage_with_ema(gpu):
    """The multi-GPU classes, the U-shaped exchange and the federated round do not launch the update: a stage that
    carries an averaged block is refused at construction, before anything runs."""
    from splitcnn import dist
    from splitcnn.engine import ClientStage, ServerStage
    from splitcnn.wide import WideClientStage, WideServerStage
    cfg = optim.EMA(device=gpu)
    c, s = ClientStage(device=gpu, ema=cfg), ServerStage(device=gpu, ema=cfg)
    w, ws = WideClientStage(device=gpu, ema=cfg), WideServerStage(device=gpu, ema=cfg)
    assert w.optim is None and ws.optim is None, "the K5 default Adam path keeps its launches"
    before = [t.params.clone() for t in (c, s, w, ws)]
    for make_it in (lambda: dist.Replicated(c, s), lambda: dist.FedAvg(c, s), lambda: dist.UShaped(c, "client", 1),
                    lambda: dist.Hub(c, 0, 2), lambda: dist.Pipeline(s, "server", 0), lambda: dist.WideHub(w, 0, 2),
                    lambda: dist.WideHub(ws, 1, 2), lambda: dist.Replicated(ClientStage(device=gpu), s)):
        with pytest.raises(ValueError, match="ema="):
            make_it()
    assert all(torch.equal(t.params, b) and torch.equal(t.ema, b) for t, b in zip((c, s, w, ws), before))
