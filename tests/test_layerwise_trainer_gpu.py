"""optim.LARS wired into engine.SplitTrainer (K2) and optim.LAMB into wide.WideTrainer (K5), B = 8.

Every step's update is the float64 closed form of tests/layerwise_ref.py stepped from the trainer's own reduced gradient
and the device state before the step (norms and ratios within the derived bounds, parameters and state within the
project's bound at the device's ratios); graph replays equal eager steps bit for bit, LRSchedule.set_lr reaches a captured
graph, batch sizes alternate on one trainer, trust_ratios() names every tensor, saved state resumes bit for bit, evaluation
in between changes nothing, and every path that cannot run the recipe refuses it."""
import numpy as np
import pytest
import torch

import layerwise_ref as L
from splitcnn import optim

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps
K2_CFG = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
K2_TABLE = [0.05, 0.1, 0.075, 0.025]
K5_TABLE = [1e-3, 2e-3, 1.5e-3, 5e-4]
B = 8


def f32(x):
    return float(np.float32(x))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


def make(which, gpu, seed=None, table=None, exclude_bias=True, **kw):
    if which == "k2":
        from splitcnn.data import init_models
        from splitcnn.engine import SplitTrainer
        sched = optim.LRSchedule.from_values(table or K2_TABLE, gpu)
        return SplitTrainer(*init_models(seed=3 if seed is None else seed), device=gpu,
                            optim=optim.LARS(0.05, exclude_bias=exclude_bias, **K2_CFG), schedule=sched, **kw)
    from splitcnn.wide import WideTrainer, init_wide_models
    sched = optim.LRSchedule.from_values(table or K5_TABLE, gpu)
    return WideTrainer(*init_wide_models(seed=0 if seed is None else seed), device=gpu,
                       optim=optim.LAMB(1e-3, exclude_bias=exclude_bias), schedule=sched, **kw)


def batches(which, gpu, sizes):
    if which == "k2":
        from splitcnn.data import SyntheticMNIST
        data = SyntheticMNIST(7)
    else:
        from splitcnn.wide import SyntheticCIFAR
        data = SyntheticCIFAR(9)
    return [tuple(t.to(gpu) for t in data.batch(b)) for b in sizes]


def state(tr):
    c, s = tr.client, tr.server
    if hasattr(c, "m"):
        out = [c.params, s.params, c.m, c.v, s.m, s.v, c.step_ctr, s.step_ctr]
    else:
        out = [c.params, s.params, c.buf, s.buf, c.step_ctr, s.step_ctr]
    return [t.clone() for t in out + [c.trust_out, s.trust_out]]


def losses(tr):
    torch.cuda.synchronize()
    return [l for _, l in tr.loss_log.flush()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def pairs(st):
    """(lo, hi, nw) of a stage's [weight | bias] pairs."""
    return list(st.PAIRS)


WHICH = ["k2", "k5"]


# ------------------------------------------------------------------ the update, per step
@pytest.mark.parametrize("exclude_bias", [True, False])
def test_k2_lars_matches_float64_per_step(gpu, exclude_bias):
    tr = make("k2", gpu, graph=False, exclude_bias=exclude_bias)
    cfg = dict(momentum=f32(0.9), nesterov=True, weight_decay=f32(5e-4), trust_coef=f32(1e-3), eps=f32(1e-8))
    for k, (x, y) in enumerate(batches("k2", gpu, [B] * 4)):
        before = [(_np(st.params), _np(st.buf)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        torch.cuda.synchronize()
        lr = float(tr.client.schedule.lr_at(k))
        for st, (p0, b0) in zip((tr.client, tr.server), before):
            g, rows = _np(st.grads), st.trust_out.cpu().numpy()
            assert len(st.trust_nblk) == len(st.PAIRS)
            for j, (lo, hi, nw) in enumerate(pairs(st)):
                nb = st.trust_nblk[j]
                wp, wb, want = L.lars_step64(p0[lo:hi], g[lo:hi], b0[lo:hi], k, lr, nw, exclude_bias=exclude_bias,
                                             ratios=(rows[2 * j][2], rows[2 * j + 1][2]), **cfg)
                ref = L.lars_step64(p0[lo:hi], g[lo:hi], b0[lo:hi], k, lr, nw, exclude_bias=exclude_bias, **cfg)[2]
                for t in (0, 1):
                    got, (wn, gn, r) = rows[2 * j + t], ref[t]
                    bn = L.norm_bound(nb, ref_terms=hi - lo)
                    assert abs(got[0] - wn) <= bn * wn and abs(got[1] - gn) <= bn * gn, (type(st).__name__, j, t, k)
                    if t == 1 and exclude_bias:
                        assert got[2] == 1.0
                    else:
                        assert abs(got[2] - r) <= L.lars_ratio_bound(nb, ref_terms=hi - lo) * r, (j, t, k, got[2], r)
                        assert got[2] != 1.0
                assert within(_np(st.params)[lo:hi], wp, p0[lo:hi]), (type(st).__name__, j, k)
                assert within(_np(st.buf)[lo:hi], wb, b0[lo:hi]), (type(st).__name__, j, k)
    assert int(tr.server.step_ctr.item()) == 4 and tr.client.step_ctr is tr.server.step_ctr


def test_k5_lamb_matches_float64_per_step(gpu):
    tr = make("k5", gpu, graph=False)
    hyp = (f32(0.9), f32(0.999), f32(1e-6))
    wd = f32(0.01)
    for k, (x, y) in enumerate(batches("k5", gpu, [B] * 3)):
        before = [(_np(st.params), _np(st.m), _np(st.v)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        torch.cuda.synchronize()
        lr = float(tr.client.schedule.lr_at(k))
        for st, (p0, m0, v0) in zip((tr.client, tr.server), before):
            g, rows = _np(st.grads), st.trust_out.cpu().numpy()
            for j, (lo, hi, nw) in enumerate(pairs(st)):
                nb, s = st.trust_nblk[j], slice(lo, hi)
                wp, wm, wv, ref = L.lamb_step64(p0[s], g[s], m0[s], v0[s], k, lr, nw, *hyp, weight_decay=wd,
                                                ratios=(rows[2 * j][2], 1.0))
                u64, e_u = L.lamb_u_error(g[s], m0[s], v0[s], p0[s], k, *hyp, wd)
                wn, un, _ = ref[0]
                ub = L.lamb_unorm_bound(nb, u64[:nw], e_u[:nw], ref_terms=nw)
                got = rows[2 * j]
                assert abs(got[0] - wn) <= L.norm_bound(nb, ref_terms=nw) * wn, (type(st).__name__, j, k)
                assert abs(got[1] - un) <= ub * un, (type(st).__name__, j, k, got[1], un, ub)
                r = L.lamb_ratio64(wn, un)
                assert abs(got[2] - r) <= L.lamb_ratio_bound(nb, ub, ref_terms=nw) * r and got[2] != 1.0
                assert rows[2 * j + 1][2] == 1.0 and rows[2 * j + 1][1] > 0, "an excluded bias reports ratio 1"
                for what, have, want, b0 in (("p", st.params, wp, p0), ("m", st.m, wm, m0), ("v", st.v, wv, v0)):
                    assert within(_np(have)[s], want, b0[s]), (type(st).__name__, what, j, k)
    assert int(tr.server.step_ctr.item()) == 3 == int(tr.client.step_ctr.item())


# ------------------------------------------------------------------ graphs, schedule, batch sizes
@pytest.mark.parametrize("which", WHICH)
def test_graph_replay_equals_eager(gpu, which):
    bs = batches(which, gpu, [B] * 3)
    eager, graphed = make(which, gpu, graph=False), make(which, gpu, graph=True)
    for x, y in bs:
        eager.step(x, y)
        graphed.step(x, y)
    assert same(state(eager), state(graphed)) and losses(eager) == losses(graphed)
    assert not same(state(eager)[:2], state(make(which, gpu, graph=False))[:2])


@pytest.mark.parametrize("which", WHICH)
def test_set_lr_reaches_the_captured_graph(gpu, which):
    bs = batches(which, gpu, [B] * 3)
    lr0 = 0.05 if which == "k2" else 1e-3
    res = []
    for graph, change in ((True, True), (False, True), (True, False)):
        tr = make(which, gpu, graph=graph, table=[lr0])
        tr.step(*bs[0])
        if change:
            tr.client.schedule.set_lr(lr0 / 4)
        tr.step(*bs[1])
        tr.step(*bs[2])
        res.append(state(tr))
    assert same(res[0], res[1]), "a replay runs at the rate written after the capture"
    assert not same(res[0][:2], res[2][:2])


@pytest.mark.parametrize("which", WHICH)
def test_batch_sizes_alternate_on_one_trainer(gpu, which):
    bs = batches(which, gpu, [8, 5, 8, 5])
    eager, graphed = make(which, gpu, graph=False), make(which, gpu, graph=True)
    for x, y in bs:
        eager.step(x, y)
        graphed.step(x, y)
    assert same(state(eager), state(graphed)) and losses(eager) == losses(graphed)


@pytest.mark.parametrize("which", WHICH)
def test_trust_ratios_names_every_tensor(gpu, which):
    tr = make(which, gpu)
    tr.step(*batches(which, gpu, [B])[0])
    t = tr.trust_ratios()
    names = {"k2": {"client": ["conv1.weight", "conv1.bias"],
                    "server": ["conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias"]},
             "k5": {"client": [f"conv{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")],
                    "server": ["fc.weight", "fc.bias"]}}[which]
    assert {k: list(v) for k, v in t.items()} == names
    for name, st in (("client", tr.client), ("server", tr.server)):
        assert set(names[name]) == set(st.model.state_dict())
        rows = st.trust_out.cpu().numpy()
        for j, n in enumerate(names[name]):
            assert t[name][n] == tuple(float(v) for v in rows[j])
            wn, xn, r = t[name][n]
            assert wn > 0 and xn > 0 and ((r == 1.0) if n.endswith("bias") else (0 < r != 1.0)), (n, t[name][n])
            if n.endswith("weight"):     # a weight moves by lr * ratio * |d| << |w| in one step: the same norm to 1e-2
                want = L.norm64(_np(st.model.state_dict()[n]))
                assert abs(wn - want) <= 1e-2 * want
    from splitcnn.engine import SplitTrainer
    from splitcnn.data import init_models
    with pytest.raises(RuntimeError, match="LARS"):
        SplitTrainer(*init_models(seed=3), device=gpu, optim=optim.SGD(0.01)).trust_ratios()


# ------------------------------------------------------------------ every stepping method of a stage runs the recipe
def _close_to(flat, ref, before):
    """Two paths that sum the same gradient but cut their partials differently: each ratio lies within the derived
    bound (3e-6) of the exact one, so the steps differ by at most 2 bounds of the step, 1e-5 here, plus rounding."""
    tol = 1e-5 * np.abs(ref - before).max() + 2 * EPS32 * np.abs(ref)
    return bool((np.abs(flat - ref) <= tol).all())


@pytest.mark.parametrize("which", WHICH)
def test_separate_and_flat_gradient_paths_run_the_recipe(gpu, which):
    """K2 without the fused client backward (each stage its own pair of launches), and the flat-gradient paths of both
    models (gradient reduced into `grads`, then step() / step_from_grads() / finish_step(): the whole block in place,
    one slice per [weight | bias] pair): the same gradients bit for bit, every tensor's ratio and the parameters equal to
    the trainer's step up to the partials' different cut; an excluded bias stays at ratio 1."""
    from splitcnn import ops
    x, y = batches(which, gpu, [B])[0]
    kw = dict(fuse_client_backward=False) if which == "k2" else {}
    ref, flat = make(which, gpu, graph=False, **kw), make(which, gpu, graph=False, **kw)
    before = [_np(st.params) for st in (flat.client, flat.server)]
    ref.step(x, y)
    c, s = flat.client, flat.server
    if which == "k2":
        act = c.forward(x)
        cut_grad, loss_i = s.compute(act, y, 1.0 / B, act_amax=c._act_amax, act16=c._act16 if c.emit_act16 else None)
        s.step()
        s.log_loss(loss_i)
        c.backward(cut_grad)
        c.step()
        ops.tick(s.step_ctr)
    else:
        dcut = s.accumulate(c.forward(x), y, 1.0 / B, 0, 0, 1)
        s.finish_step(1)
        c.backward_grads(dcut)
        c.step_from_grads()
    torch.cuda.synchronize()
    for st, rs, p0 in zip((c, s), (ref.client, ref.server), before):
        assert torch.equal(st.grads, rs.grads), type(st).__name__
        a, b = st.trust_out.cpu().numpy(), rs.trust_out.cpu().numpy()
        assert np.allclose(a, b, rtol=1e-5, atol=0) and (a[1::2, 2] == 1.0).all() and (a[0::2, 2] != 1.0).all()
        assert _close_to(_np(st.params), _np(rs.params), p0), type(st).__name__
        assert not np.array_equal(_np(st.params), p0)
        assert torch.equal(st.step_ctr, rs.step_ctr)


# ------------------------------------------------------------------ evaluation, resume
@pytest.mark.parametrize("which", WHICH)
def test_step_evaluate_step_equals_step_step(gpu, which):
    bs = batches(which, gpu, [B] * 3)
    res = []
    for evaluate in (False, True):
        tr = make(which, gpu)
        tr.step(*bs[0])
        if evaluate:
            tr.eval_batch(*bs[2])
        tr.step(*bs[1])
        res.append((state(tr), losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@pytest.mark.parametrize("which", WHICH)
def test_resume_is_bit_for_bit_and_keys_are_unchanged(gpu, which):
    bs = batches(which, gpu, [B] * 4)
    straight = make(which, gpu)
    for x, y in bs:
        straight.step(x, y)
    first = make(which, gpu)
    for x, y in bs[:2]:
        first.step(x, y)
    torch.cuda.synchronize()
    saved = ({k: v.cpu().clone() for k, v in first.client.model.state_dict().items()},
             {k: v.cpu().clone() for k, v in first.server.model.state_dict().items()}, first.optimizer_state())
    if which == "k2":
        want = {f"{s}.{k}" for s in ("client", "server") for k in ("momentum_buffer", "step")}
    else:
        want = {f"{s}.{k}" for s in ("client", "server") for k in ("exp_avg", "exp_avg_sq", "step")}
    assert set(saved[2]) == want, "trust_out is no optimizer state"
    second = make(which, gpu, seed=5)
    second.client.model.load_state_dict(saved[0])
    second.server.model.load_state_dict(saved[1])
    second.load_optimizer_state(saved[2])
    for x, y in bs[2:]:
        second.step(x, y)
    assert same(state(straight), state(second))
    assert losses(straight)[2:] == losses(second)


# ------------------------------------------------------------------ refusals
def test_constructors_validate_like_torch():
    assert isinstance(optim.LARS(0.1), optim.SGD) and isinstance(optim.LAMB(), optim.Adam)
    a, b = optim.LARS(0.1), optim.LAMB()
    assert (a.momentum, a.trust_coef, a.eps, a.exclude_bias, a.weight_decay) == (0.9, 1e-3, 1e-8, True, 0.0)
    assert (b.lr, b.betas, b.eps, b.weight_decay, b.exclude_bias) == (1e-3, (0.9, 0.999), 1e-6, 0.01, True)
    for bad in (dict(trust_coef=0.0), dict(trust_coef=-1.0), dict(trust_coef=float("nan")), dict(eps=-1e-8),
                dict(momentum=-0.1), dict(weight_decay=-1.0), dict(nesterov=True, momentum=0.0)):
        with pytest.raises(ValueError):
            optim.LARS(0.1, **bad)
    with pytest.raises(ValueError):
        optim.LARS(-0.1)
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            optim.LAMB(**bad)


def test_wrong_family_is_a_type_error(gpu):
    from splitcnn.engine import ClientStage, SplitTrainer
    from splitcnn.wide import WideClientStage, WideTrainer
    for make_it in (lambda: SplitTrainer(device=gpu, optim=optim.LAMB(1e-3)), lambda: ClientStage(device=gpu, optim=optim.LAMB()),
                    lambda: WideTrainer(device=gpu, optim=optim.LARS(0.1)), lambda: WideClientStage(device=gpu, optim=optim.LARS(0.1))):
        with pytest.raises(TypeError, match="optim"):
            make_it()


def test_clip_with_a_layerwise_config_is_refused(gpu):
    from splitcnn.engine import ServerStage, SplitTrainer
    from splitcnn.wide import WideServerStage, WideTrainer
    clip = optim.ClipNorm(1.0, device=gpu)
    for make_it in (lambda: SplitTrainer(device=gpu, optim=optim.LARS(0.1), clip=clip),
                    lambda: ServerStage(device=gpu, optim=optim.LARS(0.1), clip=clip),
                    lambda: WideTrainer(device=gpu, optim=optim.LAMB(), clip=clip),
                    lambda: WideServerStage(device=gpu, optim=optim.LAMB(), clip=clip)):
        with pytest.raises(ValueError, match="clip="):
            make_it()


def test_dist_ushaped_and_federated_paths_refuse_the_recipe(gpu):
    """The multi-GPU classes, the U-shaped exchange and the federated round step with the default optimizer only:
    a stage that carries LARS / LAMB is refused before anything runs, never stepped by plain SGD / Adam."""
    from splitcnn import dist
    from splitcnn.engine import ClientStage, ServerStage
    from splitcnn.wide import WideClientStage
    c, s = ClientStage(device=gpu, optim=optim.LARS(0.1)), ServerStage(device=gpu, optim=optim.LARS(0.1))
    w = WideClientStage(device=gpu, optim=optim.LAMB())
    before = c.params.clone()
    for make_it in (lambda: dist.Replicated(c, s), lambda: dist.FedAvg(c, s), lambda: dist.UShaped(c, "client", 1),
                    lambda: dist.Hub(c, 0, 2), lambda: dist.Pipeline(s, "server", 0), lambda: dist.WideHub(w, 0, 2)):
        with pytest.raises(ValueError, match="optimizer config"):
            make_it()
    assert torch.equal(c.params, before)


def test_a_segment_of_a_stage_with_another_recipe_is_refused(gpu):
    from splitcnn.engine import ClientStage, ServerStage
    slabs = torch.zeros(1, 320, device=gpu)
    for s_opt, c_opt in ((optim.LARS(0.1), optim.SGD(0.1, momentum=0.9)), (optim.SGD(0.1, momentum=0.9), optim.LARS(0.1))):
        server, client = ServerStage(device=gpu, optim=s_opt), ClientStage(device=gpu, optim=c_opt)
        before = client.params.clone()
        with pytest.raises(ValueError, match="layer-wise"):
            server._sgdm([client.optim_segment(slabs)], multi=True)
        assert torch.equal(client.params, before)
