"""Wiring of splitcnn.optim into the trainers: engine.SplitTrainer (K2, B = 13 and 64) and wide.WideTrainer
(K5, B = 8 / 16). The schedule and LRSchedule.set_lr reach a captured graph, graph replays equal eager steps
bit for bit (momentum buffers and step counters included, so the capture's warm-up leaves no trace), every
step's update is torch's own in float64 on the gradient the stage wrote, a config with today's constants is
bitwise today's path, evaluation in between changes nothing, and saved optimizer state resumes bit for bit.

Float64 references get the f32 hyper-parameters the C ABI receives, and the bound is the project's
Adam-formula bound, as in tests/test_optim_gpu.py."""
import numpy as np
import pytest
import torch

from splitcnn import optim

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps
K2_CFG = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
K5_CFG = dict(weight_decay=0.01)
TABLE4 = [0.01, 0.02, 0.015, 0.005]


def f32(x):
    return float(np.float32(x))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True))


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


def k2(gpu, seed=3, **kw):
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    return SplitTrainer(*init_models(seed=seed), device=gpu, **kw)


def k5(gpu, seed=0, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=seed), device=gpu, **kw)


def k2_batches(gpu, sizes, seed=7):
    from splitcnn.data import SyntheticMNIST
    data = SyntheticMNIST(seed)
    return [tuple(t.to(gpu) for t in data.batch(B)) for B in sizes]


def k5_batches(gpu, sizes, seed=9):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(seed)
    return [tuple(t.to(gpu) for t in data.batch(B)) for B in sizes]


def k2_state(tr):
    out = [tr.client.params, tr.server.params]
    if tr.server.optim is not None:
        out += [tr.client.buf, tr.server.buf, tr.client.step_ctr, tr.server.step_ctr]
    return [t.clone() for t in out]


def k5_state(tr):
    c, s = tr.client, tr.server
    return [t.clone() for t in (c.params, s.params, c.m, c.v, s.m, s.v, c.step_ctr, s.step_ctr)]


def losses(tr):
    torch.cuda.synchronize()
    return [l for _, l in tr.loss_log.flush()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def replay_static(tr, x, y):
    """Step on the trainer's static graph inputs (no per-buffer graph: len(tr._graphs) stays 1)."""
    xs, ys = tr.static_inputs(x.shape[0])
    xs.copy_(x)
    ys.copy_(y)
    tr.step(xs, ys)


# ------------------------------------------------------------------ the schedule reaches the captured graph
@pytest.mark.parametrize("which,B", [("k2", 13), ("k2", 64), ("k5", 8)])
def test_schedule_reaches_the_graph(gpu, which, B):
    """graph=True, no momentum, table [0.01, 0, 0.01]: the second replay of the one captured graph leaves both
    stages' parameters bitwise unchanged, the first and the third change them. (With the rate baked in at
    capture, as without a schedule, step 2 would move the parameters.)"""
    sched = optim.LRSchedule.from_values([0.01, 0.0, 0.01], device=gpu)
    if which == "k2":
        tr, (x, y) = k2(gpu, optim=optim.SGD(0.01), schedule=sched), k2_batches(gpu, [B])[0]
    else:
        tr, (x, y) = k5(gpu, optim=optim.Adam(0.01), schedule=sched), k5_batches(gpu, [B])[0]
    snaps = [(tr.client.params.clone(), tr.server.params.clone())]
    for _ in range(3):
        replay_static(tr, x, y)
        snaps.append((tr.client.params.clone(), tr.server.params.clone()))
    torch.cuda.synchronize()
    assert len(tr._graphs) == 1
    for i in (0, 1):   # client, server
        assert not torch.equal(snaps[1][i], snaps[0][i])
        assert torch.equal(snaps[2][i], snaps[1][i])
        assert not torch.equal(snaps[3][i], snaps[2][i])
    assert int(tr.server.step_ctr.item()) == 3 and int(tr.client.step_ctr.item()) == 3


@pytest.mark.parametrize("which,B", [("k2", 13), ("k5", 8)])
def test_set_lr_reaches_the_graph_without_recapture(gpu, which, B):
    if which == "k2":
        tr, (x, y) = k2(gpu, optim=optim.SGD(0.01)), k2_batches(gpu, [B])[0]
    else:
        tr, (x, y) = k5(gpu, optim=optim.Adam(1e-3)), k5_batches(gpu, [B])[0]
    assert tr.client.schedule is tr.server.schedule and len(tr.client.schedule) == 1
    replay_static(tr, x, y)
    n_graphs = len(tr._graphs)
    p1 = (tr.client.params.clone(), tr.server.params.clone())
    tr.client.schedule.set_lr(0.0)
    replay_static(tr, x, y)
    p2 = (tr.client.params.clone(), tr.server.params.clone())
    tr.client.schedule.set_lr(0.02)
    replay_static(tr, x, y)
    p3 = (tr.client.params.clone(), tr.server.params.clone())
    torch.cuda.synchronize()
    assert len(tr._graphs) == n_graphs == 1
    assert same(p1, p2) and not torch.equal(p3[0], p2[0]) and not torch.equal(p3[1], p2[1])


# ------------------------------------------------------------------ graph == eager
def test_k2_graph_equals_eager_with_momentum_and_schedule(gpu):
    """Six steps alternating B = 64 / 32: fails if the capture's warm-up step leaks into the momentum
    buffers or leaves the step counter at 1."""
    batches = k2_batches(gpu, [64, 32, 64, 32, 64, 32])
    res = []
    for graph in (False, True):
        tr = k2(gpu, graph=graph, optim=optim.SGD(0.01, **K2_CFG), schedule=optim.LRSchedule.from_values(TABLE4, gpu))
        for x, y in batches:
            tr.step(x, y)
        res.append((k2_state(tr), losses(tr)))
    assert same(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and len(res[0][1]) == 6
    assert int(res[1][0][-1].item()) == 6 and res[1][0][2].abs().max() > 0


def test_k5_graph_equals_eager_with_adamw_and_schedule(gpu):
    batches = k5_batches(gpu, [16, 8, 16, 8, 16, 8])
    res = []
    for graph in (False, True):
        tr = k5(gpu, graph=graph, optim=optim.Adam(1e-3, **K5_CFG),
                schedule=optim.LRSchedule.from_values([1e-3, 2e-3, 1.5e-3, 5e-4], gpu))
        for x, y in batches:
            tr.step(x, y)
        res.append((k5_state(tr), losses(tr)))
    assert same(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and len(res[0][1]) == 6
    assert int(res[1][0][-1].item()) == 6 and int(res[1][0][-2].item()) == 6


# ------------------------------------------------------------------ every step's update is torch's
@pytest.mark.parametrize("B", [13, 64])
@pytest.mark.parametrize("fuse", [True, False])
def test_k2_update_matches_torch_sgd_per_step(gpu, B, fuse):
    """Eager, 5 steps: torch.optim.SGD in float64 on the state before the step and the gradient the stage
    wrote, at that step's table value (the last entry holds from step 3 on). fuse: the client's update rides
    in the server's launch (one slk_sgdm_multi_from_slabs) / the unfused client backward steps on its own."""
    sched = optim.LRSchedule.from_values(TABLE4, gpu)
    tr = k2(gpu, graph=False, fuse_client_backward=fuse, optim=optim.SGD(0.01, **K2_CFG), schedule=sched)
    assert tr.fuse_client_backward == fuse
    tcfg = dict(momentum=f32(0.9), nesterov=True, weight_decay=f32(5e-4))
    for k, (x, y) in enumerate(k2_batches(gpu, [B] * 5)):
        before = [(_np(st.params), _np(st.buf)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        assert sched.lr_at(k) == np.float32(TABLE4[min(k, 3)])
        for st, (p0, b0) in zip((tr.client, tr.server), before):
            ref = torch.nn.Parameter(_t64(p0))
            opt = torch.optim.SGD([ref], lr=float(sched.lr_at(k)), **tcfg)
            if k > 0:
                opt.state[ref]["momentum_buffer"] = _t64(b0)
            ref.grad = _t64(_np(st.grads))
            opt.step()
            assert np.abs(_np(st.grads)).max() > 0
            assert within(_np(st.params), ref.detach().numpy(), p0), (type(st).__name__, k)
            assert within(_np(st.buf), opt.state[ref]["momentum_buffer"].numpy(), b0), (type(st).__name__, k)
    assert int(tr.server.step_ctr.item()) == 5 and tr.client.step_ctr is tr.server.step_ctr


@pytest.mark.parametrize("fuse_adam", [True, False])
def test_k5_update_matches_torch_adamw_per_step(gpu, fuse_adam):
    sched = optim.LRSchedule.from_values([1e-3, 2e-3, 1.5e-3, 5e-4], gpu)
    tr = k5(gpu, graph=False, optim=optim.Adam(1e-3, **K5_CFG), schedule=sched)
    tr.client.fuse_adam = fuse_adam
    for k, (x, y) in enumerate(k5_batches(gpu, [8] * 5)):
        before = [(_np(st.params), _np(st.m), _np(st.v)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        for st, (p0, m0, v0) in zip((tr.client, tr.server), before):
            ref = torch.nn.Parameter(_t64(p0))
            opt = torch.optim.AdamW([ref], lr=float(sched.lr_at(k)), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8),
                                    weight_decay=f32(0.01))
            opt.state[ref] = {"step": torch.tensor(float(k)), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
            ref.grad = _t64(_np(st.grads))
            opt.step()
            s = opt.state[ref]
            assert within(_np(st.params), ref.detach().numpy(), p0), (type(st).__name__, k, "p")
            assert within(_np(st.m), s["exp_avg"].numpy(), m0), (type(st).__name__, k, "m")
            assert within(_np(st.v), s["exp_avg_sq"].numpy(), v0), (type(st).__name__, k, "v")
    assert int(tr.client.step_ctr.item()) == 5 and int(tr.server.step_ctr.item()) == 5


def test_k2_every_stage_method_steps_by_the_config(gpu):
    """The other ways a K2 stage steps — separate launches (fuse_optim off: apply_grad_slabs + loss log +
    step_from_slabs) and the flat-gradient path (compute / backward into grads, then step()) — equal the
    trainer's single fused launch bit for bit over three steps: same recipe, same table, same counter."""
    from splitcnn import ops
    batches = k2_batches(gpu, [13] * 3)
    make = lambda **kw: k2(gpu, graph=False, optim=optim.SGD(0.01, **K2_CFG),  # noqa: E731
                           schedule=optim.LRSchedule.from_values(TABLE4, gpu), **kw)
    ref = make()
    unfused = make()
    unfused.server.fuse_optim = False
    ref2, byhand = make(fuse_client_backward=False), make(fuse_client_backward=False)   # the cut gradient in HBM
    c, s = byhand.client, byhand.server
    for x, y in batches:
        ref.step(x, y)
        unfused.step(x, y)
        ref2.step(x, y)
        act = c.forward(x)
        cut_grad, loss_i = s.compute(act, y, 1.0 / x.shape[0], act_amax=c._act_amax,
                                     act16=c._act16 if c.emit_act16 else None)
        s.step()
        s.log_loss(loss_i)
        c.backward(cut_grad)
        c.step()
        ops.tick(s.step_ctr)     # the trainer's job: both stages share the counter
    assert same(k2_state(ref), k2_state(unfused)) and same(k2_state(ref2), k2_state(byhand))
    assert losses(ref) == losses(unfused) == losses(ref2) == losses(byhand)


# ------------------------------------------------------------------ today's constants are today's path
@pytest.mark.parametrize("B", [13, 64])
def test_k2_default_config_is_bitwise_the_default_trainer(gpu, B):
    batches = k2_batches(gpu, [B] * 3)
    res = []
    for kw in ({}, {"optim": optim.SGD(0.01)}):
        tr = k2(gpu, **kw)
        for x, y in batches:
            tr.step(x, y)
        res.append(([tr.client.params.clone(), tr.server.params.clone()], losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1] and len(res[0][1]) == 3


def test_k5_default_config_is_bitwise_the_default_trainer(gpu):
    batches = k5_batches(gpu, [8] * 3)
    res = []
    for kw in ({}, {"optim": optim.Adam(1e-3, (0.9, 0.999), 1e-8)}):
        tr = k5(gpu, **kw)
        for x, y in batches:
            tr.step(x, y)
        res.append((k5_state(tr), losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1] and len(res[0][1]) == 3


# ------------------------------------------------------------------ evaluation leaves the optimizer alone
@pytest.mark.parametrize("which", ["k2", "k5"])
def test_step_evaluate_step_equals_step_step(gpu, which):
    if which == "k2":
        make = lambda: k2(gpu, optim=optim.SGD(0.01, **K2_CFG), schedule=optim.LRSchedule.from_values(TABLE4, gpu))  # noqa: E731
        batches, state = k2_batches(gpu, [13, 13, 13]), k2_state
    else:
        make = lambda: k5(gpu, optim=optim.Adam(1e-3, **K5_CFG))  # noqa: E731
        batches, state = k5_batches(gpu, [8, 8, 8]), k5_state
    res = []
    for evaluate in (False, True):
        tr = make()
        tr.step(*batches[0])
        if evaluate:
            tr.eval_batch(*batches[2])
        tr.step(*batches[1])
        res.append((state(tr), losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ------------------------------------------------------------------ resume
@pytest.mark.parametrize("which", ["k2", "k5"])
def test_resume_from_saved_state_is_bit_for_bit(gpu, which):
    """3 steps, save the modules' state_dict()s and optimizer_state(), load into a fresh trainer (another
    init), 3 more steps == 6 straight steps, under graph=True."""
    if which == "k2":
        make = lambda seed: k2(gpu, seed=seed, optim=optim.SGD(0.01, **K2_CFG),  # noqa: E731
                               schedule=optim.LRSchedule.from_values(TABLE4, gpu))
        batches, state = k2_batches(gpu, [13] * 6), k2_state
    else:
        make = lambda seed: k5(gpu, seed=seed, optim=optim.Adam(1e-3, **K5_CFG),  # noqa: E731
                               schedule=optim.LRSchedule.from_values([1e-3, 2e-3, 1.5e-3, 5e-4], gpu))
        batches, state = k5_batches(gpu, [8] * 6), k5_state
    straight = make(0)
    for x, y in batches:
        straight.step(x, y)
    first = make(0)
    for x, y in batches[:3]:
        first.step(x, y)
    torch.cuda.synchronize()
    saved = ({k: v.cpu().clone() for k, v in first.client.model.state_dict().items()},
             {k: v.cpu().clone() for k, v in first.server.model.state_dict().items()}, first.optimizer_state())
    assert all(t.device.type == "cpu" for t in saved[2].values())
    second = make(5)
    second.client.model.load_state_dict(saved[0])
    second.server.model.load_state_dict(saved[1])
    second.load_optimizer_state(saved[2])
    for x, y in batches[3:]:
        second.step(x, y)
    assert same(state(straight), state(second))
    assert losses(straight)[3:] == losses(second)
    with pytest.raises(ValueError, match="expected keys"):
        second.load_optimizer_state({})


def test_k2_loading_state_works_under_a_captured_graph(gpu):
    """load_optimizer_state after the graph exists: the replay reads the loaded buffers and counter."""
    batches = k2_batches(gpu, [13] * 4)
    make = lambda: k2(gpu, optim=optim.SGD(0.01, **K2_CFG), schedule=optim.LRSchedule.from_values(TABLE4, gpu))  # noqa: E731
    a = make()
    for x, y in batches[:2]:
        replay_static(a, x, y)
    torch.cuda.synchronize()
    sd = ({k: v.clone() for k, v in a.client.model.state_dict().items()},      # state_dict() returns views
          {k: v.clone() for k, v in a.server.model.state_dict().items()}, a.optimizer_state())
    replay_static(a, *batches[2])
    b = make()
    replay_static(b, *batches[3])          # captures b's graph and moves its state somewhere else
    b.client.model.load_state_dict(sd[0])
    b.server.model.load_state_dict(sd[1])
    b.load_optimizer_state(sd[2])
    replay_static(b, *batches[2])
    torch.cuda.synchronize()
    assert len(b._graphs) == 1 and same(k2_state(a), k2_state(b))


# ------------------------------------------------------------------ it trains
def test_k2_trains_with_momentum_and_warmup_cosine(gpu):
    tr = k2(gpu, optim=optim.SGD(0.01, momentum=0.9),
            schedule=optim.LRSchedule.warmup_cosine(0.01, warmup=5, total=30, device=gpu))
    for x, y in k2_batches(gpu, [64] * 30, seed=42):
        tr.step(x, y)
    ls = losses(tr)
    assert len(ls) == 30 and np.isfinite(ls).all()
    assert np.mean(ls[-5:]) < np.mean(ls[:5]), (ls[:5], ls[-5:])
