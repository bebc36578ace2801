"""optim.ClipNorm wired into the trainers: engine.SplitTrainer (K2, B = 13 and 64) and wide.WideTrainer (K5, B = 8).

The threshold of every "active" case is chosen inside the test from a measured norm — one step under
ClipNorm(inf), half of the smaller stage norm from grad_norms() — and coef < 1 is asserted on both stages, so no
case passes with clipping idle. Graph replays equal eager steps bit for bit ([norm, coef] included), set_max_norm
reaches a captured graph, ClipNorm(inf) is bitwise the trainer without clip, the fused and unfused launch layouts
agree bit for bit, each step's update is torch's clip_grad_norm_ + optimizer in float64 on the gradient the stage
wrote (the norm within the bound derived in tests/clip_ref.py, the parameters within the project's bound when the
reference scales by the kernel's coef), evaluation in between changes nothing and saved state resumes bit for bit."""
import numpy as np
import pytest
import torch

import clip_ref as C
from splitcnn import optim

pytestmark = pytest.mark.gpu

EPS32 = np.finfo(np.float32).eps
F32 = np.float32
K2_CFG = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
K5_CFG = dict(weight_decay=0.01)
TABLE4 = [0.01, 0.02, 0.015, 0.005]
K5_TABLE = [1e-3, 2e-3, 1.5e-3, 5e-4]
INF = float("inf")


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
    if tr.server.clip is not None:
        out += [tr.client.clip_out, tr.server.clip_out]
    return [t.clone() for t in out]


def k5_state(tr):
    c, s = tr.client, tr.server
    out = [c.params, s.params, c.m, c.v, s.m, s.v, c.step_ctr, s.step_ctr]
    if s.clip is not None:
        out += [c.clip_out, s.clip_out]
    return [t.clone() for t in out]


def losses(tr):
    torch.cuda.synchronize()
    return [l for _, l in tr.loss_log.flush()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def replay_static(tr, x, y):
    xs, ys = tr.static_inputs(x.shape[0])
    xs.copy_(x)
    ys.copy_(y)
    tr.step(xs, ys)


def make(which, gpu, clip, seed=None, **kw):
    """A trainer with the recipe of tests/test_optim_trainer_gpu.py and `clip` (a max_norm, a ClipNorm or None)."""
    if clip is not None and not isinstance(clip, optim.ClipNorm):
        clip = optim.ClipNorm(clip, device=gpu)
    if which == "k2":
        seed = 3 if seed is None else seed
        return k2(gpu, seed=seed, optim=optim.SGD(0.01, **K2_CFG), schedule=optim.LRSchedule.from_values(TABLE4, gpu),
                  clip=clip, **kw)
    seed = 0 if seed is None else seed
    return k5(gpu, seed=seed, optim=optim.Adam(1e-3, **K5_CFG), schedule=optim.LRSchedule.from_values(K5_TABLE, gpu),
              clip=clip, **kw)


def batches(which, gpu, sizes):
    return k2_batches(gpu, sizes) if which == "k2" else k5_batches(gpu, sizes)


_MEASURED = {}


def active_max_norm(which, gpu, B):
    """Half of the smaller stage norm of the first step, measured under ClipNorm(inf) (where coef must be 1)."""
    if (which, B) not in _MEASURED:
        tr = make(which, gpu, INF, graph=False)
        tr.step(*batches(which, gpu, [B])[0])
        n = tr.grad_norms()
        assert set(n) == {"client", "server"} and all(c == 1.0 and 0 < v < INF for v, c in n.values()), n
        _MEASURED[which, B] = 0.5 * min(v for v, _ in n.values())
    return _MEASURED[which, B]


def assert_clipping(tr):
    n = tr.grad_norms()
    assert n["client"][1] < 1 and n["server"][1] < 1, n
    return n


CASES = [("k2", 13), ("k2", 64), ("k5", 8)]


# ------------------------------------------------------------------ graph == eager, the threshold reaches the graph
@pytest.mark.parametrize("which,B", CASES)
def test_graph_replay_equals_eager_with_clipping_active(gpu, which, B):
    mx = active_max_norm(which, gpu, B)
    state = k2_state if which == "k2" else k5_state
    bs = batches(which, gpu, [B] * 4)
    res = []
    for graph in (False, True):
        tr = make(which, gpu, mx, graph=graph)
        for x, y in bs:
            tr.step(x, y)
            assert_clipping(tr)
        res.append((state(tr), losses(tr)))
    assert same(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and len(res[0][1]) == 4


@pytest.mark.parametrize("which,B", [("k2", 13), ("k5", 8)])
def test_set_max_norm_reaches_the_graph_without_recapture(gpu, which, B):
    mx = active_max_norm(which, gpu, B)
    state = k2_state if which == "k2" else k5_state
    bs = batches(which, gpu, [B] * 3)
    tr = make(which, gpu, INF)
    assert tr.client.clip is tr.server.clip
    replay_static(tr, *bs[0])
    n_graphs = len(tr._graphs)
    assert tr.grad_norms()["server"][1] == 1.0
    tr.client.clip.set_max_norm(mx)
    for x, y in bs[1:]:
        replay_static(tr, x, y)
    assert_clipping(tr)
    assert len(tr._graphs) == n_graphs == 1
    # an eager trainer: the first step unclipped, then built at the new value
    ref = make(which, gpu, INF, graph=False)
    ref.step(*bs[0])
    ref.client.clip.set_max_norm(mx)
    for x, y in bs[1:]:
        ref.step(x, y)
    assert same(state(tr), state(ref)) and losses(tr) == losses(ref)


@pytest.mark.parametrize("which,B", CASES)
def test_inf_threshold_is_bitwise_the_trainer_without_clip(gpu, which, B):
    bs = batches(which, gpu, [B] * 3)
    res = []
    for clip in (None, INF):
        tr = make(which, gpu, clip)
        for x, y in bs:
            tr.step(x, y)
        st = k2_state(tr) if which == "k2" else k5_state(tr)
        res.append((st[:8 if which == "k5" else 6], losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1] and len(res[0][1]) == 3


# ------------------------------------------------------------------ launch layouts agree
def _run_pair(which, gpu, B, tweak):
    mx = active_max_norm(which, gpu, B)
    bs = batches(which, gpu, [B] * 3)
    res = []
    for flag in (True, False):
        tr = tweak(flag, mx)
        for x, y in bs:
            tr.step(x, y)
            assert_clipping(tr)
        res.append(((k2_state if which == "k2" else k5_state)(tr), losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@pytest.mark.parametrize("B", [13, 64])
def test_k2_client_as_second_group_is_bit_identical_to_stepping_alone(gpu, B):
    """The fused K2 step: the client's segment rides in the server's two clip launches as a group of its own. Giving
    the client a ClipNorm object of its own (same threshold) makes the trainer step it alone through
    step_from_slabs on the very same slabs: every parameter, buffer, counter and [norm, coef] equal bit for bit."""
    def tweak(joined, mx):
        tr = make("k2", gpu, mx, graph=False)
        assert tr.fuse_client_backward and tr.client.clip is tr.server.clip
        if not joined:
            tr.client.clip = optim.ClipNorm(mx, device=gpu)
        return tr
    _run_pair("k2", gpu, B, tweak)


@pytest.mark.parametrize("B", [13, 64])
def test_k2_fuse_client_backward_on_and_off_with_clipping(gpu, B):
    """fuse_client_backward True against False with clipping active. The two settings run different client
    weight-gradient kernels (inside the x3 dgrad / conv1_wgrad_remask on the cut gradient in HBM) with other slab
    counts and summation orders, so already without clipping their client gradients agree only to rounding
    (tests/test_x3_gpu.py::test_trainer_fused_client_backward_matches_unfused: 1e-3 of the largest update) and bit
    identity between them is not a property of the trainer. What clipping must keep: over the first step, which both
    start from the same state, the server — whose gradient does not depend on the client's path — is bit-identical,
    [norm, coef] included; the client's norm differs by no more than its gradient does (the norm is 1-Lipschitz:
    | ||a|| - ||b|| | <= ||a - b||), and its update agrees on the existing test's bar. Both clip (coef < 1). The grouping
    itself is pinned bit for bit by the test above. Measured on the MI355X: B = 13: the two client norms 0.30055442 /
    0.30055445 (1 ulp, 9.9e-8 relative; ||g_on - g_off|| / norm 1.7e-7), update difference 3.0e-6 of the largest update;
    B = 64: the norms equal (||g_on - g_off|| / norm 1.7e-7), updates equal."""
    mx = active_max_norm("k2", gpu, B)
    x, y = k2_batches(gpu, [B])[0]
    trs = []
    for fuse in (True, False):
        tr = make("k2", gpu, mx, graph=False, fuse_client_backward=fuse)
        assert tr.fuse_client_backward == fuse
        p0 = tr.client.params.clone()
        tr.step(x, y)
        assert_clipping(tr)
        trs.append(tr)
    on, off = trs
    assert same([on.server.params, on.server.buf, on.server.clip_out, on.server.grads],
                [off.server.params, off.server.buf, off.server.clip_out, off.server.grads])
    assert losses(on) == losses(off)
    g_on, g_off = _np(on.client.grads), _np(off.client.grads)
    n_on, n_off = float(on.client.clip_out[0]), float(off.client.clip_out[0])
    bound = C.norm_bound(max(on.client.clip_npart, off.client.clip_npart))
    dn, dg = abs(n_on - n_off), float(np.linalg.norm(g_on - g_off))
    u_on, u_off = _np(on.client.params) - _np(p0), _np(off.client.params) - _np(p0)
    print(f"B={B}: norm on/off {n_on!r} {n_off!r} |dn|/n={dn / n_off:.3e} ||dg||/n={dg / n_off:.3e} "
          f"update diff/max={np.abs(u_on - u_off).max() / np.abs(u_off).max():.3e}")
    assert dn <= dg + bound * (n_on + n_off)
    assert np.abs(u_on - u_off).max() <= 1e-3 * np.abs(u_off).max()


@pytest.mark.parametrize("B", [13, 64])
def test_k2_server_fuse_optim_on_and_off_bit_identical(gpu, B):
    def tweak(flag, mx):
        tr = make("k2", gpu, mx, graph=False)
        tr.server.fuse_optim = flag
        return tr
    _run_pair("k2", gpu, B, tweak)


def test_k5_fuse_adam_on_and_off_bit_identical(gpu):
    def tweak(flag, mx):
        tr = make("k5", gpu, mx, graph=False)
        tr.client.fuse_adam = flag
        return tr
    _run_pair("k5", gpu, 8, tweak)


# ------------------------------------------------------------------ every step's update is torch's
def _check_stage_norm(st, max_norm):
    """The stage's [norm, coef] against float64 on the gradient it wrote; returns the kernel's coef."""
    norm, coef = (F32(v) for v in st.clip_out.cpu().numpy())
    g = st.grads.detach().cpu().numpy()
    bound = C.norm_bound(st.clip_npart, ref_terms=g.size)
    ref = torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64))
    ref.grad = _t64(g)
    total = float(torch.nn.utils.clip_grad_norm_([ref], float(max_norm)))
    assert abs(float(norm) - total) <= bound * total, (type(st).__name__, float(norm), total)
    assert abs(float(norm) - C.norm64([g])) <= bound * total
    assert C.ulps(coef, F32(C.coef64(float(norm), f32(max_norm)))) <= 2 and coef < 1
    return float(coef)


@pytest.mark.parametrize("B", [13, 64])
@pytest.mark.parametrize("fuse", [True, False])
def test_k2_update_matches_torch_clip_and_sgd_per_step(gpu, B, fuse):
    mx = active_max_norm("k2", gpu, B)
    tr = make("k2", gpu, mx, graph=False, fuse_client_backward=fuse)
    sched = tr.client.schedule
    tcfg = dict(momentum=f32(0.9), nesterov=True, weight_decay=f32(5e-4))
    for k, (x, y) in enumerate(k2_batches(gpu, [B] * 4)):
        before = [(_np(st.params), _np(st.buf)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        torch.cuda.synchronize()
        for st, (p0, b0) in zip((tr.client, tr.server), before):
            coef = _check_stage_norm(st, mx)
            ref = torch.nn.Parameter(_t64(p0))
            opt = torch.optim.SGD([ref], lr=float(sched.lr_at(k)), **tcfg)
            if k > 0:
                opt.state[ref]["momentum_buffer"] = _t64(b0)
            ref.grad = _t64(_np(st.grads) * coef)
            opt.step()
            assert within(_np(st.params), ref.detach().numpy(), p0), (type(st).__name__, k)
            assert within(_np(st.buf), opt.state[ref]["momentum_buffer"].numpy(), b0), (type(st).__name__, k)
    assert int(tr.server.step_ctr.item()) == 4


def test_k5_update_matches_torch_clip_and_adamw_per_step(gpu):
    mx = active_max_norm("k5", gpu, 8)
    tr = make("k5", gpu, mx, graph=False)
    sched = tr.client.schedule
    for k, (x, y) in enumerate(k5_batches(gpu, [8] * 4)):
        before = [(_np(st.params), _np(st.m), _np(st.v)) for st in (tr.client, tr.server)]
        tr.step(x, y)
        torch.cuda.synchronize()
        for st, (p0, m0, v0) in zip((tr.client, tr.server), before):
            coef = _check_stage_norm(st, mx)
            ref = torch.nn.Parameter(_t64(p0))
            opt = torch.optim.AdamW([ref], lr=float(sched.lr_at(k)), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8),
                                    weight_decay=f32(0.01))
            opt.state[ref] = {"step": torch.tensor(float(k)), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
            ref.grad = _t64(_np(st.grads) * coef)
            opt.step()
            s = opt.state[ref]
            assert within(_np(st.params), ref.detach().numpy(), p0), (type(st).__name__, k, "p")
            assert within(_np(st.m), s["exp_avg"].numpy(), m0), (type(st).__name__, k, "m")
            assert within(_np(st.v), s["exp_avg_sq"].numpy(), v0), (type(st).__name__, k, "v")


# ------------------------------------------------------------------ every stepping method of a stage clips
def test_k2_every_stage_method_clips(gpu):
    """Separate stage calls (forward_backward + apply_grad_slabs + log_loss, then backward_step) equal the unfused
    trainer bit for bit. The flat-gradient path (compute / backward into grads, then step()) sums the same gradient
    but takes its square-norm partials over 1024-column blocks of ONE slab, so its norm may differ in the last
    bits: there the gradients are compared bitwise, the norm and coef within their bounds of float64, and the
    parameters with torch's float64 update at the kernel's coef."""
    from splitcnn import ops
    B = 13
    mx = active_max_norm("k2", gpu, B)
    bs = k2_batches(gpu, [B] * 3)
    ref2 = make("k2", gpu, mx, graph=False, fuse_client_backward=False)
    byhand = make("k2", gpu, mx, graph=False, fuse_client_backward=False)
    flat = make("k2", gpu, mx, graph=False, fuse_client_backward=False)
    tcfg = dict(momentum=f32(0.9), nesterov=True, weight_decay=f32(5e-4))
    for k, (x, y) in enumerate(bs):
        ref2.step(x, y)
        c, s = byhand.client, byhand.server
        act = c.forward(x)
        a16 = c._act16 if c.emit_act16 else None
        cut_grad, loss_i, s2, s3 = s.forward_backward(act, y, 1.0 / B, act_amax=c._act_amax, act16=a16)
        s.apply_grad_slabs(s2, s3)
        s.log_loss(loss_i)
        c.backward_step(cut_grad)
        ops.tick(s.step_ctr)
        assert same(k2_state(ref2), k2_state(byhand)), k
        assert_clipping(byhand)
        # the flat-gradient path, restarted from the reference's state before this step
        c, s = flat.client, flat.server
        before = [(_np(st.params), _np(st.buf)) for st in (c, s)]
        act = c.forward(x)
        cut_grad, loss_i = s.compute(act, y, 1.0 / B, act_amax=c._act_amax, act16=c._act16 if c.emit_act16 else None)
        s.step()
        s.log_loss(loss_i)
        c.backward(cut_grad)
        c.step()
        ops.tick(s.step_ctr)
        torch.cuda.synchronize()
        for st, rs, (p0, b0) in zip((c, s), (ref2.client, ref2.server), before):
            assert torch.equal(st.grads, rs.grads)
            coef = _check_stage_norm(st, mx)
            r = torch.nn.Parameter(_t64(p0))
            opt = torch.optim.SGD([r], lr=float(c.schedule.lr_at(k)), **tcfg)
            if k > 0:
                opt.state[r]["momentum_buffer"] = _t64(b0)
            r.grad = _t64(_np(st.grads) * coef)
            opt.step()
            assert within(_np(st.params), r.detach().numpy(), p0), (type(st).__name__, k)
            st.params.copy_(rs.params)      # follow the reference trajectory: the next step's gradients agree again
            st.buf.copy_(rs.buf)
    assert losses(ref2) == losses(byhand) == losses(flat)


def test_k5_flat_gradient_paths_clip(gpu):
    """WideClientStage.step_from_grads and WideServerStage.finish_step (the g.view(1, -1) paths): same gradient as the
    trainer's step bit for bit, norm and coef within their bounds, the parameters torch's AdamW at the kernel's coef."""
    B = 8
    mx = active_max_norm("k5", gpu, B)
    x, y = k5_batches(gpu, [B])[0]
    ref = make("k5", gpu, mx, graph=False)
    ref.step(x, y)
    tr = make("k5", gpu, mx, graph=False)
    c, s = tr.client, tr.server
    before = [(_np(st.params), _np(st.m), _np(st.v)) for st in (c, s)]
    cut = c.forward(x)
    dcut = s.accumulate(cut, y, 1.0 / B, 0, 0, 1)
    s.finish_step(1)
    c.backward_grads(dcut)
    c.step_from_grads()
    torch.cuda.synchronize()
    for st, rs, (p0, m0, v0) in zip((c, s), (ref.client, ref.server), before):
        assert torch.equal(st.grads, rs.grads)
        coef = _check_stage_norm(st, mx)
        r = torch.nn.Parameter(_t64(p0))
        opt = torch.optim.AdamW([r], lr=f32(K5_TABLE[0]), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8),
                                weight_decay=f32(0.01))
        opt.state[r] = {"step": torch.tensor(0.0), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
        r.grad = _t64(_np(st.grads) * coef)
        opt.step()
        assert within(_np(st.params), r.detach().numpy(), p0), type(st).__name__


# ------------------------------------------------------------------ evaluation, resume
@pytest.mark.parametrize("which,B", [("k2", 13), ("k5", 8)])
def test_step_evaluate_step_equals_step_step(gpu, which, B):
    mx = active_max_norm(which, gpu, B)
    bs = batches(which, gpu, [B] * 3)
    state = k2_state if which == "k2" else k5_state
    res = []
    for evaluate in (False, True):
        tr = make(which, gpu, mx)
        tr.step(*bs[0])
        if evaluate:
            tr.eval_batch(*bs[2])
        tr.step(*bs[1])
        assert_clipping(tr)
        res.append((state(tr), losses(tr)))
    assert same(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@pytest.mark.parametrize("which,B", [("k2", 13), ("k5", 8)])
def test_resume_is_bit_for_bit_and_keys_are_unchanged(gpu, which, B):
    mx = active_max_norm(which, gpu, B)
    bs = batches(which, gpu, [B] * 4)
    state = k2_state if which == "k2" else k5_state
    straight = make(which, gpu, mx)
    for x, y in bs:
        straight.step(x, y)
    first = make(which, gpu, mx)
    for x, y in bs[:2]:
        first.step(x, y)
    torch.cuda.synchronize()
    saved = ({k: v.cpu().clone() for k, v in first.client.model.state_dict().items()},
             {k: v.cpu().clone() for k, v in first.server.model.state_dict().items()}, first.optimizer_state())
    assert sorted(saved[2]) == sorted(make(which, gpu, None).optimizer_state()), "clip tensors are no optimizer state"
    second = make(which, gpu, mx, seed=5)
    second.client.model.load_state_dict(saved[0])
    second.server.model.load_state_dict(saved[1])
    second.load_optimizer_state(saved[2])
    for x, y in bs[2:]:
        second.step(x, y)
    assert_clipping(second)
    assert same(state(straight), state(second))
    assert losses(straight)[2:] == losses(second)


@pytest.mark.parametrize("which,B", [("k2", 13), ("k5", 8)])
def test_clip_without_optim_selects_the_default_recipe(gpu, which, B):
    """Like schedule=, clip= alone runs the configured kernels at the default constants: with ClipNorm(inf) bitwise
    the default trainer, and the norms are there to read."""
    mk, state = (k2, lambda t: [t.client.params, t.server.params]) if which == "k2" else (k5, lambda t: k5_state(t)[:8])
    bs = batches(which, gpu, [B] * 2)
    plain, clipped = mk(gpu), mk(gpu, clip=optim.ClipNorm(INF, device=gpu))
    assert plain.server.optim is None and clipped.server.optim is not None and clipped.client.optim is not None
    for x, y in bs:
        plain.step(x, y)
        clipped.step(x, y)
    assert same([t.clone() for t in state(plain)], [t.clone() for t in state(clipped)])
    assert losses(plain) == losses(clipped)
    assert all(c == 1.0 and v > 0 for v, c in clipped.grad_norms().values())


def test_a_segment_of_a_stage_with_another_clip_setting_is_refused(gpu):
    """A clipped stage does not take an unclipped stage's segment into its own norm (or the reverse): no launch."""
    from splitcnn.engine import ClientStage, ServerStage
    slabs = torch.zeros(1, 320, device=gpu)
    cfg = optim.SGD(0.01, momentum=0.9)
    for s_clip, c_clip in ((optim.ClipNorm(1.0, device=gpu), None), (None, optim.ClipNorm(1.0, device=gpu))):
        server, client = ServerStage(device=gpu, optim=cfg, clip=s_clip), ClientStage(device=gpu, optim=cfg, clip=c_clip)
        before = client.params.clone()
        with pytest.raises(ValueError, match="clip="):
            server._sgdm([client.optim_segment(slabs)], multi=True)
        assert torch.equal(client.params, before)


def test_grad_norms_needs_clip(gpu):
    with pytest.raises(RuntimeError, match="clip="):
        make("k2", gpu, None).grad_norms()
