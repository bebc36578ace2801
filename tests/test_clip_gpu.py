"""The gradient-clipping kernels alone: slk_reduce_sqnorm_multi (pass 1) pinned bit for bit to the summation orders
include/slk.h documents, and slk_sgdm_clip_multi / slk_adamw_clip_multi (pass 2) against torch in float64.

Inputs (tests/clip_ref.py): three segments of n = 1300 columns (a partial last block of the 1024-, 256- and 64-column
forms) with 1, 17 and 65 slabs of R.reduce_case values, in two groups {0, 1} and {2}. Every output is followed by 64 NaN
sentinels and the partials buffers start as NaN. The norm is compared bitwise with the emulation and, within the bound
derived in clip_ref's docstring (k = 44: 1.37e-6 relative), with float64 and with the total_norm
torch.nn.utils.clip_grad_norm_ returns in float64 on the kernel's own gradients; coef is two correctly rounded f32
operations on the kernel's norm (2 ulps of the float64 value); the update is torch.optim's in float64 fed
grad_kernel * coef_kernel, under the project's bound (`within`, as tests/test_optim_gpu.py), restarted from the device
state every step."""
import numpy as np
import pytest
import torch

import clip_ref as C
import head_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
EPS32 = np.finfo(np.float32).eps
N, PAD = C.N, C.PAD
SGD_CONFIGS = {
    "momentum": dict(momentum=0.9),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.5),
    "weight_decay": dict(weight_decay=5e-4),
    "all": dict(momentum=0.9, nesterov=True, weight_decay=5e-4),
}


def f32(x):
    return float(np.float32(x))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True))


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy().view(np.int32)
    want = np.asarray(want, dtype=np.float32).reshape(got.shape).view(np.int32)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ from the documented order"


def _padded(values, dev):
    """A device buffer holding `values` followed by PAD NaNs; returns (buffer, view of the values)."""
    if not isinstance(values, torch.Tensor):
        values = torch.from_numpy(np.array(values, dtype=np.float32))    # a copy: the fixtures are read-only
    v = values.to(torch.float32).reshape(-1)
    buf = torch.full((v.numel() + PAD,), NAN, dtype=torch.float32, device=dev)
    buf[:v.numel()] = v.to(dev)
    return buf, buf[:v.numel()]


def _nan(n, dev):
    buf = torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev)
    return buf, buf[:n]


_SLABS = {}


def slabs_dev(i, dev):
    """Segment i's slabs on the device, shared by every test and never written."""
    if i not in _SLABS:
        _SLABS[i] = torch.from_numpy(C.case(i)[0].copy()).to(dev)
    return _SLABS[i]


def npart(ids):
    return sum(C.nblk(N, C.SLAB_COUNTS[i]) for i in ids)


class Run:
    """Device state of one clipped optimizer over `groups` (tuples of segment ids): per segment param / grad / two
    state blocks (buf or m, v), per group partials and [norm, coef], every one with its NaN tail."""

    def __init__(self, dev, groups=C.GROUPS, slabs=None, seed=11):
        self.dev, self.groups = dev, groups
        self.ids = [i for g in groups for i in g]
        self.slabs = {i: (slabs or {}).get(i, slabs_dev(i, dev)) for i in self.ids}
        gen = torch.Generator().manual_seed(seed)
        self.p, self.g, self.s1, self.s2 = {}, {}, {}, {}
        for i in (0, 1, 2):     # the same initial values whichever segments take part
            p0 = torch.randn(N, generator=gen) * 0.1
            junk = torch.randn(N, generator=gen)
            if i in self.ids:
                self.p[i], self.g[i] = _padded(p0, dev), _nan(N, dev)
                self.s1[i], self.s2[i] = _padded(junk, dev), _padded(torch.zeros(N), dev)
        self.partials = [_nan(npart(g), dev) for g in groups]
        self.out = [_nan(2, dev) for _ in groups]
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)

    def groups_for(self, adam):
        out = []
        for k, g in enumerate(self.groups):
            if adam:
                segs = [(self.p[i][1], self.g[i][1], self.s1[i][1], self.s2[i][1], self.slabs[i]) for i in g]
            else:
                segs = [(self.p[i][1], self.g[i][1], self.s1[i][1], self.slabs[i]) for i in g]
            out.append((self.partials[k][1], self.out[k][1], segs))
        return out

    def check_sentinels(self):
        for d in (self.p, self.g, self.s1, self.s2):
            for i, (buf, _) in d.items():
                R.assert_sentinel(buf, N, f"segment {i}")
        for k, g in enumerate(self.groups):
            R.assert_sentinel(self.partials[k][0], npart(g), "partials")
            R.assert_sentinel(self.out[k][0], 2, "norm_out")


def max_norm_t(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ pass 1
def test_pass1_grad_and_partials_are_the_documented_order(gpu):
    """grad == R.reduce_emulated bit for bit in all three forms, partials == the emulation, nothing written behind
    either, and with a loss riding along the ring gets slk_loss_log's value."""
    from splitcnn import ops
    r = Run(gpu)
    v = R.exact_values(300, 31)
    ring, ctr = torch.full((3,), NAN, device=gpu), torch.tensor([1], dtype=torch.int32, device=gpu)
    ops.reduce_sqnorm_multi(r.groups_for(False), loss=(torch.from_numpy(v).float().to(gpu), 0.5, ring[:2], ctr))
    torch.cuda.synchronize()
    r.check_sentinels()
    for i in r.ids:
        _same_bits(r.g[i][1], C.case(i)[1], f"grad of segment {i} ({C.SLAB_COUNTS[i]} slabs)")
    for k in range(len(C.GROUPS)):
        _same_bits(r.partials[k][1], C.group_case(k)[0], f"partials of group {k}")
        assert torch.isnan(r.out[k][1]).all(), "pass 1 does not write norm_out"
    assert ctr.item() == 2 and torch.isnan(ring[0]) and torch.isnan(ring[2])
    _same_bits(ring[1:2], [F32(v.sum() * 0.5)], "the loss block")
    want = ops.reduce_slabs(slabs_dev(2, gpu))
    assert torch.equal(r.g[2][1], want), "grad is slk_reduce_slabs' sum"


def test_pass1_in_place_leaves_the_gradient_untouched(gpu):
    """nslab = 1 with slabs == grad (the step() paths): only read; the partials are those of that gradient."""
    from splitcnn import ops
    g = C.case(0)[0][0]
    buf, grad = _padded(g, gpu)
    before = buf.clone()
    part, out = _nan(C.nblk(N, 1), gpu), _nan(2, gpu)
    p = torch.zeros(N, device=gpu)
    ops.reduce_sqnorm_multi([(part[1], out[1], [(p, None, None, grad.view(1, -1))])])
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    R.assert_sentinel(part[0], C.nblk(N, 1), "partials")
    _same_bits(part[1], C.block_partials(g, 1), "in-place partials")
    with pytest.raises(ValueError, match="ONE slab"):
        ops.reduce_sqnorm_multi([(part[1], out[1], [(p, None, None, slabs_dev(1, gpu))])])
    with pytest.raises(ValueError, match="partials"):
        ops.reduce_sqnorm_multi([(part[1][:1], out[1], [(p, None, None, grad.view(1, -1))])])


# ------------------------------------------------------------------------------------------------ pass 2
def _check_norm_and_coef(r, k, max_norm, what):
    """Group k of run r after a step at `max_norm`: returns (kernel norm, kernel coef) as float32."""
    ids = r.groups[k]
    grads = [r.g[i][1].cpu().numpy() for i in ids]
    parts, norm_e, coef_e = C.emulate(grads, [C.SLAB_COUNTS[i] for i in ids], max_norm)
    norm, coef = (F32(v) for v in r.out[k][1].cpu().numpy())
    _same_bits(r.partials[k][1], parts, f"{what}: partials of group {k}")
    _same_bits(r.out[k][1], [norm_e, coef_e], f"{what}: [norm, coef] of group {k}")
    want = C.norm64(grads)
    bound = C.norm_bound(parts.size, ref_terms=N * len(ids))
    assert abs(float(norm) - want) <= bound * want, (what, k, float(norm), want)
    ps = [torch.nn.Parameter(torch.zeros(N, dtype=torch.float64)) for _ in ids]
    for p, g in zip(ps, grads):
        p.grad = _t64(g)
    total = float(torch.nn.utils.clip_grad_norm_(ps, float(max_norm)))
    assert abs(float(norm) - total) <= bound * total, (what, k, float(norm), total)
    c64 = C.coef64(float(norm), f32(max_norm))
    assert C.ulps(coef, F32(c64)) <= 2, (what, k, float(coef), c64)
    return norm, coef


@pytest.mark.parametrize("name", sorted(SGD_CONFIGS))
def test_sgdm_clip_matches_torch_float64(gpu, name):
    """Three steps on a table [0.1, 0.05] with max_norm = half the smaller group norm (so both groups clip): per group,
    norm / coef as documented, and the update is torch.optim.SGD's on grad * coef (clipping BEFORE weight decay: a
    reference that decays first fails the bound by orders of magnitude at these gradient sizes)."""
    from splitcnn import ops
    cfg = SGD_CONFIGS[name]
    tcfg = dict(momentum=f32(cfg.get("momentum", 0.0)), dampening=f32(cfg.get("dampening", 0.0)),
                nesterov=cfg.get("nesterov", False), weight_decay=f32(cfg.get("weight_decay", 0.0)))
    table, rates = torch.tensor([0.1, 0.05], device=gpu), [f32(0.1), f32(0.05), f32(0.05)]
    mx = F32(0.5 * min(float(C.group_case(k)[1]) for k in range(2)))
    mxd = max_norm_t(mx, gpu)
    r = Run(gpu)
    groups = r.groups_for(False)
    for k in range(3):
        before = {i: (_np(r.p[i][1]), _np(r.s1[i][1])) for i in r.ids}
        ops.reduce_sqnorm_multi(groups)
        ops.sgdm_clip_multi(groups, mxd, table, r.step, **cfg)
        ops.tick(r.step)
        torch.cuda.synchronize()
        r.check_sentinels()
        for gi, ids in enumerate(r.groups):
            norm, coef = _check_norm_and_coef(r, gi, mx, f"{name} step {k}")
            assert coef < 1
            for i in ids:
                _same_bits(r.g[i][1], C.case(i)[1], "grad stays the unclipped fixed-order sum")
                p0, b0 = before[i]
                ref = torch.nn.Parameter(_t64(p0))
                opt = torch.optim.SGD([ref], lr=rates[k], **tcfg)
                if k > 0 and tcfg["momentum"] != 0:
                    opt.state[ref]["momentum_buffer"] = _t64(b0)
                ref.grad = _t64(_np(r.g[i][1]) * float(coef))
                opt.step()
                want = ref.detach().numpy()
                assert within(_np(r.p[i][1]), want, p0), (name, i, k, np.abs(_np(r.p[i][1]) - want).max())
                if tcfg["momentum"] != 0:
                    wb = opt.state[ref]["momentum_buffer"].numpy()
                    assert within(_np(r.s1[i][1]), wb, b0), (name, i, k)
                else:
                    assert np.array_equal(_np(r.s1[i][1]), b0)
    assert int(r.step.item()) == 3


@pytest.mark.parametrize("decoupled", [True, False])
def test_adamw_clip_matches_torch_float64(gpu, decoupled):
    from splitcnn import ops
    B1, B2, EPS, WD = f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
    table, rates = torch.tensor([1e-3, 5e-4], device=gpu), [f32(1e-3), f32(5e-4), f32(5e-4)]
    mx = F32(0.5 * min(float(C.group_case(k)[1]) for k in range(2)))
    mxd = max_norm_t(mx, gpu)
    r = Run(gpu)
    for i in r.ids:
        r.s1[i][1].zero_()      # Adam's m starts at 0 (v does already)
    groups = r.groups_for(True)
    Opt = torch.optim.AdamW if decoupled else torch.optim.Adam
    for k in range(3):
        before = {i: tuple(_np(d[i][1]) for d in (r.p, r.s1, r.s2)) for i in r.ids}
        ops.reduce_sqnorm_multi(groups)
        ops.adamw_clip_multi(groups, mxd, table, r.step, 0.9, 0.999, 1e-8, weight_decay=0.01, decoupled=decoupled)
        ops.tick(r.step)
        torch.cuda.synchronize()
        r.check_sentinels()
        for gi, ids in enumerate(r.groups):
            norm, coef = _check_norm_and_coef(r, gi, mx, f"adam step {k}")
            assert coef < 1
            for i in ids:
                _same_bits(r.g[i][1], C.case(i)[1], "grad stays the unclipped fixed-order sum")
                p0, m0, v0 = before[i]
                ref = torch.nn.Parameter(_t64(p0))
                opt = Opt([ref], lr=rates[k], betas=(B1, B2), eps=EPS, weight_decay=WD)
                opt.state[ref] = {"step": torch.tensor(float(k)), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
                ref.grad = _t64(_np(r.g[i][1]) * float(coef))
                opt.step()
                st = opt.state[ref]
                for what, got, want, b in (("p", r.p, ref.detach().numpy(), p0), ("m", r.s1, st["exp_avg"].numpy(), m0),
                                           ("v", r.s2, st["exp_avg_sq"].numpy(), v0)):
                    assert within(_np(got[i][1]), want, b), (what, i, k, np.abs(_np(got[i][1]) - want).max())


@pytest.mark.parametrize("adam", [False, True])
def test_a_group_does_not_depend_on_what_shares_its_launch(gpu, adam):
    """Group {2} alone == group {2} as the second group of a joint launch, bit for bit, over two steps."""
    from splitcnn import ops
    mxd = max_norm_t(0.5 * float(C.group_case(1)[1]), gpu)
    table = torch.tensor([0.05, 0.02], device=gpu)
    runs = [Run(gpu, groups=((2,),)), Run(gpu)]
    for r in runs:
        if adam:
            for i in r.ids:
                r.s1[i][1].zero_()
        groups = r.groups_for(adam)
        for _ in range(2):
            ops.reduce_sqnorm_multi(groups)
            if adam:
                ops.adamw_clip_multi(groups, mxd, table, r.step, 0.9, 0.999, 1e-8, weight_decay=0.01)
            else:
                ops.sgdm_clip_multi(groups, mxd, table, r.step, **SGD_CONFIGS["all"])
            ops.tick(r.step)
        torch.cuda.synchronize()
        r.check_sentinels()
    alone, joint = runs
    for d in ("p", "g", "s1", "s2"):
        assert torch.equal(getattr(alone, d)[2][0].view(torch.int32), getattr(joint, d)[2][0].view(torch.int32)), d
    assert torch.equal(alone.partials[0][0].view(torch.int32), joint.partials[1][0].view(torch.int32))
    assert torch.equal(alone.out[0][1], joint.out[1][1]) and alone.out[0][1][1] < 1
    assert not torch.equal(joint.out[0][1], joint.out[1][1])


# ------------------------------------------------------------------------------------------------ edges
def test_inf_max_norm_is_bitwise_the_unclipped_multi_launch(gpu):
    from splitcnn import ops
    inf = max_norm_t(float("inf"), gpu)
    table = torch.tensor([0.05, 0.02], device=gpu)
    for adam in (False, True):
        a, b = Run(gpu), Run(gpu)
        if adam:
            for r in (a, b):
                for i in r.ids:
                    r.s1[i][1].zero_()
        for _ in range(2):
            ga = a.groups_for(adam)
            ops.reduce_sqnorm_multi(ga)
            segs = [s for _, _, ss in b.groups_for(adam) for s in ss]
            if adam:
                ops.adamw_clip_multi(ga, inf, table, a.step, 0.9, 0.999, 1e-8, weight_decay=0.01)
                ops.adamw_multi_from_slabs(segs, table, b.step, 0.9, 0.999, 1e-8, weight_decay=0.01)
            else:
                ops.sgdm_clip_multi(ga, inf, table, a.step, **SGD_CONFIGS["all"])
                ops.sgdm_multi_from_slabs(segs, table, b.step, **SGD_CONFIGS["all"])
            ops.tick(a.step)
            ops.tick(b.step)
        torch.cuda.synchronize()
        for d in ("p", "g", "s1", "s2"):
            for i in a.ids:
                x, y = getattr(a, d)[i][0], getattr(b, d)[i][0]
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (adam, d, i)
        for k in range(2):
            assert a.out[k][1][1].item() == 1.0 and a.out[k][1][0].item() == float(C.group_case(k)[1])
        assert not torch.equal(a.p[0][1], Run(gpu).p[0][1])


def test_zero_gradient_gives_coef_one_and_finite_parameters(gpu):
    from splitcnn import ops
    zeros = {i: torch.zeros(C.SLAB_COUNTS[i], N, device=gpu) for i in (0, 1, 2)}
    table = torch.tensor([0.05], device=gpu)
    for adam in (False, True):
        r = Run(gpu, slabs=zeros)
        for i in r.ids:
            r.s1[i][1].zero_()
        groups = r.groups_for(adam)
        ops.reduce_sqnorm_multi(groups)
        if adam:
            ops.adamw_clip_multi(groups, max_norm_t(1.0, gpu), table, r.step, 0.9, 0.999, 1e-8)
        else:
            ops.sgdm_clip_multi(groups, max_norm_t(1.0, gpu), table, r.step, momentum=0.9)
        torch.cuda.synchronize()
        r.check_sentinels()
        for k in range(2):
            assert r.out[k][1].tolist() == [0.0, 1.0]
        for i in r.ids:
            assert torch.isfinite(r.p[i][1]).all() and torch.equal(r.g[i][1], torch.zeros(N, device=gpu))


def test_threshold_just_above_and_just_below_the_norm(gpu):
    """d = fl(norm + 1e-6f): max_norm = the next float above d gives a quotient above 1 (coef == 1, not clipped),
    the next float below d a quotient below 1 (clipped)."""
    from splitcnn import ops
    norm = C.group_case(1)[1]
    d = F32(norm + F32(1e-6))
    table = torch.tensor([0.05], device=gpu)
    for mx, clipped in ((np.nextafter(d, F32(np.inf)), False), (np.nextafter(d, F32(0)), True)):
        r = Run(gpu, groups=((2,),))
        groups = r.groups_for(False)
        ops.reduce_sqnorm_multi(groups)
        ops.sgdm_clip_multi(groups, max_norm_t(float(mx), gpu), table, r.step, momentum=0.9)
        torch.cuda.synchronize()
        got_norm, coef = r.out[0][1].tolist()
        assert F32(got_norm) == norm
        assert (coef < 1.0) if clipped else (coef == 1.0), (float(mx), coef)
        _same_bits(r.out[0][1], [norm, C.norm_coef(C.group_total(C.group_case(1)[0]), mx)[1]], "coef at the threshold")


@pytest.mark.parametrize("poison", ["inf", "nan"])
@pytest.mark.parametrize("adam", [False, True])
def test_a_non_finite_gradient_poisons_its_own_group_only(gpu, adam, poison):
    """torch's error_if_nonfinite=False. One NaN in a slab of segment 2: norm NaN, coef NaN (the clamp is a compare),
    every parameter of group {2} is NaN. One inf: norm inf, coef = max_norm / inf = 0, and coef * g is inf * 0 = NaN in
    that column and 0 in every other — exactly torch's `g.mul_(clip_coef)` — so that parameter is NaN and the others
    take the step of a zero gradient (weight decay and, for Adam, nothing else). Either way group {0, 1} steps exactly
    as without it."""
    from splitcnn import ops
    bad = slabs_dev(2, gpu).clone()
    bad[40, 700] = float(poison)
    table = torch.tensor([0.05], device=gpu)
    mxd = max_norm_t(0.5 * float(C.group_case(0)[1]), gpu)
    zero = torch.zeros(C.SLAB_COUNTS[2], N, device=gpu)
    runs = [Run(gpu), Run(gpu, slabs={2: bad}), Run(gpu, slabs={2: zero})]
    for r in runs:
        for i in r.ids:
            r.s1[i][1].zero_()
        groups = r.groups_for(adam)
        ops.reduce_sqnorm_multi(groups)
        if adam:
            ops.adamw_clip_multi(groups, mxd, table, r.step, 0.9, 0.999, 1e-8, weight_decay=0.01)
        else:
            ops.sgdm_clip_multi(groups, mxd, table, r.step, **SGD_CONFIGS["all"])
        torch.cuda.synchronize()
        r.check_sentinels()
    clean, poisoned, zeroed = runs
    if poison == "nan":
        assert torch.isnan(poisoned.p[2][1]).all() and torch.isnan(poisoned.out[1][1]).all()
    else:
        assert poisoned.out[1][1][0].item() == float("inf") and poisoned.out[1][1][1].item() == 0.0
        nan = torch.isnan(poisoned.p[2][1])
        assert nan[700] and int(nan.sum()) == 1
        assert zeroed.out[1][1].tolist() == [0.0, 1.0]
        assert torch.equal(poisoned.p[2][1][~nan], zeroed.p[2][1][~nan]), "0 * g must act as a zero gradient"
        assert not torch.equal(poisoned.p[2][1][~nan], Run(gpu).p[2][1][~nan]), "weight decay still applies"
    for i in (0, 1):
        assert torch.equal(clean.p[i][1], poisoned.p[i][1]) and torch.isfinite(poisoned.p[i][1]).all()
        assert torch.equal(clean.s1[i][1], poisoned.s1[i][1])
    assert torch.equal(clean.out[0][1], poisoned.out[0][1]) and torch.isfinite(clean.p[2][1]).all()
