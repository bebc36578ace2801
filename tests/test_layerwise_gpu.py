"""The layer-wise trust-ratio kernels alone: slk_reduce_tnorm_multi / slk_lamb_moments_multi (pass 1) pinned bit for
bit to the summation order include/slk.h documents, slk_lars_multi / slk_lamb_multi (pass 2) against the float64
closed form of tests/layerwise_ref.py within its derived bounds.

Inputs: clip_ref's three segments of n = 1300 columns with 1, 17 and 65 slabs (a partial last block in the 1024-, 256-
and 64-column forms) in two groups {0, 1} and {2}; each segment is a [W | b] pair with nw weight elements, nw in
1100 (straddles a block in all three forms), 1024 (on a boundary of all three), 1300 (no bias) and 1299 (a one-element
bias). Every output is followed by 64 NaN sentinels; partials and trust_out start as NaN."""
import ctypes

import numpy as np
import pytest
import torch

import clip_ref as C
import head_ref64 as R
import layerwise_ref as L

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
EPS32 = np.finfo(np.float32).eps
N, PAD = C.N, C.PAD
MIXED = {0: 1100, 1: 1024, 2: 1299}
SGD_CONFIGS = {
    "momentum": dict(momentum=0.9),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.5),
    "weight_decay": dict(weight_decay=5e-4),
    "all": dict(momentum=0.9, nesterov=True, weight_decay=5e-4),
}
LARS_KW = dict(trust_coef=1e-3, eps=1e-8)
B1, B2, LEPS = 0.9, 0.999, 1e-6


def f32(x):
    return float(np.float32(x))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy().view(np.int32)
    want = np.asarray(want, dtype=np.float32).reshape(got.shape).view(np.int32)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ from the documented order"


def _padded(values, dev):
    if not isinstance(values, torch.Tensor):
        values = torch.from_numpy(np.array(values, dtype=np.float32))
    v = values.to(torch.float32).reshape(-1)
    buf = torch.full((v.numel() + PAD,), NAN, dtype=torch.float32, device=dev)
    buf[:v.numel()] = v.to(dev)
    return buf, buf[:v.numel()]


def _nan(n, dev):
    buf = torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev)
    return buf, buf[:n]


_SLABS = {}


def slabs_dev(i, dev):
    if i not in _SLABS:
        _SLABS[i] = torch.from_numpy(C.case(i)[0].copy()).to(dev)
    return _SLABS[i]


def nblk(i):
    return C.nblk(N, C.SLAB_COUNTS[i])


class Run:
    """Device state of one layer-wise optimizer over `groups` (tuples of segment ids): per segment param / grad / two
    state blocks (buf or m, v), per group partials [4 per block] and trust_out [2 per segment][3], each with a NaN
    tail. `nws[i]` is segment i's weight count."""

    def __init__(self, dev, nws=MIXED, groups=C.GROUPS, slabs=None, params=None, lamb=False):
        self.dev, self.groups, self.nws, self.lamb = dev, groups, dict(nws), lamb
        self.ids = [i for g in groups for i in g]
        self.slabs = {i: (slabs or {}).get(i, slabs_dev(i, dev)) for i in self.ids}
        self.p, self.g, self.s1, self.s2 = {}, {}, {}, {}
        for i in self.ids:
            self.p[i] = _padded((params or {}).get(i, L.params_case(i)), dev)
            self.g[i] = _nan(N, dev)
            self.s1[i] = _padded(torch.zeros(N) if lamb else L.state_case(i), dev)
            self.s2[i] = _padded(torch.zeros(N), dev)
        self.partials = [_nan(4 * sum(nblk(i) for i in g), dev) for g in groups]
        self.out = [_nan(6 * len(g), dev) for g in groups]
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)

    def groups_arg(self):
        out = []
        for k, g in enumerate(self.groups):
            if self.lamb:
                segs = [(self.p[i][1], self.g[i][1], self.s1[i][1], self.s2[i][1], self.slabs[i], self.nws[i]) for i in g]
            else:
                segs = [(self.p[i][1], self.g[i][1], self.s1[i][1], self.slabs[i], self.nws[i]) for i in g]
            out.append((self.partials[k][1], self.out[k][1], segs))
        return out

    def seg_partials(self, i):
        """Segment i's [nblk, 4] partials on the host."""
        for k, g in enumerate(self.groups):
            if i in g:
                off = sum(nblk(j) for j in g[:g.index(i)])
                return self.partials[k][1].cpu().numpy().reshape(-1, 4)[off:off + nblk(i)]

    def rows(self, i):
        """Segment i's trust_out rows [[w_norm, x_norm, ratio] of the weight, of the bias] as float32."""
        for k, g in enumerate(self.groups):
            if i in g:
                return self.out[k][1].cpu().numpy().reshape(-1, 3)[2 * g.index(i):2 * g.index(i) + 2]

    def check_sentinels(self):
        for d in (self.p, self.g, self.s1, self.s2):
            for i, (buf, _) in d.items():
                R.assert_sentinel(buf, N, f"segment {i}")
        for k, g in enumerate(self.groups):
            R.assert_sentinel(self.partials[k][0], 4 * sum(nblk(i) for i in g), "partials")
            R.assert_sentinel(self.out[k][0], 6 * len(g), "trust_out")

    def step_lars(self, table, cfg, exclude_bias=True, loss=None):
        from splitcnn import ops
        ga = self.groups_arg()
        ops.reduce_tnorm_multi(ga, loss=loss)
        ops.lars_multi(ga, table, self.step, exclude_bias=exclude_bias, **cfg, **LARS_KW)
        ops.tick(self.step)

    def step_lamb(self, table, wd, exclude_bias=True):
        from splitcnn import ops
        ga = self.groups_arg()
        ops.lamb_moments_multi(ga, self.step, B1, B2, LEPS, weight_decay=wd, exclude_bias=exclude_bias)
        ops.lamb_multi(ga, table, self.step, B1, B2, LEPS, weight_decay=wd, exclude_bias=exclude_bias)
        ops.tick(self.step)


def same_run(a, b, ids, what):
    for d in ("p", "g", "s1", "s2"):
        for i in ids:
            x, y = getattr(a, d)[i][0], getattr(b, d)[i][0]
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, d, i)


# ------------------------------------------------------------------------------------------------ pass 1
@pytest.mark.parametrize("nw", L.NW_CASES)
def test_lars_pass1_grad_and_partials_are_the_documented_order(gpu, nw):
    """grad == R.reduce_emulated bit for bit in all three forms, every block's four partials == the emulation, nothing
    written behind either or to trust_out, and a loss riding along lands in the ring."""
    from splitcnn import ops
    r = Run(gpu, nws={i: nw for i in (0, 1, 2)})
    v = R.exact_values(300, 31)
    ring, ctr = torch.full((3,), NAN, device=gpu), torch.tensor([1], dtype=torch.int32, device=gpu)
    ops.reduce_tnorm_multi(r.groups_arg(), loss=(torch.from_numpy(v).float().to(gpu), 0.5, ring[:2], ctr))
    torch.cuda.synchronize()
    r.check_sentinels()
    for i in r.ids:
        _same_bits(r.g[i][1], C.case(i)[1], f"grad of segment {i}")
        want = L.partials(C.case(i)[1], L.params_case(i), C.SLAB_COUNTS[i], nw)
        _same_bits(torch.from_numpy(r.seg_partials(i).copy()), want, f"partials of segment {i}, nw {nw}")
    assert all(torch.isnan(o[1]).all() for o in r.out), "pass 1 does not write trust_out"
    assert ctr.item() == 2 and torch.isnan(ring[0]) and torch.isnan(ring[2])
    _same_bits(ring[1:2], [F32(v.sum() * 0.5)], "the loss block")


@pytest.mark.parametrize("nw", L.NW_CASES)
def test_lamb_pass1_moments_and_partials(gpu, nw):
    """grad bit for bit; m and v within the Adam op tests' bar of float64; the p^2 partials bit for bit the emulation;
    the u^2 partials within the derived bound (elementwise error of u plus the block's summation error)."""
    from splitcnn import ops
    wd = f32(0.01)
    r = Run(gpu, nws={i: nw for i in (0, 1, 2)}, lamb=True)
    for i in r.ids:       # moved moments from a non-trivial state
        r.s1[i][1].copy_(torch.from_numpy(np.array(L.state_case(i))))
        r.s2[i][1].copy_(torch.from_numpy(np.array(L.state_case(i))) ** 2)
    r.step.fill_(2)
    before = {i: (_np(r.s1[i][1]), _np(r.s2[i][1])) for i in r.ids}
    ops.lamb_moments_multi(r.groups_arg(), r.step, B1, B2, LEPS, weight_decay=wd, exclude_bias=False)
    torch.cuda.synchronize()
    r.check_sentinels()
    for i in r.ids:
        g, p = C.case(i)[1], L.params_case(i)
        m0, v0 = before[i]
        _same_bits(r.g[i][1], g, f"grad of segment {i}")
        u64, e_u = L.lamb_u_error(g, m0, v0, p, 2, f32(B1), f32(B2), f32(LEPS), wd)
        _, m1, v1 = L.lamb_direction64(g, m0, v0, p, 2, f32(B1), f32(B2), f32(LEPS), wd)
        assert within(_np(r.s1[i][1]), m1, m0) and within(_np(r.s2[i][1]), v1, v0), i
        got = r.seg_partials(i)
        want = L.partials(np.zeros(N), p, C.SLAB_COUNTS[i], nw)
        _same_bits(torch.from_numpy(got[:, [1, 3]].copy()), want[:, [1, 3]], f"p^2 partials of segment {i}")
        cols = C.cols_per_block(C.SLAB_COUNTS[i])
        for b in range(nblk(i)):
            for k, s in ((0, slice(b * cols, min((b + 1) * cols, nw))), (2, slice(max(b * cols, nw), (b + 1) * cols))):
                uu, ee = u64[s], e_u[s]
                exact = float((uu ** 2).sum())
                assert abs(float(got[b, k]) - exact) <= L.sumsq_bound(uu, ee, 22) + N * 2.0 ** -53 * exact, (i, b, k)


def test_pass1_in_place_leaves_the_gradient_untouched(gpu):
    from splitcnn import ops
    g = C.case(0)[0][0]
    for lamb in (False, True):
        buf, grad = _padded(g, gpu)
        before = buf.clone()
        part, out = _nan(4 * C.nblk(N, 1), gpu), _nan(6, gpu)
        p = torch.from_numpy(np.array(L.params_case(0))).to(gpu)
        z = [torch.zeros(N, device=gpu) for _ in range(2)]
        if lamb:
            ops.lamb_moments_multi([(part[1], out[1], [(p, None, z[0], z[1], grad.view(1, -1), 1100)])], torch.zeros(
                1, dtype=torch.int32, device=gpu), B1, B2, LEPS)
        else:
            ops.reduce_tnorm_multi([(part[1], out[1], [(p, None, z[0], grad.view(1, -1), 1100)])])
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
        R.assert_sentinel(part[0], 4 * C.nblk(N, 1), "partials")
        want = L.partials(g, L.params_case(0), 1, 1100)
        cols = [1, 3] if lamb else [0, 1, 2, 3]
        _same_bits(part[1].view(-1, 4)[:, cols].contiguous(), want[:, cols], "in-place partials")
    with pytest.raises(ValueError, match="ONE slab"):
        ops.reduce_tnorm_multi([(part[1], out[1], [(p, None, z[0], slabs_dev(1, gpu), 1100)])])
    with pytest.raises(ValueError, match="partials"):
        ops.reduce_tnorm_multi([(part[1][:4], out[1], [(p, None, z[0], grad.view(1, -1), 1100)])])
    with pytest.raises(ValueError, match="nw"):
        ops.reduce_tnorm_multi([(part[1], out[1], [(p, None, z[0], grad.view(1, -1), N + 1)])])


# ------------------------------------------------------------------------------------------------ pass 2
def _check_rows(r, i, before_p, x64, bound_x, ratio64, bound_r, excl, what):
    """Segment i's trust_out rows against float64: returns the device's (weight ratio, bias ratio)."""
    rows, nw, out = r.rows(i), r.nws[i], [1.0, 1.0]
    for k, (s, is_bias) in enumerate(L.tensors(N, nw)):
        wn, xn, ratio = (float(v) for v in rows[1 if is_bias else 0])
        wn64, xn64 = L.norm64(before_p[s]), L.norm64(x64[s])
        nb = L.norm_bound(nblk(i), ref_terms=N)
        assert abs(wn - wn64) <= nb * wn64, (what, i, is_bias, wn, wn64)
        assert abs(xn - xn64) <= bound_x(s) * xn64, (what, i, is_bias, xn, xn64)
        if is_bias and excl:
            assert ratio == 1.0, (what, i)
        else:
            want = ratio64(wn64, xn64)
            assert abs(ratio - want) <= bound_r(s) * want, (what, i, is_bias, ratio, want)
        out[1 if is_bias else 0] = ratio
    if nw == N:
        assert np.isnan(rows[1]).all(), "no bias: its row is not written"
    return out


@pytest.mark.parametrize("nws", [MIXED, {0: 1300, 1: 1300, 2: 1100}], ids=["mixed", "nobias"])
@pytest.mark.parametrize("name", sorted(SGD_CONFIGS))
def test_lars_matches_float64(gpu, name, nws):
    """Three steps on a table [0.1, 0.05]: after each, every tensor's [w_norm, g_norm, ratio] within the derived bounds
    of float64, and parameters and momentum buffers `within` one float64 step from the device state before the step,
    taken with the device's ratios. exclude_bias=False, so every bias earns a ratio of its own norms."""
    cfg = SGD_CONFIGS[name]
    c64 = dict(momentum=f32(cfg.get("momentum", 0.0)), dampening=f32(cfg.get("dampening", 0.0)),
               nesterov=cfg.get("nesterov", False), weight_decay=f32(cfg.get("weight_decay", 0.0)),
               trust_coef=f32(1e-3), eps=f32(1e-8))
    table, rates = torch.tensor([0.1, 0.05], device=gpu), [f32(0.1), f32(0.05), f32(0.05)]
    r = Run(gpu, nws=nws)
    for k in range(3):
        before = {i: (_np(r.p[i][1]), _np(r.s1[i][1])) for i in r.ids}
        r.step_lars(table, cfg, exclude_bias=False)
        torch.cuda.synchronize()
        r.check_sentinels()
        for i in r.ids:
            _same_bits(r.g[i][1], C.case(i)[1], "grad is the fixed-order sum")
            p0, b0 = before[i]
            g = _np(r.g[i][1])
            ratios = _check_rows(
                r, i, p0, g, lambda s: L.norm_bound(nblk(i), ref_terms=N),
                lambda wn, gn: L.lars_ratio64(wn, gn, c64["trust_coef"], c64["weight_decay"], c64["eps"]),
                lambda s: L.lars_ratio_bound(nblk(i), ref_terms=N), False, f"{name} step {k}")
            wp, wb, _ = L.lars_step64(p0, g, b0, k, rates[k], r.nws[i], exclude_bias=False, ratios=ratios, **c64)
            assert within(_np(r.p[i][1]), wp, p0), (name, i, k, np.abs(_np(r.p[i][1]) - wp).max())
            if c64["momentum"] != 0:
                assert within(_np(r.s1[i][1]), wb, b0), (name, i, k)
            else:
                assert np.array_equal(_np(r.s1[i][1]), b0)
            assert not np.array_equal(_np(r.p[i][1]), p0)
    assert int(r.step.item()) == 3


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_lamb_matches_float64(gpu, wd):
    """Three steps on a table [1e-3, 5e-4] with exclude_bias=False: norms and ratio within the derived bounds (u_norm's
    includes u's elementwise error), m / v / p `within` one float64 step from the device state, device ratios."""
    wd = f32(wd)
    table, rates = torch.tensor([1e-3, 5e-4], device=gpu), [f32(1e-3), f32(5e-4), f32(5e-4)]
    r = Run(gpu, lamb=True)
    hyp = (f32(B1), f32(B2), f32(LEPS))
    for k in range(3):
        before = {i: tuple(_np(d[i][1]) for d in (r.p, r.s1, r.s2)) for i in r.ids}
        r.step_lamb(table, wd, exclude_bias=False)
        torch.cuda.synchronize()
        r.check_sentinels()
        for i in r.ids:
            p0, m0, v0 = before[i]
            g = _np(r.g[i][1])
            u64, e_u = L.lamb_u_error(g, m0, v0, p0, k, *hyp, wd)
            ub = lambda s: L.lamb_unorm_bound(nblk(i), u64[s], e_u[s], ref_terms=N)   # noqa: E731
            ratios = _check_rows(r, i, p0, u64, ub, L.lamb_ratio64,
                                 lambda s: L.lamb_ratio_bound(nblk(i), ub(s), ref_terms=N), False, f"lamb step {k}")
            wp, wm, wv, _ = L.lamb_step64(p0, g, m0, v0, k, rates[k], r.nws[i], *hyp, weight_decay=wd,
                                          exclude_bias=False, ratios=ratios)
            for what, got, want, b in (("p", r.p, wp, p0), ("m", r.s1, wm, m0), ("v", r.s2, wv, v0)):
                assert within(_np(got[i][1]), want, b), (what, i, k, np.abs(_np(got[i][1]) - want).max())
    assert int(r.step.item()) == 3


def _plain(params, gpu, table, lamb, cfg):
    """The plain configured multi launch at weight decay 0 on the same inputs as a Run(gpu, params=params)."""
    from splitcnn import ops
    b = Run(gpu, params=params, lamb=lamb)
    segs = [s[:-1] for _, _, ss in b.groups_arg() for s in ss]
    if lamb:
        ops.adamw_multi_from_slabs(segs, table, b.step, B1, B2, LEPS, weight_decay=0.0)
    else:
        ops.sgdm_multi_from_slabs(segs, table, b.step, **dict(cfg, weight_decay=0.0))
    return b


@pytest.mark.parametrize("lamb", [False, True], ids=["lars", "lamb"])
def test_excluded_bias_and_zero_weight_are_bitwise_the_plain_step(gpu, lamb):
    """exclude_bias=True: every bias element is bitwise slk_sgdm_multi_from_slabs / slk_adamw_multi_from_slabs at
    weight decay 0 on the same inputs, its row reports ratio 1; an all-zero weight tensor (segment 1) takes ratio 1 and
    the same bitwise update; the other weights do not."""
    table = torch.tensor([0.05], device=gpu)
    cfg = SGD_CONFIGS["all"]
    zero_w = np.array(L.params_case(1))
    zero_w[:MIXED[1]] = 0
    r = Run(gpu, params={1: zero_w}, lamb=lamb)
    b = _plain({1: zero_w}, gpu, table, lamb, cfg)
    if lamb:
        r.step_lamb(table, 0.01, exclude_bias=True)
    else:
        r.step_lars(table, cfg, exclude_bias=True)      # step 0 overwrites the momentum buffers in both runs
    torch.cuda.synchronize()
    r.check_sentinels()
    for i in r.ids:
        nw = r.nws[i]
        for d in ("p", "s1", "s2"):
            x, y = getattr(r, d)[i][1], getattr(b, d)[i][1]
            assert torch.equal(x[nw:].view(torch.int32), y[nw:].view(torch.int32)), ("bias", d, i)
            if i == 1:
                assert torch.equal(x[:nw].view(torch.int32), y[:nw].view(torch.int32)), ("zero weight", d)
        rows = r.rows(i)
        assert rows[1][2] == 1.0 and rows[1][0] > 0 and rows[1][1] > 0
        if i == 1:
            assert rows[0][0] == 0.0 and rows[0][2] == 1.0
        else:
            assert rows[0][2] != 1.0 and not torch.equal(r.p[i][1][:nw], b.p[i][1][:nw])


@pytest.mark.parametrize("lamb", [False, True], ids=["lars", "lamb"])
def test_a_bias_gets_a_ratio_from_its_own_norms_only(gpu, lamb):
    """exclude_bias=False: changing the weight's parameters leaves the bias's row and update bit for bit."""
    table = torch.tensor([0.05], device=gpu)
    other = np.array(L.params_case(0))
    other[:MIXED[0]] *= 3
    runs = [Run(gpu, groups=((0,),), lamb=lamb), Run(gpu, groups=((0,),), params={0: other}, lamb=lamb)]
    for r in runs:
        if lamb:
            r.step_lamb(table, 0.01, exclude_bias=False)
        else:
            r.step_lars(table, SGD_CONFIGS["all"], exclude_bias=False)
    torch.cuda.synchronize()
    a, b = runs
    nw = MIXED[0]
    assert np.array_equal(a.rows(0)[1], b.rows(0)[1]) and a.rows(0)[1][2] != 1.0
    assert not np.array_equal(a.rows(0)[0], b.rows(0)[0])
    assert torch.equal(a.p[0][1][nw:].view(torch.int32), b.p[0][1][nw:].view(torch.int32))
    want = L.norm64(L.params_case(0)[nw:])
    assert abs(float(a.rows(0)[1][0]) - want) <= L.norm_bound(nblk(0), N) * want


@pytest.mark.parametrize("lamb", [False, True], ids=["lars", "lamb"])
def test_a_group_and_a_tensor_do_not_depend_on_what_shares_the_launch(gpu, lamb):
    """Group {2} alone == group {2} as the second group of a joint launch; segment 1 alone == segment 1 as the second
    segment of group {0, 1}: bit for bit over two steps, rows included."""
    table = torch.tensor([0.05, 0.02], device=gpu)
    runs = [Run(gpu, groups=((2,),), lamb=lamb), Run(gpu, groups=((1,),), lamb=lamb), Run(gpu, lamb=lamb)]
    for r in runs:
        for _ in range(2):
            if lamb:
                r.step_lamb(table, 0.01, exclude_bias=False)
            else:
                r.step_lars(table, SGD_CONFIGS["all"], exclude_bias=False)
        torch.cuda.synchronize()
        r.check_sentinels()
    alone2, alone1, joint = runs
    same_run(alone2, joint, [2], "group alone")
    same_run(alone1, joint, [1], "segment alone")
    for alone, i in ((alone2, 2), (alone1, 1)):
        assert np.array_equal(alone.rows(i), joint.rows(i)) and np.array_equal(alone.seg_partials(i), joint.seg_partials(i))


def test_zero_gradient_gives_ratio_one_and_finite_parameters(gpu):
    zeros = {i: torch.zeros(C.SLAB_COUNTS[i], N, device=gpu) for i in (0, 1, 2)}
    table = torch.tensor([0.05], device=gpu)
    for lamb in (False, True):
        r = Run(gpu, slabs=zeros, lamb=lamb)
        if lamb:
            r.step_lamb(table, 0.0, exclude_bias=False)
        else:
            r.step_lars(table, dict(momentum=0.9, weight_decay=5e-4), exclude_bias=False)
        torch.cuda.synchronize()
        r.check_sentinels()
        for i in r.ids:
            rows = r.rows(i)
            assert rows[0][1] == 0.0 and rows[0][2] == 1.0 and rows[1][2] == 1.0 and rows[0][0] > 0
            assert torch.isfinite(r.p[i][1]).all() and torch.equal(r.g[i][1], torch.zeros(N, device=gpu))


@pytest.mark.parametrize("poison", ["inf", "nan"])
@pytest.mark.parametrize("lamb", [False, True], ids=["lars", "lamb"])
def test_a_non_finite_gradient_stays_in_its_own_tensor(gpu, lamb, poison):
    """A NaN / inf planted in the WEIGHT columns of segment 1's slabs: its bias (the same segment, a straddled block
    where nw is 1100), segment 0 of the same group and group {2} are bit for bit the unpoisoned run."""
    nws = {0: 1100, 1: 1100, 2: 1299}
    bad = slabs_dev(1, gpu).clone()
    bad[5, 1050] = float(poison)
    table = torch.tensor([0.05], device=gpu)
    runs = [Run(gpu, nws=nws, lamb=lamb), Run(gpu, nws=nws, slabs={1: bad}, lamb=lamb)]
    for r in runs:
        if lamb:
            r.step_lamb(table, 0.01, exclude_bias=False)
        else:
            r.step_lars(table, SGD_CONFIGS["all"], exclude_bias=False)
        torch.cuda.synchronize()
        r.check_sentinels()
    clean, dirty = runs
    same_run(clean, dirty, [0, 2], "other segments")
    for d in ("p", "s1", "s2"):
        x, y = getattr(clean, d)[1][1][1100:], getattr(dirty, d)[1][1][1100:]
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("bias of the poisoned segment", d)
    assert np.array_equal(clean.rows(1)[1], dirty.rows(1)[1]) and np.array_equal(clean.rows(0), dirty.rows(0))
    assert not np.isfinite(dirty.rows(1)[0][1]) and not torch.isfinite(dirty.p[1][1][1050])
    assert torch.isfinite(clean.p[1][1]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_invalid_value(gpu):
    """nw > n, nw < 0, null pointers and more than four segments: hipErrorInvalidValue (1), nothing launched."""
    from splitcnn import _lib
    lib = _lib.load()
    P, I = ctypes.c_void_p, ctypes.c_int
    t = [torch.zeros(N, device=gpu) for _ in range(4)]
    sl = torch.zeros(1, N, device=gpu)
    part, out = torch.full((64,), NAN, device=gpu), torch.full((12,), NAN, device=gpu)
    step, table = torch.zeros(1, dtype=torch.int32, device=gpu), torch.tensor([0.1], device=gpu)

    def arr(vals, typ=P):
        return ctypes.cast((typ * len(vals))(*vals), P)

    def calls(nseg=1, nw=1100, null=None, ngroup=1):
        k = max(nseg, 1)
        ptr = lambda name, x: arr([None if null == name else x.data_ptr()] * k)   # noqa: E731
        geo = (arr([1] * k, I), arr([N] * k, I), arr([nw] * k, I), arr([0] * k, I), nseg)
        parts = arr([None if null == "partials" else part.data_ptr()])
        outs = arr([None if null == "out" else out.data_ptr()])
        loss = (None, 0, 0.0, None, 0, None)
        return [
            lib.slk_reduce_tnorm_multi(ptr("grad", t[1]), ptr("param", t[0]), ptr("slabs", sl), *geo, parts, ngroup,
                                       *loss, None),
            lib.slk_lars_multi(ptr("param", t[0]), ptr("grad", t[1]), ptr("state", t[2]), *geo, parts, outs, ngroup,
                               table.data_ptr(), 1, step.data_ptr(), 0.9, 0.0, 0.0, 0, 1e-3, 1e-8, 1, None),
            lib.slk_lamb_moments_multi(ptr("grad", t[1]), ptr("param", t[0]), ptr("state", t[2]), ptr("state", t[3]),
                                       ptr("slabs", sl), *geo, parts, ngroup, step.data_ptr(), 0.9, 0.999, 1e-6, 0.01,
                                       1, *loss, None),
            lib.slk_lamb_multi(ptr("param", t[0]), ptr("state", t[2]), ptr("state", t[3]), *geo, parts, outs, ngroup,
                               table.data_ptr(), 1, step.data_ptr(), 0.9, 0.999, 1e-6, 0.01, 1, None),
        ]

    assert calls(nw=N + 1) == [1, 1, 1, 1]
    assert calls(nw=-1) == [1, 1, 1, 1]
    assert calls(nseg=5) == [1, 1, 1, 1]
    assert calls(nseg=0) == [1, 1, 1, 1]
    assert calls(null="param") == [1, 1, 1, 1]
    assert calls(null="partials") == [1, 1, 1, 1]
    assert calls(null="state") == [0, 1, 1, 1]        # pass 1 of LARS takes no state
    assert calls(null="out")[1::2] == [1, 1]
    assert calls(ngroup=2) == [1, 1, 1, 1]
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and all(float(x.abs().sum()) == 0 for x in t[:1])
