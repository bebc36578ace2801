"""The optimizer kernels' per-element update against float64, element by element (tests/optim_ref64.py): every entry
point on every value class at every counter value up to *step = 2^31 - 2, the bitwise identities at late counters, and
the multi launches' block -> segment walk on segment lists with one-element, block-boundary, mixed-form and zero-length
segments, with and without the loss block, against separate launches; and both trainers resumed at counter 99,999.

What it found: lamb_multi_kernel's fourth segment slot rounded step_size * (m / denom) on its own where the other slots
and slk_adamw_from_slabs fuse it (the compiler had merged the plain line's tail with LAMB's subtraction), so an excluded
bias in a fourth segment of more than 1,024 elements differed from separate launches in its last bit ("mixed" and "empty"
layouts below). csrc/slk_adam.h now names the fused multiply-add.

Slabs hold the gradient exactly: slab 0 is g, the others +0.0, so the sum is g in any order (a -0.0 gradient becomes
+0.0, and the reference is given that). The slab counts are 1, 17 and 65, one per reduction form. Every parameter,
gradient and state buffer has 64 NaNs behind it. Each comparison is per element: inside the derived bound of float64,
or, in the overflow class (both float32 emulations give v = +inf where float64 does not), the emulations' bits.
Clipping coefficients and trust ratios are the values the device wrote (norm_out / trust_out); their own references
are tests/clip_ref.py and tests/layerwise_ref.py. Every test prints its largest error / bound ratio ("RATIO ...")."""
import ctypes

import numpy as np
import pytest
import torch

import head_ref64 as R
import optim_ref64 as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
PAD = 64
P = ctypes.c_void_p
LATE = (99999, 2 ** 31 - 2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(values, dev):
    """A device buffer holding `values` followed by PAD NaNs; returns (buffer, view of the values)."""
    v = torch.from_numpy(np.array(values, dtype=np.float32)).reshape(-1)
    buf = torch.full((v.numel() + PAD,), NAN, dtype=torch.float32, device=dev)
    buf[:v.numel()] = v.to(dev)
    return buf, buf[:v.numel()]


def _nan(n, dev):
    buf = torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev)
    return buf, buf[:n]


def _ints(dev, *vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _host(ctype, vals):
    vals = list(vals)
    return ctypes.cast((ctype * max(len(vals), 4))(*vals), P)


def _ptrs(ts):
    return _host(P, [t.data_ptr() if t is not None else None for t in ts])


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


def _slabs(g, nslab, dev):
    """[nslab, n] with slab 0 = g and +0.0 elsewhere."""
    s = torch.zeros(nslab, len(g), dtype=torch.float32, device=dev)
    s[0] = torch.from_numpy(np.array(g, dtype=np.float32)).to(dev)
    return s


def _table(table, dev):
    return torch.tensor(table, dtype=torch.float32, device=dev)


def _np(t):
    return t.detach().cpu().numpy()


def _sgd_args(cfg):
    return (cfg.get("momentum", 0.0), cfg.get("dampening", 0.0), cfg.get("weight_decay", 0.0),
            int(cfg.get("nesterov", False)))


def _check(ref, bufs, n, what):
    """bufs = {name: (buffer, view)}: sentinels intact, every element inside the bound or the emulations' bits."""
    worst = 0.0
    for name, (buf, view) in bufs.items():
        R.assert_sentinel(buf, n, f"{what} {name}")
        worst = max(worst, ref.check(name, _np(view), what))
    return worst


# ------------------------------------------------------------------------------------------------ from_slabs entries
@pytest.mark.parametrize("step", O.STEPS)
@pytest.mark.parametrize("nslab", O.SLAB_COUNTS)
def test_sgdm_from_slabs_every_class(gpu, nslab, step):
    """slk_sgdm_from_slabs under every configuration. At *step = 0 the buffer starts as NaN and must be overwritten; with
    momentum 0 it keeps its bits; the counter is not written by the launch and slk_tick advances it by exactly one."""
    from splitcnn import _lib
    ctr = _ints(gpu, step, -1)
    worst, overflow = 0.0, 0
    for cn, cfg0 in O.SGD_CONFIGS.items():
        for label, p, g, st, table, cfg in O.launches("sgd", step, cfg0):
            n = len(p)
            g = O.with_pos_zero(g)
            mom = cfg.get("momentum", 0.0) != 0
            pb = _padded(p, gpu)
            bb = _nan(n, gpu) if (mom and step == 0) else _padded(st["buf"], gpu)
            gb = _nan(n, gpu)
            tb, sl = _table(table, gpu), _slabs(g, nslab, gpu)
            _lib.call("slk_sgdm_from_slabs", pb[1].data_ptr(), gb[1].data_ptr(), bb[1].data_ptr(),
                      sl.data_ptr(), nslab, n, tb.data_ptr(), len(table), ctr.data_ptr(),
                      *_sgd_args(cfg), _stream())
            torch.cuda.synchronize()
            ref = O.Ref(lambda A: O.sgdm(A, p, g, st["buf"], step, table, **cfg))
            what = f"slk_sgdm_from_slabs {cn} {label} nslab {nslab} *step {step}"
            bufs = {"p": pb}
            if mom:
                bufs["buf"] = bb
            else:
                _same(bb[0][:n], torch.from_numpy(np.array(st["buf"])), what + ": buf without momentum")
                R.assert_sentinel(bb[0], n, what)
            worst = max(worst, _check(ref, bufs, n, what))
            overflow += int(ref.tainted.sum())
            R.assert_sentinel(gb[0], n, what)
            _same(gb[1], torch.from_numpy(g), what + ": grad")
            assert ctr.tolist() == [step, -1], what
    _lib.call("slk_tick", ctr.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert ctr.tolist() == [step + 1, -1]
    assert overflow == 0
    print(f"RATIO slk_sgdm_from_slabs nslab={nslab} step={step} {worst:.4f} overflow=0")
    assert worst <= 1.0


@pytest.mark.parametrize("step", O.STEPS)
@pytest.mark.parametrize("nslab", O.SLAB_COUNTS)
@pytest.mark.parametrize("entry", ["slk_adam_from_slabs", "slk_adamw_from_slabs"])
def test_adam_from_slabs_every_class(gpu, entry, nslab, step):
    """slk_adam_from_slabs (the rate by value: the table's entry for this counter) and slk_adamw_from_slabs without
    decay, with coupled and with decoupled decay."""
    from splitcnn import _lib
    ctr = _ints(gpu, step, -1)
    worst, overflow = 0.0, 0
    cfgs = {"adam": O.ADAM_CONFIGS["adam"]} if entry == "slk_adam_from_slabs" else O.ADAM_CONFIGS
    for cn, cfg0 in cfgs.items():
        for label, p, g, st, table, cfg in O.launches("adam", step, cfg0):
            n = len(p)
            g = O.with_pos_zero(g)
            pb, mb, vb, gb = _padded(p, gpu), _padded(st["m"], gpu), _padded(st["v"], gpu), _nan(n, gpu)
            sl = _slabs(g, nslab, gpu)     # named: it must outlive the launch
            head = (pb[1].data_ptr(), gb[1].data_ptr(), mb[1].data_ptr(), vb[1].data_ptr(), sl.data_ptr(), nslab, n)
            if entry == "slk_adam_from_slabs":
                _lib.call(entry, *head, O.rate_at(table, step), O.B1, O.B2, O.EPS, ctr.data_ptr(), _stream())
            else:
                tb = _table(table, gpu)
                _lib.call(entry, *head, tb.data_ptr(), len(table), ctr.data_ptr(), O.B1, O.B2, O.EPS,
                          cfg["weight_decay"], int(cfg["decoupled"]), _stream())
            torch.cuda.synchronize()
            ref = O.Ref(lambda A: O.adam(A, p, g, st["m"], st["v"], step, table, **cfg))
            what = f"{entry} {cn} {label} nslab {nslab} *step {step}"
            worst = max(worst, _check(ref, {"p": pb, "m": mb, "v": vb}, n, what))
            overflow += int(ref.tainted.sum())
            R.assert_sentinel(gb[0], n, what)
            _same(gb[1], torch.from_numpy(g), what + ": grad")
            assert ctr.tolist() == [step, -1], what
    _lib.call("slk_tick", ctr.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert ctr.tolist() == [step + 1, -1]
    assert overflow == O.N * len(cfgs), "the overflow class is the squared-overflow class, once per configuration"
    print(f"RATIO {entry} nslab={nslab} step={step} {worst:.4f} overflow={overflow}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ clipped entries
def _class_launches(kind, step, cfg0):
    """One launch per class (a norm or a ratio belongs to one class's values)."""
    for i, c in enumerate(O.CLASSES):
        p, g, st = O.value_class(c, kind)
        table, cfg = O.class_hyper(c, kind, step, cfg0)
        yield c, O.SLAB_COUNTS[i % 3], p, O.with_pos_zero(g), st, table, cfg


def _all_nan(bufs, n, what):
    for name, (buf, view) in bufs.items():
        R.assert_sentinel(buf, n, what)
        assert torch.isnan(view).all(), f"{what} {name}: inf * 0 is NaN in every element"


@pytest.mark.parametrize("step", O.STEPS)
@pytest.mark.parametrize("entry", ["slk_sgdm_clip_multi", "slk_adamw_clip_multi"])
def test_clip_multi_every_class(gpu, entry, step):
    """slk_reduce_sqnorm_multi + the clipped step, one class per launch (the slab count rotates with the class), at
    *max_norm = inf (coef = 1) and at half the class's own norm (coef < 1); the reference takes the coefficient the
    device wrote. The squared-overflow class has an infinite norm: coef = inf / inf = NaN at *max_norm = inf, and every
    output is NaN, as include/slk.h says; at a finite threshold coef = 0 and it runs like any other class."""
    from splitcnn import ops
    sgd = entry == "slk_sgdm_clip_multi"
    kind = "sgd" if sgd else "adam"
    cfgs = {"all": O.SGD_CONFIGS["all"]} if sgd else {k: O.ADAM_CONFIGS[k] for k in ("coupled", "adamw")}
    ctr = _ints(gpu, step, -1)
    worst, overflow = 0.0, 0
    for cn, cfg0 in cfgs.items():
        for c, nslab, p, g, st, table, cfg in _class_launches(kind, step, cfg0):
            n = len(p)
            norm64 = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
            for mx in (float("inf"), O.f32(0.5 * norm64) if np.isfinite(F32(0.5 * norm64)) else O.f32(1.0)):
                pb, gb = _padded(p, gpu), _nan(n, gpu)
                state = {k: _padded(a, gpu) for k, a in st.items()}
                if sgd and step == 0:
                    state["buf"] = _nan(n, gpu)
                part, out = _nan(ops.reduce_sqnorm_nblk(n, nslab), gpu), _nan(2, gpu)
                seg = (pb[1], gb[1], *[state[k][1] for k in (("buf",) if sgd else ("m", "v"))], _slabs(g, nslab, gpu))
                groups = [(part[1], out[1], [seg])]
                mxt, tb = _table([mx], gpu), _table(table, gpu)
                ops.reduce_sqnorm_multi(groups)
                if sgd:
                    ops.sgdm_clip_multi(groups, mxt, tb, ctr[:1], **cfg)
                else:
                    ops.adamw_clip_multi(groups, mxt, tb, ctr[:1], O.B1, O.B2, O.EPS, **cfg)
                torch.cuda.synchronize()
                what = f"{entry} {cn} {c} nslab {nslab} *step {step} max_norm {mx}"
                R.assert_sentinel(out[0], 2, what)
                R.assert_sentinel(part[0], part[1].numel(), what)
                R.assert_sentinel(gb[0], n, what)
                _same(gb[1], torch.from_numpy(g), what + ": grad keeps the unclipped gradient")
                assert ctr.tolist() == [step, -1], what
                coef = float(_np(out[1])[1])
                bufs = {"p": pb, **state}
                if np.isnan(coef):
                    assert c == "squared_overflow" and mx == float("inf"), what
                    _all_nan(bufs, n, what)
                    continue
                assert (coef == 1.0) if mx == float("inf") else (coef < 1.0), (what, coef)
                if sgd:
                    ref = O.Ref(lambda A: O.sgdm(A, p, O.scaled(A, coef, g), st["buf"], step, table, **cfg))
                else:
                    ref = O.Ref(lambda A: O.adam(A, p, O.scaled(A, coef, g), st["m"], st["v"], step, table, **cfg))
                worst = max(worst, _check(ref, bufs, n, what))
                overflow += int(ref.tainted.sum())
    print(f"RATIO {entry} step={step} {worst:.4f} overflow={overflow}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ layer-wise entries
NW = 1100      # weights [0, 1100), bias [1100, 1300): straddles a block in all three forms


@pytest.mark.parametrize("step", O.STEPS)
@pytest.mark.parametrize("entry", ["slk_lars_multi", "slk_lamb_multi"])
def test_layerwise_every_class(gpu, entry, step):
    """slk_reduce_tnorm_multi + slk_lars_multi and slk_lamb_moments_multi + slk_lamb_multi on one [W | b] segment per
    class, the bias excluded: the weight steps at the ratio the device wrote in trust_out, the bias by the plain form."""
    from splitcnn import ops
    lars = entry == "slk_lars_multi"
    kind = "sgd" if lars else "adam"
    cfg0 = O.SGD_CONFIGS["all"] if lars else O.ADAM_CONFIGS["adamw"]
    ctr = _ints(gpu, step, -1)
    worst, overflow = 0.0, 0
    for c, nslab, p, g, st, table, cfg in _class_launches(kind, step, cfg0):
        n = len(p)
        pb, gb = _padded(p, gpu), _nan(n, gpu)
        state = {k: _padded(a, gpu) for k, a in st.items()}
        if lars and step == 0:
            state["buf"] = _nan(n, gpu)
        part, out = _nan(4 * ops.reduce_sqnorm_nblk(n, nslab), gpu), _nan(6, gpu)
        seg = (pb[1], gb[1], *[state[k][1] for k in (("buf",) if lars else ("m", "v"))], _slabs(g, nslab, gpu), NW)
        groups = [(part[1], out[1], [seg])]
        tb = _table(table, gpu)
        wd = cfg["weight_decay"]
        if lars:
            ops.reduce_tnorm_multi(groups)
            ops.lars_multi(groups, tb, ctr[:1], momentum=cfg["momentum"], nesterov=True, weight_decay=wd,
                           trust_coef=1e-3, eps=1e-8, exclude_bias=True)
        else:
            ops.lamb_moments_multi(groups, ctr[:1], O.B1, O.B2, O.EPS, weight_decay=wd, exclude_bias=True)
            ops.lamb_multi(groups, tb, ctr[:1], O.B1, O.B2, O.EPS, weight_decay=wd, exclude_bias=True)
        torch.cuda.synchronize()
        what = f"{entry} {c} nslab {nslab} *step {step}"
        for b, used in ((out, 6), (part, part[1].numel()), (gb, n)):
            R.assert_sentinel(b[0], used, what)
        _same(gb[1], torch.from_numpy(g), what + ": grad")
        assert ctr.tolist() == [step, -1], what
        rows = _np(out[1]).reshape(2, 3)
        assert rows[1, 2] == 1.0, "an excluded bias reports ratio 1"
        ratio, wnorm = float(rows[0, 2]), float(rows[0, 0])
        assert np.isfinite(ratio), (what, rows)
        for sl, bias in ((slice(0, NW), False), (slice(NW, n), True)):
            s = {k: a[sl] for k, a in st.items()}
            if lars:
                ref = O.Ref(lambda A: O.lars(A, p[sl], g[sl], s["buf"], step, table, 1.0 if bias else ratio,
                                             momentum=cfg["momentum"], nesterov=True, weight_decay=0.0 if bias else wd))
            else:
                ref = O.Ref(lambda A: {k: v for k, v in O.lamb(A, p[sl], g[sl], s["m"], s["v"], step, table, ratio,
                                                               weight_decay=wd, plain=bias or wnorm == 0.0).items()
                                       if k != "u"})
            for name in ref.names:
                view = (pb if name == "p" else state[name])[1][sl]
                worst = max(worst, ref.check(name, _np(view), f"{what} {'bias' if bias else 'weight'}"))
            overflow += int(ref.tainted.sum())
        for b in [pb] + list(state.values()):
            R.assert_sentinel(b[0], n, what)
    print(f"RATIO {entry} step={step} {worst:.4f} overflow={overflow}")
    assert worst <= 1.0
    assert overflow == (0 if lars else O.N)


# ------------------------------------------------------------------------------------------------ bitwise identities
def _benign_state(kind, dev):
    p, g, st = O.value_class("benign", kind)
    return p, O.with_pos_zero(g), st


@pytest.mark.parametrize("step", LATE)
@pytest.mark.parametrize("nslab", O.SLAB_COUNTS)
def test_late_identities_adamw_is_adam_and_sgdm_is_sgd(gpu, nslab, step):
    """slk_adamw_from_slabs without decay on a one-entry table == slk_adam_from_slabs, and slk_sgdm_from_slabs plain ==
    slk_sgd_from_slabs, bit for bit at late counters."""
    from splitcnn import _lib
    ctr = _ints(gpu, step)
    p, g, st = _benign_state("adam", gpu)
    n, sl = len(p), _slabs(g, nslab, gpu)
    a = [_padded(p, gpu), _nan(n, gpu), _padded(st["m"], gpu), _padded(st["v"], gpu)]
    b = [_padded(p, gpu), _nan(n, gpu), _padded(st["m"], gpu), _padded(st["v"], gpu)]
    tb = _table([O.ADAM_TABLE[0]], gpu)
    _lib.call("slk_adam_from_slabs", *[x[1].data_ptr() for x in a], sl.data_ptr(), nslab, n, O.ADAM_TABLE[0], O.B1, O.B2,
              O.EPS, ctr.data_ptr(), _stream())
    _lib.call("slk_adamw_from_slabs", *[x[1].data_ptr() for x in b], sl.data_ptr(), nslab, n, tb.data_ptr(), 1,
              ctr.data_ptr(), O.B1, O.B2, O.EPS, 0.0, 1, _stream())
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        _same(x[0], y[0], "adamw without decay vs adam")
    assert not torch.equal(a[0][1].cpu(), torch.from_numpy(np.array(p)))
    p, g, st = _benign_state("sgd", gpu)
    a, b = [_padded(p, gpu), _nan(n, gpu)], [_padded(p, gpu), _nan(n, gpu)]
    tb = _table([O.SGD_TABLE[0]], gpu)
    sl = _slabs(g, nslab, gpu)
    _lib.call("slk_sgd_from_slabs", a[0][1].data_ptr(), a[1][1].data_ptr(), sl.data_ptr(), nslab, n, O.SGD_TABLE[0], _stream())
    _lib.call("slk_sgdm_from_slabs", b[0][1].data_ptr(), b[1][1].data_ptr(), None, sl.data_ptr(), nslab, n, tb.data_ptr(), 1,
              ctr.data_ptr(), 0.0, 0.0, 0.0, 0, _stream())
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        _same(x[0], y[0], "sgdm plain vs sgd")
    assert ctr.tolist() == [step]


@pytest.mark.parametrize("step", LATE)
def test_late_identities_clip_at_inf_and_excluded_bias(gpu, step):
    """At late counters: the clipped entries at *max_norm = inf == the unclipped multi launch, and the layer-wise entries on
    a segment that is all bias (nw = 0, excluded) == the plain multi launch at weight decay 0, bit for bit."""
    from splitcnn import ops
    ctr = _ints(gpu, step)
    inf = _table([float("inf")], gpu)
    for kind in ("sgd", "adam"):
        p, g, st = _benign_state(kind, gpu)
        n, keys = len(p), (("buf",) if kind == "sgd" else ("m", "v"))
        table = _table(O.SGD_TABLE if kind == "sgd" else O.ADAM_TABLE, gpu)
        cfg = O.SGD_CONFIGS["all"] if kind == "sgd" else O.ADAM_CONFIGS["adamw"]
        for nslab in O.SLAB_COUNTS:
            sl = _slabs(g, nslab, gpu)

            def fresh():
                return [_padded(p, gpu), _nan(n, gpu)] + [_padded(st[k], gpu) for k in keys]
            plain, clip, plain0, trust = fresh(), fresh(), fresh(), fresh()
            views = lambda bs: tuple(b[1] for b in bs)  # noqa: E731
            part, out = _nan(4 * ops.reduce_sqnorm_nblk(n, nslab), gpu), _nan(6, gpu)
            cg = [(part[1], out[1][:2], [views(clip) + (sl,)])]
            tg = [(part[1], out[1], [views(trust) + (sl, 0)])]
            if kind == "sgd":
                ops.sgdm_multi_from_slabs([views(plain) + (sl,)], table, ctr, **cfg)
                ops.reduce_sqnorm_multi(cg)
                ops.sgdm_clip_multi(cg, inf, table, ctr, **cfg)
                ops.sgdm_multi_from_slabs([views(plain0) + (sl,)], table, ctr, momentum=cfg["momentum"], nesterov=True)
                ops.reduce_tnorm_multi(tg)
                ops.lars_multi(tg, table, ctr, momentum=cfg["momentum"], nesterov=True, weight_decay=cfg["weight_decay"],
                               exclude_bias=True)
            else:
                ops.adamw_multi_from_slabs([views(plain) + (sl,)], table, ctr, O.B1, O.B2, O.EPS, **cfg)
                ops.reduce_sqnorm_multi(cg)
                ops.adamw_clip_multi(cg, inf, table, ctr, O.B1, O.B2, O.EPS, **cfg)
                ops.adamw_multi_from_slabs([views(plain0) + (sl,)], table, ctr, O.B1, O.B2, O.EPS, weight_decay=0.0)
                ops.lamb_moments_multi(tg, ctr, O.B1, O.B2, O.EPS, weight_decay=cfg["weight_decay"], exclude_bias=True)
                ops.lamb_multi(tg, table, ctr, O.B1, O.B2, O.EPS, weight_decay=cfg["weight_decay"], exclude_bias=True)
            torch.cuda.synchronize()
            for x, y in zip(plain, clip):
                _same(x[0], y[0], f"{kind} clip at inf vs unclipped, nslab {nslab}")
            for x, y in zip(plain0, trust):
                _same(x[0], y[0], f"{kind} excluded bias vs plain, nslab {nslab}")
            assert not torch.equal(plain[0][1].cpu(), torch.from_numpy(np.array(p)))
    assert ctr.tolist() == [step]


# ------------------------------------------------------------------------------------------------ layouts
LAYOUTS = {
    "mixed": [(1, 1), (17, 256), (65, 64), (16, 1025)],
    "edges": [(65, 63), (1, 1024), (17, 257), (64, 1)],
    "three": [(17, 1), (1, 1023), (65, 65)],
    "empty": [(1, 1), (17, 0), (65, 64), (16, 1025)],
}
MULTI = ("sgd", "sgdm", "adam", "adamw", "sgdm_clip", "adamw_clip", "lars", "lamb")
HAS_LOSS = ("sgd", "sgdm", "sgdm_clip", "adamw_clip", "lars", "lamb")
LOSS_N = 300


class Segs:
    """Device state of one segment list: per segment slabs, param, grad and two state blocks, each with its NaN tail; the
    loss values, ring and counters; per segment (its own group) partials and norm / trust outputs."""

    def __init__(self, dev, segs, seed=3):
        from splitcnn import ops
        gen = torch.Generator().manual_seed(seed)
        self.segs, self.dev = segs, dev
        self.slabs, self.p, self.g, self.s1, self.s2, self.part, self.out = [], [], [], [], [], [], []
        for nslab, n in segs:
            # [nslab][n]; at n = 0 one float per slab, never read (an empty tensor would have a NULL pointer)
            self.slabs.append((torch.randn(nslab * max(n, 1), generator=gen) * 1e-2).to(dev))
            self.p.append(_padded((torch.randn(n, generator=gen) * 0.1).numpy(), dev))
            self.g.append(_nan(n, dev))
            self.s1.append(_padded((torch.randn(n, generator=gen) * 1e-2).numpy(), dev))
            self.s2.append(_padded((torch.randn(n, generator=gen) * 1e-2).numpy() ** 2, dev))
            self.part.append(_nan(4 * ops.reduce_sqnorm_nblk(n, nslab), dev))
            self.out.append(_nan(6, dev))
        self.loss = torch.from_numpy(R.exact_values(LOSS_N, 41)).float().to(dev)
        self.ring = torch.full((3 + PAD,), NAN, dtype=torch.float32, device=dev)
        self.lctr = _ints(dev, 7, -1)
        self.step = _ints(dev, 99999, -1)
        self.nw = [n - n // 4 for _, n in segs]
        self.tables = {"sgd": _table(O.SGD_TABLE, dev), "adam": _table(O.ADAM_TABLE, dev)}   # allocated before any capture
        self.mx = _table([0.05], dev)

    def tensors(self):
        ts = [self.ring, self.lctr, self.step]
        for d in (self.p, self.g, self.s1, self.s2, self.part, self.out):
            ts += [b for b, _ in d]
        return ts

    def sentinels(self, what):
        for d in (self.p, self.g, self.s1, self.s2):
            for (buf, view) in d:
                R.assert_sentinel(buf, view.numel(), what)
        for (buf, view) in self.part + self.out:
            R.assert_sentinel(buf, view.numel(), what)
        R.assert_sentinel(self.ring, 3, what)
        assert self.lctr[1].item() == -1 and self.step[1].item() == -1


def _launch(S, entry, ids, loss):
    """One launch of `entry` (two for the clip and layer-wise pairs) over the segments `ids` of S; several ids = the multi
    launch, each segment its own group."""
    from splitcnn import _lib
    k = len(ids)
    col = lambda d: _ptrs([d[i][0] for i in ids])  # noqa: E731  (the buffer: a view of no elements has a NULL pointer)
    slabs = _ptrs([S.slabs[i] for i in ids])
    nslab, ns = _host(ctypes.c_int, [S.segs[i][0] for i in ids]), _host(ctypes.c_int, [S.segs[i][1] for i in ids])
    nw, group = _host(ctypes.c_int, [S.nw[i] for i in ids]), _host(ctypes.c_int, range(k))
    largs = (S.loss.data_ptr(), LOSS_N, 0.25, S.ring.data_ptr(), 3, S.lctr.data_ptr()) if loss else (None, 0, 0.0, None, 0, None)
    st, step = _stream(), S.step.data_ptr()
    tb = S.tables["sgd" if entry in ("sgdm", "sgdm_clip", "lars") else "adam"]
    tab = (tb.data_ptr(), 3, step)
    sg = (O.f32(0.9), 0.0, O.f32(5e-4), 1)
    ad = (O.B1, O.B2, O.EPS, O.f32(0.01))
    mx = S.mx
    if entry == "sgd":
        _lib.call("slk_sgd_multi_from_slabs", col(S.p), col(S.g), slabs, nslab, ns, k, O.SGD_TABLE[1], *largs, st)
    elif entry == "sgdm":
        _lib.call("slk_sgdm_multi_from_slabs", col(S.p), col(S.g), col(S.s1), slabs, nslab, ns, k, *tab, *sg, *largs, st)
    elif entry == "adam":
        _lib.call("slk_adam_multi_from_slabs", col(S.p), col(S.g), col(S.s1), col(S.s2), slabs, nslab, ns, k,
                  O.ADAM_TABLE[0], O.B1, O.B2, O.EPS, step, st)
    elif entry == "adamw":
        _lib.call("slk_adamw_multi_from_slabs", col(S.p), col(S.g), col(S.s1), col(S.s2), slabs, nslab, ns, k, *tab, *ad, 1, st)
    elif entry in ("sgdm_clip", "adamw_clip"):
        _lib.call("slk_reduce_sqnorm_multi", col(S.g), slabs, nslab, ns, group, k, col(S.part), k, *largs, st)
        if entry == "sgdm_clip":
            _lib.call("slk_sgdm_clip_multi", col(S.p), col(S.g), col(S.s1), nslab, ns, group, k, col(S.part), col(S.out), k,
                      mx.data_ptr(), *tab, *sg, st)
        else:
            _lib.call("slk_adamw_clip_multi", col(S.p), col(S.g), col(S.s1), col(S.s2), nslab, ns, group, k, col(S.part),
                      col(S.out), k, mx.data_ptr(), *tab, *ad, 1, st)
    elif entry == "lars":
        _lib.call("slk_reduce_tnorm_multi", col(S.g), col(S.p), slabs, nslab, ns, nw, group, k, col(S.part), k, *largs, st)
        _lib.call("slk_lars_multi", col(S.p), col(S.g), col(S.s1), nslab, ns, nw, group, k, col(S.part), col(S.out), k, *tab,
                  *sg, 1e-3, 1e-8, 1, st)
    elif entry == "lamb":
        _lib.call("slk_lamb_moments_multi", col(S.g), col(S.p), col(S.s1), col(S.s2), slabs, nslab, ns, nw, group, k,
                  col(S.part), k, step, *ad, 1, *largs, st)
        _lib.call("slk_lamb_multi", col(S.p), col(S.s1), col(S.s2), nslab, ns, nw, group, k, col(S.part), col(S.out), k, *tab,
                  *ad, 1, st)
    else:
        raise AssertionError(entry)


def _separate(S, entry, loss):
    """The same step as separate launches: the single-segment entry point where there is one, else the multi entry on one
    segment at a time; slk_loss_log for the loss block. A zero-length segment is left out altogether."""
    from splitcnn import _lib
    st, step = _stream(), S.step.data_ptr()
    tb = S.tables["sgd" if entry == "sgdm" else "adam"]
    for i, (nslab, n) in enumerate(S.segs):
        if n == 0:
            continue
        head = (S.p[i][1].data_ptr(), S.g[i][1].data_ptr())
        tail = (S.slabs[i].data_ptr(), nslab, n)
        if entry == "sgd":
            _lib.call("slk_sgd_from_slabs", *head, *tail, O.SGD_TABLE[1], st)
        elif entry == "sgdm":
            _lib.call("slk_sgdm_from_slabs", *head, S.s1[i][1].data_ptr(), *tail, tb.data_ptr(), 3, step, O.f32(0.9), 0.0,
                      O.f32(5e-4), 1, st)
        elif entry == "adam":
            _lib.call("slk_adam_from_slabs", *head, S.s1[i][1].data_ptr(), S.s2[i][1].data_ptr(), *tail, O.ADAM_TABLE[0], O.B1,
                      O.B2, O.EPS, step, st)
        elif entry == "adamw":
            _lib.call("slk_adamw_from_slabs", *head, S.s1[i][1].data_ptr(), S.s2[i][1].data_ptr(), *tail, tb.data_ptr(), 3, step,
                      O.B1, O.B2, O.EPS, O.f32(0.01), 1, st)
        else:
            _launch(S, entry, [i], False)
    if loss:
        _lib.call("slk_loss_log", S.loss.data_ptr(), LOSS_N, 0.25, S.ring.data_ptr(), 3, S.lctr.data_ptr(), st)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("entry", MULTI)
def test_multi_launch_layouts_bitwise_separate_launches(gpu, entry, layout):
    """Each multi entry over each segment list, with the loss block and (where it has one) without: every buffer, the
    ring and both counters equal the separate launches bit for bit, sentinels intact. Every entry accepts n[s] = 0 (its
    argument check asks n[s] >= 0 only), so the "empty" list must leave the zero-length segment's buffers untouched and
    its neighbours as if it were absent."""
    segs = LAYOUTS[layout]
    for loss in ((True, False) if entry in HAS_LOSS else (False,)):
        multi, sep = Segs(gpu, segs), Segs(gpu, segs)
        before = [t.clone() for t in multi.tensors()]
        _launch(multi, entry, list(range(len(segs))), loss)
        _separate(sep, entry, loss)
        torch.cuda.synchronize()
        what = f"{entry} {layout} loss={loss}"
        multi.sentinels(what)
        for a, b in zip(multi.tensors(), sep.tensors()):
            _same(a, b, what)
        assert multi.lctr.tolist() == [8 if loss else 7, -1] and multi.step.tolist() == [99999, -1]
        changed = sum(not torch.equal(_bits(a), _bits(b)) for a, b in zip(multi.tensors(), before))
        assert changed >= 2 * sum(n > 0 for _, n in segs), what


@pytest.mark.parametrize("entry", ["sgdm", "adamw"])
def test_multi_launch_layout_inside_a_captured_graph(gpu, entry):
    """The "edges" list captured once and replayed twice around a slk_tick == the same two eager launches around a tick."""
    from splitcnn import _lib
    from splitcnn.graphs import capture
    segs = LAYOUTS["edges"]
    ids = list(range(len(segs)))
    loss = entry in HAS_LOSS
    eager, graphed = Segs(gpu, segs), Segs(gpu, segs)
    for S in (eager, graphed):
        S.step[0] = 1          # the tick moves the rate from index 1 to the clamp
    graph, _ = capture(lambda: _launch(graphed, entry, ids, loss), gpu, preserve=graphed.tensors())
    for S, run in ((eager, lambda: _launch(eager, entry, ids, loss)), (graphed, graph.replay)):
        run()
        _lib.call("slk_tick", S.step.data_ptr(), _stream())
        run()
    torch.cuda.synchronize()
    graphed.sentinels(entry)
    for a, b in zip(eager.tensors(), graphed.tensors()):
        _same(a, b, f"{entry} graph replay")
    assert graphed.step.tolist() == [2, -1] and graphed.lctr.tolist() == [9 if loss else 7, -1]


# ------------------------------------------------------------------------------------------------ trainers resumed late
def _resumed_late(make, batches, stages_state, ref_of):
    """One step, optimizer_state() with both counters replaced by 99,999 loaded back, one more step — eager and graphed:
    equal bit for bit, the counters read 100,000, and per stage the parameters and the state are inside the bounds of the
    closed form fed the stage's own grads."""
    out = []
    for graph in (False, True):
        tr = make(graph)
        tr.step(*batches[0])
        torch.cuda.synchronize()
        state = tr.optimizer_state()
        for k in ("client.step", "server.step"):
            state[k] = torch.full_like(state[k], 99999)
        tr.load_optimizer_state(state)
        before = [{k: t.clone() for k, t in s.items()} for s in stages_state(tr)]
        tr.step(*batches[1])
        torch.cuda.synchronize()
        after = stages_state(tr)
        out.append(after)
        for st, b, a in zip((tr.client, tr.server), before, after):
            assert int(st.step_ctr.item()) == 100000
            ref = ref_of({k: _np(t) for k, t in b.items()}, _np(st.grads))
            worst = max(ref.check(name, _np(a[name]), f"graph={graph} {type(st).__name__}") for name in ref.names)
            print(f"RATIO {type(tr).__name__} graph={graph} {type(st).__name__} {worst:.4f}")
            assert not torch.equal(a["p"], b["p"])
    for x, y in zip(out[0], out[1]):
        for k in x:
            _same(x[k], y[k], f"eager vs graphed {k}")


def test_split_trainer_resumed_at_99999(gpu):
    from splitcnn import optim
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import SplitTrainer
    cfg = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
    values = [0.05, 0.02, 0.01]
    data = SyntheticMNIST(7)
    batches = [tuple(t.to(gpu) for t in data.batch(13)) for _ in range(2)]

    def make(graph):
        return SplitTrainer(*init_models(seed=3), device=gpu, graph=graph, optim=optim.SGD(0.05, **cfg),
                            schedule=optim.LRSchedule.from_values(values, gpu))

    def ref_of(b, g):
        table = tuple(O.f32(v) for v in values)
        return O.Ref(lambda A: O.sgdm(A, b["p"], g, b["buf"], 99999, table, momentum=O.f32(0.9), nesterov=True,
                                      weight_decay=O.f32(5e-4)))
    _resumed_late(make, batches, lambda tr: [{"p": s.params, "buf": s.buf} for s in (tr.client, tr.server)], ref_of)


def test_wide_trainer_resumed_at_99999(gpu):
    from splitcnn import optim
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    values = [1e-3, 5e-4, 2.5e-4]
    data = SyntheticCIFAR(9)
    batches = [tuple(t.to(gpu) for t in data.batch(8)) for _ in range(2)]

    def make(graph):
        return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, optim=optim.Adam(1e-3, weight_decay=0.01),
                           schedule=optim.LRSchedule.from_values(values, gpu))

    def ref_of(b, g):
        table = tuple(O.f32(x) for x in values)
        return O.Ref(lambda A: O.adam(A, b["p"], g, b["m"], b["v"], 99999, table, weight_decay=O.f32(0.01), decoupled=True))
    _resumed_late(make, batches, lambda tr: [{"p": s.params, "m": s.m, "v": s.v} for s in (tr.client, tr.server)], ref_of)
