"""tests/optim_ref64.py pinned on the CPU: the closed forms against torch.optim in float64, both float32 emulations
inside the derived bound on every element of every class at every counter value, the overflow class where it belongs,
and every wrong variant outside the bound somewhere.

Which class refuses which wrong variant (test_every_wrong_variant_leaves_the_bound prints the full table with -s; the
share is the largest share of a class's 1,300 elements, over the configurations and counter values, whose
separately-rounded float32 evaluation of the WRONG form lies outside the RIGHT form's bound on p or on the state):

    bias_f32                  p_zero            90 %   (Adam forms, from *step = 1 on: 1 - b2^t loses 9 bits in float32;
                                                        benign 12 %, where p's own rounding hides the rest)
    t_is_step                 every class      100 %   (*step = 0 divides by 1 - b1^0 = 0)
    eps_before_division       eps_dominant     100 %   (squared_underflow, denormal_moments 100 %; benign 22 %)
    decay_after_update        large_decay      100 %   (p_zero 97 %; benign 24 %)
    coupled_for_decoupled     large_decay      100 %   (benign, wide_scales 100 %; p_zero 50 %: its zeros have no decay)
    dampening_on_first_step   every class      100 %   (at *step = 0 only; signed_zeros 33 %: a zero gradient has no
                                                        dampening to see)
    nesterov_old_buffer       benign           100 %   (signed_zeros 70 %)
    decay_after_momentum      large_decay      100 %   (benign 100 %; p_zero 50 %)
    table_at_step_plus_1      every class      100 %   (at *step = 0 and 1; later both read the clamp)
    table_unclamped           every class      100 %   (from *step = 9 on; modelled as an index that wraps)

Known limit: a sqrt or a division that is one ulp off is inside the bound and is not claimed to be caught."""
import numpy as np
import pytest
import torch

import optim_ref64 as O

F64_TOL = 64 * 2.0 ** -53     # a step is under twenty float64 operations; torch's differ from ours in grouping only


def _close64(got, want, scale, what):
    """|got - want| <= F64_TOL * (|want| + scale): scale is the size of the operands the result was cancelled from."""
    err = np.abs(np.asarray(got) - np.asarray(want))
    assert (err <= F64_TOL * (np.abs(want) + scale)).all(), (what, float(err.max()))


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True))


def _torch_sgd(p, g, buf, step, lr, cfg):
    ref = torch.nn.Parameter(_t64(p))
    opt = torch.optim.SGD([ref], lr=lr, momentum=cfg.get("momentum", 0.0), dampening=cfg.get("dampening", 0.0),
                          nesterov=cfg.get("nesterov", False), weight_decay=cfg.get("weight_decay", 0.0), foreach=False)
    if step > 0 and cfg.get("momentum", 0.0) != 0:
        opt.state[ref]["momentum_buffer"] = _t64(buf)
    ref.grad = _t64(g)
    opt.step()
    return ref.detach().numpy(), (opt.state[ref]["momentum_buffer"].numpy() if cfg.get("momentum", 0.0) else None)


def _torch_adam(p, g, m, v, step, lr, cfg):
    ref = torch.nn.Parameter(_t64(p))
    Opt = torch.optim.AdamW if (cfg["decoupled"] and cfg["weight_decay"] != 0) else torch.optim.Adam
    opt = Opt([ref], lr=lr, betas=(O.B1, O.B2), eps=O.EPS, weight_decay=cfg["weight_decay"], foreach=False)
    # a float64 step tensor: a float32 one cannot hold 2^24 + 3
    opt.state[ref] = {"step": torch.tensor(float(step), dtype=torch.float64), "exp_avg": _t64(m), "exp_avg_sq": _t64(v)}
    ref.grad = _t64(g)
    opt.step()
    st = opt.state[ref]
    assert float(st["step"]) == float(step + 1)
    return ref.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


# ------------------------------------------------------------------------------------------------ closed forms == torch
@pytest.mark.parametrize("name", sorted(O.SGD_CONFIGS))
def test_sgd_closed_form_is_torch_five_steps_and_late_counters(name):
    cfg = O.SGD_CONFIGS[name]
    p, g, st = (np.asarray(a, dtype=np.float64) if not isinstance(a, dict) else a for a in O.value_class("benign", "sgd"))
    A = O.Exact()
    pa, ba, pt, bt = p.copy(), None, p.copy(), None
    for k in range(5):           # consecutive steps from zero state, a fresh gradient each
        gk = g * (1.0 + 0.25 * k)
        lr = O.rate_at(O.SGD_TABLE, k)
        out = O.sgdm(A, pa, gk, ba, k, O.SGD_TABLE, **cfg)
        pt, bt = _torch_sgd(pt, gk, bt, k, lr, cfg)
        pa, ba = out["p"], out.get("buf")
        _close64(pa, pt, np.abs(p), ("p", name, k))
        if bt is not None:
            _close64(ba, bt, np.abs(g), ("buf", name, k))
    buf = np.asarray(st["buf"], dtype=np.float64)
    for step in O.STEPS:         # one step from each counter value
        out = O.sgdm(A, p, g, buf, step, O.SGD_TABLE, **cfg)
        wp, wb = _torch_sgd(p, g, buf, step, O.rate_at(O.SGD_TABLE, step), cfg)
        _close64(out["p"], wp, np.abs(p), ("p", name, step))
        if wb is not None:
            _close64(out["buf"], wb, np.abs(g) + np.abs(buf), ("buf", name, step))


@pytest.mark.parametrize("name", sorted(O.ADAM_CONFIGS))
def test_adam_closed_form_is_torch_five_steps_and_late_counters(name):
    cfg = O.ADAM_CONFIGS[name]
    p, g, st = O.value_class("benign", "adam")
    p, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p, g, st["m"], st["v"]))
    A = O.Exact()
    a = [p.copy(), np.zeros_like(p), np.zeros_like(p)]
    t = [x.copy() for x in a]
    for k in range(5):
        gk = g * (1.0 + 0.25 * k)
        out = O.adam(A, a[0], gk, a[1], a[2], k, O.ADAM_TABLE, **cfg)
        a = [out["p"], out["m"], out["v"]]
        t = list(_torch_adam(t[0], gk, t[1], t[2], k, O.rate_at(O.ADAM_TABLE, k), cfg))
        for what, x, y, s in zip("pmv", a, t, (np.abs(p), np.abs(g), g * g)):
            _close64(x, y, s, (what, name, k))
    for step in O.STEPS:
        out = O.adam(A, p, g, m0, v0, step, O.ADAM_TABLE, **cfg)
        want = _torch_adam(p, g, m0, v0, step, O.rate_at(O.ADAM_TABLE, step), cfg)
        for what, y, s in zip("pmv", want, (np.abs(p), np.abs(g) + np.abs(m0), g * g + v0)):
            _close64(out[what], y, s, (what, name, step))


def test_lamb_and_lars_reduce_to_the_plain_forms():
    """At ratio 1 and weight decay 0 LARS is SGD and LAMB's plain line is Adam, in every arithmetic (the identities
    slk_lars_multi / slk_lamb_multi promise for an excluded bias); LAMB's u is layerwise_ref's float64 direction."""
    import layerwise_ref as L
    p, g, st = O.value_class("benign", "sgd")
    for A in (O.Exact(), O.Emu(False), O.Emu(True)):
        a = O.lars(A, p, g, st["buf"], 9, O.SGD_TABLE, 1.0, momentum=O.f32(0.9), nesterov=True)
        b = O.sgdm(A, p, g, st["buf"], 9, O.SGD_TABLE, momentum=O.f32(0.9), nesterov=True)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    p, g, st = O.value_class("benign", "adam")
    for A in (O.Exact(), O.Emu(False), O.Emu(True)):
        a = O.lamb(A, p, g, st["m"], st["v"], 9, O.ADAM_TABLE, 1.0, plain=True)
        b = O.adam(A, p, g, st["m"], st["v"], 9, O.ADAM_TABLE)
        assert all(np.array_equal(a[k], b[k]) for k in b)
    wd = O.f32(0.01)
    out = O.lamb(O.Exact(), p, g, st["m"], st["v"], 999, O.ADAM_TABLE, 1.0, weight_decay=wd)
    u, m1, v1 = L.lamb_direction64(g, st["m"], st["v"], p, 999, O.B1, O.B2, O.EPS, wd)
    _close64(out["u"], u, np.abs(u), "u")
    _close64(out["m"], m1, np.abs(m1), "m")


# ------------------------------------------------------------------------------------------------ emulations in the bound
def _refs(kind):
    cfgs, mk = (O.SGD_CONFIGS, O.sgd_ref) if kind == "sgd" else (O.ADAM_CONFIGS, O.adam_ref)
    for cn, cfg in cfgs.items():
        for cls in O.CLASSES:
            for step in O.STEPS:
                for coef in (None, O.f32(0.37)):
                    yield cn, cls, step, coef, mk(cls, step, cfg, coef=coef)[0]


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_both_emulations_inside_the_bound_and_overflow_class(kind):
    worst = 0.0
    for cn, cls, step, coef, r in _refs(kind):
        for e in r.emu:
            for k in r.names:
                worst = max(worst, r.check(k, e[k], f"{kind} {cn} {cls} step {step} coef {coef} emulation"))
        size = int(r.tainted.sum())
        if cls == "squared_overflow" and kind == "adam":
            assert size == O.N, (cn, step, size)
            assert r.overflow["v"].all() and r.overflow["p"].all() and not r.overflow["m"].all()
            assert np.isposinf(r.emu[0]["v"]).all()
        else:
            assert size == 0, (kind, cn, cls, step, size)
    print(f"{kind}: largest emulation error / bound = {worst:.4f}")
    assert worst <= 1.0


def test_lamb_and_lars_emulations_inside_the_bound():
    worst = 0.0
    for cls in O.CLASSES:
        for step in O.STEPS:
            p, g, st = O.value_class(cls, "adam")
            table, _ = O.class_hyper(cls, "adam", step, {})
            for plain in (False, True):
                r = O.Ref(lambda A: O.lamb(A, p, O.with_pos_zero(g), st["m"], st["v"], step, table, O.f32(0.73),
                                           weight_decay=O.f32(0.01), plain=plain))
                for e in r.emu:
                    worst = max([worst] + [r.check(k, e[k], f"lamb {cls} {step}") for k in r.names])
                assert int(r.tainted.sum()) == (O.N if cls == "squared_overflow" else 0)
            p, g, st = O.value_class(cls, "sgd")
            table, _ = O.class_hyper(cls, "sgd", step, {})
            r = O.Ref(lambda A: O.lars(A, p, O.with_pos_zero(g), st["buf"], step, table, O.f32(0.021), momentum=O.f32(0.9),
                                       nesterov=True, weight_decay=O.f32(5e-4)))
            for e in r.emu:
                worst = max([worst] + [r.check(k, e[k], f"lars {cls} {step}") for k in r.names])
            assert int(r.tainted.sum()) == 0
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ wrong variants
def _share_outside(kind, variant):
    """{class: (largest share of elements outside the right form's bound, config, step)} for one wrong variant."""
    cfgs, mk = (O.SGD_CONFIGS, O.sgd_ref) if kind == "sgd" else (O.ADAM_CONFIGS, O.adam_ref)
    best = {}
    for cn, cfg in cfgs.items():
        for cls in O.CLASSES:
            for step in O.STEPS:
                right, _ = mk(cls, step, cfg)
                with np.errstate(all="ignore"):     # t = 0 divides by zero, in every arithmetic
                    wrong, _ = mk(cls, step, cfg, variant=variant)
                out = np.zeros(O.N, dtype=bool)
                for k in right.names:
                    got = wrong.emu[0][k]
                    out |= ~right.overflow[k] & ~(right.ratio(k, got) <= 1.0)
                    out |= right.overflow[k] & (got.view(np.int32) != right.emu[0][k].view(np.int32))
                share = float(out.mean())
                if share > best.get(cls, (0.0,))[0]:
                    best[cls] = (share, cn, step)
    return best


@pytest.mark.parametrize("variant", O.VARIANTS)
def test_every_wrong_variant_leaves_the_bound(variant):
    kinds = [k for k, vs in (("sgd", O.SGD_VARIANTS), ("adam", O.ADAM_VARIANTS)) if variant in vs]
    assert kinds
    for kind in kinds:
        best = _share_outside(kind, variant)
        for cls, (share, cn, step) in sorted(best.items(), key=lambda kv: -kv[1][0]):
            print(f"{variant:26s} {kind:5s} {cls:18s} {100 * share:5.1f} %  ({cn}, *step = {step})")
        assert best and max(s for s, _, _ in best.values()) >= 0.25, (variant, kind, best)
