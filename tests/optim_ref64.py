"""One optimizer step per element (slk_sgdm_*, slk_adam_*, slk_adamw_*, the two *_clip_multi, slk_lars_multi,
slk_lamb_moments_multi + slk_lamb_multi): float64 closed forms, a derived per-element error bound, two numpy float32
emulations, the value classes and the wrong variants. Test infrastructure only (tests/test_optim_ref64_cpu.py pins it
on the CPU; tests/test_optim_exact_gpu.py uses it on the GPU).

One program, four arithmetics. Each form below (sgdm, adam, lars, lamb) is written ONCE, in the operation order
include/slk.h documents, against an arithmetic object A, and is run four times:

    Exact       float64, no rounding: the closed form (pinned against torch.optim in float64 by the CPU test);
    Emu(False)  float32, every operation rounded on its own;
    Emu(True)   float32, contracted: where the source has a * b + c (or a * b + c * d) the products are exact (a float32
                product is exact in float64) and the sum is rounded once;
    Bound       the closed form's value x of every intermediate together with a bound e on |x~ - x| for the float32
                value x~ of either emulation, or of any mixture of the two (below).

Hyper-parameters arrive already rounded to float32, as the C ABI receives them. Clipping and the trust ratios are scalar
factors in front: the caller passes the coefficient / ratio the device wrote (tests/clip_ref.py and
tests/layerwise_ref.py hold their own references and bounds; nothing of them is restated here).

The forms (fl = one float32 rounding, [..] = contractible):
    rate   lr = table[min(max(*step, 0), len - 1)]
    SGD    d = [g + wd p]                                             (wd != 0)
           buf = d (*step == 0, no dampening: torch's rule)  or  [mom buf + fl(1 - damp) d]      (mom != 0)
           d = [d + mom buf] (Nesterov)  or  buf
           p = [p - lr d]
    Adam   t = *step + 1;  bc1 = 1 - b1^t, bc2 = 1 - b2^t in double
           step_size = fl(lr / bc1);  bc2s = fl(sqrt(bc2))            (one rounding each, double -> float)
           p = fl(p fl(1 - lr wd)) (AdamW: the factor in double, rounded once)  or  g = [g + wd p] (coupled)
           m = [m + fl(1 - b1) fl(g - m)]
           v = [v b2 + fl(g g) fl(1 - b2)]
           denom = fl(fl(fl(sqrt v) / bc2s) + eps)
           p = [p - step_size fl(m / denom)]
    clip   g' = fl(coef g) in front of SGD / Adam (before either weight decay)
    LARS   d = fl(ratio fl(g + fl(wd p)))  (wd = 0: fl(ratio g)), then SGD on d at weight decay 0
    LAMB   m, v as Adam at weight decay 0;  c = fl(m / denom);  u = fl(fl(c fl(1 / bc1)) + fl(wd p));
           p = fl(p - fl(fl(lr ratio) u));  an excluded bias or a tensor of norm 0 takes Adam's last line instead.

The bound (derived, not measured). u = 2^-24 is float32's unit roundoff and D = 2^-149 its denormal spacing. Every
float32 operation satisfies fl(x) = x (1 + d) + h with |d| <= u and |h| <= D (gradual underflow: h = 0 unless the
result is denormal, and then |h| <= D / 2; one D per operation keeps the rule free of case distinctions). With x the
exact value of an operation on exact operands a, b and e_a, e_b the bounds already held for its computed operands:
    rounding        R(x, e) = e + u (|x| + e) + D
    a + b, a - b    R(x, e_a + e_b)
    a b             R(x, |a| e_b + |b| e_a + e_a e_b)
    a / b           R(x, (e_a + |x| e_b) / (|b| - e_b))              (infinite where e_b >= |b|)
    sqrt a          R(x, min(sqrt(e_a), e_a / sqrt(a)))              (|sqrt s - sqrt t| <= sqrt|s - t|, and the mean value)
    (float)x        R(x, 0) for a double rounded to float32 (step_size, bc2s, 1 / bc1, 1 - lr wd)
    [a b + c]       the product's rule, then the sum's: two roundings.
Inputs (p, g, the state, the float32 hyper-parameters) are exact: e = 0. Each rounding of the documented order is thus
counted exactly once, there is no maximum over the tensor, and no constant is chosen: the bound of an output is what
these rules give for that element's own operands. It holds with or without contraction because a contracted [a b + c]
commits only the sum's rounding of an exact product: its error is at most the propagated error plus u |x| + D, which
the two-rounding rule dominates term by term; the same holds for [a b + c d] whichever product the compiler fuses. A
float32 subtraction that happens to be exact (1 - b1, Sterbenz) is still counted: the count follows the order, not
the values. The float64 reference's own error (a few 2^-53 of the same operands) is 2^-29 of these terms and is not
carried. No margin over the count was needed: on every element of every class at every counter value both emulations
stay inside it (tests/test_optim_ref64_cpu.py), the largest ratio of an emulation's error to the bound being
0.9945 for the SGD forms (p, weight decay, benign) and 0.9903 for the Adam forms (p, large decay): the bound is the count
and nothing more, and the test asserts the ratio at 1.

Known limit, written down and not fought: an implementation of sqrt or of the division that is off by one ulp is inside
any honest bound of this kind (the bound grants one u to each) and is not claimed to be caught.

The overflow class. float32 overflows where float64 does not: with |g| ~ 1e20, fl(g g) = +inf, so v = +inf,
denom = +inf, m / denom = 0 and p keeps its bits (AdamW: the decayed p). An element belongs to the class when the two
emulations both give a non-finite output (v) where float64's outputs are all finite; each output of such an element on
which the two emulations agree bit for bit (v = +inf, p) is compared with the emulations bit for bit instead of with
float64. An output the overflow never reached (m, whose two emulations differ by their roundings) stays under the
float64 bound, as does every other element, so no element of any output is left out of both comparisons. The class is
non-empty for the squared-overflow inputs of the Adam-type forms (all 1,300 elements) and empty for every other class;
the SGD-type forms never square the gradient, so their class is empty at 1e20 as well.

Measured on an MI355X (tests/test_optim_exact_gpu.py prints them): see GPU_MEASURED at the end of this module.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
DEN = 2.0 ** -149
N = 1300                       # a partial last block in the 1024-, 256- and 64-column forms
SLAB_COUNTS = (1, 17, 65)      # one per reduction form
STEPS = (0, 1, 9, 999, 6930, 99999, 2 ** 24 + 2, 2 ** 31 - 2)   # *step; *step = 2^31 - 1 is outside the ABI's range
SGD_TABLE = tuple(float(F32(x)) for x in (0.1, 0.05, 0.025))    # index 0, index 1 and the clamp: three numbers
ADAM_TABLE = tuple(float(F32(x)) for x in (1e-3, 5e-4, 2.5e-4))
B1, B2, EPS = (float(F32(x)) for x in (0.9, 0.999, 1e-8))


def f32(x):
    return float(F32(x))


SGD_CONFIGS = {
    "momentum": dict(momentum=f32(0.9)),
    "nesterov": dict(momentum=f32(0.9), nesterov=True),
    "dampening": dict(momentum=f32(0.9), dampening=f32(0.5)),
    "weight_decay": dict(weight_decay=f32(5e-4)),
    "all": dict(momentum=f32(0.9), nesterov=True, weight_decay=f32(5e-4)),
}
ADAM_CONFIGS = {
    "adam": dict(weight_decay=0.0, decoupled=True),
    "coupled": dict(weight_decay=f32(0.01), decoupled=False),
    "adamw": dict(weight_decay=f32(0.01), decoupled=True),
}


# ------------------------------------------------------------------------------------------------ the arithmetics
class Exact:
    """float64 without rounding: the closed form."""
    name = "float64"

    def inp(self, x):
        return np.asarray(x, dtype=np.float64)

    c = inp
    rnd = inp

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def mul(self, a, b):
        return a * b

    def div(self, a, b):
        with np.errstate(all="ignore"):
            return a / b

    def sqrt(self, a):
        return np.sqrt(a)

    def neg(self, a):
        return -a

    def fma(self, a, b, c):
        return a * b + c

    def dot2(self, a, b, c, d):
        return a * b + c * d

    def out(self, a):
        return np.asarray(a, dtype=np.float64)


class Emu:
    """numpy float32; contract=False rounds every operation, contract=True rounds [a b + c] and [a b + c d] once."""

    def __init__(self, contract):
        self.contract = contract
        self.name = "float32 contracted" if contract else "float32 separate"

    def inp(self, x):
        return np.asarray(x, dtype=F32)

    c = inp

    def rnd(self, x):
        return np.asarray(np.float64(x), dtype=F32)

    def _op(self, f, *a):
        with np.errstate(all="ignore"):
            return np.asarray(f(*a), dtype=F32)

    def add(self, a, b):
        return self._op(np.add, a, b)

    def sub(self, a, b):
        return self._op(np.subtract, a, b)

    def mul(self, a, b):
        return self._op(np.multiply, a, b)

    def div(self, a, b):
        return self._op(np.divide, a, b)

    def sqrt(self, a):
        return self._op(np.sqrt, a)

    def neg(self, a):
        return self._op(np.negative, a)

    def fma(self, a, b, c):
        if not self.contract:
            return self.add(self.mul(a, b), c)
        with np.errstate(all="ignore"):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)

    def dot2(self, a, b, c, d):
        if not self.contract:
            return self.add(self.mul(a, b), self.mul(c, d))
        with np.errstate(all="ignore"):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64) * d.astype(np.float64)).astype(F32)

    def out(self, a):
        return np.asarray(a, dtype=F32)


class BV:
    """A closed-form value x with a bound e on the float32 value's distance from it."""
    __slots__ = ("x", "e")

    def __init__(self, x, e):
        self.x, self.e = x, e


def _R(x, e):
    return e + U * (np.abs(x) + e) + DEN


class Bound:
    """The rules of the module docstring."""
    name = "bound"

    def inp(self, x):
        if isinstance(x, BV):
            return x
        x = np.asarray(x, dtype=np.float64)
        return BV(x, np.zeros_like(x))

    c = inp

    def rnd(self, x):
        x = np.asarray(x, dtype=np.float64)
        return BV(x, _R(x, 0.0))

    def add(self, a, b):
        x = a.x + b.x
        return BV(x, _R(x, a.e + b.e))

    def sub(self, a, b):
        x = a.x - b.x
        return BV(x, _R(x, a.e + b.e))

    def mul(self, a, b):
        x = a.x * b.x
        return BV(x, _R(x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e))

    def div(self, a, b):
        with np.errstate(all="ignore"):
            x = a.x / b.x
            room = np.abs(b.x) - b.e
            prop = np.where(room > 0, (a.e + np.abs(x) * b.e) / np.where(room > 0, room, 1.0), np.inf)
        return BV(x, _R(x, prop))

    def sqrt(self, a):
        x = np.sqrt(a.x)
        with np.errstate(all="ignore"):
            prop = np.minimum(np.sqrt(a.e), np.where(x > 0, a.e / np.where(x > 0, x, 1.0), np.inf))
        return BV(x, _R(x, prop))

    def neg(self, a):
        return BV(-a.x, a.e)

    def fma(self, a, b, c):
        return self.add(self.mul(a, b), c)

    def dot2(self, a, b, c, d):
        return self.add(self.mul(a, b), self.mul(c, d))

    def out(self, a):
        return np.broadcast_to(a.e, np.shape(a.x)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the forms
VARIANTS = ("bias_f32", "t_is_step", "eps_before_division", "decay_after_update", "coupled_for_decoupled",
            "dampening_on_first_step", "nesterov_old_buffer", "decay_after_momentum", "table_at_step_plus_1",
            "table_unclamped")
SGD_VARIANTS = VARIANTS[5:]
ADAM_VARIANTS = VARIANTS[:5] + VARIANTS[8:]


def rate_at(table, step, variant=None):
    """lr_table[min(max(*step, 0), len - 1)]. "table_unclamped" is modelled as an index that wraps round the table (what
    an unclamped read returns is whatever lies behind the table; any value but the last entry serves)."""
    i = step + 1 if variant == "table_at_step_plus_1" else step
    if variant == "table_unclamped":
        return float(table[i % len(table)])
    return float(table[min(max(i, 0), len(table) - 1)])


def sgdm(A, p, g, buf, step, table, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, variant=None):
    """torch.optim.SGD's step. Returns {"p": ..., "buf": ...} ("buf" only with momentum)."""
    lr = rate_at(table, step, variant)
    p, d = A.inp(p), A.inp(g)
    late = variant == "decay_after_momentum"
    if weight_decay != 0 and not late:
        d = A.fma(A.c(weight_decay), p, d)
    out = {}
    if momentum != 0:
        omd = A.sub(A.c(1.0), A.c(dampening))
        if step == 0:
            b = A.mul(omd, d) if variant == "dampening_on_first_step" else d
        else:
            b = A.dot2(A.c(momentum), A.inp(buf), omd, d)
        out["buf"] = A.out(b)
        if nesterov:
            d = A.fma(A.c(momentum), A.inp(buf) if variant == "nesterov_old_buffer" else b, d)
        else:
            d = b
    if weight_decay != 0 and late:
        d = A.fma(A.c(weight_decay), p, d)
    out["p"] = A.out(A.fma(A.c(-lr), d, p))
    return out


def _bias(A, step, lr, b1, b2, variant=None):
    """(step_size, bc2s, rbc1) of step t = *step + 1: in double, each rounded to float32 once."""
    t = step if variant == "t_is_step" else step + 1
    if variant == "bias_f32":
        with np.errstate(all="ignore"):
            bc1 = F32(1) - np.power(F32(b1), F32(t), dtype=F32)
            bc2 = F32(1) - np.power(F32(b2), F32(t), dtype=F32)
            return A.c(F32(lr) / bc1), A.c(np.sqrt(bc2, dtype=F32)), A.c(F32(1) / bc1)
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    with np.errstate(all="ignore"):
        return A.rnd(np.float64(lr) / bc1), A.rnd(math.sqrt(bc2)), A.rnd(np.float64(1.0) / bc1)


def _moments(A, g, m, v, b1, b2):
    m1 = A.fma(A.sub(A.c(1.0), A.c(b1)), A.sub(g, m), m)
    v1 = A.dot2(v, A.c(b2), A.mul(g, g), A.sub(A.c(1.0), A.c(b2)))
    return m1, v1


def _denom(A, v1, bc2s, eps, variant=None):
    if variant == "eps_before_division":
        return A.div(A.add(A.sqrt(v1), A.c(eps)), bc2s)
    return A.add(A.div(A.sqrt(v1), bc2s), A.c(eps))


def adam(A, p, g, m, v, step, table, b1=B1, b2=B2, eps=EPS, weight_decay=0.0, decoupled=True, variant=None):
    """torch.optim.Adam (weight_decay 0), Adam(weight_decay) (decoupled False) or AdamW. Returns p, m, v."""
    lr = rate_at(table, step, variant)
    p, g, m, v = A.inp(p), A.inp(g), A.inp(m), A.inp(v)
    if variant == "coupled_for_decoupled":
        decoupled = not decoupled
    factor = None
    if weight_decay != 0:
        if decoupled:
            factor = A.rnd(1.0 - np.float64(lr) * np.float64(weight_decay))
            if variant != "decay_after_update":
                p = A.mul(p, factor)
        else:
            g = A.fma(A.c(weight_decay), p, g)
    step_size, bc2s, _ = _bias(A, step, lr, b1, b2, variant)
    m1, v1 = _moments(A, g, m, v, b1, b2)
    q = A.div(m1, _denom(A, v1, bc2s, eps, variant))
    p = A.fma(A.neg(step_size), q, p)
    if factor is not None and variant == "decay_after_update":
        p = A.mul(p, factor)
    return {"p": A.out(p), "m": A.out(m1), "v": A.out(v1)}


def scaled(A, coef, g):
    """fl(coef g): the clipped gradient, one multiply rounded on its own (never contracted)."""
    return A.mul(A.c(coef), A.inp(g))


def lars(A, p, g, buf, step, table, ratio, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """slk_lars_multi on one tensor at the given ratio (an excluded bias: ratio 1, weight_decay 0)."""
    p, d = A.inp(p), A.inp(g)
    if weight_decay != 0:
        d = A.add(d, A.mul(A.c(weight_decay), p))
    d = A.mul(A.c(ratio), d)
    return sgdm(A, p, d, buf, step, table, momentum=momentum, dampening=dampening, nesterov=nesterov)


def lamb(A, p, g, m, v, step, table, ratio, b1=B1, b2=B2, eps=EPS, weight_decay=0.0, plain=False):
    """slk_lamb_moments_multi + slk_lamb_multi on one tensor at the given ratio. plain: an excluded bias or a tensor of
    norm 0 (Adam's own last line at weight decay 0). Returns p, m, v and u."""
    lr = rate_at(table, step)
    p, g, m, v = A.inp(p), A.inp(g), A.inp(m), A.inp(v)
    step_size, bc2s, rbc1 = _bias(A, step, lr, b1, b2)
    m1, v1 = _moments(A, g, m, v, b1, b2)
    c = A.div(m1, _denom(A, v1, bc2s, eps))
    u = A.mul(c, rbc1)
    if weight_decay != 0 and not plain:
        u = A.add(u, A.mul(A.c(weight_decay), p))
    if plain:
        newp = A.fma(A.neg(step_size), c, p)
    else:
        newp = A.sub(p, A.mul(A.mul(A.c(lr), A.c(ratio)), u))
    return {"p": A.out(newp), "m": A.out(m1), "v": A.out(v1), "u": A.out(u)}


# ------------------------------------------------------------------------------------------------ one evaluation
class Ref:
    """What one step must give: per output the float64 value, the bound and both emulations, and the overflow class."""

    def __init__(self, form, *args, **kw):
        self.want = form(Exact(), *args, **kw)
        self.bound = form(Bound(), *args, **kw)
        self.emu = [form(Emu(False), *args, **kw), form(Emu(True), *args, **kw)]
        names = list(self.want)
        n = max(np.size(self.want[k]) for k in names)
        for d in [self.want, self.bound] + self.emu:
            for k in names:
                d[k] = np.broadcast_to(d[k], (n,)).copy()
        tainted = np.ones(n, dtype=bool) & False
        finite64 = np.ones(n, dtype=bool)
        for k in names:
            tainted |= ~np.isfinite(self.emu[0][k]) & ~np.isfinite(self.emu[1][k])
            finite64 &= np.isfinite(self.want[k])
        self.tainted = tainted & finite64
        self.overflow = {k: self.tainted & (self.emu[0][k].view(np.int32) == self.emu[1][k].view(np.int32))
                         for k in names}
        self.names = names

    def ratio(self, name, got):
        """|got - float64| / bound per element: 0 where got equals float64, inf where got is not finite."""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(all="ignore"):
            err = np.abs(got - self.want[name])
            r = np.where(err == 0, 0.0, err / self.bound[name])
        return np.where(np.isnan(r), np.inf, r)

    def check(self, name, got, what=""):
        """Every element of `got` (float32): inside the bound of float64, or, in the overflow class, the emulations'
        bits. Returns the largest error / bound ratio outside the overflow class (0 if there is none)."""
        got = np.asarray(got, dtype=F32)
        r = self.ratio(name, got)
        ov = self.overflow[name]
        bad = ~ov & ~(r <= 1.0)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what} {name}: {int(bad.sum())} of {bad.size} elements outside the bound; first at {i}: "
                                 f"got {got[i]!r}, float64 {self.want[name][i]!r}, bound {self.bound[name][i]!r}, "
                                 f"emulations {self.emu[0][name][i]!r} / {self.emu[1][name][i]!r}")
        badbits = ov & (got.view(np.int32) != self.emu[0][name].view(np.int32))
        if badbits.any():
            i = int(np.flatnonzero(badbits)[0])
            raise AssertionError(f"{what} {name}: {int(badbits.sum())} elements of the overflow class differ from the "
                                 f"emulations; first at {i}: got {got[i]!r}, want {self.emu[0][name][i]!r}")
        return float(r[~ov].max()) if (~ov).any() else 0.0


# ------------------------------------------------------------------------------------------------ value classes
CLASSES = ("benign", "p_zero", "wide_scales", "eps_dominant", "squared_underflow", "squared_overflow",
           "denormal_moments", "signed_zeros", "zero_rate", "large_decay")


def _signs(rng, n):
    return rng.choice([-1.0, 1.0], n)


def _p_mix(rng, n):
    """Parameters of the classes that say nothing about p: a third 0.1 N(0, 1), a third 1e-6 N(0, 1), a third 0."""
    p = rng.standard_normal(n) * 0.1
    k = np.arange(n) % 3
    return np.where(k == 0, p, np.where(k == 1, p * 1e-5, 0.0))


def value_class(name, kind, n=N):
    """(p, g, state) of one class as float32 arrays; state = {"buf": ...} (kind "sgd") or {"m": ..., "v": ...}
    ("adam"). Fixed seeds: the same values on every call."""
    rng = np.random.default_rng(8800 + CLASSES.index(name))
    g = rng.standard_normal(n) * 1e-2
    p = rng.standard_normal(n) * 0.1
    s1 = rng.standard_normal(n) * 1e-2          # buf or m
    v = (rng.standard_normal(n) * 1e-2) ** 2
    if name == "p_zero":
        # the update is about lr (|g| + |buf|) for SGD and about lr for Adam, at the tables' first rate
        est = SGD_TABLE[0] * (np.abs(g) + np.abs(s1)) if kind == "sgd" else np.full(n, ADAM_TABLE[0])
        near = est * 4.0 ** rng.uniform(-1, 1, n) * _signs(rng, n)
        p = np.where(np.arange(n) % 2 == 0, 0.0, near)
    elif name == "wide_scales":
        s = rng.choice([1e-12, 1e-9, 1e-6, 1.0, 1e6, 1e15], n) * 10.0 ** rng.uniform(-2, 2, n)
        g, s1 = rng.standard_normal(n) * s, rng.standard_normal(n) * s
        v = (rng.standard_normal(n) * s) ** 2
    elif name == "eps_dominant":
        g, s1 = rng.standard_normal(n) * 1e-10, rng.standard_normal(n) * 1e-10
        v = (rng.standard_normal(n) * 1e-10) ** 2
        p = _p_mix(rng, n)
    elif name == "squared_underflow":
        g, s1 = rng.standard_normal(n) * 1e-30, rng.standard_normal(n) * 1e-30
        v = (rng.standard_normal(n) * 1e-19) ** 2
        p = _p_mix(rng, n)
    elif name == "squared_overflow":
        g = 1e20 * 10.0 ** rng.uniform(0, 1, n) * _signs(rng, n)
        s1 = rng.standard_normal(n) * 1e20
        v = (rng.standard_normal(n) * 1e15) ** 2
    elif name == "denormal_moments":
        s1 = rng.integers(1, 2 ** 20, n) * DEN * _signs(rng, n)
        v = rng.integers(0, 2 ** 20, n) * DEN
        g = np.where(np.arange(n) % 2 == 0, rng.integers(1, 2 ** 22, n) * DEN * _signs(rng, n), g)
        p = _p_mix(rng, n)
    elif name == "signed_zeros":
        z = lambda a: np.where(rng.integers(0, 3, n) == 0, a, np.where(rng.integers(0, 2, n) == 0, 0.0, -0.0))  # noqa: E731
        p, g, s1 = z(p), z(g), z(s1)
    p, g, s1, v = (np.asarray(a, dtype=F32) for a in (p, g, s1, v))
    for a in (p, g, s1, v):
        a.setflags(write=False)
    return (p, g, {"buf": s1}) if kind == "sgd" else (p, g, {"m": s1, "v": v})


def class_hyper(name, kind, step, cfg):
    """(table, cfg) a class runs with at counter value `step`: the zero-rate class puts 0 at the table entry this step
    reads, the large-decay class sets weight_decay so that lr * weight_decay = 0.5 at that entry."""
    table = list(SGD_TABLE if kind == "sgd" else ADAM_TABLE)
    i = min(step, len(table) - 1)
    cfg = dict(cfg)
    if name == "zero_rate":
        table[i] = 0.0
    elif name == "large_decay" and cfg.get("weight_decay", 0.0) != 0:
        cfg["weight_decay"] = f32(0.5 / table[i])
    return tuple(table), cfg


def with_pos_zero(g):
    """The gradient the device sees: slab 0 holds g and the others +0.0, so a -0.0 gradient sums to +0.0."""
    g = np.array(g, dtype=F32)
    g[g == 0] = 0.0
    return g


def sgd_ref(name, step, cfg, coef=None, variant=None):
    """Ref of slk_sgdm_* on class `name` (at clip coefficient `coef`); also returns the inputs."""
    p, g, st = value_class(name, "sgd")
    table, cfg = class_hyper(name, "sgd", step, cfg)
    g = with_pos_zero(g)

    def form(A):
        return sgdm(A, p, g if coef is None else scaled(A, coef, g), st["buf"], step, table, variant=variant, **cfg)
    return Ref(form), (p, g, st, table, cfg)


def adam_ref(name, step, cfg, coef=None, variant=None):
    p, g, st = value_class(name, "adam")
    table, cfg = class_hyper(name, "adam", step, cfg)
    g = with_pos_zero(g)

    def form(A):
        return adam(A, p, g if coef is None else scaled(A, coef, g), st["m"], st["v"], step, table, variant=variant,
                    **cfg)
    return Ref(form), (p, g, st, table, cfg)


VALUE_CLASSES = CLASSES[:8]     # the classes that differ in their values only: they can share one launch


def launches(kind, step, cfg):
    """The launches that cover every class at one counter value and configuration: [(label, p, g, state, table, cfg)].
    The eight value classes run concatenated in one launch of 8 * 1,300 elements (again a partial last block in all three
    forms); the zero-rate and large-decay classes need their own table / weight decay and run alone."""
    parts = [value_class(c, kind) for c in VALUE_CLASSES]
    cat = lambda k: np.concatenate([a[2][k] for a in parts])  # noqa: E731
    table, base = class_hyper("benign", kind, step, cfg)
    out = [("values", np.concatenate([a[0] for a in parts]), np.concatenate([a[1] for a in parts]),
            {k: cat(k) for k in parts[0][2]}, table, base)]
    for c in CLASSES[8:]:
        p, g, st = value_class(c, kind)
        t, h = class_hyper(c, kind, step, cfg)
        out.append((c, p, g, st, t, h))
    return out


# Measured on an MI355X by tests/test_optim_exact_gpu.py: the largest |kernel - float64| / bound per entry point over every
# class, counter value, configuration and slab count (the bound is the count and nothing more, so a kernel that rounds
# every operation on its own sits just below 1, as the separately rounded emulation does), and the overflow class: all
# 1,300 elements of "squared_overflow" per configuration for the Adam-type entries (v = +inf, p and v compared with the
# emulations bit for bit), empty for the SGD-type entries. Under clipping that class has an infinite norm: coef is NaN at
# *max_norm = inf (every output NaN, asserted) and 0 at a finite threshold (no overflow left).
GPU_MEASURED = {
    "slk_sgdm_from_slabs": dict(ratio=0.9945, overflow=0),
    "slk_adam_from_slabs": dict(ratio=0.9903, overflow=1300),
    "slk_adamw_from_slabs": dict(ratio=0.9903, overflow=1300),      # per configuration (three of them)
    "slk_sgdm_clip_multi": dict(ratio=0.9946, overflow=0),
    "slk_adamw_clip_multi": dict(ratio=0.9884, overflow=0),
    "slk_lars_multi": dict(ratio=0.9875, overflow=0),
    "slk_lamb_moments_multi + slk_lamb_multi": dict(ratio=0.9906, overflow=1300),
}
