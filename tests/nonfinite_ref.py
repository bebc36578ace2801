"""Test infrastructure: what the K2 convolution-path kernels must write when ONE operand element is NaN, +inf or
-inf — the non-finite rule of include/slk.h ("NaN and +-inf", clauses 1-7) — and what plain torch writes for the same
input. tests/test_nonfinite_ref_cpu.py pins this module on the CPU; tests/test_nonfinite_k2_gpu.py holds every kernel
to it on the exact regimes of tests/test_x3_exact_gpu.py and tests/head_ref64.py, where a finite output must EQUAL
float64.

How a prediction is built. Every op here is bilinear in (a, b) once its selects (ReLU mask, pool routing: clause 5) have
been applied, so with one poisoned element a[p] = v
    op(a, b) = op(a with a[p] = 0, b) + v * op(e_p, b)                     (e_p = the indicator of p)
The first term and L = op(e_p, b) are finite float64 matmuls on finite data (no BLAS is ever handed a NaN); the second is
formed elementwise in IEEE arithmetic and only inside the dense reach, so 0 x NaN = NaN and 0 x inf = NaN exactly where a
product is formed (clause 1) and nowhere else:
    may(P)  = op(e_p, ones)    != 0      the dense reach: every output one of whose products has the poison as a factor
    must(P) = op(e_p, b != 0)  != 0      the outputs it reaches through a nonzero partner
    want    = clean + where(may, v * L, 0)
Outside may(P) an output is clean and equals float64. A kernel that forms every product (every dense MFMA and FMA
kernel) writes `want`, non-finite on all of may(P). A kernel that skips exact zeros (clause 4: the 2:4-sparse weight
gradient) or works in a transform domain (Winograd) is held to  must(P) <= non-finite <= may(P)  with may(P) widened as
its docstring says. Then the epilogue: rule_relu / rule_pool are clause 2's selects, torch_relu / torch_pool are
F.relu / F.max_pool2d, which propagate NaN.

The x3 kernels (clause 3) split a +-inf operand into (+-inf, NaN): x3_value() turns the poison into NaN before the
prediction is formed, so every output in may(P) is NaN before clause 2 applies.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

import head_ref64 as R
from ref64 import dgrad64, route64, routing64, wgrad64

F64 = torch.float64
CODE_NONE = 4
NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the poison set
class Poison(NamedTuple):
    name: str
    value: float
    sample: str     # first | mid | last
    pixel: str      # first | last | inner
    channel: str    # first | last


def _p(value, sample, pixel, channel):
    vn = "nan" if value != value else ("pinf" if value > 0 else "ninf")
    return Poison(f"{vn}-{sample}-{pixel}-{channel}", value, sample, pixel, channel)


# Three values x (first, middle, last sample) x (first, last, interior pixel) x (first, last channel), crossed as a
# Latin square: every value meets every sample and every pixel position, every sample every pixel position, and
# both channels occur with every value.
TABLE = [
    _p(NAN, "first", "inner", "first"), _p(NAN, "mid", "first", "last"), _p(NAN, "last", "last", "first"),
    _p(INF, "first", "last", "last"), _p(INF, "mid", "inner", "first"), _p(INF, "last", "first", "last"),
    _p(-INF, "first", "first", "first"), _p(-INF, "mid", "last", "last"), _p(-INF, "last", "inner", "last"),
]
NAN_ENTRIES = [e for e in TABLE if e.value != e.value]
PINF_ENTRIES = [e for e in TABLE if e.value == INF]


def _sel(which, n):
    return {"first": 0, "mid": n // 2, "last": n - 1, "inner": n // 2}[which]


def place(entry: Poison, shape, batched=True):
    """The element of a tensor of `shape` that `entry` names. Batched [B, C, ...]: sample, channel, then the pixel
    selector on every remaining axis. A weight [Co, Ci, ...]: the channel selector picks Co, the sample selector
    Ci, the pixel selector the taps (or the feature of [10, 9216]). A bias [C]: the channel selector."""
    shape = tuple(shape)
    if batched:
        idx = [_sel(entry.sample, shape[0])]
        if len(shape) > 2:
            idx.append(_sel(entry.channel, shape[1]))
        idx += [_sel(entry.pixel, n) for n in shape[len(idx):]]
        return tuple(idx)
    if len(shape) == 1:
        return (_sel(entry.channel, shape[0]),)
    idx = [_sel(entry.channel, shape[0])]
    if len(shape) > 2:
        idx.append(_sel(entry.sample, shape[1]))
    idx += [_sel(entry.pixel, n) for n in shape[len(idx):]]
    return tuple(idx)


def plant(t, idx, v):
    """A float32-exact copy of t with t[idx] = v."""
    t = t.clone()
    t[idx] = v
    return t


def x3_value(v):
    """Clause 3: an x3 kernel splits +-inf into (+-inf, inf - inf = NaN); every product of either half is NaN."""
    return NAN if math.isinf(v) else v


# ----------------------------------------------------------------------------- the generic prediction
class Pred(NamedTuple):
    want: torch.Tensor    # float64, IEEE non-finites included, BEFORE the epilogue
    must: torch.Tensor    # bool
    may: torch.Tensor     # bool
    clean: torch.Tensor   # float64: the op with the poisoned element replaced by 0


def predict(op, a, b, slot, idx, v):
    """op(a, b) bilinear in float64 (selects already applied to a and b). slot 0 / 1: the poison v sits at a[idx] /
    b[idx]; idx None: a select removed it (clause 5), the result is the clean one."""
    ops = [a.to(F64).clone(), b.to(F64).clone()]
    if idx is None:
        clean = op(*ops)
        none = torch.zeros_like(clean, dtype=torch.bool)
        return Pred(clean, none, none, clean)
    ops[slot][idx] = 0.0
    clean = op(*ops)
    e = torch.zeros_like(ops[slot])
    e[idx] = 1.0
    partner = ops[1 - slot]

    def run(part):
        # minus the part of the output that does not read the poisoned operand at all (a weight gradient's bias
        # columns are sums of the gradient alone): exact, everything here is a small integer
        z = torch.zeros_like(e)
        return op(e, part) - op(z, part) if slot == 0 else op(part, e) - op(part, z)

    lin = run(partner)
    may = run(torch.ones_like(partner)) != 0
    must = run((partner != 0).to(F64)) != 0
    contrib = torch.full_like(lin, float(v)) * lin                      # IEEE: 0 x NaN = 0 x inf = NaN
    want = clean + torch.where(may, contrib, torch.zeros_like(lin))
    return Pred(want, must, may, clean)


def bias_predict(lin_out, bias, idx, v, bdim=1):
    """out = lin_out + bias broadcast on axis bdim, bias[idx] = v: plain IEEE additions."""
    b = bias.to(F64).clone()
    b[idx] = v
    shape = [1] * lin_out.dim()
    shape[bdim] = -1
    want = lin_out + b.reshape(shape)
    may = torch.zeros_like(want, dtype=torch.bool)
    may.select(bdim, idx[0]).fill_(True)
    b0 = bias.to(F64).clone()
    b0[idx] = 0.0
    return Pred(want, may.clone(), may, lin_out + b0.reshape(shape))


# ----------------------------------------------------------------------------- epilogues: clause 2 and torch
def rule_relu(pre):
    """Clause 2: v > 0 ? v : +0. NaN and -inf give +0, +inf stays."""
    return torch.where(pre > 0, pre, torch.zeros_like(pre))


def torch_relu(pre):
    return F.relu(pre)


def rule_pool(pre):
    """Clause 2 on a conv2 pre-activation [B,64,24,24]: (pooled, code). The maximum of the window's values that compare
    greater than 0 (first one wins: ref64.routing64), else +0 with CODE_NONE."""
    code, win = routing64(rule_relu(pre))
    best = win.max(-1).values
    return torch.where(best > 0, best, torch.zeros_like(best)), code


def x3_pool(raw, bias):
    """The x3 forwards' epilogue (csrc/slk_x3.hip pool_piece) on the raw accumulators [B,64,24,24], bias excluded:
    the scan starts at the window's FIRST value and replaces it on a strict `>`, then bias, then clause 2 on that one
    value. A NaN in the first position therefore wins the window (+0, CODE_NONE); a NaN elsewhere is skipped. On
    finite values this is rule_pool(raw + bias)."""
    B = raw.shape[0]
    win = raw.reshape(B, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 64, 12, 12, 4)
    best = win[..., 0].clone()
    idx = torch.zeros(best.shape, dtype=torch.long, device=raw.device)
    for q in range(1, 4):
        bt = win[..., q] > best
        best = torch.where(bt, win[..., q], best)
        idx = torch.where(bt, torch.full_like(idx, q), idx)
    m = best + bias.to(F64)[None, :, None, None]
    pos = m > 0
    return torch.where(pos, m, torch.zeros_like(m)), torch.where(pos, idx, torch.full_like(idx, CODE_NONE))


def torch_pool(pre):
    return F.max_pool2d(F.relu(pre), 2)


def nanpropagating_pool(pre):
    """WRONG variant 1: a ReLU and pool that keep NaN (torch's), with the rule's code convention."""
    p = torch_pool(pre)
    code = rule_pool(torch.nan_to_num(pre, nan=0.0, posinf=INF, neginf=-INF))[1]
    return p, torch.where(torch.isnan(p), torch.zeros_like(code), code)


def amax_ignoring_nan(t):
    """Clause 3: max |t[b]| from 0 with fmaxf, which drops NaN; an infinity stays."""
    a = t.to(F64).abs().reshape(t.shape[0], -1)
    return torch.where(torch.isnan(a), torch.zeros_like(a), a).max(dim=1).values


def amax_counting_nan(t):
    """WRONG variant 3: a maximum that returns NaN for a row holding one."""
    return t.to(F64).abs().reshape(t.shape[0], -1).max(dim=1).values


def route_select(dp, code):
    """Clause 5: the routed conv2 output gradient, a select on the code (ref64.route64)."""
    return route64(dp, code)


def route_multiply(dp, code):
    """WRONG variant 2: the same routing as a multiplication by a 0/1 table (NaN x 0 = NaN leaks through a blocked
    window and into the three unrouted positions of a routed one)."""
    B = code.shape[0]
    onehot = torch.stack([(code.long() == q).to(F64) for q in range(4)], dim=-1)       # B,64,12,12,4
    d = dp.to(F64).reshape(B, 64, 12, 12)[..., None] * onehot
    return d.reshape(B, 64, 12, 12, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 64, 24, 24)


def routed_index(idx, code):
    """dpooled index (b, co, py, px) -> the index of its routed position in dc [B,64,24,24], or None when the code
    blocks it (clause 5)."""
    b, co, py, px = idx
    q = int(code[b, co, py, px])
    if q >= CODE_NONE:
        return None
    return (b, co, 2 * py + q // 2, 2 * px + q % 2)


# ----------------------------------------------------------------------------- K2 ops (bilinear, float64)
def conv1_lin(x, W1):
    return R.conv1_pre(x, W1, torch.zeros(32, dtype=F64, device=x.device))


def conv2_lin(act, W2):
    B = act.shape[0]
    cols = F.unfold(act.to(F64), 3)
    return torch.matmul(W2.to(F64).reshape(64, 288), cols).reshape(B, 64, 24, 24)


def conv2_dgrad_lin(dc, W2):
    return dgrad64(dc.to(F64), W2)


def conv2_wgrad_lin(act, dc):
    dW, db = wgrad64(act.to(F64), dc.to(F64))
    return torch.cat([dW.reshape(-1), db])


def conv1_wgrad_lin(x, gm):
    """[G, 320] slabs of slk_conv1_wgrad from the MASKED cut gradient gm (head_ref64.conv1_wgrad_slabs with the mask
    already applied: act = 1 everywhere)."""
    return R.conv1_wgrad_slabs(x, torch.ones_like(gm, dtype=F64), gm)


def fc_lin(pooled, W3):
    return pooled.to(F64) @ W3.to(F64).T


def fc_dgrad_lin(dl, W3):
    return dl.to(F64) @ W3.to(F64)


def fc_wgrad_lin(dl, pooled):
    return R.fc_wgrad_slabs(dl, pooled)


def widen_planes(mask):
    """may(P) widened to whole [.., H, W] planes: a kernel that stages zero padding and multiplies it (dgrad borders)
    or transforms tiles (Winograd) may carry a poisoned WEIGHT to every pixel of the planes it touches."""
    return mask.flatten(-2).any(-1)[..., None, None].expand_as(mask).clone()


def widen_taps(mask_flat):
    """may(P) of a conv2 weight gradient [18496] widened over the nine taps of each (co, ci): the Winograd filter
    gradient G^T dU G mixes the transform positions (slk_wino.hip wino_filter_grad)."""
    w = mask_flat[:18432].reshape(64, 32, 9).any(-1, keepdim=True).expand(64, 32, 9).reshape(-1)
    return torch.cat([w, mask_flat[18432:]])


# ----------------------------------------------------------------------------- comparisons
def nonfinite(t):
    return ~torch.isfinite(t)


def same_ieee(got, want64):
    """got (f32) == want64 including its non-finites: NaN where want is NaN, the same infinity where it is infinite,
    the same bits elsewhere (+0 for every zero)."""
    want = R.pos_zero(want64)
    gn, wn = torch.isnan(got), torch.isnan(want)
    ok = (gn == wn) & (gn | (got.double() == want))
    zero = ~gn & (got == 0)
    return ok & (~zero | (R.f32_bits(got) == 0))


def assert_ieee(got, want64, what):
    bad = ~same_ieee(got, want64)
    n = int(bad.sum())
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {bad.numel()} values differ from the rule; first at {i}: got "
                             f"{got[i].item()!r}, want {want64[i].item()!r}")


def assert_between(got, pred: Pred, what, may=None, hold_clean=True):
    """must(P) <= non-finite(got) <= may(P), and got == float64 outside may(P) (bit for bit; hold_clean=False: only
    finite there)."""
    may = pred.may if may is None else may
    nf = nonfinite(got)
    miss = pred.must & ~nf
    assert not miss.any(), f"{what}: {int(miss.sum())} outputs of must(P) are finite; first {tuple(miss.nonzero()[0].tolist())}"
    leak = nf & ~may
    assert not leak.any(), f"{what}: {int(leak.sum())} non-finite outputs outside may(P); first {tuple(leak.nonzero()[0].tolist())}"
    if hold_clean:
        bad = ~may & ~same_ieee(got, pred.clean)
        assert not bad.any(), f"{what}: {int(bad.sum())} clean outputs differ from float64; first {tuple(bad.nonzero()[0].tolist())}"


# ----------------------------------------------------------------------------- step level: K2, three SGD steps
K2_TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias")
K2_KEYS = dict(zip(K2_TENSORS, ("W1", "b1", "W2", "b2", "W3", "b3")))

# scenario -> (tensor name or "x", poison value). The element is place()'s for TABLE[0]'s selectors ("first" sample,
# interior pixel, first channel), so every scenario is one line.
SCENARIOS = {
    "clean": (None, 0.0),
    "x-nan": ("x", NAN), "x-pinf": ("x", INF),
    "conv1.weight-nan": ("conv1.weight", NAN), "conv1.bias-nan": ("conv1.bias", NAN),
    "conv2.weight-nan": ("conv2.weight", NAN), "conv2.bias-nan": ("conv2.bias", NAN),
    "fc1.weight-nan": ("fc1.weight", NAN), "fc1.bias-nan": ("fc1.bias", NAN),
    "fc1.weight-pinf": ("fc1.weight", INF),
}


def scenario_index(name, shape):
    return place(TABLE[0], shape, batched=name == "x")


def _inf_to_nan(t):
    return torch.where(torch.isinf(t), torch.full_like(t, NAN), t)


def k2_forward(p, x, preset, rule):
    """logits of the K2 model in float64. rule=False: torch (F.relu, F.max_pool2d). rule=True: clause 2's selects; with
    preset "x3" also clause 3 (an infinite act or W2 enters conv2 as NaN) and the x3 forwards' first-position scan."""
    pre1 = F.conv2d(x, p["W1"], p["b1"])
    if not rule:
        h = F.max_pool2d(F.relu(F.conv2d(F.relu(pre1), p["W2"], p["b2"])), 2)
        return h.flatten(1) @ p["W3"].T + p["b3"]
    act, W2 = rule_relu(pre1), p["W2"]
    if preset == "x3":
        act, W2 = _inf_to_nan(act), _inf_to_nan(W2)
    raw = F.conv2d(act, W2)
    v = rule_relu(raw + p["b2"][None, :, None, None])
    if preset == "x3":
        first = torch.isnan(raw[:, :, 0::2, 0::2])
        v = torch.where(first.repeat_interleave(2, 2).repeat_interleave(2, 3), torch.zeros_like(v), v)
    pooled = F.max_pool2d(v, 2)
    if preset == "x3" and pooled.requires_grad:
        pooled.register_hook(_inf_to_nan)           # an infinite dpooled splits like any x3 operand
    return pooled.flatten(1) @ p["W3"].T + p["b3"]


def k2_steps(params, batches, preset="x3", rule=True, lr=0.01, clip=None):
    """Plain-SGD steps of the K2 model over `batches` [(x, y)], float64 autograd. Returns one record per step:
    loss (float), `bad` = the parameter tensors holding a non-finite value AFTER the step and `whole` = those
    with no finite value left; and the final parameters.
    clip: max_norm of a per-stage global-norm clip (client = conv1.*, server = the rest), torch's clip_grad_norm_."""
    p = {k: params[k].to(F64).clone().requires_grad_(True) for k in K2_KEYS.values()}
    out = []
    for x, y in batches:
        loss = F.cross_entropy(k2_forward(p, x.to(F64), preset, rule), y)
        grads = dict(zip(p, torch.autograd.grad(loss, list(p.values()))))
        with torch.no_grad():
            for stage in (("W1", "b1"), ("W2", "b2", "W3", "b3")):
                coef = 1.0
                if clip is not None:
                    norm = torch.sqrt(sum((grads[k] ** 2).sum() for k in stage))
                    coef = clip / (norm + 1e-6)
                    coef = torch.where(coef > 1, torch.ones_like(coef), coef)      # a NaN norm keeps a NaN coef
                for k in stage:
                    p[k] -= lr * (coef * grads[k])
        out.append(dict(loss=float(loss.detach()),
                        bad={t for t, k in K2_KEYS.items() if not torch.isfinite(p[k]).all()},
                        whole={t for t, k in K2_KEYS.items() if not torch.isfinite(p[k]).any()}))
    return out, {k: v.detach() for k, v in p.items()}


def k2_eval_loss(params, x, y, preset="x3", rule=True):
    with torch.no_grad():
        return float(F.cross_entropy(k2_forward({k: v.to(F64) for k, v in params.items()}, x.to(F64), preset, rule), y))


# ----------------------------------------------------------------------------- step level: K5, three Adam steps
K5_TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc.weight",
              "fc.bias")
K5_SCENARIOS = {
    "clean": (None, 0.0), "x-nan": ("x", NAN), "x-pinf": ("x", INF),
    **{f"{t}-nan": (t, NAN) for t in K5_TENSORS}, "fc.weight-pinf": ("fc.weight", INF),
}
K5_P_DROP = 0.25


def k5_keep(seed, step, B, device="cpu"):
    """The head's dropout mask of one step, bool [B, 16384] in flatten order (head_ref64.keep_mask)."""
    return torch.from_numpy(R.keep_mask(seed, step, B, K5_P_DROP, b0=0)).to(device)


def k5_forward(p, x, keep, rule):
    """logits of the widened model in float64 (padding 1 everywhere). keep: the dropout mask, or None in evaluation.
    rule=True: clause 2's selects, and dropout as a select (clause 7: a dropped non-finite feature is 0); rule=False:
    torch (F.relu, F.max_pool2d, a multiplying dropout mask, which keeps a NaN)."""
    relu = rule_relu if rule else F.relu
    a1 = relu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"], padding=1))
    p2 = F.max_pool2d(relu(F.conv2d(a1, p["conv2.weight"], p["conv2.bias"], padding=1)), 2)
    cut = F.max_pool2d(relu(F.conv2d(p2, p["conv3.weight"], p["conv3.bias"], padding=1)), 2).flatten(1)
    if keep is not None:
        scale = 1.0 / (1.0 - K5_P_DROP)
        cut = torch.where(keep, cut * scale, torch.zeros_like(cut)) if rule else cut * keep.to(F64) * scale
    return cut @ p["fc.weight"].T + p["fc.bias"]


def k5_steps(params, batches, seed=0, rule=True, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """Adam steps (torch.optim.Adam's arithmetic) of the widened model over `batches`, float64 autograd, the dropout mask
    of step s = k5_keep(seed, s, B). One record per step: loss, `bad` = the tensors holding a non-finite value after it."""
    p = {k: params[k].to(F64).clone().requires_grad_(True) for k in K5_TENSORS}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    out = []
    for s, (x, y) in enumerate(batches):
        keep = k5_keep(seed, s, x.shape[0], x.device)
        loss = F.cross_entropy(k5_forward(p, x.to(F64), keep, rule), y)
        grads = dict(zip(p, torch.autograd.grad(loss, list(p.values()))))
        with torch.no_grad():
            for k in p:
                m[k] = betas[0] * m[k] + (1 - betas[0]) * grads[k]
                v2[k] = betas[1] * v2[k] + (1 - betas[1]) * grads[k] ** 2
                mh, vh = m[k] / (1 - betas[0] ** (s + 1)), v2[k] / (1 - betas[1] ** (s + 1))
                p[k] -= lr * mh / (vh.sqrt() + eps)
        out.append(dict(loss=float(loss.detach()), bad={t for t in K5_TENSORS if not torch.isfinite(p[t]).all()}))
    return out
