"""GPU: every K2 convolution-path entry point called ALONE with one NaN, +inf or -inf planted in one operand, held to
the non-finite rule of include/slk.h ("NaN and +-inf", clauses 1-7) as tests/nonfinite_ref.py states it, and to float64
wherever the rule leaves an output finite. Operands come from the exact regimes (tests/test_x3_exact_gpu.py's integers,
tests/head_ref64.py's), so a finite output must EQUAL float64: no tolerance anywhere. Outputs are prefilled with NaN
(codes and images with 0xFF) and carry one extra sample (or slab) of sentinel behind the last row.

Every (kernel, table entry, operand) is launched twice: with the poison, and with the poisoned element put back to its
finite value. Asserted:
  a. clause 6: every sample other than the poisoned one is bit for bit the clean launch's (which the rule's prediction,
     float64 there, also pins);
  b. in the poisoned sample the rule's prediction: a dense kernel writes exactly IEEE's value after clause 2 / 5's
     selects (nonfinite_ref.predict); a kernel that skips zeros or works in a transform domain keeps
     must(P) <= non-finite <= may(P) and float64 outside may(P);
  c. code bytes in {0, 1, 2, 3, CODE_NONE}; ReLU bit maps and act16 images agree with the f32 values beside them;
  d. slabs: columns of must(P) non-finite in the slabs' sum, columns outside may(P) == float64 and bit for bit the clean
     launch's in EVERY slab (so a slab the poisoned sample does not feed is untouched);
  e. interchangeable kernels agree bit for bit (NaNs as NaNs).

Batches: B = 3 (ragged slab counts: conv2_wgrad_nslab(3) = 9) and B = 17 (one sample past the 16-per-workgroup forms
and the 16-slab reduction form). The table (nonfinite_ref.TABLE, 9 entries) is crossed with each kernel's operands.

Sentences the GPU tests rest on beyond clauses 1-7, each read from the code:
  * x3 forwards: the window scan starts at the window's first raw accumulator with a strict `>`
    (csrc/slk_x3.hip pool_piece), so a NaN there blanks the window; a NaN in another position is skipped
    (nonfinite_ref.x3_pool).
  * Winograd (csrc/slk_wino.hip): +-inf meets inf - inf in B^T d B / G g G^T / A^T m A, so inside may(P) (all nine
    taps of a weight gradient: G^T dU G mixes them) an infinity may arrive as NaN, i.e. as +0 / CODE_NONE after
    clause 2 in a forward; only the invariants of clause 2 are asserted there. A NaN operand gives the direct kernel's
    result, in the forward and in the input gradient.
  * x3 with +-inf (clause 3): an infinite maximum moves the sample's scale to 2^0 and, in the weight gradients, a
    launch-wide one (csrc/slk_x3.hip conv2_wgrad_x3 `ma`, `md`: the maxima over all per-sample maxima); outputs outside
    may(P) are then only asserted finite, as the rule says. For a NaN poison they equal float64.
"""
import math

import pytest
import torch

import head_ref64 as R
import nonfinite_ref as N
from ref64 import route64
from test_x3_exact_gpu import _assert_bound, _exact_case, encode_relu_bits

pytestmark = pytest.mark.gpu

BATCHES = [3, 17]
IDS = [e.name for e in N.TABLE]
F32 = torch.float32


def _f32(t):
    return t.to(F32).contiguous()


def _buf(shape, dev, dtype=F32):
    """An output with one extra leading row of sentinel: NaN floats, 0xFF bytes, -1 ints."""
    full = (shape[0] + 1,) + tuple(shape[1:])
    if dtype == F32:
        return torch.full(full, float("nan"), dtype=F32, device=dev)
    return torch.full(full, 0xFF if dtype == torch.uint8 else -1, dtype=dtype, device=dev)


def _done(buf, rows, what):
    torch.cuda.synchronize()
    used = rows * (buf.numel() // buf.shape[0])
    R.assert_sentinel(buf, used, what)
    return buf[:rows]


def _bits_equal(a, b):
    if a.dtype == F32:
        return torch.equal(R.f32_bits(a), R.f32_bits(b))
    return torch.equal(a, b)


def _same(a, b):
    """Equal with NaNs compared as NaNs (two kernels may write different NaN payloads)."""
    if a.dtype != F32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(R.f32_bits(torch.where(na, torch.zeros_like(a), a)),
                                               R.f32_bits(torch.where(nb, torch.zeros_like(b), b)))


def _others(B, b):
    return [s for s in range(B) if s != b]


def _assert_codes(code, what):
    assert bool((code <= N.CODE_NONE).all()), f"{what}: a code byte outside 0..4"


def _assert_pool(pooled, code, want_p, want_c, what):
    _assert_codes(code, what)
    N.assert_ieee(pooled, want_p, what + " pooled")
    bad = code.long() != want_c
    assert not bad.any(), f"{what}: {int(bad.sum())} codes differ from the rule; first {tuple(bad.nonzero()[0].tolist())}"


def _poisoned(tensors, name, idx, v):
    """(poisoned, clean) f32 operand dicts."""
    clean = {k: _f32(t) for k, t in tensors.items()}
    bad = dict(clean)
    bad[name] = N.plant(clean[name], idx, v)
    return bad, clean


# ============================================================================ conv1 forward
def _rule_cut_bound(x, W1, b1):
    """conv1_cut_bound (csrc/slk_common.h) with its fmaxf's: max|x| ignores NaN, sum |W1[c]| and the fma are IEEE,
    max(b1, 0) and the maximum over channels ignore NaN (clause 3)."""
    xm = N.amax_ignoring_nan(x)
    ws = W1.double().abs().reshape(32, 9).sum(1)
    bc = torch.where(torch.isnan(b1.double()), torch.zeros_like(ws), b1.double().clamp_min(0.0))
    v = ws[None, :] * xm[:, None] + bc[None, :]
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).max(dim=1).values.to(F32)


def _decode_act16(a16, B):
    """act16 bytes -> (h, l) float64 [B,32,26,26], unscaled (include/slk.h: per sample an h plane then an l plane,
    [676 pixels][32 ci] f16, 8-channel chunk c8 at slot c8 ^ (x & 2))."""
    img = a16.view(torch.float16).reshape(B, 2, 26, 26, 4, 8)
    sw = img[:, :, :, :, [2, 3, 0, 1], :]
    odd = ((torch.arange(26, device=a16.device) & 2) != 0)[None, None, None, :, None, None]
    img = torch.where(odd, sw, img).reshape(B, 2, 26, 26, 32).permute(0, 1, 4, 2, 3)
    return img[:, 0].double(), img[:, 1].double()


def _x3_scale(amax):
    """2^s of x3_exp: amax * 2^s in [2^13, 2^14); 2^0 for a zero or non-finite amax."""
    a = amax.double()
    _, e = torch.frexp(torch.where(torch.isfinite(a) & (a > 0), a, torch.ones_like(a)))
    s = torch.where(torch.isfinite(a) & (a > 0), 14 - e, torch.zeros_like(e)).clamp_max(126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=a.device), s.double())


def _assert_images(a16, amax, act, what):
    """The images hold act: h * 2^-s == act exactly in the exact regime (a non-finite act as itself), l == 0 where act is
    finite and NaN where it is not (inf - inf)."""
    B = act.shape[0]
    h, l = _decode_act16(a16, B)
    sc = _x3_scale(amax)[:, None, None, None]
    N.assert_ieee((h / sc).to(F32), act.double(), what + " h plane")
    fin = torch.isfinite(act)
    assert bool((l[fin] == 0).all()) and bool(torch.isnan(l[~fin]).all()), what + " l plane"


def _run_conv1(dev, o, kind):
    from splitcnn import ops
    B = o["x"].shape[0]
    act, am = _buf((B, 32, 26, 26), dev), _buf((B,), dev)
    out = {}
    if kind == "fwd":
        ops.conv1_fwd(o["x"], o["W1"], o["b1"], out=act[:B])
    elif kind == "amax":
        ops.conv1_fwd(o["x"], o["W1"], o["b1"], out=act[:B], act_amax=am[:B])
        out["amax"] = _done(am, B, "act_amax")
    else:
        nb = ops.conv2_act16_bytes(B)
        a16 = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device=dev)
        bits = _buf((B, ops.RELU_BITS_WORDS), dev, torch.int32)
        ops.conv1_fwd_x3(o["x"], o["W1"], o["b1"], am[:B], a16[:nb], act=act[:B], relu_bits=bits[:B])
        out["amax"] = _done(am, B, "act_amax")
        out["bits"] = _done(bits, B, "relu_bits")
        R.assert_sentinel(a16, nb, "act16")
        out["a16"] = a16[:nb]
    out["act"] = _done(act, B, "act")
    return out


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_conv1_forwards(gpu, B, entry):
    """slk_conv1_fwd, slk_conv1_fwd_amax, slk_conv1_fwd_x3 with the poison in x, W1, b1: act == the rule's IEEE value
    after clause 2 everywhere; act_amax == conv1_cut_bound with NaN ignored (clause 3); relu_bits == act > 0; the images
    hold act. Clause 6 for a poisoned x. The three entries agree bit for bit."""
    x, W1, b1 = R.conv1_int_case(B, 7000 + B, gpu)
    t = dict(x=x, W1=W1, b1=b1)
    lin = N.conv1_lin(x, W1)
    for name in ("x", "W1", "b1"):
        idx = N.place(entry, t[name].shape, batched=name == "x")
        if name == "b1":
            pre = N.bias_predict(lin, b1, idx, entry.value).want
        else:
            pre = N.predict(N.conv1_lin, x, W1, 0 if name == "x" else 1, idx, entry.value).want + \
                b1.double()[None, :, None, None]
        want = N.rule_relu(pre)
        bad, clean = _poisoned(t, name, idx, entry.value)
        outs = {k: _run_conv1(gpu, bad, k) for k in ("fwd", "amax", "x3")}
        ref = _run_conv1(gpu, clean, "x3")
        what = f"conv1 {name} {entry.name} B={B}"
        for k, o in outs.items():
            N.assert_ieee(o["act"], want, f"{what} {k}")
            assert _same(o["act"], outs["fwd"]["act"])
            if name == "x":
                for s in _others(B, idx[0]):
                    assert _bits_equal(o["act"][s], ref["act"][s]), f"{what} {k}: sample {s} changed (clause 6)"
        bound = _rule_cut_bound(bad["x"], bad["W1"], bad["b1"])
        for k in ("amax", "x3"):
            assert _bits_equal(outs[k]["amax"], bound), f"{what} {k}: act_amax {outs[k]['amax'].tolist()} != {bound.tolist()}"
        assert torch.equal(outs["x3"]["bits"], encode_relu_bits(want > 0)), f"{what}: relu_bits != act > 0"
        _assert_images(outs["x3"]["a16"], outs["x3"]["amax"], outs["x3"]["act"], what)
        if name == "x":
            nb1 = outs["x3"]["a16"].numel() // B
            for s in _others(B, idx[0]):
                assert torch.equal(outs["x3"]["a16"][s * nb1:(s + 1) * nb1], ref["a16"][s * nb1:(s + 1) * nb1])
                assert torch.equal(outs["x3"]["bits"][s], ref["bits"][s])


# ============================================================================ conv1 weight gradient
def _run_c1w(dev, x, act, W1, b1, g, remask):
    from splitcnn import ops
    B = x.shape[0]
    n = ops.conv1_wgrad_nslab(B)
    slabs = _buf((n, 320), dev)
    if remask:
        ops.conv1_wgrad_remask_slabs(x, W1, b1, g, slabs=slabs[:n])
    else:
        ops.conv1_wgrad_slabs(x, act, g, slabs=slabs[:n])
    return _done(slabs, n, "conv1 wgrad slabs")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_conv1_wgrads(gpu, B, entry):
    """slk_conv1_wgrad and _remask with the poison in x, in W1 / b1 (which only the mask reads: act is the rule's
    forward of the same operands), and in the cut gradient at a position the mask passes and at one it blocks
    (clause 5: the blocked launch is bit for bit the clean one). Every slab == the rule's IEEE value; the two entries
    agree; slabs of other sample ranges are the clean launch's."""
    x, W1, b1 = R.conv1_int_case(B, 7200 + B, gpu)
    g = R.cut_grad_int(B, 7300 + B, gpu)
    t = dict(x=x, W1=W1, b1=b1, g=g)
    ranges = R.conv1_ranges(B)
    for name in ("x", "W1", "b1", "g_pass", "g_block"):
        key = name.split("_")[0]
        idx = N.place(entry, t[key].shape, batched=key in ("x", "g"))
        bad, clean = _poisoned(t, key, idx, entry.value)
        xp, W1p, b1p = (bad[k].double() for k in ("x", "W1", "b1"))
        # the forward under the rule, from the poisoned operands (IEEE elementwise: head_ref64.conv1_pre)
        if key in ("x", "W1"):
            pre = N.predict(N.conv1_lin, x, W1, 0 if key == "x" else 1, idx, entry.value).want + b1p[None, :, None, None]
        else:
            pre = N.conv1_lin(x, W1) + b1p[None, :, None, None]
        act = N.rule_relu(pre)
        if key == "g":       # choose the mask at the poisoned position through b1-free means: move the poison
            want_pass = name == "g_pass"
            cand = ((act[idx[0], idx[1]] > 0) == want_pass).nonzero()
            assert len(cand), "no such position in this plane"
            d = (cand - torch.tensor(idx[2:], device=gpu)).abs().sum(1)
            idx = (idx[0], idx[1]) + tuple(cand[d.argmin()].tolist())
            bad, clean = _poisoned(t, key, idx, entry.value)
        mask = act > 0
        gm = torch.where(mask, g.double(), torch.zeros_like(act))
        if key == "x":
            pred = N.predict(N.conv1_wgrad_lin, x, gm, 0, idx, entry.value)
        elif key == "g":
            pred = N.predict(N.conv1_wgrad_lin, x, gm, 1, idx if name == "g_pass" else None, entry.value)
        else:
            pred = N.predict(N.conv1_wgrad_lin, x, gm, 1, None, entry.value)
        what = f"conv1 wgrad {name} {entry.name} B={B}"
        if name == "g_pass":
            assert pred.must.any(), what + ": must(P) is empty"
        elif name == "x":    # a NaN pixel blocks its own reach in the mask, so it meets zeros only: 0 x NaN (clause 1)
            assert pred.may.any() and N.nonfinite(pred.want).any(), what + ": may(P) is empty"
        actf = act.to(F32)
        got = {rm: _run_c1w(gpu, bad["x"], actf, bad["W1"], bad["b1"], bad["g"], rm) for rm in (False, True)}
        ref = _run_c1w(gpu, clean["x"], None, clean["W1"], clean["b1"], clean["g"], True)   # remask: act is not read
        for rm, s in got.items():
            N.assert_ieee(s, pred.want, f"{what} remask={rm}")
        assert _same(got[False], got[True]), what + ": slk_conv1_wgrad and _remask disagree"
        if key in ("x", "g"):
            for r, (lo, hi) in enumerate(ranges):
                if not lo <= idx[0] < hi:
                    assert _bits_equal(got[True][r], ref[r]), f"{what}: slab {r} changed (clause 6)"
        if name == "g_block":
            assert _bits_equal(got[True], ref) and _bits_equal(got[False], ref), what + ": a blocked gradient leaked"


# ============================================================================ conv2 forwards
X3_FWD = ("x3", "x3s", "x3sa", "x3i", "x3p")


def _run_fwd(dev, kind, o, amax=None, a16_in=None):
    """One conv2 forward alone -> dict(pooled, code?, a16?, amax?)."""
    from splitcnn import ops
    B = o["b"]
    pooled, code = _buf((B, 64, 12, 12), dev), _buf((B, 64, 12, 12), dev, torch.uint8)
    out = {}
    nb = ops.conv2_act16_bytes(B)
    if kind in ("wino", "direct"):
        ops.conv2_fwd_pool(o["act"], o["W2"], o["b2"], pooled=pooled[:B], code=code[:B], impl=kind)
    elif kind == "x3":
        ops.conv2_fwd_pool(o["act"], o["W2"], o["b2"], pooled=pooled[:B], code=code[:B], impl="x3", act_amax=amax)
    elif kind in ("x3s", "x3sa"):
        a16 = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device=dev)
        if kind == "x3s":
            ops.conv2_fwd_pool(o["act"], o["W2"], o["b2"], pooled=pooled[:B], code=code[:B], impl="x3", act_amax=amax,
                               act16=a16[:nb])
        else:
            am = _buf((B,), dev)
            ops.conv2_fwd_pool(o["act"], o["W2"], o["b2"], pooled=pooled[:B], code=code[:B], impl="x3", act16=a16[:nb],
                               act_amax_out=am[:B])
            out["amax"] = _done(am, B, "act_amax")
        torch.cuda.synchronize()
        R.assert_sentinel(a16, nb, "act16")
        out["a16"] = a16[:nb]
    elif kind == "x3i":
        ops.conv2_fwd_pool_x3i(a16_in, amax, o["W2"], o["b2"], pooled=pooled[:B], code=code[:B])
    else:
        ops.conv2_fwd_pool_x3p(a16_in, amax, o["W2"], o["b2"], pooled=pooled[:B])
    out["pooled"] = _done(pooled, B, "pooled")
    if kind != "x3p":
        out["code"] = _done(code, B, "code")
    return out


def _win_may(may_pix):
    """pixel-level may(P) [B,64,24,24] -> window level [B,64,12,12]."""
    B = may_pix.shape[0]
    return may_pix.reshape(B, 64, 12, 2, 12, 2).any(5).any(3)


def _weak_pool(pooled, code, pre, want_p, want_c, may_w, what):
    """Winograd with +-inf: float64 outside may(P); inside, clause 2's invariants — never NaN, never negative, +0 exactly
    with CODE_NONE, and a routed value is either +inf or the value IEEE gives the pixel its code names (`pre`, a
    finite pixel of the window that the infinity did not reach)."""
    _assert_codes(code, what)
    bad = ~may_w & ~(N.same_ieee(pooled, want_p) & (code.long() == want_c))
    assert not bad.any(), f"{what}: {int(bad.sum())} windows outside may(P) differ from float64"
    assert not torch.isnan(pooled).any() and bool((pooled >= 0).all()), what + ": NaN or negative pooled value"
    none = code == N.CODE_NONE
    assert torch.equal(none, R.f32_bits(pooled) == 0), what + ": CODE_NONE and +0 disagree"
    B = pre.shape[0]
    win = pre.reshape(B, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 64, 12, 12, 4)
    named = win.gather(-1, code.long().clamp_max(3)[..., None])[..., 0]
    ok = none | torch.isinf(pooled) | (pooled.double() == named)
    assert ok.all(), f"{what}: {int((~ok).sum())} routed values are neither +inf nor the named pixel's"


@pytest.mark.parametrize("B", [1] + BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_conv2_forwards(gpu, B, entry):
    """slk_conv2_fwd_pool, _direct and the five x3 forwards with the poison in act, W2, b2.
    direct: pooled / code == IEEE's pre-activation under rule_pool. Winograd: the same for a NaN and for any b2 (the
    bias enters every output of its channel once); weak invariants for +-inf in act / W2 (module docstring). x3: the
    poison as x3_value() (b2 is added in f32 and keeps its infinity), raw accumulators under x3_pool; the five agree
    bit for bit; x3sa's act_amax ignores NaN; the images hold act. Clause 6 for a poisoned act."""
    c = _exact_case(gpu, B, seed=7400 + B)
    t = dict(act=c["act"], W2=c["W2"], b2=c["b2"])
    _assert_bound(N.conv2_lin(t["act"].abs(), t["W2"].abs()) + t["b2"].abs().double()[None, :, None, None])
    lin = N.conv2_lin(t["act"], t["W2"])
    from splitcnn import ops
    for name in ("act", "W2", "b2"):
        idx = N.place(entry, t[name].shape, batched=name == "act")
        bad, clean = _poisoned(t, name, idx, entry.value)
        bad["b"] = clean["b"] = B
        what = f"conv2 fwd {name} {entry.name} B={B}"
        b2d = bad["b2"].double()[None, :, None, None]
        raws = {}
        for fam, v in (("f32", entry.value), ("x3", N.x3_value(entry.value))):
            if name == "b2":
                raws[fam] = (lin, None)
            else:
                p = N.predict(N.conv2_lin, t["act"], t["W2"], 0 if name == "act" else 1, idx, v)
                if fam == "f32":
                    assert p.must.any(), what + ": must(P) is empty"
                raws[fam] = (p.want, p.may)
        # ---- f32
        raw, may = raws["f32"]
        want_p, want_c = N.rule_pool(raw + b2d)
        d = _run_fwd(gpu, "direct", bad)
        _assert_pool(d["pooled"], d["code"], want_p, want_c, what + " direct")
        w = _run_fwd(gpu, "wino", bad)
        if name == "b2" or math.isnan(entry.value):
            _assert_pool(w["pooled"], w["code"], want_p, want_c, what + " wino")
            assert _same(w["pooled"], d["pooled"]) and torch.equal(w["code"], d["code"])
        else:
            _weak_pool(w["pooled"], w["code"], raw + b2d, want_p, want_c, _win_may(may), what + " wino")
        # ---- x3
        raw, _ = raws["x3"]
        want_p, want_c = N.x3_pool(raw, bad["b2"].double())
        am = ops.row_amax(bad["act"])
        assert _bits_equal(am, N.amax_ignoring_nan(bad["act"]).to(F32)), what + ": slk_row_amax"
        x = {"x3": _run_fwd(gpu, "x3", bad, am), "x3s": _run_fwd(gpu, "x3s", bad, am), "x3sa": _run_fwd(gpu, "x3sa", bad)}
        x["x3i"] = _run_fwd(gpu, "x3i", bad, am, x["x3s"]["a16"])
        x["x3p"] = _run_fwd(gpu, "x3p", bad, am, x["x3s"]["a16"])
        for k, o in x.items():
            N.assert_ieee(o["pooled"], want_p, f"{what} {k} pooled")
            assert _same(o["pooled"], x["x3"]["pooled"]), f"{what}: {k} and x3 disagree"
            if k != "x3p":
                _assert_pool(o["pooled"], o["code"], want_p, want_c, f"{what} {k}")
        assert _bits_equal(x["x3sa"]["amax"], am), what + ": x3sa act_amax"
        assert torch.equal(x["x3sa"]["a16"], x["x3s"]["a16"])
        _assert_images(x["x3s"]["a16"], am, bad["act"], what + " x3s")
        # ---- clause 6
        if name == "act" and B > 1:
            refs = {"direct": _run_fwd(gpu, "direct", clean), "wino": _run_fwd(gpu, "wino", clean),
                    "x3": _run_fwd(gpu, "x3", clean, ops.row_amax(clean["act"]))}
            for k, got in (("direct", d), ("wino", w), ("x3", x["x3"])):
                for s in _others(B, idx[0]):
                    assert _bits_equal(got["pooled"][s], refs[k]["pooled"][s]) and \
                        torch.equal(got["code"][s], refs[k]["code"][s]), f"{what} {k}: sample {s} changed (clause 6)"


# ============================================================================ received cut -> images
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_cut_unpack_x3(gpu, B, entry):
    """slk_cut_unpack_x3 on a received (codec-encoded) cut holding the poison: the images slk_conv2_fwd_pool_x3s writes
    from the same dense cut and act_amax, every byte; other samples' images are the clean cut's."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    c = _exact_case(gpu, B, seed=7500 + B)
    idx = N.place(entry, c["act"].shape)
    bad, clean = _poisoned(dict(act=c["act"]), "act", idx, entry.value)
    nb = ops.conv2_act16_bytes(B)
    imgs = {}
    for tag, act in (("bad", bad["act"]), ("clean", clean["act"])):
        am = ops.row_amax(act)
        codec = CutCodec()
        n = act.numel()
        bufs = codec.buffers("t", n, gpu)
        codec.encode(act, bufs)
        ranks = codec.ranks("t", n, bufs)
        a16 = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device=gpu)
        ops.cut_unpack_x3(bufs[4], bufs[0], ranks, am, a16[:nb])
        torch.cuda.synchronize()
        R.assert_sentinel(a16, nb, "act16")
        imgs[tag] = a16[:nb]
        if tag == "bad":
            o = dict(act=act, W2=_f32(c["W2"]), b2=_f32(c["b2"]), b=B)
            assert torch.equal(a16[:nb], _run_fwd(gpu, "x3s", o, am)["a16"]), f"unpack_x3 {entry.name}: images differ"
            _assert_images(a16[:nb], am, act, f"unpack_x3 {entry.name}")
    per = nb // B
    for s in _others(B, idx[0]):
        assert torch.equal(imgs["bad"][s * per:(s + 1) * per], imgs["clean"][s * per:(s + 1) * per])


# ============================================================================ conv2 input gradient
def _run_dgrad(dev, kind, o, dpa=None):
    from splitcnn import ops
    B = o["dp"].shape[0]
    out = _buf((B, 32, 26, 26), dev)
    ops.conv2_dgrad(o["dp"], o["code"], o["W2"], out=out[:B], impl=kind, dp_amax=dpa)
    return _done(out, B, "cut_grad")


def _run_dgrad_pack(dev, o, dpa, cut):
    """slk_conv2_dgrad_x3_pack against the mask of `cut`, unpacked to a dense tensor (zeros off the mask)."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    B, n = cut.shape[0], cut.numel()
    codec = CutCodec()
    bufs = codec.buffers("p", n, dev)
    codec.encode(cut, bufs)
    ranks = codec.ranks("p", n, bufs)
    total = int(bufs[3].item())
    vals = torch.full((n + 64,), float("nan"), dtype=F32, device=dev)
    ops.conv2_dgrad_x3_pack(o["dp"], o["code"], o["W2"], dpa, bufs[0], ranks, vals[:n])
    torch.cuda.synchronize()
    R.assert_sentinel(vals, n, "packed cut gradient")
    assert bool(torch.isnan(vals[total:n]).all()), "a packed value landed past the mask's count"
    dense = torch.empty_like(cut)
    codec.unpack(dense, bufs, vals[:n])
    torch.cuda.synchronize()
    return dense


def _run_c1w_fused(dev, o, dpa):
    from splitcnn import ops
    B = o["dp"].shape[0]
    n = ops.conv2_dgrad_c1w_nslab(B)
    slabs = _buf((n, 320), dev)
    ops.conv2_dgrad_client_slabs(o["dp"], o["code"], o["W2"], o["x"], o["bits"], dp_amax=dpa, slabs=slabs[:n])
    return _done(slabs, n, "client slabs")


def _c1_cols(mask_cut, relu):
    """cut-gradient mask [B,32,26,26] -> the client gradient's columns [320] its ReLU-passed part feeds: all nine taps
    and the bias of every channel with one such pixel."""
    ch = (mask_cut & relu).flatten(2).any(2).any(0)
    return torch.cat([ch[:, None].expand(32, 9).reshape(-1), ch])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_conv2_dgrads(gpu, B, entry):
    """slk_conv2_dgrad (Winograd), _direct, _x3, _x3_pack and the cut-gradient half of _x3_c1w with the poison in
    dpooled — once under a routing code and once under CODE_NONE, where clause 5 makes every launch bit for bit the
    clean one — and in W2.
    direct, dpooled: the cut gradient == IEEE's. Every other case: must(P) <= non-finite <= may(P) and float64 outside
    may(P) (x3 with +-inf: finite outside; clause 3), with may(P) widened, for a poisoned weight, to the whole planes
    of its input channel (border pixels multiply staged zero padding). Winograd's cut gradient is non-finite exactly
    where the direct kernel's is (its window expansion is a bit-mask AND), and equals it for a NaN.
    x3, the packed form (on the mask of a cut) and the fused client backward see the same pattern; clause 6 for a
    poisoned dpooled."""
    c = _exact_case(gpu, B, seed=7600 + B)
    W2, x, relu = c["W2"], c["x"], c["relu"]
    bits = encode_relu_bits(relu)
    from splitcnn import ops
    for name in ("dp_routed", "dp_blocked", "W2"):
        key = name.split("_")[0]
        t = dict(dp=c["dp"], W2=W2)
        idx = N.place(entry, t[key].shape, batched=key == "dp")
        code = c["code"].clone()
        if key == "dp":
            if name == "dp_blocked":
                code[idx] = N.CODE_NONE
            elif int(code[idx]) == N.CODE_NONE:
                code[idx] = 2
        bad, clean = _poisoned(t, key, idx, entry.value)
        for o in (bad, clean):
            o.update(code=code, x=_f32(x), bits=bits)
        dc = route64(c["dp"], code)
        _assert_bound(N.conv2_dgrad_lin(dc.abs(), W2.abs()))
        what = f"conv2 dgrad {name} {entry.name} B={B}"
        isnan = math.isnan(entry.value)

        def pred_for(v):
            if key == "dp":
                return N.predict(N.conv2_dgrad_lin, dc, W2, 0, N.routed_index(idx, code), v)
            p = N.predict(N.conv2_dgrad_lin, dc, W2, 1, idx, v)
            return p._replace(may=N.widen_planes(p.may))
        pf, px = pred_for(entry.value), pred_for(N.x3_value(entry.value))
        if name != "dp_blocked":
            assert pf.must.any(), what + ": must(P) is empty"
        else:
            assert not pf.may.any()
        # ---- f32
        d = _run_dgrad(gpu, "direct", bad)
        if key == "dp":
            N.assert_ieee(d, pf.want, what + " direct")
        else:
            N.assert_between(d, pf, what + " direct")
        w = _run_dgrad(gpu, "wino", bad)
        N.assert_between(w, pf, what + " wino")
        if key == "dp":      # the direct kernel's reach exactly (a NaN as NaN; an infinity may meet inf - inf and be NaN)
            assert torch.equal(N.nonfinite(w), N.nonfinite(d)), what + ": Winograd and direct reach differ"
            if isnan:
                assert _same(w, d), what + ": Winograd and direct dgrad disagree"
        # ---- x3
        dpa = ops.row_amax(bad["dp"])
        assert _bits_equal(dpa, N.amax_ignoring_nan(bad["dp"]).to(F32))
        g = _run_dgrad(gpu, "x3", bad, dpa)
        N.assert_between(g, px, what + " x3", hold_clean=isnan)
        cut = _f32(c["act"])
        gp = _run_dgrad_pack(gpu, bad, dpa, cut)
        assert _same(gp, torch.where(cut != 0, g, torch.zeros_like(g))), what + ": packed and dense x3 dgrad disagree"
        # the fused client backward: the same cut gradient under the ReLU bits, times x, summed over the batch
        s = _run_c1w_fused(gpu, bad, dpa)
        sref = _run_c1w_fused(gpu, clean, ops.row_amax(clean["dp"]))
        nf = N.nonfinite(s).any(0)
        cols_g = _c1_cols(N.nonfinite(g), relu)
        must_c, may_c = _c1_cols(px.must, relu), _c1_cols(px.may, relu)
        assert not (nf & ~may_c).any(), what + " c1w: non-finite columns outside may(P)"
        db = torch.arange(320, device=gpu) >= 288
        assert bool(nf[must_c & db].all()), what + " c1w: a db1 column of must(P) is finite"
        assert torch.equal(nf[db], cols_g[db]), what + " c1w: db1's pattern differs from the dense x3 dgrad's"
        if isnan:
            assert _bits_equal(s[:, ~may_c], sref[:, ~may_c]), what + " c1w: clean columns changed"
            gm = torch.where(relu, px.clean, torch.zeros_like(px.clean))
            from test_x3_exact_gpu import _c1_ref64
            assert torch.equal(s.double().sum(0)[~may_c], _c1_ref64(x, gm)[~may_c]), what + " c1w: clean columns != float64"
        # ---- clause 5 / 6
        refs = {"direct": _run_dgrad(gpu, "direct", clean), "wino": _run_dgrad(gpu, "wino", clean),
                "x3": _run_dgrad(gpu, "x3", clean, ops.row_amax(clean["dp"]))}
        for k, got in (("direct", d), ("wino", w), ("x3", g)):
            if name == "dp_blocked":
                assert _bits_equal(got, refs[k]), f"{what} {k}: a blocked gradient leaked (clause 5)"
            elif key == "dp":
                for smp in _others(B, idx[0]):
                    assert _bits_equal(got[smp], refs[k][smp]), f"{what} {k}: sample {smp} changed (clause 6)"
        if name == "dp_blocked":
            assert _bits_equal(s, sref), what + " c1w: a blocked gradient leaked (clause 5)"


# ============================================================================ conv2 weight gradient
def _run_wgrad(dev, kind, o, am=None, dpa=None, a16=None):
    from splitcnn import ops
    B = o["dp"].shape[0]
    impl = "x3" if kind.startswith("x3") else kind
    n = ops.conv2_wgrad_nslab(B, impl=impl)
    slabs = _buf((n, 18496), dev)
    if kind == "x3s":
        ops.conv2_wgrad_slabs(None, o["dp"], o["code"], slabs=slabs[:n], impl="x3", act_amax=am, dp_amax=dpa, act16=a16)
    else:
        ops.conv2_wgrad_slabs(o["act"], o["dp"], o["code"], slabs=slabs[:n], impl=impl, act_amax=am, dp_amax=dpa)
    return _done(slabs, n, "conv2 wgrad slabs")


def _assert_slabs(s, sref, pred, may, what, hold_clean):
    nf = N.nonfinite(s).any(0)
    miss = pred.must & ~nf
    assert not miss.any(), f"{what}: {int(miss.sum())} columns of must(P) are finite; first {int(miss.nonzero()[0])}"
    leak = nf & ~may
    assert not leak.any(), f"{what}: {int(leak.sum())} non-finite columns outside may(P); first {int(leak.nonzero()[0])}"
    if hold_clean:
        assert torch.equal(s.double().sum(0)[~may], pred.clean[~may]), what + ": clean columns != float64"
        assert _bits_equal(s[:, ~may], sref[:, ~may]), what + ": a clean column changed in some slab"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_conv2_wgrads(gpu, B, entry):
    """slk_conv2_wgrad (Winograd, on the narrow operands its exact regime needs), _direct, _x3 and _x3s with the poison
    in act and in dpooled (under a routing code, and under CODE_NONE: clause 5, bit for bit the clean launch).
    Columns of must(P) are non-finite in the slabs' sum, no column outside may(P) is, and those equal float64 and the
    clean launch's in every slab. may(P) is the dense reach (clause 4: slk_conv2_wgrad_x3s, on the 2:4-sparse MFMA,
    skips exact zeros of dY and may leave a column of may(P) \\ must(P) finite), widened over the nine taps for
    Winograd. x3 / x3s with +-inf: an infinite per-sample maximum enters the launch-wide maxima `ma` / `md`
    (csrc/slk_x3.hip conv2_wgrad_x3_kernel and conv2_wgrad_x3s's prologue, "maximum over all per-sample maxima"), so
    columns outside may(P) are held to finiteness only (clause 3); for NaN they equal float64. x3 and x3s show the
    same pattern on must(P) and outside may(P)."""
    from splitcnn import ops
    wide = _exact_case(gpu, B, seed=7700 + B)
    narrow = _exact_case(gpu, B, seed=7800 + B, narrow=True, small_grad=True)
    isnan = math.isnan(entry.value)
    for name in ("act", "dp_routed", "dp_blocked"):
        key = name.split("_")[0]
        for regime, c, kinds in (("wide", wide, ("direct", "x3", "x3s")), ("narrow", narrow, ("wino",))):
            t = dict(act=c["act"], dp=c["dp"])
            idx = N.place(entry, t[key].shape)
            code = c["code"].clone()
            if key == "dp":
                if name == "dp_blocked":
                    code[idx] = N.CODE_NONE
                elif int(code[idx]) == N.CODE_NONE:
                    code[idx] = 2
            else:     # an activation meets a routed gradient somewhere in its 3 x 3 reach, so must(P) is not empty
                b, _, y, xx = idx
                code[b, 0, min(y, 23) // 2, min(xx, 23) // 2] = 2 * (min(y, 23) % 2) + min(xx, 23) % 2
                t["dp"] = N.plant(t["dp"], (b, 0, min(y, 23) // 2, min(xx, 23) // 2), 3.0)
            bad, clean = _poisoned(t, key, idx, entry.value)
            for o in (bad, clean):
                o.update(code=code, W2=_f32(c["W2"]), b2=_f32(c["b2"]), b=B)
            dc = route64(t["dp"], code)
            _assert_bound(N.conv2_wgrad_lin(t["act"].abs(), dc.abs()))
            if regime == "narrow":     # the Winograd weight gradient's transform-domain bound (test_x3_exact_gpu)
                patch = torch.nn.functional.avg_pool2d(t["act"].double().abs(), 4, stride=2) * 16
                routed = torch.where(code < 4, t["dp"].double().abs(), torch.zeros_like(t["dp"], dtype=torch.float64))
                _assert_bound(4 * torch.einsum("bot,bct->oc", routed.reshape(B, 64, 144), patch.reshape(B, 32, 144)),
                              2.0 ** 20)
            what = f"conv2 wgrad {name} {entry.name} {regime} B={B}"

            def pred_for(v):
                if key == "act":
                    return N.predict(N.conv2_wgrad_lin, t["act"], dc, 0, idx, v)
                return N.predict(N.conv2_wgrad_lin, t["act"], dc, 1, N.routed_index(idx, code), v)
            pf, px = pred_for(entry.value), pred_for(N.x3_value(entry.value))
            if name != "dp_blocked":
                assert pf.must.any(), what + ": must(P) is empty"
            got = {}
            for kind in kinds:
                if kind.startswith("x3"):
                    am, dpa = ops.row_amax(bad["act"]), ops.row_amax(bad["dp"])
                    amc, dpc = ops.row_amax(clean["act"]), ops.row_amax(clean["dp"])
                    a16 = a16c = None
                    if kind == "x3s":
                        a16 = _run_fwd(gpu, "x3s", bad, am)["a16"]
                        a16c = _run_fwd(gpu, "x3s", clean, amc)["a16"]
                    s = _run_wgrad(gpu, kind, bad, am, dpa, a16)
                    sref = _run_wgrad(gpu, kind, clean, amc, dpc, a16c)
                    _assert_slabs(s, sref, px, px.may, f"{what} {kind}", hold_clean=isnan)
                else:
                    s, sref = _run_wgrad(gpu, kind, bad), _run_wgrad(gpu, kind, clean)
                    may = N.widen_taps(pf.may) if kind == "wino" else pf.may
                    _assert_slabs(s, sref, pf, may, f"{what} {kind}", hold_clean=True)
                got[kind] = s
                if name == "dp_blocked":
                    assert _bits_equal(s, sref), f"{what} {kind}: a blocked gradient leaked (clause 5)"
            if "x3" in got:
                a, b_ = (N.nonfinite(got[k]).any(0) for k in ("x3", "x3s"))
                sure = px.must | ~px.may
                assert torch.equal(a[sure], b_[sure]), what + ": x3 and x3s disagree"


# ============================================================================ fc kernels
def _fc_ops(B, seed, dev):
    pooled, W3, b3 = R.fc_int_case(B, seed, dev)
    dl = R.dlogits_int(B, seed + 1, dev)
    return dict(pooled=pooled, W3=W3, b3=b3, dl=dl)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_fc_kernels(gpu, B, entry):
    """slk_fc_fwd (poison in pooled, W3, b3), slk_fc_dgrad / _amax (dlogits, W3), slk_fc_wgrad (dlogits, pooled) and
    slk_fc_backward (all three): dense f32 FMA chains, so every output == IEEE's value (clause 1); dp_amax ignores NaN and
    keeps an infinity (clause 3); slk_fc_backward writes what the separate entries write; clause 6 for the batched
    operands."""
    from splitcnn import ops
    t = _fc_ops(B, 7900 + B, gpu)
    for name in ("pooled", "W3", "b3", "dl"):
        idx = N.place(entry, t[name].shape, batched=name in ("pooled", "dl"))
        bad, clean = _poisoned(t, name, idx, entry.value)
        what = f"fc {name} {entry.name} B={B}"
        v = entry.value
        n = ops.fc_wgrad_nslab(B)

        def run(o):
            out = {}
            if name != "dl":
                lg = _buf((B, 10), gpu)
                ops.fc_fwd(o["pooled"], o["W3"], o["b3"], out=lg[:B])
                out["logits"] = _done(lg, B, "logits")
            if name in ("W3", "dl"):
                for amax in (False, True):
                    dp, am = _buf((B, 9216), gpu), _buf((B,), gpu)
                    ops.fc_dgrad(o["dl"], o["W3"], out=dp[:B], dp_amax=am[:B] if amax else None)
                    out["dp_amax" if amax else "dp"] = _done(dp, B, "dpooled")
                    if amax:
                        out["amax"] = _done(am, B, "dp_amax")
            if name in ("pooled", "dl"):
                sl = _buf((n, 92170), gpu)
                ops.fc_wgrad_slabs(o["dl"], o["pooled"], slabs=sl[:n])
                out["slabs"] = _done(sl, n, "fc slabs")
            dp, am, sl = _buf((B, 9216), gpu), _buf((B,), gpu), _buf((n, 92170), gpu)
            ops.fc_backward(o["dl"], o["W3"], o["pooled"], dpooled=dp[:B], dp_amax=am[:B], slabs=sl[:n])
            out["bw"] = (_done(dp, B, "dpooled"), _done(am, B, "dp_amax"), _done(sl, n, "fc slabs"))
            return out
        got, ref = run(bad), run(clean)
        smp = idx[0] if name in ("pooled", "dl") else None
        if "logits" in got:
            if name == "b3":
                p = N.bias_predict(N.fc_lin(t["pooled"], t["W3"]), t["b3"], idx, v)
                want = p.want
            else:
                p = N.predict(N.fc_lin, t["pooled"], t["W3"], 0 if name == "pooled" else 1, idx, v)
                want = p.want + t["b3"].double()
            assert p.must.any()
            N.assert_ieee(got["logits"], want, what + " slk_fc_fwd")
        if "dp" in got:
            p = N.predict(N.fc_dgrad_lin, t["dl"], t["W3"], 0 if name == "dl" else 1, idx, v)
            assert p.must.any()
            for k in ("dp", "dp_amax"):
                N.assert_ieee(got[k], p.want, f"{what} slk_fc_dgrad ({k})")
            assert _bits_equal(got["amax"], N.amax_ignoring_nan(p.want).to(F32)), what + " dp_amax"
            assert _same(got["bw"][0], got["dp"]) and _bits_equal(got["bw"][1], got["amax"])
        if "slabs" in got:
            p = N.predict(N.fc_wgrad_lin, t["dl"], t["pooled"], 0 if name == "dl" else 1, idx, v)
            assert p.must.any()
            N.assert_ieee(got["slabs"], p.want, what + " slk_fc_wgrad")
            assert _same(got["bw"][2], got["slabs"])
            per = R.fc_wgrad_per(B)
            for r in range(n):
                if smp is not None and r != smp // per:
                    assert _bits_equal(got["slabs"][r], ref["slabs"][r]), f"{what}: slab {r} changed (clause 6)"
        if smp is not None:
            for s in _others(B, smp):
                for k in ("logits", "dp"):
                    if k in got:
                        assert _bits_equal(got[k][s], ref[k][s]), f"{what}: {k} of sample {s} changed (clause 6)"
                assert _bits_equal(got["bw"][0][s], ref["bw"][0][s])
