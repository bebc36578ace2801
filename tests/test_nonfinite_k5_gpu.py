"""GPU: the K5 convolution kernels called alone with one NaN, +inf or -inf in one operand, held to the non-finite rule of
include/slk.h ("NaN and +-inf") as tests/nonfinite_ref.py states it, on the exact regime of tests/wide_ref64.py
(the stored bf16, the routing code and the f32 slabs must EQUAL float64's). The forwards:

  slk_wide_conv1_fwd + slk_wide_relu_bits      poison in x, W1, b1
  slk_wide_conv2_fwd, slk_wide_conv3_fwd       poison in the input, W, b
  slk_wide_shadows                              every W poison goes through it: the kernels read the bf16 shadow that
                                                wide.build_shadows makes of the poisoned master weight

B = 9 (one image past the 8-XCD group: tests/test_wide_conv_gpu.py) and B = 1 (clause 6 is vacuous, b and c apply).
Asserted: outputs never hold NaN and code bytes are 0..4 (test_wide_conv_gpu's runners assert both on every launch:
clause 2); the stored value and code == the rule's (IEEE pre-activation, then rule_relu / relu_pool_code) — everywhere
for a poison in the input, the bias or the CENTRE tap of a weight. The K5 convolutions pad by one pixel and a kernel
may multiply the staged zeros (clause 4 of the rule), so for a corner tap of a weight the outputs of the poisoned channel
whose tap falls into the padding (its first or last row and column; the pool windows holding them) may or may not be
0 x NaN: those alone are held to clause 2's invariants, every other output to the rule's value; clean samples bit for
bit the clean launch's (clause 6); the ReLU words == (a1 > 0) from both producers.

The backward kernels (slk_wide_conv3_dgrad / _conv2_dgrad, the three slk_wide_conv*_wgrad) follow below, at B = 9.
Then the head (slk_wide_head / _fwd / _bwd with the dropout mask on; its weights pass through slk_wide_fc_shadow).
The head's weight (through slk_wide_fc_shadow), bias and incoming dlogits follow in a test of their own.
"""
import math

import pytest
import torch

import nonfinite_ref as N
import wide_ref64 as R
from test_wide_conv_gpu import _run_conv1, _run_fwd, relu_words

pytestmark = pytest.mark.gpu

IDS = [e.name for e in N.TABLE]


def _lin(a, w):
    return R.conv_fwd(a, w)


def _same_bf16(got, want64):
    """got (bf16) == bf16(want64), infinities as themselves, +0 for every zero (never NaN on either side)."""
    want = R.bf16(R.pos_zero(want64))
    return got.view(torch.int16) == want.view(torch.int16)


def _check(got, code, want, want_code, exact, plane, what):
    """exact: everything equals the rule. Otherwise `plane` (bool, the outputs' shape) marks the outputs held to clause
    2's invariants only; all others equal the rule."""
    assert not torch.isnan(got.float()).any() and bool((got.float() >= 0).all()), what + ": NaN or negative output"
    ok = _same_bf16(got, want)
    if code is not None:
        assert int(code.max()) <= N.CODE_NONE
        ok &= code.long() == want_code
        assert torch.equal(code == N.CODE_NONE, got.view(torch.int16) == 0), what + ": CODE_NONE and +0 disagree"
    if not exact:
        ok |= plane
    bad = ~ok
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs differ from the rule; first {tuple(bad.nonzero()[0].tolist())}"


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_wide_forwards(gpu, entry, layer, B):
    inp, W, b = R.fwd_case(layer, B, "wide", seed=9000 * layer + B, device=gpu)
    R.assert_exact_operands(inp, W, b)
    R.assert_abs_bound(R.conv_fwd(inp.abs(), W.abs(), b.abs()))
    t = dict(inp=inp.double(), W=W.double(), b=b.double())
    lin = _lin(t["inp"], t["W"])

    def run(o):
        if layer == 1:
            a1, bits, bits2 = _run_conv1(gpu, o["inp"], o["W"], o["b"])
            return a1, None, (bits, bits2)
        p, c = _run_fwd(gpu, layer, o["inp"], o["W"], o["b"])
        return p, c, None

    for name in ("inp", "W", "b"):
        idx = N.place(entry, t[name].shape, batched=name == "inp")
        bad = dict(t)
        bad[name] = N.plant(t[name], idx, entry.value)
        what = f"K5 conv{layer} fwd {name} {entry.name} B={B}"
        if name == "b":
            pre = N.bias_predict(lin, t["b"], idx, entry.value).want
        else:
            p = N.predict(_lin, t["inp"], t["W"], 0 if name == "inp" else 1, idx, entry.value)
            assert p.must.any(), what + ": must(P) is empty"
            pre = p.want + t["b"][None, :, None, None]
        if layer == 1:
            want, want_code = N.rule_relu(pre), None
        else:
            want, want_code = R.relu_pool_code(N.rule_relu(pre))
        exact = name != "W" or entry.pixel == "inner"
        plane = torch.zeros(want.shape, dtype=torch.bool, device=gpu)
        if not exact:      # tap (0, 0) reads padding in the first row and column, tap (2, 2) in the last ones
            edge = torch.zeros(pre.shape[-2:], dtype=torch.bool, device=gpu)
            r = 0 if entry.pixel == "first" else -1
            edge[r, :] = True
            edge[:, r] = True
            if layer > 1:
                edge = torch.nn.functional.max_pool2d(edge[None, None].double(), 2)[0, 0] > 0
            plane[:, idx[0]] = edge
        got, code, words = run(bad)
        _check(got, code, want, want_code, exact, plane, what)
        if layer == 1:
            assert torch.equal(words[0], relu_words(got.float() > 0)), what + ": a1bits != (a1 > 0)"
            assert torch.equal(words[1], words[0]), what + ": slk_wide_relu_bits differs"
        if name == "inp" and B > 1:
            ref, rcode, rwords = run(t)
            for s in range(B):
                if s != idx[0]:
                    assert torch.equal(got[s].view(torch.int16), ref[s].view(torch.int16)), f"{what}: sample {s} changed"
                    if code is not None:
                        assert torch.equal(code[s], rcode[s])
                    else:
                        assert torch.equal(words[0][s], rwords[0][s])
        if math.isinf(entry.value) and entry.value > 0 and name == "b":
            assert bool(torch.isinf(got.float()[:, idx[0]]).all()), what + ": a +inf bias is kept (clause 2)"


# ============================================================================ backward kernels
def _c8(t, dtype):
    from splitcnn.wide import nchw_to_c8
    return nchw_to_c8(t.to(dtype))


def _run_dgrad(dev, layer, dp, code, W, relu):
    """test_wide_conv_gpu._run_dgrad without its no-NaN assertion (a poisoned gradient must come out non-finite)."""
    from splitcnn import _lib
    from splitcnn.wide import c8_to_nchw
    from test_wide_conv_gpu import _shadows, _stream
    B = dp.shape[0]
    CI, CO, HW = R.LAYERS[layer]
    sh = _shadows(dev, **{f"W{layer}": W})
    d8, c8 = _c8(dp, torch.bfloat16), _c8(code, torch.uint8)
    out = torch.full((B + 1, CI // 8, HW, HW, 8), float("nan"), dtype=torch.bfloat16, device=dev)
    out.view(torch.int16)[B:] = 0x7FC1           # the sentinel sample, a NaN pattern no kernel writes
    if layer == 3:
        _lib.call("slk_wide_conv3_dgrad", d8.data_ptr(), c8.data_ptr(), sh["w3d"].data_ptr(), out.data_ptr(), B, _stream())
    else:
        words = relu_words(relu)
        _lib.call("slk_wide_conv2_dgrad", d8.data_ptr(), c8.data_ptr(), sh["w2d"].data_ptr(), words.data_ptr(),
                  out.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16)[B:] == 0x7FC1).all()), "a write landed past the last sample"
    return c8_to_nchw(out[:B]).contiguous()


def _run_wgrad(dev, layer, inp, d, code):
    from splitcnn import _lib
    from test_wide_conv_gpu import _stream
    B = inp.shape[0]
    CI, CO, HW = R.LAYERS[layer]
    n = CO * CI * 9 + CO
    nslab = _lib.query(f"slk_wide_conv{layer}_wgrad_nslab", B)
    slabs = torch.full((nslab + 1, n), float("nan"), device=dev)
    d8 = _c8(d, torch.bfloat16)
    if layer == 1:
        xf = inp.to(torch.float32).contiguous()
        _lib.call("slk_wide_conv1_wgrad", xf.data_ptr(), d8.data_ptr(), slabs.data_ptr(), B, _stream())
    else:
        c8, i8 = _c8(code, torch.uint8), _c8(inp, torch.bfloat16)
        _lib.call(f"slk_wide_conv{layer}_wgrad", d8.data_ptr(), c8.data_ptr(), i8.data_ptr(), slabs.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(slabs[nslab]).all()), "a write landed past the last slab"
    return slabs[:nslab]


def _routed(idx, code):
    b, c, py, px = idx
    q = int(code[b, c, py, px])
    return None if q >= N.CODE_NONE else (b, c, 2 * py + q // 2, 2 * px + q % 2)


@pytest.mark.parametrize("layer", [3, 2])
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_wide_dgrads(gpu, entry, layer):
    """slk_wide_conv3_dgrad / slk_wide_conv2_dgrad at B = 9 with the poison in dpooled — under a routing code, and under
    CODE_NONE where clause 5 makes the launch bit for bit the clean one — and in W (through its bf16 shadow):
    must(P) <= non-finite <= may(P), bf16(float64) outside may(P); may(P) of a weight is widened to the whole planes of
    its input channel (padding). conv2's ReLU words are a select: a masked position is +0 whatever the gradient holds
    (sample 0 passes everything, sample 1 nothing). Clause 6 for a poisoned dpooled."""
    B = 9
    dp, code0, W, relu = R.dgrad_case(layer, B, "wide", seed=9100 * layer, device=gpu)
    R.assert_abs_bound(R.conv_dgrad(R.unpool(dp.abs(), code0), W.abs()))

    def mask(t):
        return t if relu is None else torch.where(relu, t, torch.zeros_like(t))
    for name in ("dp_routed", "dp_blocked", "W"):
        key = name.split("_")[0]
        t = dict(dp=dp.double(), W=W.double())
        idx = N.place(entry, t[key].shape, batched=key == "dp")
        code = code0.clone()
        if key == "dp":
            if name == "dp_blocked":
                code[idx] = N.CODE_NONE
            elif int(code[idx]) == N.CODE_NONE:
                code[idx] = 1
        dy = R.unpool(t["dp"], code)
        if key == "dp":
            p = N.predict(R.conv_dgrad, dy, t["W"], 0, _routed(idx, code), entry.value)
        else:
            p = N.predict(R.conv_dgrad, dy, t["W"], 1, idx, entry.value)
            p = p._replace(may=N.widen_planes(p.may))
        if relu is not None:
            p = N.Pred(mask(p.want), p.must & relu, p.may & relu, mask(p.clean))
        what = f"K5 conv{layer} dgrad {name} {entry.name}"
        if name == "dp_blocked":
            assert not p.may.any()
        else:     # the table's samples are 0, 4 and 8; conv2's all-masked sample is sample 1
            assert p.must.any(), what + ": must(P) is empty"
        bad = dict(t)
        bad[key] = N.plant(t[key], idx, entry.value)
        got = _run_dgrad(gpu, layer, bad["dp"], code, bad["W"], relu)
        ref = _run_dgrad(gpu, layer, t["dp"], code, t["W"], relu)
        nf = N.nonfinite(got.float())
        assert not (p.must & ~nf).any(), what + ": an output of must(P) is finite"
        assert not (nf & ~p.may).any(), f"{what}: {int((nf & ~p.may).sum())} non-finite outputs outside may(P)"
        clean_ok = _same_bf16(got, p.clean) | p.may
        assert clean_ok.all(), f"{what}: {int((~clean_ok).sum())} clean outputs differ from bf16(float64)"
        if relu is not None:
            assert bool((got.view(torch.int16)[~relu] == 0).all()), what + ": a ReLU-masked gradient is not +0"
        if name == "dp_blocked":
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), what + ": a blocked gradient leaked"
        elif key == "dp":
            for s in range(B):
                if s != idx[0]:
                    assert torch.equal(got[s].view(torch.int16), ref[s].view(torch.int16)), f"{what}: sample {s} changed"


@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_wide_wgrads(gpu, entry, layer):
    """slk_wide_conv1_wgrad / _conv2_wgrad / _conv3_wgrad at B = 9 with the poison in the input and in the gradient
    (layers 2, 3: under a routing code, and under CODE_NONE: bit for bit the clean launch). Columns of must(P) are
    non-finite in the slabs' sum, none outside may(P) is, and those equal float64 and the clean launch's in every slab.
    may(P) is the dense reach over every output pixel (layers 2 and 3 run on the 2:4-sparse MFMA, clause 4: a column of
    may(P) \\ must(P) may stay finite), widened for a poisoned gradient to every tap of its channel (zero padding)."""
    B = 9
    inp, d, code0 = R.wgrad_case(layer, B, "exact", seed=9200 * layer, device=gpu)

    def op(a, g):
        dW, db = R.conv_wgrad(a, g)
        return torch.cat([dW.reshape(-1), db])

    def unpooled(g, code):
        return g if layer == 1 else R.unpool(g, code)
    CI, CO, _ = R.LAYERS[layer]
    R.assert_abs_bound(op(inp.abs(), unpooled(d.abs(), code0)))
    for name in ("inp", "d_routed") + (("d_blocked",) if layer > 1 else ()):
        key = name.split("_")[0]
        t = dict(inp=inp.double(), d=d.double())
        idx = N.place(entry, t[key].shape)
        code = None if code0 is None else code0.clone()
        if key == "d" and layer > 1:
            if name == "d_blocked":
                code[idx] = N.CODE_NONE
            elif int(code[idx]) == N.CODE_NONE:
                code[idx] = 1
        # the selects first (clause 5): dy is the routed gradient, and a blocked value never becomes an operand
        dy = unpooled(t["d"], code)
        if key == "inp":
            p = N.predict(op, t["inp"], dy, 0, idx, entry.value)
        else:
            ridx = idx if layer == 1 else _routed(idx, code)
            p = N.predict(op, t["inp"], dy, 1, ridx, entry.value)
            if ridx is not None:
                # the input is zero-padded by one pixel and the kernels multiply the staged zeros (csrc/slk_wide.hip
                # `off[k] >= 0 ? img[off[k]] : 0.f`, and the MFMA operand tiles of conv2 / conv3): at a border pixel the
                # taps that fall into the padding form 0 x NaN, so may(P) is every tap of the gradient's channel
                cols = torch.zeros(CO, CI * 9, dtype=torch.bool, device=gpu)
                cols[idx[1]] = True
                p = p._replace(may=p.may | torch.cat([cols.reshape(-1), torch.zeros(CO, dtype=torch.bool, device=gpu)]))
        what = f"K5 conv{layer} wgrad {name} {entry.name}"
        if name != "d_blocked":
            assert p.must.any(), what + ": must(P) is empty"
        bad = dict(t)
        bad[key] = N.plant(t[key], idx, entry.value)
        s = _run_wgrad(gpu, layer, bad["inp"], bad["d"], code)
        sref = _run_wgrad(gpu, layer, t["inp"], t["d"], code)
        nf = N.nonfinite(s).any(0)
        assert not (p.must & ~nf).any(), f"{what}: {int((p.must & ~nf).sum())} columns of must(P) are finite"
        assert not (nf & ~p.may).any(), f"{what}: {int((nf & ~p.may).sum())} non-finite columns outside may(P)"
        assert torch.equal(s.double().sum(0)[~p.may], p.clean[~p.may]), what + ": clean columns != float64"
        assert torch.equal(s[:, ~p.may].view(torch.int32), sref[:, ~p.may].view(torch.int32)), what + ": a clean column changed"
        if name == "d_blocked":
            assert torch.equal(s.view(torch.int32), sref.view(torch.int32)), what + ": a blocked gradient leaked"


# ============================================================================ the head, dropout mask on
def _eq_nan(a, b):
    """Equal bit for bit where neither is NaN, NaN in the same places."""
    af, bf_ = a.float(), b.float()
    na, nb = torch.isnan(af), torch.isnan(bf_)
    z = torch.zeros_like(af)
    return torch.equal(na, nb) and torch.equal(torch.where(na, z, af).view(torch.int32), torch.where(nb, z, bf_).view(torch.int32))


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_wide_head_dropout_is_a_select(gpu, entry):
    """slk_wide_head_fwd, slk_wide_head_bwd and slk_wide_head at B = 9, p = 0.5, one cut feature poisoned.
    The clause-7 sentence for the head's dropout, read from csrc/slk_wide_head.hip (`(kb >> k) & 1 ? d[k] * keep_scale :
    0.f`): dropout is a SELECT. A DROPPED non-finite feature is 0 — every output of all three entries is bit for bit the
    clean launch's — where torch's Dropout (a multiplication by the mask) keeps a NaN. A KEPT one is an ordinary operand
    (clause 1): all ten logits of its sample are non-finite, column k of dWf in its group's slab is non-finite, every
    other column, dbf, and dcut (which does not read the cut) are the clean launch's; the fused entry's loss and dlogits
    row are NaN and so is its dcut row. Other samples: bit for bit the clean launch's (clause 6). The fused entry writes
    what the split pair writes from its dlogits."""
    import head_ref64 as H
    from test_wide_head_exact_gpu import B0, HALF, _keep, _operands, _run_bwd, _run_fused, _run_fwd
    B = 9
    cut, Wf, bf = H.head_int_case(B, 9300, gpu)
    dl = H.dlogits_int(B, 9301, gpu)
    y = torch.arange(B, device=gpu) % 10
    _, keep = _keep(gpu, B, 0.5, B0)
    cut8, wf8 = _operands(gpu, cut, Wf)
    clean = dict(fwd=_run_fwd(gpu, cut8, wf8, bf, HALF, B0), bwd=_run_bwd(gpu, cut8, wf8, dl, HALF, B0),
                 fused=_run_fused(gpu, cut8, wf8, bf, y, HALF, B0))
    b, k0 = N.place(entry, cut.shape)
    for kept in (False, True):
        cand = (keep[b] == kept).nonzero()[:, 0]
        k = int(cand[(cand - k0).abs().argmin()])             # the feature nearest the table's with that mask bit
        bad8 = H.c8_of_flat(N.plant(cut.double(), (b, k), entry.value)).to(torch.bfloat16).contiguous()
        what = f"K5 head {entry.name} {'kept' if kept else 'dropped'} feature {k}"
        logits = _run_fwd(gpu, bad8, wf8, bf, HALF, B0)
        dcut, slabs = _run_bwd(gpu, bad8, wf8, dl, HALF, B0)
        f = _run_fused(gpu, bad8, wf8, bf, y, HALF, B0)
        # the fused entry against the split pair on the same poisoned cut
        assert _eq_nan(f["logits"], logits), what + ": fused logits != slk_wide_head_fwd"
        d2, s2 = _run_bwd(gpu, bad8, wf8, f["dl"], HALF, B0)
        assert _eq_nan(f["dcut"], d2) and _eq_nan(f["slabs"], s2), what + ": fused backward != slk_wide_head_bwd"
        if not kept:
            assert torch.equal(logits.view(torch.int32), clean["fwd"].view(torch.int32)), what + ": logits changed"
            assert torch.equal(dcut.view(torch.int16), clean["bwd"][0].view(torch.int16))
            assert torch.equal(slabs.view(torch.int32), clean["bwd"][1].view(torch.int32)), what + ": slabs changed"
            for key in ("logits", "loss", "dl", "slabs"):
                assert torch.equal(f[key].view(torch.int32), clean["fused"][key].view(torch.int32)), f"{what}: fused {key}"
            assert torch.equal(f["dcut"].view(torch.int16), clean["fused"]["dcut"].view(torch.int16))
            continue
        others = [s for s in range(B) if s != b]
        assert bool(N.nonfinite(logits[b]).all()), what + ": a logit of the poisoned sample is finite"
        assert torch.equal(logits[others].view(torch.int32), clean["fwd"][others].view(torch.int32)), what + " (clause 6)"
        assert torch.equal(dcut.view(torch.int16), clean["bwd"][0].view(torch.int16)), what + ": dcut reads no cut"
        nf = N.nonfinite(slabs)
        want = torch.zeros_like(nf)
        want[b // 64, [j * H.CUT_F + k for j in range(10)]] = True       # dWf[j][k], flatten order, all ten classes
        assert torch.equal(nf, want), f"{what}: non-finite slab entries {nf.nonzero().tolist()[:12]}"
        assert torch.equal(slabs[~nf].view(torch.int32), clean["bwd"][1][~nf].view(torch.int32))
        assert bool(torch.isnan(f["loss"][b])) and bool(torch.isnan(f["dl"][b]).all())
        assert bool(torch.isnan(f["dcut"][b].float()[H.c8_of_flat(keep.double())[b] > 0]).all())
        for key in ("logits", "loss", "dl", "dcut"):
            a, c = f[key][others], clean["fused"][key][others]
            assert _eq_nan(a, c) and not torch.isnan(a.float()).any(), f"{what}: fused {key} of a clean sample changed"


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_wide_head_weight_bias_gradient(gpu, entry):
    """The head's other operands at B = 9, p = 0.5, each holding the poison in turn:
    Wf[j][k], through slk_wide_fc_shadow on the poisoned master weight (the shadow is the permutation of its bits,
      the poison included): slk_wide_head_fwd's logit j of EVERY sample is IEEE's (a dropped or zero feature times the
      poison is NaN: clause 1), every other logit the clean launch's; slk_wide_head_bwd's dcut column k is non-finite for
      the samples that keep feature k and +0 for those that drop it (the dropout select, clause 5), every other column
      and every slab (which read no weight) the clean launch's;
    bf[j]: logit j of every sample is IEEE's sum (an infinity stays that infinity), everything else clean;
    dlogits[b][j] (slk_wide_head_bwd): dcut[b] is non-finite at the kept features and +0 at the dropped ones, other
      samples bit for bit clean (clause 6); row j of dWf and dbf[j] in the sample's slab are non-finite, all else clean.
    slk_wide_head on the poisoned Wf / bf writes slk_wide_head_fwd's logits and, from its own dlogits, what
    slk_wide_head_bwd writes."""
    import head_ref64 as H
    from test_wide_head_exact_gpu import B0, HALF, _keep, _operands, _run_bwd, _run_fused, _run_fwd
    B = 9
    cut, Wf, bf = H.head_int_case(B, 9400, gpu)
    dl = H.dlogits_int(B, 9401, gpu)
    y = torch.arange(B, device=gpu) % 10
    _, keep = _keep(gpu, B, 0.5, B0)
    d = torch.where(keep, cut.double() * 2.0, torch.zeros_like(cut, dtype=torch.float64))      # the dropped features
    cut8, wf8 = _operands(gpu, cut, Wf)
    c_logits = _run_fwd(gpu, cut8, wf8, bf, HALF, B0)
    c_dcut, c_slabs = _run_bwd(gpu, cut8, wf8, dl, HALF, B0)
    v = entry.value

    def flat(dcut):
        return H.flat_of_c8(dcut.float())

    def bits(t):
        return t.contiguous().view(torch.int32)

    # ---- Wf, through the shadow
    j, k = N.place(entry, Wf.shape, batched=False)
    Wp = N.plant(Wf.float(), (j, k), v)
    _, wp8 = _operands(gpu, cut, Wp)
    assert _eq_nan(wp8, Wp.reshape(10, 32, 8, 64).permute(0, 1, 3, 2).reshape(10, H.CUT_F)), "slk_wide_fc_shadow"
    what = f"K5 head Wf[{j}][{k}] {entry.name}"
    logits = _run_fwd(gpu, cut8, wp8, bf, HALF, B0)
    W0 = N.plant(Wf.double(), (j, k), 0.0)
    want = H.head_fwd(cut, W0, bf, keep, 2.0)
    want[:, j] = want[:, j] + d[:, k] * v
    N.assert_ieee(logits, want, what + " slk_wide_head_fwd")
    assert bool(N.nonfinite(logits[:, j]).all())
    dcut, slabs = _run_bwd(gpu, cut8, wp8, dl, HALF, B0)
    nf = N.nonfinite(flat(dcut))
    wantnf = torch.zeros_like(nf)
    wantnf[:, k] = keep[:, k]
    assert torch.equal(nf, wantnf), what + ": dcut's non-finite pattern"
    assert torch.equal(flat(dcut)[~nf].view(torch.int32), flat(c_dcut)[~nf].view(torch.int32)), what + ": dcut changed"
    assert torch.equal(bits(slabs), bits(c_slabs)), what + ": the slabs read no weight"
    f = _run_fused(gpu, cut8, wp8, bf, y, HALF, B0)
    assert _eq_nan(f["logits"], logits), what + ": fused logits"
    d2, s2 = _run_bwd(gpu, cut8, wp8, f["dl"], HALF, B0)
    assert _eq_nan(f["dcut"], d2) and _eq_nan(f["slabs"], s2), what + ": fused backward"
    # ---- bf
    (jb,) = N.place(entry, bf.shape, batched=False)
    bp = N.plant(bf.double(), (jb,), v)
    what = f"K5 head bf[{jb}] {entry.name}"
    logits = _run_fwd(gpu, cut8, wf8, bp, HALF, B0)
    N.assert_ieee(logits, H.head_fwd(cut, Wf, bf, keep, 2.0) - bf.double() + bp, what)
    f = _run_fused(gpu, cut8, wf8, bp, y, HALF, B0)
    assert _eq_nan(f["logits"], logits), what + ": fused logits"
    d2, s2 = _run_bwd(gpu, cut8, wf8, f["dl"], HALF, B0)
    assert _eq_nan(f["dcut"], d2) and _eq_nan(f["slabs"], s2), what + ": fused backward"
    # ---- dlogits
    b, jd = N.place(entry, dl.shape)
    what = f"K5 head dlogits[{b}][{jd}] {entry.name}"
    dcut, slabs = _run_bwd(gpu, cut8, wf8, N.plant(dl.double(), (b, jd), v), HALF, B0)
    nf = N.nonfinite(flat(dcut))
    wantnf = torch.zeros_like(nf)
    wantnf[b] = keep[b]
    assert torch.equal(nf, wantnf), what + ": dcut's non-finite pattern"
    assert torch.equal(flat(dcut)[~nf].view(torch.int32), flat(c_dcut)[~nf].view(torch.int32)), what + ": dcut changed"
    assert bool((flat(dcut)[b][~keep[b]].view(torch.int32) == 0).all()), what + ": a dropped position is not +0"
    nfs = N.nonfinite(slabs)
    wants = torch.zeros_like(nfs)
    wants[b // 64, jd * H.CUT_F:(jd + 1) * H.CUT_F] = True
    wants[b // 64, 10 * H.CUT_F + jd] = True
    assert torch.equal(nfs, wants), what + ": the slabs' non-finite pattern"
    assert torch.equal(slabs[~nfs].view(torch.int32), c_slabs[~nfs].view(torch.int32)), what + ": a clean slab entry changed"
