"""The four soft-target heads (slk_xent_soft_fwd_bwd, slk_fc_logits_xent_soft, slk_fc_xent_soft, slk_wide_head_soft) on
the crafted logit rows of head_ref64 (all equal, +-100 ramps, one logit far above, magnitude 1e4, +-1e30, -inf off
the label), at B = 17 and 33: first and last slot of a 16-sample workgroup and a ragged last one.

  * smoothing = 0 on plain labels: every output bit for bit the hard-label twin's (the -inf rows too, for the entry
    that takes logits);
  * eps in {0.1, 1} x targets with wb in {0, 0.25, 1}, a != b and a == b: loss_i and dlogits against the float64
    closed form inside soft_ref64's bounds (head_ref64's plus 2^-24 per float32 rounding of the documented
    expression: derivation in soft_ref64.py), finite on finite rows, |sum_j dlogits_j| inside its bound;
  * the soft wide head's dcut and slabs are slk_wide_head_bwd's from its dlogits, bit for bit;
  * each kind of malformed target sets the flag and writes NaN for its row only;
  * smoothing outside [0, 1] or NaN is the invalid-argument status and nothing is launched.

The fused K2 heads see the rows through head_ref64's one-hot construction, the wide head through one-hot cut positions
(as tests/test_xent_edges_gpu.py). Outputs are pre-filled with NaN with a sentinel row behind the last one. The largest
observed share of each bound is printed."""
import numpy as np
import pytest
import torch

import head_ref64 as R
import soft_ref64 as S

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = [(17, 0), (17, 11), (33, 0), (33, 11)]
EPSS = (0.1, 1.0)
TARGETS = [(0.0, False), (0.25, False), (1.0, False), (0.25, True), (1.0, True)]   # (wb, a == b)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _err(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- runners (eps=None: the hard twin)
def run_xent(dev, zt, yt, eps):
    from splitcnn import _lib
    B = zt.shape[0]
    o = dict(loss=_nan((B + 1,), dev), dl=_nan((B + 1, 10), dev), err=_err(dev))
    if eps is None:
        _lib.call("slk_xent_fwd_bwd", zt.data_ptr(), yt.data_ptr(), o["loss"].data_ptr(), o["dl"].data_ptr(), 1.0,
                  o["err"].data_ptr(), B, _stream())
    else:
        _lib.call("slk_xent_soft_fwd_bwd", zt.data_ptr(), yt.data_ptr(), o["loss"].data_ptr(), o["dl"].data_ptr(), 1.0,
                  float(eps), o["err"].data_ptr(), B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(o["loss"], B, "loss_i")
    R.assert_sentinel(o["dl"], B * 10, "dlogits")
    return o


def k2_operands(dev, z, B):
    ks = R.onehot_features(B)
    W3 = torch.zeros((10, R.P_SAMPLE), dtype=torch.float32, device=dev)
    W3[:, torch.tensor(ks, device=dev)] = torch.from_numpy(z).float().to(dev).T
    pooled = R.onehot_rows(B, R.P_SAMPLE, ks, dev).float().contiguous()
    return pooled, W3.contiguous(), torch.zeros(10, dtype=torch.float32, device=dev)


def run_k2(dev, entry, opnd, yt, eps):
    """entry: 'logits_xent', 'fc_xent' (no dp_amax) or 'fc_xent_amax'."""
    from splitcnn import _lib
    pooled, W3, b3 = opnd
    B = pooled.shape[0]
    o = dict(logits=_nan((B + 1, 10), dev), loss=_nan((B + 1,), dev), dl=_nan((B + 1, 10), dev),
             dp=_nan((B + 1, R.P_SAMPLE), dev), am=_nan((B + 1,), dev), err=_err(dev))
    head = (pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), o["logits"].data_ptr(), o["loss"].data_ptr(),
            o["dl"].data_ptr())
    tail = (o["err"].data_ptr(), B, _stream())
    if entry == "logits_xent":
        if eps is None:
            _lib.call("slk_fc_logits_xent", *head, 1.0, *tail)
        else:
            _lib.call("slk_fc_logits_xent_soft", *head, 1.0, float(eps), *tail)
    elif eps is None and entry == "fc_xent":
        _lib.call("slk_fc_xent", *head, o["dp"].data_ptr(), 1.0, *tail)
    elif eps is None:
        _lib.call("slk_fc_xent_amax", *head, o["dp"].data_ptr(), o["am"].data_ptr(), 1.0, *tail)
    else:
        _lib.call("slk_fc_xent_soft", *head, o["dp"].data_ptr(), o["am"].data_ptr() if entry == "fc_xent_amax" else None,
                  1.0, float(eps), *tail)
    torch.cuda.synchronize()
    for k, used in (("logits", B * 10), ("loss", B), ("dl", B * 10),
                    ("dp", 0 if entry == "logits_xent" else B * R.P_SAMPLE), ("am", B if entry == "fc_xent_amax" else 0)):
        R.assert_sentinel(o[k], used, f"{entry} {k}")
    return o


K2_ENTRIES = ("logits_xent", "fc_xent", "fc_xent_amax")
K2_KEYS = ("logits", "loss", "dl", "dp", "am")


def _wide_positions(B):
    ps = [0, R.CUT_F - 1]
    for w in (1, 3, 7):
        ps += [2048 * w, 2048 * w + 2047]
    ps = list(dict.fromkeys(ps))
    ps += [p for p in range(37, R.CUT_F, 487) if p not in ps]
    assert B <= len(ps)
    return ps[:B]


def wide_operands(dev, zt, B):
    """A one-hot bf16 cut with the rows in columns of Wf (test_xent_edges_gpu's construction)."""
    from splitcnn import _lib
    ps = torch.tensor(_wide_positions(B), device=dev)
    cut8 = torch.zeros((B, R.CUT_F), dtype=torch.float64, device=dev)
    cut8[torch.arange(B, device=dev), ps] = 1.0
    feat = R.flat_of_c8(cut8).argmax(dim=1)
    Wf = torch.zeros((10, R.CUT_F), dtype=torch.float32, device=dev)
    Wf[:, feat] = zt.T
    wf8 = _nan((10, R.CUT_F), dev)
    _lib.call("slk_wide_fc_shadow", Wf.data_ptr(), wf8.data_ptr(), _stream())
    return cut8.to(torch.bfloat16).contiguous(), wf8, torch.zeros(10, dtype=torch.float32, device=dev)


def run_wide(dev, opnd, yt, eps, thresh=0, scale=1.0, seed=7, step_no=3):
    from splitcnn import _lib
    cut, wf8, bf = opnd
    B = cut.shape[0]
    step = torch.full((1,), step_no, dtype=torch.int32, device=dev)
    nslab, nwork = _lib.query("slk_wide_head_nslab", B), _lib.query("slk_wide_head_work", B)
    o = dict(logits=_nan((B + 1, 10), dev), loss=_nan((B + 1,), dev), dl=_nan((B + 1, 10), dev),
             dcut=_nan((B + 1, R.CUT_F), dev, torch.bfloat16), slabs=_nan((nslab + 1, 163850), dev),
             work=_nan((nwork + 512,), dev), err=_err(dev), nslab=nslab, step=step)
    a = (cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), yt.data_ptr(), step.data_ptr(), seed, thresh, scale, 1.0)
    b = (o["logits"].data_ptr(), o["loss"].data_ptr(), o["dl"].data_ptr(), o["dcut"].data_ptr(), o["slabs"].data_ptr(),
         o["work"].data_ptr(), o["err"].data_ptr(), 0, B, _stream())
    if eps is None:
        _lib.call("slk_wide_head", *a, *b)
    else:
        _lib.call("slk_wide_head_soft", *a, float(eps), *b)
    torch.cuda.synchronize()
    for k, used in (("logits", B * 10), ("loss", B), ("dl", B * 10), ("dcut", B * R.CUT_F), ("slabs", nslab * 163850),
                    ("work", nwork)):
        R.assert_sentinel(o[k], used, f"slk_wide_head {k}")
    return o


WIDE_KEYS = ("logits", "loss", "dl", "dcut", "slabs", "work")


def _batch(B, shift, dev, finite_only=True):
    names, z, y = R.xent_batch(B, shift, finite_only)
    return names, z, y, torch.from_numpy(z).float().to(dev).contiguous(), torch.from_numpy(y).to(dev)


# ----------------------------------------------------------------------------- smoothing 0, plain labels: bitwise
@pytest.mark.parametrize("B,shift", CASES)
def test_smoothing_zero_on_plain_labels_is_the_hard_head_bitwise(gpu, B, shift):
    names, z, y, zt, yt = _batch(B, shift, gpu, finite_only=False)
    hard, soft = run_xent(gpu, zt, yt, None), run_xent(gpu, zt, yt, 0.0)
    assert int(hard["err"]) == 0 and int(soft["err"]) == 0
    for k in ("loss", "dl"):
        assert _same(soft[k], hard[k]), f"slk_xent_soft_fwd_bwd: {k} differs from slk_xent_fwd_bwd"
    assert torch.isfinite(soft["loss"][:B]).all(), "a -inf logit off the label reached the loss"

    names, z, y, zt, yt = _batch(B, shift, gpu)
    opnd = k2_operands(gpu, z, B)
    for entry in K2_ENTRIES:
        hard, soft = run_k2(gpu, entry, opnd, yt, None), run_k2(gpu, entry, opnd, yt, 0.0)
        assert int(hard["err"]) == 0 and int(soft["err"]) == 0
        assert _same(hard["logits"][:B], zt), "the one-hot construction did not reproduce the rows"
        for k in K2_KEYS:
            assert _same(soft[k], hard[k]), f"{entry}: {k} differs from the hard-label twin"
    wopnd = wide_operands(gpu, zt, B)
    for thresh, scale in ((0, 1.0), (1 << 30, 4.0 / 3.0)):
        hard, soft = run_wide(gpu, wopnd, yt, None, thresh, scale), run_wide(gpu, wopnd, yt, 0.0, thresh, scale)
        assert int(hard["err"]) == 0 and int(soft["err"]) == 0
        for k in WIDE_KEYS:
            assert _same(soft[k], hard[k]), f"slk_wide_head_soft (threshold {thresh}): {k} differs from slk_wide_head"


# ----------------------------------------------------------------------------- soft targets against float64
def _check(what, names, z, y, eps, loss, dl, worst):
    loss64, d64, p64, _ = S.soft_xent64(z, y, eps)
    loss, dl = loss.cpu().numpy().astype(np.float64), dl.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(dl).all(), f"{what}: non-finite output on a finite row"
    rl = np.abs(loss - loss64) / S.soft_loss_bound(z, y, eps, loss64)
    rg = np.abs(dl - d64) / S.soft_grad_bound(z, y, eps, p64)
    rs = np.abs(dl.sum(axis=1)) / S.soft_gradsum_bound(z, y, eps)
    msg = (f"{what}: loss {rl.max():.3f} of its bound ({names[int(rl.argmax())]}), dlogits {rg.max():.3f} "
           f"({names[int(rg.max(axis=1).argmax())]}), row sum {rs.max():.3f} ({names[int(rs.argmax())]})")
    assert rl.max() <= 1.0 and rg.max() <= 1.0 and rs.max() <= 1.0, msg
    for i, r in enumerate((rl, rg, rs)):
        worst[i] = max(worst[i], float(r.max()))


@pytest.mark.parametrize("B,shift", CASES)
def test_soft_targets_meet_float64(gpu, B, shift):
    names, z, y, zt, _ = _batch(B, shift, gpu)
    opnd, wopnd = k2_operands(gpu, z, B), wide_operands(gpu, zt, B)
    worst = {e: [0.0, 0.0, 0.0] for e in ("xent",) + K2_ENTRIES + ("wide",)}
    for eps in EPSS:
        for wb, same in TARGETS:
            ym = S.mixed_cases(y, wb, same=same)
            yt = torch.from_numpy(ym).to(gpu)
            tag = f"eps={eps} wb={wb} a{'==' if same else '!='}b B={B}"
            o = run_xent(gpu, zt, yt, eps)
            assert int(o["err"]) == 0
            _check(f"slk_xent_soft_fwd_bwd {tag}", names, z, ym, eps, o["loss"][:B], o["dl"][:B], worst["xent"])
            ref = o
            for entry in K2_ENTRIES:
                o = run_k2(gpu, entry, opnd, yt, eps)
                assert int(o["err"]) == 0 and _same(o["logits"][:B], zt)
                _check(f"{entry}_soft {tag}", names, z, ym, eps, o["loss"][:B], o["dl"][:B], worst[entry])
                # one expression in every copy: the fused heads write the bits of the entry that takes logits
                assert _same(o["loss"], ref["loss"]) and _same(o["dl"], ref["dl"]), f"{entry}_soft {tag}"
                if entry != "logits_xent":
                    assert torch.isfinite(o["dp"][:B]).all()
            o = run_wide(gpu, wopnd, yt, eps)
            assert int(o["err"]) == 0 and _same(o["logits"][:B], zt)
            _check(f"slk_wide_head_soft {tag}", names, z, ym, eps, o["loss"][:B], o["dl"][:B], worst["wide"])
            assert torch.isfinite(o["dcut"][:B].float()).all() and torch.isfinite(o["slabs"][:o["nslab"]]).all()
    for e, w in worst.items():
        print(f"B={B} shift={shift} {e}: largest share of the bounds: loss {w[0]:.3f}, dlogits {w[1]:.3f}, row sum {w[2]:.3f}")


@pytest.mark.parametrize("B", (17, 33))
def test_wide_soft_dcut_and_slabs_are_head_bwd_of_its_dlogits(gpu, B):
    """Real dropout (p = 0.25), a random bf16 cut and Wf, mixed labels, eps = 0.1."""
    from splitcnn import _lib
    gen = torch.Generator().manual_seed(B)
    cut = torch.randn((B, R.CUT_F), generator=gen).clamp_min(0).to(torch.bfloat16).to(gpu).contiguous()
    Wf = (torch.randn((10, R.CUT_F), generator=gen) * 0.01).to(gpu)
    wf8 = _nan((10, R.CUT_F), gpu)
    _lib.call("slk_wide_fc_shadow", Wf.data_ptr(), wf8.data_ptr(), _stream())
    bf = (torch.randn(10, generator=gen) * 0.1).to(gpu)
    a = torch.randint(0, 10, (B,), generator=gen)
    ym = S.pack_np(a.numpy(), (a.numpy() + 4) % 10, torch.rand(B, generator=gen).numpy())
    yt = torch.from_numpy(ym).to(gpu)
    thresh, scale = 1 << 30, 4.0 / 3.0
    o = run_wide(gpu, (cut, wf8, bf), yt, 0.1, thresh, scale)
    assert int(o["err"]) == 0
    dcut = _nan((B + 1, R.CUT_F), gpu, torch.bfloat16)
    slabs = _nan((o["nslab"] + 1, 163850), gpu)
    _lib.call("slk_wide_head_bwd", cut.data_ptr(), wf8.data_ptr(), o["dl"].data_ptr(), o["step"].data_ptr(), 7, thresh, scale,
              dcut.data_ptr(), slabs.data_ptr(), 0, B, _stream())
    torch.cuda.synchronize()
    assert _same(o["dcut"], dcut), "dcut differs from slk_wide_head_bwd fed the soft head's dlogits"
    assert _same(o["slabs"], slabs), "the fc slabs differ from slk_wide_head_bwd fed the soft head's dlogits"
    assert o["dcut"][:B].float().abs().max() > 0
    # and the loss is the closed form on the head's own logits
    z = o["logits"][:B].cpu().numpy().astype(np.float64)
    loss64, d64, p64, _ = S.soft_xent64(z, ym, 0.1)
    assert (np.abs(o["loss"][:B].cpu().numpy() - loss64) <= S.soft_loss_bound(z, ym, 0.1, loss64)).all()
    assert (np.abs(o["dl"][:B].cpu().numpy() - d64) <= S.soft_grad_bound(z, ym, 0.1, p64)).all()


# ----------------------------------------------------------------------------- malformed targets
def _bad_targets():
    ok = int(S.pack_np(3, 7, np.float32(0.25)))
    return {"a=10": 10, "b=10": 3 | (10 << 8), "reserved bit": ok | (1 << 20), "wb=1.5": int(S.pack_np(3, 7, np.float32(1.5))),
            "wb=NaN": int(S.pack_np(3, 7, np.float32("nan"))), "y<0": ok - (1 << 63)}


@pytest.mark.parametrize("kind", list(_bad_targets()))
def test_malformed_target_flags_and_poisons_its_row_only(gpu, kind):
    B, eps = 33, 0.1
    names, z, y, zt, _ = _batch(B, 4, gpu)
    good = S.mixed_cases(y, 0.25)
    opnd, wopnd = k2_operands(gpu, z, B), wide_operands(gpu, zt, B)
    for row in (0, 15, 32):              # first and last slot of a workgroup, and the ragged last workgroup
        bad = good.copy()
        bad[row] = _bad_targets()[kind]
        assert kind != "y<0" or bad[row] < 0
        others = torch.tensor([r for r in range(B) if r != row], device=gpu)
        yg, yb = torch.from_numpy(good).to(gpu), torch.from_numpy(bad).to(gpu)
        runs = [("slk_xent_soft_fwd_bwd", lambda t: run_xent(gpu, zt, t, eps), ("loss", "dl"))]
        runs += [(f"{e}_soft", (lambda t, e=e: run_k2(gpu, e, opnd, t, eps)), K2_KEYS) for e in K2_ENTRIES]
        runs += [("slk_wide_head_soft", lambda t: run_wide(gpu, wopnd, t, eps), ("logits", "loss", "dl", "dcut", "work"))]
        for name, run, keys in runs:
            og, ob = run(yg), run(yb)
            what = f"{name}, {kind} in row {row}"
            assert int(og["err"]) == 0 and int(ob["err"]) != 0, f"{what}: the flag"
            assert torch.isnan(ob["loss"][row]) and torch.isnan(ob["dl"][row]).all(), f"{what}: the row is not NaN"
            for k in keys:
                if ob[k].shape[0] >= B and k != "work":
                    assert _same(ob[k][others], og[k][others]), f"{what}: {k} of another row changed"
                else:
                    assert _same(ob[k], og[k]), f"{what}: {k} changed"
            assert _same(ob["loss"][B:], og["loss"][B:])


# ----------------------------------------------------------------------------- invalid smoothing
@pytest.mark.parametrize("eps", (-0.1, 1.5, NAN))
def test_invalid_smoothing_is_refused_without_a_launch(gpu, eps):
    from splitcnn import _lib
    B = 17
    names, z, y, zt, yt = _batch(B, 0, gpu)
    with pytest.raises(_lib.SLKError, match="invalid argument"):
        run_xent(gpu, zt, yt, eps)
    lib = _lib.load()
    s = _stream()
    pooled, W3, b3 = k2_operands(gpu, z, B)
    outs = dict(logits=_nan((B, 10), gpu), loss=_nan((B,), gpu), dl=_nan((B, 10), gpu), dp=_nan((B, R.P_SAMPLE), gpu),
                am=_nan((B,), gpu))
    err = _err(gpu)
    p = {k: v.data_ptr() for k, v in outs.items()}
    assert lib.slk_xent_soft_fwd_bwd(zt.data_ptr(), yt.data_ptr(), p["loss"], p["dl"], 1.0, eps, err.data_ptr(), B, s) == 1
    assert lib.slk_fc_logits_xent_soft(pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), p["logits"], p["loss"],
                                       p["dl"], 1.0, eps, err.data_ptr(), B, s) == 1
    assert lib.slk_fc_xent_soft(pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), p["logits"], p["loss"], p["dl"],
                                p["dp"], p["am"], 1.0, eps, err.data_ptr(), B, s) == 1
    cut, wf8, bf = wide_operands(gpu, zt, B)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    dcut = _nan((B, R.CUT_F), gpu, torch.bfloat16)
    slabs = _nan((_lib.query("slk_wide_head_nslab", B), 163850), gpu)
    work = _nan((_lib.query("slk_wide_head_work", B),), gpu)
    assert lib.slk_wide_head_soft(cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), yt.data_ptr(), step.data_ptr(), 7, 0, 1.0, 1.0,
                                  eps, p["logits"], p["loss"], p["dl"], dcut.data_ptr(), slabs.data_ptr(), work.data_ptr(),
                                  err.data_ptr(), 0, B, s) == 1
    torch.cuda.synchronize()
    for k, v in list(outs.items()) + [("dcut", dcut.float()), ("slabs", slabs), ("work", work)]:
        assert torch.isnan(v).all(), f"{k} was written"
    assert int(err) == 0
    # the boundary values are accepted
    for ok in (0.0, 1.0):
        assert lib.slk_xent_soft_fwd_bwd(zt.data_ptr(), yt.data_ptr(), p["loss"], p["dl"], 1.0, ok, err.data_ptr(), B, s) == 0
    torch.cuda.synchronize()
