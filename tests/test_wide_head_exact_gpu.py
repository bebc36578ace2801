"""The K5 server head's entry points (csrc/slk_wide_head.hip: wide_head16_kernel<false / true>,
wide_head_back_kernel<false / true>) called ALONE against float64 (tests/head_ref64.py), bit for bit.

Exact regime: dropout p = 0.5 (keep_threshold 2^31, keep_scale 2.0: a kept value is doubled exactly), integer cut in
[0, 3], Wf in [-2, 2], bf and dlogits in [-3, 3]: |logit| <= 16384 * 2 * 6 + 3 < 2^24, |dcut| <= 2 * 10 * 3 * 2 = 120 (an
even integer: exact in bf16), a slab entry <= 64 * 3 * 6 = 1,152. The mask is oracle.wide_step.dropout_keep's, a
numpy restatement of the hash in 64-bit integers masked to 32.

Batch sizes 1, 15, 16, 17, 63, 64, 65, 130: 16-sample workgroups of the logits kernel, 64-sample groups of the
weight-gradient kernel (nslab = ceil(B / 64): 130 leaves a group of 2). Every output is pre-filled with NaN and has a
sentinel sample (or slab) behind its last row. The exact tests end by mutating the reference (mask drawn at b0 = 0,
the flatten-order mask applied in C8 order, the last sample of a group dropped, keep_scale applied in one direction
only) and asserting that the kernel's result differs.
"""
import numpy as np
import pytest
import torch

import head_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
BATCHES = [1, 15, 16, 17, 63, 64, 65, 130]
SEED, STEP, B0 = 7, 3, 5
HALF = (2 ** 31, 2.0)                                            # p = 0.5
QUARTER = (2 ** 30, float(np.float32(1.0 / 0.75)))               # the default p = 0.25
NSERVER = 163850


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _operands(dev, cut, Wf):
    """cut [B,16384] (flatten order) -> bf16 in C8 order; Wf -> its C8-ordered f32 shadow."""
    from splitcnn import _lib
    cut8 = R.c8_of_flat(cut).to(torch.bfloat16).contiguous()
    assert torch.equal(cut8.double(), R.c8_of_flat(cut.double())), "the cut is not exact in bf16"
    wf = Wf.to(torch.float32).contiguous()
    wf8 = _nan((10, R.CUT_F), dev)
    _lib.call("slk_wide_fc_shadow", wf.data_ptr(), wf8.data_ptr(), _stream())
    torch.cuda.synchronize()
    return cut8, wf8


def _step(dev, step=STEP):
    return torch.full((1,), step, dtype=torch.int32, device=dev)


def _run_fwd(dev, cut8, wf8, bf, drop, b0, step=STEP):
    from splitcnn import _lib
    B = cut8.shape[0]
    logits = _nan((B + 1, 10), dev)
    st = _step(dev, step)
    bff = bf.to(torch.float32).contiguous()
    _lib.call("slk_wide_head_fwd", cut8.data_ptr(), wf8.data_ptr(), bff.data_ptr(), st.data_ptr(), SEED, drop[0], drop[1],
              logits.data_ptr(), b0, B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(logits, B * 10, "slk_wide_head_fwd logits")
    return logits[:B]


def _run_bwd(dev, cut8, wf8, dl, drop, b0, step=STEP):
    from splitcnn import _lib
    B = cut8.shape[0]
    nslab = _lib.query("slk_wide_head_nslab", B)
    assert nslab == -(-B // 64)
    dcut = _nan((B + 1, R.CUT_F), dev, torch.bfloat16)
    slabs = _nan((nslab + 1, NSERVER), dev)
    st = _step(dev, step)
    dlf = dl.to(torch.float32).contiguous()
    _lib.call("slk_wide_head_bwd", cut8.data_ptr(), wf8.data_ptr(), dlf.data_ptr(), st.data_ptr(), SEED, drop[0], drop[1],
              dcut.data_ptr(), slabs.data_ptr(), b0, B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(dcut, B * R.CUT_F, "slk_wide_head_bwd dcut")
    R.assert_sentinel(slabs, nslab * NSERVER, "slk_wide_head_bwd slabs")
    return dcut[:B], slabs[:nslab]


def _run_fused(dev, cut8, wf8, bf, y, drop, b0, step=STEP, grad_scale=None):
    from splitcnn import _lib
    B = cut8.shape[0]
    nslab, nwork = _lib.query("slk_wide_head_nslab", B), _lib.query("slk_wide_head_work", B)
    assert nwork * 4 == B * 2048
    o = dict(logits=_nan((B + 1, 10), dev), loss=_nan((B + 1,), dev), dl=_nan((B + 1, 10), dev),
             dcut=_nan((B + 1, R.CUT_F), dev, torch.bfloat16), slabs=_nan((nslab + 1, NSERVER), dev),
             work=_nan((nwork + 512,), dev))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _step(dev, step)
    bff = bf.to(torch.float32).contiguous()
    _lib.call("slk_wide_head", cut8.data_ptr(), wf8.data_ptr(), bff.data_ptr(), y.data_ptr(), st.data_ptr(), SEED, drop[0],
              drop[1], 1.0 / B if grad_scale is None else grad_scale, o["logits"].data_ptr(), o["loss"].data_ptr(),
              o["dl"].data_ptr(), o["dcut"].data_ptr(), o["slabs"].data_ptr(), o["work"].data_ptr(), err.data_ptr(), b0, B,
              _stream())
    torch.cuda.synchronize()
    assert int(err) == 0
    for k, used in (("logits", B * 10), ("loss", B), ("dl", B * 10), ("dcut", B * R.CUT_F), ("slabs", nslab * NSERVER),
                    ("work", nwork)):
        R.assert_sentinel(o[k], used, f"slk_wide_head {k}")
    out = {k: v[:n] for (k, v), n in zip(o.items(), (B, B, B, B, nslab, nwork))}
    out["work"] = out["work"].view(torch.uint8).reshape(B, 2048)
    return out


def _keep(dev, B, p, b0, step=STEP):
    k = R.keep_mask(SEED, step, B, p, b0=b0)
    return k, torch.from_numpy(k).to(dev)


def _c8_mask(keep_t):
    """The flatten-order mask wrongly applied to the C8-ordered features."""
    return R.c8_of_flat(keep_t.double()) > 0


# ----------------------------------------------------------------------------- exact: forward
@pytest.mark.parametrize("B", BATCHES)
def test_head_fwd_exact(gpu, B):
    cut, Wf, bf = R.head_int_case(B, 900 + B, gpu)
    _, keep = _keep(gpu, B, 0.5, B0)
    assert float(R.head_fwd(cut, Wf.abs(), bf.abs(), keep, 2.0).max()) < 2 ** 24
    cut8, wf8 = _operands(gpu, cut, Wf)
    logits = _run_fwd(gpu, cut8, wf8, bf, HALF, B0)
    R.assert_bits_f32(logits, R.head_fwd(cut, Wf, bf, keep, 2.0), f"slk_wide_head_fwd B={B}")
    _, keep0 = _keep(gpu, B, 0.5, 0)
    for name, k, sc in (("mask at b0 = 0", keep0, 2.0), ("mask in C8 order", _c8_mask(keep), 2.0),
                        ("keep_scale missing", keep, 1.0)):
        assert not torch.equal(logits.double(), R.head_fwd(cut, Wf, bf, k, sc)), f"mutation '{name}' not noticed"


# ----------------------------------------------------------------------------- exact: backward
@pytest.mark.parametrize("B", BATCHES)
def test_head_bwd_exact(gpu, B):
    """dcut == bf16(float64) bit for bit (small even integers), every slab == float64's sum over its 64-sample group,
    dbf included."""
    cut, Wf, _ = R.head_int_case(B, 950 + B, gpu)
    dl = R.dlogits_int(B, 960 + B, gpu)
    _, keep = _keep(gpu, B, 0.5, B0)
    wdc, wsl = R.head_bwd(cut, Wf, dl, keep, 2.0)
    worst = R.head_bwd(cut, Wf.abs(), dl.abs(), keep, 2.0)
    assert float(worst[0].max()) <= 256 and float(worst[1].max()) < 2 ** 24
    cut8, wf8 = _operands(gpu, cut, Wf)
    dcut, slabs = _run_bwd(gpu, cut8, wf8, dl, HALF, B0)
    want8 = R.c8_of_flat(R.pos_zero(wdc)).to(torch.bfloat16)
    assert torch.equal(want8.double(), R.c8_of_flat(R.pos_zero(wdc)))
    bad = _bits(dcut) != _bits(want8)
    assert not bad.any(), f"dcut B={B}: {int(bad.sum())} values differ from bf16(float64)"
    R.assert_bits_f32(slabs, wsl, f"slk_wide_head_bwd slabs B={B}")
    assert torch.equal(slabs[:, 163840:].double().sum(0), dl.sum(0))
    # mutated references
    got_flat = R.flat_of_c8(dcut.double())
    _, keep0 = _keep(gpu, B, 0.5, 0)
    muts = {"mask at b0 = 0": R.head_bwd(cut, Wf, dl, keep0, 2.0),
            "mask in C8 order": R.head_bwd(cut, Wf, dl, _c8_mask(keep), 2.0),
            "keep_scale in one direction": R.head_bwd(cut, Wf, dl, keep, 2.0, mutate="scale_once")}
    if B > 1:
        muts["last sample of a group dropped"] = R.head_bwd(cut, Wf, dl, keep, 2.0, mutate="drop_last_sample")
    for name, (mdc, msl) in muts.items():
        assert not (torch.equal(got_flat, mdc) and torch.equal(slabs.double(), msl)), f"mutation '{name}' not noticed"
    assert not torch.equal(got_flat, muts["keep_scale in one direction"][0])
    assert not torch.equal(slabs.double(), muts["mask at b0 = 0"][1])
    assert not torch.equal(slabs.double(), muts["mask in C8 order"][1])


# ----------------------------------------------------------------------------- fused == split, bit for bit
@pytest.mark.parametrize("B", BATCHES)
def test_fused_head_equals_split_pair(gpu, B):
    """Real-valued cut at the default p = 0.25: slk_wide_head's logits == slk_wide_head_fwd's; from the dlogits it
    produced, slk_wide_head_bwd reproduces its dcut and its slabs; its `work` bytes are the oracle's mask."""
    gen = torch.Generator().manual_seed(1200 + B)
    cut = torch.randn((B, R.CUT_F), generator=gen).clamp_min(0.0).to(torch.bfloat16).double().to(gpu)
    Wf = (torch.randn((10, R.CUT_F), generator=gen) * 0.02).float().to(gpu)
    bf = (torch.randn((10,), generator=gen) * 0.1).float().to(gpu)
    y = torch.randint(0, 10, (B,), generator=gen).to(gpu)
    cut8, wf8 = _operands(gpu, cut, Wf)
    f = _run_fused(gpu, cut8, wf8, bf, y, QUARTER, B0)
    logits = _run_fwd(gpu, cut8, wf8, bf, QUARTER, B0)
    assert torch.equal(_bits(f["logits"]), _bits(logits)), "fused logits != slk_wide_head_fwd"
    dcut, slabs = _run_bwd(gpu, cut8, wf8, f["dl"], QUARTER, B0)
    assert torch.equal(_bits(f["dcut"]), _bits(dcut)), "fused dcut != slk_wide_head_bwd"
    assert torch.equal(_bits(f["slabs"]), _bits(slabs)), "fused slabs != slk_wide_head_bwd"
    keep, keep_t = _keep(gpu, B, 0.25, B0)
    assert np.array_equal(f["work"].cpu().numpy(), R.keep_bytes(keep)), "work bits != the oracle mask"
    # and against float64 at the f32 accumulation bar, so that two equal but wrong results cannot pass
    want = R.head_fwd(cut, Wf, bf, keep_t, QUARTER[1])
    assert (f["logits"].double() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    assert torch.equal(f["dcut"].float() != 0, R.c8_of_flat(keep_t.double()) > 0), "dcut zeros != the dropped features"


# ----------------------------------------------------------------------------- the uint32 wrap of the hash index
@pytest.mark.parametrize("b0,step", [(262140, 3), (262140, 2 ** 31 - 1), (0, 2 ** 31 - 1)])
def test_mask_index_wraps_like_the_oracle(gpu, b0, step):
    """b0 = 262140, B = 8: (b0 + b) * 16384 passes 2^32 from sample 4 on and wraps in uint32, as the oracle's 64-bit
    product masked to 32 bits does; a step counter of 2^31 - 1 multiplies in uint32 too. The mask is read from `work`
    (fused head) and from which dcut elements are zero (both backward kernels)."""
    B = 8
    gen = torch.Generator().manual_seed(77)
    cut = torch.randint(1, 4, (B, R.CUT_F), generator=gen).double().to(gpu)
    Wf = (torch.randn((10, R.CUT_F), generator=gen) * 1e-3).float().to(gpu)    # logits ~ 0.4: no saturated softmax
    bf = torch.zeros(10, device=gpu)
    y = torch.randint(0, 10, (B,), generator=gen).to(gpu)
    dl = torch.randn((B, 10), generator=gen).float().to(gpu)
    keep, keep_t = _keep(gpu, B, 0.5, b0, step)
    assert 0.45 < keep.mean() < 0.55
    if b0:
        assert (keep != R.keep_mask(SEED, step, B, 0.5, b0=0)).mean() > 0.25
        assert (keep[4:] == R.keep_mask(SEED, step, 4, 0.5, b0=0)).all(), "samples 262144.. wrap onto samples 0.."
    cut8, wf8 = _operands(gpu, cut, Wf)
    f = _run_fused(gpu, cut8, wf8, bf, y, HALF, b0, step, grad_scale=1.0)
    assert (f["dl"] != 0).all()
    assert np.array_equal(f["work"].cpu().numpy(), R.keep_bytes(keep)), "work bits != the oracle mask"
    want_nz = R.c8_of_flat(keep_t.double()) > 0
    assert torch.equal(f["dcut"].float() != 0, want_nz), "fused dcut zeros != the oracle mask"
    dcut, _ = _run_bwd(gpu, cut8, wf8, dl, HALF, b0, step)
    assert torch.equal(dcut.float() != 0, want_nz), "slk_wide_head_bwd dcut zeros != the oracle mask"
    logits = _run_fwd(gpu, cut8, wf8, bf, HALF, b0, step)
    want = R.head_fwd(cut, Wf, bf, keep_t, 2.0)
    assert (logits.double() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    assert torch.equal(_bits(logits), _bits(f["logits"]))
