"""slk_wide_head_mx (csrc/slk_wide_head_mx.hip) alone: the K5 head reading MX cut records and writing the cut gradient
as records, against the three launches it replaces (slk_cutmx_decode, slk_wide_head, slk_cutmx_encode) bit for bit, and
against float64 over the reference-decoded records (tests/cutmx_ref.py, tests/head_ref64.py).

Rows (by sample index mod 8): integer post-ReLU data in [0, 3] with exact zeros and an all-zero block (0, 4, 7);
cutmx_ref's boundary row — the 0x7F7F top clamp, bf16 subnormals at the -100 exponent clamp, -0 blocks, signed data —
with a NaN and a +inf planted (1); a corrupted header word (2); a scale byte of 26 (3); a label out of range (5);
signed gradient-like data (6). An e4m3 NaN code is planted in a received payload. Dropout p = 0.5 (keep_scale 2).
"""
import numpy as np
import pytest
import torch

import cutmx_ref as M
import head_ref64 as R

pytestmark = pytest.mark.gpu

SEED, STEP, B0 = 7, 3, 5
THRESH, KEEP_SCALE = 2 ** 31, 2.0
NSERVER = 163850
NAMES = {0: "e2m1", 1: "e4m3"}
_cache = {}


def _lib():
    from splitcnn import _lib
    return _lib


def _hsg():
    n = 1
    while _lib().query("slk_wide_head_nslab", n + 1) == 1:
        n += 1
    return n


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _clean_rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, 4, (n, R.CUT_F), generator=g) * (torch.rand((n, R.CUT_F), generator=g) < 0.6)
    rows[:, 64:96] = 0                                    # an all-zero block
    return M.to_bits(rows.to(torch.bfloat16))


def _rows(B):
    """uint16 bits [B, 16384] by the module docstring's pattern (computed once per B)."""
    if B not in _cache:
        g = torch.Generator().manual_seed(31 + B)
        rows = _clean_rows(B, 100 + B)
        for i in range(B):
            if i % 8 == 1:
                rows[i] = M._boundaries(g)
                rows[i, 40], rows[i, 5000] = 0x7FC0, 0x7F80
            if i % 8 == 6:
                rows[i] = M.to_bits((torch.randn(R.CUT_F, generator=g) * 1e-3).to(torch.bfloat16))
                rows[i, 8:16] = 0x8000
        _cache[B] = rows
    return _cache[B]


def _weights(dev):
    if "w" not in _cache:
        _, Wf, bf = R.head_int_case(1, 4321)
        _cache["w"] = (Wf, bf)
    Wf, bf = _cache["w"]
    wf8 = torch.empty((10, R.CUT_F), device=dev)
    wf = Wf.float().to(dev)
    _lib().call("slk_wide_fc_shadow", wf.data_ptr(), wf8.data_ptr(), _stream())
    return Wf, bf, wf8, bf.float().to(dev)


def _records(dev, bits, fmt):
    """slk_cutmx_encode of the rows, one guard record behind them."""
    n = bits.shape[0]
    x = M.from_bits(bits).to(dev)
    rec = torch.full((n + 1, M.RECORD[NAMES[fmt]]), 0xFF, dtype=torch.uint8, device=dev)
    _lib().call("slk_cutmx_encode", x.data_ptr(), n, fmt, rec.data_ptr(), _stream())
    return rec


def _outputs(dev, B, fmt_out, nwork):
    nslab = _lib().query("slk_wide_head_nslab", B)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    o = dict(logits=nan(B + 1, 10), loss=nan(B + 1), dl=nan(B + 1, 10), slabs=nan(nslab + 1, NSERVER),
             work=torch.zeros(nwork + 4, device=dev), label_err=torch.zeros(1, dtype=torch.int32, device=dev),
             rec_err=torch.zeros(1, dtype=torch.int32, device=dev))
    o["out"] = (torch.full((B + 1, R.CUT_F), float("nan"), dtype=torch.bfloat16, device=dev) if fmt_out < 0 else
                torch.full((B + 1, M.RECORD[NAMES[fmt_out]]), 0xFF, dtype=torch.uint8, device=dev))
    return o


def _new(dev, rec, fmt_in, fmt_out, y, wf8, bf, B, gs):
    L = _lib()
    o = _outputs(dev, B, fmt_out, L.query("slk_wide_head_mx_work", B))
    st = torch.full((1,), STEP, dtype=torch.int32, device=dev)
    L.call("slk_wide_head_mx", rec.data_ptr(), fmt_in, wf8.data_ptr(), bf.data_ptr(), y.data_ptr(), st.data_ptr(), SEED,
           THRESH, KEEP_SCALE, gs, o["logits"].data_ptr(), o["loss"].data_ptr(), o["dl"].data_ptr(), o["out"].data_ptr(),
           fmt_out, o["slabs"].data_ptr(), o["work"].data_ptr(), o["label_err"].data_ptr(), o["rec_err"].data_ptr(), B0, B,
           _stream())
    torch.cuda.synchronize()
    return o


def _three_launches(dev, rec, fmt_in, fmt_out, y, wf8, bf, B, gs):
    L = _lib()
    o = _outputs(dev, B, fmt_out, L.query("slk_wide_head_work", B))
    st = torch.full((1,), STEP, dtype=torch.int32, device=dev)
    cut = torch.empty((B, R.CUT_F), dtype=torch.bfloat16, device=dev)
    dcut = o["out"] if fmt_out < 0 else torch.empty_like(cut)
    L.call("slk_cutmx_decode", rec.data_ptr(), B, fmt_in, cut.data_ptr(), o["rec_err"].data_ptr(), _stream())
    L.call("slk_wide_head", cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), y.data_ptr(), st.data_ptr(), SEED, THRESH,
           KEEP_SCALE, gs, o["logits"].data_ptr(), o["loss"].data_ptr(), o["dl"].data_ptr(), dcut.data_ptr(),
           o["slabs"].data_ptr(), o["work"].data_ptr(), o["label_err"].data_ptr(), B0, B, _stream())
    if fmt_out >= 0:
        L.call("slk_cutmx_encode", dcut.data_ptr(), B, fmt_out, o["out"].data_ptr(), _stream())
    torch.cuda.synchronize()
    return o


def _same(a, b):
    """Bit for bit; NaNs of floats compare by NaN-ness (records and integers: every byte)."""
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    a, b = a.float(), b.float()
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


@pytest.mark.parametrize("B", [1, 17, "HSG+1"])
@pytest.mark.parametrize("fmt_out", [-1, 0, 1])
@pytest.mark.parametrize("fmt_in", [0, 1])
def test_equals_decode_head_encode(gpu, fmt_in, fmt_out, B):
    B = _hsg() + 1 if B == "HSG+1" else B
    _, _, wf8, bf = _weights(gpu)
    rec = _records(gpu, _rows(B), fmt_in)
    y = (torch.arange(B, device=gpu) * 7) % 10
    if B > 1:
        rec[2, 4] ^= 1                                   # header word 1
        rec[3, M.HEADER + 7] = 26                        # one block's scale byte below 27
        y[5] = 10
        if fmt_in == 1:
            rec[1, M.PAYLOAD + 100] = 0x7F               # an e4m3 NaN code
    got = _new(gpu, rec, fmt_in, fmt_out, y, wf8, bf, B, 1.0 / 8)
    want = _three_launches(gpu, rec, fmt_in, fmt_out, y, wf8, bf, B, 1.0 / 8)
    for k in ("logits", "loss", "dl", "slabs", "out", "label_err", "rec_err"):   # guard rows included
        assert _same(got[k], want[k]), f"{k} differs from decode + slk_wide_head + encode"
    assert int(got["rec_err"]) == int(got["label_err"]) == (1 if B > 1 else 0)
    assert not torch.isnan(got["logits"][0]).any() and (B == 1 or torch.isnan(got["logits"][1:4]).all(1).all())
    if fmt_out >= 0 and B > 1:
        assert (got["out"][1, M.HEADER:M.PAYLOAD] == 0xFF).any(), "a NaN cut gradient must leave poisoned blocks"


@pytest.mark.parametrize("fmt_in", [0, 1])
def test_clean_batch_against_float64(gpu, fmt_in):
    """All-clean rows at B = HSG + 1 (two slab groups), float64 over cutmx_ref's decode of the records. The decoded
    operands are small integers (the exact regime of head_ref64.head_int_case), so the logits are float64's bit for
    bit; loss_i and dlogits are held to head_ref64.loss_bound / grad_bound. The summed slabs are held to what those
    bounds imply: a slab entry is an fma chain of at most HSG products dl * d with d exact, so its error is at most
    sum_b grad_bound[b, j] |d[b, f]| (the dlogits' own error) + HSG 2^-24 sum_b |dl64 d| (one rounding per step)."""
    hsg = _hsg()
    B, gs = hsg + 1, 1.0 / 8
    Wf, bf64, wf8, bf = _weights(gpu)
    rec = _records(gpu, _clean_rows(B, 555), fmt_in)
    y = (torch.arange(B, device=gpu) * 3) % 10
    got = _new(gpu, rec, fmt_in, -1, y, wf8, bf, B, gs)
    assert int(got["rec_err"]) == 0 and int(got["label_err"]) == 0
    dec, flag = M.decode(rec[:B].cpu().numpy(), NAMES[fmt_in])
    assert flag == 0
    cut = R.flat_of_c8(dec.double())
    keep = torch.from_numpy(R.keep_mask(SEED, STEP, B, 0.5, b0=B0))
    z = R.head_fwd(cut, Wf, bf64, keep, KEEP_SCALE)
    R.assert_bits_f32(got["logits"][:B].cpu(), z, "logits")
    loss64, dl64, p64 = R.xent64(z.numpy(), y.cpu().numpy(), gs)
    assert (np.abs(got["loss"][:B].cpu().numpy() - loss64) <= R.loss_bound(z.numpy(), loss64)).all()
    gb = R.grad_bound(z.numpy(), p64, gs)
    assert (np.abs(got["dl"][:B].cpu().numpy() - dl64) <= gb).all()
    d = np.concatenate([(cut * keep * KEEP_SCALE).numpy(), np.ones((B, 1))], axis=1)     # [dWf | dbf] operands
    want = np.concatenate([(dl64.T @ d[:, :-1]).reshape(-1), dl64.sum(0)])
    tol = gb.T @ np.abs(d) + hsg * 2.0 ** -24 * (np.abs(dl64).T @ np.abs(d))
    tol = np.concatenate([tol[:, :-1].reshape(-1), tol[:, -1]])
    summed = got["slabs"][:2].double().sum(0).cpu().numpy()
    assert (np.abs(summed - want) <= tol).all(), float(np.abs(summed - want).max())


def test_refusals(gpu):
    L = _lib().load()
    t = torch.zeros(8192, device=gpu)
    p = t.data_ptr()
    args = [p, 0, p, p, p, p, SEED, THRESH, KEEP_SCALE, 1.0, p, p, p, p, 0, p, p, p, p, 0, 1, None]
    for pos, bad in ((20, -1), (1, 2), (1, -1), (14, 2), (14, -2), (19, -1), (0, p + 8), (13, p + 8), (16, p + 4),
                     *((i, None) for i in (0, 2, 3, 4, 5, 10, 11, 12, 13, 15, 16, 17, 18))):
        a = list(args)
        a[pos] = bad
        assert L.slk_wide_head_mx(*a) == 1, f"argument {pos} = {bad!r} was not refused"
    args[20] = 0
    assert L.slk_wide_head_mx(*args) == 0 and _lib().query("slk_wide_head_mx_work", 0) == 0
