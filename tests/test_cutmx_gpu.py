"""The slk_cutmx_* kernels alone (codec.MxCut's methods) against tests/cutmx_ref.py, bit for bit: groups of n = 1, 3
and 5 samples of the generator's set (every sample, both formats), outputs pre-filled with NaN / 0xA5 and a sentinel
row behind the last record or row; malformed records; a captured graph; the refusals."""
import numpy as np
import pytest
import torch

import cutmx_ref as R

pytestmark = pytest.mark.gpu

FMTS = list(R.FORMATS)
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ref():
    """The generator's set, and the reference's records and decoded rows per format — computed once, never written."""
    x = R.sample_tensor()
    out = {"names": [n for n, _ in R.samples()], "x": x}
    for fmt in FMTS:
        rec = R.encode(x, fmt)
        dec, flag = R.decode(rec, fmt)
        assert flag == 0
        out[fmt] = (rec, R.to_bits(dec))
    return out


def _codec(fmt):
    from splitcnn.codec import MxCut
    return MxCut(fwd=fmt, bwd=None)


def _groups(N, n):
    """Consecutive groups of n samples covering all N (the last one overlaps its neighbour)."""
    return [min(i, N - n) for i in range(0, N, n)]


def _rec_buffer(n, fmt, dev):
    """uint8 [n + 1, R] filled with 0xA5; row n is the sentinel."""
    buf = torch.full((n + 1, R.RECORD[fmt]), 0xA5, dtype=torch.uint8, device=dev)
    buf[n] = SENTINEL
    return buf


def _row_buffer(n, dev):
    """bf16 [n + 1, 32, 8, 8, 8] of NaN; row n is the sentinel (bits 0x5A5A)."""
    buf = torch.full((n + 1, 32, 8, 8, 8), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[n] = R.from_bits(np.full(R.SAMPLE, 0x5A5A, dtype=np.uint16)).view(32, 8, 8, 8).to(dev)
    return buf


def _rows_ok(buf, n):
    return bool((R.to_bits(buf[n]) == 0x5A5A).all())


def _first_diff(got, want):
    d = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return [(int(i), int(got.reshape(-1)[i]), int(want.reshape(-1)[i])) for i in d[:6]], len(d)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_encode_decode_roundtrip_match_reference(gpu, ref, fmt, n):
    q = _codec(fmt)
    want_rec, want_dec = ref[fmt]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for i in _groups(len(ref["names"]), n):
        x = ref["x"][i:i + n].view(n, 32, 8, 8, 8).to(gpu)
        # encode: records byte for byte, headers and scale bytes included
        rec = _rec_buffer(n, fmt, gpu)
        q.encode(x, rec[:n], "fwd")
        got = rec.cpu().numpy()
        assert np.array_equal(got[:n], want_rec[i:i + n]), (fmt, i, _first_diff(got[:n], want_rec[i:i + n]))
        assert (got[n] == SENTINEL).all()
        # decode of the reference's records
        out = _row_buffer(n, gpu)
        q.decode(torch.from_numpy(want_rec[i:i + n].copy()).to(gpu), out[:n], err, "fwd")
        g = R.to_bits(out[:n]).reshape(n, -1)
        assert np.array_equal(g, want_dec[i:i + n]), (fmt, i, _first_diff(g, want_dec[i:i + n]))
        assert _rows_ok(out, n)
        # roundtrip = decode(encode), out of place and in place
        rt = _row_buffer(n, gpu)
        q.roundtrip(x, rt[:n], "fwd")
        g = R.to_bits(rt[:n]).reshape(n, -1)
        assert np.array_equal(g, want_dec[i:i + n]), (fmt, i, _first_diff(g, want_dec[i:i + n]))
        assert _rows_ok(rt, n)
        inp = _row_buffer(n, gpu)
        inp[:n] = x
        q.roundtrip(inp[:n], inp[:n], "fwd")
        assert np.array_equal(R.to_bits(inp[:n]).reshape(n, -1), want_dec[i:i + n]), (fmt, i)
        assert _rows_ok(inp, n)
        # decode(encode) through the kernel's own record
        out2 = _row_buffer(n, gpu)
        q.decode(rec[:n], out2[:n], err, "fwd")
        assert torch.equal(out2[:n].view(torch.int16), rt[:n].view(torch.int16))
    assert int(err.item()) == 0   # reference records are well formed, the poisoned blocks included


@pytest.mark.parametrize("fmt", FMTS)
def test_a_slice_of_a_batch_is_the_slice_of_its_bytes(gpu, ref, fmt):
    q = _codec(fmt)
    N = len(ref["names"])
    x = ref["x"].view(N, 32, 8, 8, 8).to(gpu)
    whole = torch.zeros(N, R.RECORD[fmt], dtype=torch.uint8, device=gpu)
    q.encode(x, whole, "fwd")
    part = torch.zeros(4, R.RECORD[fmt], dtype=torch.uint8, device=gpu)
    q.encode(x[5:9], part, "fwd")
    assert torch.equal(part, whole[5:9])
    # and decoding a slice of the records (an aligned slice of bytes: R is a multiple of 16) gives the slice of rows
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    rows = torch.zeros_like(x)
    q.decode(whole, rows, err, "fwd")
    some = torch.zeros_like(x[:3])
    q.decode(whole[7:10], some, err, "fwd")
    assert torch.equal(some.view(torch.int16), rows[7:10].view(torch.int16)) and int(err.item()) == 0


def _malformed_headers(fmt):
    """name -> a function that breaks one record's header in place."""
    def word(i, v):
        def f(r):
            r[:16].view(np.uint32)[i] = v
        return f
    other = 0x11 if fmt == "e2m1" else 0x10
    return {"block_length": word(0, 16), "other_mx_format": word(1, other), "fp8_format_0": word(1, 0),
            "fp8_format_1": word(1, 1), "reserved_2": word(2, 1), "reserved_3": word(3, 0x01000000)}


@pytest.mark.parametrize("fmt", FMTS)
def test_malformed_headers_poison_their_sample_only(gpu, ref, fmt):
    q = _codec(fmt)
    want_rec, want_dec = ref[fmt]
    for kind, breaker in _malformed_headers(fmt).items():
        recs = want_rec[2:5].copy()
        breaker(recs[1])
        err = torch.zeros(1, dtype=torch.int32, device=gpu)
        out = _row_buffer(3, gpu)
        q.decode(torch.from_numpy(recs).to(gpu), out[:3], err, "fwd")
        got = R.to_bits(out[:3]).reshape(3, -1)
        assert int(err.item()) == 1, kind
        assert (got[1] == 0x7FC0).all(), kind
        assert np.array_equal(got[0], want_dec[2]) and np.array_equal(got[2], want_dec[4]) and _rows_ok(out, 3), kind
        want, flag = R.decode(recs, fmt)
        assert flag == 1 and np.array_equal(got, R.to_bits(want))


@pytest.mark.parametrize("fmt", FMTS)
def test_an_fp8_record_is_malformed_for_the_mx_decoder(gpu, fmt):
    """An FP8 cut record (int32 e, uint32 fmt 0 / 1, zeros, payload) laid into the MX decoder's stride: word 0 is not
    32 and word 1 is not 0x10 + fmt."""
    import cut8_ref
    x = torch.linspace(-3, 3, R.SAMPLE).to(torch.bfloat16)[None]
    rec8 = cut8_ref.encode(x, "e4m3")[0]
    buf = np.zeros((1, R.RECORD[fmt]), dtype=np.uint8)
    k = min(len(rec8), buf.shape[1])
    buf[0, :k] = rec8[:k]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(1, gpu)
    _codec(fmt).decode(torch.from_numpy(buf).to(gpu), out[:1], err, "fwd")
    assert int(err.item()) == 1 and (R.to_bits(out[:1]) == 0x7FC0).all() and _rows_ok(out, 1)


@pytest.mark.parametrize("fmt", FMTS)
def test_bad_scale_bytes_poison_their_block_only(gpu, ref, fmt):
    q = _codec(fmt)
    want_rec, want_dec = ref[fmt]
    recs = want_rec[:3].copy()
    blocks = {0: [0], 1: [7, 255, 256, 511], 2: [300]}
    for row, ks in blocks.items():
        for j, k in enumerate(ks):
            recs[row, R.HEADER + k] = 26 if j % 2 == 0 else 0
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(3, gpu)
    q.decode(torch.from_numpy(recs).to(gpu), out[:3], err, "fwd")
    got = R.to_bits(out[:3]).reshape(3, R.BLOCKS, R.BLOCK)
    assert int(err.item()) == 1 and _rows_ok(out, 3)
    for row, ks in blocks.items():
        assert (got[row, ks] == 0x7FC0).all()
        others = np.setdiff1d(np.arange(R.BLOCKS), ks)
        assert np.array_equal(got[row, others], want_dec[row].reshape(R.BLOCKS, R.BLOCK)[others])   # 511 (or 508) untouched
    want, flag = R.decode(recs, fmt)
    assert flag == 1 and np.array_equal(got.reshape(3, -1), R.to_bits(want))
    # scale byte 27 (e = -100) is the lowest well-formed one, 254 the highest; 0xFF is poison, not malformed
    ok = want_rec[:1].copy()
    ok[0, R.HEADER + 1], ok[0, R.HEADER + 2], ok[0, R.HEADER + 3] = 27, 254, 0xFF
    err.zero_()
    out = _row_buffer(1, gpu)
    q.decode(torch.from_numpy(ok).to(gpu), out[:1], err, "fwd")
    want, flag = R.decode(ok, fmt)
    assert flag == 0 and int(err.item()) == 0 and np.array_equal(R.to_bits(out[:1]).reshape(1, -1), R.to_bits(want))


def test_received_e4m3_nan_codes_propagate(gpu, ref):
    q = _codec("e4m3")
    want_rec, want_dec = ref["e4m3"]
    recs = want_rec[:2].copy()
    spots = [0, 31, 32, 5000, 16383]
    for j, s in enumerate(spots):
        recs[1, R.PAYLOAD + s] = 0x7F if j % 2 == 0 else 0xFF
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(2, gpu)
    q.decode(torch.from_numpy(recs).to(gpu), out[:2], err, "fwd")
    got = R.to_bits(out[:2]).reshape(2, -1)
    assert int(err.item()) == 0 and (got[1, spots] == 0x7FC0).all()
    keep = np.setdiff1d(np.arange(R.SAMPLE), spots)
    assert np.array_equal(got[1, keep], want_dec[1, keep]) and np.array_equal(got[0], want_dec[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_encode_and_decode_inside_a_captured_graph(gpu, ref, fmt):
    q = _codec(fmt)
    want_rec, want_dec = ref[fmt]
    n = 3
    x = torch.zeros(n, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu)
    rec = q.records("graph", n, gpu, direction="fwd")
    out = torch.zeros_like(x)
    rt = torch.zeros_like(x)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)

    def work():
        q.encode(x, rec, "fwd")
        q.decode(rec, out, err, "fwd")
        q.roundtrip(x, rt, "fwd")
    from splitcnn.graphs import capture
    g, _ = capture(work, gpu)
    for i in (0, 4, 9):   # new contents, same buffers
        x.copy_(ref["x"][i:i + n].view(n, 32, 8, 8, 8))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rec.cpu().numpy(), want_rec[i:i + n])
        assert np.array_equal(R.to_bits(out).reshape(n, -1), want_dec[i:i + n])
        assert torch.equal(rt.view(torch.int16), out.view(torch.int16))
    assert int(err.item()) == 0


def test_refusals_and_queries(gpu):
    from splitcnn import _lib
    from splitcnn.codec import MxCut
    assert [_lib.query("slk_cutmx_record_bytes", f) for f in (0, 1, 2, -1, 0x10)] == [8720, 16912, -1, -1, -1]
    q = MxCut()
    x = torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    rec4 = torch.zeros(2, 8720, dtype=torch.uint8, device=gpu)
    rec8 = torch.zeros(2, 16912, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="expected shape"):   # the other direction's record width
        q.encode(x, rec8, "fwd")
    with pytest.raises(ValueError, match="expected shape"):
        q.decode(rec4, x, err, "bwd")
    with pytest.raises(TypeError):             # f32 rows
        q.roundtrip(x.float(), x.float(), "fwd")
    with pytest.raises(ValueError, match="16384 elements per sample"):
        q.roundtrip(x.view(4, -1), x.view(4, -1), "fwd")
    with pytest.raises(ValueError, match="samples like x"):
        q.roundtrip(x, x[:1], "fwd")
    with pytest.raises(ValueError, match="contiguous"):
        q.roundtrip(x.transpose(1, 2), x, "fwd")
    flat = torch.zeros(2 * R.SAMPLE + 8, dtype=torch.bfloat16, device=gpu)
    off = flat[4:4 + 2 * R.SAMPLE].view(2, R.SAMPLE)   # 8 bytes past a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte aligned"):
        q.roundtrip(off, x, "fwd")
    with pytest.raises(ValueError, match="16-byte aligned"):
        q.encode(x, torch.zeros(2 * 8720 + 16, dtype=torch.uint8, device=gpu)[8:8 + 2 * 8720].view(2, 8720), "fwd")
    with pytest.raises(TypeError):             # the flag's dtype
        q.decode(rec4, x, err.float(), "fwd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.roundtrip(x.cpu(), x.cpu(), "fwd")
    # the C entries themselves: every refusal returns hipErrorInvalidValue (1) before any launch
    lib = _lib.load()
    st = torch.cuda.current_stream(gpu).cuda_stream
    X, R4, E = x.data_ptr(), rec4.data_ptr(), err.data_ptr()
    assert lib.slk_cutmx_encode(X, -1, 0, R4, st) == 1 and lib.slk_cutmx_encode(X, 2, 2, R4, st) == 1
    assert lib.slk_cutmx_encode(None, 2, 0, R4, st) == 1 and lib.slk_cutmx_encode(X, 2, 0, None, st) == 1
    assert lib.slk_cutmx_encode(X + 2, 2, 0, R4, st) == 1 and lib.slk_cutmx_encode(X, 2, 0, R4 + 8, st) == 1
    assert lib.slk_cutmx_decode(R4, -1, 0, X, E, st) == 1 and lib.slk_cutmx_decode(R4, 2, -1, X, E, st) == 1
    assert lib.slk_cutmx_decode(None, 2, 0, X, E, st) == 1 and lib.slk_cutmx_decode(R4, 2, 0, None, E, st) == 1
    assert lib.slk_cutmx_decode(R4, 2, 0, X, None, st) == 1 and lib.slk_cutmx_decode(R4 + 4, 2, 0, X, E, st) == 1
    assert lib.slk_cutmx_decode(R4, 2, 0, X + 8, E, st) == 1
    assert lib.slk_cutmx_roundtrip(X, -1, 0, X, st) == 1 and lib.slk_cutmx_roundtrip(X, 2, 3, X, st) == 1
    assert lib.slk_cutmx_roundtrip(None, 2, 0, X, st) == 1 and lib.slk_cutmx_roundtrip(X, 2, 0, None, st) == 1
    assert lib.slk_cutmx_roundtrip(X + 6, 2, 0, X, st) == 1 and lib.slk_cutmx_roundtrip(X, 2, 0, X + 2, st) == 1
    for fn in (lib.slk_cutmx_encode, lib.slk_cutmx_roundtrip):
        assert fn(None, 0, 0, None, st) == 0   # n == 0: nothing launched, no pointer looked at
    assert lib.slk_cutmx_decode(None, 0, 1, None, None, st) == 0
    torch.cuda.synchronize()
    assert not x.any() and not rec4.any() and int(err.item()) == 0   # nothing was written
