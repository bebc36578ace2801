"""The slk_cut8_* kernels alone (codec.Fp8Cut's methods) against tests/cut8_ref.py, bit for bit: groups of n = 1, 3
and 5 samples of the generator's set (every sample, both formats), outputs pre-filled with NaN / 0xFF and a sentinel
row behind the last record or row."""
import numpy as np
import pytest
import torch

import cut8_ref as R

pytestmark = pytest.mark.gpu

DIRECTION = {"e4m3": "fwd", "e5m2": "bwd"}   # Fp8Cut()'s convention
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ref():
    """The generator's set, and the reference's records and decoded rows per format — computed once, never written."""
    x = R.sample_tensor()
    out = {"names": [n for n, _ in R.samples()], "x": x}
    for fmt in R.FORMATS:
        rec = R.encode(x, fmt)
        out[fmt] = (rec, R.to_bits(R.decode(rec, fmt)[0]))
    return out


@pytest.fixture(scope="module")
def codec(gpu):
    from splitcnn.codec import Fp8Cut
    return Fp8Cut()


def _groups(N, n):
    """Consecutive groups of n samples covering all N (the last one overlaps its neighbour)."""
    return [min(i, N - n) for i in range(0, N, n)]


def _rec_buffer(n, dev):
    """uint8 [n + 1, 16400] filled with 0xFF; row n is the sentinel."""
    buf = torch.full((n + 1, R.RECORD), 0xFF, dtype=torch.uint8, device=dev)
    buf[n] = SENTINEL
    return buf


def _row_buffer(n, dev):
    """bf16 [n + 1, 32, 8, 8, 8] of NaN; row n is the sentinel (bits 0xA5A5)."""
    buf = torch.full((n + 1, 32, 8, 8, 8), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[n] = R.from_bits(np.full(R.SAMPLE, 0xA5A5, dtype=np.uint16)).view(32, 8, 8, 8).to(dev)
    return buf


def _rows_ok(buf, n):
    return bool((R.to_bits(buf[n]) == 0xA5A5).all())


@pytest.mark.parametrize("fmt", list(R.FORMATS))
@pytest.mark.parametrize("n", [1, 3, 5])
def test_encode_decode_roundtrip_match_reference(gpu, codec, ref, fmt, n):
    d = DIRECTION[fmt]
    want_rec, want_dec = ref[fmt]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for i in _groups(len(ref["names"]), n):
        x = ref["x"][i:i + n].view(n, 32, 8, 8, 8).to(gpu)
        # encode: records byte for byte, headers included
        rec = _rec_buffer(n, gpu)
        codec.encode(x, rec[:n], d)
        got = rec.cpu().numpy()
        assert np.array_equal(got[:n], want_rec[i:i + n]), (fmt, i)
        assert (got[n] == SENTINEL).all()
        # decode of the reference's records
        out = _row_buffer(n, gpu)
        codec.decode(torch.from_numpy(want_rec[i:i + n].copy()).to(gpu), out[:n], err, d)
        assert np.array_equal(R.to_bits(out[:n]).reshape(n, -1), want_dec[i:i + n]), (fmt, i)
        assert _rows_ok(out, n)
        # roundtrip = decode(encode), out of place and in place
        rt = _row_buffer(n, gpu)
        codec.roundtrip(x, rt[:n], d)
        assert np.array_equal(R.to_bits(rt[:n]).reshape(n, -1), want_dec[i:i + n]), (fmt, i)
        assert _rows_ok(rt, n)
        inp = _row_buffer(n, gpu)
        inp[:n] = x
        codec.roundtrip(inp[:n], inp[:n], d)
        assert np.array_equal(R.to_bits(inp[:n]).reshape(n, -1), want_dec[i:i + n]), (fmt, i)
        assert _rows_ok(inp, n)
    assert int(err.item()) == 0   # reference records are well formed, the poisoned ones included


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_poisoned_samples_leave_neighbours_untouched(gpu, codec, ref, fmt):
    d, names = DIRECTION[fmt], ref["names"]
    want_rec, want_dec = ref[fmt]
    rows = [names.index("amax_ex127_man60"), names.index("has_nan"), names.index("sweep_e4m3"), names.index("has_inf"),
            names.index("amax_ex140_man7f")]
    x = ref["x"][rows].view(5, 32, 8, 8, 8).to(gpu)
    rec = _rec_buffer(5, gpu)
    codec.encode(x, rec[:5], d)
    assert np.array_equal(rec[:5].cpu().numpy(), want_rec[rows])
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(5, gpu)
    codec.decode(rec[:5], out[:5], err, d)
    got = R.to_bits(out[:5]).reshape(5, -1)
    assert (got[1] == 0x7FC0).all() and (got[3] == 0x7FC0).all()
    assert np.array_equal(got, want_dec[rows]) and _rows_ok(out, 5)
    assert int(err.item()) == 0   # poisoned is not malformed
    rt = _row_buffer(5, gpu)
    codec.roundtrip(x, rt[:5], d)
    assert np.array_equal(R.to_bits(rt[:5]).reshape(5, -1), want_dec[rows])


@pytest.mark.parametrize("fmt", list(R.FORMATS))
@pytest.mark.parametrize("kind", R.MALFORMED)
def test_malformed_record_sets_flag_and_poisons_its_row_only(gpu, codec, ref, fmt, kind):
    d, names = DIRECTION[fmt], ref["names"]
    want_rec, want_dec = ref[fmt]
    rows = [names.index("amax_ex60_man61"), names.index("non_negative"), names.index("sweep_e5m2")]
    recs = want_rec[rows].copy()
    recs[1] = R.malform(recs[1], kind)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(3, gpu)
    codec.decode(torch.from_numpy(recs).to(gpu), out[:3], err, d)
    got = R.to_bits(out[:3]).reshape(3, -1)
    ref_out, ref_flag = R.decode(recs, fmt)
    assert ref_flag == 1 and int(err.item()) == 1
    assert (got[1] == 0x7FC0).all()
    assert np.array_equal(got[0], want_dec[rows[0]]) and np.array_equal(got[2], want_dec[rows[2]])
    assert np.array_equal(got, R.to_bits(ref_out)) and _rows_ok(out, 3)
    # the flag is sticky: a well-formed decode does not clear it
    codec.decode(torch.from_numpy(want_rec[rows].copy()).to(gpu), out[:3], err, d)
    assert int(err.item()) == 1


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_received_nan_and_inf_codes_propagate(gpu, codec, ref, fmt):
    """Codes an encoder never writes: every one of the 256 under one exponent, against the reference (a NaN code of
    either sign gives 0x7FC0; everything else by the reference's bits)."""
    d = DIRECTION[fmt]
    rec = ref[fmt][0][ref["names"].index("amax_ex127_man00")].copy()[None]
    rec[0, R.HEADER:] = np.arange(R.SAMPLE, dtype=np.uint32).astype(np.uint8)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _row_buffer(1, gpu)
    codec.decode(torch.from_numpy(rec).to(gpu), out[:1], err, d)
    want, flag = R.decode(rec, fmt)
    nan = torch.isnan(want[0].float()).numpy()
    got = R.to_bits(out[0]).reshape(-1)
    assert flag == 0 and int(err.item()) == 0
    assert np.array_equal(got[~nan], R.to_bits(want[0])[~nan]) and (got[nan] == 0x7FC0).all()
    assert nan.sum() == {"e4m3": 2, "e5m2": 6}[fmt] * (R.SAMPLE // 256)


def test_captured_graph_replays_to_the_eager_bits(gpu, codec, ref):
    from splitcnn.graphs import capture
    n, N = 3, len(ref["names"])
    for fmt in R.FORMATS:
        d = DIRECTION[fmt]
        x = ref["x"][:n].view(n, 32, 8, 8, 8).to(gpu)
        rec = codec.records(("graph", fmt), n, gpu)
        assert codec.records(("graph", fmt), n, gpu) is rec and codec.records(("graph", fmt), n + 1, gpu) is not rec
        out = torch.zeros_like(x)
        err = torch.zeros(1, dtype=torch.int32, device=gpu)

        def run():
            codec.encode(x, rec, d)
            codec.decode(rec, out, err, d)

        graph, _ = capture(run, gpu)
        x.copy_(ref["x"][N - n:].view(n, 32, 8, 8, 8))   # rewrite the input; the graph reads the same buffer
        rec.fill_(0xFF)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rec.cpu().numpy(), ref[fmt][0][N - n:])
        assert np.array_equal(R.to_bits(out).reshape(n, -1), ref[fmt][1][N - n:])
        assert int(err.item()) == 0


def test_refusals(gpu, codec):
    x = torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu)
    rec = torch.zeros(2, R.RECORD, dtype=torch.uint8, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(TypeError, match="bfloat16"):
        codec.roundtrip(x.float(), x, "fwd")
    with pytest.raises(TypeError, match="uint8"):
        codec.encode(x, rec.to(torch.int8), "fwd")
    with pytest.raises(TypeError, match="int32"):
        codec.decode(rec, x, err.long(), "fwd")
    with pytest.raises(ValueError, match="contiguous"):
        codec.roundtrip(torch.zeros(2, 2, R.SAMPLE, dtype=torch.bfloat16, device=gpu)[:, 0], x, "fwd")
    with pytest.raises(ValueError, match="contiguous"):
        codec.encode(x, torch.zeros(2, 2 * R.RECORD, dtype=torch.uint8, device=gpu)[:, :R.RECORD], "fwd")
    with pytest.raises(ValueError, match="per sample"):
        codec.roundtrip(torch.zeros(2, 100, dtype=torch.bfloat16, device=gpu), x, "fwd")
    with pytest.raises(ValueError, match="shape"):
        codec.encode(x, rec[:1], "fwd")
    with pytest.raises(ValueError, match="samples"):
        codec.roundtrip(x, x[:1], "fwd")
    flat = torch.zeros(2 * R.SAMPLE + 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="16-byte aligned"):
        codec.roundtrip(flat[1:2 * R.SAMPLE + 1].view(2, R.SAMPLE), x, "fwd")
    bytes_ = torch.zeros(2 * R.RECORD + 16, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="16-byte aligned"):
        codec.decode(bytes_[4:2 * R.RECORD + 4].view(2, R.RECORD), x, err, "fwd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.roundtrip(x.cpu(), x, "fwd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.decode(rec, x, err.cpu(), "fwd")
    # an empty batch launches nothing
    codec.roundtrip(x[:0], x[:0], "bwd")
    codec.encode(x[:0], rec[:0], "fwd")
