"""slk_cut8_encode_sr / slk_cut8_roundtrip_sr alone (codec.Fp8Cut(rounding="stochastic")) against tests/cut8_sr_ref.py,
byte for byte: groups of n = 1, 3 and 5 samples of cut8_ref's set (every sample, both formats) under three
(seed, step, row0) keys, one with a counter above 2^31; outputs pre-filled with NaN / 0xFF and a sentinel row behind the
last record or row."""
import numpy as np
import pytest
import torch

import cut8_ref as R
import cut8_sr_ref as S

pytestmark = pytest.mark.gpu

DIRECTION = {"e4m3": "fwd", "e5m2": "bwd"}
KEYS = [(0, 0, 0), (5, 1, 0), (0xDEADBEEF, 0x80000003, 7)]   # (seed, step, row0)
SENTINEL = 0xA5
CUT = (32, 8, 8, 8)


@pytest.fixture(scope="module")
def ref():
    """cut8_ref's set with the reference's stochastic records and decoded rows per (format, key); row i of the set is
    global row row0 + i. Computed once, never written."""
    x = R.sample_tensor()
    out = {"names": [n for n, _ in R.samples()], "x": x}
    for fmt in R.FORMATS:
        for key in KEYS:
            rec = S.encode(x, fmt, *key)
            dec, flag = R.decode(rec, fmt)
            assert flag == 0
            out[fmt, key] = (rec, R.to_bits(dec))
    return out


def _codec(seed, rounding="stochastic"):
    from splitcnn.codec import Fp8Cut
    return Fp8Cut(rounding=rounding, seed=seed)


def _counter(step, dev):
    return torch.from_numpy(np.array([step], dtype=np.uint32).view(np.int32)).to(dev)


def _groups(N, n):
    return [min(i, N - n) for i in range(0, N, n)]


def _rec_buffer(n, dev):
    buf = torch.full((n + 1, R.RECORD), 0xFF, dtype=torch.uint8, device=dev)
    buf[n] = SENTINEL
    return buf


def _row_buffer(n, dev):
    buf = torch.full((n + 1,) + CUT, float("nan"), dtype=torch.bfloat16, device=dev)
    buf[n] = R.from_bits(np.full(R.SAMPLE, 0xA5A5, dtype=np.uint16)).view(CUT).to(dev)
    return buf


def _bits(t, n):
    return R.to_bits(t[:n]).reshape(n, -1)


def _rows_ok(buf, n):
    return bool((R.to_bits(buf[n]) == 0xA5A5).all())


@pytest.mark.parametrize("fmt", list(R.FORMATS))
@pytest.mark.parametrize("n", [1, 3, 5])
def test_encode_sr_and_roundtrip_sr_match_reference(gpu, ref, fmt, n):
    d = DIRECTION[fmt]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for key in KEYS:
        seed, step, row0 = key
        q, ctr = _codec(seed), _counter(step, gpu)
        want_rec, want_dec = ref[fmt, key]
        for i in _groups(len(ref["names"]), n):
            x = ref["x"][i:i + n].view((n,) + CUT).to(gpu)
            rec = _rec_buffer(n, gpu)
            q.encode(x, rec[:n], d, step=ctr, row0=row0 + i)
            got = rec.cpu().numpy()
            assert np.array_equal(got[:n], want_rec[i:i + n]), (fmt, key, i)
            assert (got[n] == SENTINEL).all()
            # an ordinary record: the existing decode reads it
            out = _row_buffer(n, gpu)
            q.decode(rec[:n], out[:n], err, d)
            assert np.array_equal(_bits(out, n), want_dec[i:i + n]) and _rows_ok(out, n)
            # roundtrip_sr = decode(encode_sr), out of place and in place
            rt = _row_buffer(n, gpu)
            q.roundtrip(x, rt[:n], d, step=ctr, row0=row0 + i)
            assert np.array_equal(_bits(rt, n), want_dec[i:i + n]), (fmt, key, i)
            assert _rows_ok(rt, n)
            inp = _row_buffer(n, gpu)
            inp[:n] = x
            q.roundtrip(inp[:n], inp[:n], d, step=ctr, row0=row0 + i)
            assert np.array_equal(_bits(inp, n), want_dec[i:i + n]) and _rows_ok(inp, n)
        assert int(ctr.view(torch.int32).item()) == int(np.array([step], dtype=np.uint32).view(np.int32)[0])   # never written
    assert int(err.item()) == 0


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_a_slice_with_its_row0_is_the_rows_of_the_whole(gpu, ref, fmt):
    d, (seed, step, _) = DIRECTION[fmt], KEYS[1]
    q, ctr = _codec(seed), _counter(step, gpu)
    x = ref["x"][:5].view((5,) + CUT).to(gpu)
    whole, part, wrong = _rec_buffer(5, gpu), _rec_buffer(3, gpu), _rec_buffer(3, gpu)
    q.encode(x, whole[:5], d, step=ctr, row0=0)
    q.encode(x[2:5], part[:3], d, step=ctr, row0=2)
    q.encode(x[2:5], wrong[:3], d, step=ctr, row0=0)
    assert torch.equal(part[:3], whole[2:5]) and not torch.equal(wrong[:3], whole[2:5])
    assert np.array_equal(whole[:5].cpu().numpy(), ref[fmt, KEYS[1]][0][:5])
    rt_whole, rt_part = _row_buffer(5, gpu), _row_buffer(3, gpu)
    q.roundtrip(x, rt_whole[:5], d, step=ctr, row0=0)
    q.roundtrip(x[2:5], rt_part[:3], d, step=ctr, row0=2)
    assert torch.equal(rt_part[:3].view(torch.int16), rt_whole[2:5].view(torch.int16))


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_the_counter_is_read_on_the_device(gpu, ref, fmt):
    """The same launch arguments with the counter tensor overwritten give the new value's bits; a captured graph
    replayed around an ops.tick gives counter t, then t + 1."""
    from splitcnn import ops
    from splitcnn.graphs import capture
    d, n = DIRECTION[fmt], 3
    q = _codec(5)
    x = ref["x"][:n].view((n,) + CUT).to(gpu)
    want = {t: S.encode(ref["x"][:n], fmt, 5, t, 0) for t in (1, 2, 40)}
    ctr = _counter(1, gpu)
    rec, out = q.records(("sr", fmt), n, gpu), torch.zeros_like(x)
    launch = lambda: (q.encode(x, rec, d, step=ctr), q.roundtrip(x, out, d, step=ctr))  # noqa: E731
    launch()
    assert np.array_equal(rec.cpu().numpy(), want[1])
    ctr.fill_(40)
    launch()
    assert np.array_equal(rec.cpu().numpy(), want[40])
    assert np.array_equal(_bits(out, n), R.to_bits(R.decode(want[40], fmt)[0]))
    ctr.fill_(1)
    graph, _ = capture(launch, gpu)
    for t in (1, 2):
        rec.fill_(0xFF)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert int(ctr.item()) == t
        assert np.array_equal(rec.cpu().numpy(), want[t]), t
        assert np.array_equal(_bits(out, n), R.to_bits(R.decode(want[t], fmt)[0])), t
        ops.tick(ctr)
    assert not np.array_equal(want[1], want[2])


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_poisoned_zero_and_top_of_range_samples(gpu, ref, fmt):
    d, names, key = DIRECTION[fmt], ref["names"], KEYS[2]
    seed, step, row0 = key
    want_rec, want_dec = ref[fmt, key]
    rows = [names.index(n) for n in ("amax_ex127_man60", "has_nan", "all_zero", "has_inf", "amax_ex254_man7f")]
    q, ctr = _codec(seed), _counter(step, gpu)
    # the key of a row is its global row: launch each on its own row0 next to a neighbour
    for i in rows:
        x = ref["x"][i:i + 1].view((1,) + CUT).to(gpu)
        rec, rt = _rec_buffer(1, gpu), _row_buffer(1, gpu)
        q.encode(x, rec[:1], d, step=ctr, row0=row0 + i)
        q.roundtrip(x, rt[:1], d, step=ctr, row0=row0 + i)
        assert np.array_equal(rec[:1].cpu().numpy(), want_rec[i:i + 1]) and np.array_equal(_bits(rt, 1), want_dec[i:i + 1])
    for n in ("has_nan", "has_inf"):
        i = names.index(n)
        assert R.record_e(want_rec)[i] == R.POISON and not want_rec[i, R.HEADER:].any() and (want_dec[i] == 0x7FC0).all()
    z = names.index("all_zero")
    assert not want_rec[z, R.HEADER:].any() and R.record_e(want_rec)[z] == 0 and not want_dec[z].any()
    assert (want_dec[names.index("amax_ex254_man7f")] & 0x7fff).max() == 0x7f7f      # saturated, never inf
    # the sign of a zero result: +-1/4 of the smallest subnormal goes to +-0 or +-the smallest subnormal
    e = {"e4m3": -8, "e5m2": -15}[fmt]
    _, _, _, m, emin = R.FORMATS[fmt]
    t = torch.zeros(1, R.SAMPLE, dtype=torch.bfloat16)
    t[0, 0] = 1.0
    t[0, 1:2001] = -(2.0 ** (e + emin - m - 2))
    t[0, 2001:4001] = 2.0 ** (e + emin - m - 2)
    rec = _rec_buffer(1, gpu)
    q.encode(t.view((1,) + CUT).to(gpu), rec[:1], d, step=ctr, row0=3)
    got = rec[:1].cpu().numpy()
    assert np.array_equal(got, S.encode(t, fmt, seed, step, 3))
    assert set(got[0, R.HEADER + 1:R.HEADER + 2001].tolist()) == {0x80, 0x81}
    assert set(got[0, R.HEADER + 2001:R.HEADER + 4001].tolist()) == {0x00, 0x01}


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_unbiased_on_the_device(gpu, ref, fmt):
    """tests/test_cut8_sr_cpu.py's case on the device: one row over 1024 rows at row0 = 0, the per-element mean of the
    decoded values within 0.11 quanta of x (Hoeffding: cut8_sr_ref.UNBIASED_*)."""
    d = DIRECTION[fmt]
    seed, step = S.UNBIASED_KEY
    row = ref["x"][ref["names"].index(S.UNBIASED_SAMPLE)]
    x = row[None].expand(S.UNBIASED_ROWS, R.SAMPLE).contiguous().to(gpu)
    out = torch.empty_like(x)
    _codec(seed).roundtrip(x, out, d, step=_counter(step, gpu), row0=0)
    mean = out.double().mean(dim=0).cpu().numpy()
    dev = np.abs(mean - row.double().numpy()) / S.quanta(row[None], fmt)[0]
    print(f"{fmt}: max |mean - x| = {dev.max():.4f} quanta over {S.UNBIASED_ROWS} rows")
    assert dev.max() <= S.UNBIASED_T
    # nearest rounding on the same rows does not pass
    _codec(seed, "nearest").roundtrip(x, out, d)
    near = np.abs(out.double().mean(dim=0).cpu().numpy() - row.double().numpy()) / S.quanta(row[None], fmt)[0]
    assert near.max() > S.UNBIASED_T
    # the device's bits are the reference's on the first rows
    want = S.roundtrip(x[:4].cpu(), fmt, seed, step, 0)
    _codec(seed).roundtrip(x[:4], out[:4], d, step=_counter(step, gpu), row0=0)
    assert np.array_equal(R.to_bits(out[:4]), R.to_bits(want))


def test_refusals(gpu):
    from splitcnn import _lib
    from splitcnn.codec import Fp8Cut
    q = _codec(0)
    x = torch.zeros((2,) + CUT, dtype=torch.bfloat16, device=gpu)
    rec = torch.zeros(2, R.RECORD, dtype=torch.uint8, device=gpu)
    ctr = torch.zeros(1, dtype=torch.int32, device=gpu)
    for call in (lambda **kw: q.encode(x, rec, "fwd", **kw), lambda **kw: q.roundtrip(x, x, "bwd", **kw)):
        with pytest.raises(ValueError, match="needs step"):
            call()
        with pytest.raises(TypeError, match="int32"):
            call(step=ctr.long())
        with pytest.raises(ValueError, match="shape"):
            call(step=torch.zeros(2, dtype=torch.int32, device=gpu))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(step=ctr.cpu())
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(step=3)
        for bad in (-1, 2 ** 31, 1.0, True):
            with pytest.raises(ValueError, match="row0"):
                call(step=ctr, row0=bad)
    # what the nearest entries refuse
    with pytest.raises(TypeError, match="bfloat16"):
        q.roundtrip(x.float(), x, "fwd", step=ctr)
    with pytest.raises(TypeError, match="uint8"):
        q.encode(x, rec.to(torch.int8), "fwd", step=ctr)
    with pytest.raises(ValueError, match="contiguous"):
        q.roundtrip(torch.zeros(2, 2, R.SAMPLE, dtype=torch.bfloat16, device=gpu)[:, 0], x, "fwd", step=ctr)
    with pytest.raises(ValueError, match="per sample"):
        q.roundtrip(torch.zeros(2, 100, dtype=torch.bfloat16, device=gpu), x, "fwd", step=ctr)
    with pytest.raises(ValueError, match="shape"):
        q.encode(x, rec[:1], "fwd", step=ctr)
    with pytest.raises(ValueError, match="samples"):
        q.roundtrip(x, x[:1], "fwd", step=ctr)
    flat = torch.zeros(2 * R.SAMPLE + 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="16-byte aligned"):
        q.roundtrip(flat[1:2 * R.SAMPLE + 1].view(2, R.SAMPLE), x, "fwd", step=ctr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.roundtrip(x.cpu(), x, "fwd", step=ctr)
    with pytest.raises(ValueError, match="dense"):
        Fp8Cut(bwd=None, rounding={"fwd": "stochastic"}).roundtrip(x, x, "bwd", step=ctr)
    # a nearest direction takes and ignores step; the mixed codec picks the entry by direction
    mixed = Fp8Cut(rounding={"bwd": "stochastic"})
    assert torch.equal(mixed.encode(x, rec.clone(), "fwd", step=ctr), Fp8Cut().encode(x, rec.clone(), "fwd"))
    with pytest.raises(ValueError, match="needs step"):
        mixed.roundtrip(x, x, "bwd")
    # the entries themselves, on device pointers: a misaligned or missing counter, a negative row0
    lib = _lib.load()
    s = torch.cuda.current_stream(gpu).cuda_stream
    two = torch.zeros(2, dtype=torch.int16, device=gpu)
    for fn in (lib.slk_cut8_encode_sr, lib.slk_cut8_roundtrip_sr):
        dst = rec if fn is lib.slk_cut8_encode_sr else x
        assert fn(x.data_ptr(), 2, 0, dst.data_ptr(), 0, None, 0, s) == 1
        assert fn(x.data_ptr(), 2, 0, dst.data_ptr(), 0, two.data_ptr() + 2, 0, s) == 1
        assert fn(x.data_ptr(), 2, 0, dst.data_ptr(), 0, ctr.data_ptr(), -1, s) == 1
        assert fn(x.data_ptr(), 2, 2, dst.data_ptr(), 0, ctr.data_ptr(), 0, s) == 1
        assert fn(x.data_ptr() + 2, 1, 0, dst.data_ptr(), 0, ctr.data_ptr(), 0, s) == 1
        assert fn(x.data_ptr(), 0, 0, dst.data_ptr(), 0, ctr.data_ptr(), 0, s) == 0   # empty: nothing launched
    q.roundtrip(x[:0], x[:0], "bwd", step=ctr)
    torch.cuda.synchronize()
