"""The slk_cuttopk_* kernels alone (codec.TopKCut's methods) against tests/cuttopk_ref.py, bit for bit: groups of
n = 1, 3 and 5 samples x k = 8, 1000, 2048, 8192 over one fixed-seed set whose rows are the cases where a select can
go wrong; outputs pre-filled with NaN / 0xFF and a sentinel row behind the last; malformed records; a captured graph;
a second run; the refusals."""
import numpy as np
import pytest
import torch

import cuttopk_ref as R

pytestmark = pytest.mark.gpu

KS = [8, 1000, 2048, 8192]
ONE, BIG, LOW, TOP = 0x3F80, 0x4000, 0x3000, 0x7F7F


def _rows(k):
    """uint16 [20, 16384]; rows 14.. are poisoned."""
    g = np.random.default_rng(5)
    bits = lambda a: R.to_bits(torch.from_numpy(a).to(torch.bfloat16))   # noqa: E731
    sign = lambda: (g.integers(0, 2, R.SAMPLE) << 15).astype(np.uint16)  # noqa: E731
    gauss = bits(g.standard_normal(R.SAMPLE).astype(np.float32))
    rows = [bits(np.maximum(g.standard_normal(R.SAMPLE), 0).astype(np.float32)),   # post-ReLU: about half exact zeros
            gauss,
            (g.permutation(R.SAMPLE) + 300).astype(np.uint16) | sign(),             # 16,384 distinct magnitudes
            np.full(R.SAMPLE, ONE, np.uint16)]                                      # all equal: indices 0..k-1 win
    a = np.full(R.SAMPLE, ONE, np.uint16)   # a plateau with k - 3 larger values after it: the tie picks are 0, 1, 2
    a[R.SAMPLE - (k - 3):] = BIG
    rows.append(a)
    a = np.full(R.SAMPLE, LOW, np.uint16)   # ties in the last wave's quarter only; r = 5 ends inside a 16-byte piece
    a[100:100 + k - 5], a[12290:12310] = BIG, ONE
    rows.append(a)
    a = np.full(R.SAMPLE, LOW, np.uint16)   # ties across the wave boundary at 4096; r = 7: 5 before it, 2 behind
    a[8192:8192 + k - 7], a[4091:4107] = BIG, ONE
    rows.append(a)
    a = np.full(R.SAMPLE, LOW, np.uint16)   # +x / -x at the threshold: the first 4 by index whatever their sign
    ties = [3, 700, 4095, 4096, 8191, 12288, 16000, 16383]
    a[np.setdiff1d(np.arange(R.SAMPLE), ties)[-(k - 4):]] = BIG | 0x8000
    a[ties] = [ONE | 0x8000, ONE, ONE, ONE | 0x8000] * 2
    rows.append(a)
    a = np.zeros(R.SAMPLE, np.uint16)       # fewer than k nonzeros, -0 among the kept zeros (and one that is not)
    a[g.choice(R.SAMPLE, k // 2, replace=False)] = gauss[:k // 2] | 0x0100
    a[[1, 16380]] = 0x8000
    rows += [a, np.zeros(R.SAMPLE, np.uint16),
             g.integers(0, 128, R.SAMPLE).astype(np.uint16) | sign()]               # threshold in the denormal range
    a = gauss.copy()                        # threshold at the largest finite bf16, k + 10 of them
    a[g.choice(R.SAMPLE, k + 10, replace=False)] = TOP
    rows += [a, (ONE | g.integers(0, 128, R.SAMPLE)).astype(np.uint16),             # one exponent bin: pass 2 decides
             ((g.integers(1, 200, R.SAMPLE) << 7) | 0x55).astype(np.uint16) | sign()]   # one mantissa: pass 1 decides
    for bad in (0x7FC1, 0x7F80, 0xFF80):    # NaN, +inf, -inf at element 0 and at element 16,383
        for at in (0, R.SAMPLE - 1):
            a = gauss.copy()
            a[at] = bad
            rows.append(a)
    return np.stack(rows)


@pytest.fixture(scope="module")
def ref():
    """Per k: the rows, the reference's records and its decoded rows — computed once, never written."""
    out = {}
    for k in KS:
        x = _rows(k)
        rec = R.encode(x, k)
        dec, flag = R.decode(rec, k)
        assert flag == 0 and np.array_equal(dec, R.roundtrip(x, k)) and (dec[14:] == R.NAN).all()
        assert ((dec[:14] != 0).sum(1) <= k).all() and np.array_equal(R.roundtrip(dec[:14], k), dec[:14])
        assert np.flatnonzero(dec[4] == ONE).tolist() == [0, 1, 2] and (dec[8][1], dec[8][16380]) == (0x8000, 0)
        out[k] = (x, rec, dec)
    return out


def _codec(k):
    from splitcnn.codec import TopKCut
    return TopKCut(fwd=k, bwd=None)


def _dev_rows(bits, gpu, n):
    """bf16 [n + 1, 32, 8, 8, 8] on the device: `bits` (or NaN) in rows 0..n-1, the sentinel 0x5A5A in row n."""
    buf = np.full((n + 1, R.SAMPLE), 0x5A5A, np.uint16)
    buf[:n] = R.NAN if bits is None else bits
    return R.from_bits(buf).view(n + 1, 32, 8, 8, 8).to(gpu)


def _bits(t):
    return R.to_bits(t).reshape(t.shape[0], -1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_encode_decode_roundtrip_match_reference(gpu, ref, n, k):
    q, (x, want_rec, want_dec) = _codec(k), ref[k]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for i in [min(i, len(x) - n) for i in range(0, len(x), n)]:
        xs, want = _dev_rows(x[i:i + n], gpu, n), want_dec[i:i + n]
        rec = torch.full((n + 1, R.record_bytes(k)), 0xFF, dtype=torch.uint8, device=gpu)
        q.encode(xs[:n], rec[:n], "fwd")
        got = rec.cpu().numpy()
        assert np.array_equal(got[:n], want_rec[i:i + n]), (i, np.argwhere(got[:n] != want_rec[i:i + n])[:4])
        assert (got[n] == 0xFF).all()
        out = _dev_rows(None, gpu, n)
        q.decode(torch.from_numpy(want_rec[i:i + n].copy()).to(gpu), out[:n], err, "fwd")
        assert np.array_equal(_bits(out)[:n], want), (i, np.argwhere(_bits(out)[:n] != want)[:4])
        rt = _dev_rows(None, gpu, n)
        q.roundtrip(xs[:n], rt[:n], "fwd")
        assert np.array_equal(_bits(rt)[:n], want), (i, np.argwhere(_bits(rt)[:n] != want)[:4])
        q.roundtrip(xs[:n], xs[:n], "fwd")   # in place
        assert np.array_equal(_bits(xs)[:n], want), i
        assert all((_bits(t)[n] == 0x5A5A).all() for t in (out, rt, xs))
    assert int(err.item()) == 0   # poisoned records are well formed


@pytest.mark.parametrize("kind", ["other_k", "mx_format", "poison_word_2", "reserved", "bit_extra", "bit_missing"])
def test_malformed_records_poison_their_sample_only(gpu, ref, kind):
    k = 1000
    _, want_rec, want_dec = ref[k]
    recs = want_rec[:3].copy()
    word, bm = recs[1, :R.HEAD].view(np.uint32), recs[1, R.HEAD:R.VALUES]
    if kind == "bit_extra":
        bm[np.flatnonzero(bm == 0)[0]] = 1
    elif kind == "bit_missing":
        at = np.flatnonzero(bm)[-1]
        bm[at] &= bm[at] - 1   # its lowest set bit
    else:
        i, v = {"other_k": (0, k + 8), "mx_format": (1, 0x10), "poison_word_2": (2, 2), "reserved": (3, 1)}[kind]
        word[i] = v
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _dev_rows(None, gpu, 3)
    _codec(k).decode(torch.from_numpy(recs).to(gpu), out[:3], err, "fwd")
    got = _bits(out)
    want, flag = R.decode(recs, k)
    assert flag == 1 and int(err.item()) == 1 and (got[1] == R.NAN).all() and (got[3] == 0x5A5A).all()
    assert np.array_equal(got[:3], want) and np.array_equal(got[[0, 2]], want_dec[[0, 2]])


def test_a_captured_graph_follows_its_inputs_and_a_second_run_gives_the_same_bytes(gpu, ref):
    from splitcnn.graphs import capture
    k, n = 2048, 3
    q, (x, want_rec, want_dec) = _codec(k), ref[k]
    xs, rt = _dev_rows(None, gpu, n)[:n], _dev_rows(None, gpu, n)[:n]
    rec, rec2 = q.records("a", n, gpu, direction="fwd"), q.records("b", n, gpu, direction="fwd")

    def work():
        q.encode(xs, rec, "fwd")
        q.roundtrip(xs, rt, "fwd")
        q.encode(xs, rec2, "fwd")
    g, _ = capture(work, gpu)
    for i in (0, 5, 13):   # new contents, same buffers
        xs.copy_(_dev_rows(x[i:i + n], gpu, n)[:n])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rec.cpu().numpy(), want_rec[i:i + n]) and torch.equal(rec, rec2)
        assert np.array_equal(_bits(rt), want_dec[i:i + n])


def test_refusals(gpu):
    from splitcnn import _lib
    from splitcnn.codec import TopKCut
    assert [_lib.query("slk_cuttopk_record_bytes", k) for k in (1024, 2048, 0, 4, 12, 8200)] == [4112, 6160] + [-1] * 4
    for k in (0, 4, 12, 8200):
        with pytest.raises(ValueError, match="multiple of 8"):
            TopKCut(fwd=k)
    with pytest.raises(ValueError, match="both None"):
        TopKCut(fwd=None, bwd=None)
    q = TopKCut(fwd=1024, bwd=8)
    x = torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    rec = q.records("r", 2, gpu, direction="fwd")
    off = torch.zeros(2 * R.SAMPLE + 8, dtype=torch.bfloat16, device=gpu)[4:4 + 2 * R.SAMPLE].view(2, R.SAMPLE)
    for match, call in (("direction= is required", lambda: q.records("r", 2, gpu)),
                        ("expected shape", lambda: q.encode(x, rec, "bwd")),   # the other direction's record width
                        ("samples like x", lambda: q.roundtrip(x, x[:1], "fwd")),
                        ("16-byte aligned", lambda: q.roundtrip(off, x, "fwd"))):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.roundtrip(x.cpu(), x.cpu(), "fwd")
    lib, st = _lib.load(), torch.cuda.current_stream(gpu).cuda_stream
    X, RC, E = x.data_ptr(), rec.data_ptr(), err.data_ptr()
    for k in (0, 4, 12, 8200):   # a k the rule refuses: nothing is launched
        assert lib.slk_cuttopk_encode(X, 2, k, RC, st) == lib.slk_cuttopk_roundtrip(X, 2, k, X, st) == 9
        assert lib.slk_cuttopk_decode(RC, 2, k, X, E, st) == 9
    assert lib.slk_cuttopk_encode(X + 2, 2, 8, RC, st) == lib.slk_cuttopk_decode(RC, 2, 8, X, E + 2, st) == 1
    torch.cuda.synchronize()
    assert not x.any() and int(err.item()) == 0   # nothing was written
