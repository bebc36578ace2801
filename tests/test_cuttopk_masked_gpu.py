"""The masked backward of codec.TopKCut(k, "masked") alone (slk_cuttopk_roundtrip_map / _mask / _gather / _scatter)
against a few lines of numpy, bit for bit: groups of n = 1 and 3 samples x k = 8, 1000, 8192 over maps and gradient
rows where a popcount rank can go wrong, poisoned maps between valid ones, malformed records, a captured graph, the
refusals. The forward selection and its tie rows are tests/cuttopk_ref.py's and test_cuttopk_gpu.py's."""
import numpy as np
import pytest
import torch

import cuttopk_ref as R
from test_cuttopk_gpu import _bits, _rows

pytestmark = pytest.mark.gpu

KS = [8, 1000, 8192]
FMT, FILL = 0x21, 0xFFFF   # the masked record's format word; what outputs hold before a launch (a NaN that is not 0x7FC0)


def _cases(k):
    """(maps uint8 [m, 2048], gradients uint16 [m, 16384]): valid maps with a poisoned one after each of the first
    three, so that every group of three holds both."""
    x, idx = _rows(k), np.arange(R.SAMPLE)
    valid = [R.keep(x[i], k) for i in (4, 6, 5)]   # ties at 0..2, across the wave boundary at 4096, in the last wave
    valid += [idx < k, idx >= R.SAMPLE - k]
    if k == 8192:
        valid.append(idx % 2 == 1)
    if k <= 512:                                   # all of them inside round 3 of wave 2
        valid.append(np.isin(idx, 2 * 4096 + 3 * 512 + 61 * np.arange(k)))
    poison = [idx < k - 8, idx < k + 8, idx < 0]
    kept = [valid[0], poison[0], valid[1], poison[1], valid[2], poison[2]] + valid[3:]
    g = np.random.default_rng(11)
    sign = lambda: (g.integers(0, 2, R.SAMPLE) << 15).astype(np.uint16)   # noqa: E731
    grads = []
    for i, kp in enumerate(kept):
        a = [R.to_bits(torch.from_numpy(g.standard_normal(R.SAMPLE).astype(np.float32)).to(torch.bfloat16)),
             g.integers(0, 128, R.SAMPLE).astype(np.uint16) | sign(),        # zeros and denormals
             np.full(R.SAMPLE, 0x7F7F, np.uint16) | sign()][i % 3].copy()    # the largest finite value
        on, off = np.flatnonzero(kp), np.flatnonzero(~kp)
        if len(on):   # a NaN, a -0 and both infinities at kept positions: they pass; at dropped ones: they vanish
            a[on[[0, 1, -2, -1]]] = [0x7FC1, 0x8000, 0xFF80, 0x7F80]
        a[off[[0, 1, -2, -1]]] = [0x7FC1, 0x8000, 0xFF80, 0x7F80]
        grads.append(a)
    return np.stack([np.packbits(kp, bitorder="little") for kp in kept]), np.stack(grads)


def _reference(grads, maps, k):
    """(mask's rows, gather's records) by the rule of include/slk.h."""
    kept = np.unpackbits(maps, axis=1, bitorder="little").astype(bool)
    ok = kept.sum(1) == k
    dense = np.where(ok[:, None], np.where(kept, grads, 0), R.NAN).astype(np.uint16)
    rec = np.zeros((len(grads), 16 + 2 * k), np.uint8)
    for r, row, kp, o in zip(rec, grads, kept, ok):
        r[:16].view(np.uint32)[:] = (k, FMT, not o, 0)
        if o:
            r[16:].view(np.uint16)[:] = row[kp]
    return dense, rec


@pytest.fixture(scope="module")
def ref():
    """Per k: maps, gradients, mask's rows, gather's records; the forward rows, their roundtrip and their records —
    computed once, never written."""
    out = {}
    for k in KS:
        maps, grads = _cases(k)
        x = _rows(k)
        out[k] = (maps, grads, *_reference(grads, maps, k), x, R.roundtrip(x, k), R.encode(x, k)[:, R.HEAD:R.VALUES])
    return out


def _codec(k):
    from splitcnn.codec import TopKCut
    return TopKCut(fwd=k, bwd="masked")


def _dev(a, gpu):
    return (R.from_bits(a) if a.dtype == np.uint16 else torch.from_numpy(a.copy())).to(gpu)


def _out(n, gpu, width=None):
    """n + 1 prefilled rows: bf16 [n + 1, 16384], or uint8 [n + 1, width]; row n is the sentinel."""
    if width is None:
        return _dev(np.full((n + 1, R.SAMPLE), FILL, np.uint16), gpu)
    return torch.full((n + 1, width), 0xFF, dtype=torch.uint8, device=gpu)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [1, 3])
def test_all_five_entries_match_numpy(gpu, ref, n, k):
    q, (maps, grads, dense, recs, x, x_rt, x_map) = _codec(k), ref[k]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for gi, i in enumerate(min(i, len(maps) - n) for i in range(0, len(maps), n)):
        m, g, want = _dev(maps[i:i + n], gpu), _dev(grads[i:i + n], gpu), dense[i:i + n]
        out, rec, back = _out(n, gpu), _out(n, gpu, 16 + 2 * k), _out(n, gpu)
        q.roundtrip(g, out[:n], "bwd", map=m)
        assert np.array_equal(_bits(out)[:n], want), (i, np.argwhere(_bits(out)[:n] != want)[:4])
        q.encode(g, rec[:n], "bwd", map=m)
        got = rec.cpu().numpy()
        assert np.array_equal(got[:n], recs[i:i + n]), (i, np.argwhere(got[:n] != recs[i:i + n])[:4])
        q.decode(_dev(recs[i:i + n], gpu), back[:n], err, "bwd", map=m)
        assert np.array_equal(_bits(back)[:n], want), (i, np.argwhere(_bits(back)[:n] != want)[:4])
        q.roundtrip(g, g, "bwd", map=m)   # in place
        assert np.array_equal(_bits(g), want), i
        assert (_bits(out)[n] == FILL).all() and (_bits(back)[n] == FILL).all() and (got[n] == 0xFF).all()
        # the forward that writes the map: rows of the select's own cases, a poisoned one among them
        sel = (np.arange(n) * 7 + 13 * gi) % len(x)
        xs, out, fm, plain = _dev(x[sel], gpu), _out(n, gpu), _out(n, gpu, 2048), _out(n, gpu)
        q.roundtrip(xs, out[:n], "fwd", map=fm[:n])
        q.roundtrip(xs, plain[:n], "fwd")
        assert np.array_equal(_bits(out)[:n], x_rt[sel]) and torch.equal(out.view(torch.int16), plain.view(torch.int16))
        assert np.array_equal(fm.cpu().numpy()[:n], x_map[sel]) and (fm[n] == 0xFF).all()
    assert int(err.item()) == 0   # poisoned records are well formed


@pytest.mark.parametrize("kind", ["topk_format", "other_k", "word_2", "word_3", "map_popcount", "poisoned"])
def test_malformed_records_poison_their_sample_only(gpu, ref, kind):
    k = 1000
    maps, grads, dense, recs = ref[k][:4]
    rows = [0, 2, 4]   # three valid samples; the middle one is broken
    maps, want, rec = maps[rows].copy(), dense[rows].copy(), recs[rows].copy()
    if kind == "map_popcount":
        maps[1] = ref[k][0][1]   # k - 8 bits under an unpoisoned record
    else:
        i, v = {"topk_format": (1, 0x20), "other_k": (0, k + 8), "word_2": (2, 2), "word_3": (3, 1),
                "poisoned": (2, 1)}[kind]
        rec[1, :16].view(np.uint32)[i] = v
    want[1] = R.NAN
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = _out(3, gpu)
    _codec(k).decode(_dev(rec, gpu), out[:3], err, "bwd", map=_dev(maps, gpu))
    assert np.array_equal(_bits(out)[:3], want) and (_bits(out)[3] == FILL).all()
    assert int(err.item()) == (kind != "poisoned")   # a poisoned record leaves the flag alone


def test_a_captured_graph_follows_its_inputs(gpu, ref):
    from splitcnn.graphs import capture
    k, n = 1000, 3
    q, (maps, grads, dense, recs, x, x_rt, x_map) = _codec(k), ref[k]
    xs, g, m = _out(n, gpu)[:n], _out(n, gpu)[:n], _out(n, gpu, 2048)[:n]
    cut, masked, back = _out(n, gpu)[:n], _out(n, gpu)[:n], _out(n, gpu)[:n]
    rec, err = q.records("a", n, gpu, direction="bwd"), torch.zeros(1, dtype=torch.int32, device=gpu)

    def work():
        q.roundtrip(xs, cut, "fwd", map=m)
        q.roundtrip(g, masked, "bwd", map=m)
        q.encode(g, rec, "bwd", map=m)
        q.decode(rec, back, err, "bwd", map=m)
    graph, _ = capture(work, gpu)
    for i in (0, 4, 11):   # new contents, same buffers; the maps are the forward's own
        gr = grads[np.arange(i, i + n) % len(grads)]
        xs.copy_(_dev(x[i:i + n], gpu))
        g.copy_(_dev(gr, gpu))
        graph.replay()
        torch.cuda.synchronize()
        want, want_rec = _reference(gr, x_map[i:i + n], k)
        assert np.array_equal(_bits(cut), x_rt[i:i + n]) and np.array_equal(m.cpu().numpy(), x_map[i:i + n])
        assert np.array_equal(_bits(masked), want) and np.array_equal(_bits(back), want)
        assert np.array_equal(rec.cpu().numpy(), want_rec) and int(err.item()) == 0


def test_surface_and_refusals(gpu):
    from splitcnn import _lib
    from splitcnn.codec import TopKCut
    assert [_lib.query("slk_cuttopk_masked_record_bytes", k) for k in (1024, 2048, 0, 12, 8200)] == [2064, 4112, -1, -1, -1]
    with pytest.raises(ValueError, match="no selection to mask by"):
        TopKCut(fwd=None, bwd="masked")
    with pytest.raises(ValueError, match="multiple of 8"):
        TopKCut(fwd=1024, bwd="mask")
    q = TopKCut(1024, "masked")
    assert (q.format("bwd"), q.record_bytes("bwd"), q.record_bytes("fwd")) == ("masked", 16 + 2 * 1024, 2064 + 2 * 1024)
    assert repr(q) == "TopKCut(fwd=1024, bwd='masked')" and q.rounding_of("bwd") == "nearest" and q.nearest() is q
    assert tuple(q.records("r", 2, gpu, direction="bwd").shape) == (2, 2064)
    x = torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16, device=gpu)
    m = torch.zeros(2, 2048, dtype=torch.uint8, device=gpu)
    off = torch.zeros(2 * 2048 + 16, dtype=torch.uint8, device=gpu)[8:8 + 2 * 2048].view(2, 2048)
    rec, err = q.records("r", 2, gpu, direction="bwd"), torch.zeros(1, dtype=torch.int32, device=gpu)
    for match, call in (("map=", lambda: q.roundtrip(x, x, "bwd")),
                        ("map=", lambda: q.encode(x, rec, "bwd")),
                        ("map=", lambda: q.decode(rec, x, err, "bwd")),
                        ("expected shape", lambda: q.roundtrip(x, x, "bwd", map=m[:1])),
                        ("expected shape", lambda: q.roundtrip(x, x, "fwd", map=m.view(4, 1024))),
                        ("16-byte aligned", lambda: q.roundtrip(x, x, "bwd", map=off))):
        with pytest.raises(ValueError, match=match):
            call()
    lib, st = _lib.load(), torch.cuda.current_stream(gpu).cuda_stream
    X, M, RC, E = x.data_ptr(), m.data_ptr(), rec.data_ptr(), err.data_ptr()
    for k in (0, 12, 8200):   # a k the rule refuses: nothing is launched
        assert lib.slk_cuttopk_roundtrip_map(X, 2, k, X, M, st) == lib.slk_cuttopk_mask(X, M, 2, k, X, st) == 9
        assert lib.slk_cuttopk_gather(X, M, 2, k, RC, st) == lib.slk_cuttopk_scatter(RC, M, 2, k, X, E, st) == 9
    assert lib.slk_cuttopk_mask(X, M + 8, 2, 8, X, st) == lib.slk_cuttopk_scatter(RC, M, 2, 8, X, E + 2, st) == 1
    torch.cuda.synchronize()
    assert not x.any() and not m.any() and int(err.item()) == 0   # nothing was written
