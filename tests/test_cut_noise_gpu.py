"""slk_cut_noise / slk_cut_scale_rows alone (privacy.CutNoise) against tests/cut_noise_ref.py, bit for bit on the
outputs and on the (norm, coef) pairs (NaNs by NaN-ness): groups of n = 1, 3 and 5 rows of the reference's set under
four (seed, step, row0) keys, one with a counter above 2^31, for both laws and a hand-made table with a nonzero tail,
with and without a clip, with and without noise, and clip = inf. Outputs go into NaN-filled buffers with a sentinel
row behind the last."""
import numpy as np
import pytest
import torch

import cut_noise_ref as R

pytestmark = pytest.mark.gpu

CUT = (32, 8, 8, 8)
CLIPS = (None, R.CLIP, float("inf"))


def _tables(law):
    from splitcnn import privacy
    if law == "hand":
        return R.hand_table()
    t64, tail = privacy.noise_tables(law)
    return t64.astype(np.float32), float(np.float32(tail))


def _noise(law, clip, seed=0, scale=None):
    from splitcnn.privacy import CutNoise
    scale = R.SCALES[law] if scale is None else scale
    if law == "hand":
        table, tail = R.hand_table()
        return CutNoise(scale=scale, clip=clip, seed=seed, table=table, tail=tail)
    return CutNoise(law, scale=scale, clip=clip, seed=seed)


@pytest.fixture(scope="module")
def ref():
    """The reference's outputs and stats on its whole set, row i being global row row0 + i: per (law, key, clip) with
    noise, per clip without. Computed once, never written."""
    bits = R.sample_bits()
    out = {"names": [n for n, _ in R.samples()], "bits": bits}
    for law in R.LAWS:
        table, tail = _tables(law)
        for key in R.KEYS:
            seed, t, row0 = key
            for clip in CLIPS:
                out[law, key, clip] = R.apply(bits, table, tail, np.float32(R.SCALES[law]), clip, seed, t, row0)
    for clip in CLIPS:
        out[clip] = R.apply(bits, clip=clip)
    return out


def _to_dev(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).view((-1,) + CUT).to(dev)


def _bits(t, n):
    return t[:n].contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(n, -1)


def _counter(step, dev):
    return torch.from_numpy(np.array([step], dtype=np.uint32).view(np.int32)).to(dev)


def _groups(N, n):
    return [min(i, N - n) for i in range(0, N, n)]


def _row_buffer(n, dev):
    buf = torch.full((n + 1,) + CUT, float("nan"), dtype=torch.bfloat16, device=dev)
    buf[n] = _to_dev(np.full((1, R.SAMPLE), 0xA5A5, dtype=np.uint16), dev)[0]
    return buf


def _stats_buffer(n, dev):
    buf = torch.full((n + 1, 2), float("nan"), dtype=torch.float32, device=dev)
    buf[n] = -77.0
    return buf


def _sentinels_ok(rows, stats, n):
    return bool((_bits(rows[n:], 1) == 0xA5A5).all()) and (stats is None or bool((stats[n] == -77.0).all()))


@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_clip_and_noise_match_reference(gpu, ref, law, n):
    N = len(ref["names"])
    for key in R.KEYS:
        seed, step, row0 = key
        ctr = _counter(step, gpu)
        for clip in CLIPS:
            q = _noise(law, clip, seed)
            want, wstats = ref[law, key, clip]
            for i in _groups(N, n):
                x = _to_dev(ref["bits"][i:i + n], gpu)
                out = _row_buffer(n, gpu)
                stats = _stats_buffer(n, gpu) if clip is not None else None
                q.apply(x, out[:n], ctr, row0=row0 + i, stats=None if stats is None else stats[:n])
                assert R.same_bits(_bits(out, n), want[i:i + n]), (law, key, clip, i)
                assert _sentinels_ok(out, stats, n)
                if clip is not None:
                    assert R.same_f32(stats[:n].cpu().numpy(), wstats[i:i + n]), (law, key, clip, i)
                # in place, and without a stats buffer
                inp = _row_buffer(n, gpu)
                inp[:n] = x
                q.apply(inp[:n], inp[:n], ctr, row0=row0 + i)
                assert R.same_bits(_bits(inp, n), want[i:i + n]) and _sentinels_ok(inp, None, n)
        assert int(ctr.item()) == int(np.array([step], dtype=np.uint32).view(np.int32)[0])   # never written


@pytest.mark.parametrize("n", [1, 3, 5])
def test_clip_without_noise_and_the_norm_against_float64(gpu, ref, n):
    """noise=False: the clip alone (what evaluation runs), no counter needed; without a clip the copy of the bits.
    The float32 norm also lies within the derived bound of the exact float64 norm (cut_noise_ref.norm_bound)."""
    N = len(ref["names"])
    ok = R.norm_bound_applies(ref["bits"])
    n64 = np.sqrt((R.to_f32(ref["bits"]).astype(np.float64) ** 2).sum(axis=1))
    for clip in CLIPS:
        q = _noise("laplace", clip)
        want, wstats = ref[clip]
        for i in _groups(N, n):
            x = _to_dev(ref["bits"][i:i + n], gpu)
            out = _row_buffer(n, gpu)
            stats = _stats_buffer(n, gpu) if clip is not None else None
            q.apply(x, out[:n], noise=False, stats=None if stats is None else stats[:n])
            assert R.same_bits(_bits(out, n), want[i:i + n]) and _sentinels_ok(out, stats, n), (clip, i)
            if clip is not None:
                got = stats[:n].cpu().numpy()
                assert R.same_f32(got, wstats[i:i + n])
                sel = ok[i:i + n]
                err = np.abs(got[sel, 0].astype(np.float64) - n64[i:i + n][sel])
                print(f"clip {clip} rows {i}..{i + n - 1}: max |norm - norm64| / bound = "
                      f"{(err / np.maximum(R.norm_bound(n64[i:i + n][sel]), 1e-300)).max() if sel.any() else 0:.3f}")
                assert (err <= R.norm_bound(n64[i:i + n][sel])).all()
    # clip = inf: coef = 1 on every finite row, the rows' own bits out
    _, wstats = ref[float("inf")]
    finite = np.isfinite(wstats[:, 0])
    assert (wstats[finite, 1] == 1).all() and R.same_bits(ref[float("inf")][0][finite], ref["bits"][finite])


def test_scale_zero_without_a_clip_is_the_identity(gpu, ref):
    """x + (+-0) = x on rows without -0 (a -0 plus +0 is +0)."""
    names = ref["names"]
    rows = [names.index(n) for n in ("all_zero", "relu_0", "relu_1", "relu_2", "bf16_max")]
    x = _to_dev(ref["bits"][rows], gpu)
    out = _row_buffer(len(rows), gpu)
    _noise("laplace", None, seed=9, scale=0.0).apply(x, out[:len(rows)], _counter(3, gpu), row0=11)
    assert np.array_equal(_bits(out, len(rows)), ref["bits"][rows])
    table, tail = _tables("laplace")
    want, _ = R.apply(ref["bits"], table, tail, np.float32(0.0), None, 9, 3, 11)
    full = _row_buffer(len(names), gpu)
    _noise("laplace", None, seed=9, scale=0.0).apply(_to_dev(ref["bits"], gpu), full[:len(names)], _counter(3, gpu), row0=11)
    assert R.same_bits(_bits(full, len(names)), want)


def test_a_slice_with_its_row0_is_the_rows_of_the_whole(gpu, ref):
    seed, step, _ = R.KEYS[1]
    q, ctr = _noise("gaussian", R.CLIP, seed), _counter(step, gpu)
    x = _to_dev(ref["bits"][:5], gpu)
    whole, part, wrong = _row_buffer(5, gpu), _row_buffer(3, gpu), _row_buffer(3, gpu)
    sw, sp = _stats_buffer(5, gpu), _stats_buffer(3, gpu)
    q.apply(x, whole[:5], ctr, row0=0, stats=sw[:5])
    q.apply(x[2:5], part[:3], ctr, row0=2, stats=sp[:3])
    q.apply(x[2:5], wrong[:3], ctr, row0=0)
    assert np.array_equal(_bits(part, 3), _bits(whole[2:], 3)) and torch.equal(sp[:3], sw[2:5])
    assert not np.array_equal(_bits(wrong, 3), _bits(whole[2:], 3))
    assert R.same_bits(_bits(whole, 5), ref["gaussian", R.KEYS[1], R.CLIP][0][:5])


def test_graph_replay_follows_the_counter_and_the_setters(gpu, ref):
    """A captured launch replayed around ops.tick gives counter t, then t + 1; set_scale and set_clip reach the
    replay (device scalars), with the arguments of the capture."""
    from splitcnn import ops
    from splitcnn.graphs import capture
    n, seed = 3, 5
    table, tail = _tables("laplace")
    q = _noise("laplace", R.CLIP, seed)
    x = _to_dev(ref["bits"][3:3 + n], gpu)
    out, stats = torch.zeros_like(x), torch.zeros(n, 2, device=gpu)
    ctr = _counter(1, gpu)
    launch = lambda: q.apply(x, out, ctr, row0=4, stats=stats)   # noqa: E731
    launch()
    graph, _ = capture(launch, gpu)
    want = {}
    for t in (1, 2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert int(ctr.item()) == t
        want[t], ws = R.apply(ref["bits"][3:3 + n], table, tail, np.float32(R.SCALES["laplace"]), R.CLIP, seed, t, 4)
        assert R.same_bits(_bits(out, n), want[t]), t
        assert R.same_f32(stats.cpu().numpy(), ws)
        ops.tick(ctr)
    assert not np.array_equal(want[1], want[2])
    q.set_scale(0.11)
    q.set_clip(2.5)
    graph.replay()
    torch.cuda.synchronize()
    w, ws = R.apply(ref["bits"][3:3 + n], table, tail, np.float32(0.11), np.float32(2.5), seed, 3, 4)
    assert R.same_bits(_bits(out, n), w) and R.same_f32(stats.cpu().numpy(), ws)
    assert (q.scale, q.clip) == (0.11, 2.5)
    with pytest.raises(RuntimeError, match="clip=None"):
        _noise("laplace", None).set_clip(1.0)


def test_scale_rows_matches_reference(gpu, ref):
    """slk_cut_scale_rows on the forward's own stats: bit for bit, coef = 1 rows bitwise unchanged, in place too."""
    names, N = ref["names"], len(ref["names"])
    q = _noise("laplace", R.CLIP)
    x = _to_dev(ref["bits"], gpu)
    stats = torch.empty(N, 2, device=gpu)
    q.apply(x, torch.empty_like(x), noise=False, stats=stats)
    wstats = ref[R.CLIP][1]
    assert R.same_f32(stats.cpu().numpy(), wstats)
    # a gradient: the signed row, rolled differently for every sample
    g = np.stack([np.roll(ref["bits"][names.index("signed_neg_zero")], 17 * i) for i in range(N)])
    want = R.scale_rows(g, wstats)
    for n in (1, 3, 5):
        for i in _groups(N, n):
            out = _row_buffer(n, gpu)
            q.scale_rows(_to_dev(g[i:i + n], gpu), stats[i:i + n], out[:n])
            assert R.same_bits(_bits(out, n), want[i:i + n]) and _sentinels_ok(out, None, n), (n, i)
            inp = _row_buffer(n, gpu)
            inp[:n] = _to_dev(g[i:i + n], gpu)
            q.scale_rows(inp[:n], stats[i:i + n], inp[:n])
            assert R.same_bits(_bits(inp, n), want[i:i + n]) and _sentinels_ok(inp, None, n)
    one = wstats[:, 1] == 1
    assert one.sum() >= 3 and np.array_equal(want[one], g[one])
    # over_clip's coef is 1 - 1e-3, less than half a bf16 ulp from 1: only a row well past the bound moves
    assert wstats[names.index("relu_0"), 1] < 0.5
    assert not np.array_equal(want[names.index("relu_0")], g[names.index("relu_0")])


def test_refusals(gpu):
    from splitcnn import _lib
    from splitcnn.privacy import CutNoise
    for kw in ({"kind": "cauchy"}, {"kind": 3}, {"scale": -1.0}, {"scale": float("nan")}, {"scale": float("inf")},
               {"scale": True}, {"clip": 0.0}, {"clip": -2.0}, {"clip": float("nan")}, {"seed": -1}, {"seed": 2 ** 32},
               {"seed": 1.5}, {"table": np.zeros(1024)}, {"table": np.zeros(1000, dtype=np.float32)},
               {"table": [0.0] * 1024}, {"tail": 0.5}, {"table": np.zeros(1024, dtype=np.float32), "tail": float("nan")}):
        with pytest.raises(ValueError):
            CutNoise(**{"scale": 0.1, **kw})
    q = CutNoise("laplace", scale=0.1, clip=1.0)
    for bad in (-0.1, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="scale"):
            q.set_scale(bad)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip"):
            q.set_clip(bad)
    q.set_clip(float("inf"))
    x = torch.zeros((2,) + CUT, dtype=torch.bfloat16, device=gpu)
    ctr = torch.zeros(1, dtype=torch.int32, device=gpu)
    stats = torch.zeros(2, 2, device=gpu)
    with pytest.raises(ValueError, match="needs step"):
        q.apply(x, x)
    with pytest.raises(TypeError, match="int32"):
        q.apply(x, x, ctr.long())
    with pytest.raises(ValueError, match="shape"):
        q.apply(x, x, torch.zeros(2, dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.apply(x, x, ctr.cpu())
    for bad in (-1, 2 ** 31, 1.0, True):
        with pytest.raises(ValueError, match="row0"):
            q.apply(x, x, ctr, row0=bad)
    with pytest.raises(TypeError, match="bfloat16"):
        q.apply(x.float(), x, ctr)
    with pytest.raises(TypeError, match="bfloat16"):
        q.apply(x, x.float(), ctr)
    with pytest.raises(ValueError, match="contiguous"):
        q.apply(torch.zeros(2, 2, R.SAMPLE, dtype=torch.bfloat16, device=gpu)[:, 0], x, ctr)
    with pytest.raises(ValueError, match="per sample"):
        q.apply(torch.zeros(2, 100, dtype=torch.bfloat16, device=gpu), x, ctr)
    with pytest.raises(ValueError, match="samples"):
        q.apply(x, x[:1], ctr)
    flat = torch.zeros(2 * R.SAMPLE + 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="16-byte aligned"):
        q.apply(flat[1:2 * R.SAMPLE + 1].view(2, R.SAMPLE), x, ctr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.apply(x.cpu(), x, ctr)
    with pytest.raises(ValueError, match="shape"):
        q.apply(x, x, ctr, stats=stats[:1])
    with pytest.raises(TypeError, match="float32"):
        q.apply(x, x, ctr, stats=stats.double())
    with pytest.raises(ValueError, match="without a clip"):
        CutNoise(scale=0.1).apply(x, x, ctr, stats=stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.scale_rows(x.cpu(), stats, x)
    with pytest.raises(ValueError, match="shape"):
        q.scale_rows(x, stats[:1], x)
    with pytest.raises(ValueError, match="samples"):
        q.scale_rows(x, stats, x[:1])
    with pytest.raises(TypeError, match="bfloat16"):
        q.scale_rows(x.float(), stats, x)
    # the entries themselves, on device pointers
    lib = _lib.load()
    s = torch.cuda.current_stream(gpu).cuda_stream
    xp, tp, sp, cp, kp, stp = (x.data_ptr(), q.table.data_ptr(), q.scale_value.data_ptr(), q.clip_value.data_ptr(),
                               ctr.data_ptr(), stats.data_ptr())
    fn = lib.slk_cut_noise
    assert fn(xp, -1, tp, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 1
    assert fn(xp, 2, tp, 0.0, sp, cp, 0, kp, -1, xp, stp, s) == 1
    assert fn(None, 2, tp, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 1
    assert fn(xp, 2, tp, 0.0, sp, cp, 0, kp, 0, None, stp, s) == 1
    assert fn(xp + 2, 1, tp, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 1
    assert fn(xp, 1, tp, 0.0, sp, cp, 0, kp, 0, xp + 2, stp, s) == 1
    assert fn(xp, 2, None, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 1          # noise without a table
    assert fn(xp, 2, tp + 4, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 1        # a table off its 16 bytes
    assert fn(xp, 2, tp, 0.0, sp, cp, 0, None, 0, xp, stp, s) == 1          # noise without a counter
    assert fn(xp, 2, tp, 0.0, sp, cp, 0, kp + 2, 0, xp, stp, s) == 1
    assert fn(xp, 2, tp, 0.0, sp + 2, cp, 0, kp, 0, xp, stp, s) == 1
    assert fn(xp, 2, tp, 0.0, sp, cp + 2, 0, kp, 0, xp, stp, s) == 1
    assert fn(xp, 2, tp, 0.0, sp, cp, 0, kp, 0, xp, stp + 4, s) == 1        # stats off their 8 bytes
    assert fn(xp, 0, tp, 0.0, sp, cp, 0, kp, 0, xp, stp, s) == 0            # empty: nothing launched
    assert fn(xp, 2, None, 0.0, None, None, 0, None, 0, xp, None, s) == 0   # no noise, no clip: the copy
    fn = lib.slk_cut_scale_rows
    assert fn(xp, -1, stp, xp, s) == 1 and fn(None, 2, stp, xp, s) == 1 and fn(xp, 2, None, xp, s) == 1
    assert fn(xp, 2, stp, None, s) == 1 and fn(xp + 2, 1, stp, xp, s) == 1 and fn(xp, 2, stp + 4, xp, s) == 1
    assert fn(xp, 0, stp, xp, s) == 0
    q.apply(x[:0], x[:0], ctr)
    torch.cuda.synchronize()
    assert not x.any()
