"""slk_ema_multi alone, through ops.ema_multi: every segment length and pointer alignment at which the kernel changes path
(scalar head, 16-byte body, scalar tail, or scalars throughout), 1, 2 and 8 segments in one launch, sentinels around every
averaged block, results within the derived bound of tests/ema_ref.py of float64 computed from the device's own inputs, the
bitwise copy before `start`, the counter cases, launch equivalences, non-finite inputs and the entry's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import ema_ref as R
from splitcnn import optim

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)
ALIGN = {"both aligned": (0, 0), "e off by one": (1, 0), "p off by one": (0, 1), "both off, differently": (1, 3),
         "both off, alike": (3, 3)}
SENT = 12345.5
PAD = 8   # floats in front of and behind a segment: a sentinel on both sides whatever the offset


class Seg:
    """One (e, p) pair of n floats inside two padded buffers filled with sentinels, at float offsets (oe, op) from a
    16-byte boundary (torch allocations are 256-byte aligned and PAD is a multiple of 4)."""

    def __init__(self, n, oe, op, dev, rng, spread=0.05):
        self.n, self.oe, self.op = n, oe, op
        self.ebuf = torch.full((n + 2 * PAD,), SENT, device=dev)
        self.pbuf = torch.full((n + 2 * PAD,), SENT, device=dev)
        e0 = rng.standard_normal(n).astype(np.float32)
        p0 = (e0 + spread * rng.standard_normal(n)).astype(np.float32)
        self.e, self.p = self.ebuf[PAD + oe:PAD + oe + n], self.pbuf[PAD + op:PAD + op + n]
        self.e.copy_(torch.from_numpy(e0))
        self.p.copy_(torch.from_numpy(p0))
        self.e0, self.p0 = self.e.cpu().numpy().copy(), self.p.cpu().numpy().copy()   # the device's own inputs
        self.pbuf0 = self.pbuf.clone()
        if n:
            assert self.e.data_ptr() % 16 == 4 * (oe % 4) and self.p.data_ptr() % 16 == 4 * (op % 4)

    def pair(self):
        return (self.e, self.p)

    def check(self, k, start, decay, warmup):
        got = self.e.cpu().numpy()
        assert R.within(got, self.e0, self.p0, k, start, decay, warmup), (self.n, self.oe, self.op, k)
        eb = self.ebuf.cpu().numpy()
        lo, hi = PAD + self.oe, PAD + self.oe + self.n
        assert (eb[:lo] == SENT).all() and (eb[hi:] == SENT).all(), "a sentinel around e was overwritten"
        assert torch.equal(self.pbuf.view(torch.int32), self.pbuf0.view(torch.int32)), "p (or a sentinel) was written"
        if self.n and k >= start and decay < 0.99 and np.abs(self.p0 - self.e0).max() > 1e-3:
            assert not np.array_equal(got, self.e0), "e did not move"
        return got


def launch(segs, cfg, k, dev):
    from splitcnn import ops
    step = torch.tensor([k], dtype=torch.int32, device=dev)
    ops.ema_multi([s.pair() for s in segs], cfg.value, step, cfg.start, cfg.warmup)
    assert step.item() == k, "the kernel does not tick"


@pytest.mark.parametrize("align", list(ALIGN))
def test_lengths_alignments_segment_counts_and_sentinels(gpu, align):
    oe, op = ALIGN[align]
    rng = np.random.default_rng(11)
    cfg = optim.EMA(0.9, warmup=True, start=2, device=gpu)
    for n in LENGTHS:                                         # one segment per launch
        s = Seg(n, oe, op, gpu, rng)
        launch([s], cfg, 6, gpu)
        s.check(6, 2, 0.9, True)
    two = [Seg(1025, oe, op, gpu, rng), Seg(5, oe, op, gpu, rng)]
    launch(two, cfg, 6, gpu)
    eight = [Seg(n, oe, op, gpu, rng) for n in LENGTHS[1:]]   # 8 segments, every non-empty length, one launch
    launch(eight, cfg, 6, gpu)
    mixed = [Seg(n, a, b, gpu, rng) for n, (a, b) in zip((4099, 0, 1023, 7), ALIGN.values())]   # alignments mixed
    launch(mixed, cfg, 6, gpu)
    for s in two + eight + mixed:
        s.check(6, 2, 0.9, True)


@pytest.mark.parametrize("decay", R.DECAYS)
def test_accuracy_at_every_decay(gpu, decay):
    rng = np.random.default_rng(3)
    for warmup in (True, False):
        cfg = optim.EMA(decay, warmup=warmup, device=gpu)
        for k, spread in ((0, 1.0), (63, 1e-7), (100000, 1.0)):    # far apart; p within an ulp or two of e
            s = Seg(4099, 1, 1, gpu, rng, spread)
            launch([s], cfg, k, gpu)
            s.check(k, 0, decay, warmup)


def test_copy_before_start_is_bitwise(gpu):
    """t < 0: e = p bit for bit — quiet and signalling NaN payloads, -0.0, infinities, subnormals."""
    rng = np.random.default_rng(5)
    bits = np.array([0x7fc12345, 0xffc00001, 0x7fa00001, 0xff800001, 0x80000000, 0x00000000, 0x7f800000, 0xff800000,
                     0x00000001, 0x807fffff], dtype=np.uint32).view(np.int32)
    for oe, op in ALIGN.values():
        s = Seg(1030, oe, op, gpu, rng)
        s.p[3:3 + bits.size].view(torch.int32).copy_(torch.from_numpy(bits))
        s.pbuf0 = s.pbuf.clone()
        want = s.p.view(torch.int32).clone()
        for k, start in ((0, 1), (6, 7)):
            launch([s], optim.EMA(0.5, warmup=True, start=start, device=gpu), k, gpu)
            assert torch.equal(s.e.view(torch.int32), want), (oe, op, k)
        assert torch.equal(s.pbuf.view(torch.int32), s.pbuf0.view(torch.int32))
        assert (s.ebuf[:PAD + oe] == SENT).all() and (s.ebuf[PAD + oe + 1030:] == SENT).all()


@pytest.mark.parametrize("warmup", (True, False))
def test_counter_cases(gpu, warmup):
    rng = np.random.default_rng(9)
    start = 5
    for k in (0, start - 1, start, start + 1, start + 8, 2 ** 24 + 3):
        cfg = optim.EMA(0.9999, warmup=warmup, start=start, device=gpu)
        s = Seg(1025, 1, 0, gpu, rng, spread=1.0)
        launch([s], cfg, k, gpu)
        got = s.check(k, start, 0.9999, warmup)
        if k < start:
            assert got.tobytes() == s.p0.tobytes()
        else:   # the three wrong closed forms are told apart from the device's result wherever they differ in d
            b = R.bound(s.e0, s.p0, k, start, 0.9999, warmup)
            for variant in ("swapped", "start_off_by_one") + (("n_is_t",) if warmup and k - start < 1000 else ()):
                if variant == "start_off_by_one" and k != start:
                    continue
                wrong = R.step64(s.e0, s.p0, k, start, 0.9999, warmup, variant=variant)
                assert (np.abs(got.astype(np.float64) - wrong) > b).any(), (k, variant)


def test_launch_equivalences(gpu):
    from splitcnn import ops
    rng = np.random.default_rng(13)
    cfg = optim.EMA(0.99, warmup=False, device=gpu)
    specs = list(zip(LENGTHS[1:], list(ALIGN.values()) * 2))

    def fresh():
        r = np.random.default_rng(21)
        return [Seg(n, a, b, gpu, r, 1.0) for n, (a, b) in specs]

    one, each, again = fresh(), fresh(), fresh()
    launch(one, cfg, 4, gpu)
    for s in each:
        launch([s], cfg, 4, gpu)
    launch(again, cfg, 4, gpu)
    for a, b, c in zip(one, each, again):
        assert torch.equal(a.ebuf, b.ebuf), "one 8-segment launch is not eight 1-segment launches"
        assert torch.equal(a.ebuf, c.ebuf), "two runs differ"
    # set_decay between two launches changes the second one only
    s = Seg(4099, 0, 0, gpu, rng, 1.0)
    launch([s], cfg, 4, gpu)
    s.check(4, 0, 0.99, False)
    mid = s.e.cpu().numpy().copy()
    ptr = cfg.value.data_ptr()
    cfg.set_decay(0.5)
    assert cfg.value.data_ptr() == ptr
    launch([s], cfg, 5, gpu)
    assert R.within(s.e.cpu().numpy(), mid, s.p0, 5, 0, 0.5, False)
    assert not R.within(s.e.cpu().numpy(), mid, s.p0, 5, 0, 0.99, False)
    with pytest.raises(ValueError):
        ops.ema_multi([], cfg.value, torch.zeros(1, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        ops.ema_multi([s.pair()] * 9, cfg.value, torch.zeros(1, dtype=torch.int32, device=gpu))


def test_non_finite_parameters_propagate_elementwise(gpu):
    rng = np.random.default_rng(17)
    for oe, op in ((0, 0), (1, 3), (3, 3)):
        s = Seg(1025, oe, op, gpu, rng, 1.0)
        where = {0: np.nan, 1: np.inf, 6: -np.inf, 511: np.nan, 1020: np.inf, 1024: -np.inf}
        for i, v in where.items():
            s.p[i] = v
        s.p0, s.pbuf0 = s.p.cpu().numpy().copy(), s.pbuf.clone()
        launch([s], optim.EMA(0.9, warmup=True, device=gpu), 3, gpu)
        got = s.check(3, 0, 0.9, True)          # finite neighbours within the bound, the others NaN / the same infinity
        for i, v in where.items():
            assert (np.isnan(got[i]) if np.isnan(v) else got[i] == v), (i, v, got[i])
        assert np.isfinite(np.delete(got, list(where))).all()


def test_refusals_return_the_error_and_write_nothing(gpu):
    from splitcnn import _lib, ops
    rng = np.random.default_rng(19)
    s = Seg(1024, 0, 0, gpu, rng)
    cfg = optim.EMA(0.5, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    before = s.ebuf.clone()
    P, I = ctypes.c_void_p, ctypes.c_int
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def raw(e, p, n, nseg=None, decay=cfg.value.data_ptr(), stp=step.data_ptr(), start=0):
        k = len(e)
        arr = lambda vals, t: ctypes.cast((t * max(k, 1))(*vals), P)  # noqa: E731
        return _lib.load().slk_ema_multi(arr(e, P), arr(p, P), arr(n, I), k if nseg is None else nseg, decay, stp,
                                         start, 1, stream)

    e, p = s.e.data_ptr(), s.p.data_ptr()
    refused = [raw([e], [p], [-1]), raw([e], [e], [1024]), raw([e], [e + 16], [1024]), raw([None], [p], [1024]),
               raw([e], [None], [1024]), raw([e], [p], [1024], decay=None), raw([e], [p], [1024], stp=None),
               raw([e], [p], [1024], nseg=0), raw([e] * 9, [p] * 9, [1024] * 9), raw([e], [p], [1024], start=-1),
               raw([e + 2], [p], [1000]), raw([e, e], [p, e], [1024, 1024]),     # a bad segment behind a good one
               _lib.load().slk_ema_multi(None, None, None, 1, cfg.value.data_ptr(), step.data_ptr(), 0, 1, stream)]
    assert refused == [1] * len(refused)
    with pytest.raises(_lib.SLKError, match="invalid argument"):
        ops.ema_multi([(s.e, s.e)], cfg.value, step)
    with pytest.raises(ValueError):
        ops.ema_multi([(s.e, s.p[:-1])], cfg.value, step)
    with pytest.raises(TypeError):
        ops.ema_multi([(s.e, s.p.double())], cfg.value, step)
    torch.cuda.synchronize()
    assert torch.equal(s.ebuf, before) and torch.equal(s.pbuf, s.pbuf0)
    assert raw([e], [p], [0]) == 0 and raw([None], [None], [0]) == 0     # an empty segment is legal
    assert torch.equal(s.ebuf, before)
