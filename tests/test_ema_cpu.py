"""optim.EMA without a GPU: the float64 closed form and the derived bound of tests/ema_ref.py pinned against numpy
float32 evaluations of the rule (plain and with the product and sum fused), three deliberately wrong variants that must
each break that pin, the config's refusals, set_decay on a CPU tensor, the C entry's refusals, and the evaluation-graph
policy of graphs.GraphedTrainer for the averaged weights on a stub trainer (as tests/test_graph_policy_cpu.py)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ema_ref as R
from splitcnn import graphs, optim
from splitcnn.engine import LossLog

F32 = np.float32
WARM_N = tuple(range(1, 65))


def _inputs():
    """name -> (e, p) float32 blocks: random values, p within an ulp of e, magnitude ratios of 1e+-30."""
    rng = np.random.default_rng(7)
    e = rng.standard_normal(4099).astype(F32)
    p = (e + 0.01 * rng.standard_normal(4099)).astype(F32)
    near = np.concatenate([np.nextafter(e[:1000], F32(np.inf)), np.nextafter(e[1000:2000], F32(-np.inf)), e[2000:]])
    big, small = (rng.standard_normal(4099) * 1e15).astype(F32), (rng.standard_normal(4099) * 1e-15).astype(F32)
    return {"random": (e, p), "far": (e, rng.standard_normal(4099).astype(F32)), "near": (e, near.astype(F32)),
            "p>>e": (small, big), "e>>p": (big, small), "zero e": (np.zeros_like(e), p)}


INPUTS = _inputs()


@pytest.mark.parametrize("fused", (False, True))
@pytest.mark.parametrize("decay", R.DECAYS)
def test_bound_holds_for_float32_evaluations(decay, fused):
    """Every warm-up n from 1 to 64, the flat rule, and a counter past 2^24, on every input class."""
    for name, (e, p) in INPUTS.items():
        for warmup, ks in ((True, [n - 1 for n in WARM_N] + [2 ** 24 + 3]), (False, [0, 5, 2 ** 24 + 3])):
            for k in ks:
                got = R.step32(e, p, k, 0, decay, warmup, fused=fused)
                assert R.within(got, e, p, k, 0, decay, warmup), (name, decay, warmup, k, fused)


def test_bound_is_the_sketch_to_first_order():
    """bound() <= 4.5 u (|p| + |e|) up to second-order terms, and is not vacuous: >= u |e'| / 2 (one rounding)."""
    for name, (e, p) in INPUTS.items():
        for decay in R.DECAYS:
            b = R.bound(e, p, 3, 0, decay, True)
            first = 4.5 * R.U * (np.abs(p.astype(np.float64)) + np.abs(e.astype(np.float64)))
            assert (b <= first * (1 + 1e-6) + R.TINY).all(), (name, decay)
            assert (b >= 0.5 * R.U * np.abs(R.step64(e, p, 3, 0, decay, True))).all(), (name, decay)


def test_copy_before_start_is_bitwise():
    e, p = INPUTS["random"]
    p = p.copy()
    p[:3] = [np.nan, -0.0, np.inf]
    for k in (0, 4):
        got = R.step32(e, p, k, 5, 0.9, True)
        assert got.tobytes() == p.tobytes() and (R.bound(e, p, k, 5, 0.9, True) == 0).all()
    assert R.step32(e, p, 5, 5, 0.9, True).tobytes() != p.tobytes()


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v is not None])
def test_wrong_variants_break_the_pin(variant):
    """A closed form with n = t, with d and 1 - d swapped, or with `start` off by one is further from the float32
    rule than the bound on at least one of the pinned cases; the rule itself never is."""
    e, p = INPUTS["far"]
    broke = False
    for k in range(0, 8):
        for start in (0, 2):
            got = R.step32(e, p, k, start, 0.9999, True)
            assert R.within(got, e, p, k, start, 0.9999, True)
            wrong = R.step64(e, p, k, start, 0.9999, True, variant=variant)
            broke |= bool((np.abs(got.astype(np.float64) - wrong) > R.bound(e, p, k, start, 0.9999, True)).any())
    assert broke, variant


def test_warmup_rate_values():
    """d = (1 + n) / (10 + n) until it reaches decay: 2/11 at the first update, decay from n = 8991 on at 0.999."""
    assert R.rate64(0, 0, 0.999, True) == (False, 2.0 / 11.0)
    assert R.rate64(7, 5, 0.999, True) == (False, 4.0 / 13.0)
    assert R.rate64(4, 5, 0.999, True)[0] is True
    d999 = float(F32(0.999))
    assert R.rate64(8989, 0, 0.999, True)[1] < d999 and R.rate64(8991, 0, 0.999, True)[1] == d999
    assert R.rate64(3, 0, 0.999, False) == (False, d999)


# ------------------------------------------------------------------ the config
def test_config_defaults_and_refusals():
    e = optim.EMA(device="cpu")
    assert (e.decay, e.warmup, e.start) == (0.999, True, 0)
    assert e.value.dtype == torch.float32 and e.value.shape == (1,) and e.value.item() == float(F32(0.999))
    assert optim.EMA(0, device="cpu").decay == 0.0 and optim.EMA(np.float32(0.5), start=np.int64(3), device="cpu").start == 3
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), True, False, "0.9", None, 1.0 - 1e-9):
        with pytest.raises(ValueError, match="decay"):
            optim.EMA(bad, device="cpu")
    for bad in (-1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="start"):
            optim.EMA(start=bad, device="cpu")
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError, match="warmup"):
            optim.EMA(warmup=bad, device="cpu")
    assert not hasattr(e, "set_start") and not hasattr(e, "set_warmup")   # by-value constants of a captured graph
    assert optim.check_ema(None) is None and optim.check_ema(e) is e
    with pytest.raises(TypeError, match="ema"):
        optim.check_ema(0.999)
    with pytest.raises(TypeError, match="ema"):
        optim.check_ema(optim.ClipNorm(1.0, device="cpu"))


def test_set_decay_writes_the_same_tensor():
    e = optim.EMA(0.9, device="cpu")
    ptr = e.value.data_ptr()
    e.set_decay(0.99)
    assert e.value.data_ptr() == ptr and e.value.item() == float(F32(0.99)) and e.decay == 0.99
    for bad in (1.0, -1e-3, float("nan"), True):
        with pytest.raises(ValueError, match="decay"):
            e.set_decay(bad)
    assert e.value.item() == float(F32(0.99)) and e.decay == 0.99
    assert e.to("cpu") is e and e.value.data_ptr() == ptr


def test_stages_own_a_block_only_with_ema():
    """ema= selects the configured kernels on K2 (the average needs the counter); ema=None leaves the stage as it was."""
    from splitcnn.engine import ClientStage, ServerStage
    cfg = optim.EMA(0.9, device="cpu")
    c, s = ClientStage(device="cpu", ema=cfg), ServerStage(device="cpu", ema=cfg)
    for st in (c, s):
        assert st.ema_cfg is cfg and isinstance(st.optim, optim.SGD) and st.optim.lr == 0.01 and st.step_ctr is not None
        assert st.ema.dtype == torch.float32 and st.ema.shape == st.params.shape and torch.equal(st.ema, st.params)
        assert st.ema.data_ptr() != st.params.data_ptr()
    plain = ClientStage(device="cpu")
    assert plain.ema is None and plain.ema_cfg is None and plain.optim is None and plain.step_ctr is None
    with pytest.raises(TypeError, match="ema"):
        ClientStage(device="cpu", ema=0.999)


# ------------------------------------------------------------------ the C entry's refusals (no launch: no GPU needed)
def test_entry_refusals_without_gpu():
    from splitcnn import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    assert base % 4 == 0

    def call(e, p, n, nseg=None, decay=base, step=base, start=0):
        k = len(e)
        arr = lambda vals, t: ctypes.cast((t * max(k, 1))(*vals), P)  # noqa: E731
        return lib.slk_ema_multi(arr(e, P), arr(p, P), arr(n, ctypes.c_int), k if nseg is None else nseg, decay, step,
                                 start, 1, None)

    bad = 1   # hipErrorInvalidValue
    assert call([base], [base + 64], [-1]) == bad                       # negative n
    assert call([base], [base], [4]) == bad                             # e == p
    assert call([base], [base], [0]) == bad                             # ... also for an empty segment
    assert call([base], [base + 8], [4]) == bad                         # the blocks overlap
    assert call([None], [base], [4]) == bad and call([base], [None], [4]) == bad
    assert call([base], [base + 64], [4], decay=None) == bad and call([base], [base + 64], [4], step=None) == bad
    assert call([base], [base + 64], [4], nseg=0) == bad and call([base] * 9, [base + 64] * 9, [0] * 9) == bad
    assert call([base], [base + 64], [4], start=-1) == bad
    assert call([base + 2], [base + 64], [4]) == bad                    # not 4-byte aligned
    assert lib.slk_ema_multi(None, None, None, 1, base, base, 0, 1, None) == bad
    assert call([base, base], [base + 64, base], [0, 4]) == bad         # any segment
    assert call([base], [base + 64], [0]) == 0 and call([None], [None], [0]) == 0   # empty: legal, nothing launched


# ------------------------------------------------------------------ the evaluation-graph policy
class FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class Stub(graphs.GraphedTrainer):
    input_shape = (2, 3)

    def __init__(self, graph=True, ema=True):
        super().__init__("cpu", graph)
        block = torch.zeros(4) if ema else None
        self.client = SimpleNamespace(ema=block)
        self.server = SimpleNamespace(loss_log=LossLog("cpu", capacity=64), eval_logits=None, ema=block,
                                      eval_err_flag=torch.zeros(1, dtype=torch.int32))
        self.evals = []

    def _eval_eager(self, x, y, metrics=None, weights="live"):
        self._check_weights(weights)
        self.evals.append((x.data_ptr(), weights))
        self.server.eval_logits = torch.zeros(x.shape[0], 10)
        return torch.zeros(x.shape[0], dtype=torch.int64), torch.zeros(x.shape[0])


@pytest.fixture
def captures(monkeypatch):
    made = []

    def fake_capture(fn, device, preserve=()):
        g = FakeGraph()
        made.append(g)
        return g, fn()

    monkeypatch.setattr(graphs, "capture", fake_capture)
    return made


def _pair(B):
    return torch.zeros((B, 2, 3)), torch.zeros(B, dtype=torch.int64)


def test_live_and_averaged_passes_cache_under_different_keys(captures):
    tr = Stub()
    x, y = _pair(3)
    tr.eval_batch(x, y)
    live = tr._eval_graphs[3]
    tr.eval_batch(x, y, weights="ema")
    assert list(tr._eval_graphs) == [3, (3, "ema")] and tr._eval_graphs[3] is live and len(captures) == 2
    avg = tr._eval_graphs[3, "ema"]
    assert avg is not live and avg["x"] is not live["x"] and avg["graph"] is not live["graph"]
    assert [w for _, w in tr.evals] == ["live", "ema"]
    tr.eval_batch(x, y)
    tr.eval_batch(x, y, weights="ema")
    tr.eval_batch(x, y, weights="live")
    assert len(captures) == 2 and live["graph"].replays == 3 and avg["graph"].replays == 2
    assert tr._eval_graphs[3] is live and tr._graphs == {}
    tr.eval_batch(*_pair(5), weights="ema")     # another size: only the averaged pass is captured for it
    assert sorted(map(str, tr._eval_graphs)) == sorted(map(str, [3, (3, "ema"), (5, "ema")])) and 5 not in tr._eval_graphs


def test_evaluate_passes_weights_on(captures):
    tr = Stub()
    m = SimpleNamespace(acc=torch.zeros(104, dtype=torch.int64), result=lambda: "done")   # a caller's accumulator
    assert tr.evaluate([_pair(3), _pair(3)], metrics=m, weights="ema") == "done"
    assert list(tr._eval_graphs) == [(3, "ema")] and tr._eval_graphs[3, "ema"]["graph"].replays == 2
    assert tr._eval_graphs[3, "ema"]["metrics"] is m and [w for _, w in tr.evals] == ["ema"]
    assert tr.evaluate([_pair(3)], metrics=m) == "done" and list(tr._eval_graphs) == [(3, "ema"), 3]


def test_weights_refusals(captures):
    tr = Stub()
    x, y = _pair(3)
    for bad in ("EMA", "average", "", None, 1):
        with pytest.raises(ValueError, match="weights"):
            tr.eval_batch(x, y, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            tr.evaluate([(x, y)], weights=bad)
    plain = Stub(ema=False)
    with pytest.raises(RuntimeError, match="ema="):
        plain.eval_batch(x, y, weights="ema")
    with pytest.raises(RuntimeError, match="ema="):
        plain.evaluate([(x, y)], weights="ema")
    with pytest.raises(RuntimeError, match="ema="):
        plain.ema_state_dict()
    assert plain._eval_graphs == {} and captures == []
    eager = Stub(graph=False)
    eager.eval_batch(x, y, weights="ema")
    eager.eval_batch(x, y)
    assert eager._eval_graphs == {} and [w for _, w in eager.evals] == ["ema", "live"]
