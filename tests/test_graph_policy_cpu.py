"""The host policy of graphs.GraphedTrainer, pinned without a GPU: a stub trainer on device "cpu" whose
launch sequences only record their calls, with graphs.capture replaced by one that runs fn() once and
hands back a graph object that counts its replays. Which buffers get a graph, when, and how many; the
evaluation graph cache; the step bookkeeping; the optimizer state's load."""
from types import SimpleNamespace

import pytest
import torch

from splitcnn import graphs
from splitcnn.engine import LossLog

SHAPE = (2, 3)


class FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class Stub(graphs.GraphedTrainer):
    input_shape = SHAPE

    def __init__(self, graph=True, graph_inputs=4):
        super().__init__("cpu", graph, graph_inputs)
        self.client = None
        self.server = SimpleNamespace(loss_log=LossLog("cpu", capacity=64), eval_logits=None,
                                      eval_err_flag=torch.zeros(1, dtype=torch.int32))
        self.opt = {"client.step": torch.zeros(1, dtype=torch.int32), "server.step": torch.zeros(1, dtype=torch.int32)}
        self.eager, self.evals, self.written = [], [], 0

    def _eager(self, x, y):
        self.eager.append((x.data_ptr(), y.data_ptr()))

    def _eval_eager(self, x, y, metrics=None):
        self.evals.append((x.data_ptr(), y.data_ptr(), metrics))
        self.server.eval_logits = torch.zeros(x.shape[0], 10)
        return torch.zeros(x.shape[0], dtype=torch.int64), torch.zeros(x.shape[0])

    def _optim_state(self):
        return self.opt

    def _state(self):
        return list(self.opt.values())

    def _state_written(self):
        self.written += 1


@pytest.fixture
def captures(monkeypatch):
    """graphs.capture replaced: every call is listed as (graph, preserve); fn() runs once."""
    made = []

    def fake_capture(fn, device, preserve=()):
        g = FakeGraph()
        made.append((g, list(preserve)))
        return g, fn()

    monkeypatch.setattr(graphs, "capture", fake_capture)
    return made


def pair(B, fill=0.0):
    return torch.full((B,) + SHAPE, fill), torch.zeros(B, dtype=torch.int64)


def same(a, b):
    return len(a) == len(b) and all(p is q for p, q in zip(a, b))


def caller_keys(tr, B=None):
    return [k for k in tr._graphs if isinstance(k, tuple) and (B is None or k[0] == B)]


def test_second_sighting_rule(captures):
    tr = Stub()
    x, y = pair(4, 1.0)
    tr.step(x, y)                                   # first sight: the static inputs' graph, x copied in
    assert list(tr._graphs) == [4] and len(captures) == 1
    static = tr._graphs[4]
    assert static["graph"].replays == 1 and torch.equal(static["x"], x)
    assert same(captures[0][1], tr._state())        # the warm-up must leave no trace in exactly these
    assert tr._seen == {(4, x.data_ptr(), y.data_ptr()): 1}
    tr.step(x, y)                                   # second sight: a graph of its own, replayed in place
    key = (4, x.data_ptr(), y.data_ptr())
    assert caller_keys(tr) == [key] and len(captures) == 2 and tr._seen == {}
    own = tr._graphs[key]
    assert own["x"] is x and own["y"] is y and own["graph"].replays == 1 and static["graph"].replays == 1
    tr.step(x, y)
    assert len(captures) == 2 and own["graph"].replays == 2 and static["graph"].replays == 1
    for _ in range(3):                              # one-off fresh tensors are never captured
        tr.step(*pair(4, 2.0))
    assert len(captures) == 2 and caller_keys(tr) == [key] and static["graph"].replays == 4


def test_graph_inputs_budget_per_batch_size(captures):
    tr = Stub(graph_inputs=2)
    ring = [pair(4, float(i)) for i in range(3)]
    for _ in range(3):
        for x, y in ring:
            tr.step(x, y)
    assert len(caller_keys(tr, 4)) == 2             # the third pair keeps going through the copy
    assert (4, ring[2][0].data_ptr(), ring[2][1].data_ptr()) not in tr._graphs
    other = [pair(6, float(i)) for i in range(3)]   # another batch size has a budget of its own
    for _ in range(2):
        for x, y in other:
            tr.step(x, y)
    assert len(caller_keys(tr, 6)) == 2 and len(caller_keys(tr, 4)) == 2
    assert len(captures) == 2 + 2 + 2               # per size: the static inputs' graph and two pairs


def test_graph_inputs_zero_always_copies(captures):
    tr = Stub(graph_inputs=0)
    x, y = pair(4, 3.0)
    for i in range(4):
        x.fill_(float(i))
        tr.step(x, y)
        assert torch.equal(tr._graphs[4]["x"], x)
    assert list(tr._graphs) == [4] and len(captures) == 1 and tr._graphs[4]["graph"].replays == 4
    assert tr.register_inputs(x, y) is False


def test_static_inputs_are_never_captured_twice(captures):
    tr = Stub()
    sx, sy = tr.static_inputs(4)
    assert tr.static_inputs(4)[0] is sx and len(captures) == 1
    for _ in range(3):
        tr.step(sx, sy)
    assert tr.register_inputs(sx, sy) is True
    assert list(tr._graphs) == [4] and len(captures) == 1 and tr._seen == {}
    assert tr._graphs[4]["graph"].replays == 3


def test_register_inputs(captures):
    x, y = pair(4)
    assert Stub(graph=False).register_inputs(x, y) is False
    tr = Stub(graph_inputs=1)
    wide = torch.zeros((4,) + SHAPE[:-1] + (2 * SHAPE[-1],))
    assert tr.register_inputs(wide[..., ::2], y) is False               # not contiguous
    assert tr.register_inputs(x.double(), y) is False                   # wrong dtypes
    assert tr.register_inputs(x, y.int()) is False
    assert tr.register_inputs(torch.zeros(4, 3, 2), y) is False         # wrong sample shape
    assert tr.register_inputs(x, torch.zeros(5, dtype=torch.int64)) is False
    assert captures == [] and tr._graphs == {}
    assert tr.register_inputs(x, y) is True                             # captured at once
    assert caller_keys(tr) == [(4, x.data_ptr(), y.data_ptr())] and len(captures) == 1
    assert tr.register_inputs(x, y) is True and len(captures) == 1      # already registered
    assert tr.register_inputs(*pair(4)) is False and len(captures) == 1  # the budget is spent
    tr.step(x, y)
    assert tr._graphs[4, x.data_ptr(), y.data_ptr()]["graph"].replays == 1 and len(captures) == 1


def test_eval_graph_cache(captures):
    tr = Stub()
    m1, m2 = SimpleNamespace(acc=torch.zeros(3)), SimpleNamespace(acc=torch.ones(3))
    x, y = pair(3, 5.0)
    out = tr.eval_batch(x, y, m1)
    g1 = tr._eval_graphs[3]
    assert list(tr._eval_graphs) == [3] and tr._graphs == {} and g1["metrics"] is m1
    assert same(captures[0][1], [tr.server.eval_err_flag, m1.acc])
    assert torch.equal(g1["x"], x) and g1["graph"].replays == 1 and g1["out"] is out
    assert tr.server.eval_logits is g1["logits"]
    tr.eval_batch(x, y, m1)
    assert len(captures) == 1 and g1["graph"].replays == 2
    tr.eval_batch(x, y, m2)                         # another accumulator: captured again, same static inputs
    g2 = tr._eval_graphs[3]
    assert len(captures) == 2 and g2["metrics"] is m2 and g2["x"] is g1["x"] and g2["y"] is g1["y"]
    assert same(captures[1][1], [tr.server.eval_err_flag, m2.acc])
    tr.eval_batch(x, y)                             # and again for none
    assert len(captures) == 3 and same(captures[2][1], [tr.server.eval_err_flag])
    tr.eval_batch(*pair(5), m2)                     # keyed by batch size
    assert sorted(tr._eval_graphs) == [3, 5] and tr._graphs == {} and len(captures) == 4
    assert tr.server.eval_logits is tr._eval_graphs[5]["logits"]
    tr.eval_batch(x, y)
    assert tr.server.eval_logits is tr._eval_graphs[3]["logits"] and len(captures) == 4
    assert tr.global_step == 0 and tr.loss_log._steps == []
    with pytest.raises(ValueError):
        tr.eval_batch(torch.zeros(3, 3, 2), y)
    eager = Stub(graph=False)
    eager.eval_batch(x, y, m1)
    assert eager._eval_graphs == {} and eager.evals == [(x.data_ptr(), y.data_ptr(), m1)] and captures[4:] == []


def test_every_path_counts_one_step(captures):
    eager = Stub(graph=False)
    x, y = pair(4)
    for _ in range(3):
        eager.step(x, y)
    assert eager.global_step == 3 and eager.loss_log._steps == [0, 1, 2] and len(eager.eager) == 3
    assert captures == []
    tr = Stub()
    sx, sy = tr.static_inputs(4)
    n = 0
    for a, b in [(x, y), (x, y), (x, y), (sx, sy), pair(4), (sx, y), pair(6)]:
        tr.step(a, b)     # copy, capture + replay, replay, static inputs, one-off, half static, another size
        n += 1
        assert tr.global_step == n and tr.loss_log._steps == list(range(n))
    assert sum(g["graph"].replays for g in tr._graphs.values()) == n


def test_load_optimizer_state(captures):
    tr = Stub()
    saved = tr.optimizer_state()
    assert sorted(saved) == ["client.step", "server.step"]
    saved["client.step"] += 7                       # a copy: the trainer's own tensor does not move
    assert int(tr.opt["client.step"]) == 0
    with pytest.raises(ValueError):
        tr.load_optimizer_state({"client.step": saved["client.step"]})
    with pytest.raises(ValueError):
        tr.load_optimizer_state({**saved, "extra": torch.zeros(1)})
    assert tr.written == 0 and int(tr.opt["client.step"]) == 0
    tr.load_optimizer_state(saved)
    assert tr.written == 1 and int(tr.opt["client.step"]) == 7 and int(tr.opt["server.step"]) == 0
