"""GPU tests of graphs.capture on its own (tensors of a few elements) and of WideTrainer's graphs on a
caller's own input buffers (what bench.py's K5 run uses through register_inputs), bit for bit against a
trainer that always copies into the static inputs: the K5 twins of
test_gpu_parity.test_graphs_on_caller_buffers_bitwise_vs_static_inputs and
test_graph_inputs_static_buffers_and_register."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 5   # ragged: not a multiple of any tile (as test_wide_gpu.py)


def test_capture_warms_up_restores_and_replays(gpu):
    """fn() runs twice on the host — the warm-up, which executes, and the capture, whose launches are
    recorded and not executed. A tensor named in `preserve` is bitwise what it was; one that is not shows the
    warm-up's execution; every replay() advances it by one more; the captured call's return value is the
    tensor the replays write."""
    from splitcnn.graphs import capture
    ctr = torch.tensor([10, 20, 30], dtype=torch.int32, device=gpu)       # not preserved
    kept = torch.tensor([1.5, -2.0, 0.25, 1e-30], device=gpu)             # preserved
    out = torch.zeros(3, dtype=torch.int32, device=gpu)
    before = kept.clone()
    calls = []

    def fn():
        calls.append(torch.cuda.is_current_stream_capturing())
        ctr.add_(1)
        kept.mul_(3.0).add_(1.0)
        out.copy_(ctr)
        return out

    graph, ret = capture(fn, gpu, preserve=[kept])
    torch.cuda.synchronize()
    print("calls", calls, "ctr", ctr.tolist(), "kept", kept.tolist(), "out", out.tolist())
    assert calls == [False, True]                     # the warm-up and the capture both ran fn
    assert ret is out
    assert torch.equal(kept.view(torch.int32), before.view(torch.int32))
    assert ctr.tolist() == [11, 21, 31] and out.tolist() == [11, 21, 31]
    for i in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert ctr.tolist() == [11 + i, 21 + i, 31 + i] and ret.tolist() == ctr.tolist()
    want = before.clone()
    for _ in range(3):
        want.mul_(3.0).add_(1.0)
    assert torch.equal(kept.view(torch.int32), want.view(torch.int32))   # the replays do write `kept`


def wide_pair(gpu, seed, graph_inputs):
    """Two WideTrainers from one seed: `own` captures on up to graph_inputs caller pairs, `cpy` always copies."""
    from splitcnn.wide import WideTrainer, init_wide_models
    own = WideTrainer(*init_wide_models(seed=seed), device=gpu, graph=True)
    cpy = WideTrainer(*init_wide_models(seed=seed), device=gpu, graph=True)
    own.graph_inputs, cpy.graph_inputs = graph_inputs, 0
    return own, cpy


def wide_ring(gpu, seed):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(seed)
    xs, ys = zip(*(data.batch(B) for _ in range(3)))
    return torch.stack(xs).to(gpu), torch.stack(ys).to(gpu)


def n_caller(tr):
    return sum(1 for k in tr._graphs if isinstance(k, tuple))


def assert_same_training(own, cpy):
    torch.cuda.synchronize()
    for a, b in ((own.client, cpy.client), (own.server, cpy.server)):
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(a.step_ctr, b.step_ctr) and int(a.step_ctr.item()) == own.global_step == cpy.global_step
    assert [l for _, l in own.loss_log.flush()] == [l for _, l in cpy.loss_log.flush()]


def test_wide_graphs_on_caller_buffers_bitwise_vs_static_inputs(gpu):
    """WideTrainer replays graphs captured on the caller's own input buffers for up to `graph_inputs` pairs
    and falls back to the static inputs for others (the ring's third pair, then a fresh tensor every step):
    parameters, Adam's m / v, both step counters and the losses bit-identical to the always-copy trainer."""
    X, Y = wide_ring(gpu, 12)
    own, cpy = wide_pair(gpu, 5, 2)
    for i in range(9):
        x, y = X[i % 3], Y[i % 3]          # buffers 0, 1 captured; buffer 2 goes through the copy
        if i >= 6:
            x, y = x.clone(), y.clone()    # fresh tensors
        own.step(x, y)
        cpy.step(x, y)
    assert n_caller(own) == 2 and n_caller(cpy) == 0
    assert own.global_step == 9
    assert_same_training(own, cpy)


def test_wide_graph_inputs_static_buffers_and_register(gpu):
    """The static inputs handed back replay their own graph; register_inputs() captures on a declared pair at
    once; an undeclared pair is captured the second time it is seen. All bit-identical to always copying."""
    X, Y = wide_ring(gpu, 13)
    own, cpy = wide_pair(gpu, 6, 4)
    sx, sy = own.static_inputs(B)
    assert own.register_inputs(X[0], Y[0]) and not cpy.register_inputs(X[0], Y[0])
    assert n_caller(own) == 1
    sx.copy_(X[2])
    sy.copy_(Y[2])
    own.step(sx, sy)
    cpy.step(X[2], Y[2])
    assert n_caller(own) == 1                    # no graph captured on the static buffers
    own.step(X[1], Y[1])
    cpy.step(X[1], Y[1])
    assert n_caller(own) == 1                    # first sight of X[1]: static-input copy
    for i in range(4):
        own.step(X[i % 2], Y[i % 2])
        cpy.step(X[i % 2], Y[i % 2])
    assert n_caller(own) == 2 and n_caller(cpy) == 0   # X[1] captured on its second sight
    assert_same_training(own, cpy)
