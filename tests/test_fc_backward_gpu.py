"""slk_fc_backward (csrc/slk_server.hip: fc_backward_kernel, the dpooled and the wgrad role of one launch) against the
two launches it replaces, slk_fc_dgrad_amax and slk_fc_wgrad, on the same inputs: dpooled, dp_amax and every slab
(db3 columns included) torch.equal, i.e. bit for bit. The two parents are themselves checked against float64 in
test_client_fc_exact_gpu.py, so this file needs no tolerance.

Batch sizes, from the code: the dpooled role takes 8 samples per block, the wgrad role slices of
per = ceil(B / min(64, ceil(B / 64))) samples, 8 unrolled + a tail.
  B = 1, 7     one partial sample group; one slab, tail only
  B = 8, 9     an exact group, a group + 1; one slab, the unrolled 8 (+ 1)
  B = 16, 17   two groups, two + 1
  B = 33       five groups, the last of one sample
  B = 64       one slab of 64 (8 full unrolled rounds); B = 65: two slabs (33 + 32); B = 130: three (44 + 44 + 42)
The launch has 9 wgrad blocks per slab, then the dpooled blocks: 9 + 1 (B = 1) to 27 + 17 (B = 130) blocks, so the index
at which the second role begins (9, 18 and 27) and both roles' index arithmetic are exercised.

Every output is pre-filled with NaN and allocated with one sample (or slab) of sentinel after its last row: an element
the launch skips fails torch.equal, a write past a ragged batch fails the sentinel check."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
BATCHES = [1, 7, 8, 9, 16, 17, 33, 64, 65, 130]
NSLAB = {1: 1, 7: 1, 8: 1, 9: 1, 16: 1, 17: 1, 33: 1, 64: 1, 65: 2, 130: 3}
FC_SLAB = 92170
_CASES = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(dev, B):
    """Inputs and the two parents' outputs for batch B: computed once, shared, never written again."""
    if B not in _CASES:
        from splitcnn import _lib
        g = torch.Generator().manual_seed(4200 + B)
        dl = torch.randn(B, 10, generator=g) / B
        dl[1::3] = 0.0                      # all-zero rows: samples 1, 4, 7, ...
        if B > 2:
            dl[B - 1] = 0.0                 # ... and the last row of the last group / slice
        pooled = torch.relu(torch.randn(B, 9216, generator=g))
        W3 = torch.randn(10, 9216, generator=g) * 0.01
        dl, pooled, W3 = dl.to(dev), pooled.to(dev), W3.to(dev)
        nslab = _lib.query("slk_fc_wgrad_nslab", B)
        assert nslab == NSLAB[B]
        dp = torch.full((B, 9216), NAN, device=dev)
        am = torch.full((B,), NAN, device=dev)
        slabs = torch.full((nslab, FC_SLAB), NAN, device=dev)
        _lib.call("slk_fc_dgrad_amax", dl.data_ptr(), W3.data_ptr(), dp.data_ptr(), am.data_ptr(), B, _stream())
        _lib.call("slk_fc_wgrad", dl.data_ptr(), pooled.data_ptr(), slabs.data_ptr(), B, _stream())
        torch.cuda.synchronize()
        for t in (dp, am, slabs):
            assert not torch.isnan(t).any()
        _CASES[B] = (dl, pooled, W3, dp, am, slabs)
    return _CASES[B]


def _outputs(dev, B):
    """NaN-filled outputs with one sentinel row each."""
    return (torch.full((B + 1, 9216), NAN, device=dev), torch.full((B + 1,), NAN, device=dev),
            torch.full((NSLAB[B] + 1, FC_SLAB), NAN, device=dev))


def _launch(dl, W3, pooled, outs, B):
    from splitcnn import _lib
    dp, am, slabs = outs
    _lib.call("slk_fc_backward", dl.data_ptr(), W3.data_ptr(), pooled.data_ptr(), dp.data_ptr(), am.data_ptr(),
              slabs.data_ptr(), B, _stream())


def _assert_same(outs, want, B, what):
    dp, am, slabs = outs
    wdp, wam, wslabs = want
    n = NSLAB[B]
    assert torch.equal(dp[:B], wdp), f"{what}: dpooled"
    assert torch.equal(am[:B], wam), f"{what}: dp_amax"
    for s in range(n):
        assert torch.equal(slabs[s, :92160], wslabs[s, :92160]), f"{what}: dW3 of slab {s}"
        assert torch.equal(slabs[s, 92160:], wslabs[s, 92160:]), f"{what}: db3 of slab {s}"
    # nothing written past the batch
    assert torch.isnan(dp[B]).all() and torch.isnan(am[B]).all() and torch.isnan(slabs[n]).all(), f"{what}: sentinel"


@pytest.mark.parametrize("B", BATCHES)
def test_fc_backward_bitwise_vs_two_launches(gpu, B):
    """One launch into NaN-filled outputs: every element written, and equal to the parents' bit for bit."""
    dl, pooled, W3, *want = _case(gpu, B)
    outs = _outputs(gpu, B)
    _launch(dl, W3, pooled, outs, B)
    torch.cuda.synchronize()
    _assert_same(outs, want, B, f"B={B}")


@pytest.mark.parametrize("B", BATCHES)
def test_fc_backward_captured_and_replayed(gpu, B):
    """The same comparison after capture in a torch.cuda.graph, for each of two replays into re-NaN-ed outputs."""
    dl, pooled, W3, *want = _case(gpu, B)
    outs = _outputs(gpu, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(dl, W3, pooled, outs, B)            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(dl, W3, pooled, outs, B)
    for r in range(2):
        for t in outs:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(outs, want, B, f"B={B} replay {r}")


def test_ops_fc_backward_wrapper(gpu):
    """ops.fc_backward allocates what it is not given, returns (dpooled, dp_amax, slabs) and refuses a batch mismatch."""
    from splitcnn import ops
    B = 17
    dl, pooled, W3, *want = _case(gpu, B)
    dp, am, slabs = ops.fc_backward(dl, W3, pooled)
    assert torch.equal(dp, want[0]) and torch.equal(am, want[1]) and torch.equal(slabs, want[2])
    dp4 = torch.full((B, 64, 12, 12), NAN, device=gpu)
    got = ops.fc_backward(dl, W3, pooled.view(B, 64, 12, 12), dpooled=dp4.view(B, 9216))
    assert torch.equal(dp4.view(B, 9216), want[0]) and torch.equal(got[2], want[2])
    with pytest.raises(ValueError, match="batch mismatch"):
        ops.fc_backward(dl, W3, pooled[:16])


@pytest.mark.parametrize("graph", [False, True])
def test_split_trainer_step_bitwise_vs_two_launches(gpu, graph):
    """One SplitTrainer step at B = 64 with the role-split launch (the default) and with
    ServerStage.fc_backward_one_launch off (slk_fc_wgrad, then slk_fc_dgrad_amax): the same loss and parameters, bit
    for bit, eager and captured."""
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import SplitTrainer
    B = 64
    x, y = SyntheticMNIST(11).batch(B)
    x, y = x.to(gpu), y.to(gpu)
    res = []
    for one in (True, False):
        tr = SplitTrainer(*init_models(seed=0), device=gpu, graph=graph)
        assert tr.server.fc_backward_one_launch is True
        tr.server.fc_backward_one_launch = one
        tr.step(x, y)
        torch.cuda.synchronize()
        (_, loss), = tr.loss_log.flush()
        res.append((loss, tr.client.params.clone(), tr.server.params.clone()))
    (l1, c1, s1), (l2, c2, s2) = res
    init = SplitTrainer(*init_models(seed=0), device=gpu, graph=False)
    assert not torch.equal(s1, init.server.params) and not torch.equal(c1, init.client.params), "the step did not train"
    assert l1 == l2, (l1, l2)
    assert torch.equal(c1, c2), "client parameters"
    assert torch.equal(s1, s2), "server parameters"
