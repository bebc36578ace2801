"""wide.WideTrainer(cut_codec=codec.TopKCut(1024, "masked")), B = 8, two steps: the fused step — eager and as a
captured graph — is bit for bit the step composed by hand through the codec's methods (client.forward, roundtrip with
map=, server.step_request, the mask in place, client.backward_step), the row of dcut the client back-propagates is
zero outside the forward's map, and the configurations that existed before keep their bits. The kernels themselves
are held to numpy in test_cuttopk_masked_gpu.py."""
import pytest
import torch

from test_cutmx_trainer_gpu import B, CUT, _batches, _i16, _losses, _same, _stages, _state

pytestmark = pytest.mark.gpu

K, STEPS = 1024, 2


def _trainer(gpu, bwd, graph):
    from splitcnn.codec import TopKCut
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph, cut_codec=TopKCut(K, bwd))


def _bits_of(m):
    """bool [B, 16384] of a uint8 [B, 2048] map: element i is bit i & 7 of byte i >> 3."""
    return ((m.view(B, 2048, 1).int() >> torch.arange(8, device=m.device, dtype=torch.int32)) & 1).bool().view(B, -1)


@pytest.fixture(scope="module")
def hand(gpu):
    """The hand-composed steps: per step (the cut the head read, the map, the dcut back-propagated, the state)."""
    from splitcnn.codec import TopKCut
    q = TopKCut(K, "masked")
    c, s = _stages(gpu)
    m, steps = torch.empty(B, 2048, dtype=torch.uint8, device=gpu), []
    for x, y in _batches(gpu, STEPS):
        raw = c.forward(x)
        cut = q.roundtrip(raw, torch.empty_like(raw), "fwd", map=m)
        dcut, _ = s.step_request(cut, y)
        dense = dcut.clone()
        q.roundtrip(dcut, dcut, "bwd", map=m)
        kept = _bits_of(m)
        assert (kept.sum(1) == K).all() and not (_i16(cut).view(B, -1)[~kept] != 0).any()
        assert not (_i16(dcut).view(B, -1)[~kept] != 0).any() and not torch.equal(_i16(dcut), _i16(dense))
        assert torch.equal(_i16(dcut).view(B, -1)[kept], _i16(dense).view(B, -1)[kept])
        c.backward_step(dcut)
        steps.append((cut.clone(), m.clone(), dcut.clone(), _state(c, s)))
    return steps, _losses(s.loss_log)


@pytest.mark.parametrize("graph", [False, True])
def test_fused_step_is_the_hand_composed_step(gpu, hand, graph):
    tr = _trainer(gpu, "masked", graph)
    for (x, y), (cut, m, dcut, state) in zip(_batches(gpu, STEPS), hand[0]):
        tr.step(x, y)
        assert torch.equal(_i16(tr.server._b("cut_q", CUT, torch.bfloat16)), _i16(cut))   # what the head read
        assert torch.equal(tr.server._b("cut_map", (B, 2048), torch.uint8), m)
        got = _i16(tr.server._b("dcut", CUT, torch.bfloat16))   # what the client back-propagated
        assert torch.equal(got, _i16(dcut)) and not (got.view(B, -1)[~_bits_of(m)] != 0).any()
        assert _same(_state(tr.client, tr.server), state)
    assert _losses(tr.loss_log) == hand[1] and len(hand[1]) == STEPS


@pytest.mark.parametrize("bwd", [None, K])
def test_the_other_backwards_keep_their_bits(gpu, hand, bwd):
    """Eager and graphed against each other, neither equal to the masked step; evaluation under the masked codec is
    the forward-only codec's."""
    a, b = _trainer(gpu, bwd, False), _trainer(gpu, bwd, True)
    for (x, y), (_, _, _, state) in zip(_batches(gpu, STEPS), hand[0]):
        a.step(x, y)
        b.step(x, y)
        assert _same(_state(a.client, a.server), _state(b.client, b.server))
        assert not _same(_state(a.client, a.server), state)
    x, y = _batches(gpu, 1)[0]
    masked = _trainer(gpu, "masked", False)
    for p, q in zip(masked.eval_batch(x, y), _trainer(gpu, None, False).eval_batch(x, y)):
        assert torch.equal(p, q)
