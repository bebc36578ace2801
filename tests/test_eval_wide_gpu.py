"""GPU tests of the evaluation path of the widened model (K5): WideTrainer.eval_batch / evaluate / predict
against the stages' own forward and WideModelPartB.eval(), bit for bit, and their side effects (none)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else (
        t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def trainer(gpu, graph=True, seed=3):
    from splitcnn.wide import WideTrainer, init_wide_models
    a, b = init_wide_models(seed=seed)
    return WideTrainer(a, b, device=gpu, graph=graph)


def state_of(tr):
    c, s = tr.client, tr.server
    return [c.params, c.m, c.v, c.step_ctr, s.params, s.m, s.v, s.step_ctr, s.loss_log.counter, s.err_flag, s.wf8,
            *c.sh.values()]


@pytest.mark.parametrize("B", [1, 37])
def test_wide_eval_batch_bitwise_and_no_side_effects(gpu, B):
    from splitcnn import ops
    from splitcnn.metrics import EvalMetrics
    from splitcnn.wide import SyntheticCIFAR, c8_to_nchw
    data = SyntheticCIFAR(20 + B)
    (x0, y0), (x, y) = (tuple(t.to(gpu) for t in data.batch(B)) for _ in range(2))
    tr = trainer(gpu)
    tr.step(x0, y0)   # one training step first: Adam state and step counters are non-trivial
    module = tr.server.model.eval()
    module(c8_to_nchw(tr.client.forward(x0)))   # creates the module's dropout counter
    before = [t.clone() for t in state_of(tr)] + [module._drop_step.clone()]
    gs, ng = tr.global_step, len(tr._graphs)
    m = EvalMetrics(gpu)
    pred, loss_i = tr.eval_batch(x, y, m)
    pred, loss_i, logits = pred.clone(), loss_i.clone(), tr.server.eval_logits.clone()
    cut_e = tr.eval_cut.clone()
    r = m.result()
    pr, lg = tr.predict(x, return_logits=True)
    for t, v in zip(state_of(tr) + [module._drop_step], before):
        assert same_bits(t, v)
    assert tr.global_step == gs and len(tr._graphs) == ng and len(tr._eval_graphs) == 1
    # the cut is the client stage's, the logits the module's in eval mode, loss / pred eval_logits' of those
    cut = tr.client.forward(x, tag="check")
    assert same_bits(cut_e, cut)
    logits_m = module(c8_to_nchw(cut)).detach()
    assert same_bits(logits, logits_m) and same_bits(lg, logits_m)
    loss_w, pred_w = ops.eval_logits(logits_m, y)
    assert same_bits(loss_i, loss_w) and torch.equal(pred, pred_w) and torch.equal(pr, pred_w)
    assert np.array_equal(pred.cpu().numpy(), np.argmax(logits_m.cpu().numpy(), axis=1))
    assert r.n == B and r.correct == int((pred_w == y).sum().item())
    want = float(loss_w.double().sum().item()) / B
    assert abs(r.loss - want) <= 1e-10 * abs(want)
    # graph and eager agree bit for bit
    te = trainer(gpu, graph=False)
    te.step(x0, y0)
    pe, le = te.eval_batch(x, y)
    assert same_bits(le, loss_i) and torch.equal(pe, pred) and len(te._eval_graphs) == 0


def test_wide_eval_logits_and_cut_follow_the_replayed_batch_size(gpu):
    """Graphs for two batch sizes, then replays only: server.eval_logits and eval_cut are the buffers of the
    batch eval_batch was just given, bitwise the eager trainer's."""
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(31)
    b37a, b5, b37b = (tuple(t.to(gpu) for t in data.batch(B)) for B in (37, 5, 37))
    tg, te = trainer(gpu, graph=True, seed=9), trainer(gpu, graph=False, seed=9)
    tg.eval_batch(*b37a)
    tg.eval_batch(*b5)
    assert len(tg._eval_graphs) == 2
    for xb, yb in (b37b, b5, b37a):
        pg, lg = tg.eval_batch(xb, yb)
        pe, le = te.eval_batch(xb, yb)
        assert tuple(tg.server.eval_logits.shape) == (xb.shape[0], 10) and tg.eval_cut.shape[0] == xb.shape[0]
        assert same_bits(tg.server.eval_logits, te.server.eval_logits) and same_bits(tg.eval_cut, te.eval_cut)
        assert same_bits(lg, le) and torch.equal(pg, pe)
    assert len(tg._eval_graphs) == 2


def test_wide_step_evaluate_step_equals_step_step(gpu):
    from splitcnn.wide import SyntheticCIFAR
    B = 37
    data = SyntheticCIFAR(77)
    b1, b2, b3 = (tuple(t.to(gpu) for t in data.batch(B)) for _ in range(3))

    def run(evaluate):
        tr = trainer(gpu, seed=5)
        tr.step(*b1)
        if evaluate:
            assert tr.evaluate([b3, b3]).n == 2 * B
        tr.step(*b2)
        torch.cuda.synchronize()
        return [t.clone() for t in state_of(tr)], [v for _, v in tr.loss_log.flush()]

    s0, l0 = run(False)
    s1, l1 = run(True)
    for a, b in zip(s0, s1):
        assert same_bits(a, b)
    assert len(l0) == 2 and np.array_equal(np.float32(l0).view(np.int32), np.float32(l1).view(np.int32))
