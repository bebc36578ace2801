"""CPU-side checks of the evaluation path: argument validation of the new C-ABI entries without a GPU,
the host decoding of the metric accumulator (EvalResult.from_raw), and the ops' refusal of CPU tensors."""
import numpy as np
import pytest
import torch


def test_eval_entries_validate_arguments_without_gpu():
    from splitcnn import _lib
    lib = _lib.load()
    # B = -1: hipErrorInvalidValue, whatever the pointers
    assert lib.slk_fc_eval(None, None, None, None, None, None, None, None, -1, None) == 1
    assert lib.slk_eval_logits(None, None, -1, None, None, None, None) == 1
    assert lib.slk_eval_accumulate(None, None, None, -1, None, None) == 1
    assert lib.slk_conv2_fwd_pool_x3p(None, None, None, None, None, -1, None) == 1
    # empty batch: success, no launch
    assert lib.slk_fc_eval(None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.slk_eval_logits(None, None, 0, None, None, None, None) == 0
    assert lib.slk_eval_accumulate(None, None, None, 0, None, None) == 0
    assert lib.slk_conv2_fwd_pool_x3p(None, None, None, None, None, 0, None) == 0
    # null required buffers
    assert lib.slk_fc_eval(None, None, None, None, None, None, None, None, 5, None) == 1
    assert lib.slk_eval_logits(None, None, 5, None, None, None, None) == 1
    assert lib.slk_eval_accumulate(None, None, None, 5, None, None) == 1
    assert lib.slk_conv2_fwd_pool_x3p(None, None, None, None, None, 5, None) == 1
    # labels without a loss_i buffer (pred alone is the predict-only form): refused
    assert lib.slk_eval_logits(16, 16, 5, None, 16, None, None) == 1
    with pytest.raises(_lib.SLKError, match="invalid argument"):
        _lib.call("slk_eval_accumulate", None, None, None, 3, None, None)


def _raw(n, correct, bad, loss_sum, confusion):
    raw = np.zeros(104, dtype=np.int64)
    raw[0], raw[1], raw[2] = n, correct, bad
    raw[3:4].view(np.float64)[0] = loss_sum
    raw[4:] = np.asarray(confusion, dtype=np.int64).reshape(-1)
    return raw


def test_eval_result_decodes_a_hand_built_accumulator():
    from splitcnn.metrics import EvalResult
    conf = np.zeros((10, 10), dtype=np.int64)
    conf[0, 0] = 3          # class 0: 3 of 4 right
    conf[0, 7] = 1
    conf[2, 2] = 5          # class 2: all 5 right
    conf[9, 1] = 2          # class 9: none of 2 right
    r = EvalResult.from_raw(_raw(11, 8, 0, 5.5, conf))
    assert (r.n, r.correct, r.bad_labels) == (11, 8, 0)
    assert r.accuracy == 8 / 11
    assert r.loss == 5.5 / 11
    assert r.confusion.dtype == np.int64 and r.confusion.shape == (10, 10)
    assert np.array_equal(r.confusion, conf)
    assert r.per_class_accuracy[0] == 0.75 and r.per_class_accuracy[2] == 1.0 and r.per_class_accuracy[9] == 0.0
    assert np.isnan(r.per_class_accuracy[[1, 3, 4, 5, 6, 7, 8]]).all()   # classes never seen
    assert r.check() is r
    # torch tensors and lists decode the same
    assert EvalResult.from_raw(torch.from_numpy(_raw(11, 8, 0, 5.5, conf))).loss == r.loss
    with pytest.raises(ValueError, match="104"):
        EvalResult.from_raw(np.zeros(100, dtype=np.int64))


def test_eval_result_bad_labels():
    from splitcnn.metrics import EvalResult
    conf = np.zeros((10, 10), dtype=np.int64)
    conf[4, 4] = 6
    conf[5, 4] = 2
    r = EvalResult.from_raw(_raw(10, 6, 2, 4.0, conf))   # 2 of 10 samples had an out-of-range label
    assert r.bad_labels == 2
    assert r.loss == 4.0 / 8 and r.accuracy == 6 / 8       # means over the samples with a valid label
    with pytest.raises(IndexError, match=r"a label was out of range \[0, 10\)"):
        r.check()
    empty = EvalResult.from_raw(np.zeros(104, dtype=np.int64))
    assert empty.n == 0 and np.isnan(empty.loss) and np.isnan(empty.accuracy)


def test_eval_ops_refuse_cpu_tensors():
    from splitcnn import metrics, ops
    z, y = torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_logits(z, y, loss_i=torch.zeros(2), pred=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fc_eval(torch.zeros(2, 9216), torch.zeros(10, 9216), torch.zeros(10), y, logits=z,
                    loss_i=torch.zeros(2), pred=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_accumulate(torch.zeros(2), y, y, torch.zeros(104, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.evaluate_logits(z, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.EvalMetrics("cpu")
