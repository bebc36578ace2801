"""Tensor-level wrappers over the libslk.so C-ABI (include/slk.h).

Every function takes device tensors, checks device / dtype / shape / contiguity on the host (the
kernels assume the exact shapes of src/model_def.py), allocates outputs and workspaces with torch's
caching allocator when the caller does not pass them, and launches on torch's current HIP stream.
Nothing here synchronises, so a sequence of these calls can be captured in a HIP graph.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from . import _lib

CLIENT_NPARAM = 320
SERVER_NPARAM = 110666
OFF_W2, OFF_B2, OFF_W3, OFF_B3 = 0, 18432, 18496, 110656
CONV2_SLAB = 18496   # [dW2 | db2]
FC_SLAB = 92170      # [dW3 | db3]

_F32 = torch.float32


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t: torch.Tensor, name: str, shape=None, dtype=_F32) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"splitcnn: {name} is on {t.device}; the split-CNN ops run only on the MI355X HIP kernels "
            "(move the module and its inputs to a ROCm device). There is no CPU fallback.")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t.data_ptr()


def _out(out, shape, like, dtype=_F32, name="out"):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _dev(out, name, shape, dtype)
    return out


def _err_ptr(err_flag):
    return None if err_flag is None else _dev(err_flag, "err_flag", (1,), torch.int32)


def batch_of(x: torch.Tensor, tail: tuple, name: str) -> int:
    if x.dim() != 1 + len(tail) or tuple(x.shape[1:]) != tail:
        raise ValueError(f"{name}: expected shape [B,{','.join(map(str, tail))}], got {tuple(x.shape)}")
    return int(x.shape[0])


# ------------------------------------------------------------------------------------ client stage
def conv1_fwd(x, W1, b1, out=None, act_amax=None):
    """act = relu(conv1(x)); with act_amax (a [B] f32 tensor) also its per-sample x3 SCALE BOUND, fused:
    conv1_cut_bound (csrc/slk_common.h) = max_c (sum |W1[c]| * max |x| + max(b1[c], 0)) >= max act, not the
    max itself (only its power of two is used)."""
    B = batch_of(x, (1, 28, 28), "x")
    act = _out(out, (B, 32, 26, 26), x)
    if act_amax is not None:
        _lib.call("slk_conv1_fwd_amax", _dev(x, "x"), _dev(W1, "conv1.weight", (32, 1, 3, 3)),
                  _dev(b1, "conv1.bias", (32,)), _dev(act, "act"), _dev(act_amax, "act_amax", (B,)), B, _stream(x))
        return act
    _lib.call("slk_conv1_fwd", _dev(x, "x"), _dev(W1, "conv1.weight", (32, 1, 3, 3)),
              _dev(b1, "conv1.bias", (32,)), _dev(act, "act"), B, _stream(x))
    return act


RELU_BITS_WORDS = 676  # int32 words of the cut's ReLU bit map per sample (slk_relu_bits_bytes / 4)


def relu_bits_buffer(B: int, device) -> torch.Tensor:
    return torch.empty((B, RELU_BITS_WORDS), dtype=torch.int32, device=device)


def conv1_fwd_x3(x, W1, b1, act_amax, act16, act=None, relu_bits=None):
    """conv1 + ReLU writing the x3 server operand: act_amax [B] (the per-sample scale bound
    conv1_cut_bound, >= max act; see conv1_fwd) and the act16 images
    (conv2_act16_bytes(B) uint8), plus the f32 act when `act` is given and the cut's ReLU bit map
    (int32 [B, RELU_BITS_WORDS], the fused client backward's mask) when `relu_bits` is. Returns act (or None)."""
    B = batch_of(x, (1, 28, 28), "x")
    ap = _dev(act, "act", (B, 32, 26, 26)) if act is not None else None
    bp = _dev(relu_bits, "relu_bits", (B, RELU_BITS_WORDS), torch.int32) if relu_bits is not None else None
    _lib.call("slk_conv1_fwd_x3", _dev(x, "x"), _dev(W1, "conv1.weight", (32, 1, 3, 3)), _dev(b1, "conv1.bias", (32,)),
              ap, _dev(act_amax, "act_amax", (B,)), _act16(act16, B), bp, B, _stream(x))
    return act


def conv2_fwd_pool_x3i(act16, act_amax, W2, b2, pooled=None, code=None):
    """The x3 forward + pool reading the act16 images (conv1_fwd_x3 / conv2_fwd_pool(act16=...)) instead
    of the f32 act: the same pooled / code bitwise."""
    B = batch_of(act_amax, (), "act_amax")
    pooled = _out(pooled, (B, 64, 12, 12), act_amax, name="pooled")
    code = _out(code, (B, 64, 12, 12), act_amax, torch.uint8, "code")
    _lib.call("slk_conv2_fwd_pool_x3i", _act16(act16, B), _dev(act_amax, "act_amax", (B,)),
              _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
              _dev(code, "code", dtype=torch.uint8), B, _stream(act_amax))
    return pooled, code


def conv2_dgrad_c1w_nslab(B: int) -> int:
    return _lib.query("slk_conv2_dgrad_x3_c1w_nslab", B)


def conv2_dgrad_client_slabs(dpooled, code, W2, x, relu_bits, dp_amax=None, slabs=None):
    """x3 dgrad fused with the client's ReLU backward + conv1 wgrad: returns the client's gradient
    slabs [conv2_dgrad_c1w_nslab(B), 320] (conv1_wgrad_slabs' layout); the cut gradient is not
    materialised. relu_bits: the ReLU bit map conv1_fwd_x3 wrote for this cut."""
    B = _pooled_batch(dpooled)
    batch_of(x, (1, 28, 28), "x")
    if x.shape[0] != B:
        raise ValueError("x / dpooled batch mismatch")
    dp_amax = row_amax(dpooled) if dp_amax is None else dp_amax
    slabs = _out(slabs, (conv2_dgrad_c1w_nslab(B), CLIENT_NPARAM), x, name="slabs")
    _lib.call("slk_conv2_dgrad_x3_c1w", _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)),
              _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(W2, "conv2.weight", (64, 32, 3, 3)),
              _dev(x, "x"), _dev(relu_bits, "relu_bits", (B, RELU_BITS_WORDS), torch.int32),
              _dev(slabs, "slabs"), B, _stream(x))
    return slabs


def conv1_wgrad_nslab(B: int) -> int:
    return _lib.query("slk_conv1_wgrad_nslab", B)


def conv1_wgrad_slabs(x, act, cut_grad, slabs=None):
    B = batch_of(x, (1, 28, 28), "x")
    nslab = conv1_wgrad_nslab(B)
    slabs = _out(slabs, (nslab, CLIENT_NPARAM), x, name="slabs")
    _lib.call("slk_conv1_wgrad", _dev(x, "x"), _dev(act, "act", (B, 32, 26, 26)),
              _dev(cut_grad, "cut_grad", (B, 32, 26, 26)), _dev(slabs, "slabs"), B, _stream(x))
    return slabs


def conv1_wgrad_remask_slabs(x, W1, b1, cut_grad, slabs=None):
    """conv1_wgrad_slabs with the ReLU mask recomputed from x, W1, b1 (bit-identical to act > 0 for
    the forward's weights): half the HBM traffic, act is not read."""
    B = batch_of(x, (1, 28, 28), "x")
    nslab = conv1_wgrad_nslab(B)
    slabs = _out(slabs, (nslab, CLIENT_NPARAM), x, name="slabs")
    _lib.call("slk_conv1_wgrad_remask", _dev(x, "x"), _dev(W1, "conv1.weight", (32, 1, 3, 3)),
              _dev(b1, "conv1.bias", (32,)), _dev(cut_grad, "cut_grad", (B, 32, 26, 26)), _dev(slabs, "slabs"),
              B, _stream(x))
    return slabs


# ------------------------------------------------------------------------------------ server stage
def row_amax(x, out=None):
    """out[r] = max |x[r]| over each row of a [rows, ...] tensor (the x3 kernels' per-sample scales)."""
    rows = int(x.shape[0])
    n = x.numel() // max(rows, 1)
    out = _out(out, (rows,), x, name="amax")
    _lib.call("slk_row_amax", _dev(x, "x"), rows, n, _dev(out, "amax"), _stream(x))
    return out


def _impl(direct, impl):
    if impl is None:
        return "direct" if direct else "wino"
    if impl not in ("wino", "direct", "x3"):
        raise ValueError(f"conv2 impl must be 'wino', 'direct' or 'x3', got {impl!r}")
    return impl


def conv2_act16_bytes(B: int) -> int:
    """Bytes of the f16 input images conv2_fwd_pool(impl='x3', act16=...) writes for the x3 wgrad."""
    return _lib.query("slk_conv2_act16_bytes", B)


def _act16(t, B):
    _dev(t, "act16", (conv2_act16_bytes(B),), torch.uint8)
    return t.data_ptr()


def conv2_fwd_pool(act, W2, b2, pooled=None, code=None, direct=False, impl=None, act_amax=None, act16=None,
                   act_amax_out=None):
    """impl: 'wino' (Winograd F(2x2,3x3) on the f32 MFMA, default), 'direct' (direct f32 MFMA kernel,
    cross-check; also direct=True) or 'x3' (direct on the f16 MFMA with split operands; act_amax = a
    per-sample scale bound >= max |act| — the client's conv1_cut_bound, or the exact max (row_amax), computed
    here when not given; only its power of two matters). act16 (x3 only, a uint8 tensor of
    conv2_act16_bytes(B)): also write the split input images for conv2_wgrad_slabs(act16=...).
    act_amax_out (x3 with act16, act_amax not given; a float tensor [B]): the forward kernel computes the
    per-sample max itself and writes it there (slk_conv2_fwd_pool_x3sa: no separate pass over act; the
    same values as row_amax, so the same outputs bitwise)."""
    impl = _impl(direct, impl)
    B = batch_of(act, (32, 26, 26), "act")
    if act_amax_out is not None and impl != "x3":
        raise ValueError("act_amax_out is an output of the x3 forward only")
    pooled = _out(pooled, (B, 64, 12, 12), act, name="pooled")
    code = _out(code, (B, 64, 12, 12), act, torch.uint8, "code")
    if impl == "x3":
        if act_amax_out is not None:
            if act_amax is not None or act16 is None:
                raise ValueError("act_amax_out needs act16 and no act_amax")
            _lib.call("slk_conv2_fwd_pool_x3sa", _dev(act, "act"), _dev(act_amax_out, "act_amax_out", (B,)),
                      _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
                      _dev(code, "code", dtype=torch.uint8), _act16(act16, B), B, _stream(act))
            return pooled, code
        if act_amax is None:
            act_amax = row_amax(act)
        if act16 is not None:
            _lib.call("slk_conv2_fwd_pool_x3s", _dev(act, "act"), _dev(act_amax, "act_amax", (B,)),
                      _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
                      _dev(code, "code", dtype=torch.uint8), _act16(act16, B), B, _stream(act))
            return pooled, code
        _lib.call("slk_conv2_fwd_pool_x3", _dev(act, "act"), _dev(act_amax, "act_amax", (B,)),
                  _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
                  _dev(code, "code", dtype=torch.uint8), B, _stream(act))
        return pooled, code
    _lib.call("slk_conv2_fwd_pool_direct" if impl == "direct" else "slk_conv2_fwd_pool", _dev(act, "act"),
              _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
              _dev(code, "code", dtype=torch.uint8), B, _stream(act))
    return pooled, code


def _pooled_batch(pooled):
    if pooled.dim() == 2:
        return batch_of(pooled, (9216,), "pooled")
    return batch_of(pooled, (64, 12, 12), "pooled")


def fc_fwd(pooled, W3, b3, out=None):
    B = _pooled_batch(pooled)
    logits = _out(out, (B, 10), pooled)
    _lib.call("slk_fc_fwd", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
              _dev(b3, "fc1.bias", (10,)), _dev(logits, "logits"), B, _stream(pooled))
    return logits


def fc_logits_xent(pooled, W3, b3, labels, grad_scale, logits=None, loss_i=None, dlogits=None, err_flag=None):
    """fc_fwd + xent_fwd_bwd in one launch (slk_fc_logits_xent), bitwise their outputs."""
    B = _pooled_batch(pooled)
    logits = _out(logits, (B, 10), pooled, name="logits")
    loss_i = _out(loss_i, (B,), pooled, name="loss_i")
    dlogits = _out(dlogits, (B, 10), pooled, name="dlogits")
    eptr = _err_ptr(err_flag)
    _lib.call("slk_fc_logits_xent", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
              _dev(b3, "fc1.bias", (10,)), _labels(labels, B), _dev(logits, "logits"), _dev(loss_i, "loss_i"),
              _dev(dlogits, "dlogits"), float(grad_scale), eptr, B, _stream(pooled))
    return logits, loss_i, dlogits


def _labels(labels, B):
    _dev(labels, "labels", (B,), torch.int64)
    return labels.data_ptr()


# ------------------------------------------------------------------------------------ evaluation / prediction
EVAL_ACC_WORDS = 104  # int64 words of the metric accumulator (include/slk.h, slk_eval_accumulate)


def conv2_fwd_pool_x3p(act16, act_amax, W2, b2, pooled=None):
    """conv2_fwd_pool_x3i without the routing codes (the evaluation forward): the same pooled, bitwise."""
    B = batch_of(act_amax, (), "act_amax")
    pooled = _out(pooled, (B, 64, 12, 12), act_amax, name="pooled")
    _lib.call("slk_conv2_fwd_pool_x3p", _act16(act16, B), _dev(act_amax, "act_amax", (B,)),
              _dev(W2, "conv2.weight", (64, 32, 3, 3)), _dev(b2, "conv2.bias", (64,)), _dev(pooled, "pooled"),
              B, _stream(act_amax))
    return pooled


def _eval_outs(like, B, labels, loss_i, pred, err_flag):
    pred = _out(pred, (B,), like, torch.int64, "pred")
    lptr = eptr = None
    if labels is not None:
        lptr = _labels(labels, B)
        loss_i = _out(loss_i, (B,), like, name="loss_i")
        eptr = _err_ptr(err_flag)
    liptr = _dev(loss_i, "loss_i", (B,)) if loss_i is not None else None
    return pred, loss_i, lptr, liptr, eptr


def fc_eval(pooled, W3, b3, labels=None, logits=None, loss_i=None, pred=None, err_flag=None, store_logits=True):
    """The fc head in evaluation mode (slk_fc_eval): fc_logits_xent's logits and loss_i bitwise, plus pred =
    argmax (int64 [B], first maximum on ties, NaN counts as the maximum); no dlogits. labels=None predicts only
    (loss_i, when given, is left as it is). store_logits=False does not write the logits (returned as None).
    Returns (logits, loss_i, pred)."""
    B = _pooled_batch(pooled)
    logits = _out(logits, (B, 10), pooled, name="logits") if store_logits else None
    pred, loss_i, lptr, liptr, eptr = _eval_outs(pooled, B, labels, loss_i, pred, err_flag)
    _lib.call("slk_fc_eval", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)), _dev(b3, "fc1.bias", (10,)),
              lptr, _dev(logits, "logits") if logits is not None else None, liptr, _dev(pred, "pred", dtype=torch.int64),
              eptr, B, _stream(pooled))
    return logits, loss_i, pred


def eval_logits(logits, labels=None, loss_i=None, pred=None, err_flag=None):
    """fc_eval's loss_i / pred stage (the same bits) for f32 [B, 10] logits already in memory (slk_eval_logits).
    Returns (loss_i, pred); labels=None predicts only."""
    B = batch_of(logits, (10,), "logits")
    pred, loss_i, lptr, liptr, eptr = _eval_outs(logits, B, labels, loss_i, pred, err_flag)
    _lib.call("slk_eval_logits", _dev(logits, "logits"), lptr, B, liptr, _dev(pred, "pred", dtype=torch.int64), eptr,
              _stream(logits))
    return loss_i, pred


def eval_accumulate(loss_i, pred, labels, acc):
    """Add one batch to the device metric accumulator `acc` (int64 [EVAL_ACC_WORDS]; layout in include/slk.h):
    one launch, no host sync (slk_eval_accumulate)."""
    B = batch_of(loss_i, (), "loss_i")
    _lib.call("slk_eval_accumulate", _dev(loss_i, "loss_i", (B,)), _dev(pred, "pred", (B,), torch.int64),
              _labels(labels, B), B, _dev(acc, "acc", (EVAL_ACC_WORDS,), torch.int64), _stream(loss_i))
    return acc


def xent_fwd_bwd(logits, labels, grad_scale, loss_i=None, dlogits=None, err_flag=None):
    B = batch_of(logits, (10,), "logits")
    loss_i = _out(loss_i, (B,), logits, name="loss_i")
    dlogits = _out(dlogits, (B, 10), logits, name="dlogits")
    eptr = _err_ptr(err_flag)
    _lib.call("slk_xent_fwd_bwd", _dev(logits, "logits"), _labels(labels, B), _dev(loss_i, "loss_i"),
              _dev(dlogits, "dlogits"), float(grad_scale), eptr, B, _stream(logits))
    return loss_i, dlogits


def fc_dgrad(dlogits, W3, out=None, dp_amax=None):
    """dp_amax (a [B] f32 tensor): also write the per-sample max |dpooled|, fused."""
    B = batch_of(dlogits, (10,), "dlogits")
    dpooled = _out(out, (B, 9216), dlogits, name="dpooled")
    if dp_amax is None:
        _lib.call("slk_fc_dgrad", _dev(dlogits, "dlogits"), _dev(W3, "fc1.weight", (10, 9216)),
                  _dev(dpooled, "dpooled"), B, _stream(dlogits))
    else:
        _lib.call("slk_fc_dgrad_amax", _dev(dlogits, "dlogits"), _dev(W3, "fc1.weight", (10, 9216)),
                  _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)), B, _stream(dlogits))
    return dpooled


def fc_xent(pooled, W3, b3, labels, grad_scale, logits=None, loss_i=None, dlogits=None,
            dpooled=None, err_flag=None, dp_amax=None):
    """dp_amax (a [B] f32 tensor): also write the per-sample max |dpooled|, fused."""
    B = _pooled_batch(pooled)
    logits = _out(logits, (B, 10), pooled, name="logits")
    loss_i = _out(loss_i, (B,), pooled, name="loss_i")
    dlogits = _out(dlogits, (B, 10), pooled, name="dlogits")
    dpooled = _out(dpooled, tuple(pooled.shape), pooled, name="dpooled")
    eptr = _err_ptr(err_flag)
    if dp_amax is not None:
        _lib.call("slk_fc_xent_amax", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
                  _dev(b3, "fc1.bias", (10,)), _labels(labels, B), _dev(logits, "logits"),
                  _dev(loss_i, "loss_i"), _dev(dlogits, "dlogits"), _dev(dpooled, "dpooled"),
                  _dev(dp_amax, "dp_amax", (B,)), float(grad_scale), eptr, B, _stream(pooled))
        return logits, loss_i, dlogits, dpooled
    _lib.call("slk_fc_xent", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
              _dev(b3, "fc1.bias", (10,)), _labels(labels, B), _dev(logits, "logits"),
              _dev(loss_i, "loss_i"), _dev(dlogits, "dlogits"), _dev(dpooled, "dpooled"),
              float(grad_scale), eptr, B, _stream(pooled))
    return logits, loss_i, dlogits, dpooled


# ---- soft targets (splitcnn.loss): mixed labels + label smoothing, the soft forms of the entries above
def xent_soft_fwd_bwd(logits, labels, grad_scale, smoothing, loss_i=None, dlogits=None, err_flag=None):
    """xent_fwd_bwd on mixed labels with label smoothing (slk_xent_soft_fwd_bwd); smoothing 0 on plain labels is
    bitwise xent_fwd_bwd. A malformed target sets err_flag and writes NaN for its row."""
    B = batch_of(logits, (10,), "logits")
    loss_i = _out(loss_i, (B,), logits, name="loss_i")
    dlogits = _out(dlogits, (B, 10), logits, name="dlogits")
    eptr = _err_ptr(err_flag)
    _lib.call("slk_xent_soft_fwd_bwd", _dev(logits, "logits"), _labels(labels, B), _dev(loss_i, "loss_i"),
              _dev(dlogits, "dlogits"), float(grad_scale), float(smoothing), eptr, B, _stream(logits))
    return loss_i, dlogits


def fc_logits_xent_soft(pooled, W3, b3, labels, grad_scale, smoothing, logits=None, loss_i=None, dlogits=None,
                        err_flag=None):
    """fc_logits_xent on mixed labels with label smoothing in one launch (slk_fc_logits_xent_soft)."""
    B = _pooled_batch(pooled)
    logits = _out(logits, (B, 10), pooled, name="logits")
    loss_i = _out(loss_i, (B,), pooled, name="loss_i")
    dlogits = _out(dlogits, (B, 10), pooled, name="dlogits")
    eptr = _err_ptr(err_flag)
    _lib.call("slk_fc_logits_xent_soft", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
              _dev(b3, "fc1.bias", (10,)), _labels(labels, B), _dev(logits, "logits"), _dev(loss_i, "loss_i"),
              _dev(dlogits, "dlogits"), float(grad_scale), float(smoothing), eptr, B, _stream(pooled))
    return logits, loss_i, dlogits


def fc_xent_soft(pooled, W3, b3, labels, grad_scale, smoothing, logits=None, loss_i=None, dlogits=None,
                 dpooled=None, err_flag=None, dp_amax=None):
    """fc_xent on mixed labels with label smoothing (slk_fc_xent_soft); dp_amax as in fc_xent."""
    B = _pooled_batch(pooled)
    logits = _out(logits, (B, 10), pooled, name="logits")
    loss_i = _out(loss_i, (B,), pooled, name="loss_i")
    dlogits = _out(dlogits, (B, 10), pooled, name="dlogits")
    dpooled = _out(dpooled, tuple(pooled.shape), pooled, name="dpooled")
    eptr = _err_ptr(err_flag)
    _lib.call("slk_fc_xent_soft", _dev(pooled, "pooled"), _dev(W3, "fc1.weight", (10, 9216)),
              _dev(b3, "fc1.bias", (10,)), _labels(labels, B), _dev(logits, "logits"), _dev(loss_i, "loss_i"),
              _dev(dlogits, "dlogits"), _dev(dpooled, "dpooled"),
              _dev(dp_amax, "dp_amax", (B,)) if dp_amax is not None else None, float(grad_scale), float(smoothing),
              eptr, B, _stream(pooled))
    return logits, loss_i, dlogits, dpooled


def fc_wgrad_nslab(B: int) -> int:
    return _lib.query("slk_fc_wgrad_nslab", B)


def fc_wgrad_slabs(dlogits, pooled, slabs=None):
    B = batch_of(dlogits, (10,), "dlogits")
    if _pooled_batch(pooled) != B:
        raise ValueError("pooled / dlogits batch mismatch")
    slabs = _out(slabs, (fc_wgrad_nslab(B), FC_SLAB), dlogits, name="slabs")
    _lib.call("slk_fc_wgrad", _dev(dlogits, "dlogits"), _dev(pooled, "pooled"), _dev(slabs, "slabs"),
              B, _stream(dlogits))
    return slabs


def fc_backward(dlogits, W3, pooled, dpooled=None, dp_amax=None, slabs=None):
    """fc_dgrad (with dp_amax) and fc_wgrad_slabs in one role-split launch (slk_fc_backward): the same bits in
    dpooled [B, 9216], dp_amax [B] and slabs. Returns (dpooled, dp_amax, slabs)."""
    B = batch_of(dlogits, (10,), "dlogits")
    if _pooled_batch(pooled) != B:
        raise ValueError("pooled / dlogits batch mismatch")
    dpooled = _out(dpooled, (B, 9216), dlogits, name="dpooled")
    dp_amax = _out(dp_amax, (B,), dlogits, name="dp_amax")
    slabs = _out(slabs, (fc_wgrad_nslab(B), FC_SLAB), dlogits, name="slabs")
    _lib.call("slk_fc_backward", _dev(dlogits, "dlogits"), _dev(W3, "fc1.weight", (10, 9216)), _dev(pooled, "pooled"),
              _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)), _dev(slabs, "slabs"), B, _stream(dlogits))
    return dpooled, dp_amax, slabs


def _dpooled_batch(dpooled):
    return _pooled_batch(dpooled)


def conv2_dgrad(dpooled, code, W2, out=None, direct=False, impl=None, dp_amax=None):
    impl = _impl(direct, impl)
    B = _dpooled_batch(dpooled)
    cut_grad = _out(out, (B, 32, 26, 26), dpooled, name="cut_grad")
    if impl == "x3":
        if dp_amax is None:
            dp_amax = row_amax(dpooled)
        _lib.call("slk_conv2_dgrad_x3", _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)),
                  _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(W2, "conv2.weight", (64, 32, 3, 3)),
                  _dev(cut_grad, "cut_grad"), B, _stream(dpooled))
        return cut_grad
    direct = impl == "direct"
    _lib.call("slk_conv2_dgrad_direct" if direct else "slk_conv2_dgrad", _dev(dpooled, "dpooled"),
              _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(W2, "conv2.weight", (64, 32, 3, 3)),
              _dev(cut_grad, "cut_grad"), B, _stream(dpooled))
    return cut_grad


def conv2_dgrad_x3_pack(dpooled, code, W2, dp_amax, mask, ranks, vals):
    """The x3 cut gradient in the codec's packed form (slk_conv2_dgrad_x3_pack): the values of the elements
    set in `mask` (the received cut's: int32 words, ceil(B*21632/32)) at their word ranks (cut_ranks), into
    `vals` — what CutCodec.pack extracts from conv2_dgrad(..., impl="x3") without the dense gradient."""
    B = _dpooled_batch(dpooled)
    nw = (B * 21632 + 31) // 32
    _lib.call("slk_conv2_dgrad_x3_pack", _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)),
              _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(W2, "conv2.weight", (64, 32, 3, 3)),
              _dev(mask, "mask", (nw,), torch.int32), _dev(ranks, "ranks", (nw,), torch.int32),
              _dev(vals, "vals"), B, _stream(dpooled))
    return vals


def conv2_dgrad_x3_pack_parts(dpooled, code, W2, dp_amax, parts, part_b):
    """conv2_dgrad_x3_pack over the B / part_b parts of a server chunk in one launch: parts = int64 device
    table [B / part_b, 3] of (mask, ranks, vals) pointers (slk_conv2_dgrad_x3_pack_parts)."""
    B = _dpooled_batch(dpooled)
    if part_b <= 0 or B % part_b:
        raise ValueError(f"part_b {part_b} must divide the chunk's {B} samples")
    _lib.call("slk_conv2_dgrad_x3_pack_parts", _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)),
              _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(W2, "conv2.weight", (64, 32, 3, 3)),
              _dev(parts, "parts", (B // part_b, 3), torch.int64), part_b, B, _stream(dpooled))


def cut_unpack_x3_parts(parts, part_b, act_amax, act16):
    """cut_unpack_x3 over the B / part_b parts of a server chunk in one launch: parts = int64 device table
    [B / part_b, 3] of (vals, mask, ranks) pointers (slk_cut_unpack_x3_parts)."""
    B = batch_of(act_amax, (), "act_amax")
    if part_b <= 0 or B % part_b:
        raise ValueError(f"part_b {part_b} must divide the chunk's {B} samples")
    _lib.call("slk_cut_unpack_x3_parts", _dev(parts, "parts", (B // part_b, 3), torch.int64), part_b,
              _dev(act_amax, "act_amax", (B,)), B, _act16(act16, B), _stream(act_amax))
    return act16


def cut_offsets_ranks_parts(parts, n):
    """Counts, offsets, totals and word ranks of every part of a chunk from its received mask, three launches
    for all parts: parts = int64 device table [np, 5] of (mask, counts, offsets, total, ranks) pointers."""
    _lib.call("slk_cut_offsets_ranks_parts", _dev(parts, "parts", (parts.shape[0], 5), torch.int64), parts.shape[0], n,
              _stream(parts))


def mfma_probe_tflops(device=None, iters: int = 40000, reps: int = 3) -> float:
    """Measurement only: this device's sustained dense f16 MFMA rate in TFLOP/s (slk_mfma_probe: 6 independent
    v_mfma_f32_16x16x32_f16 chains per wave on varied operands, 2 waves per SIMD on every CU), median of
    `reps` launches timed with HIP events on the current stream."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    nb = _lib.query("slk_mfma_probe_blocks")
    out = torch.empty(nb * 256, device=dev)
    st = torch.cuda.current_stream(dev)
    _lib.call("slk_mfma_probe", out.data_ptr(), iters, st.cuda_stream)   # warm-up (clocks ramp)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        _lib.call("slk_mfma_probe", out.data_ptr(), iters, st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = sorted(ts)[len(ts) // 2]
    return nb * 4 * iters * 6 * 16384 / (ms * 1e-3) / 1e12


def cut_unpack_x3(vals, mask, ranks, act_amax, act16):
    """A received codec micro-batch (mask + values + word ranks, B samples) -> the x3 input images act16
    (conv2_act16_bytes(B) uint8) at the scales act_amax: conv1_fwd_x3's images of the same cut, bit for bit."""
    B = batch_of(act_amax, (), "act_amax")
    nw = (B * 21632 + 31) // 32
    _lib.call("slk_cut_unpack_x3", _dev(vals, "vals"), _dev(mask, "mask", (nw,), torch.int32),
              _dev(ranks, "ranks", (nw,), torch.int32), _dev(act_amax, "act_amax", (B,)), B, _act16(act16, B),
              _stream(act_amax))
    return act16


def conv2_wgrad_nslab(B: int, direct: bool = False, impl=None) -> int:
    impl = _impl(direct, impl)
    return _lib.query({"wino": "slk_conv2_wgrad_nslab", "direct": "slk_conv2_wgrad_direct_nslab",
                       "x3": "slk_conv2_wgrad_x3_nslab"}[impl], B)


def conv2_wgrad_slabs(act, dpooled, code, slabs=None, direct=False, impl=None, act_amax=None, dp_amax=None,
                      act16=None):
    """act16 (x3 only): the forward's split input images (conv2_fwd_pool(..., act16=...), same act and
    act_amax, or conv1_fwd_x3) — the kernel then moves them by LDS-DMA instead of loading and splitting
    act, and act may be None (act_amax is then required)."""
    impl = _impl(direct, impl)
    if act is None:
        if impl != "x3" or act16 is None or act_amax is None:
            raise ValueError("conv2_wgrad_slabs: act=None needs impl='x3', act16 and act_amax")
        B = _dpooled_batch(dpooled)
    else:
        B = batch_of(act, (32, 26, 26), "act")
        if _dpooled_batch(dpooled) != B:
            raise ValueError("act / dpooled batch mismatch")
    slabs = _out(slabs, (conv2_wgrad_nslab(B, impl=impl), CONV2_SLAB), dpooled, name="slabs")
    if impl == "x3":
        act_amax = row_amax(act) if act_amax is None else act_amax
        dp_amax = row_amax(dpooled) if dp_amax is None else dp_amax
        if act16 is not None:
            _lib.call("slk_conv2_wgrad_x3s", _act16(act16, B), _dev(act_amax, "act_amax", (B,)),
                      _dev(dpooled, "dpooled"), _dev(dp_amax, "dp_amax", (B,)),
                      _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(slabs, "slabs"), B, _stream(dpooled))
            return slabs
        _lib.call("slk_conv2_wgrad_x3", _dev(act, "act"), _dev(act_amax, "act_amax", (B,)), _dev(dpooled, "dpooled"),
                  _dev(dp_amax, "dp_amax", (B,)), _dev(code, "code", (B, 64, 12, 12), torch.uint8),
                  _dev(slabs, "slabs"), B, _stream(act))
        return slabs
    direct = impl == "direct"
    _lib.call("slk_conv2_wgrad_direct" if direct else "slk_conv2_wgrad", _dev(act, "act"), _dev(dpooled, "dpooled"),
              _dev(code, "code", (B, 64, 12, 12), torch.uint8), _dev(slabs, "slabs"), B, _stream(act))
    return slabs


# ------------------------------------------------------------------------------------ reductions
def reduce_slabs(slabs, out=None, accumulate=False):
    """out (+)= sum over slabs (fixed order)."""
    nslab, n = slabs.shape
    out = _out(out, (n,), slabs, name="out")
    _lib.call("slk_reduce_slabs", _dev(slabs, "slabs"), nslab, n, _dev(out, "out"), int(bool(accumulate)),
              _stream(slabs))
    return out


def sgd_from_slabs(param, grad, slabs, lr):
    """param -= lr * sum(slabs); grad = sum(slabs) (grad may be None). 1-D flat views."""
    nslab, n = slabs.shape
    _dev(param, "param", (n,))
    gptr = _dev(grad, "grad", (n,)) if grad is not None else None
    _lib.call("slk_sgd_from_slabs", param.data_ptr(), gptr, _dev(slabs, "slabs"), nslab, n, float(lr),
              _stream(param))


def sgd_multi_from_slabs(segments, lr, loss=None):
    """ONE launch for every optimizer step of a split step: for each (param, grad, slabs) in
    `segments` (<= 4) sgd_from_slabs(param, grad, slabs, lr), plus loss_log(*loss) when
    loss = (values, scale, ring, counter) — bit-identical to the separate launches. A segment whose
    param is None only reduces its slabs into grad (reduce_slabs of several buffers in one launch)."""
    k = len(segments)
    if not 0 <= k <= 4:
        raise ValueError("sgd_multi_from_slabs: at most 4 segments")
    cols = [[], [], [], [], []]
    stream_of = None
    for param, grad, sl in segments:
        nsl, n = sl.shape
        if param is None and grad is None:
            raise ValueError("sgd_multi_from_slabs: a segment needs a param or a grad")
        row = (_dev(param, "param", (n,)) if param is not None else None,
               _dev(grad, "grad", (n,)) if grad is not None else None, _dev(sl, "slabs"), int(nsl), int(n))
        for c, v in zip(cols, row):
            c.append(v)
        stream_of = (param if param is not None else grad) if stream_of is None else stream_of
    if stream_of is None and loss is not None:
        stream_of = loss[0]
    if stream_of is None:
        return
    _lib.call("slk_sgd_multi_from_slabs", *_host_arrays(cols), k, float(lr), *_loss_args(loss), _stream(stream_of))


def _host_arrays(columns, n_int=2, k=4):
    """Host arrays (length k) for the *_multi_from_slabs entry points, as void pointers: device pointers,
    except the last n_int columns (nslab, n), which are ints."""
    P = ctypes.c_void_p
    types = [P] * (len(columns) - n_int) + [ctypes.c_int] * n_int
    return [ctypes.cast((t * k)(*col), P) for t, col in zip(types, columns)]


def _loss_args(loss):
    if loss is None:
        return None, 0, 0.0, None, 0, None
    values, scale, ring, counter = loss
    return (_dev(values, "values"), values.numel(), float(scale), _dev(ring, "ring"), ring.numel(),
            _dev(counter, "counter", (1,), torch.int32))


def _lr_args(lr_table, step):
    """(table pointer, length, step counter pointer) of a device learning-rate table (optim.LRSchedule.table)
    and a stage's device step counter."""
    if lr_table.dim() != 1 or lr_table.numel() < 1:
        raise ValueError("lr_table: expected a 1-D table of at least one rate")
    return _dev(lr_table, "lr_table"), lr_table.numel(), _dev(step, "step", (1,), torch.int32)


def sgdm_from_slabs(param, grad, buf, slabs, lr_table, step, momentum=0.0, dampening=0.0, weight_decay=0.0,
                    nesterov=False):
    """torch.optim.SGD's step from sum(slabs) with the rate lr_table[min(step, len - 1)] read on the device
    (slk_sgdm_from_slabs); grad (may be None) receives the reduced gradient, buf is the momentum buffer
    (may be None when momentum is 0). The caller advances `step` (tick) after the stage's launches."""
    nslab, n = slabs.shape
    _dev(param, "param", (n,))
    gptr = _dev(grad, "grad", (n,)) if grad is not None else None
    bptr = _dev(buf, "buf", (n,)) if buf is not None else None
    _lib.call("slk_sgdm_from_slabs", param.data_ptr(), gptr, bptr, _dev(slabs, "slabs"), nslab, n,
              *_lr_args(lr_table, step), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
              _stream(param))


def sgdm_multi_from_slabs(segments, lr_table, step, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                          loss=None):
    """ONE launch: sgdm_from_slabs(param, grad, buf, slabs, ...) for each of `segments` (<= 4), plus
    loss_log(*loss) — bit-identical to the separate launches (slk_sgdm_multi_from_slabs)."""
    k = len(segments)
    if not 0 <= k <= 4:
        raise ValueError("sgdm_multi_from_slabs: at most 4 segments")
    cols = [[], [], [], [], [], []]
    for param, grad, buf, sl in segments:
        nsl, n = sl.shape
        row = (_dev(param, "param", (n,)), _dev(grad, "grad", (n,)) if grad is not None else None,
               _dev(buf, "buf", (n,)) if buf is not None else None, _dev(sl, "slabs"), int(nsl), int(n))
        for c, v in zip(cols, row):
            c.append(v)
    stream_of = segments[0][0] if k else (loss[0] if loss is not None else None)
    if stream_of is None:
        return
    _lib.call("slk_sgdm_multi_from_slabs", *_host_arrays(cols), k, *_lr_args(lr_table, step), float(momentum),
              float(dampening), float(weight_decay), int(bool(nesterov)), *_loss_args(loss), _stream(stream_of))


def _adam_columns(segments):
    """Checked columns (param, grad, m, v, slabs, nslab, n) of (param, grad, m, v, slabs) segments; grad may be None."""
    cols = [[], [], [], [], [], [], []]
    for param, grad, m, v, sl in segments:
        nsl, n = sl.shape
        row = (_dev(param, "param", (n,)), _dev(grad, "grad", (n,)) if grad is not None else None,
               _dev(m, "m", (n,)), _dev(v, "v", (n,)), _dev(sl, "slabs"), int(nsl), int(n))
        for c, val in zip(cols, row):
            c.append(val)
    return cols


def adamw_from_slabs(param, grad, m, v, slabs, lr_table, step, beta1, beta2, eps, weight_decay=0.0, decoupled=True):
    """torch.optim.AdamW's (decoupled) or torch.optim.Adam(weight_decay)'s step from sum(slabs), t = step + 1,
    the rate read from the device table (slk_adamw_from_slabs); grad may be None."""
    nslab, n = slabs.shape
    gptr = _dev(grad, "grad", (n,)) if grad is not None else None
    _lib.call("slk_adamw_from_slabs", _dev(param, "param", (n,)), gptr, _dev(m, "m", (n,)), _dev(v, "v", (n,)),
              _dev(slabs, "slabs"), nslab, n, *_lr_args(lr_table, step), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(bool(decoupled)), _stream(param))


def adamw_multi_from_slabs(segments, lr_table, step, beta1, beta2, eps, weight_decay=0.0, decoupled=True):
    """ONE launch: adamw_from_slabs(param, grad, m, v, slabs, ...) for each of `segments` (<= 4),
    bit-identical to the separate launches (slk_adamw_multi_from_slabs)."""
    k = len(segments)
    if not 1 <= k <= 4:
        raise ValueError("adamw_multi_from_slabs: 1 to 4 segments")
    _lib.call("slk_adamw_multi_from_slabs", *_host_arrays(_adam_columns(segments)), k, *_lr_args(lr_table, step),
              float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(decoupled)),
              _stream(segments[0][0]))


def adam_from_slabs(param, grad, m, v, slabs, lr, beta1, beta2, eps, step):
    """torch.optim.Adam's step from sum(slabs), t = step + 1, `lr` by value (slk_adam_from_slabs: the default K5
    recipe); grad may be None. The caller advances `step` (tick) after the stage's launches."""
    nslab, n = slabs.shape
    gptr = _dev(grad, "grad", (n,)) if grad is not None else None
    _lib.call("slk_adam_from_slabs", _dev(param, "param", (n,)), gptr, _dev(m, "m", (n,)), _dev(v, "v", (n,)),
              _dev(slabs, "slabs"), nslab, n, float(lr), float(beta1), float(beta2), float(eps),
              _dev(step, "step", (1,), torch.int32), _stream(param))


def adam_multi_from_slabs(segments, lr, beta1, beta2, eps, step):
    """ONE launch: adam_from_slabs(param, grad, m, v, slabs, ...) for each of `segments` (<= 4), bit-identical to
    the separate launches (slk_adam_multi_from_slabs)."""
    k = len(segments)
    if not 1 <= k <= 4:
        raise ValueError("adam_multi_from_slabs: 1 to 4 segments")
    _lib.call("slk_adam_multi_from_slabs", *_host_arrays(_adam_columns(segments)), k, float(lr), float(beta1),
              float(beta2), float(eps), _dev(step, "step", (1,), torch.int32), _stream(segments[0][0]))


# ---- global-norm gradient clipping: reduce + square-norm partials, then the clipped step (two launches)
@functools.lru_cache(maxsize=None)
def reduce_sqnorm_nblk(n, nslab):
    """Blocks (= square-norm partials) that reduce_sqnorm_multi spends on one [nslab, n] slab set (a pure function
    of the two sizes: remembered, since every clipped or layer-wise step asks it three times per segment)."""
    return _lib.query("slk_reduce_sqnorm_nblk", int(n), int(nslab))


def clip_partials_needed(segments):
    """Floats of partials one group of `segments` (each ending in its [nslab, n] slabs) needs."""
    return sum(reduce_sqnorm_nblk(seg[-1].shape[1], seg[-1].shape[0]) for seg in segments)


def _group_args(groups, who, width, trust=False):
    """The host arrays the two passes of a clipped or (trust) layer-wise step share. groups = [(partials, out,
    segments)], one per stage, out its norm_out [norm, coef] or trust_out; a segment is `width` tensors (param,
    grad, state ..., slabs) and under `trust` nw, the number of weight elements of the [W | b] pair (the rest is
    the bias). grad None: the [1, n] slabs ARE the gradient block (reduced earlier), read in place. Returns
    (columns of the tensors' pointers, nslab, n, nw (empty without trust), group ids, partials pointers, out
    pointers, a tensor to take the stream from)."""
    cols = [[] for _ in range(width)]
    nslab, ns, nws, gid, parts, outs = [], [], [], [], [], []
    for g, (partials, out, segments) in enumerate(groups):
        if not segments:
            raise ValueError(f"{who}: group {g} has no segment")
        for seg in segments:
            if len(seg) != width + trust:
                raise ValueError(f"{who}: a segment is {width} tensors" + (" and nw" if trust else ""))
            sl = seg[width - 1]
            nsl, n = sl.shape
            if trust:
                nws.append(int(seg[-1]))
                if not 0 <= nws[-1] <= n:
                    raise ValueError(f"{who}: nw = {nws[-1]} outside [0, n = {n}]")
            grad = seg[1]
            if grad is None:
                if nsl != 1:
                    raise ValueError(f"{who}: a segment without grad steps in place from ONE slab")
                grad = sl.view(-1)
            names = ("param", "grad") + ("state",) * (width - 3)
            for c, t, name in zip(cols, (seg[0], grad) + tuple(seg[2:width - 1]), names):
                c.append(_dev(t, name, (n,)) if t is not None else None)
            cols[-1].append(_dev(sl, "slabs"))
            nslab.append(int(nsl))
            ns.append(int(n))
            gid.append(g)
        need = (trust_partials_needed if trust else clip_partials_needed)(segments)
        if trust:
            if _dev(partials, "partials") % 16 or partials.numel() < need:
                raise ValueError(f"{who}: group {g} needs {need} partials (16-byte aligned), got {partials.numel()}")
            if _dev(out, "trust_out") and out.numel() < 6 * len(segments):
                raise ValueError(f"{who}: group {g} needs a trust_out of [{2 * len(segments)}, 3]")
        else:
            if _dev(partials, "partials") and partials.numel() < need:
                raise ValueError(f"{who}: group {g} needs {need} partials, got {partials.numel()}")
            _dev(out, "norm_out", (2,))
        parts.append(partials.data_ptr())
        outs.append(out.data_ptr())
    if not 1 <= len(gid) <= 4:
        raise ValueError(f"{who}: 1 to 4 segments")
    return cols, nslab, ns, nws, gid, parts, outs, groups[0][2][0][0]


def reduce_sqnorm_multi(groups, loss=None):
    """Pass 1 of a clipped step (slk_reduce_sqnorm_multi), ONE launch: every segment's grad = the fixed-order
    sum of its slabs (bitwise what sgdm_from_slabs / adamw_from_slabs write) and one partial of sum g^2 per
    block into its group's `partials`; plus loss_log(*loss). groups = [(partials, norm_out, segments)] as
    for sgdm_clip_multi / adamw_clip_multi (norm_out is not written here)."""
    width = len(groups[0][2][0])
    cols, nslab, ns, _, gid, parts, _, like = _group_args(groups, "reduce_sqnorm_multi", width)
    _lib.call("slk_reduce_sqnorm_multi", *_host_arrays([cols[1], cols[-1], nslab, ns, gid], n_int=3), len(gid),
              *_host_arrays([parts], n_int=0), len(groups), *_loss_args(loss), _stream(like))


def sgdm_clip_multi(groups, max_norm, lr_table, step, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """Pass 2 for torch.optim.SGD (slk_sgdm_clip_multi), ONE launch after reduce_sqnorm_multi(groups): per
    group (one stage) norm = sqrt(sum of its partials), coef = min(1, max_norm / (norm + 1e-6)) -> norm_out,
    then sgdm_from_slabs' update from coef * grad. groups = [(partials, norm_out, [(param, grad, buf, slabs),
    ...])]; grad stays the unclipped gradient; max_norm is a device f32[1] (optim.ClipNorm.value)."""
    cols, nslab, ns, _, gid, parts, outs, like = _group_args(groups, "sgdm_clip_multi", 4)
    _lib.call("slk_sgdm_clip_multi", *_host_arrays(cols[:3] + [nslab, ns, gid], n_int=3), len(gid),
              *_host_arrays([parts, outs], n_int=0), len(groups), _dev(max_norm, "max_norm", (1,)),
              *_lr_args(lr_table, step), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)),
              _stream(like))


def adamw_clip_multi(groups, max_norm, lr_table, step, beta1, beta2, eps, weight_decay=0.0, decoupled=True):
    """Pass 2 for torch.optim.AdamW / Adam (slk_adamw_clip_multi): as sgdm_clip_multi with segments
    (param, grad, m, v, slabs) and adamw_from_slabs' update from coef * grad."""
    cols, nslab, ns, _, gid, parts, outs, like = _group_args(groups, "adamw_clip_multi", 5)
    _lib.call("slk_adamw_clip_multi", *_host_arrays(cols[:4] + [nslab, ns, gid], n_int=3), len(gid),
              *_host_arrays([parts, outs], n_int=0), len(groups), _dev(max_norm, "max_norm", (1,)),
              *_lr_args(lr_table, step), float(beta1), float(beta2), float(eps), float(weight_decay),
              int(bool(decoupled)), _stream(like))


# ---- layer-wise trust ratios (LARS / LAMB): per-tensor norm partials, then the scaled step (two launches)
def trust_partials_needed(segments):
    """Floats of partials one group of layer-wise `segments` (each ending in its [nslab, n] slabs and nw) needs:
    four per block of reduce_tnorm_multi / lamb_moments_multi."""
    return 4 * sum(reduce_sqnorm_nblk(seg[-2].shape[1], seg[-2].shape[0]) for seg in segments)


def reduce_tnorm_multi(groups, loss=None):
    """Pass 1 of a LARS step (slk_reduce_tnorm_multi), ONE launch: every segment's grad = the fixed-order sum of
    its slabs and four partials per block, [g2_W, p2_W, g2_b, p2_b], into its group's `partials`; plus
    loss_log(*loss). groups = [(partials, trust_out, [(param, grad, buf, slabs, nw), ...])] as for lars_multi
    (trust_out is not written here)."""
    cols, nslab, ns, nws, gid, parts, _, like = _group_args(groups, "reduce_tnorm_multi", 4, trust=True)
    _lib.call("slk_reduce_tnorm_multi", *_host_arrays([cols[1], cols[0], cols[-1], nslab, ns, nws, gid], n_int=4),
              len(gid), *_host_arrays([parts], n_int=0), len(groups), *_loss_args(loss), _stream(like))


def lars_multi(groups, lr_table, step, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
               trust_coef=1e-3, eps=1e-8, exclude_bias=True):
    """Pass 2 of a LARS step (slk_lars_multi), ONE launch after reduce_tnorm_multi(groups): per tensor (the
    weight and the bias of each segment) ratio = trust_coef * |w| / (|g| + wd * |w| + eps) (1 where a norm is
    0), then sgdm_from_slabs' momentum arithmetic on ratio * (g + wd * w). trust_out[2k], [2k + 1] =
    [w_norm, g_norm, ratio] of the weight and the bias of the group's k-th segment."""
    cols, nslab, ns, nws, gid, parts, outs, like = _group_args(groups, "lars_multi", 4, trust=True)
    _lib.call("slk_lars_multi", *_host_arrays(cols[:3] + [nslab, ns, nws, gid], n_int=4), len(gid),
              *_host_arrays([parts, outs], n_int=0), len(groups), *_lr_args(lr_table, step), float(momentum),
              float(dampening), float(weight_decay), int(bool(nesterov)), float(trust_coef), float(eps),
              int(bool(exclude_bias)), _stream(like))


def lamb_moments_multi(groups, step, beta1, beta2, eps, weight_decay=0.0, exclude_bias=True, loss=None):
    """Pass 1 of a LAMB step (slk_lamb_moments_multi), ONE launch: grad = the fixed-order slab sum, Adam's m and
    v moved and stored, and four partials per block, [u2_W, p2_W, u2_b, p2_b], of the update direction
    u = m-hat / (sqrt(v-hat) + eps) + wd * p. groups = [(partials, trust_out, [(param, grad, m, v, slabs, nw),
    ...])] as for lamb_multi."""
    cols, nslab, ns, nws, gid, parts, _, like = _group_args(groups, "lamb_moments_multi", 5, trust=True)
    _lib.call("slk_lamb_moments_multi",
              *_host_arrays([cols[1], cols[0], cols[2], cols[3], cols[-1], nslab, ns, nws, gid], n_int=4), len(gid),
              *_host_arrays([parts], n_int=0), len(groups), _dev(step, "step", (1,), torch.int32), float(beta1),
              float(beta2), float(eps), float(weight_decay), int(bool(exclude_bias)), *_loss_args(loss), _stream(like))


def lamb_multi(groups, lr_table, step, beta1, beta2, eps, weight_decay=0.0, exclude_bias=True):
    """Pass 2 of a LAMB step (slk_lamb_multi), ONE launch after lamb_moments_multi(groups): per tensor
    ratio = |w| / |u| (1 where a norm is 0) and p -= lr * ratio * u, u recomputed from the stored moments."""
    cols, nslab, ns, nws, gid, parts, outs, like = _group_args(groups, "lamb_multi", 5, trust=True)
    _lib.call("slk_lamb_multi", *_host_arrays([cols[0], cols[2], cols[3], nslab, ns, nws, gid], n_int=4), len(gid),
              *_host_arrays([parts, outs], n_int=0), len(groups), *_lr_args(lr_table, step), float(beta1),
              float(beta2), float(eps), float(weight_decay), int(bool(exclude_bias)), _stream(like))


def ema_multi(segments, decay, step, start=0, warmup=True):
    """ONE launch (slk_ema_multi): e <- e + (1 - d)(p - e) for each (e, p) of `segments` (1 to 8 flat f32 blocks of
    equal length, any 4-byte alignment, e and p apart), or e <- p while *step < start; d is *decay, under `warmup`
    min(*decay, (1 + n) / (10 + n)) with n = *step - start + 1. decay (f32[1], optim.EMA.value) and step (i32[1], the
    stage's counter BEFORE its tick) are read on the device; start and warmup travel by value."""
    k = len(segments)
    if not 1 <= k <= 8:
        raise ValueError("ema_multi: 1 to 8 segments")
    es, ps, ns = [], [], []
    for e, p in segments:
        if e.dim() != 1:
            raise ValueError("ema_multi: a segment is a pair of flat blocks")
        es.append(_dev(e, "ema", None))
        ps.append(_dev(p, "param", tuple(e.shape)))
        ns.append(int(e.numel()))
    _lib.call("slk_ema_multi", *_host_arrays([es, ps, ns], n_int=1, k=k), k, _dev(decay, "decay", (1,)),
              _dev(step, "step", (1,), torch.int32), int(start), int(bool(warmup)), _stream(decay))


def tick(counter):
    """++counter on the device (a stage's optimizer step counter; advances inside a captured graph)."""
    _lib.call("slk_tick", _dev(counter, "counter", (1,), torch.int32), _stream(counter))


def sgd(param, grad, lr):
    n = param.numel()
    _lib.call("slk_sgd", _dev(param, "param"), _dev(grad, "grad", tuple(param.shape)), n, float(lr),
              _stream(param))


def loss_sum(values, scale, out=None):
    """out[0] = scale * sum(values) (fixed order); out may be a 1-element view of a bigger buffer."""
    n = values.numel()
    if out is None:
        out = torch.empty(1, dtype=_F32, device=values.device)
    _dev(out, "out")
    _lib.call("slk_loss_sum", _dev(values, "values"), n, float(scale), out.data_ptr(), _stream(values))
    return out


def loss_mean(loss_i, out=None):
    return loss_sum(loss_i, 1.0 / loss_i.numel(), out)


def loss_log(values, scale, ring, counter):
    n = values.numel()
    _lib.call("slk_loss_log", _dev(values, "values"), n, float(scale), _dev(ring, "ring"), ring.numel(),
              _dev(counter, "counter", (1,), torch.int32), _stream(values))


# ------------------------------------------------------------------------------------ data
MNIST_MEAN, MNIST_STD = 0.1307, 0.3081   # client_part.py:63


def mnist_batch(images, labels, idx, x=None, y=None, err_flag=None, mean=MNIST_MEAN, std=MNIST_STD):
    """Gather + ToTensor + Normalize one batch from the HBM-resident u8 dataset (slk_mnist_batch)."""
    n = batch_of(images, (28, 28), "images")
    if labels.shape != (n,):
        raise ValueError(f"labels: expected shape ({n},), got {tuple(labels.shape)}")
    B = int(idx.shape[0])
    x = _out(x, (B, 1, 28, 28), images, name="x")
    y = _out(y, (B,), images, dtype=torch.int64, name="y")
    _lib.call("slk_mnist_batch", _dev(images, "images", dtype=torch.uint8),
              _dev(labels, "labels", dtype=torch.uint8), n, _dev(idx, "idx", (B,), torch.int64), B,
              float(mean), float(std), x.data_ptr(), y.data_ptr(),
              _err_ptr(err_flag), _stream(x))
    return x, y


def _image_front(images, labels, idx, mean, std, x, y):
    """What image_batch, image_batch_mix and image_batch_blend check and allocate alike: (images as [N,C,H,W],
    (n, C, H, W), mean and std as c_float arrays, B, x, y)."""
    if images.dim() == 3:
        images = images.unsqueeze(1)
    if images.dim() != 4:
        raise ValueError(f"images: expected shape [N,C,H,W] or [N,H,W], got {tuple(images.shape)}")
    n, C, H, W = (int(d) for d in images.shape)
    if labels.shape != (n,):
        raise ValueError(f"labels: expected shape ({n},), got {tuple(labels.shape)}")
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != C or len(std) != C:
        raise ValueError(f"mean / std: expected {C} values each, got {len(mean)} and {len(std)}")
    B = int(idx.shape[0])
    x = _out(x, (B, C, H, W), images, name="x")
    y = _out(y, (B,), images, dtype=torch.int64, name="y")
    return images, (n, C, H, W), (ctypes.c_float * C)(*mean), (ctypes.c_float * C)(*std), B, x, y


def _image_tail(pad, flip, seed, epoch, x, y, err_flag, *mode_args):
    """The arguments the three entries end with; `mode_args` are the entry's own, between epoch and x."""
    return (int(pad), int(bool(flip)), int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, *mode_args, x.data_ptr(),
            y.data_ptr(), _err_ptr(err_flag), _stream(x))


def image_batch(images, labels, idx, *, mean, std, pad=0, flip=False, seed=0, epoch=0, x=None, y=None,
                err_flag=None):
    """RandomCrop(H, padding=pad) + RandomHorizontalFlip (if `flip`) + ToTensor + Normalize(mean, std) of the
    rows `idx` of the HBM-resident u8 dataset `images` [N,C,H,W] ([N,H,W]: C = 1), one slk_image_batch launch;
    the draws are keyed on (dataset index, epoch, seed) (include/slk.h; cifar.augment_draws is their host
    twin). pad=0, flip=False is plain gather + normalise. The library decides which (C,H,W) and pad it serves:
    anything else raises _lib.SLKError (invalid argument)."""
    images, dims, mean, std, B, x, y = _image_front(images, labels, idx, mean, std, x, y)
    _lib.call("slk_image_batch", _dev(images, "images", dtype=torch.uint8),
              _dev(labels, "labels", dtype=torch.uint8), *dims, _dev(idx, "idx", (B,), torch.int64), B, mean, std,
              *_image_tail(pad, flip, seed, epoch, x, y, err_flag))
    return x, y


def image_batch_mix(images, labels, idx, idx2, *, mean, std, prob=1.0, pad=0, flip=False, seed=0, epoch=0, x=None,
                    y=None, err_flag=None):
    """image_batch with CutMix (slk_image_batch_mix): batch position s shows row idx[s] with a box of row idx2[s]
    pasted in, each under its own crop and flip; y holds mixed labels (splitcnn.loss.unpack_mixed). The box is keyed
    on (idx[s], epoch, seed) and applied with probability `prob` (loss.cutmix_draws is the host twin). prob=0 is
    bitwise image_batch."""
    images, dims, mean, std, B, x, y = _image_front(images, labels, idx, mean, std, x, y)
    _lib.call("slk_image_batch_mix", _dev(images, "images", dtype=torch.uint8),
              _dev(labels, "labels", dtype=torch.uint8), *dims, _dev(idx, "idx", (B,), torch.int64),
              _dev(idx2, "idx2", (B,), torch.int64), B, mean, std,
              *_image_tail(pad, flip, seed, epoch, x, y, err_flag, float(prob)))
    return x, y


MIX_TABLE = 1024   # entries of slk_image_batch_blend's quantile tables


def image_batch_blend(images, labels, idx, idx2, *, mean, std, cut_table=None, lam_table=None, prob=1.0, switch=0.5,
                      pad=0, flip=False, seed=0, epoch=0, x=None, y=None, err_flag=None):
    """image_batch with CutMix at any Beta(alpha, alpha) and / or MixUp (slk_image_batch_blend): `cut_table` (1024
    uint32 box-side fractions, as a torch.uint32 or int32 tensor of the same bits) and `lam_table` (1024 float32
    weights) are device tensors built by loss.mix_tables; at least one is needed. With both, a sample is CutMix with
    probability `switch`, else MixUp. y holds mixed labels; loss.mix_draws is the host twin. prob=0 is bitwise
    image_batch."""
    images, dims, mean, std, B, x, y = _image_front(images, labels, idx, mean, std, x, y)
    if cut_table is None and lam_table is None:
        raise ValueError("image_batch_blend: needs cut_table, lam_table or both")
    pi = _dev(images, "images", dtype=torch.uint8)
    tabs = []
    for t, name, dtypes in ((cut_table, "cut_table", (torch.int32, torch.uint32)), (lam_table, "lam_table", (_F32,))):
        if t is None:
            tabs.append(None)
            continue
        if isinstance(t, torch.Tensor) and t.dtype not in dtypes:
            raise TypeError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        tabs.append(_dev(t, name, (MIX_TABLE,), t.dtype if isinstance(t, torch.Tensor) else dtypes[0]))
        if t.device != images.device:
            raise ValueError(f"{name}: is on {t.device}, images on {images.device}")
    _lib.call("slk_image_batch_blend", pi, _dev(labels, "labels", dtype=torch.uint8), *dims,
              _dev(idx, "idx", (B,), torch.int64), _dev(idx2, "idx2", (B,), torch.int64), B, mean, std,
              *_image_tail(pad, flip, seed, epoch, x, y, err_flag, float(prob), tabs[0], tabs[1], float(switch)))
    return x, y


# ------------------------------------------------------------------------------------ widened head, soft targets
def wide_head_soft(cut, wf8, bf, labels, step, seed, keep_threshold, keep_scale, grad_scale, smoothing, logits,
                   loss_i, dlogits, dcut, slabs, work, err_flag=None, b0=0):
    """slk_wide_head on mixed labels with label smoothing (slk_wide_head_soft): every buffer is the caller's (the
    shapes of wide.WideServerStage.forward_backward). Returns (dcut, loss_i, slabs)."""
    B = int(cut.shape[0])
    _lib.call("slk_wide_head_soft", _dev(cut, "cut", dtype=torch.bfloat16), _dev(wf8, "wf8", (163840,)),
              _dev(bf, "fc.bias", (10,)), _labels(labels, B), _dev(step, "step", (1,), torch.int32),
              int(seed) & 0xFFFFFFFF, int(keep_threshold) & 0xFFFFFFFF, float(keep_scale), float(grad_scale),
              float(smoothing), _dev(logits, "logits", (B, 10)), _dev(loss_i, "loss_i", (B,)),
              _dev(dlogits, "dlogits", (B, 10)), _dev(dcut, "dcut", tuple(cut.shape), torch.bfloat16),
              _dev(slabs, "slabs"), _dev(work, "work"),
              _err_ptr(err_flag), int(b0), B, _stream(cut))
    return dcut, loss_i, slabs
