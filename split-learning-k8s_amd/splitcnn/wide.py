"""Widened split CNN — BASELINE.json config 5 ("K5"): 64-256 channels, synthetic 3x32x32 batches,
deeper cut, bf16 MFMA implicit-GEMM convolutions, with the north star's dropout and Adam.

The reference has no such model; this keeps its step contract
(src/client_part.py:110-138 <-> src/server_part.py:25-58: activations out, cut gradient back, loss
logged, one optimizer step per side per request) and its module style (src/model_def.py:5-71:
client/server halves + a full model + a role factory) for a network whose convolutions are real
contractions:

  WideModelPartA (client)  conv1 3->64 3x3 p1 + ReLU; conv2 64->128 + ReLU + maxpool2;
                           conv3 128->256 + ReLU + maxpool2  -> cut [B,256,8,8]
  WideModelPartB (server)  Dropout(0.25) -> flatten -> fc Linear(16384, 10); CrossEntropyLoss(mean)
  optimiser                torch.optim.Adam(lr=1e-3) on both sides

The cut is client-heavy by construction (99.9 % of the FLOPs are on the client side), so SplitFed
with N-1 client GPUs feeding one server GPU scales (SURVEY.md §7 "server-bound scaling").
Numerics (bf16 activations and conv operands, f32 accumulation, f32 masters/head/Adam) are stated in
oracle/wide_step.py, which the GPU parity tests hold this path to.

Every op runs on the gfx950 kernels of libslk.so (csrc/slk_wide.hip, csrc/slk_wide_head.hip);
there is no CPU path. Activations live in HBM in the C8 layout [B][C/8][H][W][8] (bf16);
`c8_to_nchw` gives the logical NCHW view.
"""
from __future__ import annotations

import os
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import ops
from .codec import Fp8Cut, MxCut, check_cut_codec
from .engine import TIMER, LossLog, _Buffers
from .graphs import GraphedTrainer
from .loss import LABEL_ERROR, SoftCrossEntropy, check_loss
from .ops import _dev, _stream
from .optim import EMA, Adam, ClipNorm, LRSchedule, check_clip, check_ema
from .privacy import CutNoise, check_cut_noise
from .recipe import Seg, StageRecipe, _flatten_params

P_DROP = 0.25
KEEP_THRESHOLD = int(round(P_DROP * 4294967296.0))          # keep iff hash >= p * 2^32
KEEP_SCALE = float(np.float32(1.0 / (1.0 - P_DROP)))        # f32(1/(1-p)), as torch's dropout
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
CLIENT_NPARAM = 370816   # [W1 1728 | b1 64 | W2 73728 | b2 128 | W3 294912 | b3 256]
SERVER_NPARAM = 163850   # [Wf 163840 | bf 10]
CUT_SHAPE = (32, 8, 8, 8)  # C8 layout of [256, 8, 8]
_BF = torch.bfloat16
_U8 = torch.uint8
_F32 = torch.float32


# ------------------------------------------------------------------------------------ modules
# The module contract of src/model_def.py:5-71 for the widened network: the halves are differentiable
# (autograd Functions over the same kernels the stages launch), so the reference's own step code runs
# on them — client: activations = model(x); activations.backward(grads); optimizer.step()
# (src/client_part.py:112-133); server: client_activations.requires_grad_(True); outputs =
# model(client_activations); loss = criterion(outputs, labels); loss.backward(); optimizer.step();
# return client_activations.grad (src/server_part.py:45-57). The cut is bf16 in logical NCHW
# [B,256,8,8] at this boundary (the kernels use C8 internally). The stages (WideClientStage /
# WideServerStage / WideTrainer) are the fused fast path over the same kernels.
class WideModelPartA(nn.Module):
    """Client bottom stack: conv1 3->64 + ReLU, conv2 64->128 + ReLU + pool, conv3 128->256 + ReLU +
    pool -> cut bf16 [B,256,8,8]."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3, 1, padding=1)
        self.conv2 = nn.Conv2d(64, 128, 3, 1, padding=1)
        self.conv3 = nn.Conv2d(128, 256, 3, 1, padding=1)
        self.relu = nn.ReLU()
        self.pool = nn.MaxPool2d(2)

    def forward(self, x):
        _require_cuda(x, "WideModelPartA")
        return _WideClientFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                   self.conv3.weight, self.conv3.bias)


class WideModelPartB(nn.Module):
    """Server top stack: Dropout(0.25) -> flatten -> Linear(16384, 10). In training mode each forward
    draws a fresh dropout mask (the hash of seed, forward count, sample, feature — the stages' mask
    at the same step); eval mode keeps every feature."""

    def __init__(self):
        super().__init__()
        self.dropout = nn.Dropout(P_DROP)
        self.flatten = nn.Flatten()
        self.fc = nn.Linear(256 * 8 * 8, 10)
        self.dropout_seed = 0
        self._drop_step = None   # device forward counter (not state: keeps the state_dict contract)

    def forward(self, x):
        _require_cuda(x, "WideModelPartB")
        if self._drop_step is None or self._drop_step.device != x.device:
            self._drop_step = torch.zeros(1, dtype=torch.int32, device=x.device)
        snap = self._drop_step.clone()
        thresh, scale = (KEEP_THRESHOLD, KEEP_SCALE) if self.training else (0, 1.0)
        logits = _WideHeadFn.apply(x, self.fc.weight, self.fc.bias, snap, self.dropout_seed, thresh, scale)
        if self.training:
            ops.tick(self._drop_step)
        return logits


class WideFullModel(nn.Module):
    """The unsplit widened network; parameter names = A ∪ B (like FullModel, src/model_def.py:31-46)."""

    def __init__(self):
        super().__init__()
        a, b = WideModelPartA(), WideModelPartB()
        self.conv1, self.conv2, self.conv3 = a.conv1, a.conv2, a.conv3
        self.dropout, self.fc = b.dropout, b.fc
        self._head = [b]   # shares fc / dropout; kept out of the module tree (state_dict keys)

    def forward(self, x):
        _require_cuda(x, "WideFullModel")
        cut = _WideClientFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                  self.conv3.weight, self.conv3.bias)
        head = self._head[0]
        head.train(self.training)
        return head(cut)


def get_wide_model(role="client"):
    """Role factory in the style of get_model (src/model_def.py:49-71)."""
    mode = os.getenv("LEARNING_MODE", "split").lower()
    if mode == "federated":
        return WideFullModel()
    if mode == "split":
        return WideModelPartA() if role == "client" else WideModelPartB()
    raise ValueError(f"Unknown LEARNING_MODE: {mode}. Use 'split' or 'federated'.")


def init_wide_models(seed: int = 0):
    """Seeded default init, client (conv1, conv2, conv3) then server (fc)."""
    torch.manual_seed(seed)
    return WideModelPartA(), WideModelPartB()


class SyntheticCIFAR:
    """CIFAR-shape synthetic batches: class prototypes + noise, normalised (mean 0.5, std 0.25);
    seeded CPU generator (bit-identical everywhere, like data.SyntheticMNIST)."""

    def __init__(self, seed: int = 42):
        self.gen = torch.Generator().manual_seed(seed)
        self.proto = torch.rand(10, 3, 32, 32, generator=self.gen)

    def batch(self, B: int):
        y = torch.randint(0, 10, (B,), generator=self.gen)
        x = (self.proto[y] + 0.3 * torch.randn(B, 3, 32, 32, generator=self.gen) - 0.5) / 0.25
        return x.contiguous(), y


def c8_to_nchw(t: torch.Tensor) -> torch.Tensor:
    """[B, C/8, H, W, 8] -> logical [B, C, H, W] (a permuted copy)."""
    B, C8, H, W, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(B, C8 * 8, H, W)


def nchw_to_c8(t: torch.Tensor) -> torch.Tensor:
    B, C, H, W = t.shape
    return t.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def _q(name, *args):
    return _lib.query(name, *args)


def _k(name, *args):
    """Launch slk_<name> under the (optional) HIP-event kernel timer."""
    with TIMER(name):
        _lib.call("slk_" + name, *args)


def _require_cuda(x, who):
    if x.device.type != "cuda":
        raise RuntimeError(f"splitcnn.{who}: input is on {x.device}; the widened model runs on the MI355X HIP "
                           "kernels only (move the module and its inputs to a ROCm device). There is no CPU fallback.")


def _f32p(t, name, n):
    """Device pointer of an f32 parameter (contiguous, n elements)."""
    _dev(t, name)
    if t.numel() != n:
        raise ValueError(f"{name}: expected {n} elements, got {t.numel()}")
    return t.data_ptr()


def new_shadows(device):
    return {"w1b": torch.empty(64 * 32, dtype=_BF, device=device), "w2f": torch.empty(73728, dtype=_BF, device=device),
            "w2d": torch.empty(73728, dtype=_BF, device=device), "w3f": torch.empty(294912, dtype=_BF, device=device),
            "w3d": torch.empty(294912, dtype=_BF, device=device)}


def build_shadows(W1, W2, W3, sh, stream):
    """bf16 MFMA layouts of the conv weights from their f32 masters (slk_wide_shadows)."""
    _k("wide_shadows", _f32p(W1, "conv1.weight", 1728), _f32p(W2, "conv2.weight", 73728),
       _f32p(W3, "conv3.weight", 294912), sh["w1b"].data_ptr(), sh["w2f"].data_ptr(), sh["w2d"].data_ptr(),
       sh["w3f"].data_ptr(), sh["w3d"].data_ptr(), stream)


def client_forward_kernels(x, sh, b1, b2, b3, a1, p2, code2, cut, code3, a1bits=None):
    """conv1 + ReLU -> conv2 + ReLU + pool -> conv3 + ReLU + pool (the cut), C8 bf16. a1bits ([B, 1024]
    int64): conv1 also writes the ReLU word of every pixel (bit c = a1[c] > 0), conv2's dgrad mask."""
    B = x.shape[0]
    _dev(x, "x", (B, 3, 32, 32))
    s = _stream(x)
    b1p, b2p, b3p = _f32p(b1, "conv1.bias", 64), _f32p(b2, "conv2.bias", 128), _f32p(b3, "conv3.bias", 256)
    bits = _dev(a1bits, "a1bits", (B, 1024), torch.int64) if a1bits is not None else None
    _k("wide_conv1_fwd", x.data_ptr(), sh["w1b"].data_ptr(), b1p, a1.data_ptr(), bits, B, s)
    _k("wide_conv2_fwd", a1.data_ptr(), sh["w2f"].data_ptr(), b2p, p2.data_ptr(), code2.data_ptr(), B, s)
    _k("wide_conv3_fwd", p2.data_ptr(), sh["w3f"].data_ptr(), b3p, cut.data_ptr(), code3.data_ptr(), B, s)


def client_backward_slab_shapes(B):
    return ((_q("slk_wide_conv1_wgrad_nslab", B), 1728 + 64), (_q("slk_wide_conv2_wgrad_nslab", B), 73728 + 128),
            (_q("slk_wide_conv3_wgrad_nslab", B), 294912 + 256))


def client_backward_kernels(dcut, saved, w2d, w3d, scratch, s1, s2, s3):
    """activations.backward(dcut) of the client stack into three slab sets [dW | db] (conv1, conv2,
    conv3). saved = (x, a1, p2, code2, code3[, a1bits]) of the forward; scratch = (dp2, da1m). No
    unpooled gradient is stored: conv3's kernels route the pooled dcut by code3 while staging it, conv3's
    dgrad writes dp2 (the gradient of p2, 16 x 16) and conv2's kernels route dp2 by code2 the same way.
    conv2's dgrad masks by a1 > 0 from a1's ReLU words (slk_wide_conv1_fwd writes them; computed from a1
    here when the forward did not)."""
    x, a1, p2, code2, code3 = saved[:5]
    dp2, da1m = scratch
    B = x.shape[0]
    s = _stream(dp2)
    _dev(dcut, "dcut", (B,) + CUT_SHAPE, _BF)
    if len(saved) > 5 and saved[5] is not None:
        _dev(saved[5], "a1bits", (B, 1024), torch.int64)
        a1bits = saved[5]
    else:
        a1bits = torch.empty((B, 1024), dtype=torch.int64, device=dp2.device)
        _k("wide_relu_bits", a1.data_ptr(), a1bits.data_ptr(), B, s)
    _k("wide_conv3_wgrad", dcut.data_ptr(), code3.data_ptr(), p2.data_ptr(), s3.data_ptr(), B, s)
    _k("wide_conv3_dgrad", dcut.data_ptr(), code3.data_ptr(), w3d.data_ptr(), dp2.data_ptr(), B, s)
    _k("wide_conv2_wgrad", dp2.data_ptr(), code2.data_ptr(), a1.data_ptr(), s2.data_ptr(), B, s)
    _k("wide_conv2_dgrad", dp2.data_ptr(), code2.data_ptr(), w2d.data_ptr(), a1bits.data_ptr(), da1m.data_ptr(), B, s)
    _k("wide_conv1_wgrad", x.data_ptr(), da1m.data_ptr(), s1.data_ptr(), B, s)


def client_backward_scratch(B, get):
    """(dp2, da1m) via get(name, shape, dtype)."""
    return get("dp2", (B, 16, 16, 16, 8), _BF), get("da1m", (B, 8, 32, 32, 8), _BF)


def _reduce(slabs):
    return ops.reduce_slabs(slabs)


class _WideClientFn(torch.autograd.Function):
    """cut = WideModelPartA(x) (bf16, logical NCHW); backward = the client stack's weight gradients."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, W3, b3):
        x = x.contiguous()
        B, dev = x.shape[0], x.device
        Ws = [t.detach().contiguous() for t in (W1, b1, W2, b2, W3, b3)]
        sh = new_shadows(dev)
        build_shadows(Ws[0], Ws[2], Ws[4], sh, _stream(x))
        a1 = torch.empty((B, 8, 32, 32, 8), dtype=_BF, device=dev)
        p2 = torch.empty((B, 16, 16, 16, 8), dtype=_BF, device=dev)
        code2 = torch.empty((B, 16, 16, 16, 8), dtype=_U8, device=dev)
        cut = torch.empty((B,) + CUT_SHAPE, dtype=_BF, device=dev)
        code3 = torch.empty((B,) + CUT_SHAPE, dtype=_U8, device=dev)
        a1bits = torch.empty((B, 1024), dtype=torch.int64, device=dev)
        client_forward_kernels(x, sh, Ws[1], Ws[3], Ws[5], a1, p2, code2, cut, code3, a1bits)
        ctx.save_for_backward(x, a1, p2, code2, code3, a1bits, sh["w2d"], sh["w3d"])
        return c8_to_nchw(cut)

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("splitcnn: gradient w.r.t. the client's input images is not part of the "
                                      "split step (src/client_part.py:110-114)")
        x, a1, p2, code2, code3, a1bits, w2d, w3d = ctx.saved_tensors
        B, dev = x.shape[0], x.device
        dcut = nchw_to_c8(g.to(_BF))
        scratch = client_backward_scratch(B, lambda n, sh_, dt: torch.empty(sh_, dtype=dt, device=dev))
        slabs = [torch.empty(sh_, dtype=_F32, device=dev) for sh_ in client_backward_slab_shapes(B)]
        client_backward_kernels(dcut, (x, a1, p2, code2, code3, a1bits), w2d, w3d, scratch, *slabs)
        g1, g2, g3 = (_reduce(sl) for sl in slabs)
        return (None, g1[:1728].view(64, 3, 3, 3), g1[1728:], g2[:73728].view(128, 64, 3, 3), g2[73728:],
                g3[:294912].view(256, 128, 3, 3), g3[294912:])


class _WideHeadFn(torch.autograd.Function):
    """logits = fc(dropout(flatten(cut))) — WideModelPartB.forward; backward gives the cut gradient
    (bf16, logical NCHW) and the fc weight gradient."""

    @staticmethod
    def forward(ctx, cut_nchw, Wf, bf, step, seed, thresh, scale):
        B, dev = cut_nchw.shape[0], cut_nchw.device
        if tuple(cut_nchw.shape[1:]) != (256, 8, 8):
            raise ValueError(f"cut: expected [B,256,8,8], got {tuple(cut_nchw.shape)}")
        cut = nchw_to_c8(cut_nchw.detach().to(_BF))
        Wf, bf = Wf.detach().contiguous(), bf.detach().contiguous()
        wf8 = torch.empty(163840, dtype=_F32, device=dev)
        s = _stream(cut)
        _k("wide_fc_shadow", _f32p(Wf, "fc.weight", 163840), wf8.data_ptr(), s)
        logits = torch.empty((B, 10), dtype=_F32, device=dev)
        _k("wide_head_fwd", cut.data_ptr(), wf8.data_ptr(), _f32p(bf, "fc.bias", 10), step.data_ptr(), int(seed),
           int(thresh), float(scale), logits.data_ptr(), 0, B, s)
        ctx.save_for_backward(cut, wf8, step)
        ctx.drop = (int(seed), int(thresh), float(scale))
        ctx.in_dtype = cut_nchw.dtype
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        cut, wf8, step = ctx.saved_tensors
        seed, thresh, scale = ctx.drop
        B, dev = cut.shape[0], cut.device
        dlogits = dlogits.to(_F32).contiguous()
        dcut = torch.empty_like(cut)
        slabs = torch.empty((_q("slk_wide_head_nslab", B), SERVER_NPARAM), dtype=_F32, device=dev)
        _k("wide_head_bwd", cut.data_ptr(), wf8.data_ptr(), _dev(dlogits, "dlogits", (B, 10)), step.data_ptr(), seed,
           thresh, scale, dcut.data_ptr(), slabs.data_ptr(), 0, B, _stream(dlogits))
        g = _reduce(slabs)
        return (c8_to_nchw(dcut).to(ctx.in_dtype), g[:163840].view(10, 16384), g[163840:], None, None, None, None)

# ------------------------------------------------------------------------------------ stages
class _AdamRecipe(StageRecipe):
    """The Adam family of a K5 stage (recipe.StageRecipe holds what it shares with K2). The default is
    torch.optim.Adam(lr, betas, eps) on slk_adam_*, which already keeps m, v and a counter: ema= leaves it in place
    and only a config, a schedule or clip= selects slk_adamw_* (weight decay, AdamW's or Adam's). The clipped step
    is slk_adamw_clip_multi, the layer-wise recipe optim.LAMB (slk_lamb_moments_multi then slk_lamb_multi, `trust_out`
    rows [w_norm, u_norm, ratio]). Every launch reports under its entry's name (TIMER)."""

    CONFIG, HYPER, STATE = Adam, ("lr", "betas", "eps"), ("m", "v")
    BY_VALUE_COUNTER = TICK_TIMER = True

    def _adamw(self, segments, write_grads=True, fuse=True):
        """One optimizer step on (lo, hi, slabs) slices of this stage (slabs [nslab, hi - lo]) or recipe.Seg
        segments: ONE launch (fuse) or one per slice; write_grads False: every slabs is the gradient block."""
        segs = [g if type(g) is Seg else self.seg(*g, write_grads=write_grads) for g in segments]
        self._step(segs, multi=fuse and len(segs) > 1)

    def _by_value(self, segs, loss, multi):
        hyper = (self.lr, *self.betas, self.eps, self.step_ctr)
        if multi:
            with TIMER("adam_multi_from_slabs"):
                ops.adam_multi_from_slabs(segs, *hyper)
        else:
            for g in segs:
                with TIMER("adam_from_slabs"):
                    ops.adam_from_slabs(*g, *hyper)

    def _plain(self, segs, loss, multi, kw):
        if multi:
            with TIMER("adamw_multi_from_slabs"):
                ops.adamw_multi_from_slabs(segs, **kw)
        else:
            for g in segs:
                with TIMER("adamw_from_slabs"):
                    ops.adamw_from_slabs(*g, **kw)

    def _clipped(self, groups, loss, kw):
        with TIMER("reduce_sqnorm_multi"):
            ops.reduce_sqnorm_multi(groups, loss=loss)
        with TIMER("adamw_clip_multi"):
            ops.adamw_clip_multi(groups, self.clip.value, **kw)

    def _layerwise(self, groups, loss, kw):
        lr_table = kw.pop("lr_table")
        with TIMER("lamb_moments_multi"):
            ops.lamb_moments_multi(groups, loss=loss, **kw)
        with TIMER("lamb_multi"):
            ops.lamb_multi(groups, lr_table, **kw)


class WideClientStage(_AdamRecipe):
    """Client half: forward(x) -> cut (bf16 C8); backward_step(dcut) = activations.backward(grads) +
    Adam (client_part.py:114,132-133 for the widened model)."""

    OFF = {"W1": 0, "b1": 1728, "W2": 1792, "b2": 75520, "W3": 75648, "b3": 370560}
    PAIRS = ((0, 1792, 1728), (1792, 75648, 73728), (75648, CLIENT_NPARAM, 294912))
    TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")

    def __init__(self, model: Optional[WideModelPartA] = None, device="cuda", lr=LR, betas=(BETA1, BETA2),
                 eps=EPS, optim: Optional[Adam] = None, schedule: Optional[LRSchedule] = None,
                 clip: Optional[ClipNorm] = None, ema: Optional[EMA] = None):
        self.device = torch.device(device)
        self.model = (model if model is not None else WideModelPartA()).to(self.device)
        m = self.model
        self.params, self.grads = _flatten_params([m.conv1.weight, m.conv1.bias, m.conv2.weight, m.conv2.bias,
                                                   m.conv3.weight, m.conv3.bias], self.device)
        assert self.params.numel() == CLIENT_NPARAM
        self.lr, self.betas, self.eps = lr, betas, eps
        self._init_optim(optim, schedule, clip, ema)
        self.fuse_adam = True  # step_from_slabs: the three Adam segments in one launch
        self.sh = new_shadows(self.device)   # bf16 conv weight shadows (slk_wide_shadows layouts)
        # a second set for the averaged weights, rebuilt from them inside every evaluation pass that reads it
        self.sh_ema = new_shadows(self.device) if self.ema is not None else None
        self._buf = _Buffers()
        self._saved = {}
        self.refresh_shadows()

    def _b(self, name, shape, dtype):
        return self._buf.get(name, shape, dtype, self.device)

    def _p(self, k, n):
        o = self.OFF[k]
        return self.params[o:o + n]

    def refresh_shadows(self):
        """Rebuild the bf16 conv weight shadows from the f32 masters (after load_state_dict or Adam)."""
        build_shadows(self._p("W1", 1728), self._p("W2", 73728), self._p("W3", 294912), self.sh, _stream(self.params))

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, tag="", ema: bool = False) -> torch.Tensor:
        """cut = client forward of x; `tag` keeps separate saved tensors per micro-batch. `ema` (evaluation only):
        the averaged weights — their bf16 shadows are rebuilt from the averaged block first (slk_wide_shadows, part
        of the pass and of its graph, so they are always current) and the biases are the block's own."""
        B = x.shape[0]
        if ema:
            if self.ema is None:
                raise RuntimeError("WideClientStage: weights='ema' needs a stage built with ema= (optim.EMA)")
            e, o = self.ema, self.OFF
            build_shadows(e[o["W1"]:o["b1"]], e[o["W2"]:o["b2"]], e[o["W3"]:o["b3"]], self.sh_ema, _stream(e))
            sh, (b1, b2, b3) = self.sh_ema, (e[o["b1"]:o["W2"]], e[o["b2"]:o["W3"]], e[o["b3"]:])
        else:
            sh, (b1, b2, b3) = self.sh, (self._p("b1", 64), self._p("b2", 128), self._p("b3", 256))
        _dev(x, "x", (B, 3, 32, 32))
        a1 = self._b(f"a1{tag}", (B, 8, 32, 32, 8), _BF)
        p2 = self._b(f"p2{tag}", (B, 16, 16, 16, 8), _BF)
        code2 = self._b(f"code2{tag}", (B, 16, 16, 16, 8), _U8)
        cut = out if out is not None else self._b(f"cut{tag}", (B,) + CUT_SHAPE, _BF)
        _dev(cut, "cut", (B,) + CUT_SHAPE, _BF)
        code3 = self._b(f"code3{tag}", (B,) + CUT_SHAPE, _U8)
        a1bits = self._b(f"a1bits{tag}", (B, 1024), torch.int64)
        client_forward_kernels(x, sh, b1, b2, b3, a1, p2, code2, cut, code3, a1bits)
        self._x, self._a1, self._p2, self._code2, self._code3 = x, a1, p2, code2, code3
        self._saved[tag] = (x, a1, p2, code2, code3, a1bits)
        return cut

    def backward_slabs(self, dcut: torch.Tensor, tag=""):
        """Client backward into three slab sets (conv1, conv2, conv3); returns them."""
        B = self._saved[tag][0].shape[0]
        self._x, self._a1, self._p2, self._code2, self._code3 = self._saved[tag][:5]
        scratch = client_backward_scratch(B, self._b)
        s1, s2, s3 = (self._b(n, shp, _F32) for n, shp in zip(("s1", "s2", "s3"), client_backward_slab_shapes(B)))
        client_backward_kernels(dcut, self._saved[tag], self.sh["w2d"], self.sh["w3d"], scratch, s1, s2, s3)
        self._dp2, self._da1m = scratch
        return s1, s2, s3

    def _slab_segments(self, s1, s2, s3):
        """The three slab sets, [conv1 | conv2 | conv3], as (lo, hi, slabs) slices: the stage's PAIRS."""
        return [(lo, hi, sl) for (lo, hi, _), sl in zip(self.PAIRS, (s1, s2, s3))]

    def step_from_slabs(self, s1, s2, s3):
        """Adam on all client parameters from the three slab sets (ONE launch, bit-identical to one
        slk_adam_from_slabs per set; fuse_adam False: one per set), then shadows + step counter."""
        self._adamw(self._slab_segments(s1, s2, s3), fuse=self.fuse_adam)
        self.refresh_shadows()
        self._tick()

    def backward_step(self, dcut: torch.Tensor):
        self.step_from_slabs(*self.backward_slabs(dcut))

    # --- multi-GPU (dist.WideHub): gradient into self.grads, all-reduced by the caller, then Adam
    cut_dtype = _BF

    @staticmethod
    def cut_shape(B: int):
        return (B,) + CUT_SHAPE

    def backward_grads(self, dcut: torch.Tensor, tag="", accumulate: bool = False):
        """activations.backward(grads) into the flat gradient block (fixed-order slab reduction);
        accumulate=True adds (micro-batches of one step)."""
        for lo, hi, sl in self._slab_segments(*self.backward_slabs(dcut, tag)):
            with TIMER("reduce_slabs"):
                ops.reduce_slabs(sl, out=self.grads[lo:hi], accumulate=accumulate)

    def step_from_grads(self):
        """Adam from self.grads (e.g. after an all-reduce over the client ranks)."""
        self._adamw([self.grads_segment()])
        self.refresh_shadows()
        self._tick()


class WideServerStage(_AdamRecipe):
    """Server half: step_request(cut, labels, step) -> (dcut, loss_i): dropout + fc + CE forward and
    backward, Adam, loss logged to the device ring (server_part.py:38-58 for the widened model)."""

    PAIRS = ((0, SERVER_NPARAM, 163840),)
    TENSORS = ("fc.weight", "fc.bias")

    def __init__(self, model: Optional[WideModelPartB] = None, device="cuda", lr=LR, betas=(BETA1, BETA2),
                 eps=EPS, seed: int = 0, loss_log: Optional[LossLog] = None, optim: Optional[Adam] = None,
                 schedule: Optional[LRSchedule] = None, clip: Optional[ClipNorm] = None,
                 loss: Optional[SoftCrossEntropy] = None, ema: Optional[EMA] = None):
        self.device = torch.device(device)
        # loss=SoftCrossEntropy(eps): the head is slk_wide_head_soft (mixed labels + label smoothing, splitcnn.loss);
        # eps is a constructor constant passed by value, so a captured graph keeps it (no setter)
        self.loss = check_loss(loss)
        self.model = (model if model is not None else WideModelPartB()).to(self.device)
        self.params, self.grads = _flatten_params([self.model.fc.weight, self.model.fc.bias], self.device)
        assert self.params.numel() == SERVER_NPARAM
        self.lr, self.betas, self.eps, self.seed = lr, betas, eps, int(seed)
        self._init_optim(optim, schedule, clip, ema)
        self.wf8 = torch.empty(163840, dtype=_F32, device=self.device)
        # the averaged fc weight in the cut's order, rebuilt inside every evaluation pass that reads it
        self.wf8_ema = torch.empty_like(self.wf8) if self.ema is not None else None
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.eval_err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)  # evaluate()'s own flag
        self.eval_logits = None   # the logits of the last evaluate() (a stage buffer)
        self.loss_log = loss_log if loss_log is not None else LossLog(self.device)
        self._buf = _Buffers()
        self.refresh_shadows()

    def _b(self, name, shape, dtype):
        return self._buf.get(name, shape, dtype, self.device)

    def refresh_shadows(self):
        _k("wide_fc_shadow", self.params.data_ptr(), self.wf8.data_ptr(), _stream(self.params))

    def evaluate(self, cut, labels=None, metrics=None, ema: bool = False):
        """Forward only, as WideModelPartB.eval() runs it: slk_wide_head_fwd with every feature kept
        (keep_threshold 0, keep_scale 1), then loss_i / pred from the logits (slk_eval_logits) and, with
        `metrics` (metrics.EvalMetrics), the device accumulator. Returns (pred, loss_i); labels=None predicts
        only (loss_i is None). Own `eval_` buffers and eval_err_flag; step_ctr is read (the dropout hash input,
        unused at threshold 0) and never ticked; parameters, Adam state and the loss log are not touched. `ema`:
        the head reads the averaged block — wf8_ema is rebuilt from it first (slk_wide_fc_shadow, part of the pass
        and of its graph) and the bias is the block's own; the block is not written."""
        B = cut.shape[0]
        _dev(cut, "cut", (B,) + CUT_SHAPE, _BF)
        logits = self._b("eval_logits", (B, 10), _F32)
        wf8, flat = self.wf8, self.params
        if ema:
            if self.ema is None:
                raise RuntimeError("WideServerStage: weights='ema' needs a stage built with ema= (optim.EMA)")
            wf8, flat = self.wf8_ema, self.ema
            _k("wide_fc_shadow", flat.data_ptr(), wf8.data_ptr(), _stream(cut))
        _k("wide_head_fwd", cut.data_ptr(), wf8.data_ptr(), flat[163840:].data_ptr(),
           self.step_ctr.data_ptr(), self.seed, 0, 1.0, logits.data_ptr(), 0, B, _stream(cut))
        with TIMER("eval_logits"):
            loss_i, pred = ops.eval_logits(logits, labels,
                                           loss_i=self._b("eval_loss_i", (B,), _F32) if labels is not None else None,
                                           pred=self._b("eval_pred", (B,), torch.int64), err_flag=self.eval_err_flag)
        self.eval_logits = logits
        if metrics is not None:
            if labels is None:
                raise ValueError("metrics need labels")
            with TIMER("eval_accumulate"):
                metrics.update(loss_i, pred, labels)
        return pred, loss_i

    def forward_backward(self, cut, labels, grad_scale, dcut=None, b0: int = 0):
        B = cut.shape[0]
        _dev(cut, "cut", (B,) + CUT_SHAPE, _BF)
        _dev(labels, "labels", (B,), torch.int64)
        s = _stream(cut)
        logits = self._b("logits", (B, 10), _F32)
        loss_i = self._b("loss_i", (B,), _F32)
        dlogits = self._b("dlogits", (B, 10), _F32)
        dcut = dcut if dcut is not None else self._b("dcut", (B,) + CUT_SHAPE, _BF)
        _dev(dcut, "dcut", (B,) + CUT_SHAPE, _BF)
        sf = self._b("sf", (_q("slk_wide_head_nslab", B), SERVER_NPARAM), _F32)
        work = self._b("work", (_q("slk_wide_head_work", B),), _F32)
        if self.loss is None:
            _k("wide_head", cut.data_ptr(), self.wf8.data_ptr(), self.params[163840:].data_ptr(),
               labels.data_ptr(), self.step_ctr.data_ptr(), self.seed, KEEP_THRESHOLD, KEEP_SCALE,
               float(grad_scale), logits.data_ptr(), loss_i.data_ptr(), dlogits.data_ptr(), dcut.data_ptr(),
               sf.data_ptr(), work.data_ptr(), self.err_flag.data_ptr(), int(b0), B, s)
        else:
            with TIMER("wide_head"):
                ops.wide_head_soft(cut, self.wf8, self.params[163840:], labels, self.step_ctr, self.seed,
                                   KEEP_THRESHOLD, KEEP_SCALE, grad_scale, self.loss.label_smoothing, logits, loss_i,
                                   dlogits, dcut, sf, work, err_flag=self.err_flag, b0=b0)
        self._logits, self._dlogits = logits, dlogits
        return dcut, loss_i, sf

    def step_from_slabs(self, sf):
        self._adamw([(0, SERVER_NPARAM, sf)])
        self.refresh_shadows()
        self._tick()

    def _log(self, values, scale, step):
        with TIMER("loss_log"):
            ops.loss_log(values, scale, self.loss_log.ring, self.loss_log.counter)
        if step is not None:
            self.loss_log.note_step(step)

    def log_loss(self, loss_i, step=None):
        self._log(loss_i, 1.0 / loss_i.numel(), step)

    def step_request(self, cut, labels, step=None, dcut=None):
        """One /forward_pass for the widened model: returns (dcut, loss_i)."""
        B = cut.shape[0]
        dcut, loss_i, sf = self.forward_backward(cut, labels, 1.0 / B, dcut=dcut)
        self.log_loss(loss_i)
        self.step_from_slabs(sf)
        if step is not None:
            self.loss_log.note_step(step)
        return dcut, loss_i

    def check_labels(self):
        """Raise if any label seen so far was outside [0, 10) or, with loss=, any target was malformed."""
        if int(self.err_flag.item()) != 0:
            raise IndexError(LABEL_ERROR)

    # --- micro-batched / multi-client steps (dist.WideHub): accumulate, then one Adam step
    def accumulate(self, cut, labels, grad_scale: float, b0: int, k: int, nparts: int, dcut=None):
        """Head forward/backward for samples b0 .. b0+len(cut)-1 of the step's global batch (mean-loss
        scale grad_scale = 1/global batch); the fc gradient adds into self.grads (k = 0 starts it) and
        this part's loss sum lands in loss part k of nparts. Returns dcut."""
        dcut, loss_i, sf = self.forward_backward(cut, labels, grad_scale, dcut=dcut, b0=b0)
        with TIMER("reduce_slabs"):
            ops.reduce_slabs(sf, out=self.grads, accumulate=k > 0)
        ops.loss_sum(loss_i, grad_scale, out=self._b("loss_parts", (nparts,), _F32)[k:k + 1])
        return dcut

    def finish_step(self, nparts: int, step=None):
        """Adam from the accumulated gradient, loss logged (sum of the parts), step counter ticked."""
        self._adamw([self.grads_segment()])
        self.refresh_shadows()
        self._log(self._b("loss_parts", (nparts,), _F32), 1.0, step)
        self._tick()


class WideTrainer(GraphedTrainer):
    """Both widened stages fused on one GPU, the whole step captured as one HIP graph (like
    engine.SplitTrainer, on graphs.GraphedTrainer): client fwd -> server dropout/fc/CE/bwd/Adam -> client
    bwd/Adam.

    `optim` (optim.Adam) and `schedule` (optim.LRSchedule) replace Adam(lr=1e-3): both stages share the
    config and the schedule's device table, each indexing it with its own step counter (the server's also
    seeds the dropout mask), so the captured graph follows the schedule. Without them `lr` is a by-value
    kernel argument that a captured graph keeps (use a schedule and LRSchedule.set_lr to change it). `clip`
    (optim.ClipNorm, shared by both stages) clips each stage's gradient by that stage's own global norm before
    its Adam update; grad_norms() reads the last step's norms. An optim.LAMB config scales every tensor's step by
    its trust ratio (two launches per stage step like clipping, not combined with `clip`); trust_ratios() reads the
    last step's norms and ratios. `loss` (loss.SoftCrossEntropy) makes the head take
    mixed labels (loss.CutMix in the loader) with label smoothing, a by-value constant a captured graph keeps (no
    setter); evaluation stays the plain cross-entropy on plain labels. `ema` (optim.EMA, shared by both stages)
    keeps an exponential moving average of both parameter blocks: each stage launches slk_ema_multi before its own
    tick, inside the captured graph; evaluate / eval_batch / predict(weights="ema") run on it (bf16 shadows rebuilt
    from it inside the pass) and ema_state_dict() reads it. Its `warmup` and `start` are by-value constants a
    captured graph keeps (no setter); EMA.set_decay reaches a captured graph. `cut_codec` (codec.Fp8Cut) puts the
    arithmetic of the FP8 exchange (dist.WideHub(codec=...)) inside the step: the head reads
    roundtrip(cut, fwd) from a server-stage buffer and the client back-propagates roundtrip(dcut, bwd) — straight
    through, exactly what the wire does — two slk_cut8_roundtrip launches inside the captured graph (one per
    direction that is not None). evaluate / eval_batch / predict quantise the cut the same way, on the live and on
    the averaged weights: that is what a deployed server receives. The formats are by-value constants a captured
    graph keeps (no setter); cut_codec=None launches nothing new. A direction the codec rounds stochastically
    (Fp8Cut(rounding=...)) launches slk_cut8_roundtrip_sr with row0 = 0 and a stage counter the graph follows: the
    cut under the client's step_ctr, the cut gradient under the server's, each read before its stage's tick (the
    gradient is rounded between the head and the server's Adam), so load_optimizer_state reproduces the bits and
    the step stays dist.WideHub(codec=...)'s. Evaluation and prediction round the cut to nearest whatever the
    training rounding is: they stay a pure function of the weights, bitwise those of Fp8Cut(fwd, bwd). A codec.MxCut
    in the same place runs the block-scaled exchange (include/slk.h, "MX cut records") the same way: two
    slk_cutmx_roundtrip launches at the same two places, always to nearest, evaluation and prediction included.

    `cut_noise` (privacy.CutNoise) puts a noise defence on the cut, inside the captured step: the cut is clipped per
    sample and noised (slk_cut_noise) into the server-stage buffer `cut_n` under the client's step_ctr with row0 = 0,
    read before the client's tick — then the FP8 forward direction if there is a codec, then the head. Backward: the
    head's dcut, the FP8 backward direction if any, then — only with a clip — slk_cut_scale_rows in place (the
    coefficient held constant: straight through), then the client's backward. A replay follows the counter, so
    load_optimizer_state reproduces the bits; CutNoise.set_scale / set_clip reach a captured graph, its kind, seed,
    table and tail are by-value constants it keeps. evaluate / eval_batch / predict apply the clip and NO noise, on
    the live and on the averaged weights: evaluation stays a pure function of the weights (noisy inference is the
    user's own CutNoise.apply call). cut_stats() reads the last step's (norm, coef) per sample. cut_noise=None
    launches nothing new."""

    input_shape = (3, 32, 32)

    def __init__(self, client: Optional[WideModelPartA] = None, server: Optional[WideModelPartB] = None,
                 device="cuda", graph: bool = True, seed: int = 0, optim: Optional[Adam] = None,
                 schedule: Optional[LRSchedule] = None, clip: Optional[ClipNorm] = None,
                 loss: Optional[SoftCrossEntropy] = None, ema: Optional[EMA] = None,
                 cut_codec: Union[Fp8Cut, MxCut, None] = None, cut_noise: Optional[CutNoise] = None):
        check_clip(clip)
        check_ema(ema)
        self.cut_codec = check_cut_codec(cut_codec)
        self.cut_noise = check_cut_noise(cut_noise)
        super().__init__(device, graph)
        if self.cut_noise is not None:
            self.cut_noise.to(self.device)
        self._cut_stats_B = None
        self.client = WideClientStage(client, self.device, optim=optim, schedule=schedule, clip=clip, ema=ema)
        self.server = WideServerStage(server, self.device, seed=seed, optim=self.client.optim,
                                      schedule=self.client.schedule, clip=self.client.clip, loss=loss,
                                      ema=self.client.ema_cfg)

    def _wire(self, t, direction, name, step=None):
        """What the other side of an FP8 exchange receives for t: roundtrip(t) in `direction`'s format, in the
        server stage's buffer `name` (fwd) or in place (bwd: the server's own dcut buffer); t itself without a
        codec or where the direction is dense. `step` is the stage counter a stochastic direction is keyed on
        (row0 = 0: t is the whole batch); without it — evaluation — the rounding is to nearest."""
        q = self.cut_codec
        if q is None or q.format(direction) is None:
            return t
        if step is None:
            q = q.nearest()
        out = self.server._b(name, tuple(t.shape), _BF) if name is not None else t
        with TIMER("cutmx_roundtrip" if isinstance(q, MxCut) else "cut8_roundtrip"):
            if q.rounding_of(direction) == "stochastic":
                return q.roundtrip(t, out, direction, step=step)
            return q.roundtrip(t, out, direction)   # today's call, argument for argument

    def _noised(self, cut, name, step=None):
        """The cut the defence lets out: clip + noise of `cut` in the server stage's buffer `name`, the (norm, coef)
        pairs in `name`_stats; cut itself without a defence. `step` is the stage counter the draws are keyed on
        (row0 = 0: cut is the whole batch); without it — evaluation — only the clip runs (and nothing without one)."""
        n = self.cut_noise
        if n is None or (step is None and n.clip_value is None):
            return cut
        out = self.server._b(name, tuple(cut.shape), _BF)
        stats = self.server._b(name + "_stats", (cut.shape[0], 2), _F32) if n.clip_value is not None else None
        with TIMER("cut_noise"):
            return n.apply(cut, out, step=step, stats=stats, noise=step is not None)

    def _unclipped(self, dcut):
        """The gradient of the clip with its coefficient held constant: dcut scaled in place by the forward's
        per-sample coefficient; dcut itself without a clip."""
        n = self.cut_noise
        if n is None or n.clip_value is None:
            return dcut
        with TIMER("cut_scale_rows"):
            return n.scale_rows(dcut, self.server._b("cut_n_stats", (dcut.shape[0], 2), _F32), dcut)

    def cut_stats(self) -> torch.Tensor:
        """f32 [B, 2] on the host: (norm, coef) of every sample of the last training step's cut — its L2 norm before
        the clip and the coefficient applied (1.0: not clipped). One host sync. Needs cut_noise= with a clip
        (CutNoise(clip=float("inf")) measures without clipping)."""
        n = self.cut_noise
        if n is None or n.clip_value is None:
            raise RuntimeError("cut_stats: the trainer was built without cut_noise= or its CutNoise has clip=None")
        if self._cut_stats_B is None:
            raise RuntimeError("cut_stats: no training step has run yet")
        return self.server._b("cut_n_stats", (self._cut_stats_B, 2), _F32).cpu()

    def step(self, x, y):
        self._cut_stats_B = int(x.shape[0])   # which of the per-batch-size stats buffers the last step wrote
        super().step(x, y)

    def _eager(self, x, y):
        c, s, q = self.client, self.server, self.cut_codec
        cut = self._noised(c.forward(x), "cut_n", c.step_ctr)
        cut = self._wire(cut, "fwd", "cut_q", c.step_ctr)
        if q is not None and q.format("bwd") is not None and q.rounding_of("bwd") == "stochastic":
            # step_request with the gradient rounded before the server's tick: its words are this step's
            dcut, loss_i, sf = s.forward_backward(cut, y, 1.0 / cut.shape[0])
            dcut = self._wire(dcut, "bwd", None, s.step_ctr)
            s.log_loss(loss_i)
            s.step_from_slabs(sf)
        else:
            dcut = self._wire(s.step_request(cut, y)[0], "bwd", None, s.step_ctr)
        c.backward_step(self._unclipped(dcut))

    def _state(self):
        c, s = self.client, self.server
        return ([c.params, c.m, c.v, c.step_ctr, s.params, s.m, s.v, s.step_ctr, s.loss_log.counter] +
                [st.ema for st in (c, s) if st.ema is not None])

    def _optim_state(self):
        """Adam's m / v and the step counters of both stages, by name; with ema= the averaged blocks."""
        keys = (("exp_avg", "m"), ("exp_avg_sq", "v"), ("step", "step_ctr"))
        return {f"{n}.{k}": getattr(st, a) for n, st in (("client", self.client), ("server", self.server))
                for k, a in keys + ((("ema", "ema"),) if st.ema is not None else ())}

    def _state_written(self):
        """The bf16 / C8 weight shadows follow the f32 masters."""
        self.client.refresh_shadows()
        self.server.refresh_shadows()

    # ---- evaluation / prediction: no dropout, no tick: both step counters, the parameters, Adam's m / v
    # and the shadows are as before (the cut of the last evaluation is in eval_cut)
    def _eval_eager(self, x, y, metrics=None, weights="live"):
        ema = self._check_weights(weights)
        # the client forward under its own tag: the saved tensors of a training forward (tag "") survive
        self.eval_cut = self.client.forward(x, tag="eval", ema=ema)   # the last evaluation's cut (a stage buffer)
        cut = self._wire(self._noised(self.eval_cut, "eval_cut_n"), "fwd", "eval_cut_q")
        return self.server.evaluate(cut, y, metrics=metrics, ema=ema)

    def predict(self, x, return_logits: bool = False, weights: str = "live"):
        """pred = argmax of the logits of x (int64 [B]); with return_logits also the f32 [B, 10] logits.
        weights="ema": on the averaged weights (optim.EMA)."""
        pred, _ = self._eval_eager(x, None, weights=weights)
        return (pred.clone(), self.server.eval_logits.clone()) if return_logits else pred.clone()
