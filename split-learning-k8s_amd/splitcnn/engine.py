"""The split-CNN step engine: client stage, server stage and the 1-GPU fused trainer.

This is the MI355X-native form of the reference's step contract (src/client_part.py:110-138 <->
src/server_part.py:25-58):

    client:  zero_grad; act = model(x)                         (client_part.py:112-114)
             send {act.detach(), labels, step}                 (client_part.py:117-125)
    server:  act.requires_grad_(True); zero_grad; fwd; CE loss; backward; SGD step;
             log loss at step; return act.grad                 (server_part.py:45-58)
    client:  act.backward(cut_grad); SGD step; step += 1      (client_part.py:131-138)

API: ``ClientStage.forward(x) -> act``, ``ServerStage.step(act, labels, step) ->
(cut_grad, loss)``, ``ClientStage.backward_step(cut_grad)``. Each stage keeps its parameters in ONE
flat device block (the module's Parameters become views of it, so state_dict / load_state_dict keep
working) and its gradients in another; the weight-gradient slabs of the wgrad kernels are reduced in
fixed order inside the fused SGD launch. Nothing synchronises with the host: the loss goes to a
device ring (LossLog) flushed every N steps, replacing the per-step mlflow.log_metric REST call
(server_part.py:55). `SplitTrainer` runs both stages on one GPU and captures the whole step in a
HIP graph.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from . import ops
from .graphs import GraphedTrainer
from .loss import LABEL_ERROR, SoftCrossEntropy, check_loss
from .model_def import ModelPartA, ModelPartB
from .optim import EMA, SGD, ClipNorm, LRSchedule, check_clip, check_ema
from .recipe import TIMER, Seg, StageRecipe, _flatten_params, ema_update   # TIMER: bench.py and the tools take it from here

LR = 0.01  # optim.SGD(lr=0.01) on both sides (client_part.py:17, server_part.py:15)


class _SgdRecipe(StageRecipe):
    """The SGD family of a K2 stage (recipe.StageRecipe holds what it shares with K5). The default is the
    reference's optim.SGD(lr) on slk_sgd_*, without state or a counter, so whatever needs the counter (a schedule,
    clip=, ema=) selects slk_sgdm_* with the momentum buffers `buf`. The clipped step is slk_sgdm_clip_multi, the
    layer-wise recipe optim.LARS (slk_reduce_tnorm_multi then slk_lars_multi). The callers time the stage's whole
    update (TIMER sgd_client / sgd_server), so nothing here does."""

    CONFIG, STATE = SGD, ("buf",)

    def _sgdm(self, segments, loss=None, multi=False):
        """One optimizer step on recipe.Seg segments ((lo, hi, slabs) slices of this stage are taken too): separate
        launches, or ONE with the loss log (multi); another stage's optim_segment joins them."""
        self._step([g if type(g) is Seg else self.seg(*g) for g in segments], loss, multi)

    def _by_value(self, segs, loss, multi):
        if multi:
            ops.sgd_multi_from_slabs(segs, self.lr, loss=loss)
        else:
            for g in segs:
                ops.sgd_from_slabs(*g, self.lr)

    def _plain(self, segs, loss, multi, kw):
        if multi:
            ops.sgdm_multi_from_slabs(segs, loss=loss, **kw)
        else:
            for g in segs:
                ops.sgdm_from_slabs(*g, **kw)

    def _clipped(self, groups, loss, kw):
        ops.reduce_sqnorm_multi(groups, loss=loss)
        ops.sgdm_clip_multi(groups, self.clip.value, **kw)

    def _layerwise(self, groups, loss, kw):
        ops.reduce_tnorm_multi(groups, loss=loss)
        ops.lars_multi(groups, **kw)


class _Buffers:
    """Per-batch-size scratch owned by a stage (allocated once, reused every step).

    Keyed by (name, shape, dtype, device): a buffer is never replaced, so a HIP graph captured at one
    batch size keeps valid pointers after another size has run (a ragged loader alternates 64 / 32)."""

    def __init__(self):
        self._b = {}

    def get(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype, torch.device(device))
        t = self._b.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=device)
            self._b[key] = t
        return t


class LossLog:
    """Device-side loss log: one ring slot per server step, written by slk_loss_log (the device
    counter advances inside the kernel, so graph replays log too). `flush()` copies the ring to the
    host once and returns/sinks [(step, loss)] — the replacement of mlflow.log_metric("loss", ...,
    step=step) (src/server_part.py:55)."""

    def __init__(self, device, capacity: int = 4096, sink: Optional[Callable[[int, float], None]] = None):
        self.device = torch.device(device)
        self.capacity = capacity
        self.ring = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.sink = sink
        self._flushed = 0            # number of entries already flushed
        self._steps: List[int] = []  # host-side step ids, in logging order (no device sync needed)
        self.history: List[Tuple[int, float]] = []

    def note_step(self, step: int):
        self._steps.append(int(step))

    def flush(self) -> List[Tuple[int, float]]:
        count = int(self.counter.item())
        new = count - self._flushed
        if new <= 0:
            return []
        if new > self.capacity:
            raise RuntimeError(f"LossLog overflow: {new} unflushed steps > capacity {self.capacity}")
        ring = self.ring.cpu()
        out = []
        for i in range(self._flushed, count):
            step = self._steps[i] if i < len(self._steps) else i
            loss = float(ring[i % self.capacity])
            out.append((step, loss))
            if self.sink is not None:
                self.sink(step, loss)
        self._flushed = count
        self.history.extend(out)
        if self.sink is not None and hasattr(self.sink, "flush"):
            self.sink.flush()  # batching sinks (splitcnn.sinks) send once per flush
        return out


# conv2 implementations per op (forward+pool, dgrad, wgrad): "f32" = the Winograd F(2x2,3x3) kernels
# on the f32 MFMA; "x3" = the f16-MFMA kernels with hi/lo-split f32 operands (csrc/slk_x3.hip) where
# are used for all three ("x3"), or for forward + dgrad with the Winograd wgrad ("x3w").
CONV_PRESETS = {"f32": ("wino", "wino", "wino"), "x3": ("x3", "x3", "x3"), "x3w": ("x3", "x3", "wino")}
CONV_DEFAULT = "x3"


class ClientStage(_SgdRecipe):
    """Client half: ModelPartA on one device + SGD (src/client_part.py:16-17,112-133).

    forward(x) -> act; then either backward_step(cut_grad) (fused wgrad-slab reduce + SGD, the
    reference's `activations.backward(grads); optimizer.step()`), or backward(cut_grad,
    accumulate=...) into the flat gradient block followed by step() (micro-batched / all-reduced
    topologies)."""

    PAIRS = ((0, ops.CLIENT_NPARAM, 288),)
    TENSORS = ("conv1.weight", "conv1.bias")

    def __init__(self, model: Optional[ModelPartA] = None, lr: float = LR, device="cuda",
                 optim: Optional[SGD] = None, schedule: Optional[LRSchedule] = None,
                 clip: Optional[ClipNorm] = None, ema: Optional[EMA] = None):
        self.device = torch.device(device)
        self.model = (model if model is not None else ModelPartA()).to(self.device)
        self.lr = lr
        self.params, self.grads = _flatten_params(
            [self.model.conv1.weight, self.model.conv1.bias], self.device)
        self._init_optim(optim, schedule, clip, ema)
        self._buf = _Buffers()
        self._x = None
        self._act = None
        self._act_amax = None
        self._act16 = None
        self._relu_bits = None
        self.emit_amax = False  # forward also writes the per-sample max of act (x3 server kernels)
        # forward writes the x3 server operand (act16 images + act_amax) instead of the f32 act: the
        # fused single-GPU step, where the cut never leaves the device (forward then returns None)
        self.emit_act16 = False

    @property
    def W1(self):
        return self.model.conv1.weight

    @property
    def b1(self):
        return self.model.conv1.bias

    def bind_grads(self, view: torch.Tensor):
        """Use `view` (320 floats, e.g. a slice of an all-reduce bucket) as the gradient block."""
        view.copy_(self.grads)
        self.grads = view
        self.model.conv1.weight.grad = view[:288].view(32, 1, 3, 3)
        self.model.conv1.bias.grad = view[288:].view(32)

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """act = relu(conv1(x)) (client_part.py:114). Keeps x/act for the backward."""
        B = x.shape[0]
        if self.emit_act16:
            amax = self._buf.get("act_amax", (B,), torch.float32, self.device)
            a16 = self._buf.get("act16", (ops.conv2_act16_bytes(B),), torch.uint8, self.device)
            bits = self._buf.get("relu_bits", (B, ops.RELU_BITS_WORDS), torch.int32, self.device)
            with TIMER("conv1_fwd"):
                act = ops.conv1_fwd_x3(x, self.W1.detach(), self.b1.detach(), amax, a16, act=out, relu_bits=bits)
            self._x, self._act, self._act_amax, self._act16, self._relu_bits = x, act, amax, a16, bits
            return act
        act = out if out is not None else self._buf.get("act", (B, 32, 26, 26), torch.float32, self.device)
        amax = self._buf.get("act_amax", (B,), torch.float32, self.device) if self.emit_amax else None
        with TIMER("conv1_fwd"):
            ops.conv1_fwd(x, self.W1.detach(), self.b1.detach(), out=act, act_amax=amax)
        self._x, self._act, self._act_amax = x, act, amax
        return act

    def forward_images(self, x: torch.Tensor, act16: torch.Tensor, act_amax: torch.Tensor) -> None:
        """act = relu(conv1(x)) (client_part.py:114) written as the server's x3 operand into caller
        buffers — act16 images (ops.conv2_act16_bytes(B) bytes) + the per-sample max — for the image
        exchange of dist.Hub (images=True). No f32 act and no ReLU bit map: this client's backward
        re-derives its mask from x."""
        with TIMER("conv1_fwd"):
            ops.conv1_fwd_x3(x, self.W1.detach(), self.b1.detach(), act_amax, act16)
        self._x, self._act, self._act_amax, self._act16 = x, None, act_amax, act16

    def forward_eval(self, x: torch.Tensor, ema: bool = False):
        """The client forward of an evaluation pass: returns (act, act_amax, act16) in this stage's own
        `eval_` buffers — the x3 operand (act None) when emit_act16, else the f32 act (+ act_amax when
        emit_amax). Keeps nothing for a backward and leaves _x / _act / _act16 / _relu_bits alone, so a
        training forward ... backward_step sequence with an evaluation in between still works. `ema`: the
        kernels read the averaged block (views of it) instead of the parameters."""
        B = x.shape[0]
        W1, b1 = self._weights(((32, 1, 3, 3), (32,)), True) if ema else (self.W1.detach(), self.b1.detach())
        if self.emit_act16:
            amax = self._buf.get("eval_act_amax", (B,), torch.float32, self.device)
            a16 = self._buf.get("eval_act16", (ops.conv2_act16_bytes(B),), torch.uint8, self.device)
            with TIMER("eval_conv1_fwd"):
                ops.conv1_fwd_x3(x, W1, b1, amax, a16)
            return None, amax, a16
        act = self._buf.get("eval_act", (B, 32, 26, 26), torch.float32, self.device)
        amax = self._buf.get("eval_act_amax", (B,), torch.float32, self.device) if self.emit_amax else None
        with TIMER("eval_conv1_fwd"):
            ops.conv1_fwd(x, W1, b1, out=act, act_amax=amax)
        return act, amax, None

    def _slabs(self, cut_grad, x, act, tag="slabs"):
        x = self._x if x is None else x
        act = self._act if act is None else act
        B = x.shape[0]
        slabs = self._buf.get(tag, (ops.conv1_wgrad_nslab(B), ops.CLIENT_NPARAM), torch.float32, self.device)
        with TIMER("conv1_wgrad"):
            # the mask act > 0 is recomputed from x and W1 (unchanged since the forward: the client
            # steps after its backward), so only x and cut_grad are read
            ops.conv1_wgrad_remask_slabs(x, self.W1.detach(), self.b1.detach(), cut_grad, slabs=slabs)
        return slabs

    def backward_step(self, cut_grad: torch.Tensor, x: Optional[torch.Tensor] = None,
                      act: Optional[torch.Tensor] = None) -> None:
        """act.backward(cut_grad); optimizer.step() (client_part.py:132-133): relu-bwd + conv1
        wgrad slabs, then ONE fused reduce+SGD launch over the 320 client parameters."""
        self.step_from_slabs(self._slabs(cut_grad, x, act))

    def step_from_slabs(self, slabs: torch.Tensor) -> None:
        """optimizer.step() from gradient slabs produced elsewhere (the server's fused x3 dgrad,
        ServerStage.forward_backward(client_fuse=...)): one fused reduce + SGD launch."""
        with TIMER("sgd_client"):
            self._sgdm([self.seg(0, ops.CLIENT_NPARAM, slabs)])
            self._tick()

    def backward(self, cut_grad: torch.Tensor, x: Optional[torch.Tensor] = None,
                 act: Optional[torch.Tensor] = None, accumulate: bool = False) -> None:
        """Weight gradient into self.grads (accumulate=True adds: micro-batches)."""
        slabs = self._slabs(cut_grad, x, act)
        ops.reduce_slabs(slabs, out=self.grads, accumulate=accumulate)

    def step(self):
        """SGD from the (already reduced / all-reduced) flat gradient block."""
        with TIMER("sgd_client"):
            if self.optim is None:
                ops.sgd(self.params, self.grads, self.lr)
            else:
                self._sgdm([self.grads_segment()])
                self._tick()


class ServerStage(_SgdRecipe):
    """Server half: ModelPartB + CrossEntropyLoss + SGD + loss log (src/server_part.py:14-16,25-58)."""

    PAIRS = ((0, ops.CONV2_SLAB, 18432), (ops.CONV2_SLAB, ops.SERVER_NPARAM, 92160))
    TENSORS = ("conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias")

    def __init__(self, model: Optional[ModelPartB] = None, lr: float = LR, device="cuda",
                 loss_log: Optional[LossLog] = None, conv: str = CONV_DEFAULT,
                 optim: Optional[SGD] = None, schedule: Optional[LRSchedule] = None,
                 clip: Optional[ClipNorm] = None, loss: Optional[SoftCrossEntropy] = None,
                 ema: Optional[EMA] = None):
        self.device = torch.device(device)
        # loss=SoftCrossEntropy(eps): every head path below calls its soft entry (mixed labels + label smoothing,
        # splitcnn.loss); eps is a constructor constant passed by value, so a captured graph keeps it (no setter)
        self.loss = check_loss(loss)
        self.conv = conv
        self.impl_fwd, self.impl_dgrad, self.impl_wgrad = CONV_PRESETS[conv]
        self.share_images = True  # x3: the forward's split input images feed the wgrad (act16)
        self.model = (model if model is not None else ModelPartB()).to(self.device)
        self.lr = lr
        m = self.model
        self.params, self.grads = _flatten_params(
            [m.conv2.weight, m.conv2.bias, m.fc1.weight, m.fc1.bias], self.device)
        self._init_optim(optim, schedule, clip, ema)
        self.loss_log = loss_log if loss_log is not None else LossLog(self.device)
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.eval_err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)  # evaluate()'s own flag
        self.eval_logits = None   # the logits of the last evaluate() (a stage buffer)
        self.fuse_optim = True  # step_request: SGD of both slab kinds + the loss log in one launch
        # launch order knobs (profiling, tools/ab_trainers.py): fc1 wgrad right after the head (pooled
        # just read by it), conv2 wgrad before the dgrad. Defaults: the measured fastest order.
        self.fc_wgrad_early = False
        self.wgrad_first = False
        # the head as logits + cross-entropy, fc1 wgrad, then dpooled (+ dp_amax): fc1 wgrad re-reads
        # pooled while it is still in the Infinity Cache (the fused head's own 151 MB dpooled write
        # evicts it); same kernels, bit-identical results (tools/x3_ab.py --ops fcord --flush: 0.1010 ->
        # 0.0970 ms for head + fc1 wgrad from cold caches)
        self.fc_split = True
        # ... with its logits and cross-entropy in one launch (slk_fc_logits_xent, round 6; bitwise the two)
        self.fc_one_launch = True
        # ... and its fc1 wgrad and dpooled (+ dp_amax) as the two roles of one launch (slk_fc_backward; bitwise
        # the two launches, which False restores; the non-split orders above always use the two)
        self.fc_backward_one_launch = True
        self._buf = _Buffers()

    def bind_grads(self, view: torch.Tensor):
        view.copy_(self.grads)
        self.grads = view
        m = self.model
        m.conv2.weight.grad = view[:18432].view(64, 32, 3, 3)
        m.conv2.bias.grad = view[18432:18496].view(64)
        m.fc1.weight.grad = view[18496:110656].view(10, 9216)
        m.fc1.bias.grad = view[110656:].view(10)

    def _b(self, name, shape, dtype=torch.float32):
        return self._buf.get(name, shape, dtype, self.device)

    def forward_backward(self, act: Optional[torch.Tensor], labels: torch.Tensor, grad_scale: float,
                         cut_grad: Optional[torch.Tensor] = None, act_amax: Optional[torch.Tensor] = None,
                         act16: Optional[torch.Tensor] = None, client_fuse=None, cut_pack=None):
        """Server forward + CE + backward WITHOUT the optimizer step. Returns (cut_grad, loss_i,
        conv2 slabs, fc slabs). grad_scale = 1/global_batch (mean loss). act_amax: the per-sample x3
        scale bound of act when the client produced it (ClientStage.emit_amax: conv1_cut_bound, >= max act;
        only its power of two is used); the x3 kernels compute the exact max otherwise.
        act16 (with act_amax, x3 forward + wgrad only): the client's split input images
        (ClientStage.emit_act16) — act is then not read and may be None. client_fuse = (x, relu_bits,
        slabs) (x3 dgrad only, single-GPU step): the dgrad also runs the client's ReLU backward +
        conv1 wgrad into `slabs` and the cut gradient is not materialised (returned as None).
        cut_pack = (parts, part_b) (x3 dgrad only; the codec exchange, dist.Hub): the cut gradient leaves
        packed at the positions of each part's received mask — parts = int64 device table [B / part_b, 3] of
        (mask, ranks, vals) pointers, one part per part_b samples (ops.conv2_dgrad_x3_pack_parts) — instead
        of dense; returned as None."""
        B = labels.shape[0]
        m = self.model
        W2, b2 = m.conv2.weight.detach(), m.conv2.bias.detach()
        W3, b3 = m.fc1.weight.detach(), m.fc1.bias.detach()
        fi, di, wi = self.impl_fwd, self.impl_dgrad, self.impl_wgrad
        if act16 is not None and ((fi, wi) != ("x3", "x3") or act_amax is None):
            raise ValueError("act16 input needs the x3 forward and wgrad (conv preset 'x3') and act_amax")
        if act_amax is None and "x3" in (fi, wi):
            with TIMER("act_amax"):
                act_amax = ops.row_amax(act, out=self._b("act_amax", (B,)))
        dp_amax = self._b("dp_amax", (B,)) if "x3" in (di, wi) else None
        pooled_b, code_b = self._b("pooled", (B, 64, 12, 12)), self._b("code", (B, 64, 12, 12), torch.uint8)
        if act16 is not None:
            with TIMER("conv2_fwd_pool"):
                pooled, code = ops.conv2_fwd_pool_x3i(act16, act_amax, W2, b2, pooled=pooled_b, code=code_b)
        else:
            # x3 forward + x3 wgrad: the forward hands its split input images to the wgrad (LDS-DMA copy)
            act16 = (self._b("act16", (ops.conv2_act16_bytes(B),), torch.uint8)
                     if fi == "x3" and wi == "x3" and self.share_images else None)
            with TIMER("conv2_fwd_pool"):
                pooled, code = ops.conv2_fwd_pool(act, W2, b2, pooled=pooled_b, code=code_b, impl=fi,
                                                  act_amax=act_amax, act16=act16)
        split = self.fc_split and dp_amax is not None
        soft = None if self.loss is None else float(self.loss.label_smoothing)
        if split:
            with TIMER("fc_xent"):
                if self.fc_one_launch and soft is None:
                    _, loss_i, dlogits = ops.fc_logits_xent(
                        pooled, W3, b3, labels, grad_scale, logits=self._b("logits", (B, 10)),
                        loss_i=self._b("loss_i", (B,)), dlogits=self._b("dlogits", (B, 10)), err_flag=self.err_flag)
                elif self.fc_one_launch:
                    _, loss_i, dlogits = ops.fc_logits_xent_soft(
                        pooled, W3, b3, labels, grad_scale, soft, logits=self._b("logits", (B, 10)),
                        loss_i=self._b("loss_i", (B,)), dlogits=self._b("dlogits", (B, 10)), err_flag=self.err_flag)
                else:
                    logits = ops.fc_fwd(pooled, W3, b3, out=self._b("logits", (B, 10)))
                    if soft is None:
                        loss_i, dlogits = ops.xent_fwd_bwd(logits, labels, grad_scale, loss_i=self._b("loss_i", (B,)),
                                                           dlogits=self._b("dlogits", (B, 10)), err_flag=self.err_flag)
                    else:
                        loss_i, dlogits = ops.xent_soft_fwd_bwd(
                            logits, labels, grad_scale, soft, loss_i=self._b("loss_i", (B,)),
                            dlogits=self._b("dlogits", (B, 10)), err_flag=self.err_flag)
            s3 = self._b("s3", (ops.fc_wgrad_nslab(B), ops.FC_SLAB))
            dpooled = self._b("dpooled", (B, 64, 12, 12))
            if self.fc_backward_one_launch:
                with TIMER("fc_backward"):
                    ops.fc_backward(dlogits, W3, pooled, dpooled=dpooled.view(B, 9216), dp_amax=dp_amax, slabs=s3)
            else:
                with TIMER("fc_wgrad"):
                    ops.fc_wgrad_slabs(dlogits, pooled, slabs=s3)
                with TIMER("fc_dgrad"):
                    ops.fc_dgrad(dlogits, W3, out=dpooled.view(B, 9216), dp_amax=dp_amax)
        else:
            with TIMER("fc_xent"):
                if soft is None:
                    _, loss_i, dlogits, dpooled = ops.fc_xent(
                        pooled, W3, b3, labels, grad_scale, logits=self._b("logits", (B, 10)),
                        loss_i=self._b("loss_i", (B,)), dlogits=self._b("dlogits", (B, 10)),
                        dpooled=self._b("dpooled", (B, 64, 12, 12)), err_flag=self.err_flag, dp_amax=dp_amax)
                else:
                    _, loss_i, dlogits, dpooled = ops.fc_xent_soft(
                        pooled, W3, b3, labels, grad_scale, soft, logits=self._b("logits", (B, 10)),
                        loss_i=self._b("loss_i", (B,)), dlogits=self._b("dlogits", (B, 10)),
                        dpooled=self._b("dpooled", (B, 64, 12, 12)), err_flag=self.err_flag, dp_amax=dp_amax)
        # launch order dgrad -> wgrad -> fc wgrad (measured fastest: DESIGN.md §3a "Launch order")
        if self.fc_wgrad_early and not split:
            with TIMER("fc_wgrad"):
                s3 = ops.fc_wgrad_slabs(dlogits, pooled, slabs=self._b("s3", (ops.fc_wgrad_nslab(B), ops.FC_SLAB)))

        def wgrad():
            with TIMER("conv2_wgrad"):
                return ops.conv2_wgrad_slabs(act, dpooled, code,
                                             slabs=self._b("s2", (ops.conv2_wgrad_nslab(B, impl=wi), ops.CONV2_SLAB)),
                                             impl=wi, act_amax=act_amax, dp_amax=dp_amax, act16=act16)
        if self.wgrad_first:
            s2 = wgrad()
        if cut_pack is not None:
            if di != "x3":
                raise ValueError("cut_pack needs the x3 dgrad (conv preset 'x3' or 'x3w')")
            with TIMER("conv2_dgrad"):
                ops.conv2_dgrad_x3_pack_parts(dpooled, code, W2, dp_amax, *cut_pack)
            cut_grad = None
        elif client_fuse is not None:
            if di != "x3":
                raise ValueError("client_fuse needs the x3 dgrad (conv preset 'x3' or 'x3w')")
            cx, cbits, cslabs = client_fuse
            with TIMER("conv2_dgrad"):
                ops.conv2_dgrad_client_slabs(dpooled, code, W2, cx, cbits, dp_amax=dp_amax, slabs=cslabs)
            cut_grad = None
        else:
            if cut_grad is None:
                cut_grad = self._b("cut_grad", (B, 32, 26, 26))
            with TIMER("conv2_dgrad"):
                ops.conv2_dgrad(dpooled, code, W2, out=cut_grad, impl=di, dp_amax=dp_amax)
        if not self.wgrad_first:
            s2 = wgrad()
        if not self.fc_wgrad_early and not split:
            with TIMER("fc_wgrad"):
                s3 = ops.fc_wgrad_slabs(dlogits, pooled, slabs=self._b("s3", (ops.fc_wgrad_nslab(B), ops.FC_SLAB)))
        return cut_grad, loss_i, s2, s3

    def _slab_segments(self, s2, s3):
        """The stage's two slab kinds, [conv2 | fc1], as segments of its optimizer step."""
        return [self.seg(0, ops.CONV2_SLAB, s2), self.seg(ops.CONV2_SLAB, ops.SERVER_NPARAM, s3)]

    def apply_grad_slabs(self, s2, s3):
        """optimizer.step() (server_part.py:52): two fused reduce+SGD launches, one per slab kind."""
        with TIMER("sgd_server"):
            self._sgdm(self._slab_segments(s2, s3))
            self._tick()

    def reduce_grads(self, s2, s3, accumulate: bool = False):
        """Reduce slabs into the flat gradient block without stepping (micro-batches, all-reduce)."""
        ops.reduce_slabs(s2, out=self.grads[:ops.CONV2_SLAB], accumulate=accumulate)
        ops.reduce_slabs(s3, out=self.grads[ops.CONV2_SLAB:], accumulate=accumulate)

    def compute(self, act, labels, grad_scale, accumulate=False, cut_grad=None, act_amax=None, act16=None,
                cut_pack=None):
        """forward_backward + reduce into self.grads; returns (cut_grad, loss_i)."""
        cut_grad, loss_i, s2, s3 = self.forward_backward(act, labels, grad_scale, cut_grad=cut_grad,
                                                         act_amax=act_amax, act16=act16, cut_pack=cut_pack)
        self.reduce_grads(s2, s3, accumulate=accumulate)
        return cut_grad, loss_i

    def step(self):
        with TIMER("sgd_server"):
            if self.optim is None:
                ops.sgd(self.params, self.grads, self.lr)
            else:
                self._sgdm([self.grads_segment()])
                self._tick()

    def log_loss(self, values, scale: Optional[float] = None, step: Optional[int] = None):
        """Log scale*sum(values) (default: the mean of per-sample losses) for `step`."""
        scale = 1.0 / values.numel() if scale is None else scale
        with TIMER("loss_log"):
            ops.loss_log(values, scale, self.loss_log.ring, self.loss_log.counter)
        if step is not None:
            self.loss_log.note_step(step)

    def step_request(self, act: Optional[torch.Tensor], labels: torch.Tensor, step: Optional[int] = None,
                     cut_grad: Optional[torch.Tensor] = None, act_amax: Optional[torch.Tensor] = None,
                     act16: Optional[torch.Tensor] = None, client_fuse=None, extra_segments=()):
        """One /forward_pass request (server_part.py:38-58): returns (cut_grad, loss_i). The mean
        loss for `step` lands in the device loss log. `extra_segments`: further segments (recipe.Seg: the fused
        trainer's client update, ClientStage.optim_segment, whose slabs the dgrad wrote) run in the same
        optimizer launch and step by this stage's recipe: its lr, or its config, schedule and counter."""
        B = labels.shape[0]
        cut_grad, loss_i, s2, s3 = self.forward_backward(act, labels, 1.0 / B, cut_grad=cut_grad,
                                                         act_amax=act_amax, act16=act16, client_fuse=client_fuse)
        if self.fuse_optim:
            # optimizer.step() + log_metric in ONE launch (bit-identical to the three below); measured
            # -10 us per step at B = 4096 (tools/ab_step.py). The client's SGD stays a separate launch
            # after its wgrad: moving that wgrad ahead of the server's update measured +25-35 us.
            loss = (loss_i, 1.0 / B, self.loss_log.ring, self.loss_log.counter)
            with TIMER("sgd_server"):
                self._sgdm([*self._slab_segments(s2, s3), *extra_segments], loss=loss, multi=True)
                self._tick()
            if step is not None:
                self.loss_log.note_step(step)
        elif self.optim is None:   # the by-value recipe steps the extra segments after the loss log
            self.apply_grad_slabs(s2, s3)
            self.log_loss(loss_i, step=step)
            self._sgdm(extra_segments)
        else:
            with TIMER("sgd_server"):
                self._sgdm([*self._slab_segments(s2, s3), *extra_segments])
                self._tick()
            self.log_loss(loss_i, step=step)
        return cut_grad, loss_i

    def check_labels(self):
        """Raise if any label seen so far was outside [0, 10) (torch raises IndexError there) or, with loss=, any
        target was malformed (splitcnn.loss)."""
        if int(self.err_flag.item()) != 0:
            raise IndexError(LABEL_ERROR)

    def evaluate(self, act: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, *,
                 act16: Optional[torch.Tensor] = None, act_amax: Optional[torch.Tensor] = None,
                 metrics=None, logits: Optional[torch.Tensor] = None, ema: bool = False):
        """Forward only (model.eval(); outputs = model(act); criterion(outputs, labels); outputs.argmax(1)):
        returns (pred i64 [B], loss_i f32 [B]); labels=None predicts only (loss_i is None). With act16 +
        act_amax on the 'x3' preset the code-less image forward runs (slk_conv2_fwd_pool_x3p); with an f32
        act (a remote client, any conv preset) the preset's own forward does, its routing codes going to
        scratch. Then the fc head in evaluation mode (slk_fc_eval): logits and loss_i are bitwise the
        training forward's. `metrics` (metrics.EvalMetrics) receives the batch; `logits` (f32 [B, 10])
        receives the logits instead of this stage's buffer (self.eval_logits either way).
        Every buffer is this call's own (`eval_` names: about 0.15 GB of pooled at B = 4096 here, 0.35 GB
        of images in ClientStage.forward_eval) and the label flag is eval_err_flag: parameters, gradients,
        the training buffers, err_flag and the loss log are not written. `ema`: the kernels read the averaged block
        (views of it, optim.EMA) instead of the parameters; it is not written either."""
        m = self.model
        if ema:
            W2, b2, W3, b3 = self._weights(((64, 32, 3, 3), (64,), (10, 9216), (10,)), True)
        else:
            W2, b2 = m.conv2.weight.detach(), m.conv2.bias.detach()
            W3, b3 = m.fc1.weight.detach(), m.fc1.bias.detach()
        fi = self.impl_fwd
        if act16 is not None:
            if fi != "x3" or act_amax is None:
                raise ValueError("act16 input needs the x3 forward (conv preset 'x3' or 'x3w') and act_amax")
            B = ops.batch_of(act_amax, (), "act_amax")
            pooled = self._b("eval_pooled", (B, 64, 12, 12))
            with TIMER("eval_conv2_fwd_pool"):
                ops.conv2_fwd_pool_x3p(act16, act_amax, W2, b2, pooled=pooled)
        else:
            if act is None:
                raise ValueError("evaluate needs act, or act16 + act_amax")
            B = ops.batch_of(act, (32, 26, 26), "act")
            if act_amax is None and fi == "x3":
                act_amax = ops.row_amax(act, out=self._b("eval_act_amax", (B,)))
            pooled = self._b("eval_pooled", (B, 64, 12, 12))
            with TIMER("eval_conv2_fwd_pool"):
                ops.conv2_fwd_pool(act, W2, b2, pooled=pooled, code=self._b("eval_code", (B, 64, 12, 12), torch.uint8),
                                   impl=fi, act_amax=act_amax if fi == "x3" else None)
        logits = logits if logits is not None else self._b("eval_logits", (B, 10))
        with TIMER("eval_fc"):
            _, loss_i, pred = ops.fc_eval(pooled, W3, b3, labels, logits=logits,
                                          loss_i=self._b("eval_loss_i", (B,)) if labels is not None else None,
                                          pred=self._b("eval_pred", (B,), torch.int64), err_flag=self.eval_err_flag)
        self.eval_logits = logits
        if metrics is not None:
            if labels is None:
                raise ValueError("metrics need labels")
            with TIMER("eval_accumulate"):
                metrics.update(loss_i, pred, labels)
        return pred, loss_i


class SplitTrainer(GraphedTrainer):
    """Both stages fused on ONE GPU (BASELINE config 2): the cut tensor is handed over in place.

    `step(x, y)` = client fwd -> server fwd/loss/bwd/SGD -> client bwd/SGD, exactly one reference
    step. With `graph=True` the step is captured once per batch size into a HIP graph (static input
    buffers; `step` copies into them unless the caller hands in those very buffers or registered its
    own: graphs.GraphedTrainer, which also holds evaluate / eval_batch and the optimizer state's save / load).

    `optim` (optim.SGD) and `schedule` (optim.LRSchedule) replace the reference's optim.SGD(lr): both stages
    share the config, the schedule and ONE device step counter, ticked once at the end of the step, so the
    captured graph follows the schedule. Without them `lr` is a by-value kernel argument: changing a
    stage's `lr` attribute after the first step does not reach a captured graph (use a schedule and
    LRSchedule.set_lr). `clip` (optim.ClipNorm, shared by both stages; selects the configured kernels like a
    schedule) clips each stage's gradient by that stage's own global norm before its update; grad_norms()
    reads the last step's norms. An optim.LARS config scales every tensor's step by its trust ratio (two launches
    per step like clipping, not combined with `clip`); trust_ratios() reads the last step's norms and ratios.
    `loss` (loss.SoftCrossEntropy) makes the server's head take mixed labels with label
    smoothing; the smoothing is a by-value constant of the launch, kept by a captured graph, with no setter.
    Evaluation stays the plain cross-entropy on plain labels. `ema` (optim.EMA, shared by both stages; selects
    the configured kernels like a schedule) keeps an exponential moving average of both parameter blocks: ONE
    slk_ema_multi launch over both in front of the shared counter's tick, inside the captured graph;
    evaluate / eval_batch / predict(weights="ema") run on it and ema_state_dict() reads it. Its `warmup` and
    `start` are by-value constants a captured graph keeps (no setter); EMA.set_decay reaches a captured graph."""

    input_shape = (1, 28, 28)

    def __init__(self, client: Optional[ModelPartA] = None, server: Optional[ModelPartB] = None,
                 lr: float = LR, device="cuda", graph: bool = True, loss_log: Optional[LossLog] = None,
                 conv: str = CONV_DEFAULT, act16: bool = True, fuse_client_backward: bool = True,
                 graph_inputs: int = 4, optim: Optional[SGD] = None, schedule: Optional[LRSchedule] = None,
                 clip: Optional[ClipNorm] = None, loss: Optional[SoftCrossEntropy] = None,
                 ema: Optional[EMA] = None):
        check_clip(clip)
        check_ema(ema)
        super().__init__(device, graph, graph_inputs)
        self.client = ClientStage(client, lr, self.device, optim=optim, schedule=schedule, clip=clip, ema=ema)
        self.server = ServerStage(server, lr, self.device, loss_log, conv=conv, optim=self.client.optim,
                                  schedule=self.client.schedule, clip=self.client.clip, loss=loss,
                                  ema=self.client.ema_cfg)
        if self.server.optim is not None:
            self.client.step_ctr = self.server.step_ctr
            self.client.auto_tick = self.server.auto_tick = False   # _eager ticks the shared counter
        # the cut's per-sample max rides along with the cut (fused into conv1) for the x3 kernels; with the
        # x3 forward AND wgrad the client writes the server's split input images directly (no f32 cut)
        self.client.emit_amax = "x3" in (self.server.impl_fwd, self.server.impl_wgrad)
        self.client.emit_act16 = (self.server.impl_fwd, self.server.impl_wgrad) == ("x3", "x3") and act16
        # the x3 dgrad also runs the client's ReLU backward + conv1 wgrad (no cut gradient in HBM)
        # (the client's ReLU mask comes from the bit map conv1_fwd_x3 writes next to the images)
        self.fuse_client_backward = self.server.impl_dgrad == "x3" and self.client.emit_act16 and fuse_client_backward

    def _eager(self, x, y):
        act = self.client.forward(x)
        a16 = self.client._act16 if self.client.emit_act16 else None
        if self.fuse_client_backward:
            c = self.client
            slabs = c._buf.get("c1w_slabs", (ops.conv2_dgrad_c1w_nslab(x.shape[0]), ops.CLIENT_NPARAM),
                               torch.float32, self.device)
            # the client's update joins the server's optimizer launch (its slabs are complete once the
            # dgrad has run; bit-identical to step_from_slabs) when both stages step at one lr
            s = self.server
            if s.optim is None and c.optim is None:
                one = c.lr == s.lr
            else:   # one recipe, one schedule and one counter (a config given to this trainer)
                one = (c.optim is s.optim and c.schedule is s.schedule and c.step_ctr is s.step_ctr
                       and c.clip is s.clip)
            s.step_request(act, y, act_amax=c._act_amax, act16=a16, client_fuse=(x, c._relu_bits, slabs),
                           extra_segments=[c.optim_segment(slabs)] if one else ())
            if not one:
                c.step_from_slabs(slabs)
        else:
            cut_grad, _ = self.server.step_request(act, y, act_amax=self.client._act_amax, act16=a16)
            self.client.backward_step(cut_grad)
        if self.server.optim is not None and not self.server.auto_tick:
            ema_update([self.client, self.server])   # both blocks in ONE launch, in front of the shared tick
            ops.tick(self.server.step_ctr)

    def _optim_state(self):
        """The device tensors of the optimizer state, by name (momentum buffers and step counters; with ema= the
        averaged blocks)."""
        keys = (("momentum_buffer", "buf"), ("step", "step_ctr"))
        return {f"{n}.{k}": getattr(st, a) for n, st in (("client", self.client), ("server", self.server))
                if st.optim is not None for k, a in keys + ((("ema", "ema"),) if st.ema is not None else ())}

    def _state(self):
        """Both parameter blocks, the loss log's counter and the optimizer state (the averaged blocks with it):
        what a step writes."""
        return [self.client.params, self.server.params, self.server.loss_log.counter, *self._optim_state().values()]

    # ---- evaluation / prediction: forward only, own `eval_` buffers (about 0.5 GB extra at B = 4096), no
    # training state touched
    def _eval_eager(self, x, y, metrics=None, weights="live"):
        ema = self._check_weights(weights)
        act, amax, a16 = self.client.forward_eval(x, ema=ema)
        return self.server.evaluate(act, y, act16=a16, act_amax=amax, metrics=metrics, ema=ema)

    def predict(self, x: torch.Tensor, return_logits: bool = False, weights: str = "live"):
        """pred = argmax of the logits of x (int64 [B]); with return_logits also the f32 [B, 10] logits.
        weights="ema": on the averaged weights (optim.EMA)."""
        pred, _ = self._eval_eager(x, None, weights=weights)
        return (pred.clone(), self.server.eval_logits.clone()) if return_logits else pred.clone()
