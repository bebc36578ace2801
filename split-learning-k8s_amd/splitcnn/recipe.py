"""The optimizer recipe of a stage: which launches of splitcnn.ops one optimizer step is.

`StageRecipe` is the base of the four stage classes (engine.py: K2 on the SGD family, wide.py: K5 on the Adam
family). It owns what the two families share — the rules of construction, the typed segment `Seg`, the expansion
of a whole-stage segment into [weight | bias] pairs, the groups of the clipped and layer-wise launches, the refusal
of another stage's segment under another recipe, the averaged block's update and the counter's tick. A family
(`_SgdRecipe`, `_AdamRecipe`) adds only which ops entry runs in each case.
"""
from __future__ import annotations

import contextlib
from collections import defaultdict
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .optim import LRSchedule, check_clip, check_ema, is_layerwise


class KernelTimer:
    """HIP-event timing of named launches on the launching (current) stream. Disabled by default;
    bench.py enables it for its per-kernel pass. Never enable inside graph capture."""

    def __init__(self):
        self.enabled = False
        self._ev: Dict[str, list] = defaultdict(list)

    @contextlib.contextmanager
    def __call__(self, name: str):
        if not self.enabled:
            yield
            return
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        yield
        e.record()
        self._ev[name].append((s, e))

    def reset(self):
        self._ev.clear()

    def summary(self) -> Dict[str, Dict[str, float]]:
        torch.cuda.synchronize()
        out = {}
        for k, v in self._ev.items():
            ms = [s.elapsed_time(e) for s, e in v]
            out[k] = {"avg_ms": sum(ms) / len(ms), "min_ms": min(ms), "n": len(ms)}
        return out


TIMER = KernelTimer()
_UNTIMED = contextlib.nullcontext()


def _flatten_params(params: List[nn.Parameter], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Move `params` into one flat fp32 block; each Parameter becomes a view of it."""
    n = sum(p.numel() for p in params)
    flat = torch.empty(n, dtype=torch.float32, device=device)
    gflat = torch.zeros(n, dtype=torch.float32, device=device)
    off = 0
    for p in params:
        k = p.numel()
        flat[off:off + k].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
        p.data = flat[off:off + k].view(p.shape)
        p.grad = gflat[off:off + k].view(p.shape)
        off += k
    return flat, gflat


class Seg(NamedTuple):
    """One slice of a stage's flat blocks and the gradient slabs that step it."""
    param: torch.Tensor
    grad: Optional[torch.Tensor]        # None: the [1, n] slabs ARE the gradient block, read in place
    state: Tuple[torch.Tensor, ...]     # (), (buf,) or (m, v)
    slabs: torch.Tensor                 # [nslab, n]
    nw: Optional[int] = None            # the weight elements of a [W | b] pair (the layer-wise launches)
    owner: Optional["StageRecipe"] = None   # the stage whose partials and clip_out / trust_out it belongs to

    def args(self) -> tuple:
        """The tuple the ops wrappers take: (param, grad, state ..., slabs[, nw])."""
        return (self.param, self.grad, *self.state, self.slabs) + (() if self.nw is None else (self.nw,))


def ema_update(stages):
    """slk_ema_multi over the averaged blocks of `stages` (those built with ema=; they share the config and the
    counter): ONE launch, after their optimizer launches and before the counter's tick."""
    stages = [st for st in stages if st.ema is not None]
    if not stages:
        return
    cfg = stages[0].ema_cfg
    with TIMER("ema_multi"):
        ops.ema_multi([(st.ema, st.params) for st in stages], cfg.value, stages[0].step_ctr, cfg.start, cfg.warmup)


def _raise_nonfinite(names, ok) -> None:
    """names: [(stage, block, tensor)], ok: [bool]. Raises FloatingPointError listing every entry that is not ok."""
    bad = [f"{stage}.{tensor}" + ("" if block == "params" else f" ({block})")
           for (stage, block, tensor), good in zip(names, ok) if not good]
    if bad:
        raise FloatingPointError("splitcnn: non-finite values (NaN or inf) in " + ", ".join(bad))


class StageRecipe:
    """Optimizer state and step of a stage that keeps `params` / `grads` as flat blocks on `device`.

    Without a config (optim=None) the stage runs the family's default recipe with its hyper-parameters as by-value
    kernel arguments (frozen into a captured graph). With a config (CONFIG: optim.SGD or optim.Adam) and / or an
    optim.LRSchedule it runs the configured kernels: the rate is read from the schedule's device table at the device
    counter `step_ctr` of completed optimizer steps, so graph replays follow both. With an optim.ClipNorm (`clip`,
    which like a schedule selects the configured kernels) every step is two launches, slk_reduce_sqnorm_multi then the
    family's clipped step: the stage's gradient is clipped by its own global L2 norm before weight decay; `grads`
    keeps the unclipped gradient, `clip_out` the last step's device [norm, coef] and `clip_npart` the partials it
    spent. With a layer-wise config (optim.LARS / optim.LAMB, not combined with clip) every step is the family's two
    trust-ratio launches over the stage's [weight | bias] pairs (PAIRS: (lo, hi, weight elements) of the flat
    block); `trust_out` keeps every tensor's [w_norm, g_norm or u_norm, ratio] of the last step in TENSORS' order and
    `trust_nblk` the partials per pair. With an optim.EMA (`ema_cfg`) the stage owns `ema`, a flat block like params
    that starts as their copy; slk_ema_multi runs after the optimizer launch(es) and in front of the counter's tick
    (_tick). A trainer that shares one counter between two stages sets auto_tick False and launches both itself."""

    CONFIG = None           # the family's config class
    HYPER = ("lr",)         # the stage attributes that are CONFIG's leading arguments
    STATE = ()              # the names of the state blocks (flat, like params)
    BY_VALUE_COUNTER = False   # the default by-value recipe keeps state and a counter of its own
    TICK_TIMER = False      # _tick reports under TIMER("tick")

    def _init_optim(self, optim, schedule, clip=None, ema=None):
        cfg = self.CONFIG
        if optim is not None and not isinstance(optim, cfg):
            raise TypeError(f"optim: expected splitcnn.optim.{cfg.__name__} or None, got {type(optim).__name__}")
        check_clip(clip)
        check_ema(ema)
        # what needs the device counter selects the configured kernels at the default constants
        if optim is None and (schedule is not None or clip is not None
                              or (ema is not None and not self.BY_VALUE_COUNTER)):
            optim = cfg(*(getattr(self, k) for k in self.HYPER))
        if is_layerwise(optim) and clip is not None:
            raise ValueError(f"{type(optim).__name__} is not combined with clip= (the trust ratio already bounds "
                             "every tensor's step by its own norms)")
        self.optim, self.schedule = optim, None
        self.clip = self.clip_out = self.trust_out = None
        self.ema = self.ema_cfg = None
        self.auto_tick = True
        stateful = optim is not None or self.BY_VALUE_COUNTER
        for k in self.STATE:
            setattr(self, k, torch.zeros_like(self.params) if stateful else None)
        self.step_ctr = torch.zeros(1, dtype=torch.int32, device=self.device) if stateful else None
        if ema is not None:
            self.ema_cfg = ema.to(self.device)
            self.ema = self.params.clone()
        if optim is None:
            return
        for k in self.HYPER:
            setattr(self, k, getattr(optim, k))
        self.schedule = (schedule if schedule is not None else LRSchedule.constant(optim.lr, self.device)).to(self.device)
        if clip is not None:
            self.clip = clip.to(self.device)
            self.clip_out = torch.zeros(2, dtype=torch.float32, device=self.device)   # [norm, coef] of the last step
        if is_layerwise(optim):   # three floats for every tensor's last step, in TENSORS' order
            self.trust_out = torch.zeros(2 * len(self.PAIRS), 3, dtype=torch.float32, device=self.device)

    # ---- segments
    def _blocks(self) -> tuple:
        """The state blocks this stage has (none without a counter: the SGD family's by-value recipe)."""
        return tuple([getattr(self, k) for k in self.STATE]) if self.step_ctr is not None else ()

    def seg(self, lo, hi, slabs, write_grads=True) -> Seg:
        """[lo, hi) of this stage stepped from `slabs` [nslab, hi - lo]; write_grads False: the slabs are the
        gradient block itself (one slab), read in place."""
        return Seg(self.params[lo:hi], self.grads[lo:hi] if write_grads else None,
                   tuple([t[lo:hi] for t in self._blocks()]), slabs)

    def optim_segment(self, slabs) -> Seg:
        """This stage's whole update as a segment of another stage's optimizer launch(es); under `clip` or a
        layer-wise recipe (shared with that stage) a group of its own there."""
        return Seg(self.params, self.grads, self._blocks(), slabs, owner=self)

    def grads_segment(self) -> Seg:
        """This stage's whole update from its (already reduced / all-reduced) gradient block, in place."""
        return Seg(self.params, None, self._blocks(), self.grads.view(1, -1))

    def _pairs_of(self, seg: Seg) -> List[Seg]:
        """`seg` with nw if it is one of this stage's [weight | bias] pairs; one slice per pair if it is the whole
        stage."""
        lo = seg.param.storage_offset() - self.params.storage_offset()
        hi = lo + seg.param.numel()
        nw = {(a, b): w for a, b, w in self.PAIRS}.get((lo, hi))
        if nw is not None:
            return [seg._replace(nw=nw)]
        if (lo, hi) != (0, self.params.numel()):
            raise ValueError(f"{type(self.optim).__name__}: a segment must be one [weight | bias] pair")
        return [seg._replace(param=seg.param[a:b], grad=None if seg.grad is None else seg.grad[a:b],
                             state=tuple(t[a:b] for t in seg.state), slabs=seg.slabs[:, a:b], nw=w)
                for a, b, w in self.PAIRS]

    def _clip_group(self, segs):
        """This stage's segments as one group of the clip launches: its own partials and [norm, coef]."""
        segs = [s.args() for s in segs]
        need = self.clip_npart = ops.clip_partials_needed(segs)   # partials of this stage's last clipped step
        return (self._buf.get("clip_partials", (need,), torch.float32, self.device), self.clip_out, segs)

    def _trust_group(self, segs):
        """This stage's [W | b] pairs as one group of the layer-wise launches: its own partials and trust_out."""
        segs = [p.args() for s in segs for p in self._pairs_of(s)]
        need = ops.trust_partials_needed(segs)
        self.trust_nblk = [ops.reduce_sqnorm_nblk(g[-2].shape[1], g[-2].shape[0]) for g in segs]   # partials per pair
        return (self._buf.get("trust_partials", (need,), torch.float32, self.device), self.trust_out, segs)

    # ---- the step
    def _step(self, segs: List[Seg], loss=None, multi=False):
        """One optimizer step over `segs`: separate launches, or ONE with the loss log (multi); with `clip` or a
        layer-wise recipe always the two launches over all of them (the loss log rides in the first)."""
        layerwise = is_layerwise(self.optim)
        foreign = [s for s in segs if s.owner is not None and s.owner is not self]
        if any(s.owner.clip is not self.clip or is_layerwise(s.owner.optim) != layerwise for s in foreign):
            raise ValueError("a segment of another stage must share this stage's clip= (both clipped by one "
                             "optim.ClipNorm, or neither) and its layer-wise recipe")
        if self.optim is None:
            return self._by_value([s.args() for s in segs], loss, multi)
        kw = dict(lr_table=self.schedule.table, step=self.step_ctr, **self.optim.kernel_args())
        if not layerwise and self.clip is None:
            return self._plain([s.args() for s in segs], loss, multi, kw)
        # this stage's group, then one per segment of another stage, built by that stage over its own buffers
        build = StageRecipe._trust_group if layerwise else StageRecipe._clip_group
        own = [s for s in segs if s.owner is None or s.owner is self] if foreign else segs
        groups = [build(self, own)] + [build(s.owner, [s]) for s in foreign]
        (self._layerwise if layerwise else self._clipped)(groups, loss, kw)

    def _tick(self):
        """The averaged block's update (ema=), then ++step_ctr: the end of every stepping path of a stage that
        owns its counter."""
        if self.auto_tick and self.step_ctr is not None:
            ema_update([self])
            with TIMER("tick") if self.TICK_TIMER else _UNTIMED:
                ops.tick(self.step_ctr)

    # ---- non-finite values (include/slk.h "NaN and +-inf")
    def _finite_flags(self):
        """([(block, tensor)], device bool [n]): for every tensor of TENSORS in the parameter block, every
        optimizer-state block (STATE) and the averaged block (ema=), whether all its values are finite. Torch
        reductions on the current stream, outside the step; no host sync."""
        blocks = [("params", self.params)]
        blocks += [("momentum" if k == "buf" else k, t) for k, t in zip(self.STATE, self._blocks())]
        if self.ema is not None:
            blocks.append(("ema", self.ema))
        sd = self.model.state_dict()
        names, flags = [], []
        for bname, flat in blocks:
            off = 0
            for t in self.TENSORS:
                k = sd[t].numel()
                names.append((bname, t))
                flags.append(torch.isfinite(flat[off:off + k]).all())
                off += k
        return names, torch.stack(flags)

    def check_finite(self, stage: str = None) -> None:
        """Raise FloatingPointError naming every tensor of this stage — parameters, optimizer state (momentum, m, v),
        averaged block — that holds a NaN or an infinity. One host sync. The convolution path writes +0 for a NaN
        pre-activation (clause 2 of the non-finite rule), so a NaN weight can sit in a model whose logged loss stays
        finite: this is the supported way to notice it. It cannot see a non-finite INPUT that the rule erases before
        it reaches a parameter."""
        names, flags = self._finite_flags()
        _raise_nonfinite([(stage or type(self).__name__, b, t) for b, t in names], flags.tolist())

    def _weights(self, shapes, ema=False):
        """Views of the parameter block, or of the averaged block (ema), in the tensors' own shapes."""
        if ema and self.ema is None:
            raise RuntimeError(f"{type(self).__name__}: weights='ema' needs a stage built with ema= (optim.EMA)")
        flat, out, off = self.ema if ema else self.params, [], 0
        for shp in shapes:
            k = 1
            for d in shp:
                k *= d
            out.append(flat[off:off + k].view(shp))
            off += k
        return out
