"""HIP-graph capture and the host side every graphed trainer shares.

`capture` is the package's one way to turn a launch sequence into a graph. `GraphedTrainer` owns what
engine.SplitTrainer and wide.WideTrainer have in common around their step: the graph caches and the
policy of which buffers get a graph of their own, the evaluation pass and its graphs, and the optimizer
state save / load. A trainer supplies its launch sequences (`_eager`, `_eval_eager`) and names its
state (`_state`, `_optim_state`). Nothing here launches a kernel of its own (grad_norms reads the stages' two
device [norm, coef] pairs back)."""
from __future__ import annotations

from typing import Dict

import torch


def capture(fn, device, preserve=()):
    """Capture fn() as a HIP graph: returns (graph, what the captured call returned). fn() first runs once
    on a side stream, so its allocations happen there and not during the capture. Both runs execute; the
    tensors in `preserve` get back the values they had before them."""
    preserve = tuple(preserve)
    saved = [t.clone() for t in preserve]
    cur = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn()
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    # thread-local capture mode: ProcessGroupNCCL's watchdog thread queries the events of earlier
    # collectives while this thread captures; in the default global mode that query invalidates it
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = fn()
    for t, v in zip(preserve, saved):
        t.copy_(v)
    return graph, out


def replay_on(g, x, y):
    """Replay g["graph"] on (x, y): copied into the graph's own inputs unless they are those inputs."""
    if x.data_ptr() != g["x"].data_ptr():
        g["x"].copy_(x, non_blocking=True)
    if y.data_ptr() != g["y"].data_ptr():
        g["y"].copy_(y, non_blocking=True)
    g["graph"].replay()


class GraphedTrainer:
    """Base of the single-GPU trainers: `step(x, y)` runs `_eager(x, y)`, with `graph=True` as a HIP graph
    captured once per batch size on static inputs that `step` copies into, or on the caller's own buffers.

    A trainer provides `input_shape` (of one sample), `client` / `server` (the server stage holds
    loss_log, eval_err_flag and eval_logits), `_eager(x, y)`, `_eval_eager(x, y, metrics)` -> (pred,
    loss_i), `_optim_state()` -> {name: device tensor}, `_state()` -> the tensors a training warm-up must
    not leave a trace in, and may override `_state_written()`."""

    input_shape: tuple = ()
    eval_cut = None   # the last evaluation's cut, in trainers whose _eval_eager keeps one

    def __init__(self, device, graph: bool = True, graph_inputs: int = 4):
        self.device = torch.device(device)
        self.graph = graph
        self._graphs = {}   # B -> the step's graph on the static inputs; (B, x ptr, y ptr) -> on a caller's pair
        # graphs captured on a caller's own input buffers (a loader's ring of batch buffers): replaying
        # one reads its inputs where they already are, with no copy into the static inputs; at most
        # `graph_inputs` such buffer pairs per batch size, any others go through the static inputs
        self.graph_inputs = graph_inputs
        self._seen = {}   # (B, x ptr, y ptr) -> times a caller buffer pair went through the static inputs
        self.global_step = 0
        self._eval_graphs = {}    # batch size -> the evaluation pass's graph (never in _graphs)
        self._eval_metrics = None  # evaluate()'s own accumulator, made on first use

    @property
    def loss_log(self):
        return self.server.loss_log

    def _state_written(self):
        """Called after the device state was written from outside the step (a capture's restore,
        load_optimizer_state): rebuild whatever is derived from it. Default: nothing is."""

    # ---- the step and its graphs
    def _new_inputs(self, B: int):
        return (torch.zeros((B,) + self.input_shape, dtype=torch.float32, device=self.device),
                torch.zeros((B,), dtype=torch.int64, device=self.device))

    def _graph_for(self, B: int, x=None, y=None):
        """The step's graph for batch size B on the static inputs, or (x, y given) on those buffers. The
        warm-up and the capture leave no trace in `_state()`."""
        key = B if x is None else (B, x.data_ptr(), y.data_ptr())
        g = self._graphs.get(key)
        if g is not None:
            return g
        if x is None:
            x, y = self._new_inputs(B)
        graph, _ = capture(lambda: self._eager(x, y), self.device, self._state())
        self._state_written()
        g = {"graph": graph, "x": x, "y": y}
        self._graphs[key] = g
        return g

    def static_inputs(self, B: int):
        g = self._graph_for(B)
        return g["x"], g["y"]

    def _own_buffers_ok(self, x, y) -> bool:
        return (x.device == self.device and y.device == self.device and x.dtype == torch.float32
                and y.dtype == torch.int64 and x.is_contiguous() and y.is_contiguous()
                and tuple(x.shape[1:]) == self.input_shape and y.shape == (x.shape[0],))

    def _is_static(self, x, y) -> bool:
        st = self._graphs.get(x.shape[0])
        return st is not None and x.data_ptr() == st["x"].data_ptr() and y.data_ptr() == st["y"].data_ptr()

    def _n_caller_graphs(self, B: int) -> int:
        return sum(1 for k in self._graphs if isinstance(k, tuple) and k[0] == B)

    def register_inputs(self, x: torch.Tensor, y: torch.Tensor) -> bool:
        """Capture the step's graph on the caller's own (x, y) buffers now — a loader declaring its ring
        of batch buffers — so step() on them replays with no copy and no capture later. Counts toward
        `graph_inputs`; False (nothing captured) when the buffers do not qualify or that budget is spent."""
        if not self.graph or not self._own_buffers_ok(x, y):
            return False
        B = x.shape[0]
        if self._is_static(x, y) or (B, x.data_ptr(), y.data_ptr()) in self._graphs:
            return True
        if self._n_caller_graphs(B) >= self.graph_inputs:
            return False
        self._graph_for(B, x, y)
        return True

    def _select_graph(self, x, y):
        """The graph step() replays directly on (x, y), or None (then it copies into the static inputs).
        The static inputs handed back (static_inputs(B)) replay their own graph; a caller buffer pair gets
        a graph of its own the SECOND time it is seen (a loader's ring), so a one-off fresh tensor goes
        through the static-input copy and is not kept alive by a graph."""
        if not self._own_buffers_ok(x, y):
            return None
        if self._is_static(x, y):
            return self._graphs[x.shape[0]]
        B = x.shape[0]
        key = (B, x.data_ptr(), y.data_ptr())
        g = self._graphs.get(key)
        if g is None:
            n = self._seen.get(key, 0) + 1
            self._seen[key] = n
            if n >= 2 and self._n_caller_graphs(B) < self.graph_inputs:
                g = self._graph_for(B, x, y)
                del self._seen[key]
        return g

    def step(self, x: torch.Tensor, y: torch.Tensor):
        if not self.graph:
            self._eager(x, y)
        else:
            g = self._select_graph(x, y)
            if g is not None:
                g["graph"].replay()
            else:
                replay_on(self._graph_for(x.shape[0]), x, y)
        self.server.loss_log.note_step(self.global_step)
        self.global_step += 1

    # ---- non-finite values
    def check_finite(self) -> None:
        """Raise FloatingPointError if any parameter, optimizer-state tensor (momentum, m, v) or averaged block of
        either stage holds a NaN or an infinity, naming stage and tensor ("server.conv2.weight", "client.conv1.bias
        (momentum)"). One host sync; nothing is launched inside the step. The convolution path writes +0 for a NaN
        pre-activation (include/slk.h "NaN and +-inf", clause 2), so a NaN weight can stay in a model whose logged
        loss is finite; call this next to check_labels() to notice it. A non-finite INPUT pixel that clause 2 erases
        before it reaches a parameter is not detectable this way."""
        from .recipe import _raise_nonfinite
        names, flags = [], []
        for stage, st in (("client", self.client), ("server", self.server)):
            n, f = st._finite_flags()
            names += [(stage, b, t) for b, t in n]
            flags.append(f)
        _raise_nonfinite(names, torch.cat(flags).tolist())

    # ---- gradient clipping (optim.ClipNorm)
    def grad_norms(self) -> Dict[str, tuple]:
        """{"client": (norm, coef), "server": (norm, coef)} of the last step: each stage's global L2 gradient
        norm before clipping and the coefficient its optimizer applied (1.0: not clipped). One host sync.
        Needs `clip=` (ClipNorm(float("inf")) measures without clipping)."""
        outs = [getattr(st, "clip_out", None) for st in (self.client, self.server)]
        if any(o is None for o in outs):
            raise RuntimeError("grad_norms: the trainer was built without clip= (optim.ClipNorm)")
        (cn, cc), (sn, sc) = torch.stack(outs).tolist()
        return {"client": (cn, cc), "server": (sn, sc)}

    # ---- layer-wise trust ratios (optim.LARS / optim.LAMB)
    def trust_ratios(self) -> Dict[str, Dict[str, tuple]]:
        """{"client": {"conv1.weight": (w_norm, x_norm, ratio), "conv1.bias": ...}, "server": {...}} of the last
        step: every tensor's parameter norm before the step, the norm of its gradient (LARS) or update direction
        (LAMB) and the ratio its step was scaled by (1.0 for a bias under exclude_bias). One host sync."""
        stages = (("client", self.client), ("server", self.server))
        if any(getattr(st, "trust_out", None) is None for _, st in stages):
            raise RuntimeError("trust_ratios: the trainer was built without optim.LARS / optim.LAMB")
        rows = torch.cat([st.trust_out for _, st in stages]).tolist()
        out, k = {}, 0
        for name, st in stages:
            out[name] = {t: tuple(rows[k + j]) for j, t in enumerate(st.TENSORS)}
            k += len(st.TENSORS)
        return out

    # ---- the averaged weights (optim.EMA)
    def _check_weights(self, weights) -> bool:
        """Whether an evaluation runs on the averaged weights: "live" or "ema" (which needs ema=)."""
        if weights not in ("live", "ema"):
            raise ValueError(f"weights: expected 'live' or 'ema', got {weights!r}")
        if weights == "ema" and any(getattr(st, "ema", None) is None for st in (self.client, self.server)):
            raise RuntimeError("weights='ema': the trainer was built without ema= (optim.EMA)")
        return weights == "ema"

    def ema_state_dict(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"client": {...}, "server": {...}}: the averaged blocks as CPU tensors under the modules' own
        state_dict() names and shapes (load them into fresh modules to deploy the average). One host sync.
        Needs `ema=`."""
        stages = (("client", self.client), ("server", self.server))
        if any(getattr(st, "ema", None) is None for _, st in stages):
            raise RuntimeError("ema_state_dict: the trainer was built without ema= (optim.EMA)")
        out = {}
        for name, st in stages:
            sd, flat, off = st.model.state_dict(), st.ema.detach().cpu(), 0
            out[name] = {}
            for t in st.TENSORS:   # the flat block's order
                k = sd[t].numel()
                out[name][t] = flat[off:off + k].view(sd[t].shape).clone()
                off += k
        return out

    # ---- optimizer state
    def optimizer_state(self) -> Dict[str, torch.Tensor]:
        """CPU copies of the optimizer state, by name (empty where the optimizer has none). With the
        modules' state_dict() it resumes training bit for bit (load_optimizer_state)."""
        return {k: t.detach().cpu().clone() for k, t in self._optim_state().items()}

    def load_optimizer_state(self, state: Dict[str, torch.Tensor]) -> None:
        """Copy a saved optimizer_state() into the device state — also under already captured graphs,
        which read exactly these tensors — and rebuild what is derived from the parameters (load the
        modules' state_dict() first)."""
        own = self._optim_state()
        if set(state) != set(own):
            raise ValueError(f"load_optimizer_state: expected keys {sorted(own)}, got {sorted(state)}")
        for k, t in own.items():
            t.copy_(state[k])
        self._state_written()

    # ---- evaluation: forward only, own `eval_` buffers, no training state touched
    def _eval_graph_for(self, B: int, metrics, weights="live"):
        """The evaluation pass for batch size B as a HIP graph on static inputs: one linear chain on one
        stream (client forward, server forward, head, accumulate), kept in `_eval_graphs` — not `_graphs`,
        whose keys the step's caller-buffer budget counts. The accumulator of `metrics` is baked in: another
        metrics object (or none) recaptures on the same static inputs. Warm-up and capture leave the
        accumulator and the evaluation label flag as they were. The pass on the averaged weights
        (weights="ema") is a graph of its own under the key (B, "ema"), with its own static inputs: `_eval_graphs[B]`
        stays the live one."""
        key = B if weights == "live" else (B, weights)
        g = self._eval_graphs.get(key)
        if g is not None and g["metrics"] is metrics:
            return g
        x, y = self._new_inputs(B) if g is None else (g["x"], g["y"])
        state = [self.server.eval_err_flag] + ([metrics.acc] if metrics is not None else [])
        run = ((lambda: self._eval_eager(x, y, metrics)) if weights == "live" else
               (lambda: self._eval_eager(x, y, metrics, weights=weights)))
        graph, out = capture(run, self.device, state)
        # the buffers this graph writes: a replay runs no Python, so eval_batch re-points the public
        # attributes (server.eval_logits, and a trainer's eval_cut) at them after every replay
        g = {"graph": graph, "x": x, "y": y, "metrics": metrics, "out": out, "logits": self.server.eval_logits,
             "cut": self.eval_cut}
        self._eval_graphs[key] = g
        return g

    def eval_batch(self, x: torch.Tensor, y: torch.Tensor, metrics=None, weights: str = "live"):
        """One held-out batch, asynchronous: (pred, loss_i), stage buffers that the next batch of the same
        size overwrites (the logits are in server.eval_logits); `metrics` (metrics.EvalMetrics) updated on
        the device. With graph=True the pass replays a graph captured once per batch size on static inputs
        that x and y are copied into. The graph holds the accumulator of `metrics`: calling with another
        metrics object (or none, or alternating with evaluate(), which uses the trainer's own) captures
        that size again — a warm-up and a capture each switch — so keep to one EvalMetrics per trainer in a
        loop. Parameters, optimizer state, the loss log, err_flag and global_step are not touched.
        weights="ema" runs the same pass on the averaged weights (optim.EMA; its own graph per batch size); the
        averaged blocks are only read."""
        ema = self._check_weights(weights)
        if tuple(x.shape[1:]) != self.input_shape or tuple(y.shape) != (x.shape[0],):
            raise ValueError(f"eval_batch: expected x [B,{','.join(map(str, self.input_shape))}] and y [B], got "
                             f"{tuple(x.shape)} and {tuple(y.shape)}")
        if not self.graph:
            return self._eval_eager(x, y, metrics, weights=weights) if ema else self._eval_eager(x, y, metrics)
        g = self._eval_graph_for(x.shape[0], metrics, weights)
        g["x"].copy_(x, non_blocking=True)
        g["y"].copy_(y, non_blocking=True)
        g["graph"].replay()
        self.server.eval_logits = g["logits"]   # this batch size's buffers (another size may have run since)
        if g["cut"] is not None:
            self.eval_cut = g["cut"]
        return g["out"]

    def evaluate(self, batches, metrics=None, weights: str = "live"):
        """metrics.EvalResult over an iterable of device (x, y) batches — for example
        DeviceLoader(MnistIDX(root, train=False), 4096, shuffle=False) — with one host sync, at the end.
        With metrics=None the trainer's own EvalMetrics is reset and used; a caller's `metrics` is added to
        as it is (reset it first for a fresh evaluation). weights="ema": on the averaged weights (optim.EMA)."""
        from .metrics import EvalMetrics
        self._check_weights(weights)
        if metrics is None:
            if self._eval_metrics is None:
                self._eval_metrics = EvalMetrics(self.device)
            metrics = self._eval_metrics.reset()
        for x, y in batches:
            self.eval_batch(x, y, metrics, weights)
        return metrics.result()
