"""The training runtime of the small Dense stacks (models/zoo.py ``titanic_dnn``, ``simulated_mlp``,
``maggy_regressor``): the whole Adam / AdamW step as ONE one-workgroup kernel launch running ``nsteps`` steps over
an HBM-resident epoch (``FusedMlpStep``: csrc/ops/mlp_step.hip), and the plain fp64 reference of that step
(``reference_steps``).

Reference workloads: BASELINE config 4 "Titanic training dataset -> DNN" (maggy-ablation-titanic-example.ipynb:
233-243, retrained once per ablation trial), the simulated-data examples (E4/E6) and the maggy regressor (E12)."""
from __future__ import annotations

import os

import torch

from .. import nn as hnn
from ..ops import _C
from . import health
from .capture import graph as _capture_graph
from .launch_slots import ArgSlots, launch_shapes

MAX_LAYERS, MAX_WIDTH, MAX_BATCH = 8, 64, 64  # csrc/ops/mlp_step.hip MAXL, MAXD, MAXB
ACTS = {None: 0, "relu": 1, "sigmoid": 2}
LOSSES = {"bce_logits": 0, "mse": 1}
KINDS = {"adam": 1, "adamw": 2}


def dense_layers(model, loss_kind: str | None = None):
    """``[(Linear, activation), ...]`` if ``model`` (a Keras-style ``Sequential`` or its ``net``, or any module
    whose children run in sequence) is nothing but ``Linear`` layers behind the input cast, else None.  A Keras
    ``Sequential`` trained with ``bce_logits`` has its final sigmoid folded into the loss (keras._strip_sigmoid):
    that layer is reported with no activation."""
    net = getattr(model, "net", model)
    if net is None or not isinstance(net, torch.nn.Module):
        return None
    mods = list(net.children()) if not isinstance(net, hnn.Linear) else [net]
    if mods and type(mods[0]).__name__ == "_InputNorm":  # fp32 in, the compute dtype out: the kernel's own cast
        mods = mods[1:]
    if not mods or not all(type(m) is hnn.Linear for m in mods):
        return None
    out = [(m, m.activation) for m in mods]
    if hasattr(model, "_specs") and loss_kind == "bce_logits" and out[-1][1] == "sigmoid":
        out[-1] = (out[-1][0], None)
    for (a, _), (b, _) in zip(out, out[1:]):
        if a.out_features != b.in_features:
            return None
    return out


def _ints(layers, B: int, nbatch: int, nsteps: int, kind: str, loss_kind: str) -> list[int]:
    """The kernel's integer vector (mlp_step.hip ``fill``)."""
    lins = [m for m, _ in layers]
    dims = [lins[0].in_features] + [m.out_features for m in lins]

    def off(p):
        return int(getattr(p, "_hx_off", 0)) if p is not None else -1

    return ([len(lins), int(B), int(nbatch), int(nsteps), KINDS[kind], LOSSES[loss_kind]] + dims
            + [ACTS[a] for _, a in layers] + [off(m.weight) for m in lins] + [off(m.bias) for m in lins])


def why_not(model, optimizer, loss_kind: str, B: int, world: int = 1) -> str | None:
    """Why the one-launch step does not take this configuration (None: it does).  Everything outside the
    kernel's family is declined, never approximated."""
    if world != 1:
        return "data parallel (world > 1)"
    if loss_kind not in LOSSES:
        return f"loss {loss_kind!r}"
    if getattr(optimizer, "kind", None) not in KINDS or hasattr(optimizer, "opts"):
        return f"optimizer {getattr(optimizer, 'kind', type(optimizer).__name__)!r} (Adam / AdamW only)"
    layers = dense_layers(model, loss_kind)
    if layers is None:
        return "not a Dense-only stack"
    lins = [m for m, _ in layers]
    if not 1 <= len(lins) <= MAX_LAYERS:
        return f"{len(lins)} layers (1..{MAX_LAYERS})"
    if any(m.bias is None for m in lins):
        return "a layer without a bias"
    if any(getattr(m, "_drop_in", None) for m in lins):
        return "Dropout"
    if max([lins[0].in_features] + [m.out_features for m in lins]) > MAX_WIDTH:
        return f"a width above {MAX_WIDTH}"
    if lins[-1].out_features != 1 or layers[-1][1] is not None:
        return "the last layer is not Linear(*, 1) without activation"
    if any(a not in ACTS for _, a in layers):
        return "a hidden activation other than relu / sigmoid / none"
    if not 1 <= int(B) <= MAX_BATCH:
        return f"batch {B} (1..{MAX_BATCH})"
    arena = getattr(optimizer, "arena", None)
    params = [p for m in lins for p in (m.weight, m.bias)]
    if arena is None or any(getattr(p, "_hx_arena", None) is not arena for p in params) \
            or {id(p) for p in params} != {id(p) for p in arena.params}:
        return "the optimizer's arena is not exactly this model's parameters"
    if optimizer._sl.start != 0 or optimizer._sl.stop != arena.numel or optimizer.grad_scale != 1.0:
        return "a restricted or gradient-scaled optimizer"
    if _C.available() and _C.ext().mlp_step_ok(_ints(layers, B, 1, 1, optimizer.kind, loss_kind)) <= 0:
        return "over the kernel's LDS budget"
    return None


def supported(model, optimizer, loss_kind: str, B: int, world: int = 1) -> bool:
    return why_not(model, optimizer, loss_kind, B, world) is None


class FusedMlpStep:
    """The whole training step of a Dense-only stack as ONE kernel launch of one workgroup (csrc/ops/mlp_step.hip):
    forward, loss (``bce_logits`` / ``mse``), backward, Adam / AdamW, the step counter and the batch cursor of an
    HBM-resident epoch, ``steps_per_execution`` steps a launch with the model and optimizer state on chip.

    Same model, optimizer, arena and results as ``TrainStep(model, optimizer, loss_kind)`` (bf16 operands, fp32
    accumulation), so the two interleave on one arena.  Outputs ``{"loss", "correct", "count"}`` as device tensors."""

    kind, note = "mlp-step", None

    def __init__(self, model, optimizer, loss_kind: str = "bce_logits", steps_per_execution: int = 32):
        self.model, self.opt, self.loss_kind = model, optimizer, loss_kind
        self.layers = dense_layers(model, loss_kind)
        if self.layers is None:
            raise ValueError("FusedMlpStep needs a Dense-only stack")
        self.arena = optimizer.arena
        self.steps_per_execution = max(1, int(os.environ.get("HOPSX_STEPS_PER_EXEC", steps_per_execution)))
        dev = self.arena.device
        self.cursor = torch.zeros(1, device=dev, dtype=torch.int64)
        self._loss = torch.zeros(self.steps_per_execution, device=dev)
        self._correct = torch.zeros(self.steps_per_execution, device=dev, dtype=torch.int32)
        self.trace = None  # a bf16 [trace_elems()] tensor: the kernel stores its last step's images there
        self._slots = ArgSlots(lambda *args: _C.ext().mlp_step_store(*args))
        self._graphs: dict = {}
        self._graph_key = None
        self.use_graph, self.warmup = True, 0  # (TrainStep's attributes: no eager warm-up steps here)
        self._ok: dict = {}
        self._n = 0

    # ------------------------------------------------------------------ queries
    def ok(self, B: int) -> bool:
        r = self._ok.get(B)
        if r is None:
            r = self._ok[B] = self.arena.device.type == "cuda" and supported(self.model, self.opt, self.loss_kind, B)
        return r

    def geometry(self, B: int) -> dict:
        """LDS bytes, where the optimizer state lives, batch tiles and the trace layout of a launch at batch B."""
        g = _C.ext().mlp_step_geom(_ints(self.layers, B, 1, 1, self.opt.kind, self.loss_kind))
        if not g:
            raise ValueError("the kernel does not take this configuration")
        return {"lds_bytes": g[0], "state_in_lds": bool(g[1]), "tiles": g[2], "trace_elems": g[3], "trace_img": g[4]}

    # ------------------------------------------------------------------ launches
    def _outs(self, k: int):
        if k > self._loss.numel():
            self._loss = torch.zeros(k, device=self._loss.device)
            self._correct = torch.zeros(k, device=self._loss.device, dtype=torch.int32)
        return self._loss, self._correct

    def _launch_state(self, xs, ys, nsteps: int) -> tuple:
        """Everything a launch passes to the kernel that can change while the object lives: the argument-slot
        key is this tuple, the graph cache's key the same without ``nsteps``.  xs [nbatch, B, F] is a resident
        epoch (the kernel reads batch ``cursor``), [B, F] one batch."""
        loss, correct = self._outs(nsteps)
        a, o = self.arena, self.opt
        return (nsteps, tuple(float(v) for v in o._hp()), o.kind, self.loss_kind, xs.data_ptr(), ys.data_ptr(),
                tuple(xs.shape), xs.dim() == 3, self.cursor.data_ptr(), loss.data_ptr(), correct.data_ptr(),
                a.master.data_ptr(), _C.ptr(a.shadow), a.state(f"{o.kind}_s0").data_ptr(),
                a.state(f"{o.kind}_s1").data_ptr(), o.step_count.data_ptr(), _C.ptr(o._hp_dev), _C.ptr(self.trace),
                tuple(int(p._hx_off) for m, _ in self.layers for p in (m.weight, m.bias)))

    def _args(self, xs, ys, state: tuple):
        nsteps, fl = state[0], state[1]
        a, o, ptr = self.arena, self.opt, _C.ptr
        resident = xs.dim() == 3
        loss, correct = self._outs(nsteps)
        ptrs = [ptr(a.master), ptr(a.shadow), ptr(a.state(f"{o.kind}_s0")), ptr(a.state(f"{o.kind}_s1")), ptr(xs), ptr(ys),
                ptr(self.cursor if resident else None), ptr(loss), ptr(correct), ptr(o.step_count), ptr(o._hp_dev),
                ptr(self.trace)]
        ints = _ints(self.layers, xs.shape[-2], xs.shape[0] if resident else 1, nsteps, o.kind, self.loss_kind)
        return ptrs, ints, (list(fl) + [0.0] * 8)[:8]

    @staticmethod
    def _f32(t):
        return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()

    def _launch(self, xs, ys, nsteps: int = 1):
        for t in (xs, ys):  # (the kernel reads fp32; a resident epoch is kept that way, never converted per launch)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError("FusedMlpStep: resident xs / ys must be contiguous float32 tensors")
        if not self.ok(xs.shape[-2]):
            raise RuntimeError("FusedMlpStep: " + str(why_not(self.model, self.opt, self.loss_kind, xs.shape[-2])
                                                     or "needs a GPU"))
        self.opt.sync_hp()  # (the kernel reads the device vector; a no-op while capturing)
        state = self._launch_state(xs, ys, nsteps)
        sid = self._slots.get(state, lambda: self._args(xs, ys, state))
        _C.check(_C.ext().mlp_step_slot(sid, _C.stream()), "mlp_step")

    def _result(self, xs, k: int = 1) -> dict:
        return {"loss": self._loss[k - 1:k], "correct": self._correct[k - 1:k], "count": xs.shape[-2]}

    def __call__(self, x, y):
        """One step on an explicit batch x [B, F], y [B(, 1)]."""
        self._n += 1
        health.beat(self._n)
        self._launch(self._f32(x), self._f32(y))
        return self._result(x)

    def _graph(self, xs, ys, k: int):
        """The captured (not run) graph of one k-step launch on this resident epoch; new data, hyper-parameters or
        anything else in ``_launch_state`` drops the cached ones."""
        key = self._launch_state(xs, ys, 0)[1:]
        if self._graph_key != key:
            self._graphs, self._graph_key = {}, key
        if k not in self._graphs:
            self.opt.sync_hp()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _capture_graph(g):
                self._launch(xs, ys, nsteps=k)
            self._graphs[k] = g
        return self._graphs[k]

    def step_resident(self, xs, ys, graph: bool = True):
        """One step on batch ``cursor`` of the resident epoch xs [nb, B, F] fp32, ys [nb, B(, 1)] fp32; the kernel
        advances the cursor.  ``graph``: replay a captured one-step launch."""
        self._n += 1
        health.beat(self._n)
        if graph:
            self.opt.sync_hp()
            self._graph(xs, ys, 1).replay()
        else:
            self._launch(xs, ys)
        return self._result(xs)

    def prepare_resident(self, xs, ys, n: int | None = None) -> None:
        """Build the argument slots of the launches that run ``n`` steps, so none is built in a timed loop."""
        for k in launch_shapes(int(n or self.steps_per_execution), self.steps_per_execution):
            st = self._launch_state(xs, ys, k)
            self._slots.get(st, lambda st=st: self._args(xs, ys, st))

    def run_resident(self, xs, ys, n: int, on_out=None):
        """``n`` consecutive resident steps, ``steps_per_execution`` per launch (direct launches: a one-node graph
        replay costs more host time than the launch it replaces).  ``on_out(list of outputs)`` receives every
        step's outputs once per launch, right after it (device tensors)."""
        U, k = self.steps_per_execution, 1
        while n > 0:
            k = min(n, U)
            health.beat_range(self._n + 1, k)
            self._n += k
            self._launch(xs, ys, nsteps=k)
            if on_out is not None:
                on_out([{"loss": self._loss[i:i + 1], "correct": self._correct[i:i + 1], "count": xs.shape[-2]}
                        for i in range(k)])
            n -= k
        return self._result(xs, k)


# --------------------------------------------------------------------------- the fp64 reference of the step
def _bf(t):
    return t.float().bfloat16().double()


def reference_steps(weights, biases, acts, xs, ys, loss_kind, kind, hp, nsteps, t0=0, m=None, v=None, cursor=0,
                    emulate_bf16=False):
    """``nsteps`` training steps of the Dense stack in plain fp64 on the CPU: ordinary backprop + the
    ``optim.reference_step`` Adam / AdamW rule.  ``weights[l]`` [out, in], ``biases[l]`` [out], ``acts[l]`` in
    {None, "relu", "sigmoid"}; xs [nbatch, B, F], ys [nbatch, B(, 1)], step s trains on batch (cursor + s) % nbatch;
    ``hp`` the kernel's hyper-parameter vector (``optimizer._hp()``); ``m`` / ``v`` the moments as lists shaped
    like weights + biases (zeros when None).  ``emulate_bf16`` rounds where the kernel does: the input, the
    weights the products read, every activation and every hidden gradient (accumulation, biases, the logit
    gradient and the update stay fp64).

    Returns a dict: ``weights``, ``biases``, ``m``, ``v`` (lists), ``loss`` / ``correct`` [nsteps], and of the
    last step ``A`` (the layers' inputs, A[0] = x), ``z`` (the output), ``g`` (dloss/dz), ``G`` (G[l] = the gradient at
    layer l's pre-activation, l < L - 1), ``dW`` / ``db``."""
    from ..optim import reference_step

    rnd = _bf if emulate_bf16 else (lambda t: t)
    W = [w.detach().double().cpu() for w in weights]
    Bs = [b.detach().double().cpu() for b in biases]
    L = len(W)
    zeros = [torch.zeros_like(p) for p in W + Bs]
    m = [t.detach().double().cpu() for t in m] if m is not None else [z.clone() for z in zeros]
    v = [t.detach().double().cpu() for t in v] if v is not None else [z.clone() for z in zeros]
    xs, ys = xs.detach().double().cpu(), ys.detach().double().cpu().reshape(xs.shape[0], -1)
    losses, hits, last = [], [], {}
    for s in range(nsteps):
        bi = (cursor + s) % xs.shape[0]
        A, y = [rnd(xs[bi])], ys[bi]
        nB = y.numel()
        for l in range(L - 1):
            zl = A[-1] @ rnd(W[l]).T + Bs[l]
            A.append(rnd(torch.relu(zl) if acts[l] == "relu" else torch.sigmoid(zl) if acts[l] == "sigmoid" else zl))
        z = A[-1] @ rnd(W[-1])[0] + Bs[-1][0]
        if loss_kind == "mse":
            losses.append(((z - y) ** 2).mean())
            hits.append(torch.zeros(()))
            g = 2 * (z - y) / nB
        else:
            losses.append((z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean())
            hits.append(((z > 0) == (y > 0.5)).sum().double())
            g = (torch.sigmoid(z) - y) / nB
        dW, db, G = [None] * L, [None] * L, [None] * (L - 1)
        dW[-1], db[-1] = (g[:, None] * A[-1]).sum(0)[None, :], g.sum().reshape(1)
        up = g[:, None] * rnd(W[-1])  # dloss/dA[L-1]
        for l in range(L - 2, -1, -1):
            a = A[l + 1]
            d = (a > 0).double() if acts[l] == "relu" else a * (1 - a) if acts[l] == "sigmoid" else torch.ones_like(a)
            G[l] = rnd(up * d)
            dW[l], db[l] = G[l].T @ A[l], G[l].sum(0)
            up = G[l] @ rnd(W[l])
        for j, (p, gr) in enumerate(zip(W + Bs, dW + db)):
            pn, (mn, vn) = reference_step(kind, p, gr, [m[j], v[j]], hp, t0 + s + 1)
            (W if j < L else Bs)[j % L], m[j], v[j] = pn, mn, vn
        last = {"A": A, "z": z, "g": g, "G": G, "dW": dW, "db": db}
    return {"weights": W, "biases": Bs, "m": m, "v": v, "loss": torch.stack(losses), "correct": torch.stack(hits),
            **last}
