"""The training runtime of the Chicago-taxi wide & deep model (models/widedeep.py): the whole step as one
kernel launch (``FusedWideDeepStep``: csrc/ops/taxi_step.hip v2, csrc/ops/widedeep_step.hip v1) and the
cross-rank exchange of its data-parallel instantiation (``TaxiExchange``).

Reference workload: the TFX Chicago-taxi trainer the reference README names (README.md:99-112)."""
from __future__ import annotations

import math
import os

import torch

from .. import nn as hnn
from ..models.widedeep import N_WIDE, TRAIN_BATCH_SIZE, TaxiWideDeep
from ..ops import _C
from ..ops.functional import rng_state
from . import health
from .capture import graph as _capture_graph
from .launch_slots import ArgSlots, launch_shapes
from .peer_exchange import PeerExchange


class TaxiExchange:
    """The cross-rank exchange of the data-parallel v2 taxi step (csrc/ops/taxi_step.hip, DP
    instantiation): this rank's uncached exchange buffer and flag page, every peer's mapped through IPC
    handles exchanged over the default process group (``PeerExchange``; ranks on one node; they may share a
    GPU — the step is one workgroup), the global step counter (exchange epoch base) and a sticky error word.

    Each rank's kernel pushes its dW accumulators and wide-row gradients into every rank's buffer, raises
    its flag word in every peer's page and sums the W ranks' gradients in rank order before the update:
    one cross-rank hop per step and bit-identical replicas, the MirroredStrategy global-batch step of the
    reference's TFX trainer (README.md:99-112) at 2..8 GPUs.  ``loopback=W``: ONE process plays W ranks
    (the peers' buffers are its own), for tests."""

    def __init__(self, device, world: int | None = None, loopback: int = 0, timeout_s: float | None = None):
        from ..parallel import dist as hdist

        self.device = torch.device(device)
        xb, xf, xmax, self.pay = _C.ext().taxi_step2_xgeom()
        self.loopback = int(loopback)
        if self.loopback > 1:
            self.world, self.rank = self.loopback, 0
        else:
            self.world = int(world) if world is not None else hdist.world_size()
            self.rank = hdist.rank() if self.world > 1 else 0
        if not 2 <= self.world <= xmax:
            raise ValueError(f"the data-parallel taxi step takes 2..{xmax} ranks")
        self.timeout_ms = int(1000 * float(timeout_s or os.environ.get("HOPSX_TAXI_DP_TIMEOUT_S", "60")))
        self._px = PeerExchange(self.device, xb, xf, self.world, self.rank, loopback=self.loopback > 1, name="taxi")
        self.bufs, self.flags = self._px.bufs, self._px.flags
        self.xstep = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.err = torch.zeros(4, device=self.device, dtype=torch.int32)

    def ptrs(self) -> list[int]:
        """The kernel's data-parallel pointer tail (taxi_step.hip hopsx_taxi_step2)."""
        mode = self.world | (self.rank << 8) | ((1 if self.loopback > 1 else 0) << 16)
        return [mode, self.timeout_ms, self.err.data_ptr(), self.xstep.data_ptr()] + list(self.bufs) + list(self.flags)

    def sync_replicas(self, arena) -> None:
        """Collective: every replica starts from rank 0's parameters and optimizer state."""
        import torch.distributed as dist

        if self.loopback > 1:
            return
        gloo = dist.get_backend() == "gloo"  # (rehearsals: ranks sharing a GPU; gloo broadcasts host copies)
        for t in [arena.master] + [arena.state(k) for k in ("adagrad_s0", "ftrl_s0", "ftrl_s1")]:
            if gloo:
                h = t.cpu()
                dist.broadcast(h, 0)
                t.copy_(h)
            else:
                dist.broadcast(t, 0)
        if arena.shadow is not None:
            arena.shadow.copy_(arena.master.to(arena.shadow.dtype))
        torch.cuda.synchronize(self.device)
        dist.barrier()

    def replicas_agree(self, digest) -> bool:
        """Collective: did every rank pass the same ``digest`` (``FusedWideDeepStep.digest``)?"""
        import torch.distributed as dist

        digs = [None] * self.world
        dist.all_gather_object(digs, digest)
        return all(d == digs[0] for d in digs)

    def check(self) -> None:
        e = int(self.err[0].item()) & 0xFFFFFFFF
        if e:
            raise RuntimeError(f"taxi DP: a peer's gradients did not arrive within {self.timeout_ms} ms "
                               f"(step {e & 0xFFFFFF} of its launch); the replicas' state is partial")

    def close(self) -> None:
        self._px.close()


class FusedWideDeepStep:
    """The whole taxi training step as ONE kernel launch (csrc/ops/widedeep_step.hip): forward,
    sigmoid cross-entropy, backward, FTRL (wide) + Adagrad (deep) updates, step counters and the
    batch cursor of an HBM-resident epoch — one workgroup holding the model and the batch in LDS.

    Same model, optimizers and results as ``TrainStep(model, make_optimizer(model), "bce_logits")``
    (fp32 GEMMs instead of bf16).  Data-parallel, two forms: ``xdp`` (a :class:`TaxiExchange`) runs the
    v2 kernel's data-parallel instantiation — the replicas exchange gradients inside the launch and
    update in registers, "fused-v2-dp"; ``dp`` (a DataParallel engine): the v1 kernel stops at the
    gradients, which are all-reduced and applied by the regular optimizer kernels.  ``ok()`` says whether
    the model/batch fit one workgroup's LDS; otherwise use TrainStep."""

    def __init__(self, model: TaxiWideDeep, optimizer, dp=None, xdp: "TaxiExchange | None" = None):
        self.model, self.opt, self.dp, self.xdp = model, optimizer, dp, xdp
        if dp is not None and xdp is not None:
            raise ValueError("dp (v1 + all-reduce) and xdp (in-kernel exchange) are exclusive")
        self.arena = model.wide.weight._hx_arena
        self.ftrl, self.ada = optimizer.opts
        lins = [m for m in model.deep if isinstance(m, hnn.Linear)]
        self.lins = lins
        self.dims = [lins[0].weight.shape[1]] + [m.weight.shape[0] for m in lins]
        self.acts_ok = (all(m.activation == "relu" for m in lins[:-1]) and lins[-1].activation is None
                        and all(m.bias is not None for m in lins))
        if dp is not None:
            optimizer.grad_scale = dp.grad_scale()
        # captured graphs: steps per replay -> graph, all of them for the launch state _graph_key
        # (_launch_state without the step count); None until the first capture
        self._graphs: dict = {}
        self._graph_key = None
        # steps per replayed graph; on one GPU they run inside ONE launch (widedeep_step.hip nsteps)
        self.steps_per_execution = max(1, int(os.environ.get("HOPSX_TAXI_STEPS_PER_EXEC",
                                                             os.environ.get("HOPSX_STEPS_PER_EXEC", "32"))))
        self._slot_cache = {}
        self._n = 0
        self._B = None
        self._v2: dict = {}
        self._zn = None
        # cached v2 launch arguments: _launch_state -> C++ slot
        self._v2slots = ArgSlots(lambda *args: _C.ext().taxi_step2_store(*args))
        dev = self.arena.device
        self.loss = torch.zeros(1, device=dev)
        self.correct = torch.zeros(1, device=dev, dtype=torch.int32)
        self.cursor = torch.zeros(1, device=dev, dtype=torch.int64)
        # HOPSX_PHASE_DBG=1: the kernel stamps its phase boundaries here (tools/taxi_phases.py)
        self.dbg = (torch.zeros(32, device=dev, dtype=torch.int64)
                    if os.environ.get("HOPSX_PHASE_DBG") == "1" else None)

    def _ints(self, B: int, nbatch: int, nsteps: int = 1) -> list[int]:
        L = len(self.lins)
        iv = ([L, B, nbatch, N_WIDE, int(self.model.wide.weight._hx_off), int(self.dp is None), 2] + self.dims
              + [int(m.weight._hx_off) for m in self.lins] + [int(m.bias._hx_off) for m in self.lins])
        return iv + [int(nsteps)] if nsteps > 1 else iv

    def ok(self, B: int) -> bool:
        dev = self.arena.device
        if self.xdp is not None:  # the in-kernel exchange exists in the v2 kernel only
            return dev.type == "cuda" and self.v2(B)
        return (dev.type == "cuda" and self.acts_ok and self.dims[-1] == 1
                and (self.v2(B) or _C.ext().widedeep_step_lds(self._ints(B, 1)) > 0))

    def check(self) -> None:
        """Raise if the data-parallel exchange of any launch failed (sticky device error word)."""
        if self.xdp is not None:
            self.xdp.check()

    def digest(self) -> tuple[float, int]:
        """(sum, integer bit-sum) of the fp32 arena: equal on every replica iff the replicas agree."""
        m = self.arena.master
        return float(m.double().sum()), int(m.view(torch.int32).long().sum())

    def v2(self, B: int) -> bool:
        """The v2 kernel (csrc/ops/taxi_step.hip: bf16 MFMA, wide table + optimizer state on chip) takes
        the default taxi shape on one GPU; HOPSX_TAXI_KERNEL=v1 forces the fp32 v1 kernel."""
        key = (B, self.dp is None, os.environ.get("HOPSX_TAXI_KERNEL", "v2"), self.xdp is not None)
        r = self._v2.get(key)
        if r is None:
            r = (self.dp is None and key[2] != "v1" and self.acts_ok and self.arena.device.type == "cuda"
                 and _C.ext().taxi_step2_ok(self._ints(B, 1), int(self.model.wide.weight.shape[0])) > 0)
            self._v2[key] = r
        return r

    def _kernel(self, B: int) -> str:
        k = "v2" if self.v2(B) else "v1"
        return k + "-dp" if self.xdp is not None and k == "v2" else k

    @property
    def kernel(self) -> str:
        return self._kernel(self._B or TRAIN_BATCH_SIZE)

    def _slots(self, B: int):
        """Host-built table: LDS slot of every deep arena element for batch size B (cached)."""
        t = self._slot_cache.get(B)
        if t is None:
            lo = int(self.lins[0].weight._hx_off)
            hi = int(self.lins[-1].bias._hx_off) + self.dims[-1]
            host = torch.empty(hi - lo, dtype=torch.int32)
            _C.check(_C.ext().widedeep_slots(self._ints(B, 1), host.data_ptr(), hi - lo), "widedeep_slots")
            t = host.to(self.arena.device)
            self._slot_cache[B] = t
        return t

    def _floats(self) -> list[float]:
        def pad8(v):
            return [float(x) for x in v] + [0.0] * (8 - len(v))

        self.ada.lr = self.ada.param_groups[0]["lr"]
        self.ftrl.lr = self.ftrl.param_groups[0]["lr"]
        return pad8(self.ada._hp()) + pad8(self.ftrl._hp())

    def _launch_state(self, dense, cat, ys, nsteps: int) -> tuple:
        """(nsteps, the hyper-parameter floats, the kernel, ...): every scalar or identity ``_launch`` and ``_args``
        read that can change while the object lives.  The v2 argument-slot key is this tuple and the graph
        cache's key the same without ``nsteps``: a field the launch starts to read has this one place to go.
        ``dense`` [nbatch, B, 3] is a resident epoch (the kernel reads batch ``cursor``), [B, 3] one batch."""
        return (nsteps, tuple(self._floats()), self._kernel(dense.shape[-2]), dense.data_ptr(), cat.data_ptr(),
                ys.data_ptr(), dense.shape, self.cursor.data_ptr() if dense.dim() == 3 else None,
                os.environ.get("HOPSX_TAXI_INKERNEL_LOOP", "1"), id(self.dbg), id(self.xdp), id(self.arena.master),
                self.dp is not None)

    def _args(self, dense, cat, label, state: tuple):
        """(ptrs, ints, floats) of a v1 launch, (ptrs, ints, floats, wide rows) of a v2 launch."""
        nsteps, fl, kernel = state[:3]
        a, ptr = self.arena, _C.ptr
        B = dense.shape[-2]
        resident = dense.dim() == 3
        ptrs = [ptr(a.master), ptr(a.grad), ptr(a.shadow), ptr(a.state("adagrad_s0")), ptr(a.state("ftrl_s0")),
                ptr(a.state("ftrl_s1")), ptr(dense), ptr(cat), ptr(label), ptr(self.cursor if resident else None),
                ptr(self.loss), ptr(self.correct), ptr(self.ada.step_count), ptr(self.ftrl.step_count),
                ptr(rng_state(a.device)), ptr(self.dbg)]
        ints = self._ints(B, dense.shape[0] if resident else 1, nsteps)
        if kernel == "v1":
            return ptrs + [ptr(self._slots(B))], ints, list(fl)
        rows = int(self.model.wide.weight.shape[0])
        if self._zn is None:
            self._zn = torch.empty(rows, 2, device=a.device)  # the kernel's (z, n) scratch
        # Adagrad as w -= lr g rsq(s) (one transcendental): exact to fp32 when wd == 0 and eps is
        # below the resolution of sqrt(s), whose floor is the initial accumulator
        floor = float(getattr(self.ada, "initial_accumulator_value", 0.0))
        rsq = int(self.ada.weight_decay == 0 and floor > 0 and self.ada.hp["eps"] < 1e-7 * math.sqrt(floor))
        ptrs += [ptr(self._zn), rsq]
        if self.xdp is not None:
            ptrs += self.xdp.ptrs()
        return ptrs, ints, list(fl), rows

    def _v2_slot(self, dense, cat, label, state: tuple) -> int:
        """The C++-side argument slot of this v2 launch, built once per ``_launch_state`` (a run has a few: warm-up,
        steps_per_execution, the remainder), so no argument vector is rebuilt inside a timed loop."""
        return self._v2slots.get(state, lambda: self._args(dense, cat, label, state))

    def _launch(self, dense, cat, label, nsteps: int = 1):
        self._B = dense.shape[-2]
        state = self._launch_state(dense, cat, label, nsteps)
        if state[2] != "v1":
            _C.check(_C.ext().taxi_step2_slot(self._v2_slot(dense, cat, label, state), _C.stream()), "taxi_step2")
        else:
            _C.check(_C.ext().widedeep_step(*self._args(dense, cat, label, state), _C.stream()), "widedeep_step")

    def _finish(self):
        if self.dp is not None:
            self.dp.allreduce_all()
            self.opt.step()
            if hasattr(self.dp, "post_step"):
                self.dp.post_step()

    def _result(self, dense) -> dict:
        return {"loss": self.loss, "correct": self.correct, "count": dense.shape[-2]}

    def __call__(self, x, y):
        """One step on an explicit batch: x = (dense [B, 3], cat [B, 13] int64), y [B, 1]."""
        self._n += 1
        health.beat(self._n)
        dense, cat = x
        self._launch(dense.float().contiguous(), cat.contiguous(), y.float().contiguous())
        self._finish()
        return self._result(dense)

    def step_resident(self, xs, ys, graph: bool = True):
        """One step on batch ``cursor`` of a resident epoch xs = (dense [nb, B, 3] fp32, cat [nb, B, 13]),
        ys [nb, B, 1]; the kernel advances the cursor.  Single-GPU steps replay a captured graph."""
        self._n += 1
        health.beat(self._n)
        dense, cat = xs
        if not graph or not self._graphable():
            self._launch(dense, cat, ys)
            self._finish()
        else:
            self._graph(dense, cat, ys, 1).replay()  # (capture does not execute: the step runs through the graph)
            if self.dp is not None:
                self.dp.poll()
        return self._result(dense)

    def _direct(self, dense) -> bool:
        """Single-GPU v2 step with its in-kernel step loop: launched directly (``HOPSX_TAXI_DIRECT=0``
        keeps the graph replays)."""
        return (self.dp is None and self.arena.device.type == "cuda" and self.v2(dense.shape[-2])
                and os.environ.get("HOPSX_TAXI_INKERNEL_LOOP", "1") == "1"
                and os.environ.get("HOPSX_TAXI_DIRECT", "1") == "1")

    def _graphable(self) -> bool:
        """One GPU, or a data-parallel engine whose collectives are graph-capturable (P2P kernels)."""
        return self.arena.device.type == "cuda" and (
            self.dp is None or getattr(self.dp, "capturable", lambda: False)())

    def _sync_hp(self):
        if self.dp is not None and hasattr(self.opt, "sync_hp"):
            self.opt.sync_hp()

    def _graph_cache(self, dense, cat, ys) -> dict:
        """The captured graphs of this launch state; new data, hyper-parameters (e.g. an lr schedule), kernel
        choice or anything else in ``_launch_state`` drops them all."""
        key = self._launch_state(dense, cat, ys, 0)[1:]
        if self._graph_key != key:
            self._graphs, self._graph_key = {}, key
        return self._graphs

    def _graph(self, dense, cat, ys, k: int):
        """The graph of ``k`` consecutive steps on this resident epoch, captured (not run) if there is none."""
        graphs = self._graph_cache(dense, cat, ys)
        if k not in graphs:
            graphs[k] = self._capture(dense, cat, ys, k)
        return graphs[k]

    def _capture(self, dense, cat, ys, k: int):
        """k consecutive steps in one graph: ONE launch running k steps in-kernel on one GPU (the
        weights stay on chip between them); k launches + gradient exchanges when data-parallel (the P2P
        all-reduce + optimizers are graph nodes too)."""
        if not self.v2(dense.shape[-2]):
            self._slots(dense.shape[-2])  # host->device copy of the slot table must precede capture
        self._sync_hp()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _capture_graph(g):
            if self.dp is None and os.environ.get("HOPSX_TAXI_INKERNEL_LOOP", "1") == "1":
                self._launch(dense, cat, ys, nsteps=k)
            else:
                for _ in range(k):
                    self._launch(dense, cat, ys)
                    self._finish()
        return g

    def _multi_step_graphs(self) -> bool:
        """Multi-step graphs come after the engine's first graph step (a one-step graph)."""
        return self.steps_per_execution > 1 and self._graphable() and self._graph_key is not None

    def prepare_resident(self, xs, ys, n: int | None = None) -> None:
        """Capture (not run) the U-step graph for this resident epoch, so it is built before a timed
        loop; with ``n`` also the graph of the remainder n % U (Keras steps_per_execution tail)."""
        dense, cat = xs
        U = self.steps_per_execution
        if n and self._direct(dense):
            # direct launches (run_resident): their argument slots for the launch shapes of n steps
            for k in launch_shapes(int(n), U):
                self._v2_slot(dense, cat, ys, self._launch_state(dense, cat, ys, k))
            return
        if not self._multi_step_graphs():
            return
        for k in {U, (n or 0) % U} - {0, 1}:
            self._graph(dense, cat, ys, k)

    def run_resident(self, xs, ys, n: int, graph: bool = True):
        """``n`` consecutive resident steps, ``steps_per_execution`` (U) per launch or graph replay (Keras
        steps_per_execution; the kernel advances the device cursor), so the per-launch gap is paid once per U
        steps.  One GPU, whole steps in one kernel: launches of U, U, ..., n % U steps, issued directly (a
        one-node graph replay costs more host time than the launch it replaces) with the argument vectors
        kept in a C++ slot.  Otherwise graph replays: full chunks replay the U-step graph, a remainder its
        graph if ``prepare_resident(xs, ys, n)`` built one, everything else single steps."""
        U = self.steps_per_execution
        dense, cat = xs
        direct = graph and self._direct(dense)
        while n > 0:
            g = None
            if direct:
                k = min(n, U)
            elif graph and self._multi_step_graphs() and (n >= U or (n > 1 and n in self._graph_cache(dense, cat, ys))):
                k = min(n, U)
                g = self._graph(dense, cat, ys, k)
            else:
                self.step_resident(xs, ys, graph=graph)
                n -= 1
                continue
            health.beat_range(self._n + 1, k)
            self._n += k
            if direct:
                self._launch(dense, cat, ys, nsteps=k)
            else:
                g.replay()
                if self.dp is not None:
                    self.dp.poll()
            n -= k
        return self._result(dense)
