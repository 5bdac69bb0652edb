"""MnistEvaluator: the flagship MirroredStrategy MNIST CNN evaluated over a whole resident set in one launch.

Reference workload: the evaluate / predict / validation steps of the reference notebooks (SURVEY §3.1
``model.evaluate``; examples/ml/Experiment/keras_mnist.py:31; the validation steps of
examples/ml/Distributed_Training/mirrored_mnist_tfrecord.py) on the model of
mirroredstrategy_mnist_example.ipynb:189-207.

The training side of this model runs 32 steps per launch (runtime/persist.py); this is its inference
side: csrc/ops/mnist_eval.hip runs the forward (dropout off) of N uint8 images in ONE launch — a
workgroup per tile of 32 images, no hand-off between workgroups, so it needs no co-residency and runs on
a partitioned GPU — and leaves logits, per-image sparse softmax CE, per-image hits and their totals in
device memory.  No host sync inside ``run``; the caller reads ``totals`` when it wants the numbers.

Contract: an image's outputs depend only on that image and the weights (bit-identical for any N, any
position in the set, any grid size); ``totals`` is deterministic (fixed-order sums, no float atomics); a
label outside [0, 10) gives loss 0 / hit 0 and is reported by ``kernels.debug_errors()``.  The evaluator
caches no weights: every call reads the model's ParamArena (fp32 master + bf16 shadow), in stream order.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from .persist import PersistentMnistStep, flagship_layers

PARAMS = PersistentMnistStep.PARAMS


@dataclass
class EvalResult:
    """Device tensors of one ``MnistEvaluator.run``: ``logits`` fp32 [n, 10]; with labels also ``loss`` fp32 [n]
    (per-image sparse softmax CE), ``hit`` uint8 [n] (argmax == label, lowest index on a tie) and
    ``totals`` fp32 [2] = {sum of loss, hits}; else those are None."""
    logits: torch.Tensor
    loss: torch.Tensor | None
    hit: torch.Tensor | None
    totals: torch.Tensor | None
    n: int
    _part: torch.Tensor | None = None  # per-tile partials of totals (kernel workspace)


def _ext():
    from ..ops import _C

    return _C.ext()


def _arena_of(model):
    """The one ParamArena all 8 flagship parameters live in, or None."""
    named = dict(model.named_parameters())
    arenas = {id(getattr(named.get(k), "_hx_arena", None)) for k in PARAMS}
    a = getattr(named.get(PARAMS[0]), "_hx_arena", None)
    return a if a is not None and len(arenas) == 1 else None


class MnistEvaluator:
    @staticmethod
    def supported(model) -> bool:
        """The model has the flagship structure (``persist.flagship_layers``) and lives in a CUDA ParamArena
        with a bf16 shadow; ``HOPSX_EVAL_FUSED=0`` keeps callers on the multi-kernel forward.  No
        co-residency check: the kernel's workgroups hand nothing to each other."""
        if os.environ.get("HOPSX_EVAL_FUSED", "1") == "0":
            return False
        if flagship_layers(model) is None:
            return False
        a = _arena_of(model)
        return a is not None and a.device.type == "cuda" and a.shadow is not None

    def __init__(self, model, max_workgroups: int = 0):
        """``max_workgroups``: cap of the launch grid (0: two workgroups per CU); results do not depend on it."""
        if flagship_layers(model) is None or _arena_of(model) is None:
            raise ValueError("MnistEvaluator needs the flagship MNIST CNN in a ParamArena (see supported())")
        self.model = model
        self.max_workgroups = int(max_workgroups)
        self.launches = 0
        self.tile = int(_ext().mnist_eval_tile())

    def _alloc(self, n: int, labels: bool, dev) -> EvalResult:
        f32 = dict(device=dev, dtype=torch.float32)
        logits = torch.empty((n, 10), **f32)
        if not labels:
            return EvalResult(logits, None, None, None, n)
        ntiles = -(-n // self.tile)
        return EvalResult(logits, torch.empty(n, **f32), torch.empty(n, device=dev, dtype=torch.uint8),
                          torch.zeros(2, **f32), n, torch.empty(2 * max(ntiles, 1), **f32))

    def run(self, xs: torch.Tensor, ys: torch.Tensor | None = None, out: EvalResult | None = None) -> EvalResult:
        """Forward of ``xs`` (uint8 [n, 28, 28(, 1)], contiguous, on the model's device) in one launch on
        torch's current stream; with ``ys`` (int64 [n]) also loss / hit / totals.  ``out``: a previous
        result of the same n (and with / without labels) whose buffers are overwritten — nothing is
        allocated then, so the call can be captured into a graph.  n = 0 launches nothing."""
        from ..ops import _C

        a = _arena_of(self.model)
        if a is None or a.shadow is None or a.device.type != "cuda":
            raise RuntimeError("MnistEvaluator: the model's parameters are not in a CUDA ParamArena with a bf16 shadow")
        dev = a.device
        if (xs.dtype != torch.uint8 or xs.device != dev or not xs.is_contiguous()
                or tuple(xs.shape[1:]) not in ((28, 28), (28, 28, 1))):
            raise ValueError(f"xs must be a contiguous uint8 [n, 28, 28(, 1)] tensor on {dev}, got "
                             f"{xs.dtype} {tuple(xs.shape)} on {xs.device}")
        n = int(xs.shape[0])
        if ys is not None and (ys.dtype != torch.int64 or tuple(ys.shape) != (n,) or ys.device != dev
                               or not ys.is_contiguous()):
            raise ValueError(f"ys must be a contiguous int64 [{n}] tensor on {dev}")
        if out is None:
            out = self._alloc(n, ys is not None, dev)
        elif out.n != n or (out.totals is None) != (ys is None) or out.logits.device != dev:
            raise ValueError("out= must come from a run of the same n, with / without labels alike")
        if n == 0:
            return out
        named = dict(self.model.named_parameters())
        offs = [int(named[k]._hx_off) for k in PARAMS]
        scale, shift = self.model.conv1.in_affine
        ptrs = [a.master.data_ptr(), a.shadow.data_ptr(), xs.data_ptr(), _C.ptr(ys), out.logits.data_ptr(),
                _C.ptr(out.loss), _C.ptr(out.hit), _C.ptr(out.totals), _C.ptr(out._part)]
        rc = _ext().mnist_eval(ptrs, offs + [n, self.max_workgroups], [float(scale), float(shift)], _C.stream())
        _C.check(rc, "mnist_eval")
        self.launches += 1
        return out


def reference_logits(P: dict, x_u8: torch.Tensor, xscale: float = 1.0 / 255.0, xshift: float = -0.5,
                     emulate_bf16: bool = True, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The forward half of ``persist.reference_grads`` without dropout: logits [N, 10] of ``x_u8``
    [N, 28, 28(, 1)] in ``dtype`` from the parameters P (name -> tensor, hopsx layouts).  ``emulate_bf16``
    rounds exactly what the kernels store as bf16 MFMA operands (conv1 output, conv2 weight, the relu'd
    conv2 output, the fc1 weight).  ``dtype=torch.float32`` is the fp32 proxy of the kernel's arithmetic:
    its distance to the fp64 result measures what fp32 accumulation (and the bf16 rounding flips it
    causes) can do."""
    import torch.nn.functional as F

    rf = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if emulate_bf16 else (lambda t: t)
    with torch.no_grad():
        P = {k: v.detach().to(dtype) for k, v in P.items()}
        N = x_u8.shape[0]
        x = x_u8.reshape(N, 1, 28, 28).to(dtype) * xscale + xshift
        h = rf(F.relu(F.conv2d(x, P["conv1.weight"].permute(0, 3, 1, 2), P["conv1.bias"])))
        h = rf(F.relu(F.conv2d(h, rf(P["conv2.weight"]).permute(0, 3, 1, 2), P["conv2.bias"])))
        h = F.max_pool2d(h, 2).permute(0, 2, 3, 1).reshape(N, -1)  # NHWC flatten
        h = F.relu(F.linear(h, rf(P["fc1.weight"])) + P["fc1.bias"])
        return F.linear(h, P["fc2.weight"], P["fc2.bias"])
