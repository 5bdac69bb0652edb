"""CnnFamilyEvaluator: the E1 / E8 / E9 / E11 CNN family evaluated over a whole resident set in one launch.

Reference workload: ``model.evaluate`` / ``predict`` / per-epoch validation of the stacks whose conv kernel and
pool size are the searched hyper-parameters (models/zoo.py ``keras_mnist_cnn`` / ``fashion_mnist_cnn``,
models/mnist.py ``KerasMnistCNN`` / ``FashionMnistCNN``; maggy's Searchspace in
examples/ml/Parallel_Experiments/maggy_fashion_mnist.py: kernel and pool in [2, 8]).

csrc/ops/cnn_eval.hip runs the forward (dropout off) of N uint8 images in ONE launch for any k, p in [2, 8] and
'valid' or TF-'same' padding — a workgroup per tile of ``plan.tile`` images, nothing handed between workgroups —
and leaves logits, per-image sparse softmax CE, per-image hits and their totals in device memory.  The contract
is ``persist_eval.MnistEvaluator``'s: no host sync inside ``run``, an image's outputs depend only on that image
and the weights, deterministic totals, a label outside [0, 10) gives loss 0 / hit 0 and is reported by
``kernels.debug_errors()`` under ``cnn_eval``, and no cached weights: every call reads the ParamArena in stream
order.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch
from torch import nn

from .persist_eval import PARAMS, EvalResult, _arena_of, _ext


@dataclass(frozen=True)
class Plan:
    """The launcher's own decision for one geometry (``hopsx_cnn_eval_plan``)."""
    tile: int         # images per workgroup tile
    s: int            # pooled size
    in_features: int  # fc1 in-features, s * s * 64
    lds: int          # dynamic LDS bytes


class FamilyView(nn.Module):
    """The five layers of a matching stack under the names the arena offsets are looked up by."""

    def __init__(self, conv1, conv2, pool, fc1, fc2):
        super().__init__()
        self.conv1, self.conv2, self.pool, self.fc1, self.fc2 = conv1, conv2, pool, fc1, fc2


def pooled_size(k: int, p: int, pad: int) -> int:
    return (28 if pad else 30 - 2 * k) // p


def family_layers(model):
    """``((conv1, conv2, pool, fc1, fc2), k, p, pad)`` when ``model`` has the family's structure — Conv 1->32 and
    Conv 32->64 with the same square k in [2, 8] (relu, bias, stride 1, dilation 1, both 'valid' or both 'same',
    the uint8 input affine on conv1), MaxPool p in [2, 8] with stride p and no padding, Dense(s*s*64 -> 128, relu),
    Dense(128 -> 10) — matched on the layers, not on the class; else None.  Dropout modules do not matter:
    inference never drops."""
    from .. import nn as hnn
    from ..models import mnist as M

    L = [getattr(model, n, None) for n in ("conv1", "conv2", "pool", "fc1", "fc2")]
    if any(x is None for x in L):
        return None
    c1, c2, pool, f1, f2 = L

    def pad_of(c):
        pd = c.cfg.get("padding", 0)
        return 1 if pd == "same" else 0 if pd in (0, "valid", (0, 0)) else None

    def conv_ok(c, cin, cout):
        return (isinstance(c, hnn.Conv2d) and c.in_channels == cin and c.out_channels == cout
                and c.kernel_size[0] == c.kernel_size[1] and c.activation == "relu" and c.bias is not None
                and c.cfg.get("stride", 1) in (1, (1, 1)) and c.cfg.get("dilation", 1) in (1, (1, 1))
                and pad_of(c) is not None)

    def dense_ok(d, fin, fout, act):
        return (isinstance(d, hnn.Linear) and tuple(d.weight.shape) == (fout, fin) and d.activation == act
                and d.bias is not None)

    if not (conv_ok(c1, 1, 32) and conv_ok(c2, 32, 64) and c1.in_affine is not None
            and isinstance(pool, hnn.MaxPool2d) and isinstance(pool.k, int)):
        return None
    k, p, pad = c1.kernel_size[0], pool.k, pad_of(c1)
    if not (c2.kernel_size[0] == k and pad_of(c2) == pad and 2 <= k <= 8 and 2 <= p <= 8
            and pool.s in (None, p) and not pool.p):
        return None
    if not (dense_ok(f1, pooled_size(k, p, pad) ** 2 * 64, 128, "relu") and dense_ok(f2, 128, 10, None)):
        return None
    # the forward must be exactly that chain: a view of the layers, or one of the reference model classes
    chain = (M.KerasMnistCNN.forward, M.FashionMnistCNN.forward, M.MirroredMnistCNN.forward)
    if not (isinstance(model, FamilyView) or type(model).forward in chain):
        return None
    return L, k, p, pad


def enabled() -> bool:
    """Opt-in: ``HOPSX_EVAL_FAMILY`` set to anything but "0"."""
    return os.environ.get("HOPSX_EVAL_FAMILY", "0") != "0"


class CnnFamilyEvaluator:
    @staticmethod
    def supported(model) -> bool:
        """The model has the family's structure (``family_layers``) and lives in a CUDA ParamArena with a bf16
        shadow.  Opt-in: callers stay on the batch-by-batch forward unless ``HOPSX_EVAL_FAMILY=1`` (anything
        but "0") is set — the engine lost to batch 1024 at k = p = 8 'same' (profiles/r22_cnn_eval.txt)."""
        if not enabled() or family_layers(model) is None:
            return False
        a = _arena_of(model)
        return a is not None and a.device.type == "cuda" and a.shadow is not None

    def __init__(self, model, max_workgroups: int = 0):
        """``max_workgroups``: cap of the launch grid (0: two workgroups per CU); results do not depend on it."""
        fam = family_layers(model)
        if fam is None or _arena_of(model) is None:
            raise ValueError("CnnFamilyEvaluator needs a family CNN in a ParamArena (see supported())")
        self.model = model
        _, self.k, self.p, self.pad = fam
        self.max_workgroups = int(max_workgroups)
        self.launches = 0
        pl = _ext().cnn_eval_plan(self.k, self.p, self.pad)
        if len(pl) != 4 or pl[2] != model.fc1.weight.shape[1]:
            raise ValueError(f"cnn_eval has no plan for k={self.k} p={self.p} pad={self.pad}")
        self.plan = Plan(*(int(v) for v in pl))
        self.tile = self.plan.tile

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
        torch's current stream; with ``ys`` (int64 [n]) also loss / hit / totals.  ``out``: a previous result of
        the same n (and with / without labels) whose buffers are overwritten — nothing is allocated then, so the
        call can be captured into a graph.  n = 0 launches nothing."""
        from ..ops import _C

        a = _arena_of(self.model)
        if a is None or a.shadow is None or a.device.type != "cuda":
            raise RuntimeError("CnnFamilyEvaluator: the model's parameters are not in a CUDA ParamArena with a "
                               "bf16 shadow")
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
        offs = [int(named[q]._hx_off) for q in PARAMS]
        scale, shift = self.model.conv1.in_affine
        ptrs = [a.master.data_ptr(), a.shadow.data_ptr(), xs.data_ptr(), _C.ptr(ys), out.logits.data_ptr(),
                _C.ptr(out.loss), _C.ptr(out.hit), _C.ptr(out.totals), _C.ptr(out._part)]
        # the affine as float pairs hi + lo: conv1 runs in fp64 (the binding carries floats)
        hi = [torch.tensor(float(v), dtype=torch.float32).item() for v in (scale, shift)]
        rc = _ext().cnn_eval(ptrs, offs + [n, self.max_workgroups, self.k, self.p, self.pad],
                             hi + [float(scale) - hi[0], float(shift) - hi[1]], _C.stream())
        _C.check(rc, "cnn_eval")
        self.launches += 1
        return out


def reference_logits(P: dict, x_u8: torch.Tensor, k: int, p: int, pad: int, xscale: float = 1.0 / 255.0,
                     xshift: float = 0.0, emulate_bf16: bool = True,
                     dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """``persist_eval.reference_logits`` with the geometry as arguments: logits [N, 10] of ``x_u8``
    [N, 28, 28(, 1)] in ``dtype`` from the parameters P (name -> tensor, hopsx layouts: conv OHWI, fc1 over the
    NHWC flatten).  ``pad`` = 1 is TF 'same': (k - 1) // 2 zeros before, the rest after, of the NORMALISED image
    and of conv1's output.  ``emulate_bf16`` rounds exactly what the kernel stores as bf16 MFMA operands (conv1
    output, conv2 weight, the relu'd conv2 output, the fc1 weight).  The kernel computes conv1 in fp64 too (another
    summation order, then double -> float -> bf16), so its conv1 operands differ from this function's
    ``dtype=float64`` ones only where an fp64 sum lands within ~1e-16 relative of a rounding boundary."""
    import torch.nn.functional as F

    rf = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if emulate_bf16 else (lambda t: t)
    lo = (k - 1) // 2 if pad else 0
    hi = k - 1 - lo if pad else 0
    with torch.no_grad():
        P = {q: v.detach().to(dtype) for q, v in P.items()}
        N = x_u8.shape[0]
        x = x_u8.reshape(N, 1, 28, 28).to(dtype) * xscale + xshift
        h = rf(F.relu(F.conv2d(F.pad(x, (lo, hi, lo, hi)), P["conv1.weight"].permute(0, 3, 1, 2), P["conv1.bias"])))
        h = F.conv2d(F.pad(h, (lo, hi, lo, hi)), rf(P["conv2.weight"]).permute(0, 3, 1, 2), P["conv2.bias"])
        h = F.max_pool2d(rf(F.relu(h)), p).permute(0, 2, 3, 1).reshape(N, -1)  # floor windows, NHWC flatten
        h = F.relu(F.linear(h, rf(P["fc1.weight"])) + P["fc1.bias"])
        return F.linear(h, P["fc2.weight"], P["fc2.bias"])
