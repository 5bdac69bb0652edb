"""TaxiEvaluator: the Chicago-taxi wide & deep model evaluated over a whole resident split in one launch,
with TFMA-style metrics overall and per slice of one feature.

Reference workload: the Evaluator / model-analysis stage of the reference's TFX Chicago-taxi pipeline
(README.md:99-112, "all the way from data preparation to model analysis"): metrics per slice of
a feature (``trip_start_hour`` in the TFX example) — accuracy, log-loss, calibration, a bucketed AUC.

The training side of this model is one persistent kernel (csrc/ops/taxi_step.hip); this is its inference
side: csrc/ops/taxi_eval.hip runs the forward of N rows in ONE launch — a wave per 16-row tile, nothing
crossing workgroups but integer atomics, so it needs no co-residency — and leaves per-row logit /
probability / loss / hit plus integer accumulators (a 1,024-bin probability histogram per label, hit counts,
2^-24 fixed-point sums of loss and probability; overall and per slice) in device memory.  No host sync
inside ``run``; ``metrics`` makes one small device-to-host copy of the accumulators.

Contract: a row's outputs depend only on that row and the weights (bit-identical for any n, any position,
any grid size); the accumulators are integers, so they do not depend on atomic order or grid size; a wide
id outside the table adds nothing, a slice id outside its column's range leaves the row out of every slice
(both reported by ``kernels.debug_errors()`` under ``taxi_eval``).  The evaluator caches no weights: every
call reads the model's ParamArena (fp32 master + bf16 shadow) in stream order.

``metrics_from_rows`` computes the same dictionary in numpy from per-row arrays (same bin rule, same fixed
point, same AUC formula): the CPU path of the pipeline, and the oracle of the accumulators.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from ..models.widedeep import (BUCKET_FEATURE_KEYS, CATEGORICAL_FEATURE_KEYS, DENSE_FLOAT_FEATURE_KEYS, N_WIDE,
                               VOCAB_FEATURE_KEYS, TaxiWideDeep, hidden_units, wide_cardinalities, wide_offsets)

WIDE_FEATURE_KEYS = list(BUCKET_FEATURE_KEYS) + list(VOCAB_FEATURE_KEYS) + list(CATEGORICAL_FEATURE_KEYS)
NB = 1024  # probability bins (csrc/ops/taxi_eval.hip NB; checked against the library in TaxiEvaluator)
QSCALE = float(2 ** 24)  # fixed point of the loss / probability sums
MAX_SLICES = 128


def slice_column(slice_by) -> int:
    """``slice_by`` (None, a wide feature's name or its column index) -> column index or -1; ValueError for
    an unknown feature and for the columns with more than 128 values (vocabularies, census tracts)."""
    if slice_by is None:
        return -1
    if isinstance(slice_by, str):
        if slice_by not in WIDE_FEATURE_KEYS:
            raise ValueError(f"unknown slice feature {slice_by!r}; one of {WIDE_FEATURE_KEYS}")
        col = WIDE_FEATURE_KEYS.index(slice_by)
    else:
        col = int(slice_by)
        if not 0 <= col < N_WIDE:
            raise ValueError(f"slice column {col} outside [0, {N_WIDE})")
    if wide_cardinalities()[col] > MAX_SLICES:
        raise ValueError(f"{WIDE_FEATURE_KEYS[col]} has {wide_cardinalities()[col]} values; slicing takes "
                         f"columns of at most {MAX_SLICES}")
    return col


def slice_ids_of(cat, col: int) -> np.ndarray:
    """Per-row slice id of column ``col`` of the global one-hot ids ``cat`` [n, 13]; -1 where outside the
    column's range (the row is in no slice)."""
    c = cat.detach().cpu().numpy() if isinstance(cat, torch.Tensor) else np.asarray(cat)
    d = c[:, col].astype(np.int64) - int(wide_offsets()[col])
    return np.where((d >= 0) & (d < wide_cardinalities()[col]), d, -1)


@dataclass
class TaxiEvalResult:
    """Device tensors of one ``TaxiEvaluator.run``: ``logit`` / ``prob`` fp32 [n]; with labels also ``loss``
    fp32 [n] (BCE with logits), ``hit`` uint8 [n] ((logit > 0) == (label > 0.5)) and ``acc``, the int64
    accumulator buffer ([1 + S, 3] sums {hits, loss_q, prob_q}, then the uint32 [1 + S, 2, NB] histograms;
    index 0 is "overall", 1 + s slice s); else those are None."""
    logit: torch.Tensor
    prob: torch.Tensor
    loss: torch.Tensor | None
    hit: torch.Tensor | None
    acc: torch.Tensor | None
    n: int
    S: int = 0
    slice_col: int = -1

    def accumulators(self) -> tuple[np.ndarray, np.ndarray]:
        """(sums uint64 [1 + S, 3], hist uint32 [1 + S, 2, NB]) on the host: one device-to-host copy."""
        if self.acc is None:
            raise ValueError("a run without labels has no accumulators")
        a = self.acc.cpu().numpy()
        k = (1 + self.S) * 3
        return a[:k].view(np.uint64).reshape(1 + self.S, 3).copy(), a[k:].view(np.uint32).reshape(1 + self.S, 2, NB).copy()


def _ext():
    from ..ops import _C

    return _C.ext()


def _lins(model):
    from .. import nn as hnn

    return [m for m in model.deep if isinstance(m, hnn.Linear)]


def _arena_of(model):
    """The one ParamArena every parameter of the model lives in, or None."""
    ps = list(model.parameters())
    arenas = {id(getattr(p, "_hx_arena", None)) for p in ps}
    a = getattr(ps[0], "_hx_arena", None) if ps else None
    return a if a is not None and len(arenas) == 1 else None


def _default_shape(model) -> bool:
    if not isinstance(model, TaxiWideDeep):
        return False
    lins = _lins(model)
    dims = [len(DENSE_FLOAT_FEATURE_KEYS)] + hidden_units() + [1]
    return (len(lins) == 5 and [lins[0].weight.shape[1]] + [m.weight.shape[0] for m in lins] == dims
            and all(m.activation == "relu" for m in lins[:-1]) and lins[-1].activation is None
            and all(m.bias is not None for m in lins)
            and tuple(model.wide.weight.shape) == (int(sum(wide_cardinalities())), 1))


class TaxiEvaluator:
    @staticmethod
    def supported(model) -> bool:
        """A ``TaxiWideDeep`` with the default hidden units, in one CUDA ParamArena with a bf16 shadow;
        ``HOPSX_TAXI_EVAL_FUSED=0`` keeps callers on the chunked layer-by-layer forward."""
        if os.environ.get("HOPSX_TAXI_EVAL_FUSED", "1") == "0":
            return False
        if not _default_shape(model):
            return False
        a = _arena_of(model)
        return a is not None and a.device.type == "cuda" and a.shadow is not None

    def __init__(self, model, max_workgroups: int = 0):
        """``max_workgroups``: cap of the launch grid (0: two workgroups per CU); results do not depend on it."""
        if not _default_shape(model) or _arena_of(model) is None:
            raise ValueError("TaxiEvaluator needs the default TaxiWideDeep in a ParamArena (see supported())")
        self.model = model
        self.max_workgroups = int(max_workgroups)
        self.launches = 0
        if int(_ext().taxi_eval_bins()) != NB:
            raise RuntimeError("taxi_eval: the kernel library's bin count differs from runtime/taxi_eval.py NB")

    @staticmethod
    def _alloc(n: int, labels: bool, S: int, col: int, dev) -> TaxiEvalResult:
        f32 = dict(device=dev, dtype=torch.float32)
        logit, prob = torch.empty(n, **f32), torch.empty(n, **f32)
        if not labels:
            return TaxiEvalResult(logit, prob, None, None, None, n, S, col)
        return TaxiEvalResult(logit, prob, torch.empty(n, **f32), torch.empty(n, device=dev, dtype=torch.uint8),
                              torch.zeros((1 + S) * (3 + NB), device=dev, dtype=torch.int64), n, S, col)

    def run(self, dense: torch.Tensor, cat: torch.Tensor, label: torch.Tensor | None = None, slice_by=None,
            out: TaxiEvalResult | None = None) -> TaxiEvalResult:
        """Forward of ``dense`` (fp32 [n, 3]) / ``cat`` (int64 [n, 13] global one-hot ids), contiguous and on
        the model's device, in one launch on torch's current stream; with ``label`` (fp32 [n] or [n, 1]) also
        loss / hit / accumulators, sliced by ``slice_by`` (a wide feature's name or column index).  ``out``:
        a previous result of the same n and S (with / without labels alike) whose buffers are overwritten —
        nothing is allocated then, so the call can be captured into a graph.  n = 0 launches nothing."""
        from ..ops import _C

        a = _arena_of(self.model)
        if a is None or a.shadow is None or a.device.type != "cuda":
            raise RuntimeError("TaxiEvaluator: the model's parameters are not in a CUDA ParamArena with a bf16 shadow")
        dev = a.master.device  # (with its index: the arena may have been made on a bare "cuda")
        nd = len(DENSE_FLOAT_FEATURE_KEYS)
        if (dense.dtype != torch.float32 or dense.device != dev or not dense.is_contiguous() or dense.dim() != 2
                or dense.shape[1] != nd):
            raise ValueError(f"dense must be a contiguous fp32 [n, {nd}] tensor on {dev}")
        n = int(dense.shape[0])
        if cat.dtype != torch.int64 or cat.device != dev or not cat.is_contiguous() or tuple(cat.shape) != (n, N_WIDE):
            raise ValueError(f"cat must be a contiguous int64 [{n}, {N_WIDE}] tensor on {dev}")
        if label is not None and (label.dtype != torch.float32 or label.device != dev or not label.is_contiguous()
                                  or tuple(label.shape) not in ((n,), (n, 1))):
            raise ValueError(f"label must be a contiguous fp32 [{n}] or [{n}, 1] tensor on {dev}")
        col = slice_column(slice_by)
        if col >= 0 and label is None:
            raise ValueError("slicing needs labels: the per-slice accumulators are label histograms")
        S = wide_cardinalities()[col] if col >= 0 else 0
        if out is None:
            out = self._alloc(n, label is not None, S, col, dev)
        elif out.n != n or out.S != S or (out.acc is None) != (label is None) or out.logit.device != dev:
            raise ValueError("out= must come from a run of the same n and S, with / without labels alike")
        out.slice_col = col
        if n == 0:
            return out
        lins = _lins(self.model)
        iv = ([int(m.weight._hx_off) for m in lins] + [int(m.bias._hx_off) for m in lins]
              + [int(self.model.wide.weight._hx_off), int(self.model.wide.weight.shape[0]), n, col,
                 self.max_workgroups])
        ptrs = [a.master.data_ptr(), a.shadow.data_ptr(), dense.data_ptr(), cat.data_ptr(), _C.ptr(label),
                out.logit.data_ptr(), out.prob.data_ptr(), _C.ptr(out.loss), _C.ptr(out.hit), _C.ptr(out.acc)]
        _C.check(_ext().taxi_eval(ptrs, iv, _C.stream()), "taxi_eval")
        self.launches += 1
        return out


# ------------------------------------------------------------------------------------------- metrics
def accumulate_rows(prob, loss, label, slice_ids=None, S: int = 0, hit=None) -> tuple[np.ndarray, np.ndarray]:
    """The kernel's integer accumulators from per-row arrays, in numpy: (sums uint64 [1 + S, 3] = {hits,
    loss_q, prob_q}, hist uint32 [1 + S, 2, NB]).  bin = min(int(prob * NB), NB - 1) in float32; loss_q /
    prob_q = round-half-even(value * 2^24) of the float32 value; a row with slice id outside [0, S) is in
    "overall" only.  ``hit`` defaults to (prob > 0.5) == (label > 0.5)."""
    def host(t, dt):
        t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return t.reshape(-1).astype(dt, copy=False)

    prob, loss, label = host(prob, np.float32), host(loss, np.float32), host(label, np.float32)
    y = (label > np.float32(0.5)).astype(np.int64)
    hit = ((prob > np.float32(0.5)).astype(np.int64) == y) if hit is None else host(hit, np.int64) != 0
    bins = np.minimum((prob * np.float32(NB)).astype(np.int64), NB - 1)
    lq = np.rint(loss * np.float32(QSCALE)).astype(np.int64)
    pq = np.rint(prob * np.float32(QSCALE)).astype(np.int64)
    sums = np.zeros((1 + S, 3), np.uint64)
    hist = np.zeros((1 + S, 2, NB), np.uint32)
    sid = np.full(len(prob), -1, np.int64) if slice_ids is None or S == 0 else host(slice_ids, np.int64)
    groups = [(0, np.ones(len(prob), bool))] + [(1 + s, sid == s) for s in range(S)]
    for k, m in groups:
        sums[k] = (int(hit[m].sum()), int(lq[m].sum()), int(pq[m].sum()))
        hist[k] = np.bincount(y[m] * NB + bins[m], minlength=2 * NB).reshape(2, NB)
    return sums, hist


def _one(sums, hist) -> dict:
    neg, pos = hist[0].astype(np.int64), hist[1].astype(np.int64)
    N, P = int(neg.sum()), int(pos.sum())
    cnt = N + P
    nan = float("nan")
    hits, lq, pq = (int(v) for v in sums)
    d = {"count": cnt, "positives": P, "hits": hits, "loss_q": lq, "prob_q": pq,
         "accuracy": hits / cnt if cnt else nan, "log_loss": lq / QSCALE / cnt if cnt else nan,
         "mean_prediction": pq / QSCALE / cnt if cnt else nan, "mean_label": P / cnt if cnt else nan}
    d["calibration"] = d["mean_prediction"] / d["mean_label"] if cnt and P else nan
    if P and N:
        below = np.cumsum(neg) - neg  # negatives in lower bins
        same = int((pos * neg).sum())
        d["auc_bucketed"] = (int((pos * below).sum()) + 0.5 * same) / (P * N)
        d["auc_bound"] = same / (2.0 * P * N)
    else:
        d["auc_bucketed"] = d["auc_bound"] = nan
    return d


def metrics_from_accumulators(sums: np.ndarray, hist: np.ndarray) -> dict:
    """{"overall": {...}, "slices": [{...} per slice]}: count, positives, accuracy, log_loss, mean_prediction,
    mean_label, calibration (= mean_prediction / mean_label), auc_bucketed (over the NB bins a positive in a
    higher bin than a negative counts 1, a pair in the same bin 1/2) and auc_bound (= sum_b pos_b neg_b /
    (2 P N): the worst-case distance of auc_bucketed from the rank AUC), plus the raw integers.  A slice with
    no rows or one class only reports nan where a ratio is undefined."""
    return {"overall": _one(sums[0], hist[0]), "slices": [_one(sums[k], hist[k]) for k in range(1, len(sums))]}


def metrics(result: TaxiEvalResult) -> dict:
    """The metric dictionary of a labelled run: one small device-to-host copy of the accumulators."""
    return metrics_from_accumulators(*result.accumulators())


def metrics_from_rows(prob, loss, label, slice_ids=None, S: int = 0, hit=None) -> dict:
    """``metrics`` computed in numpy from per-row arrays (see ``accumulate_rows``)."""
    return metrics_from_accumulators(*accumulate_rows(prob, loss, label, slice_ids, S, hit))


def bce_with_logits(z: np.ndarray, label: np.ndarray) -> np.ndarray:
    """Per-row stable BCE with logits, max(z, 0) - z y + log1p(exp(-|z|)) with y = label > 0.5, in z's dtype."""
    z = np.asarray(z)
    y = (np.asarray(label).reshape(-1) > 0.5).astype(z.dtype)
    z = z.reshape(-1)
    return np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))


# ------------------------------------------------------------------------------------------- reference
def reference_logits(model_or_state, dense, cat, dtype: torch.dtype = torch.float64,
                     emulate_bf16: bool = True) -> torch.Tensor:
    """The forward half of ``models.widedeep.reference_steps``: logits [n] of ``dense`` [n, 3] / ``cat``
    [n, 13] in ``dtype`` on the CPU, from a ``TaxiWideDeep`` or its state dict.  ``emulate_bf16`` rounds
    exactly what the kernels hold as bf16 (inputs, the four hidden activations, the hidden W images).
    ``dtype=torch.float32`` is the fp32 proxy of the kernel's arithmetic: its distance to the fp64 result
    measures what fp32 accumulation (and the bf16 rounding flips it causes) can do."""
    sd = model_or_state.state_dict() if isinstance(model_or_state, torch.nn.Module) else model_or_state
    P = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    bf = (lambda t: t.to(torch.bfloat16).to(dtype)) if emulate_bf16 else (lambda t: t)
    with torch.no_grad():
        a = bf(dense.detach().cpu().to(dtype))
        c = cat.detach().cpu()
        for l in range(4):
            a = bf(torch.relu(a @ bf(P[f"deep.{l}.weight"]).T + P[f"deep.{l}.bias"]))
        return a @ P["deep.4.weight"].reshape(-1) + P["deep.4.bias"].reshape(1) + P["wide.weight"].reshape(-1)[c].sum(1)
