"""Chicago-taxi wide & deep classifier ("big tipper": tips > 20% of the fare).

The reference README names a TFX Chicago-taxi pipeline (README.md:99-112) whose
notebooks are absent from the repo, so the model follows the public
TFX taxi trainer it points to:

* dense (DNN) inputs: trip_miles, fare, trip_seconds — z-scored by the Transform stage;
* wide (linear) inputs: 13 identity-categorical columns —
  4 bucketized lat/long columns (10 buckets each), 2 vocabulary columns
  (payment_type, company: 1000 vocab + 10 OOV buckets) and 7 categorical columns
  (trip_start_hour 24, trip_start_day 31, trip_start_month 12, pickup/dropoff census
  tract 2000, pickup/dropoff community area 80) — 6,287 one-hot slots in total;
* DNN hidden units [100, 70, 48, 34] (first_dnn_layer_size=100, num_dnn_layers=4,
  dnn_decay_factor=0.7), logits = wide + deep, sigmoid cross-entropy;
* optimizers as tf.estimator.DNNLinearCombinedClassifier: FTRL (lr 0.2) on the wide
  part, Adagrad (lr 0.05, accumulator 0.1) on the deep part; train batch 40.

MI355X mapping: the wide part is a fixed-length embedding-bag (13 rows of a
[6287, 1] table per example, thread-per-bag gather / atomic scatter-add kernel);
the deep part runs on the MFMA linear kernels with fused bias+ReLU epilogues; the
two optimizers are single fused kernels over two slices of ONE parameter arena
(so data parallelism all-reduces one flat buffer); the whole step is one hipGraph.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from torch import nn

from .. import nn as hnn
from ..ops import functional as HF

DENSE_FLOAT_FEATURE_KEYS = ["trip_miles", "fare", "trip_seconds"]
BUCKET_FEATURE_KEYS = ["pickup_latitude", "pickup_longitude", "dropoff_latitude", "dropoff_longitude"]
FEATURE_BUCKET_COUNT = 10
VOCAB_FEATURE_KEYS = ["payment_type", "company"]
VOCAB_SIZE, OOV_SIZE = 1000, 10
CATEGORICAL_FEATURE_KEYS = ["trip_start_hour", "trip_start_day", "trip_start_month", "pickup_census_tract",
                            "dropoff_census_tract", "pickup_community_area", "dropoff_community_area"]
MAX_CATEGORICAL_FEATURE_VALUES = [24, 31, 12, 2000, 2000, 80, 80]
LABEL_KEY = "tips"
TRAIN_BATCH_SIZE = 40


def hidden_units(first: int = 100, num_layers: int = 4, decay: float = 0.7) -> list[int]:
    return [max(2, int(first * decay ** i)) for i in range(num_layers)]


def wide_cardinalities() -> list[int]:
    return ([FEATURE_BUCKET_COUNT] * len(BUCKET_FEATURE_KEYS) + [VOCAB_SIZE + OOV_SIZE] * len(VOCAB_FEATURE_KEYS)
            + list(MAX_CATEGORICAL_FEATURE_VALUES))


def wide_offsets() -> np.ndarray:
    c = wide_cardinalities()
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)


WIDE_ROWS = int(sum(wide_cardinalities()))  # 6287
N_WIDE = len(wide_cardinalities())  # 13


class TaxiWideDeep(nn.Module):
    def __init__(self, hidden=None):
        super().__init__()
        hidden = hidden or hidden_units()
        # wide part first, deep part second: each is one contiguous slice of the arena
        self.wide = nn.Module()
        self.wide.weight = nn.Parameter(torch.zeros(WIDE_ROWS, 1))  # linear model init = 0 (tf.estimator)
        layers, d = [], len(DENSE_FLOAT_FEATURE_KEYS)
        for h in hidden:
            layers.append(hnn.Linear(d, h, activation="relu"))
            d = h
        layers.append(hnn.Linear(d, 1, out_f32=True))
        self.deep = nn.Sequential(*layers)

    def forward(self, dense, cat):
        """dense: [B, 3] z-scored floats; cat: [B, 13] int64 ids, already offset into the
        concatenated one-hot space (see ``wide_offsets``). Returns fp32 logits [B, 1]."""
        deep = self.deep(dense if not dense.is_cuda else HF.to_compute(dense))
        wide = HF.embedding_bag(cat, self.wide.weight)
        return deep.float() + wide


def make_optimizer(model: TaxiWideDeep, ftrl_lr: float = 0.2, adagrad_lr: float = 0.05):
    from .. import optim

    return optim.Chain(optim.Ftrl(model.wide, lr=min(ftrl_lr, 1.0 / math.sqrt(N_WIDE))),
                       optim.Adagrad(model.deep, lr=adagrad_lr, initial_accumulator_value=0.1))


def reference_steps(W, b, w4, b4, wide, ada_s, ftrl_z, ftrl_n, hp_ada, hp_ftrl, dense, cat, label, steps):
    """fp64 replay of ``steps`` v2 taxi steps that rounds to bf16 exactly where the kernel
    (csrc/ops/taxi_step.hip) holds bf16 images: inputs, hidden activations, W images and the backward
    gradients G.  W/b: the 4 hidden layers ([out, in] / [out]); w4, b4: logits; wide: [rows];
    ada_s: name -> Adagrad accumulator ("W0".."W3", "b0".."b3", "w4", "b4"); ftrl_z/n: [rows];
    hp_ada / hp_ftrl: the kernel's 8-float hyper-parameter vectors; dense/cat/label: [nb, B, ...].
    Everything is updated in place; returns the per-step mean losses.  A data-parallel step of W
    replicas is this with their batches concatenated along the batch axis (global-batch mean, one FTRL
    update per touched row with the summed gradient)."""
    def bf(x):
        return x.to(torch.bfloat16).to(torch.float64)

    lr, gscale, wd, eps = hp_ada[:4]
    flr, fgs, _, l1, l2, beta = hp_ftrl[:6]

    def adagrad(p, g, s):
        g = g * gscale + wd * p
        s += g * g
        return p - lr * g / (s.sqrt() + eps)

    losses = []
    for i in range(steps):
        j = i % dense.shape[0]
        x, c, y = dense[j], cat[j], label[j].reshape(-1)
        B = x.shape[0]
        acts = [bf(x)]
        a = acts[0]
        for l in range(4):
            a = bf(torch.relu(a @ bf(W[l]).T + b[l]))
            acts.append(a)
        z = a @ w4 + b4 + wide[c].sum(1)
        p = torch.sigmoid(z)
        losses.append(float(torch.nn.functional.binary_cross_entropy_with_logits(z, y)))
        g = (p - y) / B
        grads = {"w4": g @ a, "b4": g.sum()}  # the logits layer: fp32 g times the bf16 activations
        G = bf(g[:, None] * w4[None, :] * (a > 0))
        for l in (3, 2, 1, 0):
            grads[f"W{l}"] = G.T @ acts[l]
            grads[f"b{l}"] = G.sum(0)
            if l > 0:
                G = bf((G @ bf(W[l])) * (acts[l] > 0))
        # wide: summed example gradients per touched row, FTRL
        gw = torch.zeros_like(wide)
        gw.index_add_(0, c.reshape(-1), g[:, None].expand(-1, c.shape[1]).reshape(-1))
        rows = torch.unique(c.reshape(-1))
        gr = gw[rows] * fgs
        n_old = ftrl_n[rows]
        nn_ = n_old + gr * gr
        sigma = (nn_.sqrt() - n_old.sqrt()) / flr
        ftrl_z[rows] += gr - sigma * wide[rows]
        ftrl_n[rows] = nn_
        zz = ftrl_z[rows]
        wide[rows] = torch.where(zz.abs() <= l1, torch.zeros_like(zz),
                                 -(zz - torch.sign(zz) * l1) / ((beta + nn_.sqrt()) / flr + 2 * l2))
        for l in range(4):
            W[l] = adagrad(W[l], grads[f"W{l}"], ada_s[f"W{l}"])
            b[l] = adagrad(b[l], grads[f"b{l}"], ada_s[f"b{l}"])
        w4[:] = adagrad(w4, grads["w4"], ada_s["w4"])
        b4[:] = adagrad(b4, grads["b4"].reshape(1), ada_s["b4"])
    return losses


def reference_state(model, fused):
    """The fp64 host copies ``reference_steps`` takes, from a model's arena: (W, b, w4, b4, wide, ada_s,
    ftrl_z, ftrl_n, hp_ada, hp_ftrl)."""
    a = model.wide.weight._hx_arena
    lins = fused.lins
    f64 = lambda t: t.detach().double().cpu().clone()  # noqa: E731
    W = [f64(m.weight).reshape(m.weight.shape) for m in lins[:4]]
    b = [f64(m.bias) for m in lins[:4]]
    w4 = f64(lins[4].weight).reshape(-1)
    b4 = f64(lins[4].bias).reshape(1)
    s = a.state("adagrad_s0").double().cpu()
    ada = {}
    for l in range(5):
        m = lins[l]
        ws = s[m.weight._hx_off:m.weight._hx_off + m.weight.numel()].clone()
        bs = s[m.bias._hx_off:m.bias._hx_off + m.bias.numel()].clone()
        ada[f"W{l}" if l < 4 else "w4"] = ws.reshape(m.weight.shape) if l < 4 else ws
        ada[f"b{l}" if l < 4 else "b4"] = bs
    wo, rows = int(model.wide.weight._hx_off), model.wide.weight.shape[0]
    wide = a.master[wo:wo + rows].double().cpu().clone()
    z = a.state("ftrl_s0")[wo:wo + rows].double().cpu().clone()
    n = a.state("ftrl_s1")[wo:wo + rows].double().cpu().clone()
    fl = fused._floats()
    return W, b, w4, b4, wide, ada, z, n, fl[:8], fl[8:]


def synth_taxi(n: int, seed: int = 0, device="cpu"):
    """Transformed-feature synthetic taxi trips with a learnable tip rule.
    Returns dense [n, 3] f32, cat [n, 13] int64 (global one-hot ids), label [n, 1] f32."""
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn(n, len(DENSE_FLOAT_FEATURE_KEYS), generator=g)
    card = wide_cardinalities()
    cols = []
    for c in card:
        if c == VOCAB_SIZE + OOV_SIZE:  # vocabulary columns are heavy-tailed
            r = torch.rand(n, generator=g)
            cols.append(torch.clamp((c * r ** 3).long(), max=c - 1))
        else:
            cols.append(torch.randint(0, c, (n,), generator=g))
    cat = torch.stack(cols, 1) + torch.from_numpy(wide_offsets())
    w_true = torch.randn(WIDE_ROWS, generator=g) * 0.5
    logit = dense @ torch.tensor([0.8, -0.6, 0.3]) + w_true[cat].sum(1) * 0.5
    label = (torch.rand(n, generator=g) < torch.sigmoid(logit)).float().unsqueeze(1)
    dev = torch.device(device)
    return dense.to(dev), cat.to(dev), label.to(dev)


def bench_taxi(dev, batch: int, steps: int, warmup: int, timed, world: int = 1, graph: bool = True,
               pool_examples: int = 200_000, from_transform: bool = False) -> dict:
    """Steps/sec of the taxi trainer (per-GPU batch ``batch``; DP all-reduce when world > 1).
    ``from_transform``: the training examples come from the TFX Transform stage (tfx.transform:
    raw synthetic trips analyzed + transformed on the device) instead of pre-transformed features;
    the analyze/apply time is reported, not timed with the steps."""
    from ..parallel.dp import DataParallel
    from ..runtime.arena import ParamArena
    from ..runtime.step import TrainStep
    from ..runtime.taxi_step import FusedWideDeepStep, TaxiExchange

    model = TaxiWideDeep().to(dev)
    ParamArena.from_module(model, dev)
    opt = make_optimizer(model)
    xdp = None
    if (world > 1 and dev.type == "cuda" and os.environ.get("HOPSX_TAXI_FUSED", "1") == "1"
            and os.environ.get("HOPSX_TAXI_DP_FUSED", "1") == "1" and FusedWideDeepStep(model, opt).v2(batch)):
        # every rank decides alike (same model, batch and environment): the in-kernel exchange (collective setup)
        xdp = TaxiExchange(dev, world)
    dp = DataParallel(model) if world > 1 and xdp is None else None
    nb = max(8, -(-pool_examples // batch))
    transform_s = None
    if from_transform:
        import time as _time

        from ..tfx import analyze, synth_raw_trips

        raw = synth_raw_trips(nb * batch, seed=7)
        t0 = _time.perf_counter()
        tf = analyze(raw, device=dev)
        dense, cat, label = tf.apply(raw, device=dev)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        transform_s = round(_time.perf_counter() - t0, 3)
    else:
        from ..parallel import dist as hdist

        # every replica trains on its own examples (data parallel): the seed carries the rank
        dense, cat, label = synth_taxi(nb * batch, seed=7 + 1009 * hdist.rank(), device=dev)
    cat = cat.view(nb, batch, -1)
    label = label.view(nb, batch, 1)
    out = {}
    fused = FusedWideDeepStep(model, opt, dp=dp, xdp=xdp) if os.environ.get("HOPSX_TAXI_FUSED", "1") == "1" else None
    if xdp is not None:
        xdp.sync_replicas(model.wide.weight._hx_arena)
    if fused is not None and fused.ok(batch):
        dense = dense.view(nb, batch, -1)
        path = f"fused-{fused.kernel}"

        def run(i):
            # one launch: the kernel reads batch `cursor` of the resident epoch and advances it
            out["r"] = fused.step_resident((dense, cat), label, graph=graph)

        def run_n(n):
            out["r"] = fused.run_resident((dense, cat), label, n, graph=graph)

        run.run_n = run_n
        run.prepare = lambda: fused.prepare_resident((dense, cat), label, n=steps)
    else:
        step = TrainStep(model, opt, "bce_logits", dp=dp, graph=graph, forward_fn=lambda m, x: m(*x))
        dense = dense.to(torch.bfloat16).view(nb, batch, -1)
        path = "layerwise"

        def run(i):
            j = i % nb
            out["r"] = step((dense[j], cat[j]), label[j])

    for i in range(warmup):
        run(i)
    if hasattr(run, "prepare"):
        run.prepare()  # build the multi-step graph outside the timed region
    el = timed(run, steps, dev)
    loss = float(out["r"]["loss"].reshape(-1)[0])
    replicas = None
    if xdp is not None:
        fused.check()  # the exchange's sticky error word (outside the timed region)
        replicas = xdp.replicas_agree(fused.digest())
        xdp.close()
    return {"steps_per_sec": round(steps / el, 1), "examples_per_sec": round(batch * world * steps / el, 1),
            "ms_per_step": round(el / steps * 1e3, 4), "batch_per_gpu": batch, "loss": round(loss, 4),
            "params": sum(p.numel() for p in model.parameters()), "hidden_units": hidden_units(), "step": path,
            "data": "tfx-transform" if from_transform else "synthetic-transformed",
            **({"replicas_identical": replicas} if replicas is not None else {}),
            **({"transform_s": transform_s} if transform_s is not None else {})}
