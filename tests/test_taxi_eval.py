"""The sliced taxi Evaluator's host side (runtime/taxi_eval.py, tfx/pipeline.py) on the CPU: the fp64 reference
forward against ``reference_steps``, the numpy metrics (the oracle of the kernel's integer accumulators) on a
hand-made example, the derived bound of the bucketed AUC, ``supported()``, and the pipeline's Evaluator keeping
its old numbers.  The kernel is held to these in test_taxi_eval_gpu.py."""
import json
import math

import numpy as np
import pandas as pd
import torch

from hops_examples_amd.models import widedeep as WD
from hops_examples_amd.runtime import taxi_eval as TE
from hops_examples_amd.runtime.arena import ParamArena


def _model(seed=1):
    """Default init under ``seed``, wide.weight = randn * 0.5 (the wide part initialises to zero)."""
    torch.manual_seed(seed)
    m = WD.TaxiWideDeep()
    with torch.no_grad():
        m.wide.weight.copy_(torch.randn(WD.WIDE_ROWS, 1, generator=torch.Generator().manual_seed(seed)) * 0.5)
    return m


def _rank_auc(score, y):
    ranks = pd.Series(score).rank().to_numpy()
    pos = y > 0.5
    return float((ranks[pos].sum() - pos.sum() * (pos.sum() + 1) / 2) / (pos.sum() * (~pos).sum()))


def test_reference_logits_is_the_forward_of_reference_steps():
    m = _model()
    B = 40
    dense, cat, label = WD.synth_taxi(B, seed=3)
    z = TE.reference_logits(m, dense, cat)
    assert z.dtype == torch.float64 and z.shape == (B,)
    sd = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    W = [sd[f"deep.{l}.weight"] for l in range(4)]
    b = [sd[f"deep.{l}.bias"] for l in range(4)]
    w4, b4, wide = sd["deep.4.weight"].reshape(-1), sd["deep.4.bias"].reshape(1), sd["wide.weight"].reshape(-1)
    ada = {**{f"W{l}": torch.full_like(W[l], 0.1) for l in range(4)}, **{f"b{l}": torch.full_like(b[l], 0.1) for l in range(4)},
           "w4": torch.full_like(w4, 0.1), "b4": torch.full_like(b4, 0.1)}
    losses = WD.reference_steps(W, b, w4, b4, wide, ada, torch.zeros_like(wide), torch.full_like(wide, 0.1),
                                [0.05, 1.0, 0.0, 1e-10, 0, 0, 0, 0], [0.2, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0],
                                dense.double()[None], cat[None], label.double()[None], 1)
    mean_bce = float(torch.nn.functional.binary_cross_entropy_with_logits(z, label.double().reshape(-1)))
    assert abs(mean_bce - losses[0]) <= 1e-12, (mean_bce, losses[0])
    # the state-dict form, the fp32 proxy and the unrounded forward
    assert torch.equal(TE.reference_logits(m.state_dict(), dense, cat), z)
    z32 = TE.reference_logits(m, dense, cat, dtype=torch.float32)
    assert z32.dtype == torch.float32 and float((z32.double() - z).abs().max()) < 1e-3
    exact = TE.reference_logits(m, dense, cat, emulate_bf16=False)
    with torch.no_grad():
        assert float((exact - m(dense, cat).double().reshape(-1)).abs().max()) < 1e-4  # the fp32 layer-by-layer model


def test_metrics_from_rows_on_a_handmade_example():
    prob = np.array([0.875, 0.75, 0.25, 0.125, 0.625, 0.6875, 0.0625, 0.625], np.float32)
    label = np.array([1, 0, 1, 0, 1, 1, 1, 0], np.float32)
    loss = np.array([0.125, 1.5, 1.25, 0.25, 0.5, 0.375, 2.25, 0.75], np.float32)
    sid = np.array([0, 0, 0, 0, 1, 1, 1, -1])  # the last row is in no slice; slice 2 is empty
    sums, hist = TE.accumulate_rows(prob, loss, label, sid, 3)
    assert sums.dtype == np.uint64 and hist.dtype == np.uint32 and hist.shape == (4, 2, TE.NB)
    bins = [896, 768, 256, 128, 640, 704, 64, 640]
    want = np.zeros((4, 2, TE.NB), np.uint32)
    for i, b in enumerate(bins):
        want[0, int(label[i]), b] += 1
        if sid[i] >= 0:
            want[1 + sid[i], int(label[i]), b] += 1
    assert np.array_equal(hist, want)
    q = 2 ** 24
    assert sums.tolist() == [[4, 7 * q, 4 * q], [2, int(3.125 * q), 2 * q], [2, int(3.125 * q), int(1.375 * q)], [0, 0, 0]]
    m = TE.metrics_from_rows(prob, loss, label, sid, 3)
    o, s0, s1, s2 = m["overall"], *m["slices"]
    assert (o["count"], o["positives"], o["accuracy"], o["log_loss"]) == (8, 5, 0.5, 0.875)
    assert (o["mean_prediction"], o["mean_label"], o["calibration"]) == (0.5, 0.625, 0.8)
    assert o["auc_bucketed"] == 7.5 / 15 and o["auc_bound"] == 1 / 30  # one positive shares a bin with one negative
    assert (s0["count"], s0["positives"], s0["accuracy"], s0["calibration"], s0["auc_bucketed"], s0["auc_bound"]) == (
        4, 2, 0.5, 1.0, 0.75, 0.0)
    # one class only: the ratios that need both classes are nan, nothing raises
    assert (s1["count"], s1["positives"], s1["mean_label"]) == (3, 3, 1.0) and s1["calibration"] == 1.375 / 3
    assert math.isnan(s1["auc_bucketed"]) and math.isnan(s1["auc_bound"]) and s1["accuracy"] == 2 / 3
    assert s2["count"] == 0 and all(math.isnan(s2[k]) for k in ("accuracy", "log_loss", "mean_prediction", "mean_label",
                                                                "calibration", "auc_bucketed", "auc_bound"))
    # an explicit hit column replaces the default (prob > 0.5) == (label > 0.5); prob 1.0 lands in the last bin
    m2 = TE.metrics_from_rows(prob, loss, label, sid, 3, hit=np.ones(8, np.uint8))
    assert m2["overall"]["accuracy"] == 1.0 and m2["slices"][2]["count"] == 0
    _, h1 = TE.accumulate_rows(np.ones(1, np.float32), np.zeros(1, np.float32), np.ones(1, np.float32))
    assert h1[0, 1, TE.NB - 1] == 1 and h1.sum() == 1
    json.dumps(m)  # the pipeline writes it as JSON


def test_bucketed_auc_is_within_its_bound_of_the_rank_auc():
    m = _model()
    dense, cat, label = WD.synth_taxi(2085, seed=3)
    z = TE.reference_logits(m, dense, cat, dtype=torch.float32)
    p = torch.sigmoid(z).numpy()
    y = label.numpy().reshape(-1)
    o = TE.metrics_from_rows(p, TE.bce_with_logits(z.numpy(), y), y)["overall"]
    exact = _rank_auc(p, y)
    print(f"auc_bucketed {o['auc_bucketed']:.6f} rank {exact:.6f} distance {abs(o['auc_bucketed'] - exact):.2e} "
          f"bound {o['auc_bound']:.2e}")
    # Both AUCs count a pair in different bins alike (the bins are monotone in the score); a pair inside one bin
    # counts 1/2 in the bucketed AUC and 0, 1/2 or 1 in the rank AUC: the distance is at most sum_b pos_b neg_b / (2 P N)
    assert abs(o["auc_bucketed"] - exact) <= o["auc_bound"] + 1e-12
    assert 0 < o["auc_bound"] < 5e-3 and o["count"] == 2085
    hours = TE.metrics_from_rows(p, TE.bce_with_logits(z.numpy(), y), y, TE.slice_ids_of(cat, 6), 24)["slices"]
    assert sum(s["count"] for s in hours) == 2085 and min(s["count"] for s in hours) > 0


def test_slice_column_and_supported(monkeypatch):
    assert TE.slice_column(None) == -1 and TE.slice_column("trip_start_hour") == 6 and TE.slice_column(0) == 0
    for bad in ("payment_type", "company", "pickup_census_tract", "dropoff_census_tract", 4, 5, 9, 10, "no_such", 13):
        try:
            TE.slice_column(bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    ok = [WD.wide_cardinalities()[TE.slice_column(c)] for c in range(13) if c not in (4, 5, 9, 10)]
    assert ok == [10, 10, 10, 10, 24, 31, 12, 80, 80]
    m = _model()
    ParamArena.from_module(m, torch.device("cpu"))
    assert TE.TaxiEvaluator.supported(m) is False  # a CPU model
    monkeypatch.setenv("HOPSX_TAXI_EVAL_FUSED", "0")
    assert TE.TaxiEvaluator.supported(m) is False
    assert TE.TaxiEvaluator.supported(torch.nn.Linear(3, 1)) is False


def test_pipeline_evaluator_on_the_cpu_keeps_its_numbers(tmp_path, monkeypatch):
    monkeypatch.setenv("HOPSX_PROJECT_ROOT", str(tmp_path))
    from hops_examples_amd.tfx import pipeline, synth_raw_trips

    raw = tmp_path / "raw.parquet"
    synth_raw_trips(3000, seed=2).to_parquet(raw)
    root = tmp_path / "pipe"
    pipeline.example_gen(root, raw)
    pipeline.transform(root, device="cpu")
    pipeline.trainer(root, steps=40, device="cpu")
    ev = pipeline.evaluator(root, device="cpu", slice_by=("trip_start_hour", "pickup_latitude"))
    # the old way
    dev = torch.device("cpu")
    dense, cat, label = pipeline._load_transformed(root, "eval", dev)
    model = WD.TaxiWideDeep()
    model.load_state_dict(torch.load(root / "trainer" / "model.pt", map_location="cpu", weights_only=True))
    ParamArena.from_module(model, dev)
    with torch.no_grad():
        logits = torch.cat([model(dense[i:i + 4096], cat[i:i + 4096]).float() for i in range(0, dense.shape[0], 4096)])
    p = torch.sigmoid(logits).cpu().numpy()[:, 0]
    y = label.cpu().numpy()[:, 0]
    acc = float(((p > 0.5) == (y > 0.5)).mean())
    ll = float(-(y * np.log(p + 1e-7) + (1 - y) * np.log(1 - p + 1e-7)).mean())
    old = {"accuracy": acc, "auc": pipeline._auc(p, y), "log_loss": ll, "eval_rows": int(len(y)),
           "baseline_accuracy": float(max(y.mean(), 1 - y.mean())), "blessed": acc >= 0.6}
    assert {k: ev[k] for k in old} == old
    assert ev["path"] == "layerwise" and set(ev["slices"]) == {"trip_start_hour", "pickup_latitude"}
    assert len(ev["slices"]["trip_start_hour"]) == 24 and len(ev["slices"]["pickup_latitude"]) == 10
    for f in ev["slices"]:
        assert sum(s["count"] for s in ev["slices"][f].values()) == ev["eval_rows"]
        assert sum(s["hits"] for s in ev["slices"][f].values()) == round(acc * len(y))
    o = TE.metrics_from_rows(p, TE.bce_with_logits(logits.numpy()[:, 0], y), y)["overall"]
    assert ev["auc_bucketed"] == o["auc_bucketed"] and abs(ev["auc_bucketed"] - ev["auc"]) <= o["auc_bound"] + 1e-12
    on_disk = json.loads((root / "evaluator" / "metrics.json").read_text())
    assert on_disk["path"] == "layerwise" and on_disk["slices"]["trip_start_hour"]["0"]["count"] == \
        ev["slices"]["trip_start_hour"]["0"]["count"]
    # no slices: the keys stay, the dictionary is empty; eval_every is the fused trainer's
    assert pipeline.evaluator(root, device="cpu", slice_by=())["slices"] == {}
    try:
        pipeline.trainer(root, steps=2, device="cpu", eval_every=1)
    except ValueError:
        pass
    else:
        raise AssertionError("eval_every on the CPU")
