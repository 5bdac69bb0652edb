"""The forward + metrics part of the TFX taxi Evaluator (tfx/pipeline.py evaluator): the one-launch sliced
evaluator (runtime/taxi_eval.py, csrc/ops/taxi_eval.hip) against the chunked layer-by-layer forward with the
numpy slices (HOPSX_TAXI_EVAL_FUSED=0) and against the evaluator as it was before slicing (chunked forward,
global accuracy / log-loss / rank AUC only: the parent commit's work, reproduced here), in one process, the
variants alternating call by call.  Every timed call sits between two device synchronisations; medians of
`--reps` calls after 3 warm-up calls, with min / max.  Two sizes: the pipeline example's eval split (a third
of 200,000 trips) and 1,000,000 synthetic rows.

usage (GPU): python tools/taxi_eval_bench.py [--reps 10 --out profiles/FILE.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("taxi_eval_bench: needs a GPU (timings on a CPU say nothing about it)")
    from hops_examples_amd.models import widedeep as WD
    from hops_examples_amd.runtime import taxi_eval as TE
    from hops_examples_amd.runtime.arena import ParamArena
    from hops_examples_amd.tfx import pipeline

    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    model = WD.TaxiWideDeep()
    with torch.no_grad():
        model.wide.weight.copy_(torch.randn(WD.WIDE_ROWS, 1, generator=torch.Generator().manual_seed(1)) * 0.5)
    model.to(dev)
    ParamArena.from_module(model, dev)
    ev = TE.TaxiEvaluator(model)
    say(f"# taxi_eval_bench: {a.reps} timed calls per row after 3 warm-up calls, {torch.cuda.get_device_name(0)}")
    for n in (66_667, 1_000_000):
        dense, cat, label = WD.synth_taxi(n, seed=3, device=dev)
        y = label.cpu().numpy()[:, 0]
        hour = TE.slice_column("trip_start_hour")
        keep = {}

        def chunked():
            with torch.no_grad():
                return torch.cat([model(dense[i:i + 4096], cat[i:i + 4096]).float() for i in range(0, n, 4096)])

        def fused():
            r = ev.run(dense, cat, label, slice_by="trip_start_hour", out=keep.get("out"))
            keep["out"] = r
            keep["m"] = TE.metrics(r)
            keep["p"] = r.prob.cpu().numpy()

        def kernel():
            keep["k"] = ev.run(dense, cat, label, slice_by="trip_start_hour", out=keep.get("k"))

        def layerwise():
            logits = chunked()
            p = torch.sigmoid(logits).cpu().numpy()[:, 0]
            loss = TE.bce_with_logits(logits.cpu().numpy()[:, 0], y)
            keep["m0"] = TE.metrics_from_rows(p, loss, y, TE.slice_ids_of(cat, hour), 24)

        def parent():
            p = torch.sigmoid(chunked()).cpu().numpy()[:, 0]
            acc = float(((p > 0.5) == (y > 0.5)).mean())
            ll = float(-(y * np.log(p + 1e-7) + (1 - y) * np.log(1 - p + 1e-7)).mean())
            keep["old"] = (acc, ll, pipeline._auc(p, y))

        rows = {"fused: run + metrics + probabilities to the host": fused, "fused: the kernel alone (run, out= reused)": kernel,
                "HOPSX_TAXI_EVAL_FUSED=0: chunked forward + numpy slices": layerwise,
                "before slicing: chunked forward + global metrics": parent}
        t = {k: [] for k in rows}
        for r in range(3 + a.reps):
            for k, fn in rows.items():
                ms = timed(fn)
                if r >= 3:
                    t[k].append(ms)
        say(f"\n## n = {n:,} rows (120 B each: {n * 120 / 1e6:.1f} MB of inputs)")
        for k, v in t.items():
            say(f"{k:58s} median {statistics.median(v):10.3f} ms   min {min(v):10.3f}   max {max(v):10.3f}")
        km = statistics.median(t["fused: the kernel alone (run, out= reused)"])
        say(f"kernel alone: {n * 120 / 1e9 / (km / 1e3):.0f} GB/s of inputs; fused / chunked overall accuracy "
            f"{keep['m']['overall']['accuracy']:.6f} / {keep['m0']['overall']['accuracy']:.6f}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
