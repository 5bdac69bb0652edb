"""keras evaluate / predict of the E1 / E8 / E11 CNN family: the one-launch evaluator (runtime/cnn_eval.py,
csrc/ops/cnn_eval.hip) against the batch-by-batch forward (HOPSX_EVAL_FAMILY=0, the code every earlier commit
runs) at batch 32 and 1024, in one process.  Per geometry and batch size: `--pairs` pairs of alternating windows
of `--calls` calls, every window ended by a device synchronise, after a warm-up of both routes; reported are the
ms per call of each route (median over the windows), the pairs the engine won, and the spread (max - min over
its windows) of the batch-by-batch route itself.  Also the largest |difference| of the two routes' predict
outputs, and the conv2 + fc1 operation count of the shape (FLOP/s = that count over a kernel time, which
`--kernel-only` under `rocprofv3 --kernel-trace --stats -- python tools/cnn_eval_bench.py --kernel-only` gives).

usage (GPU): python tools/cnn_eval_bench.py [--n 10000 --pairs 5 --calls 3 --out profiles/FILE.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMS = [(4, 4, 0), (3, 2, 1), (2, 2, 0), (8, 8, 1)]
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def flops(k, p, pad, n):
    """2 x multiply-adds of conv2 over the pooled (floor) region and of fc1, for n images."""
    s = (28 if pad else 30 - 2 * k) // p
    return n * 2 * ((s * p) ** 2 * k * k * 32 * 64 + s * s * 64 * 128)


def window(fn, calls, env):
    base = dict(os.environ)
    os.environ.update(env)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    finally:
        os.environ.clear()
        os.environ.update(base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="5 engine launches per geometry and nothing else")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cnn_eval_bench: needs a GPU (timings on a CPU say nothing about it)")
    from hops_examples_amd.models import zoo

    on, off = {"HOPSX_EVAL_FAMILY": "1"}, {"HOPSX_EVAL_FAMILY": "0"}
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (a.n, 28, 28, 1)).astype(np.uint8)
    y = rng.integers(0, 10, a.n).astype(np.int64)
    res = {"n": a.n, "device": torch.cuda.get_device_name(0), "rows": []}
    say(f"# cnn_eval_bench: N = {a.n} resident images, {a.pairs} pairs of alternating windows of {a.calls} calls, "
        f"{res['device']}")
    for k, p, pad in GEOMS:
        torch.manual_seed(0)
        m = (zoo.fashion_mnist_cnn if pad else zoo.keras_mnist_cnn)(kernel=k, pool=p)
        m.compile(optimizer="adam", loss="sparse_categorical_crossentropy", metrics=["accuracy"])
        os.environ.update(on)
        m.evaluate(x, y, verbose=0)  # builds the model and the engine, uploads the set
        eng = m._family_engine
        name = f"k{k} p{p} {'same' if pad else 'valid'}"
        if a.kernel_only:
            xs, ys = m._eval_resident(x, y)
            for _ in range(5):
                eng.run(xs, ys)
            torch.cuda.synchronize()
            say(f"{name}: tile {eng.plan.tile}, LDS {eng.plan.lds} B, conv2 + fc1 {flops(k, p, pad, a.n) / 1e9:.2f} GFLOP per launch")
            continue
        for bs in (32, 1024):
            ev = lambda: m.evaluate(x, y, batch_size=bs, verbose=0)  # noqa: E731
            window(ev, 1, on), window(ev, 1, off)
            t_on, t_off = [], []
            for _ in range(a.pairs):
                t_on.append(window(ev, a.calls, on))
                t_off.append(window(ev, a.calls, off))
            won = sum(u < v for u, v in zip(t_on, t_off))
            row = {"geometry": name, "batch": bs, "engine_ms": statistics.median(t_on),
                   "batched_ms": statistics.median(t_off), "won": won, "pairs": a.pairs,
                   "batched_spread_ms": max(t_off) - min(t_off)}
            res["rows"].append(row)
            say(f"{name:12s} evaluate bs={bs:<5d} engine {row['engine_ms']:8.3f} ms/call   batch-by-batch "
                f"{row['batched_ms']:8.3f} ms/call (spread {row['batched_spread_ms']:.3f})   won {won}/{a.pairs}")
        p1 = m.predict(x)
        os.environ.update(off)
        p0 = m.predict(x, batch_size=1024)
        os.environ.update(on)
        d = float(np.abs(p1 - p0).max())
        res["rows"].append({"geometry": name, "predict_max_abs_diff": d})
        say(f"{name:12s} predict: largest |engine - batch-by-batch| {d:.3e}; tile {eng.plan.tile}, LDS {eng.plan.lds} B, "
            f"conv2 + fc1 {flops(k, p, pad, a.n) / 1e9:.2f} GFLOP per launch")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
