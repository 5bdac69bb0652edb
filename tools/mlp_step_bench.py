"""The one-launch Dense-stack training step (runtime/mlp_step.py FusedMlpStep) against the layerwise TrainStep,
in alternating timed windows of ONE process (the host and GPU are shared: a difference counts only next to the
spread of both), on the Titanic DNN at batch 10 and the simulated-data MLP at batch 32.

usage: python tools/mlp_step_bench.py [--steps 3200] [--pairs 5] [--out profiles/r24_mlp_step.txt]

Each window runs ``steps`` training steps on a resident synthetic epoch and ends in a device synchronise.  The
TrainStep runs as benchmarks/run.py drives it: ``run_resident`` where its prefetch takes the batch slices (16-byte
multiples), step by step otherwise.  Both engines own a copy of the same initial model."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from hops_examples_amd import optim  # noqa: E402
from hops_examples_amd.models import zoo  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402
from hops_examples_amd.runtime.step import TrainStep, make_step  # noqa: E402

CONFIGS = {"titanic_dnn B=10": (zoo.titanic_dnn, 6, 10), "simulated_mlp B=32": (zoo.simulated_mlp, 10, 32)}


def engine(builder, B, dev, fused):
    torch.manual_seed(0)
    m = builder()
    m.build()
    m.to(dev)
    ParamArena.from_module(m, dev)
    opt = optim.Adam(m, lr=1e-3, eps=1e-7)
    if fused:
        st = make_step(m, opt, "bce_logits", batch=B)
        assert st.kind == "mlp-step", st.note
        return st
    fwd = m._strip_sigmoid() if m.net[-1].activation == "sigmoid" else None  # (keras: logits into the fused loss)
    return TrainStep(m, opt, "bce_logits", graph=True, forward_fn=(lambda mod, x: fwd(x)) if fwd else None)


def window(st, xs, ys, n, resident):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if resident:
        st.run_resident(xs, ys, n)
    else:
        for i in range(n):
            st(xs[i % len(xs)], ys[i % len(xs)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_step_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    lines = []
    for name, (builder, F, B) in CONFIGS.items():
        gen = torch.Generator().manual_seed(1)
        xs = torch.randn(64, B, F, generator=gen).to(dev)
        ys = (xs[:, :, :1] > 0).float().contiguous()
        eng, ts = engine(builder, B, dev, True), engine(builder, B, dev, False)
        ts_res = all(t[0].numel() * t.element_size() % 16 == 0 for t in (xs, ys))
        for _ in range(ts.warmup + 3):  # past the eager warm-up and the graph capture
            ts.step_resident(xs, ys) if ts_res else ts(xs[0], ys[0])
        if ts_res:
            ts.prepare_resident(xs, ys, n=a.steps)
        eng.prepare_resident(xs, ys, n=a.steps)
        window(eng, xs, ys, a.steps, True), window(ts, xs, ys, a.steps, ts_res)  # warm both windows' shapes
        pairs = [(window(eng, xs, ys, a.steps, True), window(ts, xs, ys, a.steps, ts_res)) for _ in range(a.pairs)]
        e, t = [p[0] for p in pairs], [p[1] for p in pairs]
        rec = {"config": name, "steps_per_window": a.steps, "engine_us_per_step": [round(v, 2) for v in e],
               "trainstep_us_per_step": [round(v, 2) for v in t], "trainstep_mode": "run_resident" if ts_res else "per step",
               "engine_wins": sum(x < y for x, y in pairs), "pairs": a.pairs,
               "engine_steps_per_s": round(1e6 / (sum(e) / len(e))), "trainstep_steps_per_s": round(1e6 / (sum(t) / len(t))),
               "engine_spread": round(max(e) / min(e), 3), "trainstep_spread": round(max(t) / min(t), 3),
               "steps_per_launch": eng.steps_per_execution, **eng.geometry(B)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
