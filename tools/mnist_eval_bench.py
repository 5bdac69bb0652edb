"""keras evaluate / predict / fit(validation_data=...) of the flagship MNIST CNN: the one-launch evaluator
(runtime/persist_eval.py, csrc/ops/mnist_eval.hip) against the batch-by-batch forward (HOPSX_EVAL_FUSED=0), in
one process, the variants alternating call by call (one box, one process: box-to-box variance cannot fake a
difference).  Every timed call sits between two device synchronisations; medians of `--reps` calls after a
warm-up, with min / max and the inter-quartile range as the spread.

On a tree without the evaluator module the fused rows are absent and the others are the only path there is
(that is how the parent commit is measured).

usage (GPU): python tools/mnist_eval_bench.py [--n 10000 --reps 20 --fit-reps 3 --out profiles/FILE.txt]"""
import argparse
import json
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


def data(n, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 10, n)
    x = rng.integers(0, 60, (n, 28, 28, 1)).astype(np.uint8)
    for c in range(10):  # a learnable signal: a bright class-dependent stripe
        x[y == c, 2 * c + 3: 2 * c + 5, 4:24, 0] = 230
    return x, y.astype(np.int64)


def model(keras):
    m = keras.Sequential([
        keras.layers.Conv2D(32, 2, activation="relu", input_shape=(28, 28, 1)),
        keras.layers.Conv2D(64, 2, activation="relu"),
        keras.layers.MaxPooling2D(),
        keras.layers.Dropout(0.01),
        keras.layers.Flatten(),
        keras.layers.Dense(128, activation="relu"),
        keras.layers.Dense(10, activation="softmax"),
    ])
    m.compile(optimizer=keras.optimizers.Adadelta(1.0), loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    return m


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iqr_ms": q[2] - q[0], "calls": len(v)}


def fmt(s):
    return (f"median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}   "
            f"IQR {s['iqr_ms']:7.3f}   ({s['calls']} calls)")


def alternate(variants, reps, warmup=3):
    """variants: name -> (env, fn).  Alternates them call by call; returns name -> stats."""
    base = dict(os.environ)
    out = {k: [] for k in variants}
    for r in range(warmup + reps):
        for k, (env, fn) in variants.items():
            os.environ.update(env)
            try:
                t = timed(fn)
            finally:
                os.environ.clear()
                os.environ.update(base)
            if r >= warmup:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


def accuracy(say):
    """The kernel's actual errors on the GPU tests' setup (tests/test_mnist_eval_gpu.py): seed 1, fc2.weight x 16,
    97 random images (seed 9); fp64 reference and fp32 proxy with the kernel's bf16 rounding points."""
    from hops_examples_amd.models.mnist import MirroredMnistCNN
    from hops_examples_amd.runtime import persist_eval
    from hops_examples_amd.runtime.arena import ParamArena

    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    m = MirroredMnistCNN().to(dev)
    arena = ParamArena.from_module(m, dev)
    with torch.no_grad():
        m.fc2.weight.mul_(16.0)
    arena.refresh_shadow()
    ev = persist_eval.MnistEvaluator(m)
    x = torch.randint(0, 256, (3 * ev.tile + 1, 28, 28, 1), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    named = dict(m.named_parameters())
    P = {k: named[k].detach().cpu().clone() for k in persist_eval.PARAMS}
    kw = dict(xscale=float(m.conv1.in_affine[0]), xshift=float(m.conv1.in_affine[1]), emulate_bf16=True)
    ref = persist_eval.reference_logits(P, x, **kw)
    proxy = persist_eval.reference_logits(P, x, dtype=torch.float32, **kw).double()
    am = ref.argmax(1)
    y = torch.where(torch.arange(len(x)) % 2 == 0, am, (am + 1) % 10)
    r = ev.run(x.to(dev), y.to(dev))
    z = r.logits.double().cpu()
    ce = lambda t: torch.nn.functional.cross_entropy(t, y, reduction="none")  # noqa: E731
    e32, ek = float((proxy - ref).abs().max()), float((z - ref).abs().max())
    c32, ck = float((ce(proxy) - ce(ref)).abs().max()), float((r.loss.double().cpu() - ce(ref)).abs().max())
    cos = float(torch.nn.functional.cosine_similarity(z, ref, dim=1).min())
    say(f"accuracy (97 images): logits max err kernel {ek:.3e} / fp32 proxy {e32:.3e} = {ek / e32:.2f} x;  "
        f"CE max err kernel {ck:.3e} / proxy {c32:.3e} = {ck / c32:.2f} x;  min cosine {cos:.9f}")
    return {"logits_err": ek, "e32": e32, "ce_err": ck, "ce_proxy": c32, "min_cos": cos}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--train", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mnist_eval_bench: needs a GPU (timings on a CPU say nothing about it)")
    from hops_examples_amd import keras

    try:
        from hops_examples_amd.runtime import persist_eval
    except ImportError:
        persist_eval = None
    fused = persist_eval is not None
    res = {"n": a.n, "fused_available": fused, "device": torch.cuda.get_device_name(0)}
    say(f"# mnist_eval_bench: N = {a.n} images, {a.reps} timed calls per row after 3 warm-up calls, "
        f"{res['device']}; one-launch evaluator {'present' if fused else 'ABSENT (this tree has only the batch-by-batch path)'}")
    torch.manual_seed(0)
    m = model(keras)
    x, y = data(a.n, seed=1)
    xt, yt = data(a.train, seed=2)
    m.fit(xt[:4096], yt[:4096], batch_size=32, epochs=1, verbose=0)  # builds the model, trains it a little

    off = {"HOPSX_EVAL_FUSED": "0"}
    ev_rows = {}
    if fused:
        ev_rows["evaluate fused (one launch)"] = ({}, lambda: m.evaluate(x, y, batch_size=32, verbose=0))
    ev_rows["evaluate batch-by-batch bs=32"] = (off, lambda: m.evaluate(x, y, batch_size=32, verbose=0))
    ev_rows["evaluate batch-by-batch bs=1024"] = (off, lambda: m.evaluate(x, y, batch_size=1024, verbose=0))
    if fused:
        ev_rows["predict fused (one launch)"] = ({}, lambda: m.predict(x))
    ev_rows["predict batch-by-batch bs=256"] = (off, lambda: m.predict(x, batch_size=256))
    res["calls"] = alternate(ev_rows, a.reps)
    for k, s in res["calls"].items():
        say(f"{k:34s} {fmt(s)}")
    if fused:
        a_, b_ = m.evaluate(x, y, verbose=0, return_dict=True), None
        os.environ["HOPSX_EVAL_FUSED"] = "0"
        try:
            b_ = m.evaluate(x, y, batch_size=32, verbose=0, return_dict=True)
        finally:
            os.environ.pop("HOPSX_EVAL_FUSED")
        say(f"same model, same set: fused {a_}  batch-by-batch {b_}")
        res["agreement"] = {"fused": a_, "batch": b_}
        # the kernel alone (device copies resident, no host read), and one image: 169 serial positions on one workgroup
        eng = m._eval_engine
        xs, ys = m._eval_resident(x, y)
        k_rows = {"kernel only, N images": ({}, lambda: eng.run(xs, ys)),
                  "kernel only, 1 image": ({}, lambda: eng.run(xs[:1], ys[:1]))}
        res["kernel"] = alternate(k_rows, a.reps)
        for k, s in res["kernel"].items():
            say(f"{k:34s} {fmt(s)}")

    # per-epoch cost of fit(validation_data=...): an epoch with validation minus an epoch without, batch 32
    fit_rows = {"fit epoch, no validation": ({}, lambda: m.fit(xt, yt, batch_size=32, epochs=1, verbose=0))}
    if fused:
        fit_rows["fit epoch + validation, fused"] = (
            {}, lambda: m.fit(xt, yt, batch_size=32, epochs=1, verbose=0, validation_data=(x, y)))
    fit_rows["fit epoch + validation, batch-by-batch"] = (
        off, lambda: m.fit(xt, yt, batch_size=32, epochs=1, verbose=0, validation_data=(x, y)))
    res["fit"] = alternate(fit_rows, a.fit_reps, warmup=1)
    say(f"# fit: {a.train} training images, {a.n} validation images, batch 32, one epoch per call")
    for k, s in res["fit"].items():
        say(f"{k:40s} {fmt(s)}")
    base = res["fit"]["fit epoch, no validation"]["median_ms"]
    for k, s in res["fit"].items():
        if "validation," in k:
            say(f"  per-epoch validation cost, {k.split(', ')[1]:16s} {s['median_ms'] - base:9.3f} ms  (epoch alone {base:.3f} ms)")
    if fused:
        res["accuracy"] = accuracy(say)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
