"""Batch labelling end to end, from host uint8 batches to decoded (class id, label, score) rows, in the two forms
inference.Predictor offers, in one process:

  (a) probs : predict_batches (graph: forward + torch.softmax; the [B, C] fp32 probabilities cross to the host
              behind a sync) + decode_predictions(top=3) (argsort per row on the host)
  (b) topk  : predict_topk_batches(top=3) (graph: forward + topk.hip; [B, 3] ids and scores cross through pinned
              buffers, the next replay is enqueued before the host labels this batch) + decode_topk

Both run on the same Predictor (frozen engine) over the same ring of host batches, in alternating windows — `--pairs`
pairs, each window at least `--batches` batches and at least `--window` seconds, every graph captured and warmed up
first.  The clock is the host's around a whole window: it ends when the last batch's rows are decoded, so it contains
the copies, the syncs and the host work.  The comparison is between the two forms of this build, never against a
fixed number.

Configurations: frozen ResNet-50 (224 x 224, 1000 classes) at B=100 and B=8, frozen ResNet-20 (32 x 32, 10 classes) at
B=128.  Also: the kernel alone at (B, C) = (100, 1000), (128, 10), (1024, 1000), fp32 and bf16 logits, k=3, as the time
per launch inside a captured graph of 50 launches (it contains the boundary between dependent launches).

usage (GPU): python tools/infer_topk_bench.py [--pairs 5 --batches 40 --window 0.5 --configs ... --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resnet_infer_bench import build  # noqa: E402  (the same models, BN state included)

CONFIGS = {
    "resnet50_b100": ("resnet50", 100, 224),
    "resnet50_b8": ("resnet50", 8, 224),
    "resnet20_b128": ("resnet20", 128, 32),
}
KERNEL_SHAPES = [(100, 1000), (128, 10), (1024, 1000)]
RING = 4  # distinct host batches, cycled
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def form_probs(pr, batches):
    from hops_examples_amd import inference as I

    rows = 0
    for probs in pr.predict_batches(batches):
        rows += len(I.decode_predictions(probs, top=3))
    return rows


def form_topk(pr, batches):
    from hops_examples_amd import inference as I

    rows = 0
    for ids, scores in pr.predict_topk_batches(batches, top=3):
        rows += len(I.decode_topk(ids, scores))
    return rows


FORMS = {"probs": form_probs, "topk": form_topk}


def window(form, pr, ring, n):
    """Seconds per batch over n batches, host clock; the last batch's rows are decoded inside it."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = FORMS[form](pr, (ring[i % RING] for i in range(n)))
    dt = time.perf_counter() - t0
    assert rows == n * len(ring[0])
    return dt / n


def run_config(name, pairs, nb, win):
    from hops_examples_amd import inference as I

    kind, B, hw = CONFIGS[name]
    dev = torch.device("cuda", 0)
    model = build(kind, dev)
    pr = I.Predictor(model, dev, graph=True, frozen=True)
    rng = np.random.default_rng(2)
    ring = [rng.integers(0, 256, (B, hw, hw, 3), dtype=np.uint8) for _ in range(RING)]
    # agreement of the two forms on the same batches (and the warm-up: both slots' graphs of both forms)
    probs = np.concatenate(list(pr.predict_batches(iter(ring))))
    ids, scores = (np.concatenate(x) for x in zip(*pr.predict_topk_batches(iter(ring), top=3)))
    C = probs.shape[1]
    at = np.take_along_axis(probs, ids.astype(np.int64), axis=1)
    same_top1 = float((ids[:, 0] == probs.argmax(1)).mean())
    reps = {}
    for f in FORMS:
        window(f, pr, ring, 8)
        reps[f] = max(nb, int(win / window(f, pr, ring, 12)) + 1)
    times = {f: [] for f in FORMS}
    for p in range(pairs):
        for f in (("topk", "probs") if p % 2 == 0 else ("probs", "topk")):
            times[f].append(window(f, pr, ring, reps[f]))
    wins = sum(t < q for t, q in zip(times["topk"], times["probs"]))
    med = {f: statistics.median(v) for f, v in times.items()}
    say(f"== {name}: B={B} {hw}x{hw}, {C} classes, {pairs} alternating pairs, windows of {reps['probs']} (probs) / "
        f"{reps['topk']} (topk) batches, >= {win} s")
    for f in ("probs", "topk"):
        say(f"  ({'a' if f == 'probs' else 'b'}) {f:<6} median {med[f] * 1e3:8.4f} ms/batch  {B / med[f]:10.0f} img/s   "
            f"windows [ms]: " + " ".join(f"{t * 1e3:.4f}" for t in times[f]))
    say(f"  topk / probs = {med['topk'] / med['probs']:.4f}; topk faster in {wins} of {pairs} pairs; device->host per "
        f"batch: {B * C * 4} B (probs) -> {B * 3 * 8} B (topk); max |score - prob[id]| {np.abs(scores - at).max():.3e}; "
        f"top-1 equal to argmax(probs) in {same_top1 * 100:.1f} % of {len(ids)} rows")
    return {"config": name, "batch": B, "classes": int(C), "pairs": pairs, "batches": reps,
            "probs_ms": [t * 1e3 for t in times["probs"]], "topk_ms": [t * 1e3 for t in times["topk"]],
            "ratio": med["topk"] / med["probs"], "wins": wins, "d2h_bytes": [B * C * 4, B * 3 * 8]}


def kernel_alone():
    from hops_examples_amd.ops import kernels as K
    from hops_examples_amd.runtime.capture import graph

    say("== topk.hip alone, k=3: us per launch inside a graph of 50 launches (median of 7 replays of it)")
    for B, C in KERNEL_SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            z = (torch.randn(B, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 4).to(dt)
            ids = torch.empty(B, 3, dtype=torch.int32, device="cuda")
            scores = torch.empty(B, 3, device="cuda")
            K.softmax_topk(z, 3, ids, scores)
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with graph(cg):
                for _ in range(50):
                    K.softmax_topk(z, 3, ids, scores)
            ts = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                cg.replay()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3 / 50)
            say(f"  ({B:5d}, {C:5d}) {str(dt)[6:]:<8} route {K.softmax_topk_path(z, 3)}  "
                f"{statistics.median(ts[3:]):7.2f} us/launch   logits {z.numel() * z.element_size()} B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_topk_bench: needs a GPU (nothing is measured without one)")
    if a.pairs < 5 or a.batches < 40:
        sys.exit("infer_topk_bench: at least 5 pairs of windows of at least 40 batches")
    say(f"# tools/infer_topk_bench.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    res = [run_config(c, a.pairs, a.batches, a.window) for c in a.configs.split(",") if c]
    kernel_alone()
    lost = [r["config"] for r in res if r["wins"] < r["pairs"]]
    say(f"# default (topk faster in every pair of every configuration -> batch_predict labels through it): "
        f"{'ON' if not lost else 'OPT-IN, lost at: ' + ', '.join(lost)}")
    for r in res:
        say("JSON " + json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
