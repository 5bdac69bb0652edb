"""ResNet inference, frozen (runtime/frozen.py: BatchNorm folded into the convs, the residual in the conv
epilogue) against unfrozen (model.eval(): conv + bn_fwd_infer launches), in one process: both forwards
(+ softmax, what inference.Predictor replays) are captured into hipGraphs over the same device-resident uint8
batch and timed alternately — `--pairs` pairs of windows of at least `--window` seconds each, every shape
warmed up first.  The comparison is between the two paths of this build, never against a fixed number.

Configurations: ResNet-20 at B=128, ResNet-50 (224 x 224) at B=8, 64 and 100 (the batch-inference example's
batch size).  Per configuration: the time per forward of every window, the medians, how many pairs the frozen
path won, the conv routes of the layers that take a residual, and the distance of both outputs to each other.

`--trace CONFIG`: instead, run one configuration for a separate `rocprofv3 --kernel-trace --stats -- python
tools/resnet_infer_bench.py --trace resnet50_b8 --only frozen` run: per path (`--only frozen|unfrozen`: one path)
3 eager warm-up forwards, the capture and 13 graph replays, i.e. 16 forwards in the kernel table (and, for the
frozen path, the torch elementwise kernels of the fold at freeze time, once).  The frozen table has no BatchNorm
inference kernel (bn_apply8_k) rows.

usage (GPU): python tools/resnet_infer_bench.py [--pairs 5 --window 0.5 --configs resnet20_b128,... --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "resnet20_b128": ("resnet20", 128, 32),
    "resnet50_b8": ("resnet50", 8, 224),
    "resnet50_b64": ("resnet50", 64, 224),
    "resnet50_b100": ("resnet50", 100, 224),
}
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def build(kind, dev):
    from hops_examples_amd.models.resnet import cifar_resnet, resnet50
    from hops_examples_amd.runtime.arena import ParamArena

    torch.manual_seed(0)
    m = (cifar_resnet(20) if kind == "resnet20" else resnet50()).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # a trained model's BN state is not the identity
        for mod in m.modules():
            if hasattr(mod, "running_var"):
                n = mod.weight.numel()
                mod.weight.copy_(0.5 + torch.rand(n, generator=g))
                mod.bias.copy_(torch.rand(n, generator=g) - 0.5)
                mod.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
                mod.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
    ParamArena.from_module(m, dev)
    return m


def capture(fn, x):
    from hops_examples_amd.runtime.capture import graph

    with torch.no_grad():
        for _ in range(3):  # warm-up: allocations, kernel selection, code-object loads
            fn(x)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with graph(cg):
            out = fn(x)
    for _ in range(3):
        cg.replay()
    torch.cuda.synchronize()
    return cg, out


def window(cg, n):
    """Seconds per replay over n replays between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        cg.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def residual_routes(frozen, x):
    from hops_examples_amd.ops import kernels as K

    routes = {}
    for name, xin, res, out in frozen.trace(x):
        if res is None:
            continue
        w, _ = frozen.folded(name)
        st, pd, _ = frozen._cfg[name]
        geom = K.conv_geom(xin.shape, w.shape, (st, st), (pd, pd), (1, 1))
        key = (K.conv2d_fwd_res_path(geom), f"{w.shape[3]}->{w.shape[0]} {w.shape[1]}x{w.shape[2]} @{out.shape[1]}x{out.shape[2]}")
        routes[key] = routes.get(key, 0) + 1
    return routes


def paths(model):
    from hops_examples_amd.runtime.frozen import FrozenResNet

    frozen = FrozenResNet.freeze(model)
    return frozen, {"frozen": lambda t: torch.softmax(frozen(t).float(), dim=-1),
                    "unfrozen": lambda t: torch.softmax(model(t).float(), dim=-1)}


def run_config(name, pairs, win):
    kind, B, hw = CONFIGS[name]
    dev = torch.device("cuda", 0)
    model = build(kind, dev)
    x = torch.randint(0, 256, (B, hw, hw, 3), dtype=torch.uint8, device=dev,
                      generator=torch.Generator(device=dev).manual_seed(2))
    frozen, fns = paths(model)
    graphs = {k: capture(fn, x) for k, fn in fns.items()}
    diff = (graphs["frozen"][1] - graphs["unfrozen"][1]).abs().max().item()
    reps = {k: max(3, int(win / window(cg, 20)) + 1) for k, (cg, _) in graphs.items()}
    times = {k: [] for k in graphs}
    for p in range(pairs):
        for k in (("frozen", "unfrozen") if p % 2 == 0 else ("unfrozen", "frozen")):
            times[k].append(window(graphs[k][0], reps[k]))
    wins = sum(f <= u for f, u in zip(times["frozen"], times["unfrozen"]))
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"== {name}: B={B} {hw}x{hw}, {pairs} alternating pairs, windows >= {win} s "
        f"({reps['frozen']} / {reps['unfrozen']} replays)")
    for k in ("frozen", "unfrozen"):
        say(f"  {k:<9} median {med[k] * 1e3:8.4f} ms/forward  {B / med[k]:10.0f} img/s   windows [ms]: "
            + " ".join(f"{t * 1e3:.4f}" for t in times[k]))
    say(f"  frozen / unfrozen = {med['frozen'] / med['unfrozen']:.4f}; frozen not slower in {wins} of {pairs} pairs; "
        f"max |softmax difference| {diff:.3e}")
    for (route, shape), n in sorted(residual_routes(frozen, x).items()):
        say(f"  residual convs on {route:<6} {n:2d} x {shape}")
    return {"config": name, "batch": B, "pairs": pairs, "window_s": win, "frozen_ms": [t * 1e3 for t in times["frozen"]],
            "unfrozen_ms": [t * 1e3 for t in times["unfrozen"]], "ratio": med["frozen"] / med["unfrozen"], "wins": wins,
            "softmax_diff": diff}


def trace_config(name, only):
    kind, B, hw = CONFIGS[name]
    dev = torch.device("cuda", 0)
    model = build(kind, dev)
    x = torch.randint(0, 256, (B, hw, hw, 3), dtype=torch.uint8, device=dev)
    _, fns = paths(model)
    for k, fn in fns.items():
        if only in (None, k):
            cg, _ = capture(fn, x)
            for _ in range(10):
                cg.replay()
            torch.cuda.synchronize()
            print(f"[trace] {name}: 10 more replays of the {k} graph", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, metavar="CONFIG")
    ap.add_argument("--only", default=None, choices=["frozen", "unfrozen"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resnet_infer_bench: needs a GPU (nothing is measured without one)")
    if a.pairs < 5 or a.window < 0.5:
        sys.exit("resnet_infer_bench: at least 5 pairs of windows of at least 0.5 s")
    if a.trace:
        trace_config(a.trace, a.only)
        return
    say(f"# tools/resnet_infer_bench.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    res = [run_config(c, a.pairs, a.window) for c in a.configs.split(",")]
    slower = [r["config"] for r in res if r["wins"] < r["pairs"] - 1]
    say(f"# acceptance (frozen not slower in >= pairs - 1 pairs of every configuration): "
        f"{'PASS' if not slower else 'FAIL: ' + ', '.join(slower)}")
    for r in res:
        say("JSON " + json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
