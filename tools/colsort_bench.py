"""The order rules of featurestore.rules (distinct / uniqueness / entropy / quantile) on the device route (one
colsort.hip sort of the eligible columns) against the pandas route OF THE SAME BUILD, in one process.

Frames of --rows rows x 8 numeric columns: four low-cardinality integer columns, four columns of random doubles, 1 % NaN
in the doubles.  `validate` with one expectation per order rule over all 8 columns is timed on the host clock (the
fp64 upload, the syncs and the host work are inside), in alternating windows of one validate each: --pairs pairs,
medians.  The threshold rules.ORDER_GPU_MIN_ROWS is the smallest size at which the device route wins every pair.

Reported beside it, and gated on nothing: statistics.distinct_counts on either route (approximateNumDistinctValues of
statistics.compute), the sort kernels alone (events around column_sort64 with a caller-owned workspace; per digit pass
and as effective bytes per second, passes x 16 B x rows x cols / time), column_runs64 alone, and torch.sort of the same
keys as a yardstick.

usage (GPU): python tools/colsort_bench.py [--rows 100000,1000000,10000000 --pairs 5 --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def frame(rows):
    rng = np.random.default_rng(rows)
    d = {}
    for j, card in enumerate((2, 10, 100, 1000)):
        d[f"i{j}"] = rng.integers(0, card, rows)
    for j in range(4):
        v = rng.standard_normal(rows) * 10.0 ** j
        v[rng.random(rows) < 0.01] = np.nan
        d[f"d{j}"] = v
    return pd.DataFrame(d)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def pairs_of(fa, fb, pairs):
    ta, tb = [], []
    for p in range(pairs):
        for which in ((0, 1) if p % 2 == 0 else (1, 0)):
            (ta if which == 0 else tb).append(timed(fa if which == 0 else fb)[0])
    return ta, tb


def ev_time(fn, reps=5):
    ts = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts[2:])


def run(rows, pairs):
    from hops_examples_amd.featurestore import rules, statistics as S
    from hops_examples_amd.featurestore.rules import Expectation, Rule
    from hops_examples_amd.ops import kernels as K

    df = frame(rows)
    feats = list(df.columns)
    exps = [Expectation(n.lower(), feats, [Rule(n, min=0)]) for n in rules._ORDER_RULES]

    def route(thr):
        def f():
            rules.ORDER_GPU_MIN_ROWS = thr
            v = rules.validate(df, exps, 1)
            assert v.order_device == ("gpu" if thr == 0 else "cpu")
            return [r.value for e in v.expectation_results for r in e.results]
        return f

    keep = rules.ORDER_GPU_MIN_ROWS
    try:
        _, vg = timed(route(0))  # warm-up of the device route, and agreement of the two
        tg, tc = pairs_of(route(0), route(10 ** 12), pairs)
        vc = route(10 ** 12)()
    finally:
        rules.ORDER_GPU_MIN_ROWS = keep
    diff = max(abs(float(a) - float(b)) for a, b in zip(vg, vc))
    wins = sum(a < b for a, b in zip(tg, tc))
    mg, mc = statistics.median(tg), statistics.median(tc)
    say(f"== {rows} rows x {len(feats)} columns: validate, 7 order rules x 8 features, {pairs} alternating pairs")
    say(f"  device  median {mg * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in tg))
    say(f"  pandas  median {mc * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in tc))
    say(f"  device / pandas = {mg / mc:.4f}; device faster in {wins} of {pairs} pairs; largest |value difference| {diff:.3e}")

    sg, sc = pairs_of(lambda: S.distinct_counts(df, feats, device=True), lambda: S.distinct_counts(df, feats, device=False),
                      pairs)
    swins = sum(a < b for a, b in zip(sg, sc))
    assert S.distinct_counts(df, feats, device=True) == S.distinct_counts(df, feats, device=False)
    say(f"  statistics.distinct_counts: device median {statistics.median(sg) * 1e3:.1f} ms, pandas "
        f"{statistics.median(sc) * 1e3:.1f} ms; device faster in {swins} of {pairs} pairs")

    x = torch.from_numpy(np.ascontiguousarray(df.to_numpy(np.float64))).cuda()
    ws = torch.empty(K.column_sort_ws_words(rows, 8), dtype=torch.int64, device="cuda")
    order = K.column_sort64(x, ws=ws)
    for name, sl in (("integers", slice(0, 4)), ("doubles", slice(4, 8))):
        xs = x[:, sl].contiguous()
        o = K.column_sort64(xs, ws=ws)
        npass = len(o.passes[0])
        ms = ev_time(lambda: K.column_sort64(xs, ws=ws))
        say(f"  sort alone, 4 {name} columns: {ms:8.3f} ms, {npass} digit passes {o.passes[0]}, {ms / max(npass, 1):.3f} ms "
            f"per pass (encode and histograms included), {npass * 16 * rows * 4 / (ms * 1e-3) / 1e9:.1f} GB/s effective")
    rs = ev_time(lambda: K.column_runs64(order))
    ts = ev_time(lambda: torch.sort(order.keys, dim=1))
    say(f"  column_runs64 alone, 8 columns: {rs:.3f} ms;  torch.sort of the same 8 x {rows} int64 keys: {ts:.3f} ms")
    return {"rows": rows, "device_ms": [t * 1e3 for t in tg], "pandas_ms": [t * 1e3 for t in tc], "wins": wins,
            "pairs": pairs, "stats_device_ms": [t * 1e3 for t in sg], "stats_pandas_ms": [t * 1e3 for t in sc],
            "stats_wins": swins}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000,10000000")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("colsort_bench: needs a GPU (nothing is measured without one)")
    say(f"# tools/colsort_bench.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    res = [run(int(r), a.pairs) for r in a.rows.split(",") if r]
    won = [r["rows"] for r in res if r["wins"] == r["pairs"]]
    say(f"# ORDER_GPU_MIN_ROWS: the smallest size won in every pair: {min(won) if won else 'none (device route opt-in)'}")
    for r in res:
        say("JSON " + json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
