"""The plain group-by of featurestore.window (``group_aggregates``: count / sum / mean / min / max per group) on the device
route (groupagg.hip) against the pandas route OF THE SAME BUILD, in one process.

Frames of --rows rows: one integer key column with --groups distinct values and V = 4 columns of random doubles with 1 %
NaN.  ``group_aggregates`` is timed on the host clock, end to end (the fp64 upload, the key sort, the rank search, the
syncs, the downloads and the frame are inside), in alternating windows of one call each: --pairs pairs, medians.
window.GROUP_GPU_MIN_ROWS is the smallest size at which the device route wins every pair at EVERY group count; none:
the route stays opt-in (``device="cuda"``).

Reported beside it, and gated on nothing: the stages alone, by events, on the uploaded frame: the sort of the key
column with the rank search (column_sort64 + column_pair_ranks64), group_keys_k, the sort of the group keys with the
digit passes it ran, group_heads_k (its read of G included), and the reduce and finish kernels of both passes.

usage (GPU): python tools/groupagg_bench.py [--rows 100000,1000000,10000000 --groups 50,100000 --pairs 5 --out FILE]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colsort_bench import LINES, ev_time, pairs_of, say  # noqa: E402

V = 4


def frame(rows, groups):
    rng = np.random.default_rng(rows + groups)
    d = {"key": rng.integers(0, groups, rows)}
    for j in range(V):
        v = rng.standard_normal(rows) * 10.0 ** j
        v[rng.random(rows) < 0.01] = np.nan
        d[f"d{j}"] = v
    return pd.DataFrame(d)


def run(rows, groups, pairs):
    from hops_examples_amd.featurestore import window
    from hops_examples_amd.ops import kernels as K

    df = frame(rows, groups)
    vals = [f"d{j}" for j in range(V)]

    def route(device):
        def f():
            got, r = window.group_aggregates(df, "key", vals, device=device)
            assert r == ("gpu" if device == "cuda" else "cpu")
            return got
        return f

    g = route("cuda")()  # warm-up of the device route
    c = route("cpu")()
    assert g.index.equals(c.index) and (g.xs("count", axis=1, level=1) == c.xs("count", axis=1, level=1)).all().all()
    diff = float(np.nanmax(np.abs(g.to_numpy(np.float64) - c.to_numpy(np.float64)) / np.maximum(np.abs(c.to_numpy(np.float64)), 1.0)))
    tg, tc = pairs_of(route("cuda"), route("cpu"), pairs)
    wins = sum(a < b for a, b in zip(tg, tc))
    mg, mc = statistics.median(tg), statistics.median(tc)
    say(f"== {rows} rows, {len(g)} groups, V = {V}: group_aggregates (count, sum, mean, min, max), {pairs} alternating pairs")
    say(f"  device  median {mg * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in tg))
    say(f"  pandas  median {mc * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in tc))
    say(f"  device / pandas = {mg / mc:.3f}; device faster in {wins} of {pairs} pairs; largest relative difference {diff:.2e}")

    host = np.ascontiguousarray(df.to_numpy(np.float64))
    pinned = torch.from_numpy(host).pin_memory()
    x = pinned.cuda()
    say(f"  upload of fp64 [{rows}, {1 + V}] from pinned memory: {ev_time(lambda: pinned.cuda()):.3f} ms")
    xk = x[:, :1].contiguous()
    order = K.column_sort64(xk)
    say(f"  key column sort + ranks (column_sort64, column_pair_ranks64): "
        f"{ev_time(lambda: K.column_pair_ranks64(xk, [(0, 0)], K.column_sort64(xk))):.3f} ms")
    say(f"  keys (ranks + group_keys_k): {ev_time(lambda: K.group_keys64(xk, [0], order)):.3f} ms")
    keys = K.group_keys64(xk, [0], order)
    passes = K.column_sort_keys64(keys.clone()).passes[0]
    say(f"  sort of the group keys (clone included): {ev_time(lambda: K.column_sort_keys64(keys.clone())):.3f} ms, digit passes "
        f"{passes}")
    K.column_sort_keys64(keys)
    say(f"  heads (group_heads_k x 2 + scan, the read of G included): {ev_time(lambda: K.group_segments64(keys)):.3f} ms")
    seg_off = K.group_segments64(keys)[0]
    for var in (False, True):
        ms = ev_time(lambda: K.group_aggregate64(x, range(1, 1 + V), keys, seg_off, want_var=var))
        say(f"  reduce + finish, {'both passes (var)' if var else 'first pass'} (the column gather of x included): {ms:.3f} ms")
    return {"rows": rows, "groups": groups, "pairs": pairs, "wins": wins, "device_ms": [t * 1e3 for t in tg],
            "pandas_ms": [t * 1e3 for t in tc]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000,10000000")
    ap.add_argument("--groups", default="50,100000")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("groupagg_bench: needs a GPU (nothing is measured without one)")
    say(f"# tools/groupagg_bench.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    sizes = [int(r) for r in a.rows.split(",") if r]
    res = [run(r, int(g), a.pairs) for r in sizes for g in a.groups.split(",") if g]
    won = [r for r in sizes if all(q["wins"] == q["pairs"] for q in res if q["rows"] == r)]
    say(f"# GROUP_GPU_MIN_ROWS: the smallest size won in every pair at every group count: "
        f"{min(won) if won else 'none (device route opt-in)'}")
    for r in res:
        say("JSON " + json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
