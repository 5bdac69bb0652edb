"""``Query.read`` of a two-join star query on the device route (join.hip, ``read_options={"join_device": "cuda"}``)
against the sqlite route OF THE SAME BUILD, in one process.

A feature store with sales (--rows rows: store, dept, date, weekly_sales), stores (45 rows: store, size, type) and
exogenous (45 x 143 rows: store, date, fuel_price, cpi):
``sales.select_all().join(stores.select_all()).join(exogenous.select_all())``.  One ``Query.read`` per window on the host
clock, end to end (the frames' read, the uploads, the sorts, the syncs, the downloads and the frame are inside), in
alternating windows: --pairs pairs, medians.  join.JOIN_GPU_MIN_ROWS is the smallest size at which the device route
wins every pair; none: the route stays opt-in.  Above --sql-max-rows the sqlite side is skipped (said so in the output).

Reported beside it, and gated on nothing: ``pandas.merge`` of the same frames (the yardstick for ``equi_join``, which has
no sqlite in front of it) and, at the largest size, the kernels alone by events on the uploaded sales x exogenous join:
spans, the offset scans, the expand and the gather.

usage (GPU): python tools/join_bench.py [--rows 10000,100000,1000000 --pairs 5 --sql-max-rows 1000000 --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colsort_bench import LINES, ev_time, pairs_of, say  # noqa: E402

STORES, DATES = 45, 143


def frames(rows):
    rng = np.random.default_rng(rows)
    sales = pd.DataFrame({"store": rng.integers(1, STORES + 1, rows), "dept": rng.integers(1, 100, rows),
                          "date": rng.integers(0, DATES, rows), "weekly_sales": rng.lognormal(9.0, 1.0, rows)})
    stores = pd.DataFrame({"store": np.arange(1, STORES + 1), "size": rng.integers(30000, 220000, STORES),
                           "type": rng.integers(0, 3, STORES)})
    sd = [(s, d) for s in range(1, STORES + 1) for d in range(DATES)]
    exo = pd.DataFrame({"store": [s for s, _ in sd], "date": [d for _, d in sd],
                        "fuel_price": rng.uniform(2, 4, len(sd)), "cpi": rng.uniform(120, 230, len(sd))})
    return sales, stores, exo


def kernels_alone(sales, exo):
    from hops_examples_amd.ops import _C
    from hops_examples_amd.ops import kernels as K
    from hops_examples_amd.ops._C import ptr, stream

    ext, T = _C.ext(), K.join_tile()
    xl = torch.from_numpy(np.ascontiguousarray(sales.to_numpy(np.float64))).cuda()
    xr = torch.from_numpy(np.ascontiguousarray(exo.to_numpy(np.float64))).cuda()
    nl, nr = len(xl), len(xr)
    n = nl + nr
    say(f"  kernels alone, sales x exogenous on (store, date): {nl} x {nr} rows")
    say(f"    join_pairs64 whole (key sorts, ranks, spans, scans, the read of n_out, expand): "
        f"{ev_time(lambda: K.join_pairs64(xl, xr, [0, 2], [0, 1])):.3f} ms")
    xk = torch.cat([xl[:, [0, 2]], xr[:, [0, 1]]], 0).contiguous()
    keys = K.group_keys64(xk, [0, 1], K.column_sort64(xk))
    K.column_sort_keys64(keys)
    e = lambda m, dt=torch.int64: torch.empty(m, device="cuda", dtype=dt)  # noqa: E731
    seg, first, split, ginfo, heads = e(n + 1), e(n), e(n), e(2), e((n + K.group_tile() - 1) // K.group_tile(), torch.int32)
    rbeg, rcnt, lcnt = e(nl, torch.int32), e(nl, torch.int32), e(nr, torch.int32)
    off, info, tot, nz = e(nl + 1), e(2), e((nl + T - 1) // T), e((nl + T - 1) // T, torch.int32)
    spans = lambda: ext.join_spans64(ptr(keys), nl, nr, ptr(heads), ptr(seg), ptr(first), ptr(ginfo), ptr(split),  # noqa: E731
                                     ptr(rbeg), ptr(rcnt), ptr(lcnt), 0, stream())
    scan = lambda: ext.join_offsets64(ptr(rcnt), nl, 0, ptr(tot), ptr(nz), ptr(off), ptr(info), 0, stream())  # noqa: E731
    say(f"    spans (group_heads_k x 2 + scan, split_k, spans_k): {ev_time(spans):.3f} ms")
    say(f"    offsets (totals_k, scantot_k, local_k): {ev_time(scan):.3f} ms")
    n_out = int(info.cpu()[0])
    li, ri = e(n_out, torch.int32), e(n_out, torch.int32)
    expand = lambda: ext.join_expand64(ptr(keys), nl, nr, ptr(off), ptr(rbeg), ptr(rcnt), n_out, ptr(li), ptr(ri), 0, stream())  # noqa: E731
    say(f"    expand_k, {n_out} pairs: {ev_time(expand):.3f} ms")
    ms = ev_time(lambda: K.join_gather64(xl, xr, li, ri, [0, 1, 2, 3], [2, 3]))
    say(f"    gather_k, fp64 [{n_out}, 6] (its allocation included): {ms:.3f} ms = {n_out * 6 * 16 / ms / 1e6:.1f} GB/s read + written")


def run(rows, pairs, sql_max_rows, fs, last):
    sales, stores, exo = frames(rows)
    fgs = []
    for name, df, pk in (("sales", sales, ["store", "dept", "date"]), ("stores", stores, ["store"]),
                         ("exogenous", exo, ["store", "date"])):
        fg = fs.create_feature_group(f"{name}_{rows}", 1, primary_key=pk)
        fg.save(df)
        fgs.append(fg)
    q = fgs[0].select_all().join(fgs[1].select_all()).join(fgs[2].select_all())

    def route(opts, want):
        def f():
            got = q.read(read_options=opts)
            assert q.last_read_route.startswith(want), q.last_read_route
            return got
        return f

    dev, sql = route({"join_device": "cuda"}, "gpu"), route(None, "sql")
    merge = lambda: sales.merge(stores, on="store").merge(exo, on=["store", "date"])  # noqa: E731
    g = dev()  # warm-up of the device route
    say(f"== {rows} sales rows -> {len(g)} joined rows x {g.shape[1]} columns, {pairs} alternating pairs of one Query.read")
    res = {"rows": rows, "pairs": pairs}
    if rows <= sql_max_rows:
        by = list(g.columns)
        s = sql()
        pd.testing.assert_frame_equal(g.sort_values(by, kind="stable").reset_index(drop=True),
                                      s.sort_values(by, kind="stable").reset_index(drop=True))
        tg, ts = pairs_of(dev, sql, pairs)
        wins = sum(a < b for a, b in zip(tg, ts))
        say(f"  device  median {statistics.median(tg) * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in tg))
        say(f"  sqlite  median {statistics.median(ts) * 1e3:10.1f} ms   windows [ms]: " + " ".join(f"{t * 1e3:.1f}" for t in ts))
        say(f"  device / sqlite = {statistics.median(tg) / statistics.median(ts):.3f}; device faster in {wins} of {pairs} pairs; "
            f"frames equal after sorting by all columns")
        res.update(wins=wins, device_ms=[t * 1e3 for t in tg], sqlite_ms=[t * 1e3 for t in ts])
    else:
        tg, _ = pairs_of(dev, lambda: None, pairs)
        say(f"  device  median {statistics.median(tg) * 1e3:10.1f} ms; sqlite side skipped above {sql_max_rows} rows")
        res.update(wins=None, device_ms=[t * 1e3 for t in tg])
    tm, _ = pairs_of(merge, lambda: None, pairs)
    say(f"  pandas.merge x 2 of the same frames (no store read, no SQL dtypes): median {statistics.median(tm) * 1e3:.1f} ms")
    res["merge_ms"] = [t * 1e3 for t in tm]
    if last:
        kernels_alone(sales, exo)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,100000,1000000")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sql-max-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("join_bench: needs a GPU (nothing is measured without one)")
    os.environ["HOPSX_PROJECT_ROOT"] = tempfile.mkdtemp(prefix="join_bench_")
    os.environ.setdefault("HOPSX_PROJECT_NAME", "demo")
    import hops_examples_amd.featurestore as hsfs

    fs = hsfs.connection().get_feature_store()
    say(f"# tools/join_bench.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    sizes = [int(r) for r in a.rows.split(",") if r]
    res = [run(r, a.pairs, a.sql_max_rows, fs, r == max(sizes)) for r in sizes]
    won = [q["rows"] for q in res if q["wins"] == q["pairs"]]
    say(f"# JOIN_GPU_MIN_ROWS counts the rows of all joined frames: the smallest size won in every pair: "
        f"{min(won) if won else 'none (device route opt-in)'} sales rows (+ {STORES + STORES * DATES} rows of the other two)")
    for r in res:
        say("JSON " + json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
