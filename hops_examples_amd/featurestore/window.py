"""Spark-style range windows for feature engineering:
``F.sum(col).over(Window.partitionBy(keys).orderBy(ts).rangeBetween(lo, hi))``.

Reference: notebooks/featurestore/hsfs/basics/feature_engineering.ipynb:229-249 — weekly sales
summed over the last 30/90/180/365 days (``rangeBetween(days(-N), days(-1))``) per (store, dept)
and per store, then ``fillna(0)``.

The host sorts the rows by (partition, order key) and finds the partition boundaries; the sums run
on the GPU (``window.hip``: fp64 prefix sum + two binary searches per row and window, every window
in one launch) when a GPU is present and the frame is large enough to pay for the copies, else
through the same algorithm in numpy.  An empty range gives NaN (Spark's null) — fill as the
reference does.  Result order is the input frame's order.

``group_aggregates`` is the plain group-by beside them (``groupBy().sum()`` / ``count()`` / ``avg()``,
``sales.groupby("store")``): pandas' own frame, from ``groupagg.hip`` for large numeric frames.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

GPU_MIN_ROWS = 50_000
DAY = 86_400


def days(i: int) -> int:
    """Seconds in ``i`` days (the reference's ``days = lambda i: i * 86400``)."""
    return int(i) * DAY


def _sorted_layout(df: pd.DataFrame, partition_by, order_by: str):
    keys = [partition_by] if isinstance(partition_by, str) else list(partition_by)
    ts = pd.to_numeric(df[order_by], errors="coerce")
    if ts.isna().any():
        raise ValueError(f"order column {order_by!r} has missing values")
    codes = [pd.factorize(df[k], sort=True)[0] for k in keys]
    order = np.lexsort([ts.to_numpy()] + codes[::-1])
    newseg = np.ones(len(order), bool)
    if len(order) > 1:
        newseg[1:] = False
        for c in codes:
            cs = c[order]
            newseg[1:] |= cs[1:] != cs[:-1]
    seg = np.cumsum(newseg) - 1
    seg_off = np.concatenate([np.flatnonzero(newseg), [len(order)]]).astype(np.int64)
    return order, ts.to_numpy(np.int64)[order], seg.astype(np.int32), seg_off


def _sums_sorted(ts, seg_off, v, lo, hi, with_count, device):
    """Window sums/counts of rows already sorted by (partition, order key); sorted order out."""
    n, nw = len(ts), len(lo)
    use_gpu = False
    if n:
        import torch

        use_gpu = torch.cuda.is_available() and (device is not None and torch.device(device).type == "cuda"
                                                 or (device is None and n >= GPU_MIN_ROWS))
    if use_gpu:
        import torch

        from ..ops import kernels as K

        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        seg = np.repeat(np.arange(len(seg_off) - 1, dtype=np.int32), np.diff(seg_off))
        r = K.range_window(t(ts), t(seg), t(seg_off), t(v), t(lo), t(hi), want_count=with_count)
        if with_count:
            return r[0].cpu().numpy(), r[1].cpu().numpy()
        return r.cpu().numpy(), None
    P = np.concatenate([[0.0], np.cumsum(v)])
    sums = np.full((n, nw), np.nan)
    cnts = np.zeros((n, nw), np.int64)
    for s in range(len(seg_off) - 1):
        a, b = seg_off[s], seg_off[s + 1]
        tt = ts[a:b]
        for w in range(nw):
            f = a + np.searchsorted(tt, tt + lo[w], side="left")
            e = a + np.searchsorted(tt, tt + hi[w], side="right")
            c = np.maximum(e - f, 0)
            cnts[a:b, w] = c
            sums[a:b, w] = np.where(c > 0, P[np.maximum(e, f)] - P[f], np.nan)
    return sums, cnts


def _world(process_group):
    import torch.distributed as dist

    if process_group is False or not dist.is_available() or not dist.is_initialized():
        return 1, 0
    return dist.get_world_size(process_group), dist.get_rank(process_group)


def range_sums(df: pd.DataFrame, partition_by, order_by: str, value: str, windows, device=None,
               with_count: bool = False, process_group=None):
    """Sums of ``value`` over each ``(lo, hi)`` range of the order key (inclusive, relative to the
    row's own key) within its partition.  Returns a float64 array [len(df), len(windows)] in the
    frame's row order (NaN: empty range), plus int counts with ``with_count``.

    Data-parallel (``torch.distributed`` initialised with world > 1, or an explicit
    ``process_group``; ``False`` turns it off): every rank computes the windows of the partitions it
    owns (partition i -> rank i % world, like a Spark shuffle by the partition keys) on its own
    device, then the per-rank results are all-gathered, so each rank returns the full frame's
    result — the reference runs this ``Window.partitionBy`` aggregation on Spark executors
    (feature_engineering.ipynb:229-249)."""
    windows = [(int(lo), int(hi)) for lo, hi in windows]
    n = len(df)
    order, ts, seg, seg_off = _sorted_layout(df, partition_by, order_by)
    v = pd.to_numeric(df[value], errors="coerce").fillna(0).to_numpy(np.float64)[order]
    lo = np.array([w[0] for w in windows], np.int64)
    hi = np.array([w[1] for w in windows], np.int64)
    world, rank = _world(process_group)
    if world > 1 and n:
        import torch.distributed as dist

        own = (seg % world) == rank  # this rank's partitions (whole partitions, rows contiguous)
        sizes = np.diff(seg_off)
        mine = np.arange(len(sizes)) % world == rank
        sub_off = np.concatenate([[0], np.cumsum(sizes[mine])]).astype(np.int64)
        s_sub, c_sub = _sums_sorted(ts[own], sub_off, v[own], lo, hi, with_count, device)
        parts = [None] * world
        dist.all_gather_object(parts, (order[own], s_sub, c_sub), group=process_group)
        sums = np.empty((n, len(windows)))
        cnts = np.zeros((n, len(windows)), np.int64)
        for idx, s_, c_ in parts:
            sums[idx] = s_
            if with_count:
                cnts[idx] = c_
        return (sums, cnts) if with_count else sums
    sums, cnts = _sums_sorted(ts, seg_off, v, lo, hi, with_count, device)
    out = np.empty_like(sums)
    out[order] = sums
    if not with_count:
        return out
    oc = np.empty_like(cnts)
    oc[order] = cnts
    return out, oc


def with_range_sums(df: pd.DataFrame, specs: dict, partition_by, order_by: str, value: str, device=None,
                    fill=0.0, process_group=None) -> pd.DataFrame:
    """``df`` plus one column per ``{name: (lo, hi)}`` — the reference's chain of ``withColumn(name,
    F.sum(value).over(window))`` followed by ``fillna(fill)``."""
    names = list(specs)
    sums = range_sums(df, partition_by, order_by, value, [specs[k] for k in names], device=device,
                      process_group=process_group)
    out = df.copy()
    for j, k in enumerate(names):
        col = sums[:, j]
        out[k] = np.where(np.isnan(col), fill, col) if fill is not None else col
    return out


# ---- plain group-by: df.groupby(by, sort=True)[values].agg([...]) ----
GROUP_AGGS = ("count", "sum", "mean", "min", "max", "std", "var")
GROUP_MAX_KEYS = 4
# Rows from which group_aggregates takes the device route on its own (None: only with device="cuda"): the smallest
# measured size at which the device route won five of five alternating pairs against pandas at BOTH group counts
# (tools/groupagg_bench.py on one MI355X, V = 4, upload included; profiles/r27_groupagg.txt):
#   rows         groups    device      pandas     pairs won
#   100,000          50      2.5 ms      4.7 ms   5 of 5
#   100,000      63,106      5.1 ms     12.3 ms   5 of 5
#   1,000,000        50     11.2 ms     33.2 ms   5 of 5
#   1,000,000    99,995     15.9 ms     75.8 ms   5 of 5
#   10,000,000       50     94.3 ms    309.5 ms   5 of 5
#   10,000,000  100,000     98.7 ms    576.5 ms   5 of 5
# Nothing below 100,000 rows has been measured.
GROUP_GPU_MIN_ROWS = 100_000


def group_aggregates(df: pd.DataFrame, by, values, aggs=("count", "sum", "mean", "min", "max"), device=None):
    """``(df.groupby(by, sort=True)[values].agg(list(aggs)), route)``: the frame pandas returns (the key columns first,
    as its index; one column per value and aggregate; a row with a missing key belongs to no group, a missing value is
    skipped) and the route that computed it, 'gpu' (``groupagg.hip``: the keys' dense ranks, one sort of 64-bit group
    keys, a segmented fixed-order reduction) or 'cpu' (that pandas line).  ``by`` / ``values``: a name or a list of
    names.  The reference's ``groupBy().sum()`` / ``count()`` / ``avg()`` (ComputeFeatures.scala:148-160) and
    ``sales.groupby("store")`` (feature_engineering.py).

    The device route is taken with a GPU and ``device="cuda"``, or on its own from ``GROUP_GPU_MIN_ROWS`` rows.  It
    declines, and pandas runs, for: a key or value column that is not numeric, is bool, or holds integers beyond 2^53
    (an integer value column also when rows x max |v| could pass 2^53, where pandas' int64 sum is exact and fp64 is
    not); more than 4 key columns; an aggregate outside ``GROUP_AGGS``; key columns whose class counts multiply to
    2^32 - 1 or more; no group at all.  Integer value columns come back in pandas' dtypes."""
    by = [by] if isinstance(by, str) else list(by)
    values = [values] if isinstance(values, str) else list(values)
    aggs = list(aggs)

    def host():
        return df.groupby(by, sort=True)[values].agg(aggs), "cpu"

    use_gpu = False
    if len(df) and by and values and len(by) <= GROUP_MAX_KEYS and all(a in GROUP_AGGS for a in aggs):
        import torch

        use_gpu = torch.cuda.is_available() and (
            (device is not None and torch.device(device).type == "cuda")
            or (device is None and GROUP_GPU_MIN_ROWS is not None and len(df) >= GROUP_GPU_MIN_ROWS))
    if not use_gpu:
        return host()
    from .rules import order_eligible

    if not all(order_eligible(df[c]) for c in dict.fromkeys(by + values)):
        return host()
    ints = [c for c in values if pd.api.types.is_integer_dtype(df[c].dtype)]
    if any(max(abs(int(df[c].min())), abs(int(df[c].max()))) * len(df) >= 1 << 53 for c in ints):
        return host()
    import torch

    from ..ops import kernels as K

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    x = np.stack([pd.to_numeric(df[c], errors="coerce").to_numpy(np.float64, na_value=np.nan) for c in by + values], 1)
    xt = torch.from_numpy(np.ascontiguousarray(x)).pin_memory().to(dev, non_blocking=True)
    nk = len(by)
    try:
        r = K.group_by64(xt, range(nk), range(nk, nk + len(values)), want_var="std" in aggs or "var" in aggs)
    except K.GroupKeyRange:
        return host()
    if not r["G"]:
        return host()
    first = r["first_row"].cpu().numpy()
    got = {a: r[a].cpu().numpy() for a in ("count", "sum", "mean", "min", "max", "var") if a in r}
    if "var" in got:
        got["std"] = np.sqrt(got["var"])
    keys = [df[k].to_numpy()[first] for k in by]
    index = pd.Index(keys[0], name=by[0]) if nk == 1 else pd.MultiIndex.from_arrays(keys, names=by)
    data = {}
    for j, v in enumerate(values):
        for a in aggs:
            col = got[a][:, j]
            data[(v, a)] = col.astype(df[v].dtype) if v in ints and a in ("sum", "min", "max") else col
    return pd.DataFrame(data, index=index), "gpu"
