"""Equi-joins of feature frames: ``a JOIN b ON a.k = b.k`` (inner, left, right, full), what ``Query.read`` hands to SQL
for ``sales_fg.select_all().join(store_fg.select_all())`` and every training dataset built from such a query.

``equi_join`` returns the joined frame and the route that found the row pairs: 'gpu' (``join.hip``: the key columns of
both sides stacked, ranked and sorted as 64-bit keys, then spans, offsets and a balanced expand; the numeric columns
are gathered on the device too) or 'cpu' (``pandas.merge`` on the key columns).  SQL semantics on both: a missing key
matches nothing.  Row order on both: left row order, within a left row right row order, then (full) the unmatched right
rows in row order; ``how="right"`` is the left join with the sides swapped, so its rows are in right row order.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

JOIN_KINDS = ("inner", "left", "right", "full")
# Rows, summed over the joined frames, from which ``Query.read`` takes the device route on its own (None: only with
# ``read_options={"join_device": "cuda"}``): the smallest measured size at which the device route won five of five
# alternating pairs against the sqlite route of the same build (tools/join_bench.py on one MI355X, one ``Query.read`` of
# sales x stores (45 rows) x exogenous (6,435 rows), the frames' read, uploads and downloads included;
# profiles/r28_join.txt):
#   sales rows    device      sqlite    pairs won    pandas.merge x 2 of the same frames
#   10,000        12.6 ms     45.0 ms   5 of 5         1.3 ms
#   100,000       25.4 ms    279.8 ms   5 of 5         4.0 ms
#   1,000,000    189.8 ms  2,684.8 ms   5 of 5        43.4 ms
# Nothing below 10,000 + 6,480 rows has been measured.  ``equi_join`` itself has ``pandas.merge`` as its host route, not
# sqlite, and nothing shows the device ahead of that (last column; the device figure is mostly host-side frame work,
# the kernels take under 1 ms at 10^6 rows): its device route stays opt-in (``device="cuda"``).
JOIN_GPU_MIN_ROWS = 16_480


def _want_gpu(device, rows, min_rows=None) -> bool:
    import torch

    return torch.cuda.is_available() and (
        (device is not None and torch.device(device).type == "cuda")
        or (device is None and min_rows is not None and rows >= min_rows))


def _f64(df, cols):
    if not cols:
        return np.zeros((len(df), 0))
    return np.ascontiguousarray(
        np.stack([pd.to_numeric(df[c], errors="coerce").to_numpy(np.float64, na_value=np.nan) for c in cols], 1))


def _host_pairs(left, right, left_on, right_on, how):
    """``(li, ri)`` from pandas.merge over the key columns, the rows with a missing key taken out of the match."""
    names = [f"k{i}" for i in range(len(left_on))]
    lk = left[left_on].reset_index(drop=True).set_axis(names, axis=1).assign(_li=np.arange(len(left))).dropna(subset=names)
    rk = right[right_on].reset_index(drop=True).set_axis(names, axis=1).assign(_ri=np.arange(len(right))).dropna(subset=names)
    m = lk.merge(rk, on=names, how="inner", sort=False)
    li, ri = m["_li"].to_numpy(np.int64), m["_ri"].to_numpy(np.int64)
    if how != "inner":
        rest = np.setdiff1d(np.arange(len(left)), li)
        li, ri = np.concatenate([li, rest]), np.concatenate([ri, np.full(len(rest), -1)])
    o = np.lexsort((ri, li))
    li, ri = li[o], ri[o]
    if how == "full":
        rest = np.setdiff1d(np.arange(len(right)), ri)
        li, ri = np.concatenate([li, np.full(len(rest), -1)]), np.concatenate([ri, rest])
    return li.astype(np.int64), ri.astype(np.int64)


def _take(s: pd.Series, idx):
    """The rows ``idx`` of a column, -1 a missing value (an integer column then becomes float64)."""
    return s.reset_index(drop=True).reindex(idx).reset_index(drop=True)


def equi_join(left: pd.DataFrame, right: pd.DataFrame, left_on, right_on=None, how="inner", device=None):
    """``(frame, route)``: the rows of ``left JOIN right ON left[left_on] = right[right_on]`` (``right_on`` None: the
    same names), the left frame's columns followed by the right frame's; a right key column that has its partner's
    name is left out (on a full join the key column is then missing for an unmatched right row, as SQL's ``a.k`` is).
    Any other column name on both sides is a ValueError.  ``how``: inner, left, right or full.

    The device route is taken with a GPU and ``device="cuda"`` only (see ``JOIN_GPU_MIN_ROWS``).  It declines, and the
    host route runs, for: a key column that ``rules.order_eligible`` rejects (strings, bool, integers beyond 2^53) or
    more than 4 of them; key columns whose class counts multiply to
    2^32 - 1 or more; 2^31 or more result rows; a kind outside ``JOIN_KINDS`` ('outer' is the host's name for full).
    On it the numeric columns that pass ``order_eligible`` are gathered on the device, every other column (strings,
    datetimes, large integers) on the host; an integer column without a missing row keeps its dtype on both routes."""
    from .rules import order_eligible

    left_on = [left_on] if isinstance(left_on, str) else list(left_on)
    right_on = left_on if right_on is None else ([right_on] if isinstance(right_on, str) else list(right_on))
    if not left_on or len(left_on) != len(right_on):
        raise ValueError(f"equi_join: {len(left_on)} left keys against {len(right_on)} right keys")
    gpu_kind = how in JOIN_KINDS
    how = "full" if how == "outer" else how
    if how not in JOIN_KINDS:
        raise ValueError(f"equi_join: how must be one of {JOIN_KINDS}, got {how!r}")
    dropped = {b for a, b in zip(left_on, right_on) if a == b}
    rcols = [c for c in right.columns if c not in dropped]
    if set(left.columns) & set(rcols):
        raise ValueError(f"equi_join: columns on both sides: {sorted(set(left.columns) & set(rcols))}")

    a, b, a_on, b_on, kind = (right, left, right_on, left_on, "left") if how == "right" else \
        (left, right, left_on, right_on, how)  # a: the side whose row order the result has
    pairs, got = None, None
    use_gpu = gpu_kind and len(left_on) <= 4 and _want_gpu(device, len(left) + len(right)) \
        and all(order_eligible(left[c]) for c in left_on) and all(order_eligible(right[c]) for c in right_on)
    if use_gpu:
        import torch

        from ..ops import kernels as K

        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        na = [c for c in dict.fromkeys(a.columns) if order_eligible(a[c])]
        nb = [c for c in dict.fromkeys(b.columns) if order_eligible(b[c])]
        up = lambda m: torch.from_numpy(m).pin_memory().to(dev, non_blocking=True)  # noqa: E731
        xa, xb = up(_f64(a, na)), up(_f64(b, nb))
        try:
            r = K.join_pairs64(xa, xb, [na.index(c) for c in a_on], [nb.index(c) for c in b_on], how=kind)
        except (K.GroupKeyRange, K.JoinTooLarge):
            r = None
        if r is not None:
            ga = [i for i, c in enumerate(na) if a is left or c not in dropped]
            gb = [i for i, c in enumerate(nb) if b is left or c not in dropped]
            vals = K.join_gather64(xa, xb, r["li"], r["ri"], ga, gb).cpu().numpy()
            pairs = (r["li"].cpu().numpy().astype(np.int64), r["ri"].cpu().numpy().astype(np.int64))
            got = {(id(a), na[i]): vals[:, j] for j, i in enumerate(ga)}
            got.update({(id(b), nb[i]): vals[:, len(ga) + j] for j, i in enumerate(gb)})
    if pairs is None:
        pairs = _host_pairs(a, b, a_on, b_on, kind)
    idx = {id(a): pairs[0], id(b): pairs[1]}
    data = {}
    for df, cols in ((left, list(left.columns)), (right, rcols)):
        whole = not (idx[id(df)] < 0).any()
        for c in cols:
            dt = df[c].dtype
            v = got.get((id(df), c)) if got is not None and isinstance(dt, np.dtype) else None
            if v is None:
                data[c] = _take(df[c], idx[id(df)])
            else:  # fp64 from the device: back to the column's dtype (an integer column with a missing row stays float64)
                keep = dt != np.float64 and (whole or pd.api.types.is_float_dtype(dt))
                data[c] = pd.Series(v.astype(dt) if keep else v)
    return pd.DataFrame(data, columns=list(left.columns) + rcols), ("gpu" if got is not None else "cpu")


# ---------------------------------------------------------------------------------- Query.read
_SQL_KINDS = {"INNER": "inner", "LEFT": "left", "RIGHT": "right", "FULL": "full"}


def query_plan(query, frames):
    """What ``read_query`` needs, or the reason (a str) the query stays on the sqlite line: every join INNER, LEFT,
    RIGHT or FULL on ``on`` / ``left_on`` + ``right_on`` with keys that pass ``rules.order_eligible`` on both sides, no
    filter, no feature with a ``default_value``, no bool column, and no selected column name in two feature groups
    other than as a dropped join key.  The plan: (left frame, left names, [(right frame, right names, left_on,
    right_on, kind)])."""
    from .rules import order_eligible

    if not query._joins:
        return "no join"
    if query._filter is not None or any(j.query._filter is not None for j in query._joins):
        return "a filter"
    ldf = frames[query._left_fg._table]
    lnames = [f.name for f in query._left_features]
    names, feats, joins = list(lnames), list(query._left_features), []
    for j in query._joins:
        if j.join_type not in _SQL_KINDS:
            return f"a {j.join_type} join"
        lo, ro = (list(j.on), list(j.on)) if j.on else (list(j.left_on), list(j.right_on))
        if not lo or len(lo) != len(ro) or len(lo) > 4:
            return "join keys"
        rdf = frames[j.query._left_fg._table]
        if any(k not in ldf.columns for k in lo) or any(k not in rdf.columns for k in ro):
            return "a key column that is not stored"
        if not all(order_eligible(ldf[k]) for k in lo) or not all(order_eligible(rdf[k]) for k in ro):
            return "an ineligible key"
        drop = set(j.on) | set(j.right_on)
        rn = [f.name for f in j.query._left_features if f.name not in drop]
        if any(n not in rdf.columns for n in rn) or any(rdf[n].dtype == bool for n in rn + ro):
            return "a bool or missing column"
        names += rn
        feats += [f for f in j.query._left_features if f.name not in drop]
        joins.append((rdf, rn, lo, ro, _SQL_KINDS[j.join_type]))
    if any(n not in ldf.columns for n in lnames) or any(ldf[n].dtype == bool for n in lnames):
        return "a bool or missing column"
    if len(set(names)) != len(names):
        return "a column name in two feature groups"
    if any(f.default_value is not None for f in feats):
        return "a default value"
    return ldf, lnames, joins


def _sql_frame(df):
    """The columns as the sqlite line stores them: datetimes as text."""
    d = {}
    for c in df.columns:
        d[c] = df[c].astype(str) if str(df[c].dtype).startswith("datetime") else df[c]
    return pd.DataFrame(d).reset_index(drop=True)


def read_query(query, frames, device=None):
    """``(frame, route)`` of a joined query without sqlite, or ``(None, reason)``: the joins applied in order against the
    frame built so far (every ON names the left feature group's columns), the columns those of ``to_string()``'s SELECT
    in that order, the dtypes those of the sqlite line (datetimes as str, integers int64, an integer column that gained
    nulls float64, a column without any value object).  Row order: ``equi_join``'s."""
    plan = query_plan(query, frames)
    if isinstance(plan, str):
        return None, plan
    ldf, lnames, joins = plan
    if not _want_gpu(device, len(ldf) + sum(len(j[0]) for j in joins), JOIN_GPU_MIN_ROWS):
        return None, "no device route wanted"
    lkeys = list(dict.fromkeys(k for j in joins for k in j[2]))
    cur = _sql_frame(pd.DataFrame({**{n: ldf[n] for n in lnames}, **{f"__l.{k}": ldf[k] for k in lkeys}}))
    for rdf, rn, lo, ro, kind in joins:
        rk = [f"__r.{i}" for i in range(len(ro))]
        side = _sql_frame(pd.DataFrame({**{k: rdf[c] for k, c in zip(rk, ro)}, **{n: rdf[n] for n in rn}}))
        cur, route = equi_join(cur, side, [f"__l.{k}" for k in lo], rk, how=kind, device=device or "cuda")
        if route != "gpu":
            return None, "equi_join declined"
        cur = cur.drop(columns=rk)
    out = cur.drop(columns=[f"__l.{k}" for k in lkeys])
    for c in out.columns:
        dt = out[c].dtype
        if not len(out) or out[c].isna().all():
            out[c] = pd.Series([None] * len(out), dtype=object)
        elif pd.api.types.is_integer_dtype(dt):
            out[c] = out[c].astype(np.int64)
        elif pd.api.types.is_float_dtype(dt):
            out[c] = out[c].astype(np.float64)
        elif dt == object:
            out[c] = out[c].where(out[c].notna(), None)
    return out, "gpu"
