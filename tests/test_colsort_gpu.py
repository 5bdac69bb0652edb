"""colsort.hip on the device against the host references of ``ops.functional``.

Per case: ``column_key_decode(order.keys)`` is BIT-equal to ``column_sort_reference``; count / distinct / unique are
equal as integers; the entropy satisfies |H - H_ref| <= (D + 8) * 2^-52 * max(1, ln count) with D the distinct count and
H_ref summed by ``math.fsum`` (D terms, each product and log good to about 2 ulp, summed in any order: at least twice the
worst case of ln(n) - S/n and of -sum p ln p); on the finite families both order statistics of every quantile are
bit-equal to ``np.sort(valid)[lo]`` / ``[hi]`` and the quantile to ``np.nanquantile`` (valid = the non-NaN values with
-0.0 as +0.0, the key rule's canonical form); and ``x`` is bit-unchanged.

Rows, with T the sort's tile: 1, 2, 63, 64, 65, T-1, T, T+1, 3T+5 at 1 and 3 columns; 65 columns at T+1 rows (more
columns than a wave has lanes); one column of 1,025 tiles (the tile-offset scan walks any tile count in chunks of 64,
so it has no one-workgroup limit).
"""
import functools
import math

import numpy as np
import pytest
import torch

from hops_examples_amd.ops import functional as HF

pytestmark = pytest.mark.gpu

QS = [0.0, 0.25, 0.5, 0.75, 0.999, 1.0]
NAN_BITS = 0x7FF8000000000000


def _tile():
    from hops_examples_amd.ops import kernels as K

    return K.column_sort_tile()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(fam, rows, cols):
    """(x, sorted reference, counts, entropy) computed once per case and shared; never modified."""
    x = HF.column_order_family(fam, rows, cols, seed=rows + cols, tile=_tile())
    counts, ent = HF.column_runs_reference(x)
    return x, HF.column_sort_reference(x), counts, ent


def _check(fam, rows, cols, **kw):
    from hops_examples_amd.ops import kernels as K

    x, ref_sorted, ref_counts, ref_ent = _case(fam, rows, cols)
    xd = torch.from_numpy(x).cuda()
    order = K.column_sort64(xd, **kw)
    counts, ent = K.column_runs64(order)
    tag = f"{fam} {rows}x{cols} {kw}"
    assert order.keys.shape == (cols, rows) and order.keys.dtype == torch.int64
    got = HF.column_key_decode(order.keys)
    assert np.array_equal(_bits(got), _bits(ref_sorted)), tag
    assert order.count.cpu().tolist() == ref_counts[:, 0].tolist(), tag
    assert counts.cpu().numpy().tolist() == ref_counts.tolist(), tag
    ent = ent.cpu().numpy()
    for c in range(cols):
        n, d = int(ref_counts[c, 0]), int(ref_counts[c, 1])
        bound = (d + 8) * 2.0 ** -52 * max(1.0, math.log(max(n, 1)))
        err = abs(float(ent[c]) - float(ref_ent[c]))
        if err > bound / 4:
            print(f"colsort-entropy {tag} col {c}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (tag, c, ent[c], ref_ent[c], bound)
    if fam in HF.COLUMN_ORDER_FINITE:
        n = ref_counts[:, 0]
        vi = np.array(QS)[None, :] * (n[:, None] - 1)
        lo = np.floor(vi).astype(np.int64)
        hi = np.minimum(lo + 1, n[:, None] - 1)
        v = K.column_order_values64(order, torch.from_numpy(np.concatenate([lo, hi], 1)).cuda()).cpu().numpy()
        q = K.column_quantiles64(order, QS)
        for c in range(cols):
            valid = np.sort(x[:, c] + 0.0)
            assert np.array_equal(_bits(v[c]), _bits(np.concatenate([valid[lo[c]], valid[hi[c]]]))), tag
            assert np.array_equal(_bits(q[c]), _bits(np.nanquantile(x[:, c] + 0.0, QS))), tag
    if fam == "digits":
        assert all(len(p) < 8 for p in order.passes), (tag, order.passes)  # small integers: the low digits are skipped
    if fam == "allnan":
        assert np.isnan(K.column_quantiles64(order, QS)).all() and (ent == 0.0).all()
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)), tag  # x is only read
    return order, counts, ent


def _shapes():
    T = 2048  # collection runs without the extension; test_tile_is_the_documented_one pins it
    return [(r, c) for r in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5) for c in (1, 3)]


def test_tile_is_the_documented_one():
    assert _tile() == 2048


@pytest.mark.parametrize("rows,cols", _shapes())
def test_families(rows, cols):
    for fam in HF.COLUMN_ORDER_FAMILIES:
        _check(fam, rows, cols)


@pytest.mark.parametrize("fam", ["bits", "digits", "onenan"])
def test_more_columns_than_lanes(fam):
    _check(fam, _tile() + 1, 65)


@pytest.mark.parametrize("fam", ["bits", "digits", "tworuns"])
def test_many_tiles(fam):
    _check(fam, 1025 * _tile() - 7, 1)


@pytest.mark.parametrize("fam", ["bits", "digits", "tworuns", "onenan"])
def test_grid_and_grouping_invariance(fam):
    from hops_examples_amd.ops import kernels as K

    rows, cols = 3 * _tile() + 5, 3
    base = _check(fam, rows, cols)
    assert len(base[0].passes) == 1
    assert K.column_sort_ws_words(rows, cols, 1) < K.column_sort_ws_words(rows, cols)
    for kw in ({"max_workgroups": 1}, {"max_workgroups": 3}, {"ws_cap_bytes": 1},
               {"max_workgroups": 1, "ws_cap_bytes": 1}, {"max_workgroups": 3, "ws_cap_bytes": 1}):
        got = _check(fam, rows, cols, **kw)
        if "ws_cap_bytes" in kw:
            assert len(got[0].passes) == cols  # one column per group
        assert torch.equal(got[0].keys, base[0].keys) and torch.equal(got[0].count, base[0].count), kw
        assert torch.equal(got[1], base[1]), kw
        assert np.array_equal(_bits(got[2]), _bits(base[2])), kw


@pytest.mark.parametrize("rows,cols,cap", [(3 * 2048 + 5, 3, 0), (2049, 5, 1), (64, 2, 0)])
def test_workspace_bounds(rows, cols, cap):
    from hops_examples_amd.ops import kernels as K

    need = K.column_sort_ws_words(rows, cols, cap)
    pattern = 0x5A5A5A5A5A5A5A5A
    buf = torch.full((need + 128,), pattern, dtype=torch.int64, device="cuda")
    x, ref_sorted, _, _ = _case("bits", rows, cols)
    order = K.column_sort64(torch.from_numpy(x).cuda(), ws=buf[64:64 + need], ws_cap_bytes=cap)
    assert np.array_equal(_bits(HF.column_key_decode(order.keys)), _bits(ref_sorted))
    assert (buf[:64] == pattern).all() and (buf[64 + need:] == pattern).all()


def test_refusals_and_empty():
    from hops_examples_amd.ops import kernels as K

    x = torch.from_numpy(HF.column_order_family("bits", 100, 4)).cuda()
    need = K.column_sort_ws_words(100, 4)
    ws = torch.full((need,), 7, dtype=torch.int64, device="cuda")
    for bad, kw in ((x.float(), {}), (x.t(), {}), (x.cpu(), {}), (x.reshape(10, 10, 4), {}), (x, {"ws": ws[:need - 1]}),
                    (x, {"ws": ws.int()}), (x, {"max_workgroups": -1})):
        with pytest.raises(ValueError):
            K.column_sort64(bad, **kw)
    assert (ws == 7).all()
    order = K.column_sort64(x, ws=ws)  # the stated size is enough
    assert np.array_equal(_bits(HF.column_key_decode(order.keys)), _bits(HF.column_sort_reference(x)))
    with pytest.raises(ValueError):
        K.column_order_values64(order, torch.zeros(4, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        K.column_order_values64(order, torch.zeros(3, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        K.column_quantiles64(order, [1.5])
    for shape in ((0, 3), (5, 0)):
        o = K.column_sort64(torch.empty(shape, dtype=torch.float64, device="cuda"))
        counts, ent = K.column_runs64(o)
        assert o.keys.shape == (shape[1], shape[0]) and o.count.tolist() == [0] * shape[1] and o.passes == []
        assert counts.tolist() == [[0, 0, 0]] * shape[1] and ent.tolist() == [0.0] * shape[1]
        assert K.column_quantiles64(o, [0.5]).shape == (shape[1], 1)
        assert K.column_sort_ws_words(*shape) == 0
