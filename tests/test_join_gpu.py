"""join.hip on the device (``kernels.join_pairs64`` / ``join_gather64``) against ``functional.join_reference`` and
numpy ``take``: integers and copied bits, so everything is exactly equal, order included.  Sizes 1, T - 1, T + 1 and
2T + 1 around the tile; the special shapes sit on the skew the balanced expand exists for, on the chunked LDS table
(more than L left rows under one output tile) and on n_out = T - 1, T, T + 1."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from hops_examples_amd.featurestore import join as J
from hops_examples_amd.ops import functional as HF

pytestmark = pytest.mark.gpu

T, L = 1024, 1024  # collection runs without the extension; test_constants pins them
SIZES = [(1, 1), (1, 2 * T + 1), (T - 1, T + 1), (T + 1, T - 1), (2 * T + 1, 1), (2 * T + 1, 2 * T + 1)]
LAYOUTS = ["one", "unique", "disjoint", "nan", "pair"]
SPECIAL = [("one", 1, 3 * T + 5), ("one", 3 * T + 5, 1), ("sparse", 3 * L + 7, 700), ("fan", 1, T - 1), ("fan", 1, T),
           ("fan", 1, T + 1)]
HOWS = ["inner", "left", "full"]


@functools.lru_cache(maxsize=None)
def _case(layout, nl, nr):
    """(xl, xr, key columns): the keys in front, a payload column behind; computed once, never modified."""
    rng = np.random.default_rng(nl * 7 + nr)
    il, ir = np.arange(nl, dtype=np.float64), np.arange(nr, dtype=np.float64)
    if layout == "one":  # a cross product: many output tiles from few rows
        kl, kr = il[:, None] * 0 + 5, ir[:, None] * 0 + 5
    elif layout == "unique":  # one to one where both sides have the key, rows permuted
        kl, kr = rng.permutation(il)[:, None], rng.permutation(ir)[:, None]
    elif layout == "disjoint":
        kl, kr = il[:, None], -1 - ir[:, None]
    elif layout == "nan":  # a few keys, NaN on both sides, -0.0 against +0.0
        kl, kr = rng.integers(0, 6, (nl, 1)) * 0.5, rng.integers(0, 8, (nr, 1)) * -0.5 + 1.5
        kl[rng.random(nl) < 0.2], kr[rng.random(nr) < 0.2] = np.nan, np.nan
        kl[kl == 0], kr[kr == 0] = -0.0, 0.0
    elif layout == "pair":  # two key columns, only the pair tells rows apart
        kl, kr = rng.integers(0, 4, (nl, 2)).astype(np.float64), rng.integers(0, 4, (nr, 2)).astype(np.float64)
        kr[rng.random(nr) < 0.1, 1] = np.nan
    elif layout == "sparse":  # every fifth left row has one match, the last right rows none: > L rows under one tile
        kl, kr = il[:, None], np.where(ir < 600, ir * 5, -1 - ir)[:, None]
    elif layout == "fan":  # one left row against nr matching right rows and three that do not: n_out = nr
        kl, kr = il[:, None] * 0 + 2, np.concatenate([ir * 0 + 2, [7.0, np.nan, 8.0]])[:, None]
    pay = lambda k: np.ascontiguousarray(np.concatenate([k, rng.normal(size=(len(k), 1))], 1))  # noqa: E731
    return pay(kl), pay(kr), list(range(kl.shape[1]))


@functools.lru_cache(maxsize=None)
def _ref(layout, nl, nr, how):
    xl, xr, kc = _case(layout, nl, nr)
    return HF.join_reference(xl, xr, kc, kc, how)


def _check(layout, nl, nr, how, **kw):
    from hops_examples_amd.ops import kernels as K

    xl, xr, kc = _case(layout, nl, nr)
    li, ri = _ref(layout, nl, nr, how)
    r = K.join_pairs64(torch.from_numpy(xl).cuda(), torch.from_numpy(xr).cuda(), kc, kc, how=how, **kw)
    tag = f"{layout} {nl}x{nr} {how} {kw}"
    assert r["n_out"] == len(li) and r["li"].dtype == r["ri"].dtype == torch.int32, tag
    np.testing.assert_array_equal(r["li"].cpu().numpy(), li, err_msg=tag)
    np.testing.assert_array_equal(r["ri"].cpu().numpy(), ri, err_msg=tag)
    fl, fr = _ref(layout, nl, nr, "full")
    both = (fl >= 0) & (fr >= 0)
    assert (r["matched_left"], r["matched_right"]) == (len(set(fl[both].tolist())), len(set(fr[both].tolist()))), tag
    return r


def test_constants():
    from hops_examples_amd.ops import kernels as K

    assert (K.join_tile(), K.join_table_rows()) == (T, L)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("nl,nr", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(layout, nl, nr, how):
    _check(layout, nl, nr, how)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("layout,nl,nr", SPECIAL)
def test_skew_chunked_table_and_tile_edges(layout, nl, nr, how):
    if layout == "fan":
        assert len(_ref(layout, nl, nr, "inner")[0]) == nr  # n_out = T - 1, T, T + 1
    _check(layout, nl, nr, how)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("layout,nl,nr", [("nan", 2 * T + 1, 2 * T + 1), ("sparse", 3 * L + 7, 700)])
def test_grid_and_workspace_invariance(layout, nl, nr, how):
    for kw in ({"max_workgroups": 1}, {"max_workgroups": 3}, {"ws_cap_bytes": 1 << 16}):
        _check(layout, nl, nr, how, **kw)


@pytest.mark.parametrize("cl,cr", [([1], []), ([], [0]), ([2, 0, 1], [3, 3, 0, 1])])
def test_gather(cl, cr):
    from hops_examples_amd.ops import kernels as K

    rng = np.random.default_rng(11)
    xl, xr, n = rng.normal(size=(37, 3)), rng.normal(size=(5, 4)), 2 * 256 + 3
    xl[3, 1], xr[2, 0] = np.uint64(0x7FF8DEAD0000BEEF).view(np.float64), np.nan  # a payload that must come through
    li, ri = rng.integers(-1, 37, n).astype(np.int32), rng.integers(-1, 5, n).astype(np.int32)
    li[:4], ri[:4] = [3, 3, -1, 36], [2, -1, 2, 4]
    got = K.join_gather64(*(torch.from_numpy(a).cuda() for a in (xl, xr, li, ri)), cl, cr).cpu().numpy()
    want = np.concatenate([np.where((li >= 0)[:, None], xl[li][:, cl], np.nan),
                           np.where((ri >= 0)[:, None], xr[ri][:, cr], np.nan)], 1)
    assert got.shape == (n, len(cl) + len(cr))
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def test_refusals():
    from hops_examples_amd.ops import kernels as K

    x = torch.zeros(1 << 16, 2, dtype=torch.float64).cuda()
    for xl, xr, lk, rk in ((x[:8], x[:8], [0, 1], [0]), (x[:8].float(), x[:8], [0], [0]), (x[:8].cpu(), x[:8], [0], [0]),
                           (x[:8], x[:8].t(), [0], [0]), (x[:8], x[:8], [2], [0]), (x[:8], x[:8], [], [])):
        with pytest.raises(ValueError):
            K.join_pairs64(xl, xr, lk, rk)
    with pytest.raises(ValueError):
        K.join_pairs64(x[:8], x[:8], [0], [0], how="cross")
    with pytest.raises(K.JoinTooLarge):  # 2^16 x 2^16 rows of one key: 2^32 pairs, refused before the expand
        K.join_pairs64(x, x, [0], [0])
    r = K.join_pairs64(x[:0], x[:3], [0], [0], how="full")  # an empty side: no launch
    assert r["li"].tolist() == [-1, -1, -1] and r["ri"].tolist() == [0, 1, 2] and r["n_out"] == 3


def _frames():
    rng = np.random.default_rng(2)
    n, m = T + 1, 300
    left = pd.DataFrame({"k": rng.integers(0, 400, n), "x": rng.normal(size=n), "s": [f"s{i % 17}" for i in range(n)],
                         "t": pd.to_datetime("2021-03-01") + pd.to_timedelta(rng.integers(0, 90, n), "D")})
    right = pd.DataFrame({"k": rng.integers(200, 500, m).astype(np.float64), "n": rng.integers(-5, 5, m),
                          "name": [f"r{i}" for i in range(m)], "y": rng.normal(size=m).astype(np.float32)})
    right.loc[::9, "k"] = np.nan
    return left, right


@pytest.mark.parametrize("how", J.JOIN_KINDS)
def test_equi_join_is_the_host_route(how):
    left, right = _frames()
    got, route = J.equi_join(left, right, "k", how=how, device="cuda")
    want, host = J.equi_join(left, right, "k", how=how)
    assert (route, host) == ("gpu", "cpu") and len(got) > 0
    pd.testing.assert_frame_equal(got, want)


def test_query_read(project_root):
    import hops_examples_amd.featurestore as hsfs

    fs = hsfs.connection().get_feature_store()
    left, right = _frames()
    a = fs.create_feature_group("a", 1, primary_key=["k"])
    a.save(left)
    b = fs.create_feature_group("b", 1, primary_key=["k"])
    b.save(right.dropna().astype({"k": np.int64}))
    c = fs.create_feature_group("c", 1, primary_key=["s"])
    c.save(pd.DataFrame({"s": ["s1", "s2"], "k2": [1, 2], "w": [0.5, 1.5]}))
    d = fs.create_feature_group("d", 1, primary_key=["k2"])
    d.save(pd.DataFrame({"k2": np.arange(350, 450), "z": np.arange(100) * 0.25, "u": np.arange(100)}))
    q = a.select_all().join(b.select_all(), join_type="left").join(d.select_all(), left_on=["k"], right_on=["k2"])
    got = q.read(read_options={"join_device": "cuda"})
    assert q.last_read_route == "gpu"
    want = q.read()
    assert q.last_read_route.startswith("sql") and list(got.columns) == list(want.columns)
    by = list(want.columns)
    pd.testing.assert_frame_equal(got.sort_values(by, kind="stable").reset_index(drop=True),
                                  want.sort_values(by, kind="stable").reset_index(drop=True))
    for declined in (a.select_all().join(b.select_all()).filter(a.x > 0.0), a.select_all().join(c.select_all(), on=["s"])):
        declined.read(read_options={"join_device": "cuda"})
        assert declined.last_read_route.startswith("sql")
