"""The host statements of colsort.hip (``column_key_reference`` / ``column_key_decode`` / ``column_sort_reference`` /
``column_runs_reference`` / ``column_quantile_reference``) against pandas and numpy, the quantile index rule of
``column_quantiles64``, and the order rules' cache wiring in ``featurestore.rules`` — all without a GPU.

Entropy bound (the one the GPU tests use): |H - H_ref| <= (D + 8) * 2^-52 * max(1, ln count), D the distinct count.
"""
import math
import warnings

import numpy as np
import pandas as pd
import pytest

from hops_examples_amd.ops import functional as HF

ROWS = [1, 2, 63, 65, 300, 2051]
QS = [0.0, 0.25, 0.5, 0.75, 0.999, 1.0]


def _entropy_bound(distinct, count):
    return (distinct + 8) * 2.0 ** -52 * max(1.0, math.log(max(count, 1)))


def _cases():
    for fam in HF.COLUMN_ORDER_FAMILIES:
        for rows in ROWS:
            yield fam, rows


@pytest.mark.parametrize("fam,rows", list(_cases()))
def test_references_against_pandas(fam, rows):
    from hops_examples_amd.featurestore import rules

    x = HF.column_order_family(fam, rows, 2, seed=rows, tile=256)
    counts, ent = HF.column_runs_reference(x)
    srt = HF.column_sort_reference(x)
    assert srt.shape == (2, rows)
    for c in range(2):
        s = pd.Series(x[:, c])
        vc = s.value_counts(dropna=True)
        assert counts[c].tolist() == [int(s.notna().sum()), int(s.nunique(dropna=True)), int((vc == 1).sum())]
        assert abs(ent[c] - rules._entropy(s)) <= _entropy_bound(counts[c, 1], counts[c, 0])
        n = int(counts[c, 0])
        valid = np.sort(x[~np.isnan(x[:, c]), c] + 0.0)
        assert srt[c, :n].view(np.uint64).tolist() == valid.view(np.uint64).tolist()
        assert (srt[c, n:].view(np.uint64) == np.uint64(0x7FF8000000000000)).all()
    if fam in HF.COLUMN_ORDER_FINITE:
        q = HF.column_quantile_reference(x, QS)
        for c in range(2):
            assert q[c].view(np.uint64).tolist() == np.nanquantile(x[:, c], QS).view(np.uint64).tolist()
    if fam == "allnan":
        assert np.isnan(HF.column_quantile_reference(x, QS)).all() and (ent == 0.0).all()


def test_key_rule():
    vals = np.array([-np.inf, -1e300, -2.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 1e300, np.inf])
    k = HF.column_key_reference(vals)
    assert k.dtype == np.uint64
    assert k[4] == k[5]  # -0.0 and +0.0: one key
    strict = np.delete(k, 4)
    assert (strict[1:] > strict[:-1]).all()  # a < b  =>  key(a) < key(b)
    assert k[-1] == np.uint64(0xFFF0000000000000)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                     0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001], np.uint64).view(np.float64)
    kn = HF.column_key_reference(nans)
    assert (kn == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (kn > k[-1]).all()
    # monotone on random bit patterns too
    x = HF.column_order_family("bits", 4000, 1, seed=3)[:, 0]
    x = x[~np.isnan(x)]
    o = np.argsort(x, kind="stable")
    kx = HF.column_key_reference(x)[o]
    xs = x[o]
    assert (kx[1:] >= kx[:-1]).all() and ((kx[1:] > kx[:-1]) == (xs[1:] > xs[:-1])).all()
    # decode(encode(v)) = v up to the two canonicalisations
    allv = np.concatenate([vals, nans, x])
    back = HF.column_key_decode(HF.column_key_reference(allv))
    with np.errstate(invalid="ignore"):  # signalling NaNs in the addition
        want = np.where(np.isnan(allv), np.uint64(0x7FF8000000000000), (allv + 0.0).view(np.uint64))
    assert back.view(np.uint64).tolist() == want.tolist()
    # int64 storage of the same bits decodes alike
    assert HF.column_key_decode(HF.column_key_reference(allv).view(np.int64)).view(np.uint64).tolist() == want.tolist()


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100, 1001])
def test_quantile_index_rule(n):
    """vi = q (n - 1), lo = floor(vi), hi = min(lo + 1, n - 1), g = vi - lo, np.quantile([v_lo, v_hi], g): bit-equal
    to np.nanquantile of the column (what column_quantiles64 does with the two gathered order statistics)."""
    rng = np.random.default_rng(n)
    col = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    srt = np.sort(col)
    withnan = np.concatenate([col, [np.nan, np.nan]])
    for q in [0.0, 0.1, 0.25, 0.5, 0.75, 0.999, 1.0]:
        vi = np.float64(q) * (n - 1)
        lo = int(np.floor(vi))
        hi = min(lo + 1, n - 1)
        got = np.quantile(np.array([srt[lo], srt[hi]]), vi - lo)
        assert np.float64(got).view(np.uint64) == np.float64(np.nanquantile(withnan, q)).view(np.uint64), (n, q)


def _frame(rows=400):
    rng = np.random.default_rng(7)
    f = rng.standard_normal(rows).round(1)
    f[rng.random(rows) < 0.1] = np.nan
    f[:3] = [-0.0, 0.0, 0.0]
    return pd.DataFrame({"f": f, "i": rng.integers(0, 7, rows), "s": rng.choice(["a", "b", "c"], rows),
                         "b": rng.random(rows) < 0.5,
                         "big": np.where(np.arange(rows) % 2 == 0, 2 ** 60 + 1, 2 ** 60).astype(np.int64),
                         "empty": np.full(rows, np.nan)})


def test_eligibility():
    from hops_examples_amd.featurestore import rules

    df = _frame()
    assert [c for c in df.columns if rules.order_eligible(df[c])] == ["f", "i", "empty"]
    assert rules.order_eligible(pd.Series([1, 2, None], dtype="Int64"))
    assert rules.order_eligible(pd.Series([-(2 ** 53), 2 ** 53], dtype=np.int64))
    assert not rules.order_eligible(pd.Series([0, 2 ** 53 + 1], dtype=np.int64))
    assert not rules.order_eligible(pd.Series([1, "x"]))
    # without a GPU route nothing is stored and the pandas lines run
    cache = {}
    assert rules.prefill_order(df, list(df.columns), [0.5], cache, device="cpu") == "cpu" and cache == {}


def test_rules_read_the_order_cache():
    """Every order rule's _metric from a cache filled by the references equals the pandas path on the same frame."""
    from hops_examples_amd.featurestore import rules
    from hops_examples_amd.featurestore.rules import Rule

    df = _frame()
    feats = ["f", "i", "empty"]
    x = np.stack([rules._num(df[f]) for f in feats], 1)
    counts, ent = HF.column_runs_reference(x)
    qs = [0.5, 0.9]
    qv = HF.column_quantile_reference(x, qs)
    cache = {}
    for j, f in enumerate(feats):
        cache[f] = {"order": {"count": int(counts[j, 0]), "distinct": int(counts[j, 1]), "unique": int(counts[j, 2]),
                              "entropy": float(ent[j]), "quantile": {q: float(qv[j, i]) for i, q in enumerate(qs)}}}
    rl = [Rule(n) for n in rules._ORDER_RULES] + [Rule("HAS_APPROX_QUANTILE", legal_values=[0.9])]
    assert len(rules._ORDER_RULES) == 7
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for f in feats:
            for r in rl:
                got, want = rules._metric(r, df, f, cache), rules._metric(r, df, f, {})
                if r.name == "HAS_ENTROPY":
                    assert abs(got - want) <= _entropy_bound(cache[f]["order"]["distinct"], cache[f]["order"]["count"])
                else:
                    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (f, r.name, got, want)
    # a quantile the cache does not hold falls through to pandas; numeric rules still fill their own entry
    assert rules._metric(Rule("HAS_APPROX_QUANTILE", legal_values=[0.3]), df, "f", cache) == \
        float(np.nanquantile(rules._num(df["f"]), 0.3))
    assert rules._metric(Rule("HAS_MAX"), df, "i", cache) == 6.0 and "order" in cache["i"]
