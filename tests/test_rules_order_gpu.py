"""The order rules of ``featurestore.rules`` on the device route (one colsort.hip sort of the eligible columns) against
the pandas route of the same frame: integer-valued metrics exactly, the entropy under
(D + 8) * 2^-52 * max(1, ln count), quantiles bit for bit; ineligible columns stay on pandas.
"""
import math

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

ROWS = 5000


def _frame():
    rng = np.random.default_rng(11)
    f = rng.standard_normal(ROWS).round(2)
    f[rng.random(ROWS) < 0.05] = np.nan
    f[:4] = [-0.0, 0.0, np.inf, -np.inf]
    return pd.DataFrame({"f": f, "i": rng.integers(-3, 9, ROWS), "s": rng.choice(["a", "b", "c", "d"], ROWS),
                         "big": (2 ** 60 + rng.integers(0, 50, ROWS)).astype(np.int64)})


def _rules():
    from hops_examples_amd.featurestore import rules
    from hops_examples_amd.featurestore.rules import Rule

    return [Rule(n) for n in rules._ORDER_RULES] + [Rule("HAS_APPROX_QUANTILE", legal_values=[0.999])]


def test_prefill_order_matches_pandas():
    from hops_examples_amd.featurestore import rules

    df = _frame()
    feats = list(df.columns)
    g, c = {}, {}
    assert rules.prefill_order(df, feats, [0.5, 0.999], g, device="cuda") == "gpu"
    assert rules.prefill_order(df, feats, [0.5, 0.999], c, device="cpu") == "cpu" and c == {}
    assert sorted(f for f in g if "order" in g[f]) == ["f", "i"]  # the string and the 2^60 column stay on pandas
    assert g["f"]["order"]["count"] == int(df["f"].notna().sum())
    for f in feats:
        for r in _rules():
            got, want = rules._metric(r, df, f, g), rules._metric(r, df, f, c)
            if r.name == "HAS_ENTROPY" and f in ("f", "i"):
                o = g[f]["order"]
                bound = (o["distinct"] + 8) * 2.0 ** -52 * max(1.0, math.log(max(o["count"], 1)))
                print(f"rules-entropy {f}: err {abs(got - want):.3e} bound {bound:.3e}")
                assert abs(got - want) <= bound
            elif f == "s" and r.name == "HAS_APPROX_QUANTILE":
                assert math.isnan(got) and math.isnan(want)  # _num turns the strings into NaN on either route
            else:
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (f, r.name, got, want)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_validate_statuses_on_both_routes(monkeypatch):
    from hops_examples_amd.featurestore import rules
    from hops_examples_amd.featurestore.rules import Expectation, Rule

    df = _frame()
    ref = {r.name: rules._metric(r, df, "i", {}) for r in _rules()[:7]}
    exps = [Expectation("pass", ["f", "i", "s", "big"], [Rule(n, min=0) for n in rules._ORDER_RULES if n != "HAS_APPROX_QUANTILE"]),
            Expectation("tight", ["i"], [Rule(n, min=ref[n], max=ref[n]) for n in rules._ORDER_RULES if n != "HAS_ENTROPY"]),
            Expectation("fail", ["f", "i"], [Rule("HAS_NUMBER_OF_DISTINCT_VALUES", max=3), Rule("HAS_ENTROPY", level="WARNING", max=0.1),
                                             Rule("HAS_APPROX_QUANTILE", min=100.0), Rule("HAS_MEAN", min=-1.0)])]
    out = {}
    for thr in (0, 10 ** 9):
        monkeypatch.setattr(rules, "ORDER_GPU_MIN_ROWS", thr)
        v = rules.validate(df, exps, 1)
        assert v.order_device == ("gpu" if thr == 0 else "cpu")
        out[thr] = [(e.expectation.name, r.feature, r.rule.name, r.status) for e in v.expectation_results for r in e.results]
    assert out[0] == out[10 ** 9]
    st = {s for *_, s in out[0]}
    assert st == {"SUCCESS", "WARNING", "FAILURE"}
    assert all(s == "SUCCESS" for n, *_, s in out[0] if n == "tight")
