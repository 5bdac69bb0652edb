"""The pair rules of ``featurestore.rules`` on the device route (colpair.hip) against the host route of the same frame:
the four row fractions bit for bit, the correlation within 8 x max(|np.corrcoef - long-double reference|, 2^-52) of that
reference, the mutual information within 8 x the host route's own error against the ``math.fsum`` reference (floored at
one ulp of ln(rows), three entropies); ineligible pairs stay on the host.
"""
import math

import numpy as np
import pandas as pd
import pytest

from hops_examples_amd.ops import functional as HF

pytestmark = pytest.mark.gpu

ROWS = 5000
COLS = ["f", "g", "i", "z"]


def _frame():
    rng = np.random.default_rng(12)
    f = rng.standard_normal(ROWS).round(1) + 0.0  # (round leaves -0.0 behind: only z is to hold one)
    f[rng.random(ROWS) < 0.05] = np.nan
    g = (f + rng.standard_normal(ROWS)).round(1) + 0.0
    g[rng.random(ROWS) < 0.05] = np.nan
    z = rng.integers(0, 3, ROWS).astype(np.float64)
    z[7] = -0.0
    return pd.DataFrame({"f": f, "g": g, "i": rng.integers(-3, 9, ROWS), "z": z, "s": rng.choice(["a", "b", "c"], ROWS)})


def _rules(other):
    from hops_examples_amd.featurestore import rules
    from hops_examples_amd.featurestore.rules import Rule

    return [Rule(n, legal_values=[other]) for n in rules._PAIR_RULES]


def test_prefill_pairs_matches_the_host_route():
    from hops_examples_amd.featurestore import rules

    df = _frame()
    x = df[COLS].to_numpy(np.float64)
    todo = [(r, ["f", "i"]) for r in _rules("g")] + [(r, ["f"]) for r in _rules("z") + _rules("s")]
    g, c = {}, {}
    assert rules.prefill_pairs(df, todo, g, device="cuda") == "gpu"
    assert rules.prefill_pairs(df, todo, c, device="cpu") == "cpu" and c == {}
    # -0.0 in z keeps (f, z)'s mutual information on the host while its correlation takes the device; s stays there
    assert sorted(p for p, v in g["_pairs"].items() if "mi" in v) == [("f", "g"), ("i", "g")]
    assert sorted(p for p, v in g["_pairs"].items() if "corr" in v) == [("f", "g"), ("f", "z"), ("i", "g")]
    for rule, feats in todo:
        other = rule.legal_values[0]
        for f in feats:
            got, want = rules._metric(rule, df, f, g), rules._metric(rule, df, f, c)
            if other == "s" or (other == "z" and rule.name == "HAS_MUTUAL_INFORMATION"):
                assert got == want or (math.isnan(got) and math.isnan(want))
                continue
            pr = [(COLS.index(f), COLS.index(other))]
            if rule.name == "HAS_CORRELATION":
                ref = HF.column_pair_moments_reference(x, pr)[2][0]
                bound = 8 * max(abs(want - ref), 2.0 ** -52)
                assert abs(got - ref) <= bound
            elif rule.name == "HAS_MUTUAL_INFORMATION":
                h = HF.column_pair_entropy_reference(x, pr)[0][0]
                ref = h[0] + h[1] - h[2]
                bound = 8 * max(abs(want - ref), 3 * np.spacing(math.log(ROWS)))
                assert abs(got - ref) <= bound
            else:
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (f, rule.name, got, want)


def test_validate_reports_the_pair_route(monkeypatch):
    from hops_examples_amd.featurestore import rules
    from hops_examples_amd.featurestore.rules import Expectation

    df = _frame()
    exps = [Expectation("pairs", ["f", "i"], _rules("g")), Expectation("host", ["f"], _rules("s")[:1])]
    out = {}
    for thr in (0, None):
        monkeypatch.setattr(rules, "PAIR_GPU_MIN_ROWS", thr)
        v = rules.validate(df, exps, 1)
        assert v.pair_device == ("gpu" if thr == 0 else "cpu")
        out[thr] = [(r.feature, r.rule.name, r.status) for e in v.expectation_results for r in e.results]
    assert out[0] == out[None] and {s for *_, s in out[0]} == {"SUCCESS", "FAILURE"}
