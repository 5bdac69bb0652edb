"""``functional.group_reference`` (the host statement of groupagg.hip) against ``pandas.groupby(..., sort=True).agg`` on
small frames, and ``window.group_aggregates`` on the pandas route.  Integer-valued inputs: every sum is exact, so the two
agree bit for bit."""
import numpy as np
import pandas as pd
import pytest

from hops_examples_amd.featurestore import window
from hops_examples_amd.ops import functional as HF

NAN = float("nan")
FRAMES = {
    "one_key": ([0], [[2.0, 1.0, 4.0], [1.0, 2.0, 5.0], [2.0, 3.0, 6.0], [1.0, 4.0, 7.0], [3.0, 5.0, 8.0]]),
    "two_keys": ([0, 1], [[2.0, 1.0, 4.0], [1.0, 2.0, 5.0], [2.0, 1.0, 6.0], [1.0, 3.0, 7.0], [2.0, 0.0, 8.0]]),
    "nan_keys_and_values": ([0, 1], [[1.0, NAN, 4.0], [1.0, 2.0, NAN], [NAN, 2.0, 6.0], [1.0, 2.0, 7.0], [0.0, 5.0, 8.0]]),
    "all_nan_group": ([0], [[1.0, NAN, NAN], [2.0, 3.0, 4.0], [1.0, NAN, 5.0], [2.0, 6.0, NAN]]),
    "signed_zero_is_one_key": ([0], [[-0.0, 1.0, 2.0], [0.0, 3.0, 4.0], [1.0, 5.0, 6.0], [-0.0, 7.0, 8.0]]),
}
AGGS = ["count", "sum", "min", "max", "mean", "var"]


@pytest.mark.parametrize("name", FRAMES)
def test_reference_is_pandas(name):
    key_cols, rows = FRAMES[name]
    x = np.array(rows)
    vc = [c for c in range(x.shape[1]) if c not in key_cols] + key_cols[-1:]  # a key column may be a value too
    df = pd.DataFrame(x, columns=[f"c{c}" for c in range(x.shape[1])])
    want = df.groupby([f"c{c}" for c in key_cols], sort=True)[[f"c{c}" for c in vc]].agg(AGGS)
    ref = HF.group_reference(x, key_cols, vc)
    assert ref["keys"].tolist() == [list(k) if isinstance(k, tuple) else [k] for k in want.index.tolist()]
    assert ref["dropped"] == int(df[[f"c{c}" for c in key_cols]].isna().any(axis=1).sum())
    assert np.diff(ref["seg_off"]).tolist() == df.groupby([f"c{c}" for c in key_cols]).size().tolist()
    assert x[ref["first_row"]][:, key_cols].tolist() == ref["keys"].tolist()
    for j, c in enumerate(vc):
        for a in AGGS[:-1]:
            np.testing.assert_array_equal(ref[a][:, j], want[(f"c{c}", a)].to_numpy(), err_msg=f"{name} c{c} {a}")
        # the variance is not an integer (28 / 3): pandas' fp64 Welford recurrence over <= 3 values rounds a few times
        np.testing.assert_allclose(ref["var"][:, j], want[(f"c{c}", "var")].to_numpy(), rtol=2.0 ** -50, atol=0)


def test_group_aggregates_cpu_route_is_pandas_own_frame():
    df = pd.DataFrame({"store": [3, 1, 3, 2, 1], "dept": [1.0, 1.0, NAN, 2.0, 1.0], "sales": [1.5, NAN, 2.5, 3.5, 4.5],
                       "n": [1, 2, 3, 4, 5], "name": list("abcde")})
    for by, values, aggs in (("store", ["sales", "n"], ("count", "sum", "mean", "min", "max")),
                             (["store", "dept"], "sales", ("sum", "std", "var")), ("name", ["n"], ("sum",))):
        got, route = window.group_aggregates(df, by, values, aggs=aggs, device="cpu")
        assert route == "cpu"
        pd.testing.assert_frame_equal(got, df.groupby(by, sort=True)[[values] if isinstance(values, str) else values]
                                      .agg(list(aggs)))
    assert window.GROUP_GPU_MIN_ROWS is None or window.GROUP_GPU_MIN_ROWS >= 100_000  # nothing smaller was measured
