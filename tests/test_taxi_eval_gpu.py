"""The one-launch sliced evaluator of the taxi wide & deep model (csrc/ops/taxi_eval.hip, runtime/taxi_eval.py)
against the bf16-emulating fp64 reference, its integer accumulators against the numpy oracle (exactly), its
invariance contract (a row's outputs depend only on that row and the weights; the accumulators on nothing but
the rows), the guards, graph replay, live weights after the training kernel, and the pipeline's Evaluator /
Trainer wiring.

Every numeric bound is 4 x the error of the fp32 PROXY (the reference evaluated in fp32) against the fp64
reference, computed here from the reference alone (the rule of tests/test_mnist_eval_gpu.py).  n = 2,085 =
130 full tiles + a 5-row tail; 33 workgroup trips, so max_workgroups = 3 takes several grid-stride trips.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.models import widedeep as WD  # noqa: E402
from hops_examples_amd.ops import kernels as K  # noqa: E402
from hops_examples_amd.runtime import capture  # noqa: E402
from hops_examples_amd.runtime import taxi_eval as TE  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402
from hops_examples_amd.runtime.taxi_step import FusedWideDeepStep  # noqa: E402

DEV = torch.device("cuda", 0)
N = 2085
HOUR = TE.WIDE_FEATURE_KEYS.index("trip_start_hour")


def _model(seed=1):
    """Default init under ``seed``, wide.weight = randn * 0.5 (the wide part initialises to zero)."""
    torch.manual_seed(seed)
    m = WD.TaxiWideDeep()
    with torch.no_grad():
        m.wide.weight.copy_(torch.randn(WD.WIDE_ROWS, 1, generator=torch.Generator().manual_seed(seed)) * 0.5)
    m.to(DEV)
    arena = ParamArena.from_module(m, DEV)
    return m, arena


def _refs(m, dense, cat):
    """fp64 reference logits, fp32 proxy logits (CPU, bf16 rounding emulated) and e32 = max |proxy - ref|."""
    ref = TE.reference_logits(m, dense, cat).numpy()
    proxy = TE.reference_logits(m, dense, cat, dtype=torch.float32).numpy()
    return ref, proxy, float(np.abs(proxy.astype(np.float64) - ref).max())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_rows(a, b, rows=None):
    """Bitwise equality of two results' per-row outputs (a's rows `rows` against all of b)."""
    for f in ("logit", "prob", "loss", "hit"):
        ta, tb = getattr(a, f), getattr(b, f)
        assert (ta is None) == (tb is None), f
        if ta is not None:
            assert torch.equal(_bits(ta if rows is None else ta[rows]), _bits(tb)), f


def _same_acc(a, b):
    assert torch.equal(a.acc, b.acc)


def _check_logits(z, ref, e32, what="logits"):
    err = float(np.abs(z.double().cpu().numpy() - ref).max())
    print(f"{what}: max err {err:.3e} (e32 {e32:.3e}, bound {4 * e32:.3e})")
    assert err <= 4 * e32, (err, e32)


@pytest.fixture(scope="module")
def ctx():
    m, arena = _model()
    assert TE.TaxiEvaluator.supported(m)
    dense, cat, label = WD.synth_taxi(N, seed=3)
    ref, proxy, e32 = _refs(m, dense, cat)
    ev = TE.TaxiEvaluator(m)
    d, c, y = dense.to(DEV), cat.to(DEV), label.to(DEV)
    assert K.debug_errors() == []
    res = ev.run(d, c, y, slice_by="trip_start_hour")
    torch.cuda.synchronize()
    assert K.debug_errors() == []
    return dict(m=m, arena=arena, ev=ev, dense=dense, cat=cat, label=label, d=d, c=c, y=y, ref=ref, proxy=proxy,
                e32=e32, res=res)


def test_rows_match_the_reference(ctx):
    res, ref, proxy, e32 = ctx["res"], ctx["ref"], ctx["proxy"], ctx["e32"]
    assert res.n == N and res.logit.shape == (N,) and res.prob.shape == (N,) and res.S == 24
    _check_logits(res.logit, ref, e32)
    y = ctx["label"].numpy().reshape(-1)
    loss_ref = TE.bce_with_logits(ref, y.astype(np.float64))
    e_loss = float(np.abs(TE.bce_with_logits(proxy, y).astype(np.float64) - loss_ref).max())
    err = float(np.abs(res.loss.double().cpu().numpy() - loss_ref).max())
    print(f"loss: max err {err:.3e} (proxy {e_loss:.3e}, bound {4 * e_loss:.3e})")
    assert err <= 4 * e_loss, (err, e_loss)
    p_ref = 1.0 / (1.0 + np.exp(-ref))
    p_err = float(np.abs(res.prob.double().cpu().numpy() - p_ref).max())
    print(f"prob: max err {p_err:.3e}")
    assert p_err <= 4 * e32  # |sigmoid'| <= 1/4: a looser bound than the logits'
    clear = np.abs(ref) > 4 * e32
    left_out = int((~clear).sum())
    print(f"hits: {left_out} of {N} rows left out (|z_ref| <= 4 e32)")
    assert left_out <= 0.05 * N
    hit = res.hit.cpu().numpy()
    assert res.hit.dtype == torch.uint8
    assert np.array_equal(hit[clear] != 0, ((ref > 0) == (y > 0.5))[clear])


@pytest.mark.parametrize("slice_by", ["trip_start_hour", 0])
def test_accumulators_equal_the_numpy_oracle(ctx, slice_by):
    ev = ctx["ev"]
    res = ctx["res"] if slice_by == "trip_start_hour" else ev.run(ctx["d"], ctx["c"], ctx["y"], slice_by=slice_by)
    col = TE.slice_column(slice_by)
    S = WD.wide_cardinalities()[col]
    assert res.S == S and res.slice_col == col
    sums, hist = res.accumulators()
    want_s, want_h = TE.accumulate_rows(res.prob, res.loss, ctx["label"], TE.slice_ids_of(ctx["cat"], col), S, hit=res.hit)
    assert sums.dtype == np.uint64 and hist.dtype == np.uint32
    assert np.array_equal(hist, want_h)
    assert np.array_equal(sums, want_s)
    assert int(hist[0].sum()) == N and int(hist[1:].sum()) == N
    m = TE.metrics(res)
    o = m["overall"]
    print(f"overall: {({k: o[k] for k in ('accuracy', 'log_loss', 'calibration', 'auc_bucketed', 'auc_bound')})}; "
          f"smallest slice {min(s['count'] for s in m['slices'])} rows")
    assert o["count"] == N and abs(o["log_loss"] - float(res.loss.double().mean())) <= 2.0 ** -24


def test_outputs_do_not_depend_on_grid_n_or_position(ctx):
    m, ev, d, c, y, res = ctx["m"], ctx["ev"], ctx["d"], ctx["c"], ctx["y"], ctx["res"]
    for wg in (1, 3):
        capped = TE.TaxiEvaluator(m, max_workgroups=wg).run(d, c, y, slice_by="trip_start_hour")
        _same_rows(res, capped)
        _same_acc(res, capped)
    again = ev.run(d, c, y, slice_by="trip_start_hour")
    _same_rows(res, again)
    _same_acc(res, again)
    for n in (1, 15, 16, 17, 63, 64, 65):
        part = ev.run(d[:n], c[:n], y[:n], slice_by="trip_start_hour")
        _same_rows(res, part, slice(0, n))
        sums, hist = part.accumulators()
        assert int(hist[0].sum()) == n and int(sums[0, 0]) == int(part.hit.sum())
    lo = 16 * 3 + 5  # another position in the set
    _same_rows(res, ev.run(d[lo:lo + 70], c[lo:lo + 70], y[lo:lo + 70]), slice(lo, lo + 70))
    before = ev.launches
    empty = ev.run(d[:0], c[:0], y[:0], slice_by="trip_start_hour")
    assert empty.n == 0 and empty.logit.shape == (0,) and ev.run(d[:0], c[:0]).n == 0 and ev.launches == before


def test_labels_are_optional(ctx):
    ev, d, c, res = ctx["ev"], ctx["d"], ctx["c"], ctx["res"]
    only = ev.run(d, c)
    assert only.loss is None and only.hit is None and only.acc is None
    assert torch.equal(_bits(only.logit), _bits(res.logit)) and torch.equal(_bits(only.prob), _bits(res.prob))
    with pytest.raises(ValueError):
        ev.run(d, c, slice_by="trip_start_hour")  # slices are label histograms
    with pytest.raises(ValueError):
        only.accumulators()


def test_reuse_and_graph_replay(ctx):
    ev, d, c, y, res = ctx["ev"], ctx["d"], ctx["c"], ctx["y"], ctx["res"]
    sd, sc, sy = d.clone(), c.clone(), y.clone()
    out = ev.run(sd, sc, sy, slice_by="trip_start_hour")  # eager: allocates the outputs the capture reuses
    assert ev.run(sd, sc, sy, slice_by="trip_start_hour", out=out) is out  # twice into one result: not doubled
    _same_acc(res, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture.graph(g):
        assert ev.run(sd, sc, sy, slice_by="trip_start_hour", out=out) is out
    nd, nc, ny = (t.to(DEV) for t in WD.synth_taxi(N, seed=5))
    sd.copy_(nd)
    sc.copy_(nc)
    sy.copy_(ny)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    fresh = ev.run(nd, nc, ny, slice_by="trip_start_hour")
    _same_rows(out, fresh)
    _same_acc(out, fresh)
    assert not torch.equal(out.acc, res.acc)
    with pytest.raises(ValueError):
        ev.run(nd[:5], nc[:5], ny[:5], slice_by="trip_start_hour", out=out)
    with pytest.raises(ValueError):
        ev.run(nd, nc, ny, slice_by=0, out=out)  # another S


def test_guards(ctx):
    m, ev, d, c, y, res = ctx["m"], ctx["ev"], ctx["d"], ctx["c"], ctx["y"], ctx["res"]
    for bad in ("payment_type", "company", "pickup_census_tract", "dropoff_census_tract", 4, 5, 9, 10):
        with pytest.raises(ValueError):
            ev.run(d, c, y, slice_by=bad)
    i, j = 7, 16 * 6 + 4
    bad = c.clone()
    old_id = int(bad[i, 2])
    bad[i, 2] = WD.WIDE_ROWS + 5  # a wide id past the table, in a non-slice column
    bad[j, HOUR] = int(WD.wide_offsets()[HOUR]) + 24 + 3  # a slice id past its column's range (a valid table row)
    assert K.debug_errors() == []
    if os.environ.get("HOPSX_DEBUG", "0") == "1":  # the debug build raises at the launch (tests/test_debug_checks_gpu.py)
        with pytest.raises(RuntimeError, match="taxi_eval.hip"):
            ev.run(d, bad, y, slice_by="trip_start_hour")
        return
    r = ev.run(d, bad, y, slice_by="trip_start_hour")
    errs = K.debug_errors()
    assert errs and errs[0][0] == "taxi_eval" and errs[0][1] == 2, errs
    assert K.debug_errors() == []
    wide = m.wide.weight.detach().double().cpu().numpy().reshape(-1)
    want = ctx["ref"][i] - wide[old_id]  # the reference without that table row
    err = abs(float(r.logit[i]) - want)
    print(f"guarded row: err {err:.3e} (bound {4 * ctx['e32']:.3e})")
    assert err <= 4 * ctx["e32"]
    sums, hist = r.accumulators()
    assert int(hist[0].sum()) == N and int(hist[1:].sum()) == N - 1  # row j: in "overall", in no slice
    want_s, want_h = TE.accumulate_rows(r.prob, r.loss, ctx["label"], TE.slice_ids_of(bad, HOUR), 24, hit=r.hit)
    assert np.array_equal(hist, want_h) and np.array_equal(sums, want_s)
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[i] = keep[j] = False
    for f in ("logit", "prob", "loss", "hit"):
        assert torch.equal(_bits(getattr(r, f))[keep], _bits(getattr(res, f))[keep]), f
    assert float(r.logit[j]) != float(res.logit[j])  # (it gathered the other table row)


def test_live_weights_after_the_training_kernel(ctx):
    """64 steps of the one-launch training kernel, then the evaluator with no sync in between: stream order,
    and no stale copy of any weight (fp32 master or bf16 shadow)."""
    m, _ = _model(seed=2)
    opt = WD.make_optimizer(m)
    fused = FusedWideDeepStep(m, opt)
    assert fused.ok(40)
    td, tc, ty = (t.to(DEV) for t in WD.synth_taxi(8 * 40, seed=4))
    xs, ys = (td.view(8, 40, -1), tc.view(8, 40, -1)), ty.view(8, 40, 1)
    ev = TE.TaxiEvaluator(m)
    d, c, y = ctx["d"], ctx["c"], ctx["y"]
    first = ev.run(d, c, y).logit.clone()
    fused.run_resident(xs, ys, 64)
    r = ev.run(d, c, y)
    torch.cuda.synchronize()
    assert not torch.equal(r.logit, first)
    ref, _, e32 = _refs(m, ctx["dense"], ctx["cat"])
    _check_logits(r.logit, ref, e32, "after 64 steps")


def test_pipeline_evaluator_and_trainer(tmp_path, monkeypatch):
    monkeypatch.setenv("HOPSX_PROJECT_ROOT", str(tmp_path))
    from hops_examples_amd.tfx import pipeline, synth_raw_trips

    raw = tmp_path / "raw.parquet"
    synth_raw_trips(3000, seed=2).to_parquet(raw)
    root = tmp_path / "pipe"
    pipeline.example_gen(root, raw)
    pipeline.transform(root, device="cpu")
    t0 = pipeline.trainer(root, steps=100, device="cuda")
    assert t0["step"] == "fused" and "eval_curve" not in t0
    sd0 = torch.load(root / "trainer" / "model.pt", weights_only=True)
    ev = pipeline.evaluator(root, device="cuda", slice_by=("trip_start_hour", "pickup_community_area"))
    assert ev["path"] == "fused" and set(ev["slices"]) == {"trip_start_hour", "pickup_community_area"}
    n = ev["eval_rows"]
    # the reference's view of this model and split
    dense, cat, label = pipeline._load_transformed(root, "eval", torch.device("cpu"))
    ref = TE.reference_logits(sd0, dense, cat).numpy()
    proxy = TE.reference_logits(sd0, dense, cat, dtype=torch.float32).numpy()
    e32 = float(np.abs(proxy.astype(np.float64) - ref).max())
    left_out = int((np.abs(ref) <= 4 * e32).sum())
    y = label.numpy()[:, 0].astype(np.float64)

    def eps_loss(z):  # the pipeline's per-row log-loss (with its eps), in z's precision
        p = 1 / (1 + np.exp(-z))
        eps = z.dtype.type(1e-7)
        return -(y.astype(z.dtype) * np.log(p + eps) + (1 - y.astype(z.dtype)) * np.log(1 - p + eps))

    e_ll = float(np.abs(eps_loss(proxy).astype(np.float64) - eps_loss(ref)).max())
    monkeypatch.setenv("HOPSX_TAXI_EVAL_FUSED", "0")
    lw = pipeline.evaluator(root, device="cuda", slice_by=("trip_start_hour",))
    monkeypatch.delenv("HOPSX_TAXI_EVAL_FUSED")
    assert lw["path"] == "layerwise" and lw["eval_rows"] == n
    print(f"fused acc {ev['accuracy']:.6f} log_loss {ev['log_loss']:.6f} auc {ev['auc']:.6f} | layerwise acc "
          f"{lw['accuracy']:.6f} log_loss {lw['log_loss']:.6f} auc {lw['auc']:.6f} | n {n} left out {left_out} "
          f"e32 {e32:.3e} proxy loss error {e_ll:.3e}")
    assert abs(ev["accuracy"] - lw["accuracy"]) <= left_out / n + 1e-12
    assert abs(ev["log_loss"] - lw["log_loss"]) <= 4 * e_ll
    # the slices: metrics_from_rows on the evaluator's own per-row outputs
    m = WD.TaxiWideDeep()
    m.load_state_dict(sd0)
    m.to(DEV)
    ParamArena.from_module(m, DEV)
    d, c, yy = dense.to(DEV), cat.to(DEV), label.to(DEV)
    r = TE.TaxiEvaluator(m).run(d, c, yy, slice_by="pickup_community_area")
    want = TE.metrics_from_rows(r.prob, r.loss, label, TE.slice_ids_of(cat, 11), 80, hit=r.hit)
    got = ev["slices"]["pickup_community_area"]
    assert len(got) == 80 and sum(s["count"] for s in got.values()) == n
    for v, s in enumerate(want["slices"]):
        assert {k: got[str(v)][k] for k in ("count", "positives", "hits", "loss_q", "prob_q")} == \
            {k: s[k] for k in ("count", "positives", "hits", "loss_q", "prob_q")}, v
    assert ev["auc_bucketed"] == want["overall"]["auc_bucketed"]
    assert abs(ev["auc_bucketed"] - ev["auc"]) <= want["overall"]["auc_bound"] + 1e-12
    # train_and_evaluate: two points, and the same final weights bit for bit
    t1 = pipeline.trainer(root, steps=100, device="cuda", eval_every=50)
    curve = t1["eval_curve"]
    print(f"eval_curve {curve}")
    assert [p["step"] for p in curve] == [50, 100] and all(
        set(p) == {"step", "log_loss", "accuracy", "auc_bucketed"} and p["log_loss"] == p["log_loss"] for p in curve)
    sd1 = torch.load(root / "trainer" / "model.pt", weights_only=True)
    assert set(sd0) == set(sd1) and all(torch.equal(_bits(sd0[k]), _bits(sd1[k])) for k in sd0)
    assert {k: curve[1][k] for k in ("log_loss", "accuracy", "auc_bucketed")} == \
        {k: want["overall"][k] for k in ("log_loss", "accuracy", "auc_bucketed")}  # (the same weights, the same split)
