"""The one-launch evaluator of the E1 / E8 / E11 CNN family (csrc/ops/cnn_eval.hip, runtime/cnn_eval.py) against
an fp64 PyTorch reference with the kernel's bf16 rounding points, over the geometries that isolate each thing
that can break; its invariance contract, the label guard, refusals, graph replay and the keras front end.

Every numeric bound is 4 x the error of the fp32 PROXY (the same reference in fp32) against the fp64 reference on
the test's own inputs (the rule of tests/test_mnist_eval_gpu.py).  Setup: seed 1, fc2.weight x 16 so that top-2
margins clear the rounding noise, N = 2 tiles + 3 random images (generator seed 9).

Measured on an MI355X: logits max err 6.3e-07 .. 3.0e-04 against bounds 1.5e-06 .. 6.5e-03; the tightest case is
k8-p8-valid (11 images, one pooled position, no bf16 flip in the proxy): 6.295e-07 against 1.455e-06."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.models.mnist import FashionMnistCNN, KerasMnistCNN  # noqa: E402
from hops_examples_amd.ops import _C, kernels as K  # noqa: E402
from hops_examples_amd.runtime import capture, cnn_eval  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402
from hops_examples_amd.runtime.persist_eval import PARAMS  # noqa: E402

DEV = torch.device("cuda", 0)
GEOMS = [(2, 2, 0), (4, 4, 0), (8, 8, 0), (8, 2, 0), (2, 8, 0), (5, 3, 0), (3, 2, 1), (4, 3, 1), (8, 8, 1)]


def _make(k, p, pad):
    torch.manual_seed(1)
    m = (FashionMnistCNN if pad else KerasMnistCNN)(kernel=k, pool=p)
    if pad:
        m.conv1.in_affine = (1.0 / 255.0, -0.5)  # a pad treated as pixel 0 would contribute -0.5, not 0
    m = m.to(DEV)
    arena = ParamArena.from_module(m, DEV)
    with torch.no_grad():
        m.fc2.weight.mul_(16.0)
    arena.refresh_shadow()
    ev = cnn_eval.CnnFamilyEvaluator(m)
    x = torch.randint(0, 256, (2 * ev.tile + 3, 28, 28, 1), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    return m, arena, ev, x


def _refs(m, ev, x_cpu):
    named = dict(m.named_parameters())
    P = {q: named[q].detach().cpu().clone() for q in PARAMS}
    sc, sh = m.conv1.in_affine
    kw = dict(k=ev.k, p=ev.p, pad=ev.pad, xscale=float(sc), xshift=float(sh), emulate_bf16=True)
    ref = cnn_eval.reference_logits(P, x_cpu, **kw)
    proxy = cnn_eval.reference_logits(P, x_cpu, dtype=torch.float32, **kw).double()
    return ref, proxy, float((proxy - ref).abs().max())


def _ce(z, y):
    return torch.nn.functional.cross_entropy(z, y, reduction="none")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, rows=None, fields=("logits", "loss", "hit")):
    for f in fields:
        ta = getattr(a, f) if rows is None else getattr(a, f)[rows]
        assert torch.equal(_bits(ta), _bits(getattr(b, f))), f


def _check_logits(z, ref, e32):
    z = z.double().cpu()
    err = float((z - ref).abs().max())
    cos = float(torch.nn.functional.cosine_similarity(z, ref, dim=1).min())
    print(f"logits: max err {err:.3e} (e32 {e32:.3e}, bound {4 * e32:.3e}), min cosine {cos:.9f}")
    assert err <= 4 * e32 and cos >= 0.99999, (err, e32, cos)


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: "k%d-p%d-%s" % (g[0], g[1], "same" if g[2] else "valid"))
def ctx(request):
    """One reference and one run per geometry, shared and left unchanged."""
    m, arena, ev, x = _make(*request.param)
    ref, proxy, e32 = _refs(m, ev, x)
    am = ref.argmax(1)
    y = torch.where(torch.arange(len(x)) % 2 == 0, am, (am + 1) % 10)
    xs, ys = x.to(DEV), y.to(DEV)
    res = ev.run(xs, ys)
    torch.cuda.synchronize()
    assert K.debug_errors() == []
    return dict(m=m, ev=ev, y=y, xs=xs, ys=ys, ref=ref, proxy=proxy, e32=e32, res=res)


def test_against_the_reference(ctx):
    ref, proxy, y, res, e32, n = ctx["ref"], ctx["proxy"], ctx["y"], ctx["res"], ctx["e32"], len(ctx["y"])
    assert ctx["ev"].plan.in_features == ctx["m"].fc1.weight.shape[1] and res.logits.shape == (n, 10)
    _check_logits(res.logits, ref, e32)
    ce_ref = _ce(ref, y)
    e_ce = float((_ce(proxy, y) - ce_ref).abs().max())
    loss = res.loss.double().cpu()
    err = float((loss - ce_ref).abs().max())
    print(f"loss: max err {err:.3e} (proxy {e_ce:.3e}, bound {4 * e_ce:.3e})")
    assert err <= 4 * e_ce, (err, e_ce)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * 4 * e32
    print(f"hits: {int((~clear).sum())} of {n} images left out")
    assert int((~clear).sum()) <= 0.05 * n
    hit = res.hit.cpu()
    assert torch.equal(hit[clear].bool(), (ref.argmax(1) == y)[clear])
    totals = res.totals.cpu()
    assert float(totals[1]) == float(hit.sum())
    s = float(loss.sum())
    assert abs(float(totals[0]) - s) <= n * 2.0 ** -24 * abs(s), (float(totals[0]), s)


def test_outputs_depend_only_on_the_image(ctx):
    ev, xs, ys, res, t = ctx["ev"], ctx["xs"], ctx["ys"], ctx["res"], ctx["ev"].tile
    sizes = (1, t - 1, t, t + 1) if (ev.k, ev.p, ev.pad) in ((4, 4, 0), (4, 3, 1)) else (1,)
    for n in sizes:
        _same(res, ev.run(xs[:n], ys[:n]), slice(0, n))
    lo = t + 1  # another position: the set's image lo is the run's image 0
    _same(res, ev.run(xs[lo:lo + 2], ys[lo:lo + 2]), slice(lo, lo + 2))
    one = cnn_eval.CnnFamilyEvaluator(ctx["m"], max_workgroups=1).run(xs, ys)
    _same(res, one, fields=("logits", "loss", "hit", "totals"))
    only = ev.run(xs)
    assert only.loss is None and only.totals is None and torch.equal(_bits(only.logits), _bits(res.logits))
    before = ev.launches
    assert ev.run(xs[:0], ys[:0]).n == 0 and ev.launches == before


def test_label_guard():
    m, arena, ev, x = _make(4, 4, 0)
    xs = x.to(DEV)
    ys = torch.arange(len(x), device=DEV) % 10
    res = ev.run(xs, ys)
    bad = ys.clone()
    i, j = 5, ev.tile + 3
    bad[i], bad[j] = -1, 10
    assert K.debug_errors() == []
    if os.environ.get("HOPSX_DEBUG", "0") == "1":  # the debug build raises at the launch
        with pytest.raises(RuntimeError, match="cnn_eval.hip"):
            ev.run(xs, bad)
        return
    r = ev.run(xs, bad)
    errs = K.debug_errors()
    assert errs and errs[0][0] == "cnn_eval" and errs[0][1] == 2 and K.debug_errors() == [], errs
    assert float(r.loss[i]) == 0.0 and float(r.loss[j]) == 0.0 and int(r.hit[i]) == 0 and int(r.hit[j]) == 0
    keep = torch.ones(len(xs), dtype=torch.bool, device=DEV)
    keep[i] = keep[j] = False
    assert torch.equal(_bits(r.logits), _bits(res.logits))
    assert torch.equal(_bits(r.loss[keep]), _bits(res.loss[keep])) and torch.equal(r.hit[keep], res.hit[keep])
    assert float(r.totals[1]) == float(r.hit.sum())


@pytest.mark.parametrize("k,p", [(9, 4), (4, 1)])
def test_launcher_refuses_a_geometry_outside_the_family(k, p):
    m, arena, ev, x = _make(4, 4, 0)
    xs, ys = x.to(DEV), torch.zeros(len(x), dtype=torch.int64, device=DEV)
    out = ev._alloc(len(x), True, DEV)
    for t in (out.logits, out.loss, out.totals):
        t.fill_(-7.0)
    out.hit.fill_(9)
    named = dict(m.named_parameters())
    ptrs = [arena.master.data_ptr(), arena.shadow.data_ptr(), xs.data_ptr(), ys.data_ptr(), out.logits.data_ptr(),
            out.loss.data_ptr(), out.hit.data_ptr(), out.totals.data_ptr(), out._part.data_ptr()]
    iv = [int(named[q]._hx_off) for q in PARAMS] + [len(x), 0, k, p, 0]
    assert _C.ext().cnn_eval(ptrs, iv, [1.0 / 255.0, 0.0], _C.stream()) != 0 and _C.ext().cnn_eval_plan(k, p, 0) == []
    torch.cuda.synchronize()
    assert bool((out.logits == -7.0).all() and (out.loss == -7.0).all() and (out.totals == -7.0).all()
                and (out.hit == 9).all())


def test_graph_replay_reads_the_live_weights():
    m, arena, ev, x = _make(3, 2, 1)
    xs = x.to(DEV)
    ys = torch.arange(len(x), device=DEV) % 10
    res = ev.run(xs, ys)  # eager: allocates the outputs the capture reuses
    first = res.logits.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture.graph(g):
        assert ev.run(xs, ys, out=res) is res
    with torch.no_grad():
        gen = torch.Generator(device=DEV).manual_seed(2)
        arena.master.add_(torch.randn(arena.master.shape, device=DEV, generator=gen) * 2e-3)
    arena.refresh_shadow()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(res.logits, first)
    _same(res, ev.run(xs, ys), fields=("logits", "loss", "hit", "totals"))
    ref, _, e32 = _refs(m, ev, x)
    _check_logits(res.logits, ref, e32)
    with pytest.raises(ValueError):
        ev.run(xs[:5], ys[:5], out=res)


# ------------------------------------------------------------------------------------------- keras
def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 28, 28, 1)).astype(np.uint8), rng.integers(0, 10, n).astype(np.int64)


@pytest.mark.parametrize("builder", ["keras_mnist_cnn", "fashion_mnist_cnn"])  # k4 p4 valid softmax / k3 p2 same
def test_keras_front_end(builder, monkeypatch):
    from hops_examples_amd.models import zoo

    monkeypatch.setenv("HOPSX_EVAL_FAMILY", "1")
    torch.manual_seed(0)
    m = getattr(zoo, builder)()
    m.compile(optimizer="adam", loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    x, y = _data(37)
    loss, acc = m.evaluate(x, y, verbose=0)
    ev = m._family_engine
    assert ev.launches == 1 and m._evaluator(x) is None and getattr(m, "_eval_engine", None) is None
    r = ev.run(*m._eval_resident(x, y))
    tl, tc = (float(v) for v in r.totals.tolist())
    assert loss == tl / len(x) and acc == tc / len(x)
    pr = m.predict(x)
    assert ev.launches == 3 and pr.shape == (len(x), 10) and pr.dtype == np.float32
    assert np.array_equal(pr.argmax(1), r.logits.argmax(1).cpu().numpy())
    if builder == "keras_mnist_cnn":  # the stack that ends in a softmax
        assert float(np.abs(pr.sum(1) - 1.0).max()) <= 1e-6
    else:
        assert np.array_equal(pr, r.logits.cpu().numpy())
    xv, yv = _data(19, seed=5)
    h = m.fit(x, y, batch_size=16, epochs=2, verbose=0, validation_data=(xv, yv))
    assert ev.launches == 5 and len(h.history["val_loss"]) == 2
    monkeypatch.setenv("HOPSX_EVAL_FAMILY", "0")  # the batch-by-batch route: same keys and shapes, no launch here
    d1 = m.evaluate(x, y, verbose=0, return_dict=True)
    p0 = m.predict(x)
    assert ev.launches == 5 and list(d1) == ["loss", "accuracy"] and p0.shape == pr.shape and p0.dtype == pr.dtype
