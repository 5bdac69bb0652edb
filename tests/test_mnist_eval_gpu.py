"""The one-launch evaluator of the flagship MNIST CNN (csrc/ops/mnist_eval.hip, runtime/persist_eval.py)
against an fp64 PyTorch reference with the kernel's bf16 rounding points, its invariance contract (an image's
outputs depend only on that image and the weights), determinism of the totals, the label guard, graph
replay, live weights, and the keras front end that routes evaluate / predict / validation to it.

Every numeric bound is 4 x the error of the fp32 PROXY (the same reference function evaluated in fp32)
against the fp64 reference, computed here on the test's own inputs: the kernel is another fp32 ordering of
the same sums, the factor covers a different set of bf16 rounding flips.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd import optim  # noqa: E402
from hops_examples_amd.models.mnist import MirroredMnistCNN  # noqa: E402
from hops_examples_amd.ops import kernels as K  # noqa: E402
from hops_examples_amd.runtime import capture, persist, persist_eval  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402

DEV = torch.device("cuda", 0)
PARAMS = persist.PersistentMnistStep.PARAMS


def _make():
    """The issue's setup: seed 1, fc2.weight x 16 (random-init logits are ~0.03 in size, their top-2 margins
    below the rounding noise; x 16 they reach ~1.9), 97 = 3 tiles + 1 random images (generator seed 9)."""
    torch.manual_seed(1)
    m = MirroredMnistCNN().to(DEV)  # (left in training mode: inference never drops)
    arena = ParamArena.from_module(m, DEV)
    with torch.no_grad():
        m.fc2.weight.mul_(16.0)
    arena.refresh_shadow()
    ev = persist_eval.MnistEvaluator(m)
    n = 3 * ev.tile + 1
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, 256, (n, 28, 28, 1), dtype=torch.uint8, generator=g)
    return m, arena, ev, x


def _snapshot(m):
    named = dict(m.named_parameters())
    return {k: named[k].detach().cpu().clone() for k in PARAMS}


def _refs(m, P, x_cpu):
    """fp64 reference logits, fp32 proxy logits (both on the CPU, bf16 rounding emulated) and e32."""
    scale, shift = m.conv1.in_affine
    kw = dict(xscale=float(scale), xshift=float(shift), emulate_bf16=True)
    ref = persist_eval.reference_logits(P, x_cpu, **kw)
    proxy = persist_eval.reference_logits(P, x_cpu, dtype=torch.float32, **kw).double()
    return ref, proxy, float((proxy - ref).abs().max())


def _ce(z, y):
    return torch.nn.functional.cross_entropy(z, y, reduction="none")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, rows=None, totals=False):
    """Bitwise equality of two results' per-image outputs (a's rows `rows` against all of b)."""
    for f in ("logits", "loss", "hit") + (("totals",) if totals else ()):
        ta, tb = getattr(a, f), getattr(b, f)
        if rows is not None:
            ta = ta[rows]
        assert torch.equal(_bits(ta), _bits(tb)), f


def _check_logits(z, ref, e32):
    """Test 1's criterion."""
    z = z.double().cpu()
    err = float((z - ref).abs().max())
    cos = torch.nn.functional.cosine_similarity(z, ref, dim=1)
    print(f"logits: max err {err:.3e} (e32 {e32:.3e}, bound {4 * e32:.3e}), min cosine {float(cos.min()):.9f}")
    assert err <= 4 * e32, (err, e32)
    assert float(cos.min()) >= 0.99999, float(cos.min())


@pytest.fixture(scope="module")
def ctx():
    m, arena, ev, x = _make()
    P = _snapshot(m)
    ref, proxy, e32 = _refs(m, P, x)
    am = ref.argmax(1)
    y = torch.where(torch.arange(len(x)) % 2 == 0, am, (am + 1) % 10)
    xs, ys = x.to(DEV), y.to(DEV)
    res = ev.run(xs, ys)
    torch.cuda.synchronize()
    assert K.debug_errors() == []
    return dict(m=m, arena=arena, ev=ev, x=x, y=y, xs=xs, ys=ys, ref=ref, proxy=proxy, e32=e32, res=res)


def test_logits_match_the_reference(ctx):
    assert ctx["res"].logits.shape == (len(ctx["x"]), 10) and ctx["res"].n == len(ctx["x"])
    print(f"e32 = {ctx['e32']:.3e}")
    _check_logits(ctx["res"].logits, ctx["ref"], ctx["e32"])


def test_loss_hits_and_totals(ctx):
    ref, proxy, y, res = ctx["ref"], ctx["proxy"], ctx["y"], ctx["res"]
    n = len(y)
    ce_ref = _ce(ref, y)
    e_ce = float((_ce(proxy, y) - ce_ref).abs().max())
    loss = res.loss.double().cpu()
    err = float((loss - ce_ref).abs().max())
    print(f"loss: max err {err:.3e} (proxy {e_ce:.3e}, bound {4 * e_ce:.3e})")
    assert err <= 4 * e_ce, (err, e_ce)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 3e-3
    left_out = int((~clear).sum())
    print(f"hits: {left_out} of {n} images left out (reference top-2 margin < 3e-3)")
    assert left_out <= 0.05 * n
    hit = res.hit.cpu()
    assert hit.dtype == torch.uint8
    assert torch.equal(hit[clear].bool(), (ref.argmax(1) == y)[clear])
    totals = res.totals.cpu()
    assert float(totals[1]) == float(hit.sum())
    s = float(loss.sum())
    assert abs(float(totals[0]) - s) <= n * 2.0 ** -24 * abs(s), (float(totals[0]), s)


def test_outputs_do_not_depend_on_n_or_position(ctx):
    ev, xs, ys, res = ctx["ev"], ctx["xs"], ctx["ys"], ctx["res"]
    t = ev.tile
    for n in (1, t - 1, t, t + 1, len(xs)):
        _same(res, ev.run(xs[:n], ys[:n]), slice(0, n))
    lo = t + 8
    _same(res, ev.run(xs[lo:lo + t + 1], ys[lo:lo + t + 1]), slice(lo, lo + t + 1))
    _same(res, ev.run(xs, ys), totals=True)  # two identical calls: every output, totals included
    only = ev.run(xs)  # without labels: logits only
    assert only.loss is None and only.hit is None and only.totals is None
    assert torch.equal(_bits(only.logits), _bits(res.logits))
    empty = ev.run(xs[:0], ys[:0])
    before = ev.launches
    assert empty.n == 0 and empty.logits.shape == (0, 10) and ev.run(xs[:0]).n == 0 and ev.launches == before


def test_grid_wrap(ctx):
    """10,000 images in one call (more tiles than the grid holds on a partitioned GPU, and always with a capped
    grid) against ten calls of 1,000: the grid-stride loop changes nothing."""
    ev = ctx["ev"]
    g = torch.Generator().manual_seed(4)
    xs = torch.randint(0, 256, (10000, 28, 28), dtype=torch.uint8, generator=g).to(DEV)
    ys = torch.randint(0, 10, (10000,), dtype=torch.int64, generator=g).to(DEV)
    whole = ev.run(xs, ys)
    hits = 0.0
    for k in range(10):
        part = ev.run(xs[1000 * k:1000 * (k + 1)], ys[1000 * k:1000 * (k + 1)])
        _same(whole, part, slice(1000 * k, 1000 * (k + 1)))
        hits += float(part.totals[1])
    assert float(whole.totals[1]) == hits == float(whole.hit.sum())
    capped = persist_eval.MnistEvaluator(ctx["m"], max_workgroups=7)  # 313 tiles on 7 workgroups
    _same(whole, capped.run(xs, ys), totals=True)


def test_live_weights_after_a_perturbation():
    m, arena, ev, x = _make()
    xs = x.to(DEV)
    first = ev.run(xs).logits.clone()
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(2)
        arena.master.add_(torch.randn(arena.master.shape, device=DEV, generator=g) * 2e-3)
    arena.refresh_shadow()
    z = ev.run(xs).logits
    assert not torch.equal(z, first)
    ref, _, e32 = _refs(m, _snapshot(m), x)
    _check_logits(z, ref, e32)


def test_live_weights_after_persistent_training_steps():
    """Two steps of the persistent training engine, then the evaluator with no sync in between: stream order,
    and no stale copy of any weight."""
    from hops_examples_amd.ops import functional as HF

    m, arena, ev, x = _make()
    HF.seed_device_rng(11, DEV)
    opt = optim.Adadelta(m, lr=1.0)
    eng = persist.PersistentMnistStep(m, opt)
    g = torch.Generator().manual_seed(12)
    tx = torch.randint(0, 256, (2, 32, 28, 28, 1), dtype=torch.uint8, generator=g).to(DEV)
    ty = torch.randint(0, 10, (2, 32), dtype=torch.int64, generator=g).to(DEV)
    xs = x.to(DEV)
    before = _snapshot(m)
    eng.run_resident(tx, ty, 2)
    z = ev.run(xs).logits
    torch.cuda.synchronize()
    eng.check()
    P = _snapshot(m)
    assert not torch.equal(P["fc1.weight"], before["fc1.weight"])
    ref, _, e32 = _refs(m, P, x)
    _check_logits(z, ref, e32)


def test_label_guard(ctx):
    ev, xs, ys, res = ctx["ev"], ctx["xs"], ctx["ys"], ctx["res"]
    bad = ys.clone()
    i, j = 5, ev.tile + 3
    bad[i], bad[j] = -1, 10
    assert K.debug_errors() == []
    if os.environ.get("HOPSX_DEBUG", "0") == "1":  # the debug build raises at the launch (tests/test_debug_checks_gpu.py)
        with pytest.raises(RuntimeError, match="mnist_eval.hip"):
            ev.run(xs, bad)
        return
    r = ev.run(xs, bad)
    errs = K.debug_errors()
    assert errs and errs[0][0] == "mnist_eval" and errs[0][1] == 2, errs
    assert K.debug_errors() == []
    assert float(r.loss[i]) == 0.0 and float(r.loss[j]) == 0.0 and int(r.hit[i]) == 0 and int(r.hit[j]) == 0
    keep = torch.ones(len(xs), dtype=torch.bool, device=DEV)
    keep[i] = keep[j] = False
    assert torch.equal(_bits(r.logits), _bits(res.logits))
    assert torch.equal(_bits(r.loss[keep]), _bits(res.loss[keep])) and torch.equal(r.hit[keep], res.hit[keep])
    assert float(r.totals[1]) == float(r.hit.sum())


def test_graph_replay(ctx):
    ev, xs, ys = ctx["ev"], ctx["xs"], ctx["ys"]
    sx, sy = xs.clone(), ys.clone()
    res = ev.run(sx, sy)  # eager: allocates the outputs the capture reuses
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture.graph(g):
        assert ev.run(sx, sy, out=res) is res
    gen = torch.Generator().manual_seed(21)
    nx = torch.randint(0, 256, tuple(xs.shape), dtype=torch.uint8, generator=gen).to(DEV)
    ny = torch.randint(0, 10, tuple(ys.shape), dtype=torch.int64, generator=gen).to(DEV)
    sx.copy_(nx)
    sy.copy_(ny)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    _same(res, ev.run(nx, ny), totals=True)
    with pytest.raises(ValueError):
        ev.run(nx[:5], ny[:5], out=res)


# ------------------------------------------------------------------------------------------- keras
def _keras_model(keras):
    m = keras.Sequential([  # the stack of tests/test_keras_persist_gpu.py
        keras.layers.Conv2D(32, 2, activation="relu", input_shape=(28, 28, 1)),
        keras.layers.Conv2D(64, 2, activation="relu"),
        keras.layers.MaxPooling2D(),
        keras.layers.Dropout(0.01),
        keras.layers.Flatten(),
        keras.layers.Dense(128, activation="relu"),
        keras.layers.Dense(10, activation="softmax"),
    ])
    m.compile(optimizer=keras.optimizers.Adadelta(1.0), loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    return m


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 10, n)
    x = rng.integers(0, 60, (n, 28, 28, 1)).astype(np.uint8)
    for c in range(10):  # a learnable signal: a bright class-dependent stripe
        x[y == c, 2 * c + 3: 2 * c + 5, 4:24, 0] = 230
    return x, y.astype(np.int64)


def test_keras_evaluate_and_predict_take_the_evaluator(monkeypatch):
    from hops_examples_amd import keras

    torch.manual_seed(0)
    m = _keras_model(keras)
    x, y = _data(3 * 32 + 5)
    loss, acc = m.evaluate(x, y, verbose=0)
    ev = m._eval_engine
    assert ev.launches == 1
    r = ev.run(*m._eval_resident(x, y))
    tl, tc = (float(v) for v in r.totals.tolist())
    assert loss == tl / len(x) and acc == tc / len(x)
    d = m.evaluate(x, y, batch_size=1024, verbose=0, return_dict=True)
    assert d == {"loss": loss, "accuracy": acc} and ev.launches == 3
    p = m.predict(x[:, :, :, 0])  # (28, 28) images too
    assert ev.launches == 4 and p.shape == (len(x), 10) and p.dtype == np.float32
    assert float(np.abs(p.sum(1) - 1.0).max()) <= 1e-6
    assert np.array_equal(p.argmax(1), r.logits.argmax(1).cpu().numpy())
    # the existing path: same keys and shapes (and it launches nothing here)
    monkeypatch.setenv("HOPSX_EVAL_FUSED", "0")
    d0 = m.evaluate(x, y, verbose=0, return_dict=True)
    p0 = m.predict(x)
    assert ev.launches == 4 and list(d0) == list(d) and p0.shape == p.shape and p0.dtype == p.dtype
    print(f"fused {d} vs batch-by-batch {d0}; max |predict difference| {float(np.abs(p - p0).max()):.3e}")
    monkeypatch.delenv("HOPSX_EVAL_FUSED")
    # a float32 input does not take the evaluator
    m.evaluate(x.astype(np.float32) / 255.0, y, verbose=0)
    m.predict(x.astype(np.float32) / 255.0)
    assert ev.launches == 4


def test_keras_fit_validation_takes_the_evaluator():
    from hops_examples_amd import keras

    torch.manual_seed(0)
    m = _keras_model(keras)
    x, y = _data(4096)
    xv, yv = _data(256 + 7, seed=5)
    h = m.fit(x, y, batch_size=32, epochs=2, verbose=0, validation_data=(xv, yv), seed=3)
    ev = m._eval_engine  # (built by the first epoch's validation)
    assert ev.launches == 2
    assert len(h.history["val_loss"]) == 2 and len(h.history["val_accuracy"]) == 2
    # neither one-entry cache evicted the other
    assert m._eval_cache[0] is xv and (m._fast is None or m._res_cache[0][0] == id(x))
    loss, acc = m.evaluate(xv, yv, verbose=0)
    assert h.history["val_loss"][-1] == loss and h.history["val_accuracy"][-1] == acc
    # the stripes are trivially separable (tests/test_keras_persist_gpu.py reaches > 0.9 in two such epochs);
    # chance is 0.1: a validation pass that read the wrong weights or scaled the input wrongly stays there
    assert acc > 0.5, h.history


def test_keras_e1_stack_does_not_take_the_evaluator():
    from hops_examples_amd import keras

    torch.manual_seed(0)
    m = keras.Sequential([
        keras.layers.Conv2D(32, 4, activation="relu", input_shape=(28, 28, 1)),
        keras.layers.Conv2D(64, 4, activation="relu"),
        keras.layers.MaxPooling2D(4),
        keras.layers.Dropout(0.5),
        keras.layers.Flatten(),
        keras.layers.Dense(128, activation="relu"),
        keras.layers.Dropout(0.5),
        keras.layers.Dense(10, activation="softmax"),
    ])
    m.compile(optimizer="adam", loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    x, y = _data(64)
    out = m.evaluate(x, y, verbose=0)
    assert len(out) == 2 and m._evaluator(x) is None and getattr(m, "_eval_engine", None) is None
    assert m.predict(x).shape == (64, 10)
