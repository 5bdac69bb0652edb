"""CPU side of the one-launch flagship evaluator (runtime/persist_eval.py): the fp64 reference forward agrees
with the training reference's loss, the evaluator declines a CPU model, and keras evaluate / predict on the
CPU are the plain forward they always were."""
import numpy as np
import torch

from hops_examples_amd.models.mnist import MirroredMnistCNN
from hops_examples_amd.runtime import persist, persist_eval


def _params(m):
    named = dict(m.named_parameters())
    return {k: named[k].detach().double().clone() for k in persist.PersistentMnistStep.PARAMS}


def test_reference_logits_is_the_forward_of_reference_grads():
    torch.manual_seed(3)
    m = MirroredMnistCNN()
    P = _params(m)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (8, 28, 28, 1), dtype=torch.uint8, generator=g)
    y = torch.randint(0, 10, (8,), dtype=torch.int64, generator=g)
    scale, shift = m.conv1.in_affine
    kw = dict(xscale=float(scale), xshift=float(shift))
    z = persist_eval.reference_logits(P, x, emulate_bf16=False, **kw)
    assert z.shape == (8, 10) and z.dtype == torch.float64
    ce = float(torch.nn.functional.cross_entropy(z, y, reduction="sum"))
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    _, ref = persist.reference_grads(Pg, x, y, 0, 0, 0, 0.0, emulate_bf16=False, **kw)
    assert abs(ce - ref) <= 1e-12 * abs(ref), (ce, ref)
    # the same rounding points as the training reference when bf16 is emulated
    zb = persist_eval.reference_logits(P, x, emulate_bf16=True, **kw)
    _, refb = persist.reference_grads(Pg, x, y, 0, 0, 0, 0.0, emulate_bf16=True, **kw)
    ceb = float(torch.nn.functional.cross_entropy(zb, y, reduction="sum"))
    assert abs(ceb - refb) <= 1e-12 * abs(refb), (ceb, refb)
    # and the fp32 proxy is the same function in fp32
    z32 = persist_eval.reference_logits(P, x, dtype=torch.float32, **kw)
    assert z32.dtype == torch.float32 and float((z32.double() - zb).abs().max()) < 1e-3


def test_evaluator_declines_a_cpu_model():
    m = MirroredMnistCNN()
    assert persist.flagship_layers(m) is not None
    assert persist_eval.MnistEvaluator.supported(m) is False


def test_keras_evaluate_and_predict_on_the_cpu_are_the_plain_forward(monkeypatch):
    from hops_examples_amd import keras

    monkeypatch.setattr(keras, "_default_device", lambda: torch.device("cpu"))
    torch.manual_seed(0)
    m = keras.Sequential([
        keras.layers.Conv2D(32, 2, activation="relu", input_shape=(28, 28, 1)),
        keras.layers.Conv2D(64, 2, activation="relu"),
        keras.layers.MaxPooling2D(),
        keras.layers.Dropout(0.01),
        keras.layers.Flatten(),
        keras.layers.Dense(128, activation="relu"),
        keras.layers.Dense(10, activation="softmax"),
    ])
    m.compile(optimizer=keras.optimizers.Adadelta(1.0), loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (40, 28, 28, 1)).astype(np.uint8)
    y = rng.integers(0, 10, 40).astype(np.int64)
    m.build()  # (so that the eval() at the top of predict / evaluate reaches the layers)
    pr = m.predict(x, batch_size=16)
    assert pr.shape == (40, 10)
    loss, acc = m.evaluate(x, y, batch_size=16, verbose=0)
    assert m.device.type == "cpu" and m._evaluator(x) is None and getattr(m, "_eval_engine", None) is None
    with torch.no_grad():
        m.eval()
        direct = m.forward(torch.from_numpy(x)).float()
    assert np.allclose(pr, direct.numpy(), rtol=0, atol=1e-6)
    ce = float(torch.nn.functional.nll_loss(torch.log(direct.double()), torch.from_numpy(y)))
    assert abs(loss - ce) < 1e-5 * max(1.0, abs(ce)), (loss, ce)
    assert abs(acc - float((direct.argmax(-1).numpy() == y).mean())) < 1e-12
