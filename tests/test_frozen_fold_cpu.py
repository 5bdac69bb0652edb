"""Frozen ResNet inference, CPU side: the conv + BN fold, the fp64 reference anchored to the model itself, and
the cases in which the engine declines."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hops_examples_amd import inference
from hops_examples_amd.models.mnist import MirroredMnistCNN
from hops_examples_amd.models.resnet import ResNet50, cifar_resnet
from hops_examples_amd.runtime.frozen import FrozenResNet, fold_conv_bn, reference_forward


def randomize_bn(model, seed):
    """Per-channel BN state from a seeded generator: gamma in [0.5, 1.5], beta and the running mean in
    [-0.5, 0.5], the running variance in [0.5, 2].  With the defaults (1 / 0 / 0 / 1) a swapped mean / var or
    a dropped eps would be invisible."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "running_var"):
                n = m.weight.numel()
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(torch.rand(n, generator=g) - 0.5)
                m.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
                m.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
    return model


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2)])
def test_fold_matches_conv_then_bn(k, stride):
    g = torch.Generator().manual_seed(5)
    ci, co = 6, 10
    x = torch.randn(2, ci, 9, 9, generator=g, dtype=torch.float64)
    w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64)
    gamma = 0.5 + torch.rand(co, generator=g, dtype=torch.float64)
    beta = torch.rand(co, generator=g, dtype=torch.float64) - 0.5
    rmean = torch.rand(co, generator=g, dtype=torch.float64) - 0.5
    rvar = 0.5 + 1.5 * torch.rand(co, generator=g, dtype=torch.float64)
    eps = 1e-3  # large enough that dropping it would show
    want = F.batch_norm(F.conv2d(x, w, None, stride, k // 2), rmean, rvar, gamma, beta, False, 0.1, eps)
    wf, bf = fold_conv_bn(w, gamma, beta, rmean, rvar, eps)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    got = F.conv2d(x, wf, bf, stride, k // 2)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["resnet20", "resnet50_1111"])
def test_reference_matches_the_model(name):
    torch.manual_seed(3)
    if name == "resnet20":
        model, hw = cifar_resnet(20), 32
    else:
        model, hw = ResNet50(10, layers=(1, 1, 1, 1)), 64
    model = randomize_bn(model, 11).double().eval()
    x = torch.randint(0, 256, (2, hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = model(x)
    assert want.dtype == torch.float64
    got = reference_forward(model, x, dtype=torch.float64, emulate_bf16=False)
    rel = (got - want).abs().max() / want.abs().max()
    assert rel < 1e-9, rel
    # and the bf16 emulation moves it (so the flag does something) but not far
    emu = reference_forward(model, x, dtype=torch.float64, emulate_bf16=True)
    rel_emu = (emu - want).abs().max() / want.abs().max()
    assert 0 < rel_emu < 0.1, rel_emu


def test_declines_on_cpu_and_other_models():
    assert not FrozenResNet.supported(cifar_resnet(20))  # on the CPU
    assert not FrozenResNet.supported(MirroredMnistCNN())
    with pytest.raises(ValueError):
        FrozenResNet.freeze(cifar_resnet(20))


def test_cpu_predictor_is_unchanged():
    torch.manual_seed(0)
    model = randomize_bn(cifar_resnet(20), 11).eval()
    x = np.random.RandomState(1).randint(0, 256, (3, 32, 32, 3)).astype(np.uint8)
    pr = inference.Predictor(model, "cpu")
    assert pr.frozen is None
    got = np.concatenate(list(pr.predict_batches([x])))
    with torch.no_grad():
        want = torch.softmax(model(torch.from_numpy(x)).float(), dim=-1).numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(inference.predict(model, x, device="cpu", frozen=False), want)
    with pytest.raises(ValueError):
        inference.Predictor(model, "cpu", frozen=True)
