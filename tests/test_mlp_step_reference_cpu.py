"""runtime/mlp_step.py on the CPU: ``reference_steps`` (the fp64 statement of the one-launch Dense-stack step) against
torch autograd + ``optim.reference_step``, and what ``dense_layers`` / ``supported`` accept and refuse."""
import pytest
import torch

from hops_examples_amd import nn as hnn
from hops_examples_amd import optim
from hops_examples_amd.models import zoo
from hops_examples_amd.runtime import mlp_step as M
from hops_examples_amd.runtime.arena import ParamArena

TITANIC = ((6, 64, 64, 32, 32, 2, 1), ("relu", "relu", "relu", "relu", "sigmoid", None), "bce_logits", "adam")
SMALL = ((2, 8, 1), ("relu", None), "mse", "adamw")


@pytest.mark.parametrize("dims,acts,loss_kind,kind", [TITANIC, SMALL], ids=["titanic", "2-8-1-mse"])
def test_reference_steps_match_autograd(dims, acts, loss_kind, kind):
    gen = torch.Generator().manual_seed(3)
    L, B, nb = len(dims) - 1, 5, 2
    W = [torch.randn(dims[l + 1], dims[l], generator=gen, dtype=torch.float64) * 0.3 for l in range(L)]
    Bs = [torch.randn(dims[l + 1], generator=gen, dtype=torch.float64) * 0.3 for l in range(L)]
    xs = torch.randn(nb, B, dims[0], generator=gen, dtype=torch.float64)
    ys = (torch.rand(nb, B, 1, generator=gen, dtype=torch.float64) > 0.5).double()
    hp = [1e-2, 1.0, 0.01 if kind == "adamw" else 0.0, 0.9, 0.999, 1e-7]
    got = M.reference_steps(W, Bs, acts, xs, ys, loss_kind, kind, hp, 3, cursor=1)
    p = [t.clone().requires_grad_() for t in W + Bs]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    for s in range(3):
        h = xs[(1 + s) % nb]
        for l in range(L):
            h = h @ p[l].T + p[L + l]
            h = torch.relu(h) if acts[l] == "relu" else torch.sigmoid(h) if acts[l] == "sigmoid" else h
        y = ys[(1 + s) % nb]
        loss = (torch.nn.functional.mse_loss(h, y) if loss_kind == "mse"
                else torch.nn.functional.binary_cross_entropy_with_logits(h, y))
        grads = torch.autograd.grad(loss, p)
        torch.testing.assert_close(got["loss"][s], loss.detach(), rtol=1e-12, atol=0)
        for j in range(2 * L):
            pn, (m[j], v[j]) = optim.reference_step(kind, p[j], grads[j], [m[j], v[j]], hp, s + 1)
            p[j] = pn.requires_grad_()
    # rtol = 1e-12 (fp64 round-off) on the weights; a moment is a cancelling sum over the batch, good only to the
    # round-off of its terms under another summation order: m and v get an absolute floor of 1e-12 of their largest entry
    def close(a, b, floor=0.0):
        torch.testing.assert_close(a, b.detach(), rtol=1e-12, atol=floor * b.detach().abs().max().item())

    for j, (a, b) in enumerate(zip(got["weights"] + got["biases"], p)):
        close(a, b)
        close(got["m"][j], m[j], 1e-12)
        close(got["v"][j], v[j], 1e-12)
    # the bf16 option rounds where the kernel does; what it returns for the trace checks is self-consistent
    bf = M.reference_steps(W, Bs, acts, xs, ys, loss_kind, kind, hp, 1, emulate_bf16=True)
    rep = lambda t: torch.equal(t, t.float().bfloat16().double())  # noqa: E731
    assert all(rep(t) for t in bf["A"] + bf["G"]) and not rep(got["A"][-1] if L > 1 else got["z"])
    assert torch.equal(bf["z"], bf["A"][-1] @ W[-1].float().bfloat16().double()[0] + Bs[-1][0])
    for l in range(L - 1):
        assert torch.equal(bf["dW"][l], bf["G"][l].T @ bf["A"][l]) and torch.equal(bf["db"][l], bf["G"][l].sum(0))
    assert torch.equal(bf["dW"][-1][0], (bf["g"][:, None] * bf["A"][-1]).sum(0)) and torch.equal(bf["db"][-1][0], bf["g"].sum())


def _built(model):
    model.build()
    ParamArena.from_module(model)
    return model


@pytest.mark.parametrize("builder,loss_kind", [(zoo.simulated_mlp, "bce_logits"), (zoo.titanic_dnn, "bce_logits"),
                                               (zoo.maggy_regressor, "mse")])
def test_zoo_builders_accepted(builder, loss_kind):
    m = _built(builder())
    assert M.dense_layers(m, loss_kind) is not None
    assert M.supported(m, optim.Adam(m), loss_kind, 10, 1)


def _stack(dims, drop=False):
    mods = [hnn.Linear(a, b, activation="relu" if i + 2 < len(dims) else None)
            for i, (a, b) in enumerate(zip(dims, dims[1:]))]
    if drop:
        mods.insert(1, hnn.Dropout(0.5))
    net = torch.nn.Sequential(*mods)
    ParamArena.from_module(net)
    return net


@pytest.mark.parametrize("dims,B,opt,world,drop", [
    ((6, 65, 1), 10, "adam", 1, False), ((4,) * 9 + (1,), 10, "adam", 1, False), ((6, 8, 1), 65, "adam", 1, False),
    ((6, 8, 2), 10, "adam", 1, False), ((6, 8, 1), 10, "adam", 1, True), ((6, 8, 1), 10, "sgd", 1, False),
    ((6, 8, 1), 10, "adam", 2, False)], ids=["width65", "9layers", "B65", "last2", "dropout", "sgd", "world2"])
def test_refused(dims, B, opt, world, drop):
    net = _stack(dims, drop)
    assert not M.supported(net, optim.get(opt, net), "bce_logits", B, world)
    ok = _stack((6, 8, 1))  # (the control: the same family inside the limits is taken)
    assert M.supported(ok, optim.Adam(ok), "bce_logits", 10, 1)
