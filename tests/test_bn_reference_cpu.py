"""The host references of the BatchNorm kernels (hops_examples_amd.ops.functional ``bn_stats_reference`` /
``bn_reference`` / ``bn_bwd_reference``) against fp64 ``torch.nn.functional.batch_norm`` and autograd: residual on
and off, all four activations, gamma / beta absent, M = 1, the running-statistics update (torch's uses the unbiased
variance; at M = 1 torch refuses training mode, so that case is anchored to the definition) and inference from
running statistics.  No GPU, no extension."""
import pytest
import torch
import torch.nn.functional as F

from hops_examples_amd.ops.functional import bn_bwd_reference, bn_reference, bn_stats_reference

f64 = torch.float64
EPS = 1e-5
EPS64 = float(torch.tensor(EPS, dtype=torch.float32))  # the kernels' eps is the fp32 value
ACT = {None: lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}
TOL = 1e-11


def _close(a, b, tol=TOL):
    assert a.dtype == f64 and a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


def _operands(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(torch.bfloat16)
    res = torch.randn(M, C, generator=g).to(torch.bfloat16)
    dy = torch.randn(M, C, generator=g).to(torch.bfloat16)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return x, res, dy, gamma, beta, rm, rv


@pytest.mark.parametrize("M,C", [(2, 3), (37, 8), (300, 5)])
def test_stats_reference(M, C):
    x = _operands(M, C, 1)[0]
    s, q, mean, var, unb = bn_stats_reference(x)
    xd = x.double()
    _close(s, xd.sum(0))
    _close(q, (xd * xd).sum(0))
    _close(mean, xd.mean(0))
    _close(var, xd.var(0, unbiased=False))
    _close(unb, xd.var(0, unbiased=True))
    s32 = bn_stats_reference(x, torch.float32)
    assert all(t.dtype == torch.float32 for t in s32)


def test_stats_reference_single_row():
    x = _operands(1, 6, 2)[0]
    s, q, mean, var, unb = bn_stats_reference(x)
    assert torch.equal(mean, x.double()[0]) and torch.equal(s, x.double()[0])
    assert float(var.abs().max()) == 0.0 and torch.equal(unb, var)


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("affine", ["gb", "g", "b", ""])
def test_forward_and_backward_against_torch(act, with_res, affine):
    M, C, mom = 53, 7, 0.1
    x, res, dy, gamma, beta, rm, rv = _operands(M, C, 3)
    gamma = gamma if "g" in affine else None
    beta = beta if "b" in affine else None
    xt = x.double().requires_grad_(True)
    rt = res.double().requires_grad_(True)
    gt = gamma.double().requires_grad_(True) if gamma is not None else None
    bt = beta.double().requires_grad_(True) if beta is not None else None
    rm_t, rv_t = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(xt, rm_t, rv_t, gt, bt, training=True, momentum=mom, eps=EPS64)
    yt = ACT[act](z + rt if with_res else z)
    yt.backward(dy.double())

    s, q, mean, var, unb = bn_stats_reference(x)
    rstd = 1.0 / torch.sqrt(var + EPS64)
    y = bn_reference(x, gamma, beta, mean, rstd, EPS, res if with_res else None, act)
    _close(y, yt.detach())
    # the running-statistics update the kernels make: (1 - m) old + m stat, the variance unbiased
    _close((1 - mom) * rm.double() + mom * mean, rm_t)
    _close((1 - mom) * rv.double() + mom * unb, rv_t)
    # act' from the stored output (here the unrounded one) and from the reference's own z
    for ysrc in ([y] if with_res else [y, None]):
        dz, s1, s2, dx = bn_bwd_reference(dy, x, ysrc, gamma, beta, mean, rstd, act)
        _close(dx, xt.grad, 1e-9)
        if with_res:
            _close(dz, rt.grad)
        if bt is not None:
            _close(s1, bt.grad, 1e-9)
        if gt is not None:
            _close(s2, gt.grad, 1e-9)
        _close(s1, dz.sum(0))


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
def test_act_grad_from_the_rounded_output(act):
    """With the bf16 y the derivative is the kernels' act_grad_from_out of THAT value, not the exact one."""
    M, C = 9, 4
    x, res, dy, gamma, beta, _, _ = _operands(M, C, 4)
    _, _, mean, var, _ = bn_stats_reference(x)
    rstd = 1.0 / torch.sqrt(var + EPS64)
    yb = bn_reference(x, gamma, beta, mean, rstd, EPS, res, act).to(torch.bfloat16)
    dz = bn_bwd_reference(dy, x, yb, gamma, beta, mean, rstd, act)[0]
    yd = yb.double()
    g = {None: torch.ones_like(yd), "relu": (yd > 0).double(), "sigmoid": yd * (1 - yd), "tanh": 1 - yd * yd}[act]
    assert torch.equal(dz, dy.double() * g)


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
def test_single_row(act):
    """M = 1: var = 0, xhat = 0, y = act(beta + res); dx = 0 exactly (dz - sum_dz / 1 - 0)."""
    x, res, dy, gamma, beta, rm, rv = _operands(1, 5, 5)
    _, _, mean, var, unb = bn_stats_reference(x)
    rstd = 1.0 / torch.sqrt(var + EPS64)
    y = bn_reference(x, gamma, beta, mean, rstd, EPS, res, act)
    _close(y, ACT[act](beta.double() + res.double()))
    dz, s1, s2, dx = bn_bwd_reference(dy, x, y, gamma, beta, mean, rstd, act)
    assert float(dx.abs().max()) == 0.0 and float(s2.abs().max()) == 0.0 and torch.equal(s1, dz[0])


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("with_res", [False, True])
def test_inference_from_running_statistics(act, with_res):
    x, res, _, gamma, beta, rm, rv = _operands(21, 6, 6)
    rv[2] = 0.0  # rsqrt(eps)
    want = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=False,
                        eps=EPS64)
    want = ACT[act](want + res.double() if with_res else want)
    got = bn_reference(x, gamma, beta, rm, rv, EPS, res if with_res else None, act, var_mode=True)
    _close(got, want, 1e-10)
    assert bn_reference(x, gamma, beta, rm, rv, EPS, None, act, var_mode=True, dtype=torch.float32).dtype \
        == torch.float32
