"""hops_examples_amd.ops.functional.gemm_reference / linear_bwd_reference (the fp64 statements that
tests/test_gemm_paths_gpu.py holds the dense GEMM kernels to) against fp64 torch autograd of ``act(x w^T + b)``, the
masked operand's single bf16 rounding point, every layout, and the pooled form against autograd through max_pool2d.
The route reporters' host logic runs through the built extension, nothing is launched.  No GPU."""
import os

import pytest
import torch
import torch.nn.functional as F

from hops_examples_amd.ops.functional import (dense_reference, dropout_keep_reference, gemm_reference,
                                              linear_bwd_reference, pool_reference)

bf, f64 = torch.bfloat16, torch.float64
LATCHED = ("HOPSX_GEMM_T64_MIN", "HOPSX_GEMM_T128_MIN", "HOPSX_GEMM_SPLIT_CFG", "HOPSX_GEMM_SPLIT_TARGET",
           "HOPSX_SPLIT_MINKT")
ACTS = {None: lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def _ops(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g).to(bf), torch.randn(N, K, generator=g).to(bf), torch.randn(N, generator=g),
            torch.randn(M, N, generator=g).to(bf))


@pytest.mark.parametrize("act", [None, "relu", "sigmoid", "tanh"])
def test_forward_and_backward_against_autograd(act):
    M, N, K = 7, 5, 13
    x, w, b, dy = _ops(M, N, K, 1)
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    y = ACTS[act](xd @ wd.t() + bd)
    out, cs, rs = gemm_reference(x, w, True, True, "store", bias=b, act=act)
    assert torch.equal(out, y.detach())
    assert torch.equal(out, dense_reference(x, w, b, act))
    assert torch.allclose(cs, y.detach().sum(0), rtol=0, atol=1e-13)
    assert torch.allclose(rs, x.double().sum(1), rtol=0, atol=1e-13)
    # backward with the UNROUNDED mask (relu's is exact in bf16; the others: no mask in the operand, act' applied to
    # the fp64 upstream gradient instead, which is what autograd does)
    up = dy.double()
    gx, gw, gb = torch.autograd.grad(y, (xd, wd, bd), up)
    if act in (None, "relu"):
        dx, dw, db = linear_bwd_reference(dy, w, x, y=y.detach().to(bf) if act else None, act=act)
        # (bf16(y) > 0 <=> y > 0 unless y underflows bf16: not at these magnitudes)
    else:
        gpre = up * {"sigmoid": lambda v: v * (1 - v), "tanh": lambda v: 1 - v * v}[act](y.detach())
        dx, dw, db = linear_bwd_reference(gpre, w, x)  # (fp64 operand: nothing is rounded)
    for got, want in ((dx, gx), (dw, gw), (db, gb)):
        assert torch.allclose(got, want, rtol=0, atol=1e-12), (got - want).abs().max()


def test_dact_epilogue_is_the_previous_layers_mask():
    M, N, K = 6, 4, 9
    x, w, b, dy = _ops(M, N, K, 2)
    for act in ("relu", "sigmoid", "tanh"):
        h = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).double().requires_grad_()
        yprev = ACTS[act](h)
        out = (yprev @ w.double().t()) * dy.double()
        (gh,) = torch.autograd.grad(out.sum(), h)
        dx, _, _ = linear_bwd_reference(dy, w, x, yprev=yprev.detach(), act_prev=act)
        assert torch.allclose(dx, gh, rtol=0, atol=1e-12)


def test_masked_operand_has_one_rounding_point():
    """A = bf16(a * act'(y)): a = 1 + 2^-7 (exact in bf16) times sigmoid' = 0.25 * (1 - 2^-14)-ish is not; the
    reference must use the rounded product, in both layouts, in the row sums too."""
    a = torch.tensor([[1.0078125, -3.0], [2.5, 0.3125]]).to(bf)
    y = torch.tensor([[0.3125, 0.75], [0.4375, 0.9375]]).to(bf)
    b = torch.tensor([[3.0, 5.0]]).to(bf)
    prod = a.double() * (y.double() * (1 - y.double()))
    rounded = prod.to(bf).double()
    assert not torch.equal(prod, rounded)  # the case does distinguish the two
    out, _, rs = gemm_reference(a, b, True, True, "atomic", a_mask_y=y, a_mask_act="sigmoid")
    assert torch.equal(out, rounded @ b.double().t())
    assert torch.equal(rs, rounded.sum(1))
    out_t, _, rs_t = gemm_reference(a.t().contiguous(), b.t().contiguous(), False, False, "atomic",
                                    a_mask_y=y.t().contiguous(), a_mask_act=2)
    assert torch.equal(out_t, out) and torch.equal(rs_t, rs)
    # relu: a 0 / 1 mask, no rounding at all
    out_r, _, _ = gemm_reference(a, b, True, True, "atomic", a_mask_y=y - 0.5, a_mask_act="relu")
    assert torch.equal(out_r, (a.double() * ((y - 0.5) > 0)) @ b.double().t())


def test_layouts_alpha_beta_and_epilogues():
    M, N, K = 5, 3, 11
    x, w, b, old = _ops(M, N, K, 4)
    old = old.float()
    want = x.double() @ w.double().t()
    for a_kc in (True, False):
        for b_kc in (True, False):
            a_ = x if a_kc else x.t().contiguous()
            b_ = w if b_kc else w.t().contiguous()
            out, cs, rs = gemm_reference(a_, b_, a_kc, b_kc, "store", alpha=0.5, bias=b, act="relu", beta=2.0, old=old)
            full = torch.relu(0.5 * want + b.double()) + 2.0 * old.double()
            assert torch.equal(out, full) and torch.allclose(cs, full.sum(0), atol=1e-13, rtol=0)
            out, cs, _ = gemm_reference(a_, b_, a_kc, b_kc, "atomic", alpha=-2.0, old=old)
            assert torch.equal(out, old.double() - 2.0 * want)
            assert torch.allclose(cs, (-2.0 * want).sum(0), atol=1e-13, rtol=0)  # the increment, not the total
            aux = torch.sigmoid(old).to(bf)
            out, _, _ = gemm_reference(a_, b_, a_kc, b_kc, "dact", act="sigmoid", aux=aux)
            assert torch.equal(out, want * (aux.double() * (1 - aux.double())))
    out, _, _ = gemm_reference(x[:, :0], w[:, :0], bias=b, act="tanh")  # K = 0: act(bias)
    assert torch.equal(out, torch.tanh(b.double()).expand(M, N))


@pytest.mark.parametrize("k,H,W,premask,p", [((2, 2), 5, 4, True, 0.0), ((3, 2), 7, 5, False, 0.0),
                                             ((2, 2), 4, 5, True, 0.25)])
def test_pooled_backward_against_autograd(k, H, W, premask, p):
    B, C, N = 3, 2, 4
    PH, PW = H // k[0], W // k[1]
    K = PH * PW * C
    g = torch.Generator().manual_seed(H * 10 + W)
    z = torch.randn(B, H, W, C, generator=g).to(bf)  # (distinct with probability ~1: no argmax ties)
    w = torch.randn(N, K, generator=g).to(bf)
    dy = torch.randn(B, N, generator=g).to(bf)
    rng, salt = torch.tensor([12345, 7], dtype=torch.int64), 3
    zd = z.double().requires_grad_()
    pin = torch.relu(zd) if premask else zd
    pooled = F.max_pool2d(pin.permute(0, 3, 1, 2), k, k).permute(0, 2, 3, 1)  # NHWC again, floor windows
    keep = dropout_keep_reference(rng, salt, (B, PH, PW, C), p) if p > 0 else torch.ones(B, PH, PW, C, dtype=torch.bool)
    scale = float(1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))
    x = pooled * keep * scale
    out = x.reshape(B, K) @ w.double().t()
    (gz,) = torch.autograd.grad(out, zd, dy.double())
    _, am = pool_reference(torch.relu(z.double()) if premask else z.double(), k, k, 0)
    xb = x.detach().reshape(B, K)
    dx, dw, db = linear_bwd_reference(dy, w, xb, pool=(am, premask, (B, H, W, C), k, "relu", rng, salt, p))
    assert dx.shape == (B, H, W, C)
    assert torch.allclose(dx, gz, rtol=0, atol=1e-12), (dx - gz).abs().max()
    assert torch.equal(dx[:, PH * k[0]:], torch.zeros_like(dx[:, PH * k[0]:]))  # floor remainder rows
    assert torch.allclose(dw, dy.double().t() @ xb, rtol=0, atol=1e-12)
    assert torch.equal(db, dy.double().sum(0))


# ------------------------------------------------------- the route reporters' host logic (no launch, no device)
def _ext():
    from hops_examples_amd.ops import _C
    return _C.ext()


def test_gemm_path_host_logic(monkeypatch):
    """gemm.hip gemm_route through the raw extension with made-up (never dereferenced) addresses."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    if os.environ.get("HOPSX_DETERMINISTIC", "") == "1" or any(k in os.environ for k in LATCHED):
        pytest.skip("default-knob expectations")
    e = _ext()
    path = lambda M, N, K, epi, ws=0, tickets=0, a=16, lda=8, ay=0: e.gemm_path(a, lda, 16, 8, M, N, K, epi, 16 if ws else 0, ws, ay, tickets)  # noqa: E731
    assert path(7, 5, 0, 0) == [0, 32, 1, 64, 1, 1, 1, 0]                    # K = 0: one slice, the epilogue alone
    assert path(1409, 1409, 40, 0)[:5] == [0, 64, 1, 64, 529]
    assert path(2049, 2049, 72, 0)[:5] == [0, 128, 1, 128, 289]
    assert path(32, 128, 1024, 0, ws=4096, tickets=16)[:5] == [2, 32, 4, 256, 4]
    assert path(32, 128, 1024, 0, ws=4096)[0] == 3                           # no ticket counters: the finish route
    assert path(32, 128, 1024, 0, ws=4095, tickets=16)[:3] == [0, 32, 1]     # one element short: direct
    assert path(32, 128, 1024, 2, ws=4096, tickets=16)[:3] == [1, 32, 4]     # atomic epilogue: no workspace route
    assert path(0, 5, 2048, 1, ws=64, tickets=16)[:5] == [0, 32, 1, 64, 0]   # nothing to launch, nothing divided
    assert path(20, 70, 513, 2)[:5] == [1, 32, 3, 192, 3]
    assert path(8, 8, 8, 0, a=18)[5:7] == [0, 1] and path(8, 8, 8, 0, lda=9)[5] == 0
    assert path(8, 8, 8, 0, ay=18)[5] == 0 and path(8, 8, 8, 0, ay=32)[5] == 1
    for env, route in (("splitk", 0), ("splitk_ticket", 3), ("conv_splitk", 2), ("pool8,splitk_ticket", 3),
                       ("splitk_ticket,splitk", 0), ("splitk_tickets", 2), ("xsplitk", 2), ("", 2)):
        monkeypatch.setenv("HOPSX_DISABLE", env)  # whole comma-separated tokens, read on every call
        assert path(32, 128, 1024, 0, ws=4096, tickets=16)[0] == route, env


def test_linear_bwd_pair_path_host_logic(monkeypatch):
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    if os.environ.get("HOPSX_DETERMINISTIC", "") == "1" or any(k in os.environ for k in LATCHED):
        pytest.skip("default-knob expectations")
    e = _ext()
    assert e.linear_bwd_pair_path(33, 10, 20, [], 1) == [0, 32, 32, 1, 1, 1, 0, 2, 1]
    assert e.linear_bwd_pair_path(300, 50, 77, [], 1) == [0, 32, 32, 1, 2, 0, 0, 30, 6]   # a split wgrad: atomics
    assert e.linear_bwd_pair_path(32, 1024, 128, [], 0)[0] == -2                           # split-K dgrad: separate
    assert e.linear_bwd_pair_path(0, 10, 20, [], 0)[0] == -2
    ok = [5, 2, 2, 2, 2, 0, 5, 4]
    assert e.linear_bwd_pair_path(8, 10, 20, ok, 0)[:7] == [0, 32, 32, 1, 1, 0, 1]
    for H, W in ((6, 4), (3, 4), (5, 6), (5, 3)):  # not the floor windows of H x W
        assert e.linear_bwd_pair_path(8, 10, 20, ok[:6] + [H, W], 0)[0] == -3
    assert e.linear_bwd_pair_path(8, 10, 20, [4] + ok[1:], 0)[0] == -2                      # C PH PW != K
    for env, want in (("bwd_pair", [-2, 0]), ("bwd_pair_gemm", [0, 1]), ("dw_store", [0, 0])):
        monkeypatch.setenv("HOPSX_DISABLE", env)
        v = e.linear_bwd_pair_path(33, 10, 20, [], 1)
        assert [v[0], v[5]] == want, env
