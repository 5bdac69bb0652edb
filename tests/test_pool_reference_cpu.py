"""The host references of the pooling kernels (hops_examples_amd.ops.functional ``pool_reference`` /
``pool_bwd_reference`` / ``gap_reference`` / ``gap_bwd_reference`` / ``dropout_keep_reference``) against fp64
``torch.nn.functional.max_pool2d(..., return_indices=True)``, autograd and ``x.mean``: the window geometries of
tests/test_pool_paths_gpu.py, ties, padded borders, stride larger than the window, the translation between
torch's flat input index and the kernels' tap index, and the column-sum increment.  No GPU, no extension."""
import math

import pytest
import torch
import torch.nn.functional as F

from hops_examples_amd.ops.functional import (dropout_keep_reference, gap_bwd_reference, gap_reference,
                                              pool_bwd_reference, pool_reference)
from hops_examples_amd.runtime.persist import dropout_keep

f64 = torch.float64

# (H, W, k, s, p): the geometries of the GPU suite
GEOMS = [
    (7, 10, (2, 2), (2, 2), (0, 0)), (9, 9, (2, 2), (2, 2), (0, 0)), (8, 6, (2, 2), (2, 2), (0, 0)),
    (10, 11, (3, 3), (3, 3), (0, 0)), (9, 10, (2, 3), (2, 3), (0, 0)), (2, 2, (2, 2), (2, 2), (0, 0)),
    (22, 23, (4, 4), (4, 4), (0, 0)),
    (7, 10, (3, 3), (2, 2), (1, 1)), (15, 9, (3, 3), (2, 2), (1, 1)), (7, 10, (3, 3), (1, 1), (1, 1)),
    (15, 9, (2, 2), (1, 1), (0, 0)), (7, 10, (3, 3), (3, 3), (1, 1)), (15, 9, (3, 2), (2, 1), (1, 0)),
    (7, 10, (5, 5), (2, 2), (2, 2)), (8, 9, (7, 7), (1, 1), (3, 3)), (7, 10, (2, 2), (3, 3), (0, 0)),
    (15, 9, (2, 2), (3, 3), (0, 0)), (16, 17, (16, 16), (16, 16), (0, 0)),
]
IDS = [f"{h}x{w}-k{k[0]}x{k[1]}-s{s[0]}x{s[1]}-p{p[0]}x{p[1]}" for h, w, k, s, p in GEOMS]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def torch_pool(x, k, s, p):
    """fp64 torch on NHWC x: (y, tap index translated from torch's flat index ih * W + iw of the plane)."""
    B, H, W, C = x.shape
    y, idx = F.max_pool2d(_nchw(x.to(f64)), k, s, p, return_indices=True)
    y, idx = _nhwc(y), _nhwc(idx)
    OH, OW = y.shape[1], y.shape[2]
    ih, iw = idx // W, idx % W
    oh = torch.arange(OH).view(1, OH, 1, 1)
    ow = torch.arange(OW).view(1, 1, OW, 1)
    kh, kw = ih - (oh * s[0] - p[0]), iw - (ow * s[1] - p[1])
    assert bool(((kh >= 0) & (kh < k[0]) & (kw >= 0) & (kw < k[1])).all())
    return y, (kh * k[1] + kw).to(torch.uint8)


def brute(x, k, s, p):
    """The rule spelled out one output at a time (python loops; tiny shapes only)."""
    B, H, W, C = x.shape
    OH, OW = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
    y = torch.empty(B, OH, OW, C, dtype=f64)
    am = torch.empty(B, OH, OW, C, dtype=torch.uint8)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(C):
                    best, bi = None, 0
                    for kh in range(k[0]):
                        for kw in range(k[1]):
                            ih, iw = oh * s[0] - p[0] + kh, ow * s[1] - p[1] + kw
                            if 0 <= ih < H and 0 <= iw < W:
                                v = float(x[b, ih, iw, c])
                                if best is None or v > best:
                                    best, bi = v, kh * k[1] + kw
                    y[b, oh, ow, c], am[b, oh, ow, c] = best, bi
    return y, am


@pytest.mark.parametrize("H,W,k,s,p", GEOMS, ids=IDS)
def test_forward_matches_torch(H, W, k, s, p):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 3, generator=g).to(torch.bfloat16)
    y, am = pool_reference(x, k, s, p)
    yt, amt = torch_pool(x, k, s, p)
    assert y.dtype == f64 and am.dtype == torch.uint8 and y.shape == yt.shape
    assert torch.equal(y, yt) and torch.equal(am, amt)
    if k == (16, 16):
        x[0, 15, 15, 1] = 100.0  # the last tap of the 256
        assert int(pool_reference(x, k, s, p)[1][0, 0, 0, 1]) == 255


@pytest.mark.parametrize("H,W,k,s,p", [g for g in GEOMS if g[0] * g[1] <= 150], ids=lambda v: str(v))
def test_ties_take_the_first_tap_in_kh_major_order(H, W, k, s, p):
    """Values from {-1, 0, 1}: nearly every window has a tied maximum; padded taps never count."""
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-1, 2, (1, H, W, 2), generator=g).to(torch.bfloat16)
    y, am = pool_reference(x, k, s, p)
    yb, amb = brute(x, k, s, p)
    assert torch.equal(y, yb) and torch.equal(am, amb)
    yt, amt = torch_pool(x, k, s, p)
    assert torch.equal(y, yt) and torch.equal(am, amt)
    xc = torch.full((1, H, W, 2), 0.5).to(torch.bfloat16)  # constant: always the first IN-BOUNDS tap
    amc = pool_reference(xc, k, s, p)[1]
    assert torch.equal(amc, brute(xc, k, s, p)[1])
    if p != (0, 0):
        assert int(amc[0, 0, 0, 0]) == p[0] * k[1] + p[1]  # the corner window's first row and column are padding
    else:
        assert int(amc.max()) == 0


def test_infinities():
    x = torch.randn(1, 4, 6, 2).to(torch.bfloat16)
    x[0, 0:2, 0:2, 0] = float("-inf")
    x[0, 2, 3, 1] = float("inf")
    y, am = pool_reference(x, (2, 2), (2, 2), (0, 0))
    assert y[0, 0, 0, 0] == float("-inf") and am[0, 0, 0, 0] == 0
    assert y[0, 1, 1, 1] == float("inf") and am[0, 1, 1, 1] == 1


ACTS = {None: lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


@pytest.mark.parametrize("drop", (False, True))
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("H,W,k,s,p", GEOMS, ids=IDS)
def test_backward_matches_autograd(H, W, k, s, p, act, drop):
    """z -> x = act(z) -> max-pool -> x mask / (1 - p) against dy: d/dz is the reference's dx (act' written
    through x), its per-channel sum the column-sum increment; the argmax comes from the reference forward."""
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + len(str(act)))
    B, C = 2, 3
    z = torch.randn(B, H, W, C, generator=g, dtype=f64).requires_grad_()
    x = ACTS[act](z)
    y = _nhwc(F.max_pool2d(_nchw(x), k, s, p))
    dy = torch.randn(y.shape, generator=g, dtype=f64)
    drop_p = 0.3
    mask = dropout_keep_reference((12345, 6), 99, y.shape, drop_p) if drop else None
    out = y
    if drop:
        scale = (1.0 / (1.0 - torch.tensor(drop_p, dtype=torch.float32))).double()
        out = y * mask.double() * scale
    out.backward(dy)
    am = pool_reference(x.detach(), k, s, p)[1]
    dx, cs = pool_bwd_reference(dy, am, z.shape, k, s, p, x=x.detach(), act=act, mask=mask, drop_p=drop_p)
    assert dx.dtype == f64 and dx.shape == z.shape and cs.shape == (C,)
    tol = 1e-12 * max(1.0, float(dy.abs().max())) * math.prod(-(-a // b) for a, b in zip(k, s))
    assert float((dx - z.grad).abs().max()) <= tol
    assert float((cs - z.grad.sum((0, 1, 2))).abs().max()) <= tol * B * H * W
    # pixels no window covers: exactly zero
    OH, OW = y.shape[1], y.shape[2]
    cover = F.conv_transpose2d(torch.ones(1, 1, OH, OW, dtype=f64), torch.ones(1, 1, *k, dtype=f64), stride=s)[0, 0]
    cover = F.pad(cover, (0, W + p[1], 0, H + p[0]))[p[0]:p[0] + H, p[1]:p[1] + W]  # (the floor remainder: zero)
    assert cover.shape == (H, W) and torch.count_nonzero(dx[:, cover == 0]) == 0
    if p == (0, 0) and (s[0] > k[0] or (H - k[0]) % s[0]):
        assert bool((cover == 0).any())


def test_backward_without_x_applies_no_act_and_skips_foreign_argmax():
    dy = torch.arange(1.0, 13.0, dtype=f64).view(1, 2, 3, 2)
    am = torch.zeros(1, 2, 3, 2, dtype=torch.uint8)
    am[0, 0, 0, 0] = 255  # names no tap of a 2x2 window
    am[0, 1, 2, 1] = 3
    dx, cs = pool_bwd_reference(dy, am, (1, 5, 6, 2), (2, 2), (2, 2), (0, 0), act="relu")
    assert dx[0, 0, 0, 0] == 0 and dx[0, 0, 0, 1] == 2 and dx[0, 3, 5, 1] == 12 and dx[0, 2, 4, 1] == 0
    assert torch.count_nonzero(dx[0, 4]) == 0  # the floor remainder row
    assert cs[0] == dy[..., 0].sum() - 1 and cs[1] == dy[..., 1].sum()


def test_dropout_keep_reference_is_the_linear_index_hash():
    shape = (2, 3, 5, 8)
    m = dropout_keep_reference(torch.tensor([77, 3]), 5, shape, 0.3)
    p32 = float(torch.tensor(0.3, dtype=torch.float32))
    assert p32 != 0.3
    want = dropout_keep(77, 3, 5, torch.arange(240), p32).view(shape)
    assert m.dtype == torch.bool and torch.equal(m, want)
    big = dropout_keep_reference((77, 3), 5, (1 << 16,), 0.3)
    assert abs(float(big.double().mean()) - 0.7) < 4 * math.sqrt(0.21 / (1 << 16))
    assert not torch.equal(big, dropout_keep_reference((77, 4), 5, (1 << 16,), 0.3))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (5, 1, 3, 10), (2, 2, 2, 24), (3, 7, 7, 16), (2, 8, 8, 3)])
def test_global_average_references(B, H, W, C):
    g = torch.Generator().manual_seed(B + H + C)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    y = gap_reference(x)
    assert y.dtype == f64 and float((y - x.double().mean((1, 2))).abs().max()) <= 1e-15
    assert gap_reference(x, torch.float32).dtype == torch.float32
    xr = x.double().requires_grad_()
    dy = torch.randn(B, C, generator=g, dtype=f64)
    xr.mean((1, 2)).backward(dy)
    dx = gap_bwd_reference(dy, x.shape)
    assert dx.shape == x.shape and float((dx - xr.grad).abs().max()) <= 1e-15
