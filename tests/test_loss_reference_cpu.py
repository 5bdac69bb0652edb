"""Self-checks of the fp64 reference the loss-kernel tests compare with (functional.loss_reference and
head_reference: plain tensors, no kernel), and the LDS size formula the mlp_head launcher decides with."""
import pytest
import torch
import torch.nn.functional as F

from hops_examples_amd.ops import functional as HF
from hops_examples_amd.ops import kernels as K

f64 = torch.float64


def _autograd(fn, z):
    z = z.double().requires_grad_(True)
    l = fn(z)
    (g,) = torch.autograd.grad(l, (z,))
    return l.detach(), g


@pytest.mark.parametrize("B,C", [(1, 1), (7, 10), (5, 130)])
def test_softmax_kinds_against_autograd(B, C):
    gen = torch.Generator().manual_seed(B * 1000 + C)
    z = torch.randn(B, C, generator=gen) * 3
    lab = torch.randint(0, C, (B,), generator=gen)
    gs = 1.0 / 8  # a power of two: exact in fp32
    l, c, dl = HF.loss_reference(0, z, lab, gs)
    lr, gr = _autograd(lambda v: F.cross_entropy(v, lab, reduction="sum") * gs, z)
    assert l.dtype == f64 and dl.dtype == f64
    torch.testing.assert_close(l, lr, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dl, gr, rtol=1e-11, atol=1e-13)
    assert c == int((z.argmax(1) == lab).sum())  # (no ties in randn)
    t = torch.rand(B, C, generator=gen)  # rows that do not sum to 1
    l, c, dl = HF.loss_reference(1, z, t, gs)
    lr, gr = _autograd(lambda v: -(t.double() * F.log_softmax(v, 1)).sum() * gs, z)
    torch.testing.assert_close(l, lr, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dl, gr, rtol=1e-11, atol=1e-13)
    assert c == int((z.argmax(1) == t.argmax(1)).sum())


def test_first_maximal_index_wins():
    z = torch.tensor([[1.0, 5.0, 5.0, 2.0], [7.0, 0.0, 7.0, 7.0], [0.0, 0.0, 0.0, 0.0]])
    for lab, want in (([1, 0, 0], 3), ([2, 2, 1], 0), ([1, 3, 0], 2)):
        assert HF.loss_reference(0, z, torch.tensor(lab), 1.0)[1] == want
    t = torch.tensor([[0.5, 0.5, 0.0, 0.0], [0.0, 0.2, 0.4, 0.4], [0.0, 0.0, 0.0, 0.0]])
    # argmax rows: logits 1, 0, 0; targets 0, 2, 0 -> only the all-zero row agrees
    assert HF.loss_reference(1, z, t, 1.0)[1] == 1


def test_large_logits_stay_finite():
    z = torch.tensor([[80.0, 20.0, -75.0], [-80.0, -79.0, 60.0]])
    l, _, dl = HF.loss_reference(0, z, torch.tensor([1, 0]), 0.5)
    assert torch.isfinite(l) and torch.isfinite(dl).all()
    torch.testing.assert_close(l, torch.tensor(0.5 * (60.0 + 140.0), dtype=f64), rtol=1e-12, atol=0)
    l32, _, dl32 = HF.loss_reference(0, z, torch.tensor([1, 0]), 0.5, dtype=torch.float32)
    assert l32.dtype == torch.float32 and torch.isfinite(l32) and torch.isfinite(dl32).all()


def test_label_out_of_range_contributes_lse():
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(4, 6, generator=gen)
    lab = torch.tensor([2, 6, -1, 0])
    l, c, dl = HF.loss_reference(0, z, lab, 1.0)
    lse = torch.logsumexp(z.double(), 1)
    want = (lse[0] - z[0, 2]) + lse[1] + lse[2] + (lse[3] - z[3, 0])
    torch.testing.assert_close(l, want, rtol=1e-13, atol=0)
    torch.testing.assert_close(dl[1:3], torch.softmax(z.double(), 1)[1:3], rtol=1e-12, atol=0)
    valid = torch.tensor([True, False, False, True])
    assert c == int(((z.argmax(1) == lab) & valid).sum())


def test_elementwise_kinds_against_autograd():
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(9, 5, generator=gen) * 3
    y = torch.rand(9, 5, generator=gen).round()
    gs = 1.0 / 64
    l, c, dl = HF.loss_reference(2, z, y, gs)
    lr, gr = _autograd(lambda v: F.binary_cross_entropy_with_logits(v, y.double(), reduction="sum") * gs, z)
    torch.testing.assert_close(l, lr, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dl, gr, rtol=1e-11, atol=1e-13)
    assert c == int(((z > 0) == (y > 0.5)).sum())
    t = torch.randn(9, 5, generator=gen)
    l, c, dl = HF.loss_reference(3, z, t, gs)
    lr, gr = _autograd(lambda v: F.mse_loss(v, t.double(), reduction="sum") * gs, z)
    torch.testing.assert_close(l, lr, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dl, gr, rtol=1e-11, atol=1e-13)
    assert c == 0
    p = torch.rand(9, 5, generator=gen) * 0.98 + 0.01
    l, c, dl = HF.loss_reference(4, p, y, gs)
    lr, gr = _autograd(lambda v: F.binary_cross_entropy(v, y.double(), reduction="sum") * gs, p)
    torch.testing.assert_close(l, lr, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dl, gr, rtol=1e-11, atol=1e-13)
    assert c == int(((p > 0.5) == (y > 0.5)).sum())


def test_probability_bce_clamps_with_the_fp32_constants():
    eps = torch.tensor(1e-7, dtype=torch.float32)
    hi = torch.tensor(1.0, dtype=torch.float32) - eps
    assert float(eps) != 1e-7 and float(hi) != 1 - 1e-7  # the rounded constants differ from the decimal ones
    z = torch.stack([torch.tensor(0.0), torch.tensor(1.0), eps, hi, torch.tensor(-3.0), torch.tensor(2.0),
                     torch.nextafter(eps, torch.tensor(1.0)), torch.nextafter(hi, torch.tensor(0.0)),
                     torch.tensor(0.5), torch.tensor(0.25)]).view(1, -1)
    y = torch.tensor([[1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0]])
    l, c, dl = HF.loss_reference(4, z, y, 1.0)
    assert torch.isfinite(l) and torch.isfinite(dl).all()
    assert torch.count_nonzero(dl[0, :6]) == 0 and torch.count_nonzero(dl[0, 6:]) == 4
    e, h = float(eps), float(hi)
    import math
    want = -(math.log(e) + math.log(1 - h) + math.log(e) + math.log(1 - h) + math.log(1 - e) + math.log(h))
    torch.testing.assert_close(l - HF.loss_reference(4, z[:, 6:], y[:, 6:], 1.0)[0], torch.tensor(want, dtype=f64),
                               rtol=1e-12, atol=0)
    # correct: (z > 0.5) == (y > 0.5): 0/1 no, 1/0 no, eps/1 no, hi/0 no, -3/0 yes, 2/1 yes, ~eps/1 no, ~hi/0 no,
    # 0.5/1 no, 0.25/0 yes
    assert c == 3


def test_head_reference_against_autograd():
    gen = torch.Generator().manual_seed(5)
    B, C, KD = 6, 4, 9
    h = torch.randn(B, KD, generator=gen).to(torch.bfloat16)
    w = torch.randn(C, KD, generator=gen).to(torch.bfloat16)
    b = torch.randn(C, generator=gen)
    lab = torch.randint(0, C, (B,), generator=gen)
    hh, ww, bb = (v.double().requires_grad_(True) for v in (h, w, b))
    lr = F.cross_entropy(hh @ ww.t() + bb, lab, reduction="sum") * 0.25
    gh, gw, gb = torch.autograd.grad(lr, (hh, ww, bb))
    logits = HF.dense_reference(h, w, b)
    torch.testing.assert_close(logits, (hh @ ww.t() + bb).detach(), rtol=1e-14, atol=0)
    l, _, _, dw, db, dh = HF.head_reference(0, logits, lab, 0.25, h, w)
    for got, want in ((l, lr.detach()), (dw, gw), (db, gb), (dh, gh)):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-13)
    mask = torch.rand(B, KD, generator=gen) >= 0.25
    hd = HF.dropout_reference(h, mask, 0.25)
    assert hd.dtype == torch.bfloat16 and torch.count_nonzero(hd[~mask]) == 0
    torch.testing.assert_close(hd[mask].double(), h[mask].double() * 4 / 3, rtol=2.0 ** -8, atol=0)
    dhd = HF.head_reference(0, logits, lab, 0.25, hd, w, mask=mask, p=0.25)[5]
    assert torch.count_nonzero(dhd[~mask]) == 0
    torch.testing.assert_close(dhd[mask], gh[mask] * 4 / 3, rtol=2.0 ** -8 + 1e-6, atol=0)


def test_mlp_head_lds_formula():
    """Hand evaluation of loss.hip MlpLds; the launcher takes a shape up to 64 KiB."""
    sizes = {(16, 256): 65856, (32, 256): 80512, (32, 224): 72192, (32, 240): 76352, (15, 256): 64944,
             (32, 192): 63872, (10, 128): None}
    for (C, N1), want in sizes.items():
        got = K.mlp_head_lds(C, N1)
        assert want is None or got == want, (C, N1, got)
        assert got % 16 == 0 and got > 0
    assert K.mlp_head_lds(10, 128) <= K.MLP_HEAD_LDS_MAX == 65536
    for C, N1 in ((0, 128), (33, 128), (10, 8), (10, 24), (10, 272)):
        assert K.mlp_head_lds(C, N1) == 0, (C, N1)
    # monotone in both arguments: the guard cannot admit a larger shape than one it refuses
    for C in range(1, 32):
        for N1 in range(16, 256, 16):
            assert K.mlp_head_lds(C, N1) <= K.mlp_head_lds(C + 1, N1)
            assert K.mlp_head_lds(C, N1) < K.mlp_head_lds(C, N1 + 16)
