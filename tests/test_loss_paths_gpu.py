"""The loss family of csrc/ops/loss.hip (``loss_k``, ``head_ce_k``, ``mlp_head_k``) against the plain fp64
reference of hops_examples_amd.ops.functional (``loss_reference`` / ``head_reference`` / ``dense_reference`` /
``dropout_reference``) on every path of the three launchers.

How an output is compared (MARGIN = 8 everywhere; the yardstick is the same reference evaluated in fp32 by plain
torch, which knows nothing of the kernel):

* fp32 tensors (dlogits, dW, db, fp32 logits): ``max|x - ref64| / max|ref64 - old|`` (``old``: the pre-fill of an
  output the kernel adds to, else 0) must be within MARGIN x the yardstick's figure.  The yardstick is floored at
  one fp32 ulp (2^-23) of the SCALE of the terms that are added and cancelled on the way (``term_scales``: the
  softmax value and the one-hot it is subtracted from, sum |dl| |h| of a gradient dot product plus the
  pre-fill): a single fp32 evaluation is a single sample and lands within a tenth of an ulp by luck, while a
  confident row's p - 1 cannot be better than an ulp of p;
* where n partial sums are added one after another at the size of the total (loss_k's workgroup partials and
  head_ce_k's dW / db partials of n row blocks as float atomics, its n slot totals) the floor is
  1 + 0.29 sqrt(n - 1) ulp: the standard deviation of n roundings.  torch's fp32 sum is pairwise and does not
  show them; loss_k at 1024 workgroups measures 9 ulp;
* bf16 tensors (y, bf16 logits, dh, bf16 dlogits), per element: ``|x - ref64| <= n 2^-8 |ref64| + MARGIN acc``,
  n the number of bf16 roundings on the way (1; 2 for dh under a folded Dropout), ``acc`` the yardstick's largest
  absolute error on that tensor (floor: one fp32 ulp of max|ref64|).  In the terms of
  test_elementwise_bounds_gpu.py: frac = MARGIN acc / rms, measured per case instead of a constant;
* the loss: ``|loss - ref64| <= MARGIN max(|yardstick - ref64|, floor)`` with the floor as above on the sum of
  the magnitudes of the rows' terms, and never looser than ``1e-5 |ref64| + 1e-6``;
* ``correct``, every sentinel around an output, inputs, refused launches' outputs, mlp_head's workspace and
  arrival words: exact.  A second launch of a case must reproduce the totals (and, with one row block, dh and
  the logits bit for bit).

Where a kernel stores a value that a later stage reads (bf16 ``y``, the logits), that stage's reference starts
from the STORED tensor, which is itself checked against its own reference: a bf16 rounding that falls the other
way next to a tie is then no error of the stages behind it.

Every check prints ``LOSSERR <case> <output> kernel <e> yardstick <y> ratio <e / y>`` (the table at the end).

Out-of-range labels (kind 0): all three kernels follow the rule documented in ``row_thread``: the row reads no
logit and contributes its logsumexp, its dlogits are the plain softmax x gs, it is never counted correct, and
kernels.debug_errors() names the translation unit.

Measured on an MI355X, release build: the worst kernel / yardstick ratio (yardstick floored as above) over the
cases of each group, with the error figures of that case (relative to max|ref64 - old| for fp32 tensors, absolute
beyond the bf16 rounding allowance for bf16 ones, absolute for the loss).  Nothing needs more than 8x; ``__expf``
and ``__logf`` do not show at |z| = 80 (ratio 1.00), because the arguments that matter there are the small ones.

  kernel      regime      output   cases  worst ratio  kernel   yardstick
  loss_k      ordinary    loss     242    1.15         1.9e-06  1.6e-06
  loss_k      ordinary    dl       163    3.29         3.9e-07  1.2e-07   (B 1, C 32: __expf on a confident row)
  loss_k      |z| = 80    loss      12    0.25         1.6e-06  6.4e-06
  loss_k      |z| = 80    dl        12    1.00         3.8e-06  3.8e-06
  loss_k      ties        loss      16    0.41         2.5e-06  6.2e-06
  loss_k      ties        dl        12    1.09         8.0e-07  7.3e-07
  loss_k      kind-4 ends loss       5    0.83         8.8e-07  1.1e-06
  loss_k      kind-4 ends dl         5    0.41         4.9e-08  1.2e-07
  head_ce_k   ordinary    logits    44    1.26         1.5e-07  1.2e-07
  head_ce_k   ordinary    loss      88    0.81         1.1e-07  1.3e-07
  head_ce_k   ordinary    dw        88    4.41         5.7e-07  1.3e-07   (B 1: dl of one row times h)
  head_ce_k   ordinary    db        48    1.49         4.5e-07  3.0e-07
  head_ce_k   ordinary    dh        88    0.14         2.1e-11  1.5e-10
  head_ce_k   dropout     logits    12    0.49         5.9e-08  1.2e-07
  head_ce_k   dropout     loss      16    0.45         2.3e-07  5.1e-07
  head_ce_k   dropout     dw        16    0.85         3.4e-07  4.0e-07
  head_ce_k   dropout     db        16    1.27         3.4e-07  2.7e-07
  head_ce_k   dropout     dh        16    0.00         0        6.6e-10
  mlp_head_k  ordinary    y         92    0.08         4.5e-08  5.4e-07
  mlp_head_k  ordinary    logits    92    1.27         1.5e-07  1.2e-07
  mlp_head_k  ordinary    loss      92    1.10         5.4e-07  4.9e-07
  mlp_head_k  ordinary    dw        92    1.53         1.9e-07  1.3e-07
  mlp_head_k  ordinary    db        76    1.35         1.8e-07  1.3e-07
  mlp_head_k  ordinary    dh        92    0.00         0        3.2e-09
  mlp_head_k  dropout     y         24    0.00         0        4.9e-07
  mlp_head_k  dropout     logits    24    0.95         1.1e-07  1.2e-07
  mlp_head_k  dropout     loss      24    0.65         2.7e-07  4.1e-07
  mlp_head_k  dropout     dw        24    1.63         2.9e-07  1.8e-07
  mlp_head_k  dropout     db        24    1.86         2.7e-07  1.5e-07
  mlp_head_k  dropout     dh        24    0.00         0        2.0e-09
  out-of-range labels (all three)   24    0.75         9.2e-08  1.2e-07
"""
import itertools
import math
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.ops import _C  # noqa: E402
from hops_examples_amd.ops import functional as HF  # noqa: E402
from hops_examples_amd.ops import kernels as K  # noqa: E402
from hops_examples_amd.ops.functional import (dense_reference, dropout_reference, head_reference,  # noqa: E402
                                              loss_reference)

dev = torch.device("cuda", 0)
f32, bf, f64 = torch.float32, torch.bfloat16, torch.float64
MARGIN = 8.0
ULP32 = 2.0 ** -23
PAD = 64  # sentinel elements in front of and behind every framed tensor
SENT = {f32: -7777.25, bf: -3.0, torch.int32: -77}
DROP_P = 0.25
EPS4 = torch.tensor(1e-7, dtype=f32)
HI4 = torch.tensor(1.0, dtype=f32) - EPS4


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.encode()))


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


class Frame:
    """A device buffer of sentinels with the tensor as its view [off, off + n); off = PAD + 1 puts a bf16 tensor
    2 bytes off a 16-byte boundary."""

    def __init__(self, shape, dtype, init=None, off=PAD):
        self.n, self.off, self.sent = math.prod(shape), off, SENT[dtype]
        self.buf = torch.full((off + self.n + PAD,), self.sent, dtype=dtype, device=dev)
        self.v = self.buf[off:off + self.n].view(shape)
        if init is not None:
            self.v.copy_(init)

    def host(self):
        return self.v.cpu()

    def all(self):
        return self.buf.cpu()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.off] == self.sent).all()) and bool((b[self.off + self.n:] == self.sent).all())


# ------------------------------------------------------------------------------------------------- comparisons
def _line(case, name, e, y):
    print(f"LOSSERR {case} {name} kernel {e:.3e} yardstick {y:.3e} ratio {e / y if y else 0.0:.2f}")


def _ulps(chain):
    """fp32 ulps of the terms' scale the yardstick is floored at: 1, plus the standard deviation 0.29 sqrt(n) of n
    partial sums added one after another (workgroup partials arriving as float atomics, the row-block slots)."""
    return ULP32 * (1.0 + 0.29 * math.sqrt(chain - 1))


def check32(fails, case, name, x, ref, yard, base=None, scale=0.0, chain=1):
    ref = ref.double()
    den = (ref - (base.double() if base is not None else 0.0)).abs().max().item()
    scale = max(float(scale), den)
    if den == 0.0:
        den = scale  # an all-zero reference (softmax over one class): the size of the terms that cancel
    e = (x.double() - ref).abs().max().item() / den
    y = max((yard.double() - ref).abs().max().item(), _ulps(chain) * scale) / den
    _line(case, name, e, y)
    if not e <= MARGIN * y:
        fails.append((name, e, y))


def check16(fails, case, name, x, ref, yard, nround=1):
    ref = ref.double()
    acc = max((yard.double() - ref).abs().max().item(), ULP32 * ref.abs().max().item())
    over = (x.double() - ref).abs() - nround * 2.0 ** -8 * ref.abs()
    e = max(over.max().item(), 0.0)
    _line(case, name, e, acc)
    if not e <= MARGIN * acc:
        fails.append((name, e, acc, int((over > MARGIN * acc).sum())))


def check_loss(fails, case, x, ref, yard, scale, chain=1):
    ref, x, yard = float(ref), float(x), float(yard)
    e, y = abs(x - ref), max(abs(yard - ref), _ulps(chain) * max(float(scale), abs(ref)))
    _line(case, "loss", e, y)
    if not (math.isfinite(x) and e <= min(MARGIN * y, 1e-5 * abs(ref) + 1e-6)):
        fails.append(("loss", x, ref, e, y))


def term_scales(kind, z, t, gs):
    """The size of what is added and cancelled on the way to the loss sum and to one dlogits element (fp64): a
    result cannot be expected to be better than an fp32 ulp of these, however small it comes out itself (a
    confident row's p - 1; sum t lse - sum t z of a one-class row, which is exactly 0)."""
    z = z.double()
    if kind in (0, 1):
        lse = torch.logsumexp(z, 1)
        if kind == 0:
            inr = (t >= 0) & (t < z.shape[1])
            zl = z[torch.arange(z.shape[0]), t.clamp(0, z.shape[1] - 1)].abs() * inr
            return gs * (lse.abs() + zl).sum().item(), gs
        td = t.double()
        ts = td.sum(1)
        return gs * ((ts * lse).abs() + (td * z).abs().sum(1)).sum().item(), gs * max(1.0, ts.max().item())
    y = t.double()
    if kind == 2:
        return gs * (z.clamp(min=0) + (z * y).abs() + torch.log1p((-z.abs()).exp())).sum().item(), gs
    if kind == 3:
        return gs * ((z.abs() + y.abs()) ** 2).sum().item(), gs * 2 * (z.abs() + y.abs()).max().item()
    return 0.0, 0.0  # kind 4: a sum of positive terms; the quotient's terms do not cancel


# ------------------------------------------------------------------------------------------------------ inputs
def tie_pair(C, gen, row, wave):
    if wave and C > 65 and row == 0:
        return 3, 65  # lane 3 and lane 1 of the per-wave loop: the later lane holds the earlier class
    j = torch.randperm(C, generator=gen)[:2].sort().values
    return int(j[0]), int(j[1])


def make_inputs(kind, B, C, lf32, regime, gen, wave=False):
    """Host logits (in the logits dtype) and targets for one case."""
    ldt = f32 if lf32 else bf
    if kind == 4:
        z = torch.rand(B, C, generator=gen) * 0.98 + 0.01
    else:
        z = torch.randn(B, C, generator=gen) * 3
    if kind == 0:
        t = torch.randint(0, C, (B,), generator=gen)
    elif kind == 1:
        t = torch.rand(B, C, generator=gen)  # rows that do not sum to 1 ...
        if B % 2:
            t = torch.softmax(t * 4, 1)  # ... and rows that do (up to rounding)
    elif kind == 3:
        t = torch.randn(B, C, generator=gen)
    else:
        t = torch.rand(B, C, generator=gen)
        t = torch.where(torch.rand(B, C, generator=gen) < 0.8, t.round(), t)  # mostly hard 0 / 1, some soft
    if regime == "big":  # |z| about 80, signs mixed; row 0: the top two 60 apart, everything else below
        z = (70 + 20 * torch.rand(B, C, generator=gen)) * torch.where(torch.rand(B, C, generator=gen) < 0.5, -1.0, 1.0)
        if C > 1:
            z[0] = -60 * torch.rand(C, generator=gen)
            z[0, C // 2], z[0, C - 1] = 80.0, 20.0
    elif regime == "ties":  # exact ties of the maximum (bf16 logits, dense targets)
        z = z.to(bf).float()
        for r in range(B):
            j1, j2 = tie_pair(C, gen, r, wave)
            top = (z[r].max() + 1).to(bf).float()
            if kind == 0:
                z[r, j1] = z[r, j2] = top
                t[r] = j1 if r % 2 == 0 else j2  # the first maximal class counts, the second does not
            else:
                cls = r % 4  # 0/1: logits tie, unique target at the first / second; 2/3: the other way round
                if cls < 2:
                    z[r, j1] = z[r, j2] = top
                    t[r, j1 if cls == 0 else j2] = 2.0
                else:
                    z[r, j1 if cls == 2 else j2] = top
                    t[r, j1] = t[r, j2] = 2.0
    elif regime == "k4edge":  # exactly 0, 1, eps, 1 - eps, values outside [0, 1] and values inside
        i = torch.arange(B * C).view(B, C) % 9
        for k, v in enumerate((0.0, 1.0, float(EPS4), float(HI4), -0.5, 1.5)):
            z = torch.where(i == k, torch.tensor(v), z)
    return z.to(ldt), (t if kind == 0 else t.float())


def gscale(kind, B, C):
    return 1.0 / (B * (C if kind in (2, 3, 4) else 1))


# ------------------------------------------------------------------------------------------------------ loss_k
COMBOS = list(itertools.product((True, False), ("f32", "bf16", None)))  # logits fp32 / bf16 x dlogits dtype


def run_loss(case, kind, B, C, lf32, dmode, regime="randn3", wave=False):
    z, t = make_inputs(kind, B, C, lf32, regime, _gen(case), wave)
    gs = gscale(kind, B, C)
    L, T = Frame((B, C), z.dtype, z), t.to(dev)
    D = Frame((B, C), f32 if dmode == "f32" else bf) if dmode else None
    ls, cor = Frame((1,), f32), Frame((1,), torch.int32)  # (the sentinels are the garbage the totals start from)
    K.loss_fwd_bwd(kind, L.v, T, gs, ls.v, cor.v, D.v if D else None)
    torch.cuda.synchronize()
    ref, yard = loss_reference(kind, z, t, gs), loss_reference(kind, z, t, gs, dtype=f32)
    lscale, dscale = term_scales(kind, z, t, gs)
    # workgroups whose partial losses arrive as float atomics (the launcher's grid)
    if C <= 32 and "loss_thread" not in os.environ.get("HOPSX_DISABLE", ""):
        chain = 1 if B <= 1024 else min(1024, -(-B // 256))
    else:
        chain = 1 if B <= 16 else min(1024, -(-B // 4))
    fails = []
    check_loss(fails, case, ls.host().item(), ref[0], yard[0], lscale, chain)
    assert cor.host().item() == ref[1], (case, "correct", cor.host().item(), ref[1])
    if D is not None:
        dl = D.host()
        assert torch.isfinite(dl).all(), case
        if dmode == "f32":
            check32(fails, case, "dl", dl, ref[2], yard[2], scale=dscale)
        else:
            check16(fails, case, "dl", dl, ref[2], yard[2])
        if kind == 4:  # the clamped ends have exactly no gradient
            flat = (z.float() <= EPS4) | (z.float() >= HI4)
            assert torch.count_nonzero(dl[flat]) == 0, case
    assert not fails, (case, fails)
    for fr in (L, ls, cor) + ((D,) if D else ()):
        assert fr.intact(), case
    assert bits_equal(L.host(), z) and bits_equal(T.cpu(), t), case
    return ls.host().item()


def sweep_loss(tag, kind, shapes, regime="randn3", wave=False, combos=COMBOS):
    for i, (B, C) in enumerate(shapes):
        lf32, dmode = combos[(i + kind) % len(combos)]
        run_loss(f"{tag} k{kind} B{B} C{C} {'f32' if lf32 else 'bf16'}->{dmode} {regime}", kind, B, C, lf32, dmode,
                 regime, wave)


@pytest.mark.parametrize("kind", range(5))
def test_loss_per_thread(kind):
    """C <= 32: one workgroup of 64 .. 1024 threads that overwrites the (garbage) totals up to B = 1024, then
    several workgroups of 256 adding to zeroed totals (B = 1025: 5)."""
    sweep_loss("thread", kind, list(itertools.product((1, 63, 64, 65, 1024, 1025), (1, 2, 10, 32))))


@pytest.mark.parametrize("kind", (2, 3))
def test_loss_per_thread_grid_stride(kind):
    """B = 262,145 > 1024 workgroups x 256 threads: thread 0 of workgroup 0 takes a second row."""
    sweep_loss("stride", kind, [(262_145, 1)], combos=[(True, "f32")])


@pytest.mark.parametrize("kind", range(5))
def test_loss_per_wave(kind):
    """C > 32: one 1024-thread workgroup (B <= 16), workgroups of 4 waves (B = 17) and their grid-stride loop
    (B = 4097 > 1024 x 4)."""
    sweep_loss("wave", kind, list(itertools.product((1, 16, 17), (33, 64, 65, 130, 1000))) + [(4097, 33)], wave=True)


@pytest.mark.parametrize("kind", range(5))
def test_loss_per_wave_code_at_small_C(kind, monkeypatch):
    """HOPSX_DISABLE=loss_thread (read on every call): the per-wave code with most lanes idle."""
    monkeypatch.setenv("HOPSX_DISABLE", "loss_thread")
    sweep_loss("wave-smallC", kind, list(itertools.product((1, 16, 17, 65), (10, 32))), wave=True)


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_loss_large_logits(kind, monkeypatch):
    """|z| about 80 in fp32 and a row whose top two are 60 apart: finite, and inside the same bounds."""
    shapes = [(65, 10), (17, 130), (5, 2)]
    sweep_loss("thread", kind, shapes, "big", combos=[(True, "f32"), (True, "bf16")])
    monkeypatch.setenv("HOPSX_DISABLE", "loss_thread")
    sweep_loss("wave-smallC", kind, shapes[:1], "big", wave=True, combos=[(True, "f32")])


@pytest.mark.parametrize("kind", (0, 1))
def test_loss_argmax_ties(kind, monkeypatch):
    """Exact ties of the maximum in bf16 logits and in dense targets: the first maximal index wins in both."""
    sweep_loss("tie", kind, [(64, 2), (65, 10), (33, 32), (17, 65), (16, 130), (18, 1000)], "ties", wave=True,
               combos=[(False, "bf16"), (False, "f32"), (False, None)])
    monkeypatch.setenv("HOPSX_DISABLE", "loss_thread")
    sweep_loss("tie wave-smallC", kind, [(17, 10), (16, 32)], "ties", wave=True, combos=[(False, "f32")])


def test_loss_probability_bce_edges(monkeypatch):
    """Kind 4 at exactly 0, 1, eps, 1 - eps, outside [0, 1] and inside: finite loss, zero gradient at the clamp."""
    shapes = [(9, 1), (65, 10), (17, 65), (1025, 2)]
    sweep_loss("k4", 4, shapes, "k4edge", combos=[(True, "f32"), (True, "bf16"), (False, "f32")])
    monkeypatch.setenv("HOPSX_DISABLE", "loss_thread")
    sweep_loss("k4 wave-smallC", 4, shapes[1:2], "k4edge", wave=True, combos=[(True, "f32")])


# --------------------------------------------------------------------------------------------------- head_ce_k
def drop_mask(shape, rng, salt):
    return (K.dropout(torch.ones(shape, device=dev, dtype=bf), DROP_P, rng, salt) != 0).cpu()


def head_operands(kind, B, C, KD, gen):
    h = torch.randn(B, KD, generator=gen).to(bf)
    w = (torch.randn(C, KD, generator=gen) * ((0.2 if kind == 4 else 1.0) / math.sqrt(KD))).to(bf)
    b = torch.randn(C, generator=gen) * 0.1 + (0.5 if kind == 4 else 0.0)
    return h, w, b


def check_head(fails, case, kind, z, t, gs, hin, w, mask, got, old_dw, old_db, chain=1):
    """got = (loss, correct, dw, db or None, dh) on the host, from the logits ``z`` the loss saw.  chain: the row
    blocks, whose loss partials are summed one after another and whose dw / db partials arrive as float atomics."""
    p = DROP_P if mask is not None else 0.0
    ref = head_reference(kind, z, t, gs, hin, w, mask, p)
    yard = head_reference(kind, z, t, gs, hin, w, mask, p, dtype=f32)
    check_loss(fails, case, got[0], ref[0], yard[0], term_scales(kind, z, t, gs)[0], chain)
    assert got[1] == ref[1], (case, "correct", got[1], ref[1])
    adl = ref[2].abs()  # the scale of a dot product: sum |a| |b|
    check32(fails, case, "dw", got[2], old_dw.double() + ref[3], old_dw + yard[3], base=old_dw,
            scale=(adl.t() @ hin.double().abs()).max().item() + old_dw.abs().max().item(), chain=chain)
    if got[3] is not None:
        check32(fails, case, "db", got[3], old_db.double() + ref[4], old_db + yard[4], base=old_db,
                scale=adl.sum(0).max().item() + old_db.abs().max().item(), chain=chain)
    check16(fails, case, "dh", got[4], ref[5], yard[5], nround=2 if mask is not None else 1)


def run_head(case, kind, B, C, KD, lf32=True, forward=True, bias=True, with_db=True, mis=None, drop=False):
    gen = _gen(case)
    assert K.head_ce_ok(C, KD), case
    h, w, b = head_operands(kind, B, C, KD, gen)
    zin, t = make_inputs(kind, B, C, lf32, "randn3", gen)
    gs = gscale(kind, B, C)
    H = Frame((B, KD), bf, h, off=PAD + (mis == "h"))
    W = Frame((C, KD), bf, w, off=PAD + (mis == "w"))
    assert (H.v.data_ptr() % 16 != 0) == (mis == "h") and (W.v.data_ptr() % 16 != 0) == (mis == "w")
    T, bd = t.to(dev), (b.to(dev) if bias and forward else None)
    dw0, db0 = torch.randn(C, KD, generator=gen) * 0.01, torch.randn(C, generator=gen) * 0.01

    def outputs():
        return (Frame((B, C), zin.dtype, None if forward else zin), Frame((C, KD), f32, dw0),
                Frame((C,), f32, db0) if with_db else None, Frame((1,), f32), Frame((1,), torch.int32))

    Lg, DW, DB, ls, cor = outputs()
    rng = torch.tensor([zlib.crc32(case.encode()), 5], device=dev, dtype=torch.int64) if drop else None
    salt = 0x9E3779B1
    mask = drop_mask((B, KD), rng, salt) if drop else None
    hin = dropout_reference(h, mask, DROP_P) if drop else h
    seen = []
    for k in range(2):
        old_dw, old_db = DW.host(), (DB.host() if DB else None)
        ls.v.fill_(SENT[f32])
        cor.v.fill_(SENT[torch.int32])
        dh = K.head_ce(kind, Lg.v, T, H.v, W.v, DW.v, DB.v if DB else None, gs, ls.v, cor.v, bias=bd,
                       forward=forward, drop=(DROP_P, rng, salt) if drop else None)
        torch.cuda.synchronize()
        fails, tag = [], f"{case}#{k}"
        z = Lg.host()
        if forward:
            args = (hin, w, b if bias else None)
            (check32 if lf32 else check16)(fails, tag, "logits", z, dense_reference(*args),
                                           dense_reference(*args, dtype=f32))
        else:
            assert bits_equal(z, zin), tag
        got = (ls.host().item(), cor.host().item(), DW.host(), DB.host() if DB else None, dh.cpu())
        check_head(fails, tag, kind, z, t, gs, hin, w, mask, got, old_dw, old_db, chain=(B + 31) // 32)
        assert not fails, (tag, fails)
        for fr in (Lg, DW, ls, cor, H, W) + ((DB,) if DB else ()):
            assert fr.intact(), tag
        assert bits_equal(H.host(), h) and bits_equal(W.host(), w), tag
        seen.append((ls.host(), got[1], got[4], z, got[2], got[3]))
        if k == 0 and drop and B <= 32:
            # the unfused chain: dropout_k -> head_ce_k -> dropout_k on dh, from the same pre-fills; one row
            # block: every dw element receives a single add onto the same start value, so bit for bit
            Lu, DWu, DBu, lsu, coru = outputs()
            dhu = K.head_ce(kind, Lu.v, T, K.dropout(H.v, DROP_P, rng, salt), W.v, DWu.v, DBu.v if DBu else None, gs,
                            lsu.v, coru.v, bias=bd, forward=forward)
            dhu = K.dropout(dhu, DROP_P, rng, salt)
            torch.cuda.synchronize()
            for name, a, c in (("logits", Lu.host(), z), ("loss", lsu.host(), ls.host()), ("dw", DWu.host(), got[2]),
                               ("dh", dhu.cpu(), got[4]), ("correct", coru.host(), cor.host())):
                assert bits_equal(a, c), (tag, "fused dropout != unfused chain", name)
            if DB:
                assert bits_equal(DBu.host(), got[3]), (tag, "fused dropout != unfused chain", "db")
    a, c = seen
    assert a[1] == c[1], (case, "correct of the second launch")
    if (B + 31) // 32 <= 64:  # stored totals (one block, or the slots summed in row-block order)
        assert bits_equal(a[0], c[0]), (case, "loss of the second launch", a[0], c[0])
    if B <= 32:
        assert bits_equal(a[2], c[2]) and bits_equal(a[3], c[3]), (case, "dh / logits of the second launch")


def _head_kind(C, i):
    return {1: (2, 4)[i % 2], 3: 3, 10: 0, 17: 1, 32: (0, 1)[i % 2]}[C]


HEAD_KD = [(8, None), (24, None), (33, None), (100, None), (128, None), (264, None), (128, "h"), (128, "w")]
HEAD_OPTS = list(itertools.product((True, False), (True, False), (True, False)))  # forward, logits fp32, bias/db


def _head_cases():
    i = 0
    for (KD, mis), C in itertools.product(HEAD_KD, (1, 3, 10, 17, 32)):
        B = (1, 31, 32, 33)[(i + i // 4) % 4]
        fwd, lf32, bdb = HEAD_OPTS[(i + i // 8) % 8]
        yield pytest.param(_head_kind(C, i // 5), B, C, KD, lf32, fwd, bdb, mis,
                           id=f"k{_head_kind(C, i // 5)}-B{B}-C{C}-KD{KD}{mis or ''}-{'fwd' if fwd else 'bwd'}-"
                              f"{'f32' if lf32 else 'bf16'}-{'bias' if bdb else 'nobias'}")
        i += 1


@pytest.mark.parametrize("kind,B,C,KD,lf32,forward,bdb,mis", list(_head_cases()))
def test_head_ce(kind, B, C, KD, lf32, forward, bdb, mis):
    """KD 8 / 24 / 128: the 16-byte staging (one and four column blocks); 33: the scalar staging (vec == 0); 100:
    scalar, column blocks of 34 / 34 / 32; 264: 8 blocks of 33; 128 with h or w one element off: misaligned, so
    scalar.  B 33: two row blocks (the slot totals)."""
    run_head(f"head k{kind} B{B} C{C} KD{KD}{mis or ''} fwd{int(forward)} f32{int(lf32)} b{int(bdb)}", kind, B, C, KD,
             lf32, forward, bdb, bdb, mis)


@pytest.mark.parametrize("B", (2048, 2049))
@pytest.mark.parametrize("forward,lf32", ((True, False), (False, True)))
def test_head_ce_row_block_totals(B, forward, lf32):
    """64 row blocks: the slot path at its limit; 65: zeroed totals and atomics."""
    run_head(f"head rows B{B} fwd{int(forward)}", 0, B, 10, 24, lf32, forward)


@pytest.mark.parametrize("kind,B,C,KD,forward,lf32", [
    (0, 32, 10, 128, True, False), (0, 1, 10, 24, True, True), (1, 31, 17, 33, True, True),
    (0, 33, 10, 128, True, False), (2, 32, 1, 100, False, True), (3, 17, 3, 264, True, False),
    (4, 32, 1, 8, True, True), (1, 65, 32, 128, False, False)])
def test_head_ce_folded_dropout(kind, B, C, KD, forward, lf32):
    """p = 0.25 with the project's own mask; at one row block also bit for bit the unfused chain."""
    run_head(f"head drop k{kind} B{B} C{C} KD{KD} fwd{int(forward)}", kind, B, C, KD, lf32, forward, drop=True)


def test_head_ce_refusals():
    """-2: B = 0 or a (C, KD) head_ce_ok refuses; -3: a dropout without h, without rng or with p >= 1.  Nothing
    is launched: every output keeps its pre-fill."""
    gen = _gen("refusals")
    assert not K.head_ce_ok(32, 512) and not K.head_ce_ok(33, 8) and K.head_ce_ok(32, 264)
    rng = torch.tensor([1, 2], device=dev, dtype=torch.int64)
    for what, B, C, KD, drop, code, no_h in (("B0", 0, 10, 24, None, -2, False), ("lds", 4, 32, 512, None, -2, False),
                                             ("C33", 4, 33, 8, None, -2, False),
                                             ("p1", 4, 10, 24, (1.0, rng, 7), -3, False),
                                             ("norng", 4, 10, 24, (0.25, None, 7), -3, False),
                                             ("noh", 4, 10, 24, (0.25, rng, 7), -3, True)):
        Bn = max(B, 1)
        h, w, b = head_operands(0, Bn, C, KD, gen)
        H, W = Frame((Bn, KD), bf, h), Frame((C, KD), bf, w)
        Lg, DW, DB = Frame((Bn, C), f32), Frame((C, KD), f32), Frame((C,), f32)
        ls, cor, DH = Frame((1,), f32), Frame((1,), torch.int32), Frame((Bn, KD), bf)
        T = torch.zeros(Bn, device=dev, dtype=torch.int64)
        before = [fr.all() for fr in (Lg, DW, DB, ls, cor, DH)]
        if no_h:
            rc = _C.ext().head_ce(0, K.ptr(Lg.v), 1, K.ptr(T), B, C, KD, 0.25, 0, K.ptr(W.v), K.ptr(DW.v), K.ptr(DB.v),
                                  K.ptr(DH.v), K.ptr(ls.v), K.ptr(cor.v), 0, 0, 0.25, K.ptr(rng), 7, K.stream())
            assert rc == code, (what, rc)
        else:
            with pytest.raises(RuntimeError, match=f"head_ce failed with hipError {code}$"):
                K.head_ce(0, Lg.v[:B], T[:B], H.v[:B], W.v, DW.v, DB.v, 0.25, ls.v, cor.v, bias=b.to(dev),
                          forward=True, drop=drop)
        torch.cuda.synchronize()
        for fr, o in zip((Lg, DW, DB, ls, cor, DH), before):
            assert bits_equal(fr.all(), o), what


# -------------------------------------------------------------------------------------------------- mlp_head_k
def mlp_operands(kind, B, Kd, N1, C, gen):
    x = torch.randn(B, Kd, generator=gen).to(bf)
    w1 = (torch.randn(N1, Kd, generator=gen) / math.sqrt(Kd)).to(bf)
    b1 = torch.randn(N1, generator=gen) * 0.1
    w2 = (torch.randn(C, N1, generator=gen) * ((0.2 if kind == 4 else 1.0) / math.sqrt(N1))).to(bf)
    b2 = torch.randn(C, generator=gen) * 0.1 + (0.5 if kind == 4 else 0.0)
    return x, w1, b1, w2, b2


def mlp_frames(B, N1, C, lf32, dw0, db0):
    return (Frame((B, N1), bf), Frame((B, C), f32 if lf32 else bf), Frame((C, N1), f32, dw0),
            Frame((C,), f32, db0) if db0 is not None else None, Frame((1,), f32), Frame((1,), torch.int32))


def ws_at_rest(B, N1):
    ws, arrive = K._mlp_ws(dev, B * N1)
    return torch.count_nonzero(ws).item() == 0 and torch.count_nonzero(arrive).item() == 0


def run_mlp(case, B, Kd, N1, C, kind, lf32=False, act="relu", has_b1=True, has_b2=True, has_db2=True, drop=False,
            label_fix=None):
    gen = _gen(case)
    x, w1, b1, w2, b2 = mlp_operands(kind, B, Kd, N1, C, gen)
    t = make_inputs(kind, B, C, True, "randn3", gen)[1]
    if label_fix:
        for r, v in label_fix.items():
            t[r] = v
    gs = gscale(kind, B, C)
    X, W1, W2 = Frame((B, Kd), bf, x), Frame((N1, Kd), bf, w1), Frame((C, N1), bf, w2)
    b1d, b2d, T = (b1.to(dev) if has_b1 else None), (b2.to(dev) if has_b2 else None), t.to(dev)
    dw0, db0 = torch.randn(C, N1, generator=gen) * 0.01, torch.randn(C, generator=gen) * 0.01
    Y, Lg, DW, DB, ls, cor = mlp_frames(B, N1, C, lf32, dw0, db0 if has_db2 else None)
    rng = torch.tensor([zlib.crc32(case.encode()), 9], device=dev, dtype=torch.int64) if drop else None
    salt = 0x51ED27
    mask = drop_mask((B, N1), rng, salt) if drop else None
    seen = []
    for k in range(2):
        old_dw, old_db = DW.host(), (DB.host() if DB else None)
        ls.v.fill_(SENT[f32])
        cor.v.fill_(SENT[torch.int32])
        dh = K.mlp_head(X.v, W1.v, b1d, act, Y.v, kind, Lg.v, T, W2.v, b2d, DW.v, DB.v if DB else None, gs, ls.v,
                        cor.v, drop=(DROP_P, rng, salt) if drop else None)
        assert dh is not False, case
        torch.cuda.synchronize()
        fails, tag = [], f"{case}#{k}"
        assert ws_at_rest(B, N1), (tag, "workspace / arrival words not zero at rest")
        y, z = Y.host(), Lg.host()
        dargs = (x, w1, b1 if has_b1 else None, act)
        check16(fails, tag, "y", y, dense_reference(*dargs), dense_reference(*dargs, dtype=f32))
        hin = dropout_reference(y, mask, DROP_P) if drop else y  # the head reads the STORED y
        largs = (hin, w2, b2 if has_b2 else None)
        (check32 if lf32 else check16)(fails, tag, "logits", z, dense_reference(*largs),
                                       dense_reference(*largs, dtype=f32))
        got = (ls.host().item(), cor.host().item(), DW.host(), DB.host() if DB else None, dh.cpu())
        check_head(fails, tag, kind, z, t, gs, hin, w2, mask, got, old_dw, old_db)
        assert not fails, (tag, fails)
        for fr in (Y, Lg, DW, ls, cor, X, W1, W2) + ((DB,) if DB else ()):
            assert fr.intact(), tag
        assert bits_equal(X.host(), x) and bits_equal(W1.host(), w1) and bits_equal(W2.host(), w2), tag
        seen.append((ls.host(), got[1], z))
    # (the split-K partials arrive in any order, so y may differ in a last bit between the launches: each launch
    # is held to its own stored y and logits above, not to the other launch)
    return seen[1][0].item(), seen[1][2], t


# head configuration: C, kind, logits fp32, act1, b1, b2, db2, dropout.  C <= 16: the MFMA tail (mlp_loss16), C > 16
# the FMA tail (row_thread).  Each runs at every B of MLP_B, every K of MLP_K and every N1 it fits with.
MLP_PATHS = {
    "C10-k0": (10, 0, False, "relu", True, True, True, False),
    "C10-k1-f32-noact": (10, 1, True, "none", True, True, True, False),
    "C10-k0-drop": (10, 0, False, "relu", True, True, True, True),
    "C1-k2-nob1": (1, 2, False, "relu", False, True, True, False),
    "C1-k4-f32": (1, 4, True, "relu", True, True, True, False),
    "C3-k3-nob2-nodb2": (3, 3, False, "relu", True, False, False, False),
    "C3-k0-f32": (3, 0, True, "none", True, True, True, False),
    "C16-k0": (16, 0, False, "relu", True, True, True, False),
    "C16-k1-f32-drop": (16, 1, True, "relu", True, True, True, True),
    "C17-k0": (17, 0, False, "relu", True, True, True, False),
    "C17-k1-f32-noact-nobias": (17, 1, True, "none", False, False, False, False),
    "C32-k0-drop": (32, 0, False, "relu", True, True, True, True),
    "C32-k1-f32": (32, 1, True, "relu", True, True, True, False),
    "C17-k3": (17, 3, False, "relu", True, True, True, False),
}
MLP_B, MLP_K = (1, 16, 17, 32), (8, 200, 1032)


def _mlp_n1(C):
    """N1 = 256 needs more than 64 KiB of LDS from C = 16 on (the launcher refuses it): 256 goes with C <= 15."""
    return (16, 48, 128, 256) if C <= 15 else (16, 48, 128, 48)


@pytest.mark.parametrize("j", range(4))
@pytest.mark.parametrize("path", list(MLP_PATHS))
def test_mlp_head(path, j):
    """B 16 / 17: the RF = 1 / RF = 2 instantiations; N1 48: the trailing 16-deep MFMA step (C <= 16), nq = 1
    (C > 16); N1 128: nq = 4; K 8: one workgroup, 1032: nine with a partial last chunk."""
    C, kind, lf32, act, hb1, hb2, hdb2, drop = MLP_PATHS[path]
    i = list(MLP_PATHS).index(path)
    B, N1, Kd = MLP_B[j], _mlp_n1(C)[(i + j) % 4], MLP_K[(i + j) % 3]
    run_mlp(f"mlp {path} B{B} N{N1} K{Kd}", B, Kd, N1, C, kind, lf32, act, hb1, hb2, hdb2, drop)


def test_mlp_head_value_coverage():
    """The sparse crossing above meets every B, N1 (256 only where it fits) and K with every head configuration."""
    for i, (path, cfg) in enumerate(MLP_PATHS.items()):
        n1s = {_mlp_n1(cfg[0])[(i + j) % 4] for j in range(4)}
        assert n1s == set(_mlp_n1(cfg[0])), path
        assert {MLP_K[(i + j) % 3] for j in range(4)} == set(MLP_K), path
    assert K.mlp_head_lds(16, 48) <= K.MLP_HEAD_LDS_MAX and K.mlp_head_lds(32, 128) <= K.MLP_HEAD_LDS_MAX


def _mlp_refused(case, B, Kd, N1, C, x_off=PAD):
    gen = _gen(case)
    x, w1, b1, w2, b2 = mlp_operands(0, B, Kd, N1, C, gen)
    X, W1, W2 = Frame((B, Kd), bf, x, off=x_off), Frame((N1, Kd), bf, w1), Frame((C, N1), bf, w2)
    Y, Lg, DW, DB, ls, cor = mlp_frames(B, N1, C, False, torch.ones(C, N1), torch.ones(C))
    T = torch.zeros(B, device=dev, dtype=torch.int64)
    before = [fr.all() for fr in (Y, Lg, DW, DB, ls, cor)]
    r = K.mlp_head(X.v, W1.v, b1.to(dev), "relu", Y.v, 0, Lg.v, T, W2.v, b2.to(dev), DW.v, DB.v, 1.0 / B, ls.v, cor.v)
    torch.cuda.synchronize()
    assert r is False, (case, "expected a refusal")
    for fr, o in zip((Y, Lg, DW, DB, ls, cor), before):
        assert bits_equal(fr.all(), o), case
    assert ws_at_rest(B, N1), case


@pytest.mark.parametrize("what,B,Kd,N1,C,x_off", [
    ("B33", 33, 200, 128, 10, PAD), ("N24", 8, 200, 24, 10, PAD), ("N272", 8, 200, 272, 10, PAD),
    ("K12", 8, 12, 128, 10, PAD), ("x-misaligned", 8, 200, 128, 10, PAD + 1), ("C33", 8, 200, 128, 33, PAD)])
def test_mlp_head_refused_shapes(what, B, Kd, N1, C, x_off):
    _mlp_refused(f"mlp refused {what}", B, Kd, N1, C, x_off)


# ------------------------------------------------------------------------------------------------ the LDS guard
def _two_layer_step(monkeypatch, C, N1, B=8, Kd=64):
    """Dense(N1, relu) -> Dense(C) -> sparse CE through loss_and_grad_root with both layers deferred, as TrainStep
    arms them.  Returns what mlp_head answered and the fused step's results."""
    from hops_examples_amd.runtime.arena import ParamArena

    gen = _gen(f"two-layer C{C} N{N1}")
    net = torch.nn.Sequential(torch.nn.Linear(Kd, N1), torch.nn.Linear(N1, C)).to(dev)
    with torch.no_grad():
        net[0].weight.copy_(torch.randn(N1, Kd, generator=gen) / math.sqrt(Kd))
        net[0].bias.copy_(torch.randn(N1, generator=gen) * 0.1)
        net[1].weight.copy_(torch.randn(C, N1, generator=gen) / math.sqrt(N1))
        net[1].bias.copy_(torch.randn(C, generator=gen) * 0.1)
    ParamArena.from_module(net, dev)
    x = torch.randn(B, Kd, generator=gen).to(bf).to(dev)
    t = torch.randint(0, C, (B,), generator=gen)
    answers = []
    real = K.mlp_head

    def spy(*a, **kw):
        answers.append(real(*a, **kw))
        return answers[-1]

    monkeypatch.setattr(K, "mlp_head", spy)
    monkeypatch.setitem(HF.HEAD, "defer", True)
    monkeypatch.setitem(HF.PREHEAD, "w", net[0].weight)
    h = HF.linear(x, net[0].weight, net[0].bias, act="relu")
    out = HF.linear(h, net[1].weight, net[1].bias, out_f32=True)
    assert getattr(out, "_hx_dense_head")[4] and HF.PREHEAD["pending"], "the two layers were not deferred"
    loss, correct, count, root, grad = HF.loss_and_grad_root(out, t.to(dev), "sparse_ce")
    torch.cuda.synchronize()
    assert len(answers) == 1 and root.data_ptr() == h.data_ptr() and count == B and not HF.PREHEAD["pending"]
    fails, case = [], f"two-layer C{C} N{N1}"
    w1, b1 = net[0].weight.detach().to(bf).cpu(), net[0].bias.detach().cpu()
    w2, b2 = net[1].weight.detach().to(bf).cpu(), net[1].bias.detach().cpu()
    y, z = h.detach().cpu(), out.detach().cpu()
    check16(fails, case, "y", y, dense_reference(x.cpu(), w1, b1, "relu"),
            dense_reference(x.cpu(), w1, b1, "relu", dtype=f32))
    check32(fails, case, "logits", z, dense_reference(y, w2, b2), dense_reference(y, w2, b2, dtype=f32))
    ref = head_reference(0, z, t, 1.0 / B, y, w2)
    yard = head_reference(0, z, t, 1.0 / B, y, w2, dtype=f32)
    check_loss(fails, case, loss.item(), ref[0], yard[0], term_scales(0, z, t, 1.0 / B)[0])
    assert int(correct) == ref[1], case
    check16(fails, case, "dh", grad.cpu(), ref[5], yard[5])
    assert not fails, (case, fails)
    return answers[0]


@pytest.mark.parametrize("C,N1", [(16, 256), (32, 224), (32, 256)])
def test_mlp_head_over_the_lds_limit_falls_back(monkeypatch, C, N1):
    """More than 64 KiB of LDS: refused before anything is launched, nothing written, and loss_and_grad_root
    still gives the right loss through the Dense forward + head_ce."""
    assert K.mlp_head_lds(C, N1) > K.MLP_HEAD_LDS_MAX and K.head_ce_ok(C, N1)
    _mlp_refused(f"mlp lds C{C} N{N1}", 8, 64, N1, C)
    assert _two_layer_step(monkeypatch, C, N1) is False


@pytest.mark.parametrize("C,N1", [(15, 256), (32, 192)])
def test_mlp_head_just_under_the_lds_limit_is_fused(monkeypatch, C, N1):
    assert 60000 < K.mlp_head_lds(C, N1) <= K.MLP_HEAD_LDS_MAX
    run_mlp(f"mlp lds C{C} N{N1}", 17, 200, N1, C, 0)
    assert _two_layer_step(monkeypatch, C, N1) is not False


# ------------------------------------------------------------------------------------------ out-of-range labels
def test_label_out_of_range_same_rule_on_every_path(monkeypatch):
    """Rows 2 (label C) and 5 (label -1) among valid ones, through mlp_head_k (C = 10: mlp_loss16; C = 17: its
    row_thread tail), then head_ce_k and loss_k (per thread and per wave) on the logits it stored."""
    if os.environ.get("HOPSX_DEBUG", "0") == "1":
        pytest.skip("the debug library raises at the launch (test_debug_checks_gpu.py)")
    K.debug_errors()  # (clear)
    try:
        for C in (10, 17):
            B, N1, Kd = 8, 48, 200
            bad = {2: C, 5: -1}
            case = f"label C{C}"
            lm, z, t = run_mlp(f"{case} mlp", B, Kd, N1, C, 0, lf32=True, label_fix=bad)  # (all checks, vs the rule)
            errs = K.debug_errors()
            assert errs and errs[0][0] == "loss" and errs[0][1] >= 2, errs
            gs = 1.0 / B
            ref = loss_reference(0, z, t, gs)
            lse = torch.logsumexp(z.double(), 1)
            valid = torch.tensor([r not in bad for r in range(B)])
            want = ((lse - z.double()[torch.arange(B), t.clamp(0, C - 1)]) * valid + lse * ~valid).sum() * gs
            assert abs(float(ref[0]) - float(want)) <= 1e-12 * abs(float(want))
            losses = {"mlp_head": lm}
            # head_ce_k on the same logits (not forward): dl shows in db = sum dl and dw
            gen = _gen(case)
            h, w, _ = head_operands(0, B, C, 24, gen)
            DW, DB = Frame((C, 24), f32, torch.zeros(C, 24)), Frame((C,), f32, torch.zeros(C))
            ls, cor, Lg = Frame((1,), f32), Frame((1,), torch.int32), Frame((B, C), f32, z)
            dh = K.head_ce(0, Lg.v, t.to(dev), h.to(dev), w.to(dev), DW.v, DB.v, gs, ls.v, cor.v)
            errs = K.debug_errors()
            assert errs and errs[0][0] == "loss", errs
            fails = []
            check_head(fails, f"{case} head_ce", 0, z, t, gs, h, w, None,
                       (ls.host().item(), cor.host().item(), DW.host(), DB.host(), dh.cpu()), torch.zeros(C, 24),
                       torch.zeros(C))
            assert not fails, fails
            assert all(fr.intact() for fr in (DW, DB, ls, cor, Lg))
            losses["head_ce"] = ls.host().item()
            # loss_k: dl itself
            for tag, env in (("loss_k", ""), ("loss_k per wave", "loss_thread")):
                monkeypatch.setenv("HOPSX_DISABLE", env)
                D, ls, cor = Frame((B, C), f32), Frame((1,), f32), Frame((1,), torch.int32)
                K.loss_fwd_bwd(0, Lg.v, t.to(dev), gs, ls.v, cor.v, D.v)
                errs = K.debug_errors()
                assert errs and errs[0][0] == "loss" and errs[0][1] == 2, errs
                yard = loss_reference(0, z, t, gs, dtype=f32)
                fails = []
                check_loss(fails, f"{case} {tag}", ls.host().item(), ref[0], yard[0], term_scales(0, z, t, gs)[0])
                check32(fails, f"{case} {tag}", "dl", D.host(), ref[2], yard[2], scale=gs)
                bad_rows = torch.tensor(sorted(bad))
                check32(fails, f"{case} {tag}", "dl bad rows", D.host()[bad_rows],
                        torch.softmax(z.double(), 1)[bad_rows] * gs, yard[2][bad_rows], scale=gs)
                assert not fails, fails
                assert cor.host().item() == ref[1] == int(((z.argmax(1) == t) & valid).sum())
                assert all(fr.intact() for fr in (D, ls, cor, Lg))
                losses[tag] = ls.host().item()
            tol = 4 * ULP32 * term_scales(0, z, t, gs)[0]
            assert max(losses.values()) - min(losses.values()) <= tol, (losses, float(ref[0]))
    finally:
        K.debug_errors()  # drain: later tests see no record
