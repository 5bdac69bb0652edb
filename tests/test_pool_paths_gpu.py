"""The ten kernels of csrc/ops/pool.hip behind their four launchers against the plain fp64 references of
hops_examples_amd.ops.functional (``pool_reference`` / ``pool_bwd_reference`` / ``gap_reference`` /
``gap_bwd_reference``, the Dropout mask from ``dropout_keep_reference``), each case on the launcher path it names
(``kernels.maxpool_fwd_path`` / ``maxpool_bwd_path``: 0 scalar, 1 general vector, 2 non-overlapping fast).

Operands are built on the host from a seeded generator (x on a 1/8 grid, ReLU outputs with their zeros: ties of
the window maximum are everywhere); every output lives inside a larger buffer whose sentinel bands must stay
untouched, dx starts as bf16 NaN, inputs must be unchanged, and a second launch must reproduce y, argmax and dx
bit for bit.

How an output is compared (all derived, nothing tuned):

* forward without dropout: y and argmax bit-identical to the reference (a maximum of bf16 values is one of them);
* forward with dropout: dropped elements (host mask) are +0, kept ones satisfy |y - ref64| <= 2^-8 |ref64| with
  ref64 = max x float32(1 / (1 - p)): one bf16 rounding, the fp32 product is far below it;
* dx: bit-identical to bf16(ref64) when every input pixel receives at most one term, there is no dropout and act
  is none or relu; otherwise |dx - ref64| <= 2^-8 |ref64| + T 2^-23 sum|terms|, T = ceil(KH / sh) ceil(KW / sw)
  the number of windows that can cover a pixel;
* colsum: (colsum - old) against the reference increment, the rule of test_loss_paths_gpu.py for float-atomic
  partial sums: within MARGIN = 8 x the error of the fp32 torch evaluation of the same reference, that yardstick
  floored at 1 + 0.29 sqrt(n - 1) fp32 ulp of sum|g| + |old|; n = the partials arriving at the channel: the
  workgroups' global atomics plus the LDS atomics of one workgroup (deterministic mode: the B H W rows);
* exact twins: every backward case again with integer dy (|v| <= 8), an integer pre-fill of colsum and drop_p 0.5
  where the case has dropout (scale exactly 2): every partial sum is an integer below 2^24 in any order, so dx
  must equal bf16(ref64) and colsum must equal old + increment EXACTLY on every path.  (sigmoid / tanh cases run
  their twin with relu on the same x: act' must be 0 or 1 for the sums to stay integers.)  Global average: integer
  x with HW a power of two gives exactly the bf16 rounding of the exact mean;
* cross-path: aligned C % 8 == 0 cases run again under HOPSX_DISABLE=pool8 and =pool8,poolv; the path functions
  must report the fallback, y / argmax / dx must be bit-identical across the paths, colsum follows its rule;
* global average, random inputs: |y - ref64| <= 2^-8 |ref64| + HW 2^-23 mean|x|; backward
  |dx - ref64| <= (2^-8 + 2^-22) |ref64| (the rounded 1 / HW and one product).

Every check prints ``POOLERR <case> <output> ...``.

Defect found by this file: windows of more than 256 taps (17x17) were accepted by the scalar kernels, which
stored the tap index truncated to a byte; test_window_over_256_taps_is_refused caught it (the launchers now return
-2 before anything is launched, hopsx_maxpool2d_*_path).

Measured on an MI355X, release build: worst ratio error / bound per kernel and output over this file's cases
(dx: only the cases under the tolerance rule; exact comparisons have no ratio).

  kernel (path)              output          rule       checks  worst ratio
  maxpool_fwd8_k (2)         y, argmax       exact          44  no mismatch
  maxpool_fwd8_k (2)         y, dropout      2^-8           15  0.853
  maxpool_fwdv_k (1)         y, argmax       exact         122  no mismatch
  maxpool_fwdv_k (1)         y, dropout      2^-8           32  0.853
  maxpool_fwd_k  (0)         y, argmax       exact         202  no mismatch
  maxpool_fwd_k  (0)         y, dropout      2^-8           62  0.853
  maxpool_bwd8_k (2)         dx              exact          38  no mismatch  (28 of them integer twins)
  maxpool_bwd8_k (2)         dx              tolerance      18  0.988
  maxpool_bwd8_k (2)         colsum          8 x yard       32  0.41   (grid-stride case: 0.01)
  maxpool_bwd8_k (2)         colsum, twin    exact          32  no mismatch
  maxpool_bwdv_k (1)         dx              exact          81  no mismatch  (65 twins)
  maxpool_bwdv_k (1)         dx              tolerance      49  0.996
  maxpool_bwd_k  (0)         dx              exact         177  no mismatch  (145 twins)
  maxpool_bwd_k  (0)         dx              tolerance     114  0.996
  maxpool_bwd_k  (0)         colsum          8 x yard      116  0.54
  maxpool_bwd_k  (0)         colsum, twin    exact         116  no mismatch
  deterministic detour       colsum          8 x yard        6  0.05
  gap_fwdv_k                 y               tolerance      25  0.996  (twins: 12 exact)
  gap_fwd_k                  y               tolerance      13  0.996  (twins: 7 exact)
  gap_bwdv_k                 dx              tolerance      26  0.919  (twins: 13 exact)
  gap_bwd_k                  dx              tolerance      13  0.919  (twins: 7 exact)

(The dx and y ratios near 1 are the bf16 rounding itself: 2^-8 |ref| is reached just above a power of two; the
colsum ratio is error / yardstick, allowed up to MARGIN.)
"""
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.ops import kernels as K  # noqa: E402
from hops_examples_amd.ops.functional import (dropout_keep_reference, gap_bwd_reference, gap_reference,  # noqa: E402
                                              pool_bwd_reference, pool_reference)

dev = torch.device("cuda", 0)
f32, bf, f64, u8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8
MARGIN = 8.0
ULP32 = 2.0 ** -23
PAD = 64  # sentinel elements in front of and behind every framed tensor
SENT = {f32: -7777.25, bf: -3.0, u8: 0xA5}
ACTF = {None: lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.encode()))


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


class Frame:
    """A device buffer of sentinels with the tensor as its view [off, off + n); off = PAD + 1 starts a bf16
    tensor 2 bytes and a uint8 tensor 1 byte past an aligned address."""

    def __init__(self, shape, dtype, init=None, off=PAD):
        self.n, self.off, self.sent = math.prod(shape), off, SENT[dtype]
        self.buf = torch.full((off + self.n + PAD,), self.sent, dtype=dtype, device=dev)
        self.v = self.buf[off:off + self.n].view(shape)
        if init is not None:
            self.v.copy_(init)

    def host(self):
        return self.v.cpu()

    def intact(self):
        a, b = self.buf[:self.off].cpu(), self.buf[self.off + self.n:].cpu()
        return bool((a == self.sent).all()) and bool((b == self.sent).all())


def _ulps(n):
    return ULP32 * (1.0 + 0.29 * math.sqrt(max(n, 1) - 1))


def _line(case, name, text):
    print(f"POOLERR {case} {name} {text}")


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


# ------------------------------------------------------------------------------------------------- comparisons
def check_exact(case, name, got, want):
    bad = int((got.view(torch.int16 if got.element_size() == 2 else got.dtype)
               != want.view(torch.int16 if want.element_size() == 2 else want.dtype)).sum())
    _line(case, name, f"exact mismatches {bad} of {got.numel()}")
    assert bad == 0 and got.dtype == want.dtype and got.shape == want.shape, (case, name, bad)


def check_tol(case, name, got, ref, bound):
    err = (got.double() - ref).abs()
    ok = err <= bound  # (a NaN left in dx compares false)
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf"))[bound > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _line(case, name, f"tolerance worst ratio {worst:.3f} over {got.numel()}")
    assert bool(ok.all()), (case, name, int((~ok).sum()), worst)


def check_colsum(case, name, cs, old, inc64, inc32, absg, n):
    """cs, old fp32 [C] (host); inc64 / inc32: the reference increment in fp64 / fp32; absg: sum |g| per channel."""
    e = (cs.double() - old.double() - inc64).abs()
    y = torch.maximum((inc32.double() - inc64).abs(), _ulps(n) * (absg + old.double().abs()))
    ratio = (e / y.clamp_min(1e-300))[y > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _line(case, name, f"kernel {float(e.max()):.3e} yardstick {float(y.max()):.3e} ratio {worst:.2f} n {n}")
    assert bool((e <= MARGIN * y).all()), (case, name, worst)


# ------------------------------------------------------------------------------------------------------ max-pool
_MASK_TIED = []


def keep_mask(rng, salt, shape, p):
    """The host statement of the mask; once per process it is tied to the stand-alone dropout kernel."""
    m = dropout_keep_reference(rng.cpu(), salt, shape, p)
    if not _MASK_TIED:
        k = (K.dropout(torch.ones(shape, device=dev, dtype=bf), p, rng, salt) != 0).cpu()
        assert torch.equal(m, k), "dropout_keep_reference != K.dropout(ones) != 0"
        _MASK_TIED.append(1)
    return m


def make_x(gen, shape, act):
    """The pool input: an activation's output.  none / relu: multiples of 1/8 (exact in bf16, ties everywhere)."""
    if math.prod(shape) > (1 << 22):  # (the large cases: the same grid, drawn as integers)
        z = torch.randint(-40, 41, shape, generator=gen, dtype=torch.int8).to(bf).float() / 8
    else:
        z = (torch.randn(shape, generator=gen) * 8).round() / 8 + 0.0  # (+ 0.0: no negative zeros)
    return ACTF[act](z).to(bf)


def bwd_partials(path, B, H, W, C, OH, OW):
    """n of the colsum rule: the workgroups adding to a channel plus the LDS adds of one of them."""
    if path == 2:
        wgs = min(-(-(B * OH * OW * (C // 8)) // 256), 1024)
        return wgs + max(256 // (C // 8), 1)
    total = B * H * W * C
    wgs = min(-(-total // 256), 1024)
    iters = -(-total // (wgs * 256))
    return wgs + -(-256 // C) * iters


class Op:
    """The operands and references of one case, computed once and shared by every path it runs on."""

    def __init__(self, case, B, H, W, C, k, s=None, p=0, act=None, with_x=True, drop_p=0.0, colsum=False, old=True,
                 mis=False, dead=False, inf=False, backward=True, ref_dtype=f64, edit=None):
        self.case, self.k, self.s, self.p = case, _pair(k), _pair(s if s is not None else k), _pair(p)
        self.B, self.H, self.W, self.C = B, H, W, C
        self.act, self.with_x, self.drop_p, self.colsum = act, with_x, drop_p, colsum
        self.mis, self.backward = mis, backward
        gen = _gen(case)
        self.x = make_x(gen, (B, H, W, C), act)
        if edit:
            edit(self.x)
        if inf:  # one window entirely -inf, one holding +inf (unpadded windows)
            self.x[0, :self.k[0], :self.k[1], 0] = float("-inf")
            self.x[B - 1, self.s[0] + 1, self.s[1], C - 1] = float("inf")
        self.OH, self.OW = K.pool_out(H, W, self.k, self.s, self.p)
        self.yshape = (B, self.OH, self.OW, C)
        self.T = -(-self.k[0] // self.s[0]) * -(-self.k[1] // self.s[1])
        self.salt = zlib.crc32(case.encode()) & 0xFFFFFFFF
        self.rng = torch.tensor([zlib.crc32(case.encode()) + 11, 5], device=dev, dtype=torch.int64)
        self.y_ref, self.am_ref = pool_reference(self.x, self.k, self.s, self.p, dtype=ref_dtype)
        self.masks = {}
        if not backward:
            return
        self.am_in = self.am_ref.clone()
        if dead:  # the conv epilogue's dead-ReLU mark on a third of the outputs
            self.am_in[torch.rand(self.yshape, generator=gen) < 0.33] = 0xFF
        self.dy = {"rand": torch.randn(self.yshape, generator=gen).to(bf),
                   "twin": torch.randint(-8, 9, self.yshape, generator=gen).to(bf)}
        self.old = {"rand": (torch.randn(C, generator=gen) * 3 if old else torch.zeros(C)),
                    "twin": (torch.randint(-100, 101, (C,), generator=gen).float() if old else torch.zeros(C))}
        self.refs = {}

    def mask(self, p):
        if p and p not in self.masks:
            self.masks[p] = keep_mask(self.rng, self.salt, self.yshape, p)
        return self.masks.get(p)

    def bwd_ref(self, kind):
        if kind not in self.refs:
            p = self.drop_p if kind == "rand" else (0.5 if self.drop_p else 0.0)
            act = self.act if kind == "rand" or self.act in (None, "relu") else "relu"
            args = (self.am_in, self.x.shape, self.k, self.s, self.p)
            kw = dict(x=self.x if self.with_x else None, act=act, mask=self.mask(p), drop_p=p)
            dy = self.dy[kind]
            dx64, inc64 = pool_bwd_reference(dy, *args, **kw)
            terms, absg = pool_bwd_reference(dy.abs(), *args, **kw)
            inc32 = pool_bwd_reference(dy, *args, dtype=f32, **kw)[1] if self.colsum else None
            self.refs[kind] = (p, act, dx64, inc64, terms, absg, inc32)
        return self.refs[kind]


def run_forward(op, fpath):
    off = PAD + int(op.mis)
    X = Frame(op.x.shape, bf, op.x, off=off)
    assert (X.v.data_ptr() % 16 != 0) == op.mis
    outs = []
    for rep in range(2):
        Y, AM = Frame(op.yshape, bf, off=off), Frame(op.yshape, u8, off=off)
        kw = dict(out=Y.v, argmax=AM.v, drop_p=op.drop_p, rng=op.rng if op.drop_p else None, salt=op.salt)
        got = K.maxpool_fwd_path(X.v, op.k, op.s, op.p, **kw)
        assert got == fpath, (op.case, "forward path", got, fpath)
        K.maxpool2d_fwd(X.v, op.k, op.s, op.p, **kw)
        torch.cuda.synchronize()
        assert Y.intact() and AM.intact() and X.intact(), (op.case, "sentinels")
        outs.append((Y.host(), AM.host()))
    assert bits_equal(X.host(), op.x), (op.case, "x changed")
    y, am = outs[0]
    assert bits_equal(y, outs[1][0]) and bits_equal(am, outs[1][1]), (op.case, "second forward launch differs")
    tag = f"{op.case} fwd{fpath}"
    check_exact(tag, "argmax", am, op.am_ref)
    if not op.drop_p:
        check_exact(tag, "y", y, op.y_ref.to(bf))
    else:
        mask = op.mask(op.drop_p)
        scale = (1.0 / (1.0 - torch.tensor(op.drop_p, dtype=f32))).double()
        ref = op.y_ref.double() * scale
        dropped = y.view(torch.int16)[~mask]
        assert torch.count_nonzero(dropped) == 0, (op.case, "a dropped element is not +0")
        assert int((ref[mask] != 0).sum()) > 0
        assert bool(((y != 0) == (mask & (ref != 0))).all()), (op.case, "kept set != host mask")
        check_tol(tag, "y", y[mask], ref[mask], 2.0 ** -8 * ref[mask].abs())
    return y, am


def run_backward(op, bpath, kinds=("rand", "twin")):
    off = PAD + int(op.mis)
    B, H, W, C = op.x.shape
    res = {}
    X = Frame(op.x.shape, bf, op.x, off=off) if op.with_x else None
    AM = Frame(op.yshape, u8, op.am_in, off=off)
    for kind in kinds:
        p, act, dx64, inc64, terms, absg, inc32 = op.bwd_ref(kind)
        DY = Frame(op.yshape, bf, op.dy[kind], off=off)
        outs = []
        for rep in range(2):
            DX = Frame(op.x.shape, bf, torch.full(op.x.shape, float("nan")), off=off)
            CS = Frame((C,), f32, op.old[kind]) if op.colsum else None
            kw = dict(x=X.v if X else None, act=act or 0, out=DX.v, colsum=CS.v if CS else None, drop_p=p,
                      rng=op.rng if p else None, salt=op.salt)
            got = K.maxpool_bwd_path(DY.v, AM.v, op.x.shape, op.k, op.s, op.p, **kw)
            assert got == bpath, (op.case, kind, "backward path", got, bpath)
            K.maxpool2d_bwd(DY.v, AM.v, op.x.shape, op.k, op.s, op.p, **kw)
            torch.cuda.synchronize()
            assert DX.intact() and DY.intact() and AM.intact() and (CS is None or CS.intact()), (op.case, "sentinels")
            assert X is None or X.intact()
            outs.append((DX.host(), CS.host() if CS else None))
        assert bits_equal(DY.host(), op.dy[kind]) and bits_equal(AM.host(), op.am_in), (op.case, "inputs changed")
        assert X is None or bits_equal(X.host(), op.x)
        dx, cs = outs[0]
        assert bits_equal(dx, outs[1][0]), (op.case, kind, "second backward launch differs")
        tag = f"{op.case} bwd{bpath} {kind}"
        n = bwd_partials(bpath, B, H, W, C, op.OH, op.OW)
        if kind == "twin":
            check_exact(tag, "dx", dx, dx64.to(bf))
            for c in [o[1] for o in outs if o[1] is not None]:
                bad = int((c.double() != op.old[kind].double() + inc64).sum())
                _line(tag, "colsum", f"exact mismatches {bad} of {C}")
                assert bad == 0, (tag, "colsum", bad)
        else:
            if op.T == 1 and not p and (act in (None, "relu") or not op.with_x):
                check_exact(tag, "dx", dx, dx64.to(bf))
            else:
                check_tol(tag, "dx", dx, dx64, 2.0 ** -8 * dx64.abs() + op.T * ULP32 * terms)
            for c in [o[1] for o in outs if o[1] is not None]:
                check_colsum(tag, "colsum", c, op.old[kind], inc64, inc32, absg, n)
        res[kind] = (dx, cs)
    return res


def run_case(monkeypatch, op, fpath, bpath, cross=None):
    """The case on its own path, then (cross) on the fallbacks: pool8 off, then pool8 and poolv off."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    y, am = run_forward(op, fpath)
    res = run_backward(op, bpath) if op.backward else None
    if cross is None:
        cross = op.C % 8 == 0 and not op.mis and (fpath > 0 or bpath > 0)
    if not cross:
        return
    taps = op.k[0] * op.k[1]
    steps = [("pool8,poolv", 0, 0)]
    if 2 in (fpath, bpath):
        steps.insert(0, ("pool8", 1 if taps <= 255 else 0, 0 if op.colsum or taps > 255 else 1))
    for env, fp, bp in steps:
        monkeypatch.setenv("HOPSX_DISABLE", env)
        y2, am2 = run_forward(op, fp)
        assert bits_equal(y, y2) and bits_equal(am, am2), (op.case, env, "forward differs across paths")
        if op.backward:
            res2 = run_backward(op, bp)
            for kind in res:
                assert bits_equal(res[kind][0], res2[kind][0]), (op.case, env, kind, "dx differs across paths")
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)


# ---- the non-overlapping fast path
FAST_GEOMS = [(7, 10, (2, 2)), (9, 9, (2, 2)), (8, 6, (2, 2)), (10, 11, (3, 3)), (9, 10, (2, 3)), (2, 2, (2, 2))]
ACT_OPTS = [(None, True), ("relu", True), ("sigmoid", True), ("tanh", True), ("relu", False)]  # (act, x given)
DROPS = (0.0, 0.3, 0.5)


def _fast_cases():
    i = 0
    for (H, W, k) in FAST_GEOMS:
        for C in (8, 64, 256, 2048):
            act, with_x = ACT_OPTS[i % 5]
            drop = DROPS[(i + i // 3) % 3] if with_x else 0.0
            colsum = (i % 2 == 0) or k == (3, 3)  # (9 taps, few outputs and no colsum: few_big, the general kernel)
            yield pytest.param(H, W, k, C, act, with_x, drop, colsum, i % 4 < 2,
                               id=f"{H}x{W}-k{k[0]}x{k[1]}-C{C}-{act}{'' if with_x else '-nox'}-p{drop}-cs{int(colsum)}")
            i += 1


FAST = list(_fast_cases())


def test_fast_case_coverage():
    v = [c.values for c in FAST]
    assert {(a[4], a[5]) for a in v} == set(ACT_OPTS) and {a[6] for a in v} == set(DROPS)
    assert {a[7] for a in v} == {True, False} and {a[8] for a in v if a[7]} == {True, False}
    for act, _ in ACT_OPTS[:4]:
        assert {a[7] for a in v if a[4] == act and a[5]} == {True, False}, act
    assert any(a[6] and a[7] for a in v) and any(a[6] and not a[7] for a in v)


@pytest.mark.parametrize("H,W,k,C,act,with_x,drop,colsum,old", FAST)
def test_maxpool_fast_path(monkeypatch, H, W, k, C, act, with_x, drop, colsum, old):
    """maxpool_fwd8_k / maxpool_bwd8_k: remainder rows and columns (7x10, 9x9, 10x11, 9x10), none (8x6), a single
    output pixel (2x2), G = C / 8 = 1, 8, 32, 256; then the same operands on the general and scalar kernels."""
    B = 3 if C <= 64 else 2
    op = Op(f"fast {H}x{W} k{k} C{C} {act} x{int(with_x)} p{drop} cs{int(colsum)}", B, H, W, C, k, act=act,
            with_x=with_x, drop_p=drop, colsum=colsum, old=old)
    run_case(monkeypatch, op, 2, 2)




_OPS = {}


def _shared(key, make):
    """Operands and references of a large case, built once for the tests that share it."""
    if key not in _OPS:
        _OPS[key] = make()
    return _OPS[key]


@pytest.mark.parametrize("kind", ("twin", "rand"))
def test_bwd8_grid_stride_loop(monkeypatch, kind):
    """B 8, 64x64, k 2, C 512 with colsum: 524,288 thread items over the 1,024 workgroups the grid is capped at,
    so every thread takes two; its register column sums stay under one channel group only because the stride is
    a multiple of C / 8."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    assert 8 * 32 * 32 * (512 // 8) == 2 * 1024 * 256
    op = _shared("bwd8 stride", lambda: Op("bwd8 stride", 8, 64, 64, 512, 2, act="relu", drop_p=0.5, colsum=True))
    if kind == "twin":
        run_forward(op, 2)
    run_backward(op, 2, kinds=(kind,))


@pytest.mark.parametrize("B,H,W,C,fpath", [(17, 64, 64, 1024, 2), (4, 180, 180, 70, 0)], ids=("vector", "scalar"))
def test_forward_grid_stride_loop(monkeypatch, B, H, W, C, fpath):
    """Just above the forward's cap of 8,192 workgroups x 256 threads: 2,228,224 vector items, 2,268,000 scalar."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    assert B * (H // 2) * (W // 2) * (C // 8 if fpath else C) > 8192 * 256
    run_forward(Op(f"fwd stride {fpath}", B, H, W, C, 2, backward=False, ref_dtype=f32), fpath)


def test_few_big_reroute(monkeypatch):
    """k 4 on 22x23, C 64 (the E1 model's pool): without colsum the backward goes to maxpool_bwdv_k, which writes
    the remainder rows and columns as zeros itself; with colsum it stays on maxpool_bwd8_k; same dx."""
    a = Op("few_big", 2, 22, 23, 64, 4, act="relu")
    b = Op("few_big", 2, 22, 23, 64, 4, act="relu", colsum=True)
    assert bits_equal(a.x, b.x) and bits_equal(a.dy["rand"], b.dy["rand"])
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    run_forward(a, 2)
    ra, rb = run_backward(a, 1), run_backward(b, 2)
    for kind in ra:
        assert bits_equal(ra[kind][0], rb[kind][0]), kind
        assert torch.count_nonzero(ra[kind][0][:, 20:]) == 0 and torch.count_nonzero(ra[kind][0][:, :, 20:]) == 0
    run_case(monkeypatch, a, 2, 1)


@pytest.mark.parametrize("B,bpath", [(16, 2), (15, 1)])
def test_few_big_boundary(monkeypatch, B, bpath):
    """B OH OW C / 8 = 32,768 at B 16 (48x48, k 3, C 64): not few_big; 30,720 at B 15: few_big."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    assert 16 * 16 * 16 * 8 == 32768
    run_backward(Op(f"few_big edge B{B}", B, 48, 48, 64, 3), bpath)


# ---- the general vector path
GV_GEOMS = [(3, 2, 1), (3, 1, 1), (2, 1, 0), (3, 3, 1), ((3, 2), (2, 1), (1, 0)), (5, 2, 2), (7, 1, 3), (2, 3, 0)]


def _gv_cases():
    i = 0
    for (k, s, p) in GV_GEOMS:
        for (H, W) in ((8, 9), (8, 9)) if k == 7 else ((7, 10), (15, 9)):
            for C in (8, 24, 40):
                yield pytest.param(H, W, k, s, p, C, (None, "relu")[i % 2], (0.0, 0.3)[(i // 2 + i // 6) % 2],
                                   id=f"{H}x{W}-k{k}-s{s}-p{p}-C{C}-{i}")
                i += 1
    for i, (H, W) in enumerate(((7, 10), (15, 9))):  # non-overlapping, but G = 3 does not divide 256
        yield pytest.param(H, W, 2, 2, 0, 24, (None, "relu")[i], (0.3, 0.0)[i], id=f"{H}x{W}-k2-s2-C24")


GV = list(_gv_cases())


def test_general_case_coverage():
    v = [c.values for c in GV]
    for g in GV_GEOMS:
        mine = [a for a in v if a[2:5] == g]
        assert {(a[6], a[7]) for a in mine} == {(None, 0.0), (None, 0.3), ("relu", 0.0), ("relu", 0.3)}, g
        assert {a[5] for a in mine} == {8, 24, 40}


@pytest.mark.parametrize("H,W,k,s,p,C,act,drop", GV)
def test_maxpool_general_vector_path(monkeypatch, H, W, k, s, p, C, act, drop):
    """maxpool_fwdv_k / maxpool_bwdv_k: overlapping, padded, strided past the window, non-square; then the same
    operands on the scalar kernels."""
    op = Op(f"general {H}x{W} k{k} s{s} p{p} C{C} {act} p{drop}", 3 if C == 8 else 2, H, W, C, k, s, p, act=act,
            drop_p=drop)
    run_case(monkeypatch, op, 1, 1)


# ---- the scalar path
SC_GEOMS = [(7, 10, 2, 2, 0), (9, 9, 2, 2, 0), (10, 11, 3, 3, 0), (9, 10, (2, 3), (2, 3), 0), (7, 10, 3, 2, 1),
            (15, 9, 3, 1, 1), (15, 9, (3, 2), (2, 1), (1, 0)), (7, 10, 5, 2, 2), (8, 9, 7, 1, 3), (7, 10, 2, 3, 0)]


def _scalar_cases():
    i = 0
    for (H, W, k, s, p) in SC_GEOMS:
        for C in (1, 3, 10, 60, 300):
            act, with_x = ACT_OPTS[(i + i // 5) % 5]
            drop = DROPS[(i + i // 3) % 3] if with_x else 0.0
            yield pytest.param(H, W, k, s, p, C, act, with_x, drop, i % 2 == 0, i % 4 < 2,
                               id=f"{H}x{W}-k{k}-s{s}-p{p}-C{C}-{act}{'' if with_x else '-nox'}-p{drop}-cs{i % 2 == 0}")
            i += 1


@pytest.mark.parametrize("H,W,k,s,p,C,act,with_x,drop,colsum,old", list(_scalar_cases()))
def test_maxpool_scalar_path(monkeypatch, H, W, k, s, p, C, act, with_x, drop, colsum, old):
    """maxpool_fwd_k / maxpool_bwd_k at C % 8 != 0 (300: more channels than threads in a workgroup)."""
    op = Op(f"scalar {H}x{W} k{k} s{s} p{p} C{C} {act} x{int(with_x)} p{drop} cs{int(colsum)}", 2, H, W, C, k, s, p,
            act=act, with_x=with_x, drop_p=drop, colsum=colsum, old=old)
    run_case(monkeypatch, op, 0, 0)


def test_scalar_backward_over_its_grid_cap(monkeypatch):
    """B 3, 40x40, C 60: 288,000 elements over the 1,024 workgroups the scalar backward is capped at."""
    assert 3 * 40 * 40 * 60 > 1024 * 256
    run_case(monkeypatch, Op("scalar cap", 3, 40, 40, 60, 2, act="relu", drop_p=0.3, colsum=True), 0, 0)


def test_colsum_with_overlapping_windows_is_scalar(monkeypatch):
    """C % 8 == 0, aligned, k 3 s 2 p 1 with colsum: no vector backward has a column sum, so maxpool_bwd_k."""
    run_case(monkeypatch, Op("overlap colsum", 2, 7, 10, 64, 3, 2, 1, act="relu", drop_p=0.3, colsum=True), 1, 0)


@pytest.mark.parametrize("k,s,p,colsum", [(2, 2, 0, True), (3, 2, 1, False)])
def test_misaligned_operands_are_scalar(monkeypatch, k, s, p, colsum):
    """C 64 with x / y / dy / dx one element and argmax one byte into their storage: neither vector kernel."""
    run_case(monkeypatch, Op(f"misaligned k{k}", 2, 7, 10, 64, k, s, p, act="relu", drop_p=0.3, colsum=colsum,
                             mis=True), 0, 0)


# ---- the 1-byte argmax
def test_window_of_256_taps(monkeypatch):
    """16x16 on 16x17: tap indices 0 .. 255 fit the byte; the vector kernels stop at 255 taps, so path 0 at C 8."""
    def last_tap(x):
        x[0, 15, 15, 1] = 100.0

    op = Op("256 taps", 2, 16, 17, 8, 16, act="relu", colsum=True, edit=last_tap)
    assert int(op.am_ref[0, 0, 0, 1]) == 255
    run_case(monkeypatch, op, 0, 0)


@pytest.mark.parametrize("C", (8, 3))
def test_window_over_256_taps_is_refused(monkeypatch, C):
    """17x17 = 289 taps: both launchers return -2 before anything is launched."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    gen = _gen("289 taps")
    k = (17, 17)
    X = Frame((1, 17, 18, C), bf, torch.randn(1, 17, 18, C, generator=gen).to(bf))
    Y, AM, DX, CS = Frame((1, 1, 1, C), bf), Frame((1, 1, 1, C), u8), Frame((1, 17, 18, C), bf), Frame((C,), f32)
    before = [fr.buf.cpu() for fr in (Y, AM, DX, CS)]
    assert K.maxpool_fwd_path(X.v, k, k, (0, 0), out=Y.v, argmax=AM.v) == -2
    with pytest.raises(RuntimeError, match="maxpool_fwd failed with hipError -2$"):
        K.maxpool2d_fwd(X.v, k, k, (0, 0), out=Y.v, argmax=AM.v)
    for cs in (None, CS.v):
        assert K.maxpool_bwd_path(Y.v, AM.v, X.v.shape, k, k, (0, 0), x=X.v, act="relu", out=DX.v, colsum=cs) == -2
        with pytest.raises(RuntimeError, match="maxpool_bwd failed with hipError -2$"):
            K.maxpool2d_bwd(Y.v, AM.v, X.v.shape, k, k, (0, 0), x=X.v, act="relu", out=DX.v, colsum=cs)
    torch.cuda.synchronize()
    for fr, o in zip((Y, AM, DX, CS), before):
        assert bits_equal(fr.buf.cpu(), o)


@pytest.mark.parametrize("k,s,p,C,path", [(2, 2, 0, 64, 2), (3, 2, 1, 8, 1)])
def test_dead_relu_argmax_gives_no_gradient(monkeypatch, k, s, p, C, path):
    """argmax bytes of 0xFF (the conv epilogue's mark of a dead ReLU) on the vector kernels: that output's gradient
    goes nowhere.  (The scalar kernel is left out: the debug build's bound check rejects the value by design.)"""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    op = Op(f"dead k{k}", 2, 7, 10, C, k, s, p, dead=True)
    assert int((op.am_in == 0xFF).sum()) > 0 and int((op.am_ref == 0xFF).sum()) == 0
    run_backward(op, path)


def test_infinite_inputs(monkeypatch):
    """One window entirely -inf (argmax 0, y -inf) and one holding +inf, on all three forward kernels."""
    op = Op("inf", 2, 8, 6, 8, 2, inf=True, backward=False)
    assert op.y_ref[0, 0, 0, 0] == float("-inf") and int(op.am_ref[0, 0, 0, 0]) == 0
    assert op.y_ref[1, 1, 1, 7] == float("inf")
    run_case(monkeypatch, op, 2, 2)


# ---------------------------------------------------------------------------------------- global average pool
def run_gap(case, B, H, W, C, mis=False, twin=False, forward=True):
    gen, HW, off = _gen(case), H * W, PAD + int(mis)
    draw = (lambda sh: torch.randint(-8, 9, sh, generator=gen).to(bf)) if twin else \
        (lambda sh: torch.randn(sh, generator=gen).to(bf))
    x, dy = draw((B, H, W, C)), draw((B, C))
    X, DY = Frame(x.shape, bf, x, off=off), Frame(dy.shape, bf, dy, off=off)
    assert (X.v.data_ptr() % 16 != 0) == mis
    tag = f"{case} {'vec' if C % 8 == 0 and not mis else 'scalar'}{' twin' if twin else ''}"
    if forward:
        ys = []
        for rep in range(2):
            Y = Frame((B, C), bf, off=off)
            K.gap_fwd(X.v, out=Y.v)
            torch.cuda.synchronize()
            assert Y.intact() and X.intact(), case
            ys.append(Y.host())
        assert bits_equal(ys[0], ys[1]) and bits_equal(X.host(), x), case
        ref = gap_reference(x)
        if twin:
            check_exact(tag, "gap y", ys[0], ref.to(bf))
        else:
            check_tol(tag, "gap y", ys[0], ref, 2.0 ** -8 * ref.abs() + HW * ULP32 * x.double().abs().mean((1, 2)))
    dxs = []
    for rep in range(2):
        DX = Frame(x.shape, bf, torch.full(x.shape, float("nan")), off=off)
        K.gap_bwd(DY.v, x.shape, out=DX.v)
        torch.cuda.synchronize()
        assert DX.intact() and DY.intact(), case
        dxs.append(DX.host())
    assert bits_equal(dxs[0], dxs[1]) and bits_equal(DY.host(), dy), case
    ref = gap_bwd_reference(dy, x.shape)
    if twin:
        check_exact(tag, "gap dx", dxs[0], ref.to(bf))
    else:
        check_tol(tag, "gap dx", dxs[0], ref, (2.0 ** -8 + 2.0 ** -22) * ref.abs())


GAP_HW = [(1, 1), (1, 3), (2, 2), (7, 1), (7, 7), (4, 16)]


@pytest.mark.parametrize("C", (8, 16, 24, 2056, 10, 300))
def test_global_avg_pool(C):
    """gap_fwdv_k / gap_bwdv_k (C % 8 == 0; 2056: G = 257, a second and mostly idle blockIdx.x) and gap_fwd_k /
    gap_bwd_k (10; 300: a second trip of the channel loop); HW % 4 != 0 ends in the tail loop of gap_fwdv_k.
    HW 1, 4, 64 again with integer x: exactly the bf16 rounding of the exact mean."""
    for i, (H, W) in enumerate(GAP_HW):
        B = (1, 5)[(i + C // 8) % 2]
        run_gap(f"gap B{B} {H}x{W} C{C}", B, H, W, C)
        if (H * W) & (H * W - 1) == 0:
            run_gap(f"gap B{6 - B} {H}x{W} C{C}", 6 - B, H, W, C, twin=True)


def test_global_avg_pool_long_window_and_misaligned():
    run_gap("gap 112x112", 2, 112, 112, 8)
    run_gap("gap misaligned", 5, 7, 7, 64, mis=True)
    run_gap("gap misaligned twin", 1, 4, 16, 64, mis=True, twin=True)


def test_global_avg_pool_backward_grid_stride_loop():
    """B 256, HW 49, C 2048: 3,211,264 vector items over the cap of 8,192 workgroups x 256."""
    assert 256 * 49 * 256 > 8192 * 256
    run_gap("gap bwd stride", 256, 7, 7, 2048, forward=False)
    run_gap("gap bwd stride twin", 256, 8, 8, 2048, twin=True, forward=False)


# ------------------------------------------------------------------------------------------ deterministic mode
_CHILD = """
import sys
import torch
from hops_examples_amd.ops import kernels as K
dev = torch.device("cuda", 0)
cases, out = torch.load(sys.argv[1]), {}
for name, c in cases.items():
    dy, am, x, runs = c["dy"].to(dev), c["am"].to(dev), c["x"].to(dev), []
    for rep in range(2):
        dx = torch.full(c["shape"], float("nan"), device=dev, dtype=torch.bfloat16)
        cs = c["old"].to(dev)
        kw = dict(x=x, act="relu", out=dx, colsum=cs)
        path = K.maxpool_bwd_path(dy, am, c["shape"], c["k"], c["s"], c["p"], **kw)
        K.maxpool2d_bwd(dy, am, c["shape"], c["k"], c["s"], c["p"], **kw)
        torch.cuda.synchronize()
        runs.append((dx.cpu(), cs.cpu(), path))
    out[name] = runs
torch.save(out, sys.argv[2])
"""


def test_deterministic_mode_detour(monkeypatch, tmp_path):
    """HOPSX_DETERMINISTIC=1 is latched per process: one child runs a fast-path and a scalar-path backward with a
    pre-filled colsum twice each.  Its dx is the parent's bit for bit, its colsum repeats bit for bit and is the
    sum of the STORED bf16 dx (what that mode adds up) within the colsum rule."""
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)
    ops = {"fast": (Op("det fast", 2, 7, 10, 64, 2, act="relu", colsum=True), 2),
           "scalar": (Op("det scalar", 2, 7, 10, 10, 3, 2, 1, act="relu", colsum=True), 0)}
    cases = {n: dict(dy=o.dy["rand"], am=o.am_in, x=o.x, old=o.old["rand"], shape=tuple(o.x.shape), k=o.k, s=o.s,
                     p=o.p) for n, (o, _) in ops.items()}
    torch.save(cases, tmp_path / "in.pt")
    (tmp_path / "child.py").write_text(_CHILD)
    env = dict(os.environ, HOPSX_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("HOPSX_DISABLE", None)
    r = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "in.pt"), str(tmp_path / "out.pt")],
                       env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = torch.load(tmp_path / "out.pt")
    for name, (op, path) in ops.items():
        mine = run_backward(op, path, kinds=("rand",))["rand"][0]
        (dx0, cs0, p0), (dx1, cs1, p1) = got[name]
        assert p0 == p1 == path, (name, p0, p1)
        assert bits_equal(dx0, mine) and bits_equal(dx1, mine), (name, "dx differs from the parent's")
        assert bits_equal(cs0, cs1), (name, "colsum differs between the child's runs")
        B, H, W, C = op.x.shape
        check_colsum(f"det {name}", "colsum", cs0, op.old["rand"], dx0.double().sum((0, 1, 2)),
                     dx0.float().sum((0, 1, 2)), dx0.double().abs().sum((0, 1, 2)), B * H * W)
