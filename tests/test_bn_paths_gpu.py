"""The thirteen kernels of csrc/ops/norm.hip behind their five launchers against the plain fp64 references of
hops_examples_amd.ops.functional (``bn_stats_reference`` / ``bn_reference`` / ``bn_bwd_reference``), each case on the
launcher route it names: ``kernels.bn_*_path`` report the launcher's own plan (scalar / defer / selffin / fold / coop
/ apply / refuse plus the grids) and every case asserts it before anything is compared.

Operands are built on the host from a seeded generator; every tensor lives inside a larger buffer whose sentinel
bands must stay untouched, outputs start as NaN, inputs must be unchanged, and after EVERY launch the accumulator
(all BN_NREP x 2C replica floats, the 9 x 32 arrival words and the barrier's count line) is read back and must be
zero.  (The barrier's generation word counts launches by design and its timeout word is read by bn_coop_timeouts.)

The environment knobs HOPSX_BN_DEFER_MAXC / _FOLD_MINC / _MAXG / _APPLY_MAXG / _COOP are latched at their first
use in a process (function-local statics in norm.hip), so every non-default value runs in a fresh child process
that imports this module and runs the same checks; only HOPSX_DISABLE and HOPSX_BN_RPT change in-process.

Each stage is compared with fp64 evaluated from the KERNEL'S OWN upstream outputs (all derived, nothing tuned):

* sums (mean * M, ws[0:C], ws[C:2C]): within MARGIN = 8 x the error of the fp32 torch evaluation of the same
  reference, that yardstick floored at 1 + 0.29 sqrt(n - 1) fp32 ulp of the sum of magnitudes; n = the partials
  arriving at a channel: the reduction's workgroups plus the row partials folded inside one (256 / (C / 8) lanes, 4
  waves for the scalar kernels) plus the BN_NREP replica rows; deterministic mode: the workgroups.
* rstd: var_k = 1 / rstd^2 - eps against the fp64 variance.  var = q / M - (s / M)^2, so to first order
  |dvar| <= Bq / M + 2 |mean| Bs / M with Bs, Bq the two sums' bounds above; the finisher's own fp32 steps (s / M,
  q / M, mu * mu, the difference: half an ulp each of q / M + mean^2) add 4 x 2^-24 x 2 (q / M + mean^2), and rsqrtf
  plus the rounding of rstd are 4 ulp of rstd, i.e. 8 ulp of var + eps.
* running statistics: (1 - m) old + m stat with the kernel's published mean resp. the fp64 unbiased variance (M = 1:
  the biased one): 2 fp32 ulp of |(1 - m) old| + |m stat| (1 - m, two products, one sum) + m x the var bound x
  M / (M - 1), and for the variance 1 more ulp of m x unbiased (the M / (M - 1) product and quotient).
* y: |y - ref64| <= 2^-8 |ref64| + 4 x 2^-23 (|x sc| + |sh| + |res|), ref64 from the published mean / rstd;
  inference: ref64 from the given running statistics, so rsqrtf's 4 ulp of sc and the rounding of sc itself act on
  x sc and on mean sc: 6 x 2^-23 (|x sc| + |mean sc| + |beta| + |res|).  ReLU zeros must be +0.
* dres: bit-identical to bf16(dz) for none / relu, 2^-8 |ref| otherwise.
* dx: ref64 = k1 (dz - ws0 / M - xhat ws1 / M) from the published ws, mean and rstd;
  |dx - ref64| <= 2^-8 |ref64| + 6 x 2^-23 |k1| (|dz| + |ws0 / M| + |xhat ws1 / M|): act' (2 roundings), 1 / M and
  its two products, xhat (2), xhat k2, two differences, k1 and the last product are 11 roundings of half an ulp.
* dgamma / dbeta: bit-identical to float32(old + ws) with a non-zero old.
* exact twins: every case again with integer x / dy / residual (|v| <= 8) and act none / relu: all partial sums are
  integers below 2^24, so round(mean * M), ws[0:C] and dbeta - old are EXACT, and mean / rstd / y / dres are
  bit-identical across the vector routes of the case (defer, selffin, fold, the grid-stride knobs, cooperative); dx
  is bit-identical in every channel whose published ws[C:2C] is (see same_backward: sum dz xhat is no integer sum).
* zmask (ReLU, no residual, zbeta = beta): y is a NaN frame on the route the reporter says does not read it; the
  twin's dx and sums equal the y-read result exactly.  dres and dx are compared by VALUE there: a masked negative
  gradient is -0 when act' multiplies it (y route) and +0 when the z test selects it (zmask), both are zero.

Every check prints ``BNERR <case> <route> <output> err bound ratio``.

acc == nullptr (test_null_accumulator) goes through the raw extension: kernels.bn_fwd_train / bn_bwd always pass the
per-width accumulator.

Measured on an MI355X, release build, over this file's cases; a child process's checks count in the same rows as
the parent's (run_child merges them), and test_zz_measured_table prints exactly these rows.  Worst = the worst ratio
error / bound; for the "8 x yard" rule error / yardstick, allowed up to MARGIN = 8.

  kernel                     output           rule                               checks  worst
  bn_apply8_k                y                tolerance                             84  0.996
  bn_apply8_k (infer)        y                tolerance                             12  0.996
  bn_apply_fin8_k            rstd             propagated                           216  0.115
  bn_apply_fin8_k            running_mean     2 ulp                                152  0.438
  bn_apply_fin8_k            running_var      2 ulp + m Bvar                       152  0.341
  bn_apply_fin8_k            y                tolerance                            216  0.996
  bn_apply_k                 y                tolerance                             75  0.996
  bn_apply_k (infer)         y                tolerance                             16  0.991
  bn_bwd_apply8_k            dres             2^-8                                  15  0.996
  bn_bwd_apply8_k            dres             exact                                 51  no mismatch
  bn_bwd_apply8_k            dx               tolerance                            132  0.996
  bn_bwd_apply_fin8_k        dbeta            float32(old + ws)                    124  no mismatch
  bn_bwd_apply_fin8_k        dgamma           float32(old + ws)                    131  no mismatch
  bn_bwd_apply_fin8_k        dres             2^-8                                  11  0.996
  bn_bwd_apply_fin8_k        dres             exact                                 65  no mismatch
  bn_bwd_apply_fin8_k        dres             value                                 12  no mismatch
  bn_bwd_apply_fin8_k        dx               tolerance                            155  0.996
  bn_bwd_apply_k             dres             2^-8                                  11  0.996
  bn_bwd_apply_k             dres             exact                                 44  no mismatch
  bn_bwd_apply_k             dx               tolerance                             79  0.996
  bn_bwd_coop8_k             dbeta            float32(old + ws)                     41  no mismatch
  bn_bwd_coop8_k             dgamma           float32(old + ws)                     46  no mismatch
  bn_bwd_coop8_k             dres             2^-8                                  12  0.996
  bn_bwd_coop8_k             dres             exact                                 27  no mismatch
  bn_bwd_coop8_k             dx               tolerance                             63  0.996
  bn_bwd_coop8_k             ws[0:C]          8 x yard                              63  0.819
  bn_bwd_coop8_k             ws[0:C], twin    exact                                 30  no mismatch
  bn_bwd_coop8_k             ws[C:2C]         8 x yard                              63  0.760
  bn_bwd_coop8_k<1>          launches         count                                 60  no mismatch
  bn_bwd_coop8_k<2>          launches         count                                  1  no mismatch
  bn_bwd_coop8_k<4>          launches         count                                  1  no mismatch
  bn_bwd_coop8_k<8>          launches         count                                  1  no mismatch
  bn_bwd_reduce_k            ws[0:C]          8 x yard                              79  0.587
  bn_bwd_reduce_k            ws[0:C], twin    exact                                 38  no mismatch
  bn_bwd_reduce_k            ws[C:2C]         8 x yard                              79  0.967
  bn_colred8_k<0>            mean*M           8 x yard                             265  0.344
  bn_colred8_k<0>            mean*M, twin     exact                                132  no mismatch
  bn_colred8_k<0> finish     rstd             propagated                            68  0.115
  bn_colred8_k<0> finish     running_mean     2 ulp                                 44  0.438
  bn_colred8_k<0> finish     running_var      2 ulp + m Bvar                        44  0.341
  bn_colred8_k<1>            ws[0:C]          8 x yard                             252  0.515
  bn_colred8_k<1>            ws[0:C], twin    exact                                127  no mismatch
  bn_colred8_k<1>            ws[C:2C]         8 x yard                             252  0.744
  bn_colred8_k<1> finish     dbeta            float32(old + ws)                     62  no mismatch
  bn_colred8_k<1> finish     dgamma           float32(old + ws)                     68  no mismatch
  bn_finalize_k              rstd             propagated                            75  0.115
  bn_finalize_k              running_mean     2 ulp                                 53  0.470
  bn_finalize_k              running_var      2 ulp + m Bvar                        53  0.265
  bn_fold_k<0>               rstd             propagated                            16  0.070
  bn_fold_k<0>               running_mean     2 ulp                                 10  0.399
  bn_fold_k<0>               running_var      2 ulp + m Bvar                        10  0.286
  bn_fold_k<1>               dbeta            float32(old + ws)                     30  no mismatch
  bn_fold_k<1>               dgamma           float32(old + ws)                     34  no mismatch
  bn_grad_acc_k              dbeta            float32(old + ws)                     55  no mismatch
  bn_grad_acc_k              dgamma           float32(old + ws)                     65  no mismatch
  bn_stats_k                 mean*M           8 x yard                              75  0.826
  bn_stats_k                 mean*M, twin     exact                                 36  no mismatch
  cross-route                db               bit-identical                          2  no mismatch
  cross-route                dg               bit-identical                          2  no mismatch
  cross-route                dres             bit-identical                         51  no mismatch
  cross-route                dx               bit-identical                         51  no mismatch
  cross-route                dx               bit-identical where ws[C:2C] is       36  no mismatch
  cross-route                mean             bit-identical                         93  no mismatch
  cross-route                rstd             bit-identical                         93  no mismatch
  cross-route                ws               bit-identical                         51  no mismatch
  cross-route                y                bit-identical                         93  no mismatch
  deterministic mode         all outputs      two launches bit-identical             2  no mismatch
  host replicas              mean*M           8 x yard                              35  0.436
  host replicas              mean*M, twin     exact                                 16  no mismatch
  host replicas              ws[0:C]          8 x yard                              35  0.158
  host replicas              ws[0:C], twin    exact                                 16  no mismatch
  host replicas              ws[C:2C]         8 x yard                              35  0.631

The y, dx and dres ratios near 1 are the bf16 rounding itself (2^-8 |ref| is reached just above a power of two);
every sum stays below ONE yardstick (worst: bn_bwd_reduce_k's sum dz xhat).  "bit-identical where ws[C:2C] is" counts
the comparisons between routes with different reduction grids (see same_backward).

No defect was found in norm.hip by this file.  Scratch mutations that each turned checks red: k2 read from ws[0:C], r1
one row short in bn_colred8_k, no re-zero in bn_fold_k, the biased variance in bn_apply_fin8_k's running_var, and
bn_apply8_k's shift rounded twice (caught only by the cancellation test: bf16 y hides it elsewhere).
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
from hops_examples_amd.ops.functional import bn_bwd_reference, bn_reference, bn_stats_reference  # noqa: E402

dev = torch.device("cuda", 0)
f32, bf, f64 = torch.float32, torch.bfloat16, torch.float64
MARGIN = 8.0
ULP32 = 2.0 ** -23
PAD = 64
SENT = {f32: -7777.25, bf: -3.0}
NREP = K.BN_NREP
EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=f32))
MOM32 = float(torch.tensor(MOM, dtype=f32))
OMM32 = float(torch.tensor(1.0, dtype=f32) - torch.tensor(MOM, dtype=f32))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {}  # (kernel, output, rule) -> [checks, worst ratio]
KNOBS = ("HOPSX_BN_DEFER_MAXC", "HOPSX_BN_FOLD_MINC", "HOPSX_BN_MAXG", "HOPSX_BN_APPLY_MAXG", "HOPSX_BN_COOP",
         "HOPSX_DETERMINISTIC", "HOPSX_DISABLE", "HOPSX_BN_RPT")

@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A sticky HIP error (a fault in an earlier test) ends the session: nothing more is started on that GPU."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU error before this test, stopping: {e}", returncode=3)
    yield


def EXT():
    """The raw extension module: the bindings take every pointer as an integer, so 0 is a null pointer."""
    from hops_examples_amd.ops import _C
    return _C.ext()


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.encode()))


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


class Frame:
    """A device buffer of sentinels with the tensor as its view [off, off + n); off = PAD + 1 starts a bf16 tensor
    2 bytes past a 16-byte line."""

    def __init__(self, shape, dtype, init, off=PAD):
        self.n, self.off, self.sent = math.prod(shape), off, SENT[dtype]
        self.buf = torch.full((off + self.n + PAD,), self.sent, dtype=dtype, device=dev)
        self.v = self.buf[off:off + self.n].view(shape)
        self.init = None
        if isinstance(init, float):
            self.v.fill_(init)
        else:
            self.init = init.to(dtype).contiguous()
            self.v.copy_(self.init)

    def host(self):
        return self.v.cpu()

    def intact(self):
        a, b = self.buf[:self.off].cpu(), self.buf[self.off + self.n:].cpu()
        return bool((a == self.sent).all()) and bool((b == self.sent).all())

    def unchanged(self):
        return self.intact() and bits_equal(self.host(), self.init)


def _v(fr):
    return None if fr is None else fr.v


def _ulps(n):
    return ULP32 * (1.0 + 0.29 * math.sqrt(max(n, 1) - 1))


def _rec(kern, out, rule, ratio=None):
    e = STATS.setdefault((kern, out, rule), [0, 0.0])
    e[0] += 1
    if ratio is not None:
        e[1] = max(e[1], ratio)


def _line(tag, out, err, bound, ratio):
    print(f"BNERR {tag} {out} {err:.3e} {bound:.3e} {ratio:.3f}")


def acc_at_rest(acc, C, tag):
    w = acc.cpu().view(torch.int32)[:NREP * 2 * C + 10 * 32]
    assert not bool(w.any()), (tag, "accumulator not zero at rest", int(w.count_nonzero()))


# ------------------------------------------------------------------------------------------------- comparisons
def check_sum(tag, kern, out, got, ref64, ref32, absmag, n):
    """The float-atomic sum rule; returns the bound (for the propagated checks)."""
    e = (got.double() - ref64).abs()
    yard = torch.maximum((ref32.double() - ref64).abs(), _ulps(n) * absmag)
    ratio = (e / yard.clamp_min(1e-300))[yard > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _line(tag, out, float(e.max()), MARGIN * float(yard.max()), worst / MARGIN)
    _rec(kern, out, "8 x yard", worst)
    assert bool((e <= MARGIN * yard).all()), (tag, out, worst)
    return MARGIN * yard


def check_tol(tag, kern, out, got, ref, bound, rule="tolerance"):
    err = (got.double() - ref).abs()
    ok = err <= bound  # (a NaN left in an output compares false)
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf"))[bound > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _line(tag, out, float(err.nan_to_num(nan=float("inf")).max()), float(bound.max()), worst)
    _rec(kern, out, rule, worst)
    assert bool(ok.all()), (tag, out, int((~ok).sum()), worst)


def check_exact(tag, kern, out, got, want, rule="exact"):
    bad = got.numel() if got.shape != want.shape or got.dtype != want.dtype else \
        int((got.view(torch.int16 if got.element_size() == 2 else torch.int32)
             != want.view(torch.int16 if want.element_size() == 2 else torch.int32)).sum())
    print(f"BNERR {tag} {out} exact mismatches {bad} of {got.numel()}")
    _rec(kern, out, rule)
    assert bad == 0, (tag, out, bad)


# ------------------------------------------------------------------------------------------------------- cases
OPTS = [  # paired sparsely; test_option_coverage checks that every value of every option is there
    dict(act="relu", res=1, g=1, b=1, run=1, dg=1, db=1, dres=1),
    dict(act=None, res=0, g=1, b=1, run=1, dg=1, db=1, dres=0),
    dict(act="sigmoid", res=1, g=0, b=1, run=0, dg=0, db=1, dres=1),
    dict(act="tanh", res=0, g=1, b=0, run=1, dg=1, db=0, dres=0),
    dict(act="relu", res=0, g=1, b=1, run=1, dg=1, db=1, dres=0),
    dict(act=None, res=1, g=0, b=0, run=0, dg=0, db=0, dres=1),
    dict(act="tanh", res=1, g=1, b=1, run=0, dg=1, db=1, dres=1),
    dict(act="sigmoid", res=0, g=0, b=1, run=1, dg=1, db=0, dres=1),
]
KERN = {  # route -> kernels that produce (sums, finish, apply) in forward and backward
    ("f", "scalar"): ("bn_stats_k", "bn_finalize_k", "bn_apply_k"),
    ("f", "defer"): ("bn_colred8_k<0>", "bn_apply_fin8_k", "bn_apply_fin8_k"),
    ("f", "selffin"): ("bn_colred8_k<0>", "bn_colred8_k<0> finish", "bn_apply8_k"),
    ("f", "fold"): ("host replicas", "bn_fold_k<0>", "bn_apply8_k"),
    ("f", "pre"): ("host replicas", "bn_apply_fin8_k", "bn_apply_fin8_k"),
    ("b", "scalar"): ("bn_bwd_reduce_k", "bn_grad_acc_k", "bn_bwd_apply_k"),
    ("b", "defer"): ("bn_colred8_k<1>", "bn_bwd_apply_fin8_k", "bn_bwd_apply_fin8_k"),
    ("b", "selffin"): ("bn_colred8_k<1>", "bn_colred8_k<1> finish", "bn_bwd_apply8_k"),
    ("b", "fold"): ("bn_colred8_k<1>", "bn_fold_k<1>", "bn_bwd_apply8_k"),
    ("b", "coop"): ("bn_bwd_coop8_k", "bn_bwd_coop8_k", "bn_bwd_coop8_k"),
    ("p", "defer"): ("host replicas", "bn_bwd_apply_fin8_k", "bn_bwd_apply_fin8_k"),
    ("p", "fold"): ("host replicas", "bn_fold_k<1>", "bn_bwd_apply8_k"),
}


def test_option_coverage():
    for key, vals in dict(act=(None, "relu", "sigmoid", "tanh"), res=(0, 1), g=(0, 1), b=(0, 1), run=(0, 1), dg=(0, 1),
                          db=(0, 1), dres=(0, 1)).items():
        assert {o[key] for o in OPTS} == set(vals), key
    for a, b in (("g", "b"), ("dg", "db")):  # null independently
        assert {(o[a], o[b]) for o in OPTS} >= {(0, 1), (1, 0)}, (a, b)


class Case:
    """The operands of one case for both kinds (random and the integer twin), built once."""

    def __init__(self, name, M, C, opt, mis=None):
        self.name, self.M, self.C, self.o, self.mis = name, M, C, opt, mis
        g = _gen(name)
        offs, spread = torch.randn(C, generator=g) * 1.5, torch.rand(C, generator=g) + 0.5
        ri = lambda: torch.randint(-8, 9, (M, C), generator=g).to(bf)  # noqa: E731
        self.x = {"rand": (torch.randn(M, C, generator=g) * spread + offs).to(bf), "twin": ri()}
        self.res = {"rand": torch.randn(M, C, generator=g).to(bf), "twin": ri()}
        self.dy = {"rand": torch.randn(M, C, generator=g).to(bf), "twin": ri()}
        self.gamma, self.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        self.rm, self.rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        self.dg = {"rand": torch.randn(C, generator=g) * 3, "twin": torch.randint(-100, 101, (C,), generator=g).float()}
        self.db = {"rand": torch.randn(C, generator=g) * 3, "twin": torch.randint(-100, 101, (C,), generator=g).float()}
        self._stats = {}

    def act(self, kind):
        a = self.o["act"]
        return a if kind == "rand" or a in (None, "relu") else "relu"

    def g_(self):
        return self.gamma if self.o["g"] else None

    def b_(self):
        return self.beta if self.o["b"] else None

    def r_(self, kind):
        return self.res[kind] if self.o["res"] else None

    def off(self, name):
        return PAD + (1 if self.mis == name else 0)

    def stats(self, kind):
        """(s64, q64, s32, q32, sum|x|, q64): the sums' references and magnitudes."""
        if kind not in self._stats:
            x = self.x[kind]
            s64, q64 = bn_stats_reference(x)[:2]
            s32, q32 = bn_stats_reference(x, f32)[:2]
            self._stats[kind] = (s64, q64, s32, q32, x.double().abs().sum(0), q64)
        return self._stats[kind]


def n_partials(plan, C):
    if plan["route"] == "scalar":
        return plan["g"] + 4
    return max(plan["g"], 1) + 256 // (C // 8) + NREP


# ------------------------------------------------------------------------------------------------------ forward
def check_forward(tag, route, cs, kind, out, stats, n, launcher="f"):
    """mean / rstd / running statistics / y of one forward against fp64 from the stated sums and the kernel's own
    published mean / rstd.  stats = (s64, q64, s32, q32, |s| magnitudes, |q| magnitudes)."""
    ks, kf, ka = KERN[(launcher, route)]
    M, C, o = cs.M, cs.C, cs.o
    s64, q64, s32, q32, abs_s, abs_q = stats
    mean, rstd = out["mean"].double(), out["rstd"].double()
    Bs = check_sum(tag, ks, "mean*M", mean * M, s64, s32, abs_s, n)
    if kind == "twin":
        bad = int((torch.round(mean * M) != s64).sum())
        print(f"BNERR {tag} mean*M exact mismatches {bad} of {C}")
        _rec(ks, "mean*M, twin", "exact")
        assert bad == 0, (tag, "integer sum not exact", bad)
    Bq = MARGIN * torch.maximum((q32.double() - q64).abs(), _ulps(n) * abs_q)
    mean64 = s64 / M
    var64 = (q64 / M - mean64 * mean64).clamp_min(0)
    Bvar = Bq / M + 2 * mean64.abs() * Bs / M + 4 * ULP32 * (q64 / M + mean64 * mean64) + 8 * ULP32 * (var64 + EPS32)
    check_tol(tag, kf, "rstd", 1.0 / (rstd * rstd) - EPS32, var64, Bvar, "propagated")
    if o["run"]:
        f = M / (M - 1) if M > 1 else 1.0
        a, b = OMM32 * cs.rm.double(), MOM32 * mean
        check_tol(tag, kf, "running_mean", out["rm"], a + b, 2 * ULP32 * (a.abs() + b.abs()), "2 ulp")
        a, b = OMM32 * cs.rv.double(), MOM32 * var64 * f
        check_tol(tag, kf, "running_var", out["rv"], a + b,
                  2 * ULP32 * (a.abs() + b.abs()) + MOM32 * f * Bvar + ULP32 * b.abs(), "2 ulp + m Bvar")
    x, res, act = cs.x[kind], cs.r_(kind), cs.act(kind)
    ref = bn_reference(x, cs.g_(), cs.b_(), out["mean"], out["rstd"], EPS, res, act)
    sc = rstd * (cs.gamma.double() if o["g"] else 1.0)
    sh = (cs.beta.double() if o["b"] else 0.0) - mean * sc
    mag = (x.double() * sc).abs() + sh.abs() + (res.double().abs() if res is not None else 0.0)
    check_tol(tag, ka, "y", out["y"], ref, 2.0 ** -8 * ref.abs() + 4 * ULP32 * mag)
    if act == "relu":
        z = out["y"].view(torch.int16)[out["y"] == 0]
        assert int(z.count_nonzero()) == 0, (tag, "a ReLU zero is not +0")


def run_forward(cs, kind, want, n=None, check=True, null_acc=False):
    """null_acc: the launcher and its reporter get acc == nullptr through the raw extension (kernels.bn_fwd_train
    always passes the per-width accumulator)."""
    M, C, o = cs.M, cs.C, cs.o
    X = Frame((M, C), bf, cs.x[kind], cs.off("x"))
    RES = Frame((M, C), bf, cs.res[kind], cs.off("res")) if o["res"] else None
    Y = Frame((M, C), bf, float("nan"), cs.off("y"))
    MEAN, RSTD = Frame((C,), f32, float("nan")), Frame((C,), f32, float("nan"))
    RM, RV = (Frame((C,), f32, cs.rm), Frame((C,), f32, cs.rv)) if o["run"] else (None, None)
    G = Frame((C,), f32, cs.gamma) if o["g"] else None
    B = Frame((C,), f32, cs.beta) if o["b"] else None
    p = K.ptr
    if null_acc:
        plan = K._bn_plan(EXT().bn_fwd_train_path(p(X.v), p(Y.v), p(_v(RES)), 0, M, C))
    else:
        plan = K.bn_fwd_train_path(X.v, Y.v, _v(RES))
    tag = f"{cs.name} {kind} fwd:{plan['route']}{' acc=null' if null_acc else ''}"
    assert plan["route"] == want, (tag, "route", want)
    if null_acc:
        K.check(EXT().bn_fwd_train(p(X.v), p(Y.v), p(_v(G)), p(_v(B)), p(MEAN.v), p(RSTD.v), p(_v(RM)), p(_v(RV)), MOM,
                                   EPS, M, C, p(_v(RES)), K.act_id(cs.act(kind)), 0, K.stream()), "bn_fwd_train")
    else:
        K.bn_fwd_train(X.v, _v(G), _v(B), MEAN.v, RSTD.v, _v(RM), _v(RV), MOM, EPS, residual=_v(RES),
                       act=cs.act(kind), out=Y.v)
    torch.cuda.synchronize()
    if not null_acc:  # (the null-accumulator test fills bn_acc with a pattern and compares it itself)
        acc_at_rest(K.bn_acc(dev, C), C, tag)
    for fr in (X, RES, G, B):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    for fr in (Y, MEAN, RSTD, RM, RV):
        assert fr is None or fr.intact(), (tag, "sentinels")
    out = dict(mean=MEAN.host(), rstd=RSTD.host(), y=Y.host(), rm=RM.host() if RM else None,
               rv=RV.host() if RV else None, plan=plan)
    if check:
        check_forward(tag, want, cs, kind, out, cs.stats(kind), n or n_partials(plan, C))
    return out


# ----------------------------------------------------------------------------------------------------- backward
def check_backward(tag, route, cs, kind, fwd, out, n, y_for_ref, act, launcher="b", stated=None):
    """ws / dres / dx / dgamma / dbeta.  The sums' reference is fp64 over the tensors (or `stated`, the replica rows
    the test wrote itself: (s1_64, s2_64, s1_32, s2_32, |.|, |.|))."""
    ks, kf, ka = KERN[(launcher, route)]
    M, C, o = cs.M, cs.C, cs.o
    dy, x = cs.dy[kind], cs.x[kind]
    g, b, mean, rstd = cs.g_(), cs.b_(), fwd["mean"], fwd["rstd"]
    dz, s1, s2, _ = bn_bwd_reference(dy, x, y_for_ref, g, b, mean, rstd, act)
    xhat = (x.double() - mean.double()) * rstd.double()
    ws = out["ws"].double()
    if stated is None:
        _, t1, t2, _ = bn_bwd_reference(dy, x, y_for_ref, g, b, mean, rstd, act, dtype=f32)
        stated = (s1, s2, t1, t2, dz.abs().sum(0), (dz * xhat).abs().sum(0))
    check_sum(tag, ks, "ws[0:C]", ws[:C], stated[0], stated[2], stated[4], n)
    check_sum(tag, ks, "ws[C:2C]", ws[C:], stated[1], stated[3], stated[5], n)
    if kind == "twin":
        bad = int((ws[:C] != stated[0]).sum())
        print(f"BNERR {tag} ws[0:C] exact mismatches {bad} of {C}")
        _rec(ks, "ws[0:C], twin", "exact")
        assert bad == 0, (tag, "integer sum not exact", bad)
    if out["dres"] is not None:
        if act in (None, "relu"):
            if out.get("dres_by_value"):
                _rec(ka, "dres", "value")
                assert torch.equal(out["dres"].float(), dz.to(bf).float()), (tag, "dres")
            else:
                check_exact(tag, ka, "dres", out["dres"], dz.to(bf))
        else:
            check_tol(tag, ka, "dres", out["dres"], dz, 2.0 ** -8 * dz.abs(), "2^-8")
    k1 = rstd.double() * (cs.gamma.double() if o["g"] else 1.0)
    t0, t1 = ws[:C] / M, xhat * ws[C:] / M
    ref = k1 * (dz - t0 - t1)
    mag = k1.abs() * (dz.abs() + t0.abs() + t1.abs())
    check_tol(tag, ka, "dx", out["dx"], ref, 2.0 ** -8 * ref.abs() + 6 * ULP32 * mag)
    if o["db"]:
        check_exact(tag, kf, "dbeta", out["db"], cs.db[kind] + out["ws"][:C], "float32(old + ws)")
        if kind == "twin":
            assert bool((out["db"].double() - cs.db[kind].double() == stated[0]).all()), (tag, "dbeta - old not exact")
    if o["dg"]:
        check_exact(tag, kf, "dgamma", out["dg"], cs.dg[kind] + out["ws"][C:], "float32(old + ws)")


def run_backward(cs, kind, fwd, want, zbeta=False, n=None, null_acc=False):
    """fwd: the forward's published outputs (mean, rstd, y) the backward consumes.  null_acc: as run_forward."""
    M, C, o, act = cs.M, cs.C, cs.o, cs.act(kind)
    DY = Frame((M, C), bf, cs.dy[kind], cs.off("dy"))
    X = Frame((M, C), bf, cs.x[kind], cs.off("x"))
    Y = Frame((M, C), bf, fwd["y"], cs.off("y"))
    DX = Frame((M, C), bf, float("nan"), cs.off("dx"))
    DRES = Frame((M, C), bf, float("nan"), cs.off("dres")) if o["dres"] else None
    G = Frame((C,), f32, cs.gamma) if o["g"] else None
    ZB = Frame((C,), f32, cs.beta) if zbeta else None
    MEAN, RSTD = Frame((C,), f32, fwd["mean"]), Frame((C,), f32, fwd["rstd"])
    DG = Frame((C,), f32, cs.dg[kind]) if o["dg"] else None
    DB = Frame((C,), f32, cs.db[kind]) if o["db"] else None
    WS = Frame((2 * C,), f32, float("nan"))
    p = K.ptr
    if null_acc:
        plan = K._bn_plan(EXT().bn_bwd_path(p(DY.v), p(X.v), p(Y.v), p(DX.v), p(_v(DRES)), 0, p(_v(ZB)), M, C,
                                            K.act_id(act)))
    else:
        plan = K.bn_bwd_path(DY.v, X.v, Y.v, DX.v, act=act, dresidual=_v(DRES), zbeta=_v(ZB))
    tag = f"{cs.name} {kind} bwd:{plan['route']}{plan['R'] or ''}{' zbeta' if zbeta else ''}"
    tag += " acc=null" if null_acc else ""
    assert plan["route"] == want, (tag, "route", want)
    assert plan["reads_y"] == (act is not None and not (zbeta and act == "relu" and want == "defer"
                                                        and "bn_zmask" not in os.environ.get("HOPSX_DISABLE", ""))), tag
    if not plan["reads_y"]:
        Y = Frame((M, C), bf, float("nan"), cs.off("y"))  # must not be read
        Y.init = torch.full((M, C), float("nan"), dtype=bf)
    if null_acc:
        K.check(EXT().bn_bwd(p(DY.v), p(X.v), p(Y.v), p(_v(G)), p(MEAN.v), p(RSTD.v), p(DX.v), p(_v(DG)), p(_v(DB)),
                             p(WS.v), M, C, K.act_id(act), p(_v(DRES)), 0, p(_v(ZB)), K.stream()), "bn_bwd")
    else:
        K.bn_bwd(DY.v, X.v, Y.v, _v(G), MEAN.v, RSTD.v, _v(DG), _v(DB), WS.v, act=act, dresidual=_v(DRES), out=DX.v,
                 zbeta=_v(ZB))
    torch.cuda.synchronize()
    if not null_acc:
        acc_at_rest(K.bn_acc(dev, C), C, tag)
    for fr in (DY, X, Y, G, ZB, MEAN, RSTD):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    for fr in (DX, DRES, DG, DB, WS):
        assert fr is None or fr.intact(), (tag, "sentinels")
    out = dict(ws=WS.host(), dx=DX.host(), dres=DRES.host() if DRES else None, dg=DG.host() if DG else None,
               db=DB.host() if DB else None, plan=plan, dres_by_value=not plan["reads_y"] and act == "relu")
    check_backward(tag, want, cs, kind, fwd, out, n or n_partials(plan, C), fwd["y"], act)
    if want == "coop":
        assert K.bn_coop_timeouts(dev, C) == 0, (tag, "grid barrier timed out")
        _rec(f"bn_bwd_coop8_k<{plan['R']}>", "launches", "count")
    return out


def same_bits(tag, a, b, keys):
    for k in keys:
        if a.get(k) is None or b.get(k) is None:
            continue
        _rec("cross-route", k, "bit-identical")
        assert bits_equal(a[k], b[k]), (tag, k, "differs across routes")


FWD_KEYS = ("mean", "rstd", "y")
BWD_KEYS = ("dx", "dres")


def same_backward(tag, a, b):
    """dres and ws[0:C] (integer sums) bit for bit.  dx bit for bit where both routes reduce with bn_colred8_k on the
    same grid of at most BN_NREP workgroups (defer, selffin, fold: one workgroup per replica row, folded in row order,
    so ws[C:2C] is the same float); otherwise in every channel whose published ws[C:2C] agrees bit for bit.  (sum dz
    xhat is no integer sum: another split of the rows over workgroups, the cooperative grid or HOPSX_BN_MAXG, may
    round it differently, and dx = k1 (dz - ws0 / M - xhat ws1 / M) follows the ws it was computed from, to which
    check_backward ties it on every route.)  Returns (agreeing, all) channels."""
    same_bits(tag, a, b, ("dres",))
    C = a["ws"].numel() // 2
    assert torch.equal(a["ws"][:C], b["ws"][:C]), (tag, "ws[0:C] differs across routes")
    pa, pb = a["plan"], b["plan"]
    if "coop" not in (pa["route"], pb["route"]) and (pa["g"], pa["rpb"]) == (pb["g"], pb["rpb"]) and pa["g"] <= NREP:
        same_bits(tag, a, b, ("ws", "dx"))
        return C, C
    agree = a["ws"][C:].view(torch.int32) == b["ws"][C:].view(torch.int32)
    print(f"BNERR {tag} dx across routes: ws[C:2C] bit-identical in {int(agree.sum())} of {C} channels")
    _rec("cross-route", "dx", "bit-identical where ws[C:2C] is")
    assert bits_equal(a["dx"][:, agree].contiguous(), b["dx"][:, agree].contiguous()), (tag, "dx differs across routes")
    return int(agree.sum()), C


def run_pair(cs, kind, froute, broute, zbeta=False):
    f = run_forward(cs, kind, froute)
    return f, run_backward(cs, kind, f, broute, zbeta=zbeta)


# ------------------------------------------------------------------------------------------------ vector routes
VEC_C = (8, 16, 64, 512, 1024, 2048)


def vec_Ms(C):
    rpi = 256 // (C // 8)
    return (1, 2, rpi * 4 - 1, rpi * 4 + 1, rpi * 4 * 2 + rpi + 1)  # the last: 3 workgroups, a ragged last slab


def vec_cases(C):
    ci = VEC_C.index(C)
    return [Case(f"v C{C} M{M}", M, C, OPTS[(ci * 5 + mi) % 8]) for mi, M in enumerate(vec_Ms(C))]


_DEFAULT = {}


def default_pair(cs, kind):
    """The case on the default route (deferred fold), once per process."""
    key = (cs.name, kind)
    if key not in _DEFAULT:
        _DEFAULT[key] = run_pair(cs, kind, "defer", "defer")
    return _DEFAULT[key]


def _clean(monkeypatch):
    for k in ("HOPSX_DISABLE", "HOPSX_BN_RPT"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("C", VEC_C)
def test_vector_routes(monkeypatch, C):
    """bn_colred8_k<0/1> + bn_apply_fin8_k / bn_bwd_apply_fin8_k (default), then with HOPSX_DISABLE=bn_defer the
    self-finishing bn_colred8_k + bn_apply8_k / bn_bwd_apply8_k: M = 1, 2, one row under / over a full pass of
    BN_UNR rows per lane, and three workgroups with a ragged last slab."""
    _clean(monkeypatch)
    cases = vec_cases(C)
    rpb = K.bn_fwd_train_path(*(torch.empty(cases[-1].M, C, device=dev, dtype=bf),) * 2)
    assert rpb["g"] == 3 and cases[-1].M % rpb["rpb"] != 0, rpb
    for cs in cases:
        for kind in ("rand", "twin"):
            monkeypatch.delenv("HOPSX_DISABLE", raising=False)
            f0, b0 = default_pair(cs, kind)
            monkeypatch.setenv("HOPSX_DISABLE", "bn_defer")
            f1, b1 = run_pair(cs, kind, "selffin", "selffin")
            if kind == "twin":
                same_bits(cs.name, f0, f1, FWD_KEYS)
                same_backward(cs.name, b0, b1)


@pytest.mark.parametrize("C", VEC_C)
def test_shift_is_one_fma_on_every_route(monkeypatch, C):
    """The forward's shift is ONE fma on every route (norm.hip bn_shift; the backward's zmask recomputes it).  An
    integer twin whose beta makes act-free y cancel at the value x[0, c] of every channel, beta = -(x[0, c] - mean)
    rstd gamma: y there is the rounding residue of x sc + sh, a few fp32 ulp of sh, so a shift rounded twice on one
    route (product, then difference) changes those bf16 values, while mean / rstd stay bit-identical (exact sums).
    Compared across routes only: the rounding of sc = rstd gamma moves y by half an ulp of |mean sc|, a term the y
    bound has no need for elsewhere and which is all there is at a cancellation."""
    _clean(monkeypatch)
    cs = Case(f"cancel C{C}", vec_Ms(C)[-1], C, OPTS[1])
    _, _, mean, var, _ = bn_stats_reference(cs.x["twin"])
    cs.beta = (-(cs.x["twin"][0].double() - mean) * cs.gamma.double() / torch.sqrt(var + EPS32)).float()
    f0 = run_forward(cs, "twin", "defer", check=False)
    monkeypatch.setenv("HOPSX_DISABLE", "bn_defer")
    f1 = run_forward(cs, "twin", "selffin", check=False)
    same_bits(cs.name, f0, f1, FWD_KEYS)
    hit = cs.x["twin"] == cs.x["twin"][0]
    assert float(f0["y"][hit].float().abs().max()) < 2.0 ** -12 * float(cs.beta.abs().max()), "no cancellation"


@pytest.mark.parametrize("C", (8, 64, 2048))
def test_zmask(monkeypatch, C):
    """ReLU without residual, zbeta = beta: the deferred pair takes act' from z and must not read y (a NaN frame);
    under HOPSX_DISABLE=bn_zmask, and on the self-finishing route (whose plain apply has no zmask), y is read."""
    _clean(monkeypatch)
    for mi, M in enumerate(vec_Ms(C)[2:]):
        cs = Case(f"zmask C{C} M{M}", M, C, OPTS[4] if mi % 2 else dict(OPTS[4], dres=1, g=0))
        for kind in ("rand", "twin"):
            monkeypatch.delenv("HOPSX_DISABLE", raising=False)
            f, b = default_pair(cs, kind)
            bz = run_backward(cs, kind, f, "defer", zbeta=True)
            assert not bz["plan"]["reads_y"]
            monkeypatch.setenv("HOPSX_DISABLE", "bn_zmask")
            bo = run_backward(cs, kind, f, "defer", zbeta=True)
            monkeypatch.setenv("HOPSX_DISABLE", "bn_defer")
            bs = run_backward(cs, kind, f, "selffin", zbeta=True)
            assert bo["plan"]["reads_y"] and bs["plan"]["reads_y"]
            if kind == "twin":
                for other in (bz, bo, bs):
                    # by value: a column of masked gradients gives -0 through act' * dy and +0 through the z test
                    assert torch.equal(b["dx"].float(), other["dx"].float()), (cs.name, "dx")
                    assert torch.equal(b["ws"][:C], other["ws"][:C]), (cs.name, "ws[0:C]")
                    if b["dres"] is not None:
                        assert torch.equal(b["dres"].float(), other["dres"].float()), (cs.name, "dres")


@pytest.mark.parametrize("rpt", (1, 16))
def test_rows_per_thread_knob(monkeypatch, rpt):
    """HOPSX_BN_RPT (read on every call) = 1: 10 workgroups of 32 rows at C 64, M 300; 16: a single one."""
    _clean(monkeypatch)
    cs = Case("rpt C64 M300", 300, 64, OPTS[0])
    for kind in ("rand", "twin"):
        monkeypatch.delenv("HOPSX_BN_RPT", raising=False)
        f0, b0 = default_pair(cs, kind)
        monkeypatch.setenv("HOPSX_BN_RPT", str(rpt))
        f1, b1 = run_pair(cs, kind, "defer", "defer")
        assert f1["plan"]["g"] == {1: 10, 16: 1}[rpt] and b1["plan"]["g"] == f1["plan"]["g"]
        if kind == "twin":
            same_bits(cs.name, f0, f1, FWD_KEYS)
            same_backward(cs.name, b0, b1)


# ------------------------------------------------------------------------------------------------- scalar route
SC_C = (1, 3, 24, 96, 130, 2056)
SC_M = (1, 2, 5, 301, 777)  # 301: two slabs of 151 + 150 rows; 777: four of 195, 195, 195, 192


@pytest.mark.parametrize("C", SC_C)
def test_scalar_route(monkeypatch, C):
    """bn_stats_k / bn_finalize_k / bn_apply_k and bn_bwd_reduce_k / bn_bwd_apply_k / bn_grad_acc_k: C % 8 != 0, C / 8
    not dividing 256 (24), three 64-column strips with a ragged last one (130), C / 8 > 256 (2056)."""
    _clean(monkeypatch)
    ci = SC_C.index(C)
    for mi, M in enumerate(SC_M):
        cs = Case(f"s C{C} M{M}", M, C, OPTS[(ci * 5 + mi + 3) % 8])
        for kind in ("rand", "twin"):
            f, b = run_pair(cs, kind, "scalar", "scalar")
            if M == 301:
                assert f["plan"]["g"] == 2 and f["plan"]["rpb"] == 151 and f["plan"]["gx"] == (C + 63) // 64


@pytest.mark.parametrize("mis", ("x", "y", "res", "dy", "dx", "dres", "bn_vec"))
def test_scalar_by_gate(monkeypatch, mis):
    """C 64 is a vector width; one pointer 2 bytes off a 16-byte line (each in turn), or HOPSX_DISABLE=bn_vec, sends
    the launcher that sees it to the scalar kernels."""
    _clean(monkeypatch)
    if mis == "bn_vec":
        monkeypatch.setenv("HOPSX_DISABLE", "bn_vec")
    cs = Case(f"gate {mis}", 301, 64, OPTS[0], mis=None if mis == "bn_vec" else mis)
    fr = "scalar" if mis in ("x", "y", "res", "bn_vec") else "defer"
    br = "scalar" if mis != "res" else "defer"
    for kind in ("rand", "twin"):
        run_pair(cs, kind, fr, br)


def test_null_accumulator(monkeypatch):
    """C 64, aligned, acc == nullptr: bn_fwd_train and bn_bwd take the scalar kernels (same checks as any scalar
    case, zbeta given too), bn_fwd_apply_fin and bn_bwd_pre refuse with -2 and write nothing; the per-width
    accumulator, filled with a pattern meanwhile, is bit-unchanged."""
    _clean(monkeypatch)
    C = 64
    acc = K.bn_acc(dev, C)
    pattern = torch.randn(acc.numel(), generator=_gen("null acc"))
    acc.copy_(pattern)
    try:
        before = acc.cpu()
        for cs in (Case("null acc M301", 301, C, OPTS[0]), Case("null acc M37", 37, C, OPTS[4])):
            for kind in ("rand", "twin"):
                f = run_forward(cs, kind, "scalar", null_acc=True)
                run_backward(cs, kind, f, "scalar", zbeta=cs.o is OPTS[4], null_acc=True)
        cs = Case("null acc refuse", 9, C, OPTS[0])
        X, O = Frame((9, C), bf, cs.x["rand"]), Frame((9, C), bf, float("nan"))
        V = [Frame((C,), f32, cs.gamma) for _ in range(6)]
        WS = Frame((2 * C,), f32, float("nan"))
        frames = (X, O, WS, *V)
        snap = [fr.buf.cpu() for fr in frames]
        p, e = K.ptr, EXT()
        assert K.bn_prestats_ok(C)
        assert e.bn_fwd_apply_fin_path(p(X.v), p(O.v), 0, 0, 9, C)[0] == -2
        assert e.bn_fwd_apply_fin(p(X.v), p(O.v), p(V[0].v), p(V[1].v), p(V[2].v), p(V[3].v), p(V[4].v), p(V[5].v), MOM,
                                  EPS, 9, C, 0, 1, 0, K.stream()) == -2
        assert e.bn_bwd_pre_path(p(X.v), p(X.v), p(O.v), 0, 9, C)[0] == -2
        assert e.bn_bwd_pre(p(X.v), p(X.v), p(V[0].v), p(V[2].v), p(V[3].v), p(O.v), p(V[4].v), p(V[5].v), p(WS.v), 9,
                            C, 0, K.stream()) == -2
        torch.cuda.synchronize()
        for fr, b in zip(frames, snap):
            assert bits_equal(fr.buf.cpu(), b), "a refused launcher wrote something"
        assert bits_equal(acc.cpu(), before), "bn_acc touched by a launcher that was given no accumulator"
    finally:
        acc.zero_()


def test_scalar_apply_grid_stride(monkeypatch):
    """C 96, M 21,900: 2,102,400 elements over the 8,192 x 256 threads bn_apply_k / bn_bwd_apply_k are capped at."""
    _clean(monkeypatch)
    assert 21900 * 96 > 8192 * 256
    cs = Case("s cap", 21900, 96, OPTS[0])
    f, b = run_pair(cs, "rand", "scalar", "scalar")
    assert f["plan"]["ga"] == 8192 and b["plan"]["ga"] == 8192


# ------------------------------------------------------------------- statistics the test states: apply_fin / pre
REP_ROWS = (0, 2, 3, 5, 7)  # the replica rows that receive a row group; 1, 4, 6 stay zero


def _replicas(M, C, a, b):
    """fp32 partial sums of five row groups of a / b ([M, C] fp32) in their replica rows: [NREP, 2C]."""
    rep = torch.zeros(NREP, 2 * C, dtype=f32)
    edges = [round(i * M / len(REP_ROWS)) for i in range(len(REP_ROWS) + 1)]
    for r, lo, hi in zip(REP_ROWS, edges, edges[1:]):
        rep[r, :C], rep[r, C:] = a[lo:hi].sum(0), b[lo:hi].sum(0)
    return rep


def _stated(rep, C):
    d = rep.double()
    s32 = torch.zeros(2 * C, dtype=f32)
    for r in range(NREP):  # the kernels' fold order
        s32 = s32 + rep[r]
    return d.sum(0), s32, d.abs().sum(0)


def run_apply_fin(cs, kind, want):
    M, C, o = cs.M, cs.C, cs.o
    xf = cs.x[kind].float()
    rep = _replicas(M, C, xf, xf * xf)
    acc = K.bn_acc(dev, C)
    acc[:NREP * 2 * C].copy_(rep.view(-1))
    X = Frame((M, C), bf, cs.x[kind])
    RES = Frame((M, C), bf, cs.res[kind]) if o["res"] else None
    Y = Frame((M, C), bf, float("nan"))
    MEAN, RSTD = Frame((C,), f32, float("nan")), Frame((C,), f32, float("nan"))
    RM, RV = (Frame((C,), f32, cs.rm), Frame((C,), f32, cs.rv)) if o["run"] else (None, None)
    G = Frame((C,), f32, cs.gamma) if o["g"] else None
    B = Frame((C,), f32, cs.beta) if o["b"] else None
    plan = K.bn_fwd_apply_fin_path(X.v, Y.v, _v(RES))
    tag = f"{cs.name} {kind} apply_fin:{plan['route']}"
    assert plan["route"] == want and K.bn_prestats_ok(C), tag
    K.bn_fwd_apply_fin(X.v, _v(G), _v(B), MEAN.v, RSTD.v, _v(RM), _v(RV), MOM, EPS, residual=_v(RES),
                       act=cs.act(kind), out=Y.v)
    torch.cuda.synchronize()
    acc_at_rest(acc, C, tag)
    for fr in (X, RES, G, B):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    for fr in (Y, MEAN, RSTD, RM, RV):
        assert fr is None or fr.intact(), (tag, "sentinels")
    out = dict(mean=MEAN.host(), rstd=RSTD.host(), y=Y.host(), rm=RM.host() if RM else None,
               rv=RV.host() if RV else None, plan=plan)
    t64, t32, tabs = _stated(rep, C)
    check_forward(tag, "pre" if want == "defer" else "fold", cs, kind, out,
                  (t64[:C], t64[C:], t32[:C], t32[C:], tabs[:C], tabs[C:]), NREP)
    return out


def run_bwd_pre(cs, kind, want):
    """g = dy is the act'-masked gradient; mean / rstd are the fp32 roundings of the fp64 statistics of x."""
    M, C, o = cs.M, cs.C, cs.o
    _, _, mean64, var64, _ = bn_stats_reference(cs.x[kind])
    fwd = dict(mean=mean64.float(), rstd=(1.0 / torch.sqrt(var64 + EPS32)).float())
    gf = cs.dy[kind].float()
    xhat = (cs.x[kind].float() - fwd["mean"]) * fwd["rstd"]
    rep = _replicas(M, C, gf, gf * xhat)
    acc = torch.zeros(NREP * 2 * C + 12 * 32, device=dev, dtype=f32)
    acc[:NREP * 2 * C].copy_(rep.view(-1))
    DY, X = Frame((M, C), bf, cs.dy[kind]), Frame((M, C), bf, cs.x[kind])
    DX = Frame((M, C), bf, float("nan"))
    G = Frame((C,), f32, cs.gamma) if o["g"] else None
    MEAN, RSTD = Frame((C,), f32, fwd["mean"]), Frame((C,), f32, fwd["rstd"])
    DG = Frame((C,), f32, cs.dg[kind]) if o["dg"] else None
    DB = Frame((C,), f32, cs.db[kind]) if o["db"] else None
    WS = Frame((2 * C,), f32, float("nan"))
    plan = K.bn_bwd_pre_path(DY.v, X.v, DX.v, acc)
    tag = f"{cs.name} {kind} bwd_pre:{plan['route']}"
    assert plan["route"] == want, tag
    K.bn_bwd_pre(DY.v, X.v, _v(G), MEAN.v, RSTD.v, _v(DG), _v(DB), WS.v, acc, out=DX.v)
    torch.cuda.synchronize()
    acc_at_rest(acc, C, tag)
    for fr in (DY, X, G, MEAN, RSTD):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    for fr in (DX, DG, DB, WS):
        assert fr is None or fr.intact(), (tag, "sentinels")
    out = dict(ws=WS.host(), dx=DX.host(), dres=None, dg=DG.host() if DG else None, db=DB.host() if DB else None)
    t64, t32, tabs = _stated(rep, C)
    check_backward(tag, want, cs, kind, fwd, out, NREP, None, None, launcher="p",
                   stated=(t64[:C], t64[C:], t32[:C], t32[C:], tabs[:C], tabs[C:]))
    return out


PRE_SHAPES = ((8, 1030), (64, 37), (512, 21), (2048, 5), (16, 1))


def pre_cases():
    return [Case(f"pre C{C} M{M}", M, C, OPTS[i % 8]) for i, (C, M) in enumerate(PRE_SHAPES)] + \
        [Case(f"pre2 C{C} M{M}", M, C, OPTS[(i + 5) % 8]) for i, (C, M) in enumerate(PRE_SHAPES[:3])]


def test_apply_fin_and_bwd_pre(monkeypatch):
    """bn_apply_fin8_k / bn_bwd_apply_fin8_k on replica rows the test wrote itself (five row groups in rows 0, 2, 3,
    5, 7; rows 1, 4, 6 zero): the published mean / ws are those of the stated replicas."""
    _clean(monkeypatch)
    for cs in pre_cases():
        for kind in ("rand", "twin"):
            run_apply_fin(cs, kind, "defer")
            run_bwd_pre(cs, kind, "defer")


@pytest.mark.parametrize("C,mis", [(96, None), (2056, None), (64, "x"), (64, "out")])
def test_prestats_refusal(monkeypatch, C, mis):
    """No vector route: both launchers return -2 before anything is launched; nothing is written."""
    _clean(monkeypatch)
    M = 9
    g = _gen(f"refuse {C}")
    x = torch.randn(M, C, generator=g).to(bf)
    X = Frame((M, C), bf, x, PAD + (mis == "x"))
    O = Frame((M, C), bf, float("nan"), PAD + (mis == "out"))
    V = [Frame((C,), f32, torch.randn(C, generator=g)) for _ in range(6)]
    WS = Frame((2 * C,), f32, float("nan"))
    acc = K.bn_acc(dev, C)
    own = torch.zeros(NREP * 2 * C + 12 * 32, device=dev, dtype=f32)
    rep = torch.randn(NREP * 2 * C, generator=g)
    acc[:NREP * 2 * C].copy_(rep)
    own[:NREP * 2 * C].copy_(rep)
    before = [fr.buf.cpu() for fr in (X, O, WS, *V)] + [acc.cpu(), own.cpu()]
    try:
        assert K.bn_prestats_ok(C) == (mis is not None)
        assert K.bn_fwd_apply_fin_path(X.v, O.v)["code"] == -2
        with pytest.raises(RuntimeError, match="bn_fwd_apply_fin failed with hipError -2$"):
            K.bn_fwd_apply_fin(X.v, V[0].v, V[1].v, V[2].v, V[3].v, V[4].v, V[5].v, MOM, EPS, act="relu", out=O.v)
        assert K.bn_bwd_pre_path(X.v, X.v, O.v, own)["code"] == -2
        with pytest.raises(RuntimeError, match="bn_bwd_pre failed with hipError -2$"):
            K.bn_bwd_pre(X.v, X.v, V[0].v, V[2].v, V[3].v, V[4].v, V[5].v, WS.v, own, out=O.v)
        torch.cuda.synchronize()
        after = [fr.buf.cpu() for fr in (X, O, WS, *V)] + [acc.cpu(), own.cpu()]
        for a, b in zip(before, after):
            assert bits_equal(a, b)
    finally:
        acc.zero_()


# ---------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("C,M,mis", [(8, 1, None), (64, 301, None), (2048, 3, None), (64, 301, "y"), (3, 5, None),
                                     (24, 301, None), (2056, 2, None)])
def test_inference(monkeypatch, C, M, mis):
    """bn_apply8_k alone / bn_apply_k with var_mode: running_var holds a 0 (rsqrt(eps)); residual with each act."""
    _clean(monkeypatch)
    want = "apply" if C % 8 == 0 and C <= 2048 and 256 % (C // 8) == 0 and mis is None else "scalar"
    for i, act in enumerate((None, "relu", "sigmoid", "tanh")):
        cs = Case(f"infer C{C} M{M} {act}", M, C, dict(OPTS[0], act=act, res=int(i != 0 or M > 1), g=int(i != 2),
                                                        b=int(i != 3)), mis=mis)
        cs.rv[0] = 0.0
        o = cs.o
        X = Frame((M, C), bf, cs.x["rand"], cs.off("x"))
        RES = Frame((M, C), bf, cs.res["rand"]) if o["res"] else None
        Y = Frame((M, C), bf, float("nan"), cs.off("y"))
        G = Frame((C,), f32, cs.gamma) if o["g"] else None
        B = Frame((C,), f32, cs.beta) if o["b"] else None
        RM, RV = Frame((C,), f32, cs.rm), Frame((C,), f32, cs.rv)
        plan = K.bn_fwd_infer_path(X.v, Y.v, _v(RES))
        tag = f"{cs.name} infer:{plan['route']}"
        assert plan["route"] == want, tag
        K.bn_fwd_infer(X.v, _v(G), _v(B), RM.v, RV.v, EPS, residual=_v(RES), act=act, out=Y.v)
        torch.cuda.synchronize()
        for fr in (X, RES, G, B, RM, RV):
            assert fr is None or fr.unchanged(), (tag, "an input changed")
        assert Y.intact(), tag
        y = Y.host()
        ref = bn_reference(cs.x["rand"], cs.g_(), cs.b_(), cs.rm, cs.rv, EPS, cs.r_("rand"), act, var_mode=True)
        sc = (cs.gamma.double() if o["g"] else 1.0) / torch.sqrt(cs.rv.double() + EPS32)
        mag = (cs.x["rand"].double() * sc).abs() + (cs.rm.double() * sc).abs()
        mag = mag + (cs.beta.double().abs() if o["b"] else 0) + (cs.res["rand"].double().abs() if o["res"] else 0)
        check_tol(tag, "bn_apply8_k (infer)" if want == "apply" else "bn_apply_k (infer)", "y", y, ref,
                  2.0 ** -8 * ref.abs() + 6 * ULP32 * mag)
        if act == "relu":
            assert int(y.view(torch.int16)[y == 0].count_nonzero()) == 0, (tag, "a ReLU zero is not +0")


# ------------------------------------------------------------------------------------------------ child processes
STRIDE_SHAPES = ((8, 1317), (64, 165), (512, 21), (16, 660))  # M C / 8 = 5 x 256 + 37 / 40 / 64 / 40 chunks


def stride_cases():
    return [Case(f"stride C{C} M{M}", M, C, OPTS[i]) for i, (C, M) in enumerate(STRIDE_SHAPES)]


def _twin_outs(pairs):
    return {name: dict(f={k: f[k] for k in FWD_KEYS}, b={k: b[k] for k in BWD_KEYS + ("ws", "plan")})
            for name, (f, b) in pairs.items()}


def child_fold():
    """HOPSX_BN_FOLD_MINC=0: bn_fold_k<1> + bn_bwd_apply8_k behind the deferred bn_colred8_k<1>; bn_fold_k<0/1> behind
    the stated replicas."""
    pairs = {}
    for C in (8, 512, 2048):
        for cs in vec_cases(C):
            for kind in ("rand", "twin"):
                f = run_forward(cs, kind, "defer")
                b = run_backward(cs, kind, f, "fold", zbeta=(cs.o["act"] == "relu" and not cs.o["res"]))
                if kind == "twin":
                    pairs[cs.name] = (f, b)
    for cs in pre_cases():
        for kind in ("rand", "twin"):
            run_apply_fin(cs, kind, "fold")
            run_bwd_pre(cs, kind, "fold")
    return _twin_outs(pairs)


def child_stride():
    """HOPSX_BN_MAXG=1, HOPSX_BN_APPLY_MAXG=1: one reduction workgroup walks every row, one apply workgroup takes three
    trips of two chunks, the last with its second chunk partly absent; both vector routes."""
    pairs = {}
    for cs in stride_cases():
        for kind in ("rand", "twin"):
            os.environ.pop("HOPSX_DISABLE", None)
            f, b = run_pair(cs, kind, "defer", "defer")
            assert f["plan"]["g"] == 1 and f["plan"]["ga"] == 1 and b["plan"]["ga"] == 1 and f["plan"]["rpb"] == cs.M
            os.environ["HOPSX_DISABLE"] = "bn_defer"
            f1, b1 = run_pair(cs, kind, "selffin", "selffin")
            if kind == "twin":
                same_bits(cs.name, f, f1, FWD_KEYS)
                same_backward(cs.name, b, b1)
                pairs[cs.name] = (f, b)
    os.environ.pop("HOPSX_DISABLE", None)
    for cs in pre_cases()[:3]:
        run_apply_fin(cs, "rand", "defer")
        run_bwd_pre(cs, "rand", "defer")
    return _twin_outs(pairs)


def child_coop():
    """HOPSX_BN_COOP=1: bn_bwd_coop8_k<1> at the small shapes, <2/4/8> at C 2048 with M raised in quarter
    octaves until the reporter names the next R (below 16 MB per tensor)."""
    pairs = {}
    for C in VEC_C:
        for cs in vec_cases(C):
            for kind in ("rand", "twin"):
                f = run_forward(cs, kind, "defer")
                b = run_backward(cs, kind, f, "coop")
                assert b["plan"]["R"] == 1, (cs.name, b["plan"])
                if kind == "twin":
                    pairs[cs.name] = (f, b)
    C, seen = 2048, set()
    probe = lambda m: K.bn_bwd_path(*(torch.empty(m, C, device=dev, dtype=bf),) * 4, act="relu")  # noqa: E731
    for M in sorted({int(16 * 2 ** (k / 4)) for k in range(33)}):  # 16 .. 4096 rows in quarter octaves
        p = probe(M - 3)
        if p["route"] == "coop" and p["R"] > 1 and p["R"] not in seen:
            seen.add(p["R"])
            cs = Case(f"coop R{p['R']}", M - 3, C, OPTS[(0, 2, 6)[len(seen) % 3]])
            for kind in ("rand",):
                f = run_forward(cs, kind, "defer")
                b = run_backward(cs, kind, f, "coop")
                assert b["plan"]["R"] == p["R"]
    for R in (2, 4, 8):
        if R not in seen:
            print(f"BNSKIP bn_bwd_coop8_k<{R}> not reachable below 16 MB per tensor on this device")
    return _twin_outs(pairs)


def child_det():
    """HOPSX_DETERMINISTIC=1: the workgroups add in workgroup order; two launches from the same state agree bit for
    bit and obey the sum rule with n = the workgroups adding to a channel."""
    for cs, route in ((Case("det C64 M300", 300, 64, OPTS[0]), "defer"),
                      (Case("det C130 M777", 777, 130, OPTS[0]), "scalar")):
        runs = []
        for rep in range(2):
            plan = K.bn_fwd_train_path(*(torch.empty(cs.M, cs.C, device=dev, dtype=bf),) * 2)
            assert plan["g"] * max(plan["gx"], 1) >= 3
            f = run_forward(cs, "rand", route, n=plan["g"])
            b = run_backward(cs, "rand", f, route, n=plan["g"])
            runs.append((f, b))
        same_bits(cs.name, runs[0][0], runs[1][0], FWD_KEYS)
        same_bits(cs.name, runs[0][1], runs[1][1], ("ws", "dx", "dres", "dg", "db"))
        _rec("deterministic mode", "all outputs", "two launches bit-identical")
    return {}


CHILDREN = {
    "fold": (child_fold, dict(HOPSX_BN_FOLD_MINC="0")),
    "stride": (child_stride, dict(HOPSX_BN_MAXG="1", HOPSX_BN_APPLY_MAXG="1")),
    "coop": (child_coop, dict(HOPSX_BN_COOP="1")),
    "det": (child_det, dict(HOPSX_DETERMINISTIC="1")),
}


def child_main(mode, out_path):
    outs = CHILDREN[mode][0]()
    torch.cuda.synchronize()
    torch.save(dict(outs=outs, stats=STATS), out_path)


def run_child(mode, tmp_path, timeout=150):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(CHILDREN[mode][1])
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")])
    out = tmp_path / f"{mode}.pt"
    code = "import sys, test_bn_paths_gpu as T\nT.child_main(sys.argv[1], sys.argv[2])"
    try:
        r = subprocess.run([sys.executable, "-c", code, mode, str(out)], env=env, timeout=timeout, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on that card
        pytest.exit(f"BN child '{mode}' did not end within {timeout} s, stopping the session: {e}", returncode=3)
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):  # killed by a signal / abort / segmentation fault
        pytest.exit(f"BN child '{mode}' died with {r.returncode}, stopping the session:\n{r.stderr[-3000:]}",
                    returncode=3)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = torch.load(out, weights_only=False)
    for k, (n, w) in got["stats"].items():
        e = STATS.setdefault(k, [0, 0.0])  # the child's checks count in the same rows as the parent's
        e[0], e[1] = e[0] + n, max(e[1], w)
    return got["outs"]


def _compare_with_default(monkeypatch, outs, cases, forward=True):
    _clean(monkeypatch)
    by = {cs.name: cs for cs in cases}
    assert set(outs) == set(by)
    for name, o in outs.items():
        f, b = default_pair(by[name], "twin")
        if forward:
            same_bits(name, f, o["f"], FWD_KEYS)
        agree, of = same_backward(name, b, o["b"])
        if by[name].M == 1:  # one term per channel: sum dz xhat cannot depend on the route
            assert agree == of, (name, "ws[C:2C] of a single row differs across routes")


def test_fold_first_child(monkeypatch, tmp_path):
    outs = run_child("fold", tmp_path)
    _compare_with_default(monkeypatch, outs, [cs for C in (8, 512, 2048) for cs in vec_cases(C)])


def test_grid_stride_child(monkeypatch, tmp_path):
    outs = run_child("stride", tmp_path)
    _compare_with_default(monkeypatch, outs, stride_cases())


def test_cooperative_backward_child(monkeypatch, tmp_path):
    outs = run_child("coop", tmp_path, timeout=240)
    _compare_with_default(monkeypatch, outs, [cs for C in VEC_C for cs in vec_cases(C)])


def test_deterministic_mode_child(tmp_path):
    run_child("det", tmp_path)


EXACT_RULES = ("exact", "value", "float32(old + ws)", "count")


def test_zz_measured_table():
    """Prints what this process and its children measured, in the layout of the module docstring's table (run the
    whole file with -s): kernel, output, rule, checks, worst ratio error / bound."""
    print()
    for (kern, out, rule), (n, w) in sorted(STATS.items()):
        worst = "no mismatch" if rule in EXACT_RULES or "bit-identical" in rule else f"{w:.3f}"
        print(f"BNTABLE   {kern:26s} {out:16s} {rule:34s} {n:5d}  {worst}")
