"""The dense GEMM of csrc/ops/gemm.hip (the dense half of gemm_core.h) behind kernels.gemm_raw / linear_fwd /
linear_dgrad / linear_wgrad / linear_bwd_pair against the plain fp64 references of hops_examples_amd.ops.functional
(``gemm_reference`` / ``linear_bwd_reference``), each case on the route it names: ``kernels.gemm_path`` and
``kernels.linear_bwd_pair_path`` report the launcher's own decision (direct / atomic / ticket / finish, the tile, the K
split, the vector loaders; pair / separate / refuse, the two tiles, store / atomic dW, dact / pool epilogue) and every
case asserts it before anything is compared.

Operands are built on the host from a seeded generator; every tensor lives inside a larger buffer whose sentinel
bands (and, with a leading dimension above the row length, gap columns) must stay untouched; outputs start as NaN,
accumulating outputs from a non-zero ``old``; inputs must be unchanged.  After EVERY launch that was given a
workspace the whole workspace and all 8192 words of kernels.ticket() are read back and must be zero.

Exact twins are the backbone: every case runs with integer operands, |v| <= 8 (sigmoid / tanh masks and aux from
{0, 0.5, 1}, whose derivatives 0.25 / 0.75 / 1 / 0 keep products exact; the sigmoid / tanh STORE epilogues run as
relu in the twin).  Every partial sum is an integer (or a quarter) far below 2^24, so the result is exact in any
accumulation order: fp32 outputs, column sums, row sums and atomic dW (``float32(old + exact)``) are compared bit for
bit, bf16 outputs equal the bf16 rounding of the exact value, ReLU zeros are +0.

Tolerance cases (normal operands; sigmoid and tanh epilogues) use the project's rule: an fp32 value within
MARGIN = 8 x the error of the fp32 torch CPU evaluation of the same reference, that yardstick floored at
(1 + 0.29 sqrt(n - 1)) fp32 ulp of sum |a||b| |alpha| + |bias| + |beta old| (x |act'| for the DACT epilogue); n = K,
for a column sum M K and the sum over M of the magnitudes, for a row sum K and sum |a|.  bf16 outputs add
2^-8 |ref64|.  Every check prints ``GEMMERR <case> <route> <output> err bound ratio``.

The latched knobs (HOPSX_GEMM_T64_MIN / _T128_MIN / _SPLIT_CFG / _SPLIT_TARGET, HOPSX_SPLIT_MINKT,
HOPSX_DETERMINISTIC) run in fresh child processes, one at a time, each under its own timeout, that import this module
and rerun a stated subset; their twins must equal the parent's bits.  HOPSX_DISABLE is read per call and toggled
in-process.

Measured on an MI355X, release build, over this file's cases (profiles/r26_gemm_paths.txt; test_zz_measured_table
prints exactly these rows; a child's checks count in the parent's rows).  Worst = worst error / yardstick for the
"8 x yard" rule (allowed up to MARGIN = 8), error / bound for the bf16 rule.

  kernel / route                               output           rule                         checks  worst
  cross-route                                  HOPSX_DISABLE    bit-identical                    8  no mismatch
  cross-route                                  deterministic mode bit-identical                   24  no mismatch
  cross-route                                  finish = ticket  bit-identical                    9  no mismatch
  cross-route                                  split knobs      bit-identical                   26  no mismatch
  cross-route                                  tile knobs t128  bit-identical                   48  no mismatch
  cross-route                                  tile knobs t64   bit-identical                   48  no mismatch
  deterministic mode                           out, colsum      two launches bit-identical       1  no mismatch
  linear_bwd_pair_k<128,128> atomic dact       dbias            8 x yard                         1  0.031
  linear_bwd_pair_k<128,128> atomic dact       dbias            exact                            1  no mismatch
  linear_bwd_pair_k<128,128> atomic dact       dw               8 x yard                         1  0.150
  linear_bwd_pair_k<128,128> atomic dact       dw               exact                            1  no mismatch
  linear_bwd_pair_k<128,128> atomic dact       dx               8 x yard + 2^-8                  1  0.988
  linear_bwd_pair_k<128,128> atomic dact       dx               exact                            1  no mismatch
  linear_bwd_pair_k<128,32> atomic dact        dbias            8 x yard                         1  0.028
  linear_bwd_pair_k<128,32> atomic dact        dbias            exact                            1  no mismatch
  linear_bwd_pair_k<128,32> atomic dact        dw               8 x yard                         1  0.207
  linear_bwd_pair_k<128,32> atomic dact        dw               exact                            1  no mismatch
  linear_bwd_pair_k<128,32> atomic dact        dx               8 x yard + 2^-8                  1  0.984
  linear_bwd_pair_k<128,32> atomic dact        dx               exact                            1  no mismatch
  linear_bwd_pair_k<128,64> atomic dact        dbias            8 x yard                         1  0.033
  linear_bwd_pair_k<128,64> atomic dact        dbias            exact                            1  no mismatch
  linear_bwd_pair_k<128,64> atomic dact        dw               8 x yard                         1  0.152
  linear_bwd_pair_k<128,64> atomic dact        dw               exact                            1  no mismatch
  linear_bwd_pair_k<128,64> atomic dact        dx               8 x yard + 2^-8                  1  0.987
  linear_bwd_pair_k<128,64> atomic dact        dx               exact                            1  no mismatch
  linear_bwd_pair_k<32,128> atomic dact        dbias            8 x yard                         1  0.101
  linear_bwd_pair_k<32,128> atomic dact        dbias            exact                            1  no mismatch
  linear_bwd_pair_k<32,128> atomic dact        dw               8 x yard                         1  0.256
  linear_bwd_pair_k<32,128> atomic dact        dw               exact                            1  no mismatch
  linear_bwd_pair_k<32,128> atomic dact        dx               8 x yard + 2^-8                  1  0.962
  linear_bwd_pair_k<32,128> atomic dact        dx               exact                            1  no mismatch
  linear_bwd_pair_k<32,32> atomic dact         dbias            8 x yard                        24  0.103
  linear_bwd_pair_k<32,32> atomic dact         dbias            exact                           25  no mismatch
  linear_bwd_pair_k<32,32> atomic dact         dw               8 x yard                        27  0.316
  linear_bwd_pair_k<32,32> atomic dact         dw               exact                           28  no mismatch
  linear_bwd_pair_k<32,32> atomic dact         dx               8 x yard + 2^-8                 27  0.995
  linear_bwd_pair_k<32,32> atomic dact         dx               exact                           28  no mismatch
  linear_bwd_pair_k<32,32> atomic pool         dbias            8 x yard                         4  0.070
  linear_bwd_pair_k<32,32> atomic pool         dbias            exact                            4  no mismatch
  linear_bwd_pair_k<32,32> atomic pool         dw               8 x yard                         4  0.216
  linear_bwd_pair_k<32,32> atomic pool         dw               exact                            4  no mismatch
  linear_bwd_pair_k<32,32> atomic pool         dx               8 x yard + 2^-8                  6  0.989
  linear_bwd_pair_k<32,32> atomic pool         dx               exact                            2  no mismatch
  linear_bwd_pair_k<32,32> store dact          dbias            8 x yard                         3  0.030
  linear_bwd_pair_k<32,32> store dact          dbias            exact                            5  no mismatch
  linear_bwd_pair_k<32,32> store dact          dw               8 x yard                         3  0.169
  linear_bwd_pair_k<32,32> store dact          dw               exact                            5  no mismatch
  linear_bwd_pair_k<32,32> store dact          dx               8 x yard + 2^-8                  3  0.990
  linear_bwd_pair_k<32,32> store dact          dx               exact                            5  no mismatch
  linear_bwd_pair_k<32,64> atomic dact         dbias            8 x yard                         3  0.103
  linear_bwd_pair_k<32,64> atomic dact         dbias            exact                            3  no mismatch
  linear_bwd_pair_k<32,64> atomic dact         dw               8 x yard                         3  0.290
  linear_bwd_pair_k<32,64> atomic dact         dw               exact                            3  no mismatch
  linear_bwd_pair_k<32,64> atomic dact         dx               8 x yard + 2^-8                  3  0.989
  linear_bwd_pair_k<32,64> atomic dact         dx               exact                            3  no mismatch
  linear_bwd_pair_k<64,128> atomic dact        dbias            8 x yard                         1  0.062
  linear_bwd_pair_k<64,128> atomic dact        dbias            exact                            1  no mismatch
  linear_bwd_pair_k<64,128> atomic dact        dw               8 x yard                         1  0.316
  linear_bwd_pair_k<64,128> atomic dact        dw               exact                            1  no mismatch
  linear_bwd_pair_k<64,128> atomic dact        dx               8 x yard + 2^-8                  1  0.990
  linear_bwd_pair_k<64,128> atomic dact        dx               exact                            1  no mismatch
  linear_bwd_pair_k<64,32> atomic dact         dbias            8 x yard                         3  0.046
  linear_bwd_pair_k<64,32> atomic dact         dbias            exact                            3  no mismatch
  linear_bwd_pair_k<64,32> atomic dact         dw               8 x yard                         3  0.207
  linear_bwd_pair_k<64,32> atomic dact         dw               exact                            3  no mismatch
  linear_bwd_pair_k<64,32> atomic dact         dx               8 x yard + 2^-8                  3  0.984
  linear_bwd_pair_k<64,32> atomic dact         dx               exact                            3  no mismatch
  linear_bwd_pair_k<64,64> atomic dact         dbias            8 x yard                         9  0.062
  linear_bwd_pair_k<64,64> atomic dact         dbias            exact                            9  no mismatch
  linear_bwd_pair_k<64,64> atomic dact         dw               8 x yard                         9  0.316
  linear_bwd_pair_k<64,64> atomic dact         dw               exact                            9  no mismatch
  linear_bwd_pair_k<64,64> atomic dact         dx               8 x yard + 2^-8                  9  0.991
  linear_bwd_pair_k<64,64> atomic dact         dx               exact                            9  no mismatch
  linear_wgrad                                 atomic           8 x yard                         3  0.031
  linear_wgrad                                 atomic           exact                            3  no mismatch
  linear_wgrad                                 rowsum           8 x yard                         3  0.008
  linear_wgrad                                 rowsum           exact                            3  no mismatch
  mfma_gemm<128> atomic                        atomic           8 x yard                         2  0.233
  mfma_gemm<128> atomic                        atomic           exact                            2  no mismatch
  mfma_gemm<128> atomic                        rowsum           8 x yard                         2  0.067
  mfma_gemm<128> atomic                        rowsum           exact                            2  no mismatch
  mfma_gemm<128> direct                        bf16             8 x yard + 2^-8                  1  0.992
  mfma_gemm<128> direct                        bf16             exact                            2  no mismatch
  mfma_gemm<128> direct                        colsum           8 x yard                         2  0.003
  mfma_gemm<128> direct                        colsum           exact                            2  no mismatch
  mfma_gemm<128> direct                        dact             8 x yard + 2^-8                  1  0.972
  mfma_gemm<128> direct                        dact             exact                            1  no mismatch
  mfma_gemm<128> direct                        f32              8 x yard                         2  0.187
  mfma_gemm<128> direct                        f32              exact                            2  no mismatch
  mfma_gemm<128> direct                        rowsum           8 x yard                         1  0.036
  mfma_gemm<128> direct                        rowsum           exact                            1  no mismatch
  mfma_gemm<32> atomic                         atomic           8 x yard                        37  0.288
  mfma_gemm<32> atomic                         atomic           exact                           43  no mismatch
  mfma_gemm<32> atomic                         colsum           8 x yard                         4  0.003
  mfma_gemm<32> atomic                         colsum           exact                            4  no mismatch
  mfma_gemm<32> atomic                         rowsum           8 x yard                        35  0.110
  mfma_gemm<32> atomic                         rowsum           exact                           41  no mismatch
  mfma_gemm<32> direct                         bf16             8 x yard + 2^-8                 25  0.992
  mfma_gemm<32> direct                         bf16             exact                           21  no mismatch
  mfma_gemm<32> direct                         colsum           8 x yard                        52  0.048
  mfma_gemm<32> direct                         colsum           exact                           49  no mismatch
  mfma_gemm<32> direct                         dact             8 x yard + 2^-8                 18  0.985
  mfma_gemm<32> direct                         dact             exact                           18  no mismatch
  mfma_gemm<32> direct                         f32              8 x yard                        33  0.187
  mfma_gemm<32> direct                         f32              exact                           34  no mismatch
  mfma_gemm<32> direct                         rowsum           8 x yard                        10  0.060
  mfma_gemm<32> direct                         rowsum           exact                           10  no mismatch
  mfma_gemm<32> finish                         bf16             8 x yard + 2^-8                  5  0.918
  mfma_gemm<32> finish                         bf16             exact                            5  no mismatch
  mfma_gemm<32> finish                         colsum           8 x yard                        11  0.006
  mfma_gemm<32> finish                         colsum           exact                           11  no mismatch
  mfma_gemm<32> finish                         dact             8 x yard + 2^-8                  3  0.962
  mfma_gemm<32> finish                         dact             exact                            3  no mismatch
  mfma_gemm<32> finish                         f32              8 x yard                         3  0.026
  mfma_gemm<32> finish                         f32              exact                            3  no mismatch
  mfma_gemm<32> ticket                         bf16             8 x yard + 2^-8                  6  0.918
  mfma_gemm<32> ticket                         bf16             exact                           21  no mismatch
  mfma_gemm<32> ticket                         colsum           8 x yard                        18  0.007
  mfma_gemm<32> ticket                         colsum           exact                           52  no mismatch
  mfma_gemm<32> ticket                         dact             8 x yard + 2^-8                  6  0.962
  mfma_gemm<32> ticket                         dact             exact                           18  no mismatch
  mfma_gemm<32> ticket                         f32              8 x yard                         6  0.026
  mfma_gemm<32> ticket                         f32              exact                           16  no mismatch
  mfma_gemm<32> ticket                         f32              graph = eager                    2  no mismatch
  mfma_gemm<64> atomic                         atomic           8 x yard                         4  0.233
  mfma_gemm<64> atomic                         atomic           exact                            4  no mismatch
  mfma_gemm<64> atomic                         rowsum           8 x yard                         4  0.067
  mfma_gemm<64> atomic                         rowsum           exact                            4  no mismatch
  mfma_gemm<64> direct                         bf16             8 x yard + 2^-8                  3  0.992
  mfma_gemm<64> direct                         bf16             exact                            4  no mismatch
  mfma_gemm<64> direct                         colsum           8 x yard                         6  0.004
  mfma_gemm<64> direct                         colsum           exact                            6  no mismatch
  mfma_gemm<64> direct                         dact             8 x yard + 2^-8                  3  0.972
  mfma_gemm<64> direct                         dact             exact                            3  no mismatch
  mfma_gemm<64> direct                         f32              8 x yard                         6  0.187
  mfma_gemm<64> direct                         f32              exact                            6  no mismatch
  mfma_gemm<64> direct                         rowsum           8 x yard                         3  0.036
  mfma_gemm<64> direct                         rowsum           exact                            3  no mismatch

Defects this file pins down:

* ``K = 0`` read one element of A and B (launch_gemm raised K to 1): wrong result from valid operands, an
  out-of-bounds read from empty ones.  Held by test_degenerate.  The kernel now runs the epilogue on a zero
  accumulator and reads nothing.
* ``M = 0`` (or ``N = 0``) with a workspace divided by a zero tile count on the host (want_splitk -> plan_gemm).
  Held by test_degenerate and test_gemm_reference_cpu.py.
* The ``finish`` route left the partial sums in the workspace (not zero at rest: the next ticket GEMM on the same
  workspace would add onto them).  Held by the at-rest check of test_finish_route.  splitk_finish_k now zeroes what
  it reads.
* The ticket finish's column sum left out ``beta * old`` where the direct epilogue includes it.  Held by
  test_ticket_split_k's beta case (colsum twin, equal to the finish route's bits in test_finish_route).
* ``hopsx_disabled`` matched substrings: HOPSX_DISABLE=splitk_ticket also turned ``splitk`` off, so the ``finish``
  route was unreachable from the launchers.  Held by test_disable_knobs.  Whole comma-separated tokens now.

Each of these four reverts was built on a scratch copy of gemm_core.h and run against the twins; the case that failed:
the rowsum's ``tn == 0`` condition: test_atomic_split_wgrad[513-20-70] (three column tiles: 19 of 20 dbias rows
wrong, the all-zero dY column alone still right); the re-zeroing of the workspace tile: the at-rest check after the
first launch of test_ticket_split_k (all 4096 workspace words left non-zero); the ``i + 8 <= ilim`` guard of the
vector load: test_loader_branches ``tail`` without a mask and with the aligned mask (K = 77 in rows of 80: the last
chunk carries the gap columns' sentinels into the product, 1750 of 1755 outputs wrong; the misaligned mask takes the
scalar branch and passes); the ``beta`` term in the ticket finish: the ``splitk f32 beta`` twin of
test_ticket_split_k (4075 of 4096 outputs wrong).
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
from hops_examples_amd.ops._C import ptr, stream  # noqa: E402
from hops_examples_amd.ops.functional import _act_grad_from_out, gemm_reference, linear_bwd_reference  # noqa: E402

dev = torch.device("cuda", 0)
f32, bf, f64 = torch.float32, torch.bfloat16, torch.float64
MARGIN = 8.0
ULP32 = 2.0 ** -23
PAD = 64
SENT = {f32: -7777.25, bf: -3.0}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {}  # (kernel, output, rule) -> [checks, worst ratio]
KNOBS = ("HOPSX_GEMM_T64_MIN", "HOPSX_GEMM_T128_MIN", "HOPSX_GEMM_SPLIT_CFG", "HOPSX_GEMM_SPLIT_TARGET",
         "HOPSX_SPLIT_MINKT", "HOPSX_DETERMINISTIC", "HOPSX_DISABLE")
EPI = {"bf16": K.EPI_STORE_BF16, "f32": K.EPI_STORE_F32, "atomic": K.EPI_ATOMIC_F32, "dact": K.EPI_DACT_BF16}
REF_EPI = {"bf16": "store", "f32": "store", "atomic": "atomic", "dact": "dact"}
DET = os.environ.get("HOPSX_DETERMINISTIC", "") == "1"


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


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Fr:
    """A [rows, cols] tensor with leading dimension ``ld`` inside a device buffer of sentinels, starting ``off``
    elements in (off = PAD: 16-byte aligned; PAD + 1: one element past).  ``init``: a host tensor or a fill value."""

    def __init__(self, rows, cols, dtype, init, ld=None, off=PAD):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, dtype
        span = (rows - 1) * ld + cols if rows > 0 and cols > 0 else 0
        h = torch.full((off + span + PAD,), SENT[dtype], dtype=dtype)
        self.inside = torch.zeros(h.numel(), dtype=torch.bool)
        hv = torch.as_strided(h, (rows, cols), (ld, 1), off)
        torch.as_strided(self.inside, (rows, cols), (ld, 1), off).fill_(True)
        if isinstance(init, float):
            hv.fill_(init)
        else:
            hv.copy_(init.to(dtype))
        self.h0 = h
        self.buf = h.to(dev)
        self.v = torch.as_strided(self.buf, (rows, cols), (ld, 1), off)

    def host(self):
        return self.v.cpu().contiguous()

    def intact(self):
        h = self.buf.cpu()
        return torch.equal(_bits(h)[~self.inside], _bits(self.h0)[~self.inside])

    def unchanged(self):
        return torch.equal(_bits(self.buf.cpu()), _bits(self.h0))

    def refill(self):
        self.buf.copy_(self.h0)


def _v(fr):
    return None if fr is None else fr.v


def _ulps(n):
    return ULP32 * (1.0 + 0.29 * math.sqrt(max(n, 1) - 1))


def _rec(kern, out, rule, ratio=None):
    e = STATS.setdefault((kern, out, rule), [0, 0.0])
    e[0] += 1
    if ratio is not None:
        e[1] = max(e[1], ratio)


def check_yard(tag, kern, out, got, ref64, ref32, absmag, n, bf16_out=False):
    """MARGIN x max(fp32 torch error, floor) (+ 2^-8 |ref64| for a bf16 output)."""
    e = (got.double() - ref64).abs()
    yard = torch.maximum((ref32.double() - ref64).abs(), _ulps(n) * absmag)
    bound = MARGIN * yard + (2.0 ** -8 * ref64.abs() if bf16_out else 0.0)
    ok = e <= bound  # (a NaN left in an output compares false)
    ratio = (e / (bound / (1.0 if bf16_out else MARGIN)).clamp_min(1e-300)).nan_to_num(nan=float("inf"))[bound > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"GEMMERR {tag} {out} {float(e.nan_to_num(nan=float('inf')).max()):.3e} {float(bound.max()):.3e} "
          f"{worst / (1.0 if bf16_out else MARGIN):.3f}")
    _rec(kern, out, "8 x yard + 2^-8" if bf16_out else "8 x yard", worst)
    assert bool(ok.all()), (tag, out, int((~ok).sum()), worst)


def check_exact(tag, kern, out, got, want, rule="exact"):
    bad = got.numel() if got.shape != want.shape or got.dtype != want.dtype else int((_bits(got) != _bits(want)).sum())
    print(f"GEMMERR {tag} {out} exact mismatches {bad} of {got.numel()}")
    _rec(kern, out, rule)
    assert bad == 0, (tag, out, bad)


def at_rest(tag, ws):
    """The workspace (a Fr, or the launchers' persistent buffer) and every ticket word read zero."""
    torch.cuda.synchronize()
    if isinstance(ws, Fr):
        assert ws.intact(), (tag, "workspace sentinels")
        w = _bits(ws.host())
    else:
        w = _bits(ws.cpu())
    assert not bool(w.any()), (tag, "workspace not zero at rest", int(w.count_nonzero()))
    t = K.ticket(dev).cpu()
    assert t.numel() == 8192 and not bool(t.any()), (tag, "tickets not zero at rest", int(t.count_nonzero()))


# ------------------------------------------------------------------------------------------------- one GEMM case
DEFAULTS = dict(a_kc=True, b_kc=True, epi="bf16", alpha=1.0, beta=0.0, bias=False, act=None, colsum=False, mask=None,
                mask_off=PAD, rowsum=False, a_off=PAD, b_off=PAD, a_pad=0, b_pad=0, ldo_pad=0, ldaux_pad=0, ws=None,
                tickets=True, zero_col=False, route=None, tile=None, avec=None, bvec=None, split_min=None)


class Spec:
    def __init__(self, name, M, N, K, **kw):
        bad = set(kw) - set(DEFAULTS)
        assert not bad, bad
        self.name, self.M, self.N, self.K = name, M, N, K
        self.__dict__.update({**DEFAULTS, **kw})
        self._ops = {}

    def act_of(self, kind):
        a = self.act
        if self.epi in ("bf16", "f32") and kind == "twin" and a in ("sigmoid", "tanh"):
            return "relu"  # (a transcendental is not exact; the tolerance run keeps it)
        return a

    def ops(self, kind):
        """Host operands and both references of the case, built once per kind."""
        if kind in self._ops:
            return self._ops[kind]
        M, N, Kd = self.M, self.N, self.K
        g = _gen(f"{self.name} {kind}")
        twin = kind == "twin"
        ri = lambda *s: torch.randint(-8, 9, s, generator=g).float()  # noqa: E731
        rn = lambda *s: torch.randn(*s, generator=g) if math.prod(s) else torch.zeros(*s)  # noqa: E731

        def act_out(act, *s):  # an activation OUTPUT for act' (mask y / aux)
            if act == "relu" or act is None:
                return (ri(*s) if twin else rn(*s)).to(bf)
            if twin:
                return (torch.randint(0, 3, s, generator=g).float() / 2).to(bf)
            u = torch.rand(*s, generator=g)
            return (u if act == "sigmoid" else 2 * u - 1).to(bf)

        a = (ri(M, Kd) if twin else rn(M, Kd)).to(bf)
        b = (ri(N, Kd) if twin else rn(N, Kd)).to(bf)
        if self.zero_col:  # wgrad: A = dY^T, a dY column = an A row
            a[min(1, M - 1)] = 0
        o = dict(a=a if self.a_kc else a.t().contiguous(), b=b if self.b_kc else b.t().contiguous())
        o["y"] = None
        if self.mask:
            y = act_out(self.mask, M, Kd)
            o["y"] = y if self.a_kc else y.t().contiguous()
        o["bias"] = (ri(N) if twin else rn(N)) if self.bias else None
        old = (torch.randint(-100, 101, (M, N), generator=g).float() if twin else rn(M, N) * 3)
        o["old"] = old if (self.epi == "atomic" or self.beta != 0.0) else None
        o["aux"] = act_out(self.act, M, N) if self.epi == "dact" and self.act else None
        o["cs_old"] = (torch.randint(-100, 101, (N,), generator=g).float() if twin else rn(N) * 3)
        o["rs_old"] = (torch.randint(-100, 101, (M,), generator=g).float() if twin else rn(M) * 3)
        act = self.act_of(kind)
        kw = dict(a_kc=self.a_kc, b_kc=self.b_kc, epi=REF_EPI[self.epi], alpha=self.alpha, bias=o["bias"], act=act,
                  beta=self.beta, old=o["old"], aux=o["aux"], a_mask_y=o["y"], a_mask_act=self.mask)
        o["ref64"] = gemm_reference(o["a"], o["b"], dtype=f64, **kw)
        o["ref32"] = o["ref64"] if twin else gemm_reference(o["a"], o["b"], dtype=f32, **kw)
        # magnitudes for the floor of the yardstick
        A = o["a"].double()
        if o["y"] is not None:  # |masked A| with the reference's rounding point (an identity GEMM costs K^2 M)
            A = (A * _act_grad_from_out(o["y"].double(), self.mask)).to(bf).double()
        A = A if self.a_kc else A.t()
        Bm = o["b"].double() if self.b_kc else o["b"].double().t()
        mag = abs(self.alpha) * (A.abs() @ Bm.abs().t())
        if o["bias"] is not None and self.epi in ("bf16", "f32"):
            mag = mag + o["bias"].double().abs()
        if self.epi == "dact" and o["aux"] is not None:
            x = o["aux"].double()
            mag = mag * {"relu": (x > 0).double(), "sigmoid": (x * (1 - x)).abs(), "tanh": (1 - x * x).abs()}[self.act]
        if self.epi == "f32" and self.beta != 0.0:
            mag = mag + abs(self.beta) * o["old"].double().abs()
        o["mag_el"] = mag + (o["old"].double().abs() if self.epi == "atomic" else 0.0)
        o["mag_cs"] = mag.sum(0)
        o["mag_rs"] = A.abs().sum(1)
        self._ops[kind] = o
        return o


def run_gemm(sp, kind, ws=None, calls=1, env_tag=""):
    """Frames, the reporter, the launch(es), the untouched / at-rest checks, the comparison.  Returns the host
    outputs (for bit comparisons across routes)."""
    M, N, Kd = sp.M, sp.N, sp.K
    o = sp.ops(kind)
    act = sp.act_of(kind)
    ar, ac = (M, Kd) if sp.a_kc else (Kd, M)
    br, bc = (N, Kd) if sp.b_kc else (Kd, N)
    A = Fr(ar, ac, bf, o["a"], ld=ac + sp.a_pad, off=sp.a_off)
    B = Fr(br, bc, bf, o["b"], ld=bc + sp.b_pad, off=sp.b_off)
    Y = Fr(ar, ac, bf, o["y"], ld=ac + sp.a_pad, off=sp.mask_off) if o["y"] is not None else None
    odt = f32 if sp.epi in ("f32", "atomic") else bf
    O = Fr(M, N, odt, o["old"] if o["old"] is not None else float("nan"), ld=N + sp.ldo_pad)
    BIAS = Fr(1, N, f32, o["bias"].view(1, N)) if o["bias"] is not None else None
    AUX = Fr(M, N, bf, o["aux"], ld=N + sp.ldaux_pad) if o["aux"] is not None else None
    CS = Fr(1, N, f32, o["cs_old"].view(1, N)) if sp.colsum else None
    RS = Fr(1, M, f32, o["rs_old"].view(1, M)) if sp.rowsum else None
    if ws is None and sp.ws is not None:
        ws = Fr(1, M * N - (1 if sp.ws == "short" else 0), f32, 0.0)
    wsv = None if ws is None else ws.v.view(-1)
    if sp.tickets:
        plan = K.gemm_path(A.v, A.ld, B.v, B.ld, M, N, Kd, EPI[sp.epi], ws=wsv, a_mask_y=_v(Y))
    else:
        v = EXT().gemm_path(ptr(A.v), A.ld, ptr(B.v), B.ld, M, N, Kd, EPI[sp.epi], ptr(wsv),
                            0 if wsv is None else wsv.numel(), ptr(_v(Y)), 0)
        plan = dict(route=K.GEMM_ROUTES[v[0]], tile=v[1], split=v[2], kps=v[3], grid=v[4], avec=bool(v[5]),
                    bvec=bool(v[6]), det=bool(v[7]))
    tag = f"{sp.name}{env_tag} {kind} {plan['route']}/{plan['tile']}x{plan['split']}"
    print(f"GEMMPLAN {tag} {plan}")
    for key in ("route", "tile", "avec", "bvec"):
        want = getattr(sp, key)
        if want is not None and not (DET and key == "route"):
            assert plan[key] == want, (tag, key, plan)
    if sp.split_min is not None and not DET:
        assert plan["split"] >= sp.split_min, (tag, plan)
    if DET:
        assert plan["split"] == 1 and plan["route"] in ("direct", "atomic"), (tag, plan)
    assert plan["kps"] % 64 == 0 and plan["split"] == max(1, -(-Kd // plan["kps"])), (tag, plan)
    assert plan["grid"] == (-(-M // plan["tile"])) * (-(-N // plan["tile"])), (tag, plan)
    for _ in range(calls):
        if sp.tickets:
            K.gemm_raw(A.v, A.ld, sp.a_kc, B.v, B.ld, sp.b_kc, M, N, Kd, EPI[sp.epi], O.v, O.ld, bias=_v(BIAS),
                       alpha=sp.alpha, beta=sp.beta, act=act, aux=_v(AUX), ldaux=AUX.ld if AUX else 0, colsum=_v(CS),
                       ws=wsv, a_mask_y=_v(Y), a_mask_act=sp.mask, a_rowsum=_v(RS))
        else:
            rc = EXT().gemm(ptr(A.v), A.ld, int(sp.a_kc), ptr(B.v), B.ld, int(sp.b_kc), M, N, Kd, EPI[sp.epi],
                            ptr(O.v), O.ld, ptr(_v(BIAS)), sp.alpha, sp.beta, K.act_id(act), ptr(_v(AUX)),
                            AUX.ld if AUX else 0, ptr(_v(CS)), ptr(wsv), 0 if wsv is None else wsv.numel(),
                            ptr(_v(Y)), K.act_id(sp.mask), ptr(_v(RS)), 0, stream())
            assert rc == 0, (tag, rc)
        if ws is not None:
            at_rest(tag, ws)
    torch.cuda.synchronize()
    for fr in (A, B, Y, BIAS, AUX):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    for fr in (O, CS, RS):
        assert fr is None or fr.intact(), (tag, "sentinels or gap columns of an output changed")
    kern = f"mfma_gemm<{plan['tile']}> {plan['route']}"
    out, r64, r32 = O.host(), o["ref64"], o["ref32"]
    got = dict(out=out, plan=plan)
    if CS is not None:
        got["cs"] = CS.host().view(-1)
    if RS is not None:
        got["rs"] = RS.host().view(-1)
    if calls > 1:  # accumulating epilogues only: old + calls * increment (exact for the twin)
        assert sp.epi == "atomic" and sp.beta == 0.0
    inc = calls  # the column / row sums accumulate with every call
    ref_out64 = r64[0] if calls == 1 else o["old"].double() + calls * (r64[0] - o["old"].double())
    ref_out32 = r32[0] if calls == 1 else o["old"].float() + calls * (r32[0] - o["old"].float())
    if kind == "twin":
        check_exact(tag, kern, sp.epi, out, ref_out64.to(odt))
        if act == "relu" and sp.epi in ("bf16", "f32"):
            assert int(_bits(out)[out == 0].count_nonzero()) == 0, (tag, "a ReLU zero is not +0")
        if CS is not None:
            check_exact(tag, kern, "colsum", got["cs"], (o["cs_old"].double() + inc * r64[1]).float())
        if RS is not None:
            check_exact(tag, kern, "rowsum", got["rs"], (o["rs_old"].double() + inc * r64[2]).float())
    else:
        check_yard(tag, kern, sp.epi, out, ref_out64, ref_out32, calls * o["mag_el"], Kd, bf16_out=odt == bf)
        if CS is not None:
            check_yard(tag, kern, "colsum", got["cs"], o["cs_old"].double() + inc * r64[1],
                       o["cs_old"] + inc * r32[1], o["cs_old"].double().abs() + inc * o["mag_cs"], M * max(Kd, 1))
        if RS is not None:
            check_yard(tag, kern, "rowsum", got["rs"], o["rs_old"].double() + inc * r64[2],
                       o["rs_old"] + inc * r32[2], o["rs_old"].double().abs() + inc * o["mag_rs"], Kd)
    return got


def both(sp, **kw):
    return {kind: run_gemm(sp, kind, **kw) for kind in ("twin", "rand")}


def _clean(monkeypatch):
    monkeypatch.delenv("HOPSX_DISABLE", raising=False)


# --------------------------------------------------------------------------------------------------------- tiles
T32 = ((7, 5, 13), (33, 10, 20), (300, 50, 77))


@pytest.mark.parametrize("M,N,Kd", T32)
def test_tile32_ragged(monkeypatch, M, N, Kd):
    """Ragged M, N and K on the 32 x 32 tile: N below a fragment, K below one BK of 64, several tiles."""
    _clean(monkeypatch)
    both(Spec(f"t32 fwd {M}x{N}x{Kd}", M, N, Kd, bias=True, act="relu", colsum=True, route="direct", tile=32))
    both(Spec(f"t32 dgrad {M}x{N}x{Kd}", M, N, Kd, b_kc=False, epi="dact", act="relu", mask="relu", colsum=True,
              route="direct", tile=32))
    both(Spec(f"t32 wgrad {M}x{N}x{Kd}", M, N, Kd, a_kc=False, b_kc=False, epi="atomic", rowsum=True, mask="relu",
              route="atomic", tile=32))


@pytest.mark.parametrize("M,N,Kd,tile", [(1409, 1409, 40, 64), (2049, 2049, 72, 128)])
def test_big_tiles_default_knobs(monkeypatch, M, N, Kd, tile):
    """The 64 x 64 and 128 x 128 tiles as linear_fwd reaches them on the default knobs (integer twins)."""
    _clean(monkeypatch)
    if DET:
        pytest.skip("default-knob case")
    g = _gen(f"big {M}")
    x = torch.randint(-8, 9, (M, Kd), generator=g).to(bf)
    w = torch.randint(-8, 9, (N, Kd), generator=g).to(bf)
    b = torch.randint(-8, 9, (N,), generator=g).float()
    X, W, BIAS, O = Fr(M, Kd, bf, x), Fr(N, Kd, bf, w), Fr(1, N, f32, b.view(1, N)), Fr(M, N, bf, float("nan"))
    plan = K.gemm_path(X.v, Kd, W.v, Kd, M, N, Kd, EPI["bf16"])
    tag = f"linear_fwd {M}x{N}x{Kd} twin {plan['route']}/{plan['tile']}"
    assert plan["route"] == "direct" and plan["tile"] == tile and plan["split"] == 1, (tag, plan)
    K.linear_fwd(X.v, W.v, bias=BIAS.v.view(-1), act="relu", out=O.v)
    torch.cuda.synchronize()
    assert X.unchanged() and W.unchanged() and BIAS.unchanged() and O.intact(), tag
    ref = torch.relu((x.float() @ w.float().t()) + b)  # (integers below 2^24: the fp32 matmul is exact)
    check_exact(tag, f"mfma_gemm<{tile}> direct", "bf16", O.host(), ref.to(bf))


# ------------------------------------------------------------------------------------------- layouts x epilogues
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("epi", ["bf16", "f32", "atomic", "dact"])
def test_layouts_and_epilogues(monkeypatch, a_kc, b_kc, epi):
    _clean(monkeypatch)
    M, N, Kd = 37, 41, 70
    sp = Spec(f"layout {int(a_kc)}{int(b_kc)} {epi}", M, N, Kd, a_kc=a_kc, b_kc=b_kc, epi=epi, bias=epi in ("bf16", "f32"),
              act="relu" if epi != "atomic" else None, colsum=True, rowsum=not a_kc,
              route="atomic" if epi == "atomic" else "direct", tile=32)
    both(sp)


# ------------------------------------------------------------------------------------------------ loader branches
LOADER = {  # name: (a_off, a_pad, K, avec)
    "aligned": (PAD, 0, 72, True),      # ld % 8 == 0, 16-byte base, no tail
    "base+1": (PAD + 1, 0, 72, False),  # the base moved by one element
    "ld=K+1": (PAD, 1, 70, False),      # ld = 71: ld % 8 != 0
    "tail": (PAD, 3, 77, True),         # ld = 80, K = 77: the last chunk has i + 8 > ilim, gap columns = sentinels
}


@pytest.mark.parametrize("name", list(LOADER))
@pytest.mark.parametrize("mask", [None, "aligned", "misaligned"])
def test_loader_branches(monkeypatch, name, mask):
    """The vector and the scalar DenseLoader branch of A (KC and RC layout) and of B, with and without the act' mask;
    a mask 2 bytes off a 16-byte line turns the vector branch off while A itself is aligned."""
    _clean(monkeypatch)
    a_off, a_pad, Kd, avec = LOADER[name]
    if mask == "misaligned":
        avec = False
    kw = dict(mask=None if mask is None else ("relu" if name != "tail" else "tanh"),
              mask_off=a_off if mask != "misaligned" else a_off + 1)
    both(Spec(f"loader {name} {mask} kc", 45, 39, Kd, epi="f32", a_off=a_off, a_pad=a_pad, b_off=a_off, b_pad=a_pad,
              avec=avec, bvec=LOADER[name][3], route="direct", **kw))
    # RC: the contiguous axis is M (A) / N (B): M = Kd makes the same ld / tail arithmetic apply there
    both(Spec(f"loader {name} {mask} rc", Kd, Kd, 45, a_kc=False, b_kc=False, epi="atomic", rowsum=True, a_off=a_off,
              a_pad=a_pad, b_off=a_off, b_pad=a_pad, avec=avec, bvec=LOADER[name][3], route="atomic", **kw))


# ----------------------------------------------------------------------------------------------- epilogue options
def test_epilogue_options(monkeypatch):
    _clean(monkeypatch)
    M, N, Kd = 45, 39, 70
    for act in (None, "relu", "sigmoid", "tanh"):
        both(Spec(f"epi bf16 {act}", M, N, Kd, epi="bf16", alpha=0.5, bias=True, act=act, colsum=True, ldo_pad=3,
                  route="direct"))
        both(Spec(f"epi f32 {act}", M, N, Kd, epi="f32", alpha=-2.0, beta=2.0, bias=True, act=act, colsum=True,
                  ldo_pad=3, route="direct"))
        both(Spec(f"epi dact {act}", M, N, Kd, b_kc=False, epi="dact", act=act, colsum=True, ldo_pad=3, ldaux_pad=5,
                  mask=act, route="direct"))
    both(Spec("epi atomic alpha", M, N, Kd, a_kc=False, b_kc=False, epi="atomic", alpha=0.25, ldo_pad=3, rowsum=True,
              route="atomic"))
    both(Spec("epi f32 plain", M, N, Kd, epi="f32", route="direct"))  # beta = 0 onto NaN: old is never read


# ------------------------------------------------------------------------------------------------- ticket split-K
TICKET = [dict(M=32, N=128, K=1024), dict(M=32, N=128, K=1030), dict(M=5, N=33, K=769)]


def ticket_specs(route, tickets=True):
    want = route if not DET else None
    out = []
    for i, s in enumerate(TICKET):
        M, N, Kd = s["M"], s["N"], s["K"]
        kw = dict(ws="own", tickets=tickets, route=want, split_min=4 if route in ("ticket", "finish") else None)
        out += [Spec(f"splitk fwd {M}x{N}x{Kd}", M, N, Kd, epi="bf16", bias=True, act=("relu", "tanh", "sigmoid")[i],
                     colsum=True, **kw),
                Spec(f"splitk f32 beta {M}x{N}x{Kd}", M, N, Kd, epi="f32", alpha=0.5, beta=2.0, bias=True, colsum=True,
                     ldo_pad=3, **kw),
                Spec(f"splitk dgrad {M}x{N}x{Kd}", M, N, Kd, b_kc=False, epi="dact", act=("relu", "sigmoid", "tanh")[i],
                     mask="relu", colsum=True, ldaux_pad=5, **kw)]
    return out


def test_ticket_split_k(monkeypatch):
    """The in-launch finish: K tails (1030: a 6-element last slice; 769: one element), beta and colsum inside the
    finish, the workspace and the tickets zero after every launch, two GEMMs back to back on one workspace."""
    _clean(monkeypatch)
    for sp in ticket_specs("ticket"):
        both(sp)
    sp = ticket_specs("ticket")[0]
    ws = Fr(1, sp.M * sp.N, f32, 0.0)
    a = run_gemm(sp, "twin", ws=ws)
    b = run_gemm(ticket_specs("ticket")[2], "twin", ws=ws)  # a smaller GEMM on the same workspace
    c = run_gemm(sp, "twin", ws=ws)
    assert bits_equal(a["out"], c["out"]) and bits_equal(a["cs"], c["cs"]) and b["plan"]["route"] == a["plan"]["route"]


def test_short_workspace_goes_direct(monkeypatch):
    _clean(monkeypatch)
    s = TICKET[2]
    both(Spec("splitk short ws", s["M"], s["N"], s["K"], epi="bf16", bias=True, ws="short", route="direct"))


def test_ticket_through_the_launchers(monkeypatch):
    """linear_fwd and linear_dgrad with the launchers' own persistent workspace (kernels._splitk_ws)."""
    _clean(monkeypatch)
    for Kd in (1024, 1030):
        M, N = 32, 128
        g = _gen(f"launcher {Kd}")
        x = torch.randint(-8, 9, (M, Kd), generator=g).to(bf)
        w = torch.randint(-8, 9, (N, Kd), generator=g).to(bf)
        b = torch.randint(-8, 9, (N,), generator=g).float()
        X, W, O = Fr(M, Kd, bf, x), Fr(N, Kd, bf, w), Fr(M, N, bf, float("nan"))
        ws = K._splitk_ws(M, N, Kd, dev)
        assert ws is not None and ws.numel() == M * N
        plan = K.gemm_path(X.v, Kd, W.v, Kd, M, N, Kd, EPI["bf16"], ws=ws)
        tag = f"linear_fwd 32x128x{Kd} twin {plan['route']}"
        assert plan["route"] == ("direct" if DET else "ticket") and (DET or plan["split"] >= 4), (tag, plan)
        K.linear_fwd(X.v, W.v, bias=b.to(dev), act="relu", out=O.v)
        at_rest(tag, K._SPLITK_WS[dev])
        assert X.unchanged() and W.unchanged() and O.intact(), tag
        r64, _, _ = gemm_reference(x, w, bias=b, act="relu")
        check_exact(tag, f"mfma_gemm<{plan['tile']}> {plan['route']}", "bf16", O.host(), r64.to(bf))
        # dgrad: dy [M, Kd] . w2 [Kd, N]: the reduction is the layer's width Kd
        w2 = torch.randint(-8, 9, (Kd, N), generator=g).to(bf)
        yp = torch.randint(-8, 9, (M, N), generator=g).to(bf)
        W2, YP, DX = Fr(Kd, N, bf, w2), Fr(M, N, bf, yp), Fr(M, N, bf, float("nan"))
        cs = torch.zeros(N, device=dev)
        plan = K.gemm_path(X.v, Kd, W2.v, N, M, N, Kd, EPI["dact"], ws=K._splitk_ws(M, N, Kd, dev))
        tag = f"linear_dgrad 32x128x{Kd} twin {plan['route']}"
        assert plan["route"] == ("direct" if DET else "ticket"), (tag, plan)
        K.linear_dgrad(X.v, W2.v, yprev=YP.v, act_prev="relu", out=DX.v, colsum=cs)
        at_rest(tag, K._SPLITK_WS[dev])
        assert X.unchanged() and W2.unchanged() and YP.unchanged() and DX.intact(), tag
        r64, c64, _ = gemm_reference(x, w2, True, False, "dact", act="relu", aux=yp)
        check_exact(tag, f"mfma_gemm<{plan['tile']}> {plan['route']}", "dact", DX.host(), r64.to(bf))
        check_exact(tag, f"mfma_gemm<{plan['tile']}> {plan['route']}", "colsum", cs.cpu(), c64.float())


def test_ticket_graph_replay(monkeypatch):
    """One ticket GEMM captured in a graph and replayed twice: identical bits to the eager result, at rest after."""
    _clean(monkeypatch)
    if DET:
        pytest.skip("no split-K in deterministic mode")
    s = TICKET[1]
    M, N, Kd = s["M"], s["N"], s["K"]
    sp = Spec("splitk graph", M, N, Kd, epi="f32", bias=True, act="relu", ws="own", route="ticket")
    o = sp.ops("twin")
    A, B, BIAS = Fr(M, Kd, bf, o["a"]), Fr(N, Kd, bf, o["b"]), Fr(1, N, f32, o["bias"].view(1, N))
    O, ws = Fr(M, N, f32, float("nan")), Fr(1, M * N, f32, 0.0)
    launch = lambda: K.gemm_raw(A.v, Kd, True, B.v, Kd, True, M, N, Kd, EPI["f32"], O.v, N, bias=BIAS.v, act="relu",  # noqa: E731
                                ws=ws.v.view(-1))
    assert K.gemm_path(A.v, Kd, B.v, Kd, M, N, Kd, EPI["f32"], ws=ws.v.view(-1))["route"] == "ticket"
    launch()
    at_rest("graph eager", ws)
    eager = O.host()
    check_exact("splitk graph twin ticket", "mfma_gemm<32> ticket", "f32", eager, o["ref64"][0].float())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for rep in range(2):
        O.refill()
        graph.replay()
        at_rest(f"graph replay {rep}", ws)
        check_exact(f"splitk graph replay {rep}", "mfma_gemm<32> ticket", "f32", O.host(), eager, rule="graph = eager")
        assert O.intact()


# -------------------------------------------------------------------------------------------------- finish route
def test_finish_route(monkeypatch):
    """memset + atomic split-K GEMM + splitk_finish_k, reached through the raw extension with tickets = 0: the same
    cases as the ticket route, equal bits on the twins, the workspace zero at rest afterwards."""
    _clean(monkeypatch)
    for spt, spf in zip(ticket_specs("ticket"), ticket_specs("finish", tickets=False)):
        f = both(spf)
        t = run_gemm(spt, "twin")
        assert bits_equal(f["twin"]["out"], t["out"]) and bits_equal(f["twin"]["cs"], t["cs"]), spf.name
        _rec("cross-route", "finish = ticket", "bit-identical")


# ------------------------------------------------------------------------------------------- atomic split (wgrad)
WGRAD = ((513, 20, 10), (2048, 77, 10), (513, 20, 70))  # (batch = the reduction, N = dY columns, K = x columns)


@pytest.mark.parametrize("Mb,N,Kx", WGRAD)
def test_atomic_split_wgrad(monkeypatch, Mb, N, Kx):
    """dW [N, Kx] += (dY * act'(y))^T x over a split batch, dbias from the tn == 0 tiles only (Kx = 70: three column
    tiles), a dY column that is all zero (the ``s != 0`` skip), a second call accumulates."""
    _clean(monkeypatch)
    sp = Spec(f"wgrad {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic", rowsum=True, mask="relu",
              zero_col=True, route="atomic", split_min=2)
    r = both(sp)
    if Kx == 70:
        assert r["twin"]["plan"]["grid"] == 3 and r["twin"]["plan"]["tile"] == 32
    both(sp, calls=2)
    # through the launcher, sigmoid mask (y from {0, 0.5, 1} in the twin)
    for kind in ("twin", "rand"):
        sm = Spec(f"wgrad launcher {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic", rowsum=True,
                  mask="sigmoid", route="atomic")
        o = sm.ops(kind)
        DY, X, Y = Fr(Mb, N, bf, o["a"]), Fr(Mb, Kx, bf, o["b"]), Fr(Mb, N, bf, o["y"])
        DW, DB = Fr(N, Kx, f32, o["old"]), Fr(1, N, f32, o["rs_old"].view(1, N))
        K.linear_wgrad(DY.v, X.v, DW.v, y=Y.v, act="sigmoid", dbias=DB.v.view(-1))
        torch.cuda.synchronize()
        assert DY.unchanged() and X.unchanged() and Y.unchanged() and DW.intact() and DB.intact()
        tag = f"{sm.name} {kind} atomic"
        if kind == "twin":
            check_exact(tag, "linear_wgrad", "atomic", DW.host(), o["ref64"][0].float())
            check_exact(tag, "linear_wgrad", "rowsum", DB.host().view(-1), (o["rs_old"].double() + o["ref64"][2]).float())
        else:
            check_yard(tag, "linear_wgrad", "atomic", DW.host(), o["ref64"][0], o["ref32"][0], o["mag_el"], Mb)
            check_yard(tag, "linear_wgrad", "rowsum", DB.host().view(-1), o["rs_old"].double() + o["ref64"][2],
                       o["rs_old"] + o["ref32"][2], o["rs_old"].double().abs() + o["mag_rs"], Mb)


# ----------------------------------------------------------------------------------------------------- degenerate
def test_degenerate(monkeypatch):
    _clean(monkeypatch)
    # K = 0: act(bias), from operands with no element (null pointers)
    for epi, act in (("bf16", "tanh"), ("f32", "relu")):
        N, M = 5, 7
        b = torch.tensor([-2.0, -0.5, 0.0, 0.5, 3.0])
        BIAS, O = Fr(1, N, f32, b.view(1, N)), Fr(M, N, f32 if epi == "f32" else bf, float("nan"))
        v = EXT().gemm_path(0, 0, 0, 0, M, N, 0, EPI[epi], 0, 0, 0, 0)
        assert K.GEMM_ROUTES[v[0]] == "direct" and v[2] == 1 and v[4] == 1, v
        rc = EXT().gemm(0, 0, 1, 0, 0, 1, M, N, 0, EPI[epi], ptr(O.v), N, ptr(BIAS.v), 1.0, 0.0, K.act_id(act), 0, 0, 0,
                        0, 0, 0, 0, 0, 0, stream())
        torch.cuda.synchronize()
        assert rc == 0 and O.intact() and BIAS.unchanged()
        ref = gemm_reference(torch.zeros(M, 0), torch.zeros(N, 0), bias=b, act=act)[0]
        if act == "relu":
            check_exact(f"K=0 {epi}", "mfma_gemm<32> direct", epi, O.host(), ref.float())
        else:
            check_yard(f"K=0 {epi}", "mfma_gemm<32> direct", epi, O.host(), ref, ref.float(), ref.abs() + 1.0, 1,
                       bf16_out=True)
    both(Spec("1x1x1", 1, 1, 1, epi="f32", bias=True, route="direct", tile=32))
    both(Spec("1x1x70", 1, 1, 70, a_kc=False, b_kc=False, epi="atomic", rowsum=True, route="atomic"))
    # M = 0 or N = 0: nothing is written, with and without a workspace (the planner is never asked)
    for M, N in ((0, 5), (5, 0)):
        O, ws = Fr(1, 8, f32, float("nan")), Fr(1, 64, f32, 0.0)
        A = Fr(8, 8, bf, torch.ones(8, 8))
        for w in (None, ws.v.view(-1)):
            plan = K.gemm_path(A.v, 8, A.v, 8, M, N, 2048, EPI["f32"], ws=w)
            assert plan["route"] == "direct" and plan["grid"] == 0, plan
            K.gemm_raw(A.v, 8, True, A.v, 8, True, M, N, 2048, EPI["f32"], O.v, 8, ws=w)
        at_rest(f"{M}x{N}", ws)
        assert O.unchanged() and A.unchanged()


# ------------------------------------------------------------------------------------------------ linear_bwd_pair
def pair_case(name, M, N, Kd, kind, y_act=None, dbias=True, dw_store=False, pool=None, want=None, env_tag=""):
    """pool = (KH, KW, H, W, C, premask, p).  Returns the host outputs."""
    g = _gen(f"{name} {kind}")
    twin = kind == "twin"
    rt = lambda *s: (torch.randint(-8, 9, s, generator=g).float() if twin else torch.randn(*s, generator=g)).to(bf)  # noqa: E731
    dy, w, x = rt(M, N), rt(N, Kd), rt(M, Kd)
    y = None
    if y_act == "relu":
        y = rt(M, N)
    elif y_act:
        y = ((torch.randint(0, 3, (M, N), generator=g).float() / 2) if twin else torch.rand(M, N, generator=g)).to(bf)
    old_w = torch.zeros(N, Kd) if dw_store else (torch.randint(-100, 101, (N, Kd), generator=g).float()
                                                 if twin else torch.randn(N, Kd, generator=g) * 3)
    old_b = torch.randint(-100, 101, (N,), generator=g).float() if twin else torch.randn(N, generator=g) * 3
    DY, W, X = Fr(M, N, bf, dy), Fr(N, Kd, bf, w), Fr(M, Kd, bf, x)
    Y = Fr(M, N, bf, y) if y is not None else None
    DW, DB = Fr(N, Kd, f32, old_w), (Fr(1, N, f32, old_b.view(1, N)) if dbias else None)
    pk = rp = None
    if pool is not None:
        KH, KW, H, Wd, C, premask, p = pool
        PH, PW = H // KH, Wd // KW
        assert C * PH * PW == Kd
        am = torch.randint(0, KH * KW, (M, PH, PW, C), generator=g).to(torch.uint8)
        am[0, 0, 0, 0] = 0xFF  # (a fused conv-pool's "ReLU' == 0": matches no tap)
        rng = torch.tensor([0x1234567, 3], dtype=torch.int64)
        amd, rngd = am.to(dev), rng.to(dev)
        pk = (amd, premask, (M, H, Wd, C), (KH, KW), "relu", rngd, 5, p)
        rp = (am, premask, (M, H, Wd, C), (KH, KW), "relu", rng, 5, p)
    plan = K.linear_bwd_pair_path(M, N, Kd, pool=pk, dw_store=dw_store)
    tag = f"{name}{env_tag} {kind} {plan['route']}/{plan['bma']}+{plan['bmb']}x{plan['gyB']} {plan['dw']} {plan['epilogue']}"
    print(f"GEMMPLAN {tag} {plan}")
    for k_, v_ in (want or {}).items():
        assert plan[k_] == v_, (tag, k_, plan)
    if plan["route"] == "pair":
        assert plan["epilogue"] == ("pool" if pool else "dact") and plan["gyA"] == 1 and (plan["gyB"] == 1 or not DET)
    poison = torch.full((M * (Kd if pool is None else pool[2] * pool[3] * pool[4]),), float("nan"), dtype=bf, device=dev)
    del poison  # (the launcher allocates dx itself: the caching allocator hands this block back, NaN-filled)
    dx = K.linear_bwd_pair(DY.v, W.v, X.v, DW.v, y=_v(Y), act=y_act or 0, dbias=None if DB is None else DB.v.view(-1),
                           pool=pk, dw_store=dw_store)
    torch.cuda.synchronize()
    assert (dx is False) == (plan["route"] == "separate"), tag
    for fr in (DY, W, X, Y):
        assert fr is None or fr.unchanged(), (tag, "an input changed")
    if dx is False:
        assert DW.unchanged() and (DB is None or DB.unchanged()), (tag, "a refused launch wrote")
        return dict(plan=plan)
    assert DW.intact() and (DB is None or DB.intact()), tag
    if pool is not None:
        assert torch.equal(amd.cpu(), am) and torch.equal(rngd.cpu(), rng), (tag, "pool inputs changed")
    kern = f"linear_bwd_pair_k<{plan['bma']},{plan['bmb']}> {plan['dw']} {plan['epilogue']}"
    refs = [linear_bwd_reference(dy, w, x, y=y, act=y_act, pool=rp, dtype=dt) for dt in ((f64,) if twin else (f64, f32))]
    r64, r32 = refs[0], refs[-1]
    dxh, dwh = dx.cpu(), DW.host()
    got = dict(plan=plan, dx=dxh, dw=dwh)
    eye = torch.eye(N).to(bf)
    gabs = gemm_reference(dy, eye, True, True, "atomic", a_mask_y=y, a_mask_act=y_act)[0].abs()
    if twin:
        if pool is not None and pool[6] > 0:  # 1 / (1 - p) is no power of two: the fp32 product, then bf16
            check_yard(tag, kern, "dx", dxh, r64[0], r64[0].float(), r64[0].abs(), 1, bf16_out=True)
        else:
            check_exact(tag, kern, "dx", dxh, r64[0].to(bf))
        check_exact(tag, kern, "dw", dwh, (old_w.double() + r64[1]).float())
        if DB is not None:
            got["db"] = DB.host().view(-1)
            check_exact(tag, kern, "dbias", got["db"], (old_b.double() + r64[2]).float())
    else:
        magx = gabs @ w.double().abs()
        if pool is not None:  # the element bound of the scattered value: the reference's own |.| path
            magx = linear_bwd_reference(gabs.to(f64), w.double().abs(), x, pool=rp)[0].abs() + 0.0
            check_yard(tag, kern, "dx", dxh, r64[0], r32[0], magx, N, bf16_out=True)
        else:
            check_yard(tag, kern, "dx", dxh, r64[0], r32[0], magx, N, bf16_out=True)
        check_yard(tag, kern, "dw", dwh, old_w.double() + r64[1], old_w + r32[1],
                   old_w.double().abs() + gabs.t() @ x.double().abs(), M)
        if DB is not None:
            check_yard(tag, kern, "dbias", DB.host().view(-1), old_b.double() + r64[2], old_b + r32[2],
                       old_b.double().abs() + gabs.sum(0), M)
    if pool is not None:  # rows / columns no window covers
        KH, KW, H, Wd, C, _, _ = pool
        assert not bool(_bits(dxh[:, (H // KH) * KH:]).any()) and not bool(_bits(dxh[:, :, (Wd // KW) * KW:]).any()), tag
    return got


PAIR = ((33, 10, 20), (64, 10, 500), (300, 50, 77))


@pytest.mark.parametrize("M,N,Kd", PAIR)
def test_linear_bwd_pair(monkeypatch, M, N, Kd):
    _clean(monkeypatch)
    split = M > 256 and not DET  # the wgrad part splits the batch above 4 k-tiles
    for kind in ("twin", "rand"):
        pair_case(f"pair {M}x{N}x{Kd}", M, N, Kd, kind, y_act="relu",
                  want=dict(route="pair", bma=32, bmb=32, dw="atomic"))
        pair_case(f"pair sig {M}x{N}x{Kd}", M, N, Kd, kind, y_act="sigmoid", dbias=False, want=dict(route="pair"))
        a = pair_case(f"pair store {M}x{N}x{Kd}", M, N, Kd, kind, dw_store=True,
                      want=dict(route="pair", dw="atomic" if split else "store"))
        assert (a["plan"]["gyB"] > 1) == split


def test_linear_bwd_pair_separate(monkeypatch):
    """A dgrad that wants split-K (M 32, reduction N 1024) keeps its own launch: False, nothing written."""
    _clean(monkeypatch)
    if DET:
        pytest.skip("no split-K in deterministic mode")
    r = pair_case("pair separate", 32, 1024, 128, "twin", want=dict(route="separate"))
    assert set(r) == {"plan"}


POOLS = {  # name: (M, N, (KH, KW, H, W, C, premask, p))
    "2x2": (33, 10, (2, 2, 5, 4, 5, True, 0.0)),        # H = PH KH + 1: a floor remainder row; K = 5 * 2 * 2 = 20
    "3x2": (33, 10, (3, 2, 7, 5, 3, False, 0.0)),       # remainder row and column; K = 3 * 2 * 2 = 12
    "2x2 drop": (64, 10, (2, 2, 4, 5, 25, True, 0.25)),  # K = 25 * 2 * 2 = 100, the host-stated keep mask
    "3x2 drop": (33, 10, (3, 2, 6, 4, 3, False, 0.25)),
}


@pytest.mark.parametrize("name", list(POOLS))
def test_linear_bwd_pair_pool(monkeypatch, name):
    _clean(monkeypatch)
    M, N, pool = POOLS[name]
    Kd = pool[4] * (pool[2] // pool[0]) * (pool[3] // pool[1])
    for kind in ("twin", "rand"):
        pair_case(f"pool {name}", M, N, Kd, kind, y_act="relu", pool=pool, want=dict(route="pair", epilogue="pool"))


def test_linear_bwd_pair_pool_refusals(monkeypatch):
    _clean(monkeypatch)
    M, N, Kd = 8, 10, 20
    # the launcher's own vector {C, PH, PW, KH, KW, act, H, W}: H = 6 with PH = 2, KH = 2 is no floor window of H
    for pl, code in (([5, 2, 2, 2, 2, 0, 6, 4], -3), ([5, 2, 2, 2, 2, 0, 3, 4], -3), ([5, 2, 2, 2, 2, 0, 5, 6], -3),
                     ([4, 2, 2, 2, 2, 0, 5, 4], -2)):
        v = EXT().linear_bwd_pair_path(M, N, Kd, pl, 0)
        assert v[0] == code and K.PAIR_ROUTES[code] == ("refuse" if code == -3 else "separate"), (pl, v)
        D = [Fr(M, N, bf, torch.ones(M, N)), Fr(N, Kd, bf, torch.ones(N, Kd)), Fr(M, Kd, bf, torch.ones(M, Kd))]
        DX, DW = Fr(M, pl[6] * pl[7] * pl[0], bf, float("nan")), Fr(N, Kd, f32, float("nan"))
        am = torch.zeros(M * Kd, dtype=torch.uint8, device=dev)
        rc = EXT().linear_bwd_pair(ptr(D[0].v), ptr(D[1].v), ptr(D[2].v), ptr(DX.v), 0, 0, 0, 0, 0, ptr(DW.v), 0, M, N,
                                   Kd, pl, ptr(am), 0, 0, 0, 0.0, 0, stream())
        torch.cuda.synchronize()
        assert rc == code and DX.unchanged() and DW.unchanged(), (pl, rc)
        if code == -3:
            with pytest.raises(RuntimeError, match="linear_bwd_pair"):
                from hops_examples_amd.ops._C import check
                check(rc, "linear_bwd_pair")


# ---------------------------------------------------------------------------------------------------------- knobs
def test_disable_knobs(monkeypatch):
    """HOPSX_DISABLE is read per call and matches whole tokens: splitk -> direct, splitk_ticket -> finish (not
    direct: 'splitk' is a substring of it), a longer token leaves both alone; bwd_pair -> separate (bwd_pair_gemm
    does not), dw_store -> atomic.  Twin bits are the same on every route."""
    if DET:
        pytest.skip("no split-K in deterministic mode")
    sp = {r: ticket_specs(r)[0] for r in ("ticket", "direct", "finish")}
    outs = {}
    for env, route in (("", "ticket"), ("splitk", "direct"), ("splitk_ticket", "finish"), ("conv_splitk", "ticket"),
                       ("pool8,splitk_ticket", "finish"), ("splitk_ticket,splitk", "direct")):
        monkeypatch.setenv("HOPSX_DISABLE", env)
        outs[env] = run_gemm(sp[route], "twin", env_tag=f" [{env}]")
        if route != "ticket":
            run_gemm(sp[route], "rand", env_tag=f" [{env}]")
    for env, o in outs.items():
        assert bits_equal(o["out"], outs[""]["out"]) and bits_equal(o["cs"], outs[""]["cs"]), env
        _rec("cross-route", "HOPSX_DISABLE", "bit-identical")
    M, N, Kd = PAIR[0]
    res = {}
    for env, want in (("", dict(route="pair", dw="store")), ("bwd_pair", dict(route="separate")),
                      ("bwd_pair_gemm", dict(route="pair", dw="store")), ("dw_store", dict(route="pair", dw="atomic"))):
        monkeypatch.setenv("HOPSX_DISABLE", env)
        res[env] = pair_case("pair knobs", M, N, Kd, "twin", dw_store=True, want=want, env_tag=f" [{env}]")
    for env in ("bwd_pair_gemm", "dw_store"):
        assert all(bits_equal(res[env][k], res[""][k]) for k in ("dx", "dw", "db")), env
        _rec("cross-route", "HOPSX_DISABLE", "bit-identical")


# ------------------------------------------------------------------------------------------------ child processes
def tile_specs(tile_a, tile_b):
    """(130, 129, 70) and (65, 49, 70) over the epilogues; the expected tiles come from the child's knobs."""
    out = []
    for (M, N, Kd), tile in (((130, 129, 70), tile_a), ((65, 49, 70), tile_b)):
        out += [Spec(f"tiles fwd {M}x{N}", M, N, Kd, epi="bf16", bias=True, act="relu", colsum=True, tile=tile),
                Spec(f"tiles f32 {M}x{N}", M, N, Kd, epi="f32", alpha=0.5, beta=2.0, bias=True, act="tanh", ldo_pad=3,
                     tile=tile),
                Spec(f"tiles dgrad {M}x{N}", M, N, Kd, b_kc=False, epi="dact", act="relu", mask="relu", colsum=True,
                     a_pad=1, tile=tile),
                Spec(f"tiles wgrad {M}x{N}", M, N, Kd, a_kc=False, b_kc=False, epi="atomic", rowsum=True, mask="relu",
                     tile=tile),
                Spec(f"tiles kc-rc {M}x{N}", M, N, Kd, a_kc=False, b_kc=True, epi="f32", rowsum=True, tile=tile)]
    return out


# (M, N, K): bma comes from the dgrad plan of [M x K], bmb from the wgrad plan of [N x K]; with the children's knobs
# these ten shapes reach all nine linear_bwd_pair_k<bma, bmb> instantiations (default knobs: <32,32> for every one)
PAIR_CHILD = ((130, 129, 70), (65, 49, 70), (300, 50, 77), (130, 129, 140), (130, 100, 140), (33, 65, 70), (65, 33, 70),
              (33, 130, 140), (65, 130, 140), (130, 33, 140))


def _run_tiles(tile_a, tile_b, pair_tiles):
    outs = {}
    for sp in tile_specs(tile_a, tile_b):
        r = both(sp)
        outs[sp.name] = {k: v for k, v in r["twin"].items() if k != "plan"}
    for (M, N, Kd), (bma, bmb) in zip(PAIR_CHILD, pair_tiles):
        for kind in ("twin", "rand"):
            want = dict(route="pair") if bma is None else dict(route="pair", bma=bma, bmb=bmb)
            r = pair_case(f"tiles pair {M}x{N}x{Kd}", M, N, Kd, kind, y_act="relu", want=want)
            if kind == "twin":
                outs[f"pair {M}x{N}x{Kd}"] = {k: v for k, v in r.items() if k != "plan"}
    return outs


def child_default():
    return _run_tiles(32, 32, ((32, 32),) * 10)


def child_t64():
    """HOPSX_GEMM_T64_MIN=0: every shape with M, N >= 48 takes the 64 x 64 tile (the pair's dgrad [M x K] and wgrad
    [N x K] parts by their own shapes: the pair kernels <64,64>, <32,64> and <64,32>)."""
    return _run_tiles(64, 64, ((64, 64),) * 5 + ((32, 64), (64, 32), (32, 64), (64, 64), (64, 32)))


def child_t128():
    """HOPSX_GEMM_T64_MIN=0 HOPSX_GEMM_T128_MIN=0: 128 x 128 where M, N >= 128, 64 x 64 below; the pair kernels
    <128,128>, <128,64>, <128,32>, <32,128> and <64,128> (and <64,64>, <32,64>, <64,32> again)."""
    return _run_tiles(128, 64, ((64, 64), (64, 64), (64, 64), (128, 128), (128, 64), (32, 64), (64, 32), (32, 128), (64, 128),
                                 (128, 32)))


def split_cfg_spec(tile):
    """An atomic wgrad with M, N >= 128 and a reduction of 8200 >= 8192: the one plan HOPSX_GEMM_SPLIT_CFG changes
    (64 x 64 by default, 128 x 128 with the knob at 0).  |v| <= 8: every partial sum stays below 64 x 8200 < 2^24."""
    return Spec("wgrad split_cfg 130x129x8200", 130, 129, 8200, a_kc=False, b_kc=False, epi="atomic", rowsum=True,
                mask="relu", route="atomic", tile=tile, split_min=8)


def child_split():
    """HOPSX_GEMM_SPLIT_TARGET=8 HOPSX_SPLIT_MINKT=1 HOPSX_GEMM_SPLIT_CFG=0: more, shorter K slices on the ticket and
    the atomic routes (one BK tile per slice at K = 769: 13 slices); the 128 x 128 tile of a big-K split GEMM."""
    outs = {}
    for sp in ticket_specs("ticket"):
        r = both(sp)
        outs[sp.name] = {k: v for k, v in r["twin"].items() if k != "plan"}
        assert r["twin"]["plan"]["kps"] == 64, r["twin"]["plan"]
    for Mb, N, Kx in WGRAD:
        sp = Spec(f"wgrad {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic", rowsum=True, mask="relu",
                  zero_col=True, route="atomic", split_min=8)
        r = both(sp)
        outs[sp.name] = {k: v for k, v in r["twin"].items() if k != "plan"}
    sp = split_cfg_spec(128)
    outs[sp.name] = {k: v for k, v in both(sp)["twin"].items() if k != "plan"}
    return outs


def child_det():
    """HOPSX_DETERMINISTIC=1: the reporter says split 1 everywhere (run_gemm asserts it) and ``det`` where a split
    was taken away; two runs of a colsum case agree bit for bit."""
    outs = {}
    for sp in ticket_specs(None) + [Spec(f"wgrad {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic",
                                         rowsum=True, mask="relu", zero_col=True) for Mb, N, Kx in WGRAD]:
        r = both(sp)
        assert r["twin"]["plan"]["det"], (sp.name, r["twin"]["plan"])
        outs[sp.name] = {k: v for k, v in r["twin"].items() if k != "plan"}
    sp = Spec("det colsum", 300, 50, 77, epi="bf16", bias=True, act="tanh", colsum=True, route="direct")
    assert not run_gemm(sp, "rand")["plan"]["det"]
    a, b = run_gemm(sp, "rand"), run_gemm(sp, "rand")
    assert bits_equal(a["out"], b["out"]) and bits_equal(a["cs"], b["cs"])
    _rec("deterministic mode", "out, colsum", "two launches bit-identical")
    for kind in ("twin", "rand"):
        pair_case("det pair", 300, 50, 77, kind, y_act="relu", dw_store=True, want=dict(route="pair", dw="store"))
    return outs


CHILDREN = {
    "t64": (child_t64, dict(HOPSX_GEMM_T64_MIN="0")),
    "t128": (child_t128, dict(HOPSX_GEMM_T64_MIN="0", HOPSX_GEMM_T128_MIN="0")),
    "split": (child_split, dict(HOPSX_GEMM_SPLIT_TARGET="8", HOPSX_SPLIT_MINKT="1", HOPSX_GEMM_SPLIT_CFG="0")),
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
    code = "import sys, test_gemm_paths_gpu as T\nT.child_main(sys.argv[1], sys.argv[2])"
    try:
        r = subprocess.run([sys.executable, "-c", code, mode, str(out)], env=env, timeout=timeout, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on that card
        pytest.exit(f"GEMM child '{mode}' did not end within {timeout} s, stopping the session: {e}", returncode=3)
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):  # killed by a signal / abort / segmentation fault
        pytest.exit(f"GEMM child '{mode}' died with {r.returncode}, stopping the session:\n{r.stderr[-3000:]}",
                    returncode=3)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = torch.load(out, weights_only=False)
    for k, (n, w) in got["stats"].items():
        e = STATS.setdefault(k, [0, 0.0])  # the child's checks count in the same rows as the parent's
        e[0], e[1] = e[0] + n, max(e[1], w)
    return got["outs"]


def _same_as(outs, mine, what):
    assert set(outs) == set(mine), (set(outs) ^ set(mine))
    for name, o in outs.items():
        for k, v in o.items():
            assert bits_equal(v, mine[name][k]), (what, name, k)
            _rec("cross-route", what, "bit-identical")


@pytest.mark.parametrize("mode", ["t64", "t128"])
def test_tile_knob_children(monkeypatch, tmp_path, mode):
    """The 64 x 64 and 128 x 128 tiles of every epilogue, layout and pair kernel: the child's twins equal this
    process's 32 x 32 bits."""
    _clean(monkeypatch)
    if DET:
        pytest.skip("default-knob parent")
    _same_as(run_child(mode, tmp_path), child_default(), f"tile knobs {mode}")


def test_split_knob_child(monkeypatch, tmp_path):
    _clean(monkeypatch)
    if DET:
        pytest.skip("default-knob parent")
    outs = run_child("split", tmp_path)
    mine = {}
    for sp in ticket_specs("ticket"):
        mine[sp.name] = {k: v for k, v in run_gemm(sp, "twin").items() if k != "plan"}
    for Mb, N, Kx in WGRAD:
        sp = Spec(f"wgrad {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic", rowsum=True, mask="relu",
                  zero_col=True, route="atomic")
        mine[sp.name] = {k: v for k, v in run_gemm(sp, "twin").items() if k != "plan"}
    sp = split_cfg_spec(64)
    mine[sp.name] = {k: v for k, v in both(sp)["twin"].items() if k != "plan"}
    _same_as(outs, mine, "split knobs")


def test_deterministic_mode_child(monkeypatch, tmp_path):
    _clean(monkeypatch)
    if DET:
        pytest.skip("default-knob parent")
    outs = run_child("det", tmp_path)
    mine = {}
    for sp in ticket_specs("ticket") + [Spec(f"wgrad {Mb}x{N}x{Kx}", N, Kx, Mb, a_kc=False, b_kc=False, epi="atomic",
                                             rowsum=True, mask="relu", zero_col=True) for Mb, N, Kx in WGRAD]:
        mine[sp.name] = {k: v for k, v in run_gemm(sp, "twin").items() if k != "plan"}
    _same_as(outs, mine, "deterministic mode")


def test_zz_measured_table():
    """Prints what this process and its children measured, in the layout of the module docstring's table (run the
    whole file with -s): kernel, output, rule, checks, worst ratio."""
    print()
    for (kern, out, rule), (n, w) in sorted(STATS.items()):
        worst = f"{w:.3f}" if "yard" in rule else "no mismatch"
        print(f"GEMMTABLE   {kern:44s} {out:16s} {rule:28s} {n:5d}  {worst}")
