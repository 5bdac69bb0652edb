"""topk.hip (row softmax + top-k of logits) against the fp64 reference on both launcher routes.

Every check is made on the route ``softmax_topk_path`` reports (0 a wave per row, 1 a workgroup per row), and the shape
list must reach both.

ids: EXACTLY ``softmax_topk_reference``'s, ties included, for every case — the selection is integer work on the logits'
bits, so there is nothing to tolerate.

scores: the project's yardstick rule (test_bn_paths_gpu.py).  Per input family and dtype, over all shapes: YARD = the
largest relative error of the fp32 reference (``softmax_topk_reference(dtype=float32)``: an fp32 softmax of the same
logits) against the fp64 one; the kernel is allowed MARGIN = 8 times that, plus a floor of one fp32 ulp of the score:
``|score - ref64| <= 8 YARD ref64 + ulp32(ref64)``.  A -inf class has ref64 = 0 and must score 0 (to one subnormal).
Each test prints ``topk-err`` lines (family, dtype, YARD, the kernel's largest relative error, the worst error / bound)
before it asserts.

Families: Gaussian logits of standard deviation 1, 4, 16; integer-valued logits from 5 distinct values (ties everywhere,
exact in bf16); Gaussian rows with -inf entries.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 8.0
# (B, C, k): small, odd, tile-edge and batch-inference shapes, one shape on either side of the route threshold
# (C = 1024 | 1025), and C = 300 / 700 for the wave route's 2- and 4-pass fp32 kernels (C <= 256 is one pass, 1000 four)
SHAPES = [(1, 10, 1), (3, 8, 8), (5, 63, 3), (5, 64, 5), (5, 65, 8), (100, 1000, 3), (9, 4099, 8),
          (6, 1024, 3), (6, 1025, 3), (4, 300, 4), (4, 700, 2)]
FAMILIES = ["gauss1", "gauss4", "gauss16", "int5", "minf"]
DTYPES = [torch.float32, torch.bfloat16]


def _logits(family, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    if family.startswith("gauss"):
        return torch.randn(B, C, generator=g) * float(family[5:])
    if family == "int5":
        return torch.randint(-2, 3, (B, C), generator=g).float()
    z = torch.randn(B, C, generator=g) * 4.0
    drop = torch.rand(B, C, generator=g) < 0.4
    drop[:, int(torch.randint(0, C, (1,), generator=g))] = False  # at least one finite value per row
    return z.masked_fill(drop, float("-inf"))


@functools.lru_cache(maxsize=None)
def _case(family, dtype, shape):
    """(logits on the host in ``dtype``, ids, fp64 scores, fp32-yardstick scores), computed once and shared."""
    from hops_examples_amd.ops.functional import softmax_topk_reference

    B, C, k = shape
    z = _logits(family, B, C, seed=1000 * FAMILIES.index(family) + SHAPES.index(shape)).to(dtype)
    ids, s64 = softmax_topk_reference(z, k)
    ids32, s32 = softmax_topk_reference(z, k, dtype=torch.float32)
    assert torch.equal(ids, ids32)
    return z, ids, s64, s32


def _yard(family, dtype):
    worst = 0.0
    for shape in SHAPES:
        _, _, s64, s32 = _case(family, dtype, shape)
        nz = s64 > 0
        if nz.any():
            worst = max(worst, float(((s32.double() - s64).abs()[nz] / s64[nz]).max()))
    return worst


def _ulp32(s64):
    return torch.from_numpy(np.spacing(s64.numpy().astype(np.float32)).astype(np.float64))


def _run(z, k, **kw):
    from hops_examples_amd.ops import kernels as K

    ids, scores = K.softmax_topk(z.cuda(), k, **kw)
    torch.cuda.synchronize()
    return ids.cpu(), scores.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_ids_exact_and_scores_within_the_yardstick_on_both_routes(family, dtype):
    from hops_examples_amd.ops import kernels as K

    yard = _yard(family, dtype)
    routes, worst_rel, worst_ratio, bad = set(), 0.0, 0.0, []
    for shape in SHAPES:
        B, C, k = shape
        z, ids, s64, _ = _case(family, dtype, shape)
        zd = z.cuda()
        route = K.softmax_topk_path(zd, k)
        assert route == (0 if C <= 1024 else 1), (shape, route)
        routes.add(route)
        got_ids, got = K.softmax_topk(zd, k)
        got_ids, got = got_ids.cpu(), got.cpu()
        assert got_ids.dtype == torch.int32 and got.dtype == torch.float32 and got.shape == (B, k)
        assert torch.equal(got_ids, ids), (family, dtype, shape, "ids differ from the reference")
        err = (got.double() - s64).abs()
        bound = MARGIN * yard * s64 + _ulp32(s64)
        nz = s64 > 0
        if nz.any():
            worst_rel = max(worst_rel, float((err[nz] / s64[nz]).max()))
        worst_ratio = max(worst_ratio, float((err / bound).max()))
        if not bool((err <= bound).all()):
            bad.append((shape, route, float((err / bound).max())))
        if family == "minf":
            assert bool((got[s64 == 0] == 0).all()), (shape, "a -inf class must score 0")
    print(f"topk-err family={family} dtype={str(dtype)[6:]} yard_rel={yard:.3e} kernel_rel={worst_rel:.3e} "
          f"worst_err_over_bound={worst_ratio:.3f} (bound = {MARGIN:g} yard ref + ulp32)")
    assert routes == {0, 1}
    assert not bad, bad


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (3, 1001)), (torch.bfloat16, (3, 1003)),
                                         (torch.float32, (3, 4099)), (torch.bfloat16, (3, 4099))],
                         ids=["fp32-1001", "bf16-1003", "fp32-4099", "bf16-4099"])
def test_rows_off_16_byte_alignment(dtype, shape):
    """Rows 1.. of an odd-C tensor: the base is 4-byte (fp32) / 2-byte (bf16) aligned only, the kernels take their
    element loads; same ids as the reference, and the same BYTES as the rows copied to an aligned tensor."""
    from hops_examples_amd.ops import kernels as K
    from hops_examples_amd.ops.functional import softmax_topk_reference

    B, C = shape
    full = (_logits("gauss4", B, C, seed=77)).to(dtype).cuda()
    view = full[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    for k in (3, 8):
        assert K.softmax_topk_path(view, k) == (0 if C <= 1024 else 1)
        ids, scores = K.softmax_topk(view, k)
        aligned = view.clone()
        assert aligned.data_ptr() % 16 == 0
        ids_a, scores_a = K.softmax_topk(aligned, k)
        rid, r64 = softmax_topk_reference(view.cpu(), k)
        assert torch.equal(ids.cpu(), rid) and torch.equal(ids_a.cpu(), rid)
        assert torch.equal(scores.view(torch.int32), scores_a.view(torch.int32))
        _, r32 = softmax_topk_reference(view.cpu(), k, dtype=torch.float32)  # the yardstick on these very logits
        yard = float(((r32.double() - r64).abs() / r64).max())
        err = (scores.cpu().double() - r64).abs()
        print(f"topk-err misaligned {tuple(shape)} {str(dtype)[6:]} k={k} yard_rel={yard:.3e} "
              f"kernel_rel={float((err / r64).max()):.3e}")
        assert bool((err <= MARGIN * yard * r64 + _ulp32(r64)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1000, 4099], ids=["wave", "workgroup"])
def test_a_rows_bytes_do_not_depend_on_batch_position_or_grid(C, dtype):
    from hops_examples_amd.ops import kernels as K

    k = 5
    z = _logits("gauss4", 9, C, seed=5).to(dtype).cuda()
    z[2, :40] = z[2, 40:80]  # ties in one row
    assert K.softmax_topk_path(z, k) == (0 if C <= 1024 else 1)
    ids, scores = K.softmax_topk(z, k)
    base = (ids.cpu(), scores.cpu().view(torch.int32))
    for cap in (1, 2, 0):  # 9 rows: the grid-stride loop runs at 1 and 2 workgroups
        for _ in range(2):  # and two runs give equal bytes
            i2, s2 = K.softmax_topk(z, k, max_workgroups=cap)
            assert torch.equal(i2.cpu(), base[0]) and torch.equal(s2.cpu().view(torch.int32), base[1]), cap
    for r in (0, 4, 8):
        i1, s1 = K.softmax_topk(z[r:r + 1].clone(), k)  # alone
        assert torch.equal(i1.cpu()[0], base[0][r]) and torch.equal(s1.cpu().view(torch.int32)[0], base[1][r])
    big = torch.cat([z.flip(0), z, z[:3]])  # 21 rows: row r of z sits at 8 - r, 9 + r (and 18 + r)
    ib, sb = K.softmax_topk(big, k)
    ib, sb = ib.cpu(), sb.cpu().view(torch.int32)
    for r in range(9):
        for pos in (8 - r, 9 + r):
            assert torch.equal(ib[pos], base[0][r]) and torch.equal(sb[pos], base[1][r]), (r, pos)


def test_guards_refuse_before_any_launch():
    from hops_examples_amd.ops import _C
    from hops_examples_amd.ops import kernels as K

    z = torch.randn(4, 6, device="cuda")
    ids = torch.full((4, 3), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((4, 3), -7.0, device="cuda")
    for bad_k in (0, 9, 7):  # k = 7 > C = 6
        with pytest.raises(ValueError):
            K.softmax_topk(z, bad_k, ids, scores)
        with pytest.raises(ValueError):
            K.softmax_topk_path(z, bad_k)
    wide = torch.randn(4, 12, device="cuda")
    with pytest.raises(ValueError):
        K.softmax_topk(wide[:, ::2], 3, ids, scores)  # non-contiguous view
    with pytest.raises(ValueError):
        K.softmax_topk(z, 3, ids.long(), scores)  # int64 ids
    with pytest.raises(ValueError):
        K.softmax_topk(z, 3, ids, scores.double())
    with pytest.raises(ValueError):
        K.softmax_topk(z.cpu(), 3)  # a CPU tensor
    with pytest.raises(ValueError):
        K.softmax_topk(z.double(), 3, ids, scores)
    with pytest.raises(ValueError):
        K.softmax_topk(z, 3, ids[:2], scores)  # wrong shape
    # the launcher itself: hipErrorInvalidValue (1), nothing launched; the route query says -2
    ext, st = _C.ext(), _C.stream()
    for args in ((z.data_ptr(), 0, 4, 6, 0, ids.data_ptr(), scores.data_ptr()),
                 (z.data_ptr(), 0, 4, 6, 9, ids.data_ptr(), scores.data_ptr()),
                 (z.data_ptr(), 0, 4, 6, 7, ids.data_ptr(), scores.data_ptr()),
                 (z.data_ptr(), 0, -1, 6, 3, ids.data_ptr(), scores.data_ptr()),
                 (0, 0, 4, 6, 3, ids.data_ptr(), scores.data_ptr()),
                 (z.data_ptr(), 0, 4, 6, 3, 0, scores.data_ptr()),
                 (z.data_ptr(), 0, 4, 6, 3, ids.data_ptr(), 0)):
        assert ext.softmax_topk_path(*args) == -2
        assert ext.softmax_topk(*args, 0, st) == 1
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((scores == -7.0).all())  # untouched by every refusal above
    e_ids, e_scores = K.softmax_topk(torch.empty(0, 6, device="cuda"), 3)  # B = 0: empty outputs, no launch
    assert e_ids.shape == (0, 3) and e_ids.dtype == torch.int32 and e_scores.shape == (0, 3)
    assert K.softmax_topk_path(torch.empty(0, 6, device="cuda"), 3) == 0


@pytest.mark.parametrize("C", [1000, 1500], ids=["wave", "workgroup"])
def test_rows_out_of_contract_stay_in_bounds_and_do_not_touch_their_neighbours(C):
    from hops_examples_amd.ops import kernels as K

    B, k = 6, 8
    z = _logits("gauss4", B, C, seed=9).cuda()
    clean_ids, clean_scores = K.softmax_topk(z, k)
    dirty = z.clone()
    dirty[1, ::7] = float("nan")
    dirty[1, 3] = float("inf")
    dirty[4, 5] = float("inf")
    dirty[4, C - 1] = float("inf")
    ids_buf = torch.full((B * k + 64,), -7, dtype=torch.int32, device="cuda")
    sc_buf = torch.full((B * k + 64,), -7.0, device="cuda")
    ids, scores = ids_buf[:B * k].view(B, k), sc_buf[:B * k].view(B, k)
    K.softmax_topk(dirty, k, ids, scores)
    torch.cuda.synchronize()
    assert bool((ids_buf[B * k:] == -7).all()) and bool((sc_buf[B * k:] == -7.0).all())  # canaries
    for r in (1, 4):
        row = ids[r].cpu().tolist()
        assert len(set(row)) == k and all(0 <= i < C for i in row), (r, row)
    for r in (0, 2, 3, 5):
        assert torch.equal(ids[r], clean_ids[r])
        assert torch.equal(scores[r].view(torch.int32), clean_scores[r].view(torch.int32))


@pytest.mark.parametrize("C", [1000, 1500], ids=["wave", "workgroup"])
def test_launch_is_capturable_and_replays_on_new_logits(C):
    from hops_examples_amd.ops import kernels as K
    from hops_examples_amd.runtime.capture import graph as capture

    B, k = 7, 3
    buf = _logits("gauss4", B, C, seed=11).to(torch.bfloat16).cuda()
    ids = torch.empty(B, k, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, k, device="cuda")
    K.softmax_topk(buf, k, ids, scores)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(g):
        K.softmax_topk(buf, k, ids, scores)
    new = _logits("gauss16", B, C, seed=12).to(torch.bfloat16).cuda()
    buf.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    e_ids, e_scores = K.softmax_topk(new, k)
    assert torch.equal(ids, e_ids) and torch.equal(scores.view(torch.int32), e_scores.view(torch.int32))
