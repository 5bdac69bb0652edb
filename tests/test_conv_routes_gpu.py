"""The conv launchers' route queries (kernels.conv2d_fwd_path / conv2d_dgrad_path) against the routes the launchers
took before the route was a value, and every launcher on every route it can take against an fp64 reference computed
from the bf16 operands the kernels read.  Only the stored tensor is checked on the bnstats and dgrad_bn routes: the BN
sums they accumulate are zeroed or dropped here (tests/test_bnstats_gpu.py and tests/test_bn_dgrad_sums_gpu.py hold them).

Bound of every element-wise comparison (tests/test_frozen_resnet_gpu.py's): ``2^-8 |ref| + (1 + 2^-8) * 4 * e32``,
half a bf16 ulp of the stored value plus the project's factor 4 on e32 = max |fp32 proxy - fp64| of the same formula on
the test's own inputs.  An fp32 store has no bf16 rounding and is held to the same (then looser than needed) bound; a
column sum to the sum of its column's element bounds.

The pinned routes are those of the kernel trace of the commit before conv_fwd_route / conv_dgrad_route existed
(tools/conv_routes.py under rocprofv3, joined; profiles/r20_conv_routes.txt keeps the summary).  The trace line named
next to each case is the `CASE <group>:<geometry> | <launcher>` line of that join, default settings unless it says
``paroff`` (HOPSX_DISABLE=dgrad_par, the only way an aligned 1x1 strided dgrad reaches the scatter epilogue)."""
import pytest
import torch
import torch.nn.functional as F

from test_frozen_resnet_gpu import CASES as FROZEN, bound

BF16 = torch.bfloat16

# name: (B, H, C, CO, k, stride).  The smallest shape on each route (the thresholds, from conv.hip / gemm_glds.h):
#   frozen *  : tests/test_frozen_resnet_gpu.py CASES (its comments derive them)
#   direct    : K = 9 <= 64, K * CO = 288 <= 1024: the input-layer kernel
#   par       : 3x3 stride 2; the whole dgrad GEMM (M = 44 * 44 = 1,936 rows, N = C = 256) is 16 x 2 = 32 tiles of
#               128 x 128, the gg engine's floor (43 x 43 gives 30 and gemm_core.h's engine)
#   scatter   : 1x1 stride 2 with H = 2 OH; the scatter GEMM runs over the OH * OW = 1,936 output pixels: H = 88
#   dense     : 1x1 stride 1, C = 256 (no direct MFMA dgrad: C <= 128 there), 1,936 rows x 256 columns
#   gather    : the frozen gg_3x3_64_64 (K = 576 > 512: no direct MFMA dgrad; 3,969 rows = 32 tiles)
GEOMS = {n: (c[0], c[1], c[3], c[4], c[5], c[6]) for n, c in FROZEN.items()}
#   bn_gemm   : a BN-statistics forward on gemm_core.h's engine: CO = 64 has the vector BN path, K = 576 > 512 no
#               MFMA kernel, 25 rows neither the gg engine nor split-K
GEOMS.update(direct=(1, 6, 1, 32, 3, 1), par=(1, 44, 256, 16, 3, 2), scatter=(1, 88, 256, 64, 1, 2),
             dense=(1, 44, 256, 64, 1, 1), bn_gemm=(1, 5, 64, 64, 3, 1))

# (geometry, kind): route  # trace line of the parent's join
FWD = {
    ("mfma16", "store"): "mfma",            # frozen:1x5x5x16->16 k3 s1 p1 | fwd
    ("mfma32", "store"): "mfma",            # frozen:1x5x5x32->32 k3 s1 p1 | fwd
    ("mfma_1x1_256_64", "store"): "mfma",   # frozen:1x5x5x256->64 k1 s1 p0 | fwd
    ("gemm", "store"): "gemm",              # frozen:2x5x5x64->40 k1 s1 p0 | fwd
    ("gg_3x3_64_64", "store"): "gg",        # frozen:1x63x63x64->64 k3 s1 p1 | fwd
    ("gg_1x1_64_256", "store"): "gg",       # frozen:1x44x44x64->256 k1 s1 p0 | fwd
    ("splitk", "store"): "splitk",          # frozen:2x7x7x512->512 k3 s1 p1 | fwd
    ("direct", "store"): "direct",          # routes:1x6x6x1->32 k3 s1 p1 | fwd
    ("mfma16", "colsum"): "gemm",           # frozen:1x5x5x16->16 k3 s1 p1 | fwd_colsum
    ("direct", "colsum"): "gemm",           # routes:1x6x6x1->32 k3 s1 p1 | fwd_colsum
    ("gg_1x1_64_256", "colsum"): "gg",      # frozen:1x44x44x64->256 k1 s1 p0 | fwd_colsum
    ("splitk", "colsum"): "splitk",         # frozen:2x7x7x512->512 k3 s1 p1 | fwd_colsum
    ("mfma16", "f32"): "gemm",              # frozen:1x5x5x16->16 k3 s1 p1 | fwd_f32
    ("gg_1x1_64_256", "f32"): "gemm",       # frozen:1x44x44x64->256 k1 s1 p0 | fwd_f32
    ("splitk", "f32"): "gemm",              # frozen:2x7x7x512->512 k3 s1 p1 | fwd_f32
    ("mfma16", "bnstats"): "mfma",          # frozen:1x5x5x16->16 k3 s1 p1 | fwd_bnstats
    ("gemm", "bnstats"): -2,                # frozen:2x5x5x64->40 k1 s1 p0 | fwd_bnstats (CO = 40: no vector BN)
    ("gg_3x3_64_64", "bnstats"): "gg",      # frozen:1x63x63x64->64 k3 s1 p1 | fwd_bnstats
    ("splitk", "bnstats"): "splitk",        # frozen:2x7x7x512->512 k3 s1 p1 | fwd_bnstats
    ("mfma_1x1_256_64", "bnstats"): "mfma", # frozen:1x5x5x256->64 k1 s1 p0 | fwd_bnstats
    ("bn_gemm", "bnstats"): "gemm",         # routes:1x5x5x64->64 k3 s1 p1 | fwd_bnstats
    ("direct", "bnstats"): -2,              # routes:1x6x6x1->32 k3 s1 p1 | fwd_bnstats (C % 8 != 0 past the MFMA test)
}
FWD.update({(n, "res"): c[8] for n, c in FROZEN.items()})  # (test_frozen_resnet_gpu.py asserts these)

# (geometry, launcher form, environment): route  # trace line
DGRAD = {
    ("mfma16", "plain", ""): "mfma",                 # frozen:1x5x5x16->16 k3 s1 p1 | dgrad
    ("mfma16", "y", ""): "mfma",                     # frozen:1x5x5x16->16 k3 s1 p1 | dgrad_y
    ("mfma16", "addend", ""): "gemm",                # frozen:1x5x5x16->16 k3 s1 p1 | dgrad_addend
    ("par", "plain", ""): "gg_par",                  # routes:1x44x44x256->16 k3 s2 p1 | dgrad
    ("par", "addend", ""): "gg_par",                 # routes:1x44x44x256->16 k3 s2 p1 | dgrad_addend
    ("scatter", "plain", ""): "gg_par",              # routes:1x88x88x256->64 k1 s2 p0 | dgrad
    ("scatter", "plain", "dgrad_par"): "gg_scatter", # paroff routes:1x88x88x256->64 k1 s2 p0 | dgrad
    ("scatter", "addend", "dgrad_par"): "gg_scatter",  # paroff routes:1x88x88x256->64 k1 s2 p0 | dgrad_addend
    ("dense", "plain", ""): "gg_dense",              # routes:1x44x44x256->64 k1 s1 p0 | dgrad
    ("dense", "y", ""): "gemm",                      # routes:1x44x44x256->64 k1 s1 p0 | dgrad_y
    ("gg_3x3_64_64", "plain", ""): "gg_gather",      # frozen:1x63x63x64->64 k3 s1 p1 | dgrad
    ("splitk", "plain", ""): "splitk",               # frozen:2x7x7x512->512 k3 s1 p1 | dgrad
    ("splitk", "y", ""): "splitk",                   # frozen:2x7x7x512->512 k3 s1 p1 | dgrad_y
    ("mfma_1x1_256_64", "plain", ""): "gemm",        # frozen:1x5x5x256->64 k1 s1 p0 | dgrad
    ("dense", "addend", ""): "gg_dense",             # routes:1x44x44x256->64 k1 s1 p0 | dgrad_addend
    ("gg_3x3_64_64", "addend", ""): "gg_gather",     # frozen:1x63x63x64->64 k3 s1 p1 | dgrad_addend
    ("splitk", "addend", ""): "splitk",              # frozen:2x7x7x512->512 k3 s1 p1 | dgrad_addend
    ("scatter", "colsum", ""): "gg_par",             # routes:1x88x88x256->64 k1 s2 p0 | dgrad_colsum
    ("scatter", "colsum", "dgrad_par"): "gg_gather", # paroff routes:1x88x88x256->64 k1 s2 p0 | dgrad_colsum (no scatter)
    ("par", "bn", ""): -2,                           # routes:1x44x44x256->16 k3 s2 p1 | dgrad_bn (a stride)
    ("splitk", "bn", ""): -2,                        # frozen:2x7x7x512->512 k3 s1 p1 | dgrad_bn (would split K)
    ("mfma16", "bn", ""): "mfma",                    # frozen:1x5x5x16->16 k3 s1 p1 | dgrad_bn
    ("dense", "bn", ""): "gg_dense",                 # routes:1x44x44x256->64 k1 s1 p0 | dgrad_bn
    ("gg_3x3_64_64", "bn", ""): "gg_gather",         # frozen:1x63x63x64->64 k3 s1 p1 | dgrad_bn
    ("mfma_1x1_256_64", "bn", ""): "gemm",           # frozen:1x5x5x256->64 k1 s1 p0 | dgrad_bn
}

_CACHE = {}


def _conv(x, w, s, dtype):
    k = w.shape[1]
    return F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(0, 3, 1, 2), None, s, k // 2).permute(0, 2, 3, 1)


def operands(name):
    """CPU operands of a geometry and the unmasked references both passes share, computed once."""
    if name not in _CACHE:
        B, H, C, CO, k, s = GEOMS[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)) + 20)
        d = dict(x=torch.randn(B, H, H, C, generator=g).to(BF16),
                 w=(torch.randn(CO, k, k, C, generator=g) * (2.0 / (k * k * C)) ** 0.5).to(BF16),
                 bias=torch.randn(CO, generator=g) * 0.1)
        d["o64"], d["o32"] = _conv(d["x"], d["w"], s, torch.float64), _conv(d["x"], d["w"], s, torch.float32)
        d["res"] = (torch.randn(d["o64"].shape, generator=g) * 2 * d["o64"].std().item()).to(BF16)
        d["dy"] = torch.randn(d["o64"].shape, generator=g).to(BF16)
        d["y"] = torch.randn(d["o64"].shape, generator=g).to(BF16)   # this conv's output, for the act' mask on dY
        d["add"] = torch.randn(B, H, H, C, generator=g).to(BF16)
        _CACHE[name] = d
    return _CACHE[name]


def dgrad_ref(d, name, dy, dtype):
    """conv_transpose(dy, w) in ``dtype`` (the gradient of sum(conv(x, w) * dy) with respect to x)."""
    s = GEOMS[name][5]
    x = d["x"].to(dtype).requires_grad_(True)
    (_conv(x, d["w"], s, dtype) * dy.to(dtype)).sum().backward()
    return x.grad


def geom_of(name):
    from hops_examples_amd.ops import kernels as K

    B, H, C, CO, k, s = GEOMS[name]
    return K.conv_geom((B, H, H, C), (CO, k, k, C), (s, s), (k // 2, k // 2), (1, 1))


def held(got, ref64, ref32, what):
    e32 = (ref32.double() - ref64).abs().max().item()
    err, lim = (got.double().cpu() - ref64).abs(), bound(ref64, e32)
    print(f"{what}: e32 {e32:.3e} max err {err.max():.3e} worst err/bound {(err / lim).max():.3f}")
    assert bool((err <= lim).all()), (what, (err / lim).max())
    return lim


def test_every_route_a_kind_can_take_is_pinned():
    """Per launcher kind, not over their union: the routes conv_fwd_route / conv_dgrad_route leave that kind."""
    fwd = {kind: {r for (n, k), r in FWD.items() if k == kind} for kind in ("store", "colsum", "f32", "res", "bnstats")}
    assert fwd == {"store": {"direct", "mfma", "gg", "splitk", "gemm"}, "colsum": {"gg", "splitk", "gemm"},
                   "f32": {"gemm"}, "res": {"mfma", "gg", "splitk", "gemm"},
                   "bnstats": {-2, "mfma", "gg", "splitk", "gemm"}}
    dg = {form: {r for (n, f, env), r in DGRAD.items() if f == form} for form in ("plain", "y", "addend", "colsum", "bn")}
    gg = {"gg_par", "gg_scatter", "gg_dense", "gg_gather"}
    assert dg == {"plain": gg | {"mfma", "splitk", "gemm"}, "y": {"mfma", "splitk", "gemm"},
                  "addend": gg | {"splitk", "gemm"}, "colsum": {"gg_par", "gg_gather"},
                  "bn": {-2, "mfma", "gg_dense", "gg_gather", "gemm"}}


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", list(FWD))
def test_forward_route_and_result(name, kind):
    from hops_examples_amd.ops import kernels as K

    d, geom, route = operands(name), geom_of(name), FWD[name, kind]
    assert K.conv2d_fwd_path(geom, kind) == route
    if kind == "res":
        assert K.conv2d_fwd_res_path(geom) == route
    x, w, bias, res = (d[k].cuda() for k in ("x", "w", "bias", "res"))
    CO = geom[6]
    act = lambda t: t.clamp_min(0)
    if kind == "bnstats":
        got = K.conv2d_fwd_bnstats(x, w, geom)
        if got is not None:
            torch.cuda.synchronize()
            K.bn_acc(x.device, CO)[: K.BN_NREP * 2 * CO].zero_()  # (at rest again: no apply follows here)
        assert (got is None) == (route == -2)
        if got is not None:
            held(got, d["o64"], d["o32"], f"{name} bnstats {route}")
        return
    if kind == "res":
        got = K.conv2d_fwd_res(x, w, geom, bias=bias, act=1, residual=res)
        held(got, act(d["o64"] + bias.double().cpu() + d["res"].double()),
             act(d["o32"] + bias.cpu() + d["res"].float()), f"{name} res {route}")
        return
    colsum = torch.zeros(CO, device=x.device) if kind == "colsum" else None
    out = torch.empty(d["o64"].shape, device=x.device) if kind == "f32" else None
    got = K.conv2d_fwd(x, w, geom, bias=bias, act=1, colsum=colsum, out=out)
    assert got.dtype == (torch.float32 if kind == "f32" else BF16)
    ref = act(d["o64"] + bias.double().cpu())
    lim = held(got, ref, act(d["o32"] + bias.cpu()), f"{name} {kind} {route}")
    if colsum is not None:
        cerr = (colsum.double().cpu() - ref.reshape(-1, CO).sum(0)).abs()
        assert bool((cerr <= lim.reshape(-1, CO).sum(0)).all()), (cerr / lim.reshape(-1, CO).sum(0)).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,env", list(DGRAD))
def test_dgrad_route_and_result(monkeypatch, name, form, env):
    from hops_examples_amd.ops import kernels as K

    if env:
        monkeypatch.setenv("HOPSX_DISABLE", env)  # (read by the launchers on every call)
    d, geom, route = operands(name), geom_of(name), DGRAD[name, form, env]
    assert K.conv2d_dgrad_path(geom, y=form == "y", addend=form == "addend", bn=form == "bn",
                               colsum=form == "colsum") == route
    if form == "bn":  # (the trace's dgrad_bn launches carried an addend: it does not enter a bn caller's route)
        assert K.conv2d_dgrad_path(geom, addend=True, bn=True) == route
    w, dy, y, add, x = (d[k].cuda() for k in ("w", "dy", "y", "add", "x"))
    C = geom[3]
    if form == "bn":
        # the epilogue's dX alone (its column sums: tests/test_bn_dgrad_sums_gpu.py): dgrad * relu'(x).  Without an
        # addend: the direct MFMA kernel adds it to the bf16-rounded dgrad (conv_mfma.hip, "bf16 + bf16 -> bf16,
        # exactly autograd's accumulation"), two roundings where this bound allows one (measured with an addend on
        # mfma16: worst err / bound 32.7 where the two parts cancel); the other routes add in fp32.
        acc = torch.zeros(K.BN_NREP * 2 * C + 12 * 32, device=w.device)
        mean, rstd = torch.zeros(C, device=w.device), torch.ones(C, device=w.device)
        got = K.conv2d_dgrad_bn(dy, w, geom, (x, mean, rstd, x, "relu", acc))
        assert (got is False) == (route == -2)
        if got is not False:
            mask = (d["x"] > 0)
            held(got, dgrad_ref(d, name, d["dy"], torch.float64) * mask,
                 dgrad_ref(d, name, d["dy"], torch.float32) * mask, f"{name} dgrad_bn {route}")
        return
    dyr = d["dy"].double() * (d["y"] > 0) if form == "y" else d["dy"].double()  # (exact in fp32 too: a 0 / 1 mask)
    r64, r32 = dgrad_ref(d, name, dyr, torch.float64), dgrad_ref(d, name, dyr, torch.float32)
    if form == "addend":
        r64, r32 = r64 + d["add"].double(), r32 + d["add"].float()
    colsum = torch.zeros(C, device=w.device) if form == "colsum" else None
    if form == "colsum":  # the producing layer's relu' (its output yprev = x here) and its bias gradient
        r64, r32 = r64 * (d["x"] > 0), r32 * (d["x"] > 0)
    got = K.conv2d_dgrad(dy, w, geom, y=y if form == "y" else None, act="relu" if form == "y" else 0,
                         addend=add if form == "addend" else None, yprev=x if form == "colsum" else None,
                         act_prev="relu" if form == "colsum" else 0, colsum=colsum)
    lim = held(got, r64, r32, f"{name} dgrad {form} {env} {route}")
    if colsum is not None:
        cerr, clim = (colsum.double().cpu() - r64.reshape(-1, C).sum(0)).abs(), lim.reshape(-1, C).sum(0)
        assert bool((cerr <= clim).all()), (cerr / clim).max()
