"""Frozen ResNet inference on the GPU: the residual conv epilogue on every forward route, the engine layer by
layer and end to end against fp64 references computed from the bf16 operands the kernels read, and the
Predictor routing.

Bound of every element-wise comparison against fp64: ``2^-8 |ref| + (1 + 2^-8) * 4 * e32``.  The first term
is half a bf16 ulp of the stored value; ``e32`` is max |fp32 proxy - fp64| of the same formula on the test's
own inputs and 4 the project's factor for another fp32 summation order."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_frozen_fold_cpu import randomize_bn

BF16 = torch.bfloat16
RELU, NONE = 1, 0

# name: (B, H, W, C, CO, k, stride, act, route).  The smallest shapes that can still go wrong on each route:
#   mfma  : M = 25 leaves a ragged 16-row pixel group; CO = 16 / 32 / 64 are three kernel instantiations.  The
#           256 -> 64 1x1 conv the ResNet-50 blocks open with takes this route at every size (K <= 512, CO = 64).
#   gemm  : M = 50, N = 40: the scalar epilogue with N no multiple of 16, ragged 32-row tiles.
#   gg    : the LDS-DMA engine needs >= 32 workgroups of 128 x 128: 64 -> 64 3x3 from 63 x 63 pixels on
#           (3,969 rows = 32 tiles), and, as the 256 -> 64 1x1 is not routed there, the bottleneck's expanding
#           64 -> 256 1x1 conv (the one that takes the residual in ResNet-50) from 44 x 44 on (16 x 2 tiles).
#   splitk: 512 -> 512 3x3 at 7 x 7, B = 2 (K = 4,608 split over the ticket finish).
CASES = {
    "mfma16": (1, 5, 5, 16, 16, 3, 1, RELU, "mfma"),
    "mfma32": (1, 5, 5, 32, 32, 3, 1, RELU, "mfma"),
    "mfma_1x1_256_64": (1, 5, 5, 256, 64, 1, 1, NONE, "mfma"),
    "gemm": (2, 5, 5, 64, 40, 1, 1, RELU, "gemm"),
    "gg_3x3_64_64": (1, 63, 63, 64, 64, 3, 1, RELU, "gg"),
    "gg_1x1_64_256": (1, 44, 44, 64, 256, 1, 1, RELU, "gg"),
    "splitk": (2, 7, 7, 512, 512, 3, 1, RELU, "splitk"),
}


def bound(ref, e32):
    return 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * 4 * e32


def conv_ref(x, w, bias, res, act, stride, dtype):
    """act(conv(x, w) + bias + res) in ``dtype`` on the CPU from bf16 operands (NHWC, w [CO, KH, KW, C])."""
    k = w.shape[1]
    o = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(0, 3, 1, 2), bias.to(dtype), stride, k // 2)
    o = o.permute(0, 2, 3, 1)
    pre = o if res is None else o + res.to(dtype)
    return (pre.clamp_min(0) if act == RELU else pre), o


_CASE_CACHE = {}


def case_data(name):
    """CPU operands and references of a kernel case, computed once."""
    if name not in _CASE_CACHE:
        B, H, W, C, CO, k, s, act, route = CASES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(B, H, W, C, generator=g).to(BF16)
        w = (torch.randn(CO, k, k, C, generator=g) * (2.0 / (k * k * C)) ** 0.5).to(BF16)
        bias = torch.randn(CO, generator=g) * 0.1
        _, o = conv_ref(x, w, bias, None, NONE, s, torch.float64)
        # the residual at twice the conv output's spread: the add then flips the sign of about a third of the
        # elements (atan(2) / pi), so an epilogue that applies the ReLU before the add cannot pass
        res = (torch.randn(o.shape, generator=g) * 2 * o.std().item()).to(BF16)
        ref, o = conv_ref(x, w, bias, res, act, s, torch.float64)
        flipped = ((o > 0) != ((o + res.double()) > 0)).double().mean().item()
        ref32, _ = conv_ref(x, w, bias, res, act, s, torch.float32)
        e32 = (ref32.double() - ref).abs().max().item()
        ref0, _ = conv_ref(x, w, bias, None, act, s, torch.float64)  # (without the residual)
        ref0_32, _ = conv_ref(x, w, bias, None, act, s, torch.float32)
        e32_0 = (ref0_32.double() - ref0).abs().max().item()
        _CASE_CACHE[name] = dict(x=x, w=w, bias=bias, res=res, ref=ref, e32=e32, flipped=flipped, ref0=ref0,
                                 e32_0=e32_0)
    return _CASE_CACHE[name]


def geom_of(name):
    from hops_examples_amd.ops import kernels as K

    B, H, W, C, CO, k, s, act, route = CASES[name]
    return K.conv_geom((B, H, W, C), (CO, k, k, C), (s, s), (k // 2, k // 2), (1, 1))


@pytest.mark.parametrize("name", list(CASES))
def test_residual_flips_signs_on_the_reference(name):
    assert case_data(name)["flipped"] >= 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_residual_epilogue_per_route(name):
    from hops_examples_amd.ops import kernels as K

    act, route = CASES[name][7], CASES[name][8]
    d = case_data(name)
    geom = geom_of(name)
    assert K.conv2d_fwd_res_path(geom) == route
    x, w, bias, res = (d[k].cuda() for k in ("x", "w", "bias", "res"))
    got = K.conv2d_fwd_res(x, w, geom, bias=bias, act=act, residual=res)
    assert got.dtype == BF16 and tuple(got.shape) == tuple(d["ref"].shape)
    err = (got.double().cpu() - d["ref"]).abs()
    lim = bound(d["ref"], d["e32"])
    print(f"{name}: route {route} e32 {d['e32']:.3e} max err {err.max():.3e} worst err/bound {(err / lim).max():.3f}")
    assert bool((err <= lim).all()), (err / lim).max()
    # a second launch: the split-K workspace and its tickets are back at rest, so it meets the bound again (its
    # K slices meet in fp32 atomics, in any order); every other route has one summation order and gives the same bits
    again = K.conv2d_fwd_res(x, w, geom, bias=bias, act=act, residual=res)
    assert bool(((again.double().cpu() - d["ref"]).abs() <= lim).all())
    assert route == "splitk" or torch.equal(again, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_without_residual_it_is_conv2d_fwd(name):
    from hops_examples_amd.ops import _C, kernels as K

    act, route = CASES[name][7], CASES[name][8]
    d = case_data(name)
    geom = geom_of(name)
    x, w, bias = (d[k].cuda() for k in ("x", "w", "bias"))
    want = K.conv2d_fwd(x, w, geom, bias=bias, act=act)
    got = K.conv2d_fwd_res(x, w, geom, bias=bias, act=act, residual=None)
    raw = torch.full_like(want, 7.0)
    rc = _C.ext().conv2d_fwd_res(x.data_ptr(), w.data_ptr(), geom, raw.data_ptr(), bias.data_ptr(), act, 0, _C.stream())
    assert rc == 0
    if route != "splitk":
        assert torch.equal(got, want) and torch.equal(raw, want)
        return
    # split-K: the K slices meet in fp32 atomics in arrival order, so two launches of conv2d_fwd itself may differ
    # in the last bit; bitwise equality of separate launches does not exist on this route, and each launch is
    # held to the fp64 bound (residual=None is the same launcher call as conv2d_fwd, in Python and in C).
    lim = bound(d["ref0"], d["e32_0"])
    for t in (want, got, raw):
        assert bool(((t.double().cpu() - d["ref0"]).abs() <= lim).all())


@pytest.mark.gpu
def test_aliased_or_misaligned_residual_is_refused():
    from hops_examples_amd.ops import _C, kernels as K

    d = case_data("mfma16")
    geom = geom_of("mfma16")
    x, w, bias, res = (d[k].cuda() for k in ("x", "w", "bias", "res"))
    out = torch.full(tuple(res.shape), 7.0, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="alias"):
        K.conv2d_fwd_res(x, w, geom, bias=bias, act=RELU, residual=out, out=out)
    buf = torch.zeros(res.numel() + 8, device="cuda", dtype=BF16)
    off = buf[1:1 + res.numel()].view(res.shape)
    off.copy_(res)
    assert off.data_ptr() % 16 == 2
    with pytest.raises(ValueError, match="aligned"):
        K.conv2d_fwd_res(x, w, geom, bias=bias, act=RELU, residual=off, out=out)
    with pytest.raises(ValueError, match="relu"):
        K.conv2d_fwd_res(x, w, geom, bias=bias, act="tanh", residual=res, out=out)
    # the launcher itself refuses too, and launches nothing
    ext, st = _C.ext(), _C.stream()
    args = (x.data_ptr(), w.data_ptr(), geom, out.data_ptr(), bias.data_ptr(), RELU)
    assert ext.conv2d_fwd_res(*args, out.data_ptr(), st) == -5
    assert ext.conv2d_fwd_res(*args, out.data_ptr() + 32, st) == -5  # a partial overlap
    assert ext.conv2d_fwd_res(*args, off.data_ptr(), st) == -4
    assert ext.conv2d_fwd_res(*args[:5], 3, res.data_ptr(), st) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ the engine
def build(name):
    from hops_examples_amd.models.resnet import ResNet50, cifar_resnet

    torch.manual_seed(3)
    model = cifar_resnet(20) if name == "resnet20" else ResNet50(10, layers=(1, 1, 1, 1))
    return randomize_bn(model, 11).eval()


_MODELS = {}


def models(name):
    """(CPU model, its GPU copy, the frozen engine of the copy), built once; tests leave them unchanged."""
    if name not in _MODELS:
        from hops_examples_amd.runtime.frozen import FrozenResNet

        cpu = build(name)
        gpu = copy.deepcopy(cpu).cuda().eval()
        _MODELS[name] = (cpu, gpu, FrozenResNet.freeze(gpu))
    return _MODELS[name]


def images(name, n, seed=9):
    hw = 32 if name == "resnet20" else 64
    return torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["resnet20", "resnet50_1111"])
def test_every_layer_teacher_forced(name):
    from hops_examples_amd.models.resnet import ConvBN

    cpu, gpu, eng = models(name)
    rec = eng.trace(images(name, 2).cuda())
    convbn = dict((n, m) for n, m in gpu.named_modules() if isinstance(m, ConvBN))
    assert [r[0] for r in rec] and sorted(r[0] for r in rec) == sorted(convbn)
    with_res = 0
    for lname, xin, res, out in rec:
        w, b = eng.folded(lname)
        w = w.cpu()
        if xin.shape[-1] != w.shape[-1]:  # the stem's input is laid out as 8 channels, 3..7 zero
            assert lname == "stem" and bool((xin[..., w.shape[-1]:] == 0).all())
            w = F.pad(w, (0, xin.shape[-1] - w.shape[-1]))
        m = convbn[lname]
        act = RELU if m.bn.activation == "relu" else NONE
        st = int(m.conv.cfg["stride"])
        r = None if res is None else res.cpu()
        ref, _ = conv_ref(xin.cpu(), w, b.cpu(), r, act, st, torch.float64)
        ref32, _ = conv_ref(xin.cpu(), w, b.cpu(), r, act, st, torch.float32)
        e32 = (ref32.double() - ref).abs().max().item()
        err = (out.double().cpu() - ref).abs()
        lim = bound(ref, e32)
        assert bool((err <= lim).all()), (lname, (err / lim).max().item())
        with_res += res is not None
    assert with_res == len(gpu.blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("resnet20", 16), ("resnet50_1111", 4)])
def test_logits_against_the_emulated_reference(name, n):
    from hops_examples_amd.runtime.frozen import reference_forward

    cpu, gpu, eng = models(name)
    x = images(name, n)
    ref = reference_forward(cpu, x, torch.float64, emulate_bf16=True)
    proxy = reference_forward(cpu, x, torch.float32, emulate_bf16=True)
    e32 = (proxy.double() - ref).abs().max().item()
    got = eng(x.cuda()).double().cpu()
    with torch.no_grad():
        unfrozen = gpu(x.cuda()).double().cpu()
    exact = reference_forward(cpu, x, torch.float64, emulate_bf16=False)
    err = (got - ref).abs().max().item()
    print(f"{name}: |logits| {ref.abs().max():.2f} e32 {e32:.4f} frozen-vs-emulated {err:.4f}; to the exact fp64 "
          f"forward: frozen {(got - exact).abs().max():.4f} unfrozen {(unfrozen - exact).abs().max():.4f} "
          f"emulated {(ref - exact).abs().max():.4f}")
    assert err <= 4 * e32, (err, e32)


@pytest.mark.gpu
def test_no_bn_launch_and_one_conv_per_convbn(monkeypatch):
    from hops_examples_amd.models.resnet import ConvBN
    from hops_examples_amd.ops import kernels as K

    cpu, gpu, eng = models("resnet20")
    x = images("resnet20", 2).cuda()
    want = eng(x)
    calls = []

    def boom(*a, **k):
        raise AssertionError("bn_fwd_infer launched on the frozen path")

    def counted(fn):
        def f(*a, **k):
            calls.append(fn.__name__)
            return fn(*a, **k)
        return f

    monkeypatch.setattr(K, "bn_fwd_infer", boom)
    monkeypatch.setattr(K, "conv2d_fwd", counted(K.conv2d_fwd))
    monkeypatch.setattr(K, "conv2d_fwd_res", counted(K.conv2d_fwd_res))
    got = eng(x)
    assert torch.equal(got, want)
    n = sum(isinstance(m, ConvBN) for m in gpu.modules())
    assert n == 21 and len(calls) == n and calls.count("conv2d_fwd_res") == len(gpu.blocks)
    with pytest.raises(AssertionError), torch.no_grad():
        gpu(x)  # the unfrozen path does launch it


@pytest.mark.gpu
def test_refresh_refolds_in_place_and_graphs_stay_valid():
    from hops_examples_amd.runtime.capture import graph as capture
    from hops_examples_amd.runtime.frozen import FrozenResNet

    gpu = copy.deepcopy(models("resnet20")[1])
    eng = FrozenResNet.freeze(gpu)
    x = images("resnet20", 2).cuda()
    y0 = eng(x).clone()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with capture(cg):
        out = eng(x)
    cg.replay()
    assert torch.equal(out, y0)
    ptrs = [t.data_ptr() for t in eng.buffers()]
    with torch.no_grad():
        gpu.blocks[1].b.bn.weight[3] *= 1.5
        gpu.blocks[4].a.bn.running_mean[5] += 0.75
        gpu.stem.bn.running_mean[0] -= 0.5
    assert torch.equal(eng(x), y0)  # a snapshot: nothing changes until refresh()
    eng.refresh()
    fresh = FrozenResNet.freeze(gpu)(x)
    assert not torch.equal(fresh, y0)
    assert torch.equal(eng(x), fresh)
    assert [t.data_ptr() for t in eng.buffers()] == ptrs
    cg.replay()
    assert torch.equal(out, fresh)


@pytest.mark.gpu
def test_predictor_routing(monkeypatch):
    from hops_examples_amd import inference as I
    from hops_examples_amd.models.mnist import MirroredMnistCNN
    from hops_examples_amd.runtime.frozen import FrozenResNet

    gpu = models("resnet20")[1]
    assert isinstance(I.Predictor(gpu).frozen, FrozenResNet)
    assert isinstance(I.Predictor(gpu, frozen=True).frozen, FrozenResNet)
    assert I.Predictor(gpu, frozen=False).frozen is None
    monkeypatch.setenv("HOPSX_INFER_FROZEN", "0")
    assert I.Predictor(gpu).frozen is None
    monkeypatch.delenv("HOPSX_INFER_FROZEN")
    other = MirroredMnistCNN().cuda()
    assert I.Predictor(other).frozen is None
    with pytest.raises(ValueError):
        I.Predictor(other, frozen=True)
    imgs = images("resnet20", 10).numpy()
    eager = I.predict(gpu, imgs, batch_size=4, graph=False)
    pr = I.Predictor(gpu, graph=True)
    replay = np.concatenate(list(pr.predict_batches(imgs[i:i + 4] for i in range(0, 10, 4))))
    assert pr.frozen is not None and pr.replays == 3  # 4 + 4 + a ragged 2
    np.testing.assert_array_equal(replay, eager)
    off = I.predict(gpu, imgs, batch_size=4, frozen=False)
    assert np.abs(off.sum(1) - 1).max() < 1e-4 and np.abs(eager.sum(1) - 1).max() < 1e-4
