"""The one-workgroup Dense-stack training step (csrc/ops/mlp_step.hip, runtime/mlp_step.py) on the GPU.

One step from a zero Adam state, weights N(0, 0.3), with ``trace`` on, checked stage by stage; each stage's fp64
reference starts from the kernel's own stored tensors (MARGIN = 8; the yardstick is the same reference evaluated in
fp32 by plain torch, floored at one fp32 ulp of the scale of the terms summed):
  forward / backward   per element of a bf16 image: |x - ref| <= 2^-8 |ref| + MARGIN acc; padding exactly zero
  logits, loss, g      fp32 values: |x - ref| <= MARGIN acc
  gradients            g = m / (1 - b1) and v against dW, db from the stored A, G: max|x - ref| / max|ref|
  update               new master from the stored m, v: test_optim_paths_gpu.py's max|x - ref| / max|ref - old|
Every check prints ``MLPERR <case> <stage> kernel <e> yardstick <y> ratio <e / y>``.  Then launch splitting (12 steps
as 12 / 8 + 4 / 1 x 12 / graph replays, trace on / off: bit-identical) and the public interface.

Measured on an MI355X, worst kernel / yardstick ratio per stage over the cases below (profiles/r24_mlp_step.txt):
forward and backward images 0.00 (no element beyond the bf16 term), z 0.27, loss 1.00, g 1.75, dW 0.60 (v 0.88),
db 0.81 (v 1.58), update 1.17; keras.fit's mean |loss difference| per epoch against the layerwise engine 1.7e-4."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd import keras as K  # noqa: E402
from hops_examples_amd import nn as hnn, optim  # noqa: E402
from hops_examples_amd.models import zoo  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402
from hops_examples_amd.runtime.mlp_step import FusedMlpStep  # noqa: E402
from hops_examples_amd.runtime.step import make_step  # noqa: E402

dev = torch.device("cuda", 0)
MARGIN, ULP = 8.0, 2.0 ** -23
R4 = ("relu",) * 4
CASES = {  # dims (input first), activations, loss, optimizer, weight decay
    "2-1": ((2, 1), (None,), "mse", "adam", 0.0),
    "2-8-8-1": ((2, 8, 8, 1), ("relu", "relu", None), "mse", "adam", 0.0),
    "10-16-1": ((10, 16, 1), ("relu", None), "bce_logits", "adam", 0.0),
    "titanic": ((6, 64, 64, 32, 32, 2, 1), R4 + ("sigmoid", None), "bce_logits", "adam", 0.0),
    "33-17-64-1": ((33, 17, 64, 1), ("sigmoid", None, None), "mse", "adam", 0.0),
    "64x8": ((64,) * 8 + (1,), ("relu",) * 7 + (None,), "bce_logits", "adamw", 0.01),
}
RUNS = [("2-1", 1), ("2-8-8-1", 7), ("10-16-1", 16), ("10-16-1", 17), ("titanic", 10), ("titanic", 64),
        ("33-17-64-1", 5), ("64x8", 48)]


def build(case, B, nbatch=1, seed=0):
    dims, acts, loss, kind, wd = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    lins = [hnn.Linear(a, b, activation=act) for a, b, act in zip(dims, dims[1:], acts)]
    for m in lins:
        m.weight.data = torch.randn(m.weight.shape, generator=gen) * 0.3
        m.bias.data = torch.randn(m.bias.shape, generator=gen) * 0.3
    net = torch.nn.Sequential(*lins).to(dev)
    ParamArena.from_module(net, dev)
    opt = optim.get(kind, net, lr=1e-2, eps=1e-7, weight_decay=wd)
    xs = torch.randn(nbatch, B, dims[0], generator=gen).to(dev)
    ys = (torch.rand(nbatch, B, 1, generator=gen) > 0.5).float().to(dev)
    return net, opt, FusedMlpStep(net, opt, loss), xs, ys


def line(tag, e, y):
    print(f"MLPERR {tag} kernel {e:.3e} yardstick {y:.3e} ratio {e / y if y else 0.0:.2f}")


def check_bf16(tag, x, ref, yard):
    acc = max((yard.double() - ref).abs().max().item(), ULP * ref.abs().max().item())
    over = (x.double() - ref).abs() - 2.0 ** -8 * ref.abs()
    line(tag, over.max().item(), acc)
    assert (over <= MARGIN * acc).all(), tag


def check_max(tag, x, ref, yard, scale, den=None):
    den = ref.abs().max().item() if den is None else den
    e, y = (x.double() - ref).abs().max().item() / den, max((yard.double() - ref).abs().max().item(), ULP * scale) / den
    line(tag, e, y)
    assert e <= MARGIN * y, tag


def act(z, a):
    return torch.relu(z) if a == "relu" else torch.sigmoid(z) if a == "sigmoid" else z


def dact(a, kind):
    return (a > 0).to(a.dtype) if kind == "relu" else a * (1 - a) if kind == "sigmoid" else torch.ones_like(a)


@pytest.mark.parametrize("case,B", RUNS)
def test_one_step_stage_by_stage(case, B):
    dims, acts, loss_kind, kind, wd = CASES[case]
    net, opt, eng, xs, ys = build(case, B)
    L, arena, geo = len(dims) - 1, opt.arena, eng.geometry(B)
    eng.trace = torch.zeros(geo["trace_elems"], device=dev, dtype=torch.bfloat16)
    old = arena.master.cpu().clone()
    out = eng.step_resident(xs, ys, graph=False)
    torch.cuda.synchronize()
    n = geo["trace_img"]
    img = eng.trace[:16 * n].cpu().view(16, 64, 64)
    zg = eng.trace[16 * n:].view(torch.float32).cpu().double()
    z, g, y = zg[:B], zg[64:64 + B], ys[0, :, 0].cpu().double()
    W = [m.weight._hx_off for m in net], [m.bias._hx_off for m in net]
    w_old = [old[o:o + m.weight.numel()].view(m.weight.shape) for m, o in zip(net, W[0])]
    b_old = [old[o:o + m.bias.numel()] for m, o in zip(net, W[1])]
    wb = [w.bfloat16() for w in w_old]
    A = [img[l, :B, :dims[l]] for l in range(L)]
    G = [img[8 + l, :B, :dims[l + 1]] for l in range(L - 1)]
    for l in list(range(L)) + list(range(8, 8 + L - 1)):  # padding rows and columns: exactly zero
        pad = img[l].clone()
        pad[:B, :dims[l % 8 + (l >= 8)]] = 0
        assert torch.count_nonzero(pad) == 0, (case, "padding", l)
    assert torch.equal(A[0], xs[0].cpu().bfloat16())
    # 1. forward, from the previous stored image and the bf16 weights
    for l in range(L - 1):
        f = lambda dt: act(A[l].to(dt) @ wb[l].to(dt).T + b_old[l].to(dt), acts[l])  # noqa: E731
        check_bf16(f"{case}/B{B} fwd{l}", A[l + 1], f(torch.float64), f(torch.float32))
    f = lambda dt: A[-1].to(dt) @ wb[-1].to(dt)[0] + b_old[-1].to(dt)[0]  # noqa: E731
    terms = (A[-1].double().abs() @ wb[-1].double().abs()[0]).max().item() + b_old[-1].abs().item()
    check_max(f"{case}/B{B} z", z, f(torch.float64), f(torch.float32), terms)

    def loss_g(dt):
        zz, yy = z.to(dt), y.to(dt)
        if loss_kind == "mse":
            return ((zz - yy) ** 2).mean(), 2 * (zz - yy) / B
        return (zz.clamp_min(0) - zz * yy + torch.log1p(torch.exp(-zz.abs()))).mean(), (torch.sigmoid(zz) - yy) / B

    (l64, g64), (l32, g32) = loss_g(torch.float64), loss_g(torch.float32)
    check_max(f"{case}/B{B} loss", out["loss"].cpu(), l64.reshape(1), l32.reshape(1), l64.abs().item())
    check_max(f"{case}/B{B} g", g, g64, g32, 1.0 / B)
    if loss_kind != "mse":
        assert int(out["correct"]) == int(((z > 0) == (y > 0.5)).sum())
    # 2. backward, from the stored next G (the top one from the stored g)
    for l in range(L - 2, -1, -1):
        if l == L - 2:
            f = lambda dt: g.to(dt)[:, None] * wb[-1].to(dt) * dact(A[l + 1].to(dt), acts[l])  # noqa: E731
        else:
            f = lambda dt: (G[l + 1].to(dt) @ wb[l + 1].to(dt)) * dact(A[l + 1].to(dt), acts[l])  # noqa: E731
        check_bf16(f"{case}/B{B} bwd{l}", G[l], f(torch.float64), f(torch.float32))
    # 3. gradients from the stored A and G, through m = (1 - b1) g and v = (1 - b2) g^2
    hp = torch.tensor(opt._hp(), dtype=torch.float32).double()
    lr, b1, b2, eps = hp[0], hp[3], hp[4], hp[5]
    new, m1, v1 = arena.master.cpu(), arena.state(f"{kind}_s0").cpu(), arena.state(f"{kind}_s1").cpu()
    for l in range(L):
        top = g[:, None].float() if l == L - 1 else G[l].float()
        for name, off, shape, fn in (("dW", W[0][l], w_old[l].shape, lambda t, dt, l=l: t.to(dt).T @ A[l].to(dt)),
                                     ("db", W[1][l], b_old[l].shape, lambda t, dt: t.to(dt).sum(0))):
            k = w_old[l].numel() if name == "dW" else b_old[l].numel()
            r64, r32 = fn(top, torch.float64).reshape(shape), fn(top, torch.float32).reshape(shape)
            scale = (fn(top.abs(), torch.float64) if name == "db" else top.double().abs().T @ A[l].double().abs()).max().item()
            mk, vk = m1[off:off + k].view(shape).double(), v1[off:off + k].view(shape).double()
            if r64.abs().max() > 0:
                check_max(f"{case}/B{B} {name}{l}", mk / (1 - b1), r64, r32, scale)
                check_max(f"{case}/B{B} v{name}{l}", vk, (1 - b2) * r64 ** 2, ((1 - b2).float() * r32 ** 2), scale ** 2 * (1 - b2).item())
            else:  # (every unit dead: the moments stay exactly zero)
                assert mk.abs().max() == 0 and vk.abs().max() == 0, (case, name, l)
            # 4. the update from the kernel's own m, v and the old weight (test_optim_paths_gpu.py's metric)
            po = old[off:off + k].view(shape)

            def rule(dt, po=po, mk=mk, vk=vk):
                p = po.to(dt) * (1 - (lr * wd).to(dt)) if kind == "adamw" else po.to(dt)
                return p - lr.to(dt) * (mk.to(dt) / (1 - b1).to(dt)) / ((vk.to(dt) / (1 - b2).to(dt)).sqrt() + eps.to(dt))

            r64 = rule(torch.float64)
            check_max(f"{case}/B{B} p{name}{l}", new[off:off + k].view(shape), r64, rule(torch.float32), 0.0,
                      den=(r64 - po.double()).abs().max().item())
    assert torch.equal(arena.shadow.cpu(), new.bfloat16()) and torch.count_nonzero(arena.grad) == 0
    assert float(opt.step_count) == 1.0 and int(eng.cursor) == 0


@pytest.mark.parametrize("case,B", [("titanic", 10), ("titanic", 64)])  # (state in LDS; state in the arena)
def test_launch_splitting_and_trace_are_bit_neutral(case, B):
    net, opt, eng, xs, ys = build(case, B, nbatch=5)
    arena, kind = opt.arena, CASES[case][3]
    start = arena.master.clone()

    def run(per_launch, graph=False, trace=False):
        arena.master.copy_(start)
        arena.refresh_shadow()
        for t in (arena.state(f"{kind}_s0"), arena.state(f"{kind}_s1"), opt.step_count, eng.cursor):
            t.zero_()
        eng.trace = torch.zeros(eng.geometry(B)["trace_elems"], device=dev, dtype=torch.bfloat16) if trace else None
        eng.steps_per_execution, losses = per_launch, []
        if graph:
            losses = [eng.step_resident(xs, ys)["loss"].clone() for _ in range(12)]
        else:
            eng.run_resident(xs, ys, 12, on_out=lambda outs: losses.extend(o["loss"].clone() for o in outs))
        torch.cuda.synchronize()
        assert int(eng.cursor) == 12 % 5 and float(opt.step_count) == 12.0
        return [t.cpu().clone() for t in (arena.master, arena.state(f"{kind}_s0"), arena.state(f"{kind}_s1"),
                                          arena.shadow.view(torch.int16), torch.cat(losses))]

    ref = run(12)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[4]).all()
    for tag, kw in {"8+4": dict(per_launch=8), "1x12": dict(per_launch=1), "graph": dict(per_launch=1, graph=True),
                    "trace": dict(per_launch=12, trace=True)}.items():
        got = run(**kw)
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(ref, got)), tag


def _titanic(kind="adam"):
    m = zoo.titanic_dnn()
    m.build()
    m.to(dev)
    ParamArena.from_module(m, dev)
    return m, optim.get(kind, m, lr=1e-3)


@pytest.mark.parametrize("why,env,kind,loss,batch", [
    (None, None, "adam", "bce_logits", 10), ("env", "0", "adam", "bce_logits", 10), ("sgd", None, "sgd", "bce_logits", 10),
    ("batch", None, "adam", "bce_logits", 65), ("loss", None, "adam", "bce", 10)])
def test_make_step_picks_or_declines(monkeypatch, why, env, kind, loss, batch):
    if env is not None:
        monkeypatch.setenv("HOPSX_MLP_STEP", env)
    m, opt = _titanic(kind)
    eng = make_step(m, opt, loss, batch=batch)
    assert (eng.kind, eng.note is None) == (("mlp-step", True) if why is None else ("trainstep", False))


@pytest.mark.parametrize("u8,B", [(False, 10), (True, 16)], ids=["float-B10", "uint8-B16"])
def test_keras_fit_trains_and_tracks_the_layerwise_engine(monkeypatch, u8, B):
    """105 rows: the full batches on the engine, the partial one on the TrainStep, same arena.  uint8 features are
    scaled by 1 / 255 in the model's input layer, which the engine does not do: they stay on the TrainStep."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (105, 6), generator=gen, dtype=torch.uint8).numpy() if u8 else torch.randn(105, 6, generator=gen).numpy()
    y = ((x[:, 0] > 127) if u8 else (x[:, 0] + 0.5 * x[:, 1] > 0)).astype("float32").reshape(-1, 1)
    hist = {}
    for env in ("1", "0"):
        monkeypatch.setenv("HOPSX_MLP_STEP", env)
        # (the layerwise run batch by batch: TrainStep's resident prefetch needs 16-byte batch slices, 10 labels are 40)
        monkeypatch.setenv("HOPSX_KERAS_RESIDENT", "1" if u8 else env)
        torch.manual_seed(11)
        m = K.Sequential([K.layers.Dense(16, activation="relu", input_shape=(6,)), K.layers.Dense(1, activation="sigmoid")])
        m.compile(optimizer=K.optimizers.Adam(learning_rate=0.01), loss="binary_crossentropy", metrics=["accuracy"])
        hist[env] = m.fit(x, y, batch_size=B, epochs=8, verbose=0, shuffle=False).history
        eng = m._mlp_engine(B)
        assert (eng is not None) == (env == "1") and (eng is None or (eng._n > 0) == (not u8))
    a, b = torch.tensor(hist["1"]["loss"]), torch.tensor(hist["0"]["loss"])
    print(f"MLPERR keras-fit mean |loss difference| per epoch {(a - b).abs().mean().item():.3e}")
    assert set(hist["1"]) == set(hist["0"]) and a[-1] < a[0]
    # bf16 noise between the engines: test_taxi_v2_tracks_fp32_training's 5e-2, tightened to 30x the measured 1.7e-4
    assert (a - b).abs().mean() <= 5e-3
