"""SHA-256 digests of what five persistent flagship steps (csrc/ops/mnist_persist.hip) leave behind, from inputs
that depend on numpy alone: the bit-level fingerprint tests/test_persist_parent_bits_gpu.py compares with
tests/golden/persist_parent_bits.json.

A change that only re-schedules the kernel (when operands are read, how long they are held) must keep every
float operation's operands and order, hence every bit.  The golden file is recorded on the build of the commit
BEFORE such a change, never from the code under test:
usage (GPU): python tools/persist_bits.py            print the digests of this build
             python tools/persist_bits.py --record [--commit SHA]   write tests/golden/persist_parent_bits.json
             python tools/persist_bits.py --per-tensor [--record]   one digest per parameter tensor (below)

--per-tensor: one SHA-256 per parameter tensor and per arena (master, s1, s2, bf16 shadow) instead of one per arena,
plus `out`, for one process (W = 1) and for the data-parallel instantiation playing two ranks in-process
(loopback 2).  A change that moves parameters between workgroups (the conv slice owners) then shows a mistake as
the tensor it corrupts.  Recorded into tests/golden/persist_parent_conv_bits.json, which
tests/test_persist_slices_gpu.py compares."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "persist_parent_bits.json")
GOLDEN_TENSORS = os.path.join(ROOT, "tests", "golden", "persist_parent_conv_bits.json")
WORLDS = {"w1": 0, "loopback2": 2}  # --per-tensor: the loopback argument of PersistentMnistStep
CASES = {"model_rate": None, "rate_0.5": 0.5}  # dropout rate: the model's own (0.01), and one where KEEP carries weight
LAUNCHES = (3, 2)  # 5 steps, cut into two launches (the state written back between them is part of the bits)


def _sha(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:  # (numpy has no bf16: the same bytes as int16)
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def digests(drop, seed: int = 20261, loopback: int = 0, per_tensor: bool = False) -> dict:
    from hops_examples_amd import optim
    from hops_examples_amd.models.mnist import MirroredMnistCNN
    from hops_examples_amd.ops import functional as HF
    from hops_examples_amd.runtime import persist
    from hops_examples_amd.runtime.arena import ParamArena

    dev = torch.device("cuda", 0)
    HF.seed_device_rng(11, dev)
    m = MirroredMnistCNN().to(dev)
    m.pool.salt = 7919
    if drop is not None:
        m.pool.dropout = drop
    ParamArena.from_module(m, dev)
    opt = optim.Adadelta(m, lr=1.0)
    eng = persist.PersistentMnistStep(m, opt, loopback=loopback)
    rng = np.random.default_rng(seed)
    named = dict(m.named_parameters())
    with torch.no_grad():
        for k in eng.PARAMS:  # uniform +-1/sqrt(fan_in), a bias with its weight's fan_in; drawn in PARAMS order
            w = named[k.rsplit(".", 1)[0] + ".weight"]
            bound = 1.0 / np.sqrt(w.numel() // w.shape[0])
            v = rng.uniform(-bound, bound, size=tuple(named[k].shape)).astype(np.float32)
            named[k].copy_(torch.from_numpy(v))
    nb = 5
    xs = torch.from_numpy(rng.integers(0, 256, size=(nb, 32, 28, 28, 1), dtype=np.uint8)).to(dev)
    ys = torch.from_numpy(rng.integers(0, 10, size=(nb, 32), dtype=np.int64)).to(dev)
    outs = []
    for k in LAUNCHES:
        eng.run_resident(xs, ys, k)
        torch.cuda.synchronize()
        eng.check()
        outs.append(eng.losses(k).clone().flatten())
    eng.close()  # (loopback: the exchange buffers; the arenas below are the model's)
    arenas ={"master": eng.arena.master, "s1": eng.s1, "s2": eng.s2}
    if not per_tensor:
        return {**{k: _sha(v) for k, v in arenas.items()}, "out": _sha(torch.cat(outs))}
    arenas["shadow"] = eng.arena.shadow
    res = {}
    for k in eng.PARAMS:
        o, n = int(named[k]._hx_off), named[k].numel()
        for an, av in arenas.items():
            res[f"{k}/{an}"] = _sha(av[o:o + n])
    res["out"] = _sha(torch.cat(outs))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the golden file (on the parent commit's build only)")
    ap.add_argument("--commit", default=None, help="the commit whose build is running (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="the golden file to write (default: the mode's own)")
    ap.add_argument("--per-tensor", action="store_true", help="one digest per parameter tensor, W = 1 and loopback 2")
    a = ap.parse_args()
    if a.per_tensor:
        res = {wn: {name: digests(drop, loopback=lb, per_tensor=True) for name, drop in CASES.items()}
               for wn, lb in WORLDS.items()}
    else:
        res = {name: digests(drop) for name, drop in CASES.items()}
    print(json.dumps(res, indent=1))
    if a.record:
        rev = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        with open(a.out or (GOLDEN_TENSORS if a.per_tensor else GOLDEN), "w") as f:
            json.dump({"recorded_on_commit": rev, "device": torch.cuda.get_device_name(0), "launches": list(LAUNCHES),
                       "digests": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
