"""SHA-256 digests of what twelve v2 taxi steps (csrc/ops/taxi_step.hip) leave behind, from inputs and weights
that depend on numpy alone: the bit-level fingerprint tests/test_taxi_parent_bits_gpu.py compares with
tests/golden/taxi_parent_bits.json.

A change to the step's Python runtime (where it lives, how it keys its launch slots and graphs) must hand the
kernel the same arguments in the same order of launches, hence leave every bit.  The v2 kernel sums in a fixed
order, so the bits are reproducible; the v1 kernel's float atomics are not, and it has no case here.  The golden
file is recorded on the build of the commit BEFORE such a change, never from the code under test (the engine is
imported from runtime/taxi_step.py, or from models/widedeep.py on a tree that predates the move):
usage (GPU): python tools/taxi_bits.py            print the digests of this build
             python tools/taxi_bits.py --record [--commit SHA]   write tests/golden/taxi_parent_bits.json"""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "taxi_parent_bits.json")
B, NB, STEPS = 13, 4, 12
# name -> (HOPSX_TAXI_DIRECT, loopback ranks, steps per execution, run_resident calls)
#  direct:    launches of 8 + 4 steps
#  graph:     the one-step graph, then 11 prepared steps: the 8-step graph and the 3-step remainder graph
#  loopback2: the data-parallel instantiation, one process playing both ranks, 4 + 4 + 4
CASES = {"direct": ("1", 0, 8, (12,)), "graph": ("0", 0, 8, (1, 11)), "loopback2": ("1", 2, 4, (12,))}


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _engine():
    try:
        from hops_examples_amd.runtime.taxi_step import FusedWideDeepStep, TaxiExchange
    except ImportError:  # a tree from before the runtime left the model file
        from hops_examples_amd.models.widedeep import FusedWideDeepStep, TaxiExchange
    return FusedWideDeepStep, TaxiExchange


def digests(case: str, seed: int = 20262) -> dict:
    from hops_examples_amd.models import widedeep as WD
    from hops_examples_amd.ops import functional as HF
    from hops_examples_amd.runtime.arena import ParamArena

    FusedWideDeepStep, TaxiExchange = _engine()
    direct, loopback, spe, calls = CASES[case]
    dev = torch.device("cuda", 0)
    HF.seed_device_rng(11, dev)
    rng = np.random.default_rng(seed)
    m = WD.TaxiWideDeep()
    with torch.no_grad():  # a trained-looking wide part; the deep layers uniform +-1/sqrt(fan_in)
        m.wide.weight.copy_(torch.from_numpy(rng.normal(0, 0.05, size=(WD.WIDE_ROWS, 1)).astype(np.float32)))
        for p in m.deep.parameters():
            bound = 1.0 / np.sqrt(p.shape[-1]) if p.dim() > 1 else 0.1
            p.copy_(torch.from_numpy(rng.uniform(-bound, bound, size=tuple(p.shape)).astype(np.float32)))
    n = NB * B
    dense = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).view(NB, B, 3).to(dev)
    cols = [rng.integers(0, c, size=n) for c in WD.wide_cardinalities()]
    cat = torch.from_numpy(np.stack(cols, 1).astype(np.int64) + WD.wide_offsets()).view(NB, B, -1).to(dev)
    label = torch.from_numpy((rng.random(n) < 0.4).astype(np.float32)).view(NB, B, 1).to(dev)
    m = m.to(dev)
    ParamArena.from_module(m, dev)
    opt = WD.make_optimizer(m)
    old = os.environ.get("HOPSX_TAXI_DIRECT")
    os.environ["HOPSX_TAXI_DIRECT"] = direct
    xdp = TaxiExchange(dev, loopback=loopback, timeout_s=5) if loopback > 1 else None
    try:
        fs = FusedWideDeepStep(m, opt, xdp=xdp)
        assert fs.kernel == ("v2-dp" if xdp else "v2"), fs.kernel
        fs.steps_per_execution = spe
        losses = []
        for k in calls:
            if k == 1:
                fs.step_resident((dense, cat), label)
            else:
                fs.prepare_resident((dense, cat), label, k)
                fs.run_resident((dense, cat), label, k)
            torch.cuda.synchronize()
            losses.append(fs.loss.clone())
        fs.check()
        assert int(fs.cursor.item()) == STEPS % NB
        a = m.wide.weight._hx_arena
        return {"master": _sha(a.master), "adagrad_s0": _sha(a.state("adagrad_s0")), "ftrl_s0": _sha(a.state("ftrl_s0")),
                "ftrl_s1": _sha(a.state("ftrl_s1")), "loss": _sha(torch.cat(losses))}
    finally:
        if xdp is not None:
            xdp.close()
        if old is None:
            os.environ.pop("HOPSX_TAXI_DIRECT", None)
        else:
            os.environ["HOPSX_TAXI_DIRECT"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the golden file (on the parent commit's build only)")
    ap.add_argument("--commit", default=None, help="the commit whose build is running (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    res = {name: digests(name) for name in CASES}
    print(json.dumps(res, indent=1))
    if a.record:
        rev = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        with open(a.out, "w") as f:
            json.dump({"recorded_on_commit": rev, "device": torch.cuda.get_device_name(0), "batch": B, "nbatch": NB,
                       "steps": STEPS, "digests": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
