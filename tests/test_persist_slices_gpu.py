"""The conv slice owners of the persistent flagship step (csrc/ops/mnist_persist.hip, hand-offs C and D) with
line-aligned slices, against the bits of the parent build.

A slice is 64 conv parameters: two whole 128-byte lines of every partial row of hand-off C, and one whole bf16
line (or two whole fp32 lines) of hand-off D.  Which workgroup owns a parameter changes no float operation: every
element is still the fp32 sum of the 169 partials in the order (v[0] + ... + v[8]) per group, then the 19 groups,
then Adadelta.  So five steps (launches of 3 + 2) from numpy-drawn inputs must leave, tensor by tensor, the bytes
the parent commit's build left: SHA-256 of master, both Adadelta states and the bf16 shadow of each of the eight
parameter tensors, and of the per-step (loss, correct) outputs, recorded on that build by
``tools/persist_bits.py --per-tensor --record`` into tests/golden/persist_parent_conv_bits.json (the file names the
commit).  One digest per tensor makes a wrong slice show up as the tensor it corrupts: slices 0..127 are
conv2.weight, 128 conv2.bias, 129 and 130 conv1.weight, 131 (half filled) conv1.bias.

Cases: the default (progressive) form of the owners' gather and the flag form (``HOPSX_PERSIST_PROG=0``), both
dropout rates; the data-parallel instantiation playing two ranks in-process (loopback 2) against its own parent
digests.
"""
import contextlib
import functools
import json
import os
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.runtime import persist  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import persist_bits  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "persist_parent_conv_bits.json").read_text())


@contextlib.contextmanager
def _knobs(**kv):
    """Launch knobs for the launches inside the block (the host wrapper caches them: reload)."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    persist._ext().mnist_persist_reload_knobs()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        persist._ext().mnist_persist_reload_knobs()


@functools.lru_cache(maxsize=None)
def _digests(world: str, case: str, prog: int) -> dict:
    with _knobs(HOPSX_PERSIST_PROG=prog):
        return persist_bits.digests(persist_bits.CASES[case], loopback=persist_bits.WORLDS[world], per_tensor=True)


def test_slice_geometry():
    """A slice row is whole 128-byte lines, no slice straddles conv2.weight's end, every parameter has an owner,
    every owner is a position workgroup, and the exchange slot holds exactly the slices."""
    from hops_examples_amd.models.mnist import MirroredMnistCNN

    g = persist.geometry()
    conv2w = dict(MirroredMnistCNN().named_parameters())["conv2.weight"].numel()
    assert g["slice"] * 4 % 128 == 0
    assert conv2w % g["slice"] == 0
    assert g["nslice"] * g["slice"] >= g["nconv"]
    assert (g["nslice"] - 1) * g["slice"] < g["nconv"]  # (no owner without a parameter)
    assert g["nslice"] <= g["npos"]
    assert g["xs_conv"] == g["nslice"] * g["slice"] * 4


def test_golden_covers_every_tensor():
    assert GOLDEN["launches"] == list(persist_bits.LAUNCHES)
    want = {f"{k}/{a}" for k in persist.PersistentMnistStep.PARAMS for a in ("master", "s1", "s2", "shadow")} | {"out"}
    for world in persist_bits.WORLDS:
        for case in persist_bits.CASES:
            assert set(GOLDEN["digests"][world][case]) == want, (world, case)


@pytest.mark.parametrize("prog", [3, 0], ids=["progressive", "flag_form"])
@pytest.mark.parametrize("case", list(persist_bits.CASES))
def test_owners_keep_parent_bits_per_tensor(case, prog):
    """W = 1: both forms of the owners' gather leave every tensor of every arena as the parent's build did."""
    got = _digests("w1", case, prog)
    want = GOLDEN["digests"]["w1"][case]
    bad = sorted(k for k in want if got.get(k) != want[k])
    print(case, prog, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("case", list(persist_bits.CASES))
def test_loopback2_keeps_parent_bits_per_tensor(case):
    """The data-parallel instantiation (two ranks played in-process: the slice sums cross the exchange buffer,
    whose slots follow the slice geometry) against its own parent digests."""
    got = _digests("loopback2", case, 3)
    want = GOLDEN["digests"]["loopback2"][case]
    bad = sorted(k for k in want if got.get(k) != want[k])
    print(case, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("which", ["slabC", "slabD"])
def test_launcher_refuses_unaligned_slabs(which):
    """The owners read whole lines of slabC and write whole lines of slabD: a slab that is not 128-byte aligned is
    refused by the launcher (hipErrorInvalidValue), nothing is launched."""
    from hops_examples_amd import optim
    from hops_examples_amd.models.mnist import MirroredMnistCNN
    from hops_examples_amd.runtime.arena import ParamArena

    dev = torch.device("cuda", 0)
    m = MirroredMnistCNN().to(dev)
    ParamArena.from_module(m, dev)
    eng = persist.PersistentMnistStep(m, optim.Adadelta(m, lr=1.0))
    n = getattr(eng, which).numel()
    shifted = torch.empty(n + 16, device=dev, dtype=torch.float32)[16:]  # 64 bytes off a line
    assert shifted.data_ptr() % 128 == 64
    setattr(eng, which, shifted)
    xs = torch.zeros(1, 32, 28, 28, 1, dtype=torch.uint8, device=dev)
    ys = torch.zeros(1, 32, dtype=torch.int64, device=dev)
    before = eng.arena.master.clone()
    with pytest.raises(RuntimeError, match="hipError 1"):
        eng.run_resident(xs, ys, 1)
    torch.cuda.synchronize()
    assert torch.equal(eng.arena.master, before)
