"""The positions' VALU work on element pairs in the persistent flagship step (csrc/ops/mnist_persist.hip, position_wg),
against the bits of the path without it and of the parent build.

``HOPSX_PERSIST_PACK``, one bit per part, default all parts in the tree (1); 0 is the path of the build before it:
1  conv1 on channel pairs: a thread owns channels 2cp, 2cp + 1 of images 2bg, 2bg + 1 instead of one channel of four
   images; the four multiply-adds of an output pair are packed fp32 fused multiply-adds (the patch value in both halves,
   the two channels' taps and biases as pairs), the two bf16 converts one packed convert and the two 2-byte LDS stores
   one 32-bit store.
(Bits 2 and 4, the conv2 epilogue and the pool backward, are reserved: no such part is in the tree, and the knob word
masks them.)

Each half of a packed multiply-add is the same IEEE fused multiply-add on the same operands in the same order, the packed
convert rounds to nearest even like the scalar one, and a wave still writes exactly the images it reads.  So five steps
from numpy-drawn inputs (tools/persist_bits.py) must leave every arena word (fp32 master, both Adadelta accumulators,
bf16 shadow; one SHA-256 per parameter tensor and arena) and every step's (loss, correct) exactly as ``PACK=0`` does and
exactly as the parent build did (tests/golden/persist_parent_conv_bits.json), at both dropout rates, in both
instantiations (one process, and the data-parallel one playing two ranks) and with launches of 1 + 2 + 2 steps: both
step parities, step 0 as a launch of its own and a launch boundary.  Equality of digests: no tolerance, no retry.

A second channel that takes tap k1 where k2 belongs, and a pair stored at 2cp + 1, were built once as mutations: each
failed this file (profiles/r23_persist_pack.txt).
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

KNOB = "HOPSX_PERSIST_PACK"
GOLDEN_TENSORS = json.loads((ROOT / "tests" / "golden" / "persist_parent_conv_bits.json").read_text())
CASES = list(persist_bits.CASES)  # both dropout cases
WORLDS = {"w1": 0, "loopback2": 2}  # one process, and the data-parallel instantiation playing two ranks
PLAN = (1, 2, 2)  # launches: step 0 alone, then both parities inside a launch and across a launch boundary
ALL = 1  # every part in the tree
PARTS = {"conv1": 1, "default": None}  # None: the knob is not set (all parts)


@contextlib.contextmanager
def _pack(v):
    """The knob for the launches inside the block (the host wrapper caches the knobs: reload); None: unset."""
    old = os.environ.get(KNOB)
    if v is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(v)
    persist._ext().mnist_persist_reload_knobs()
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old
        persist._ext().mnist_persist_reload_knobs()


@functools.lru_cache(maxsize=None)
def _digests(case: str, pack, loopback: int) -> dict:
    """Per-tensor digests of the plan's five steps; computed once per setting and shared (PACK=0, the path without
    the change, is every test's reference)."""
    old = persist_bits.LAUNCHES
    persist_bits.LAUNCHES = PLAN
    try:
        with _pack(pack):
            d = persist_bits.digests(persist_bits.CASES[case], loopback=loopback, per_tensor=True)
            # (what the knob came to in these launches: not a digest, popped by the tests)
            return {**d, "pack": persist.launch_knobs()["pack"]}
    finally:
        persist_bits.LAUNCHES = old


@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("part", list(PARTS))
def test_parts_equal_the_path_without_them(part, case, world):
    """Each part alone and all of them (the default): every arena word and every loss of PACK=0."""
    want = dict(_digests(case, 0, WORLDS[world]))
    got = dict(_digests(case, PARTS[part], WORLDS[world]))
    # the two were really different launches: the kernel's knob word followed the environment (all parts when unset)
    assert (want.pop("pack"), got.pop("pack")) == (0, ALL if PARTS[part] is None else PARTS[part])
    assert set(got) == set(want) and len(want) > 4
    bad = sorted(k for k in want if got[k] != want[k])
    print(part, case, world, PLAN, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
def test_default_equals_the_parent_build(case, world):
    """The default against the parent build's recorded digests (five steps: the same for every cut into launches)."""
    want = GOLDEN_TENSORS["digests"][world][case]
    got = dict(_digests(case, None, WORLDS[world]))
    assert got.pop("pack") == ALL
    assert set(got) == set(want) and len(want) > 4
    bad = sorted(k for k in want if got[k] != want[k])
    print(case, world, PLAN, "default vs parent, differing:", bad)
    assert not bad, bad
