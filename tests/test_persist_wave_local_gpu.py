"""The positions' wave-local staging of the persistent flagship step (csrc/ops/mnist_persist.hip, position_wg),
against the bits of the path without it and of the parent build.

``HOPSX_PERSIST_WLOCAL``, one bit per part, default all (7); 0 is the path of the build before it:
1  the forward up to the pooled tile without workgroup barriers (XIN fill -> conv1 -> conv2: producer and consumer of
   XIN and C1 are the same wave, so a wave-level ordering point stands where the two barriers stood);
2  hand-off A published per wave: a wave stages its 32 x 32 block of the fc1 partial product, reads it back itself and
   stores it without waiting for the other waves;
4  the backward with ONE workgroup barrier instead of two: pool backward -> conv2 weight gradient is wave-local, every
   wave publishes its own 16 x 128 block of C's part 1 as soon as its MFMAs are done, and the barrier stands in front
   of the conv2 input gradient's transposed DC2 reads, the only ones that cross waves.

None of this changes a float operation's operands or order, a payload byte, a flag or an epoch, so five steps from
numpy-drawn inputs (tools/persist_bits.py) must leave every arena word (fp32 master, both Adadelta accumulators, bf16
shadow; one SHA-256 per parameter tensor and arena) and every step's (loss, correct) exactly as ``WLOCAL=0`` does,
with each bit alone and with the default, at both dropout rates, in both instantiations (one process, and the
data-parallel one playing two ranks) and with launches of 1 + 2 + 2 steps: both step parities, step 0 as a launch of
its own and a launch boundary.  Equality of digests: no tolerance, no retry.  The parent build's bytes themselves are
the golden files of tests/test_persist_parent_bits_gpu.py and its siblings.

A wave that reads back another wave's block of A publishes other words, and DC2 read in front of the backward's
barrier can be read before it is written: built once as mutations, each failed this file
(profiles/r21_persist_wave_local.txt).
"""
import contextlib
import functools
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

KNOB = "HOPSX_PERSIST_WLOCAL"
CASES = list(persist_bits.CASES)  # both dropout cases
WORLDS = {"w1": 0, "loopback2": 2}  # one process, and the data-parallel instantiation playing two ranks
PLAN = (1, 2, 2)  # launches: step 0 alone, then both parities inside a launch and across a launch boundary
PARTS = {"forward": 1, "publish_a": 2, "backward": 4, "default": None}  # None: the knob is not set (all parts)


@contextlib.contextmanager
def _wlocal(v):
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
def _digests(case: str, wlocal, loopback: int) -> dict:
    """Per-tensor digests of the plan's five steps; computed once per setting and shared (WLOCAL=0, the path without
    the change, is every test's reference)."""
    old = persist_bits.LAUNCHES
    persist_bits.LAUNCHES = PLAN
    try:
        with _wlocal(wlocal):
            d = persist_bits.digests(persist_bits.CASES[case], loopback=loopback, per_tensor=True)
            # (what the knob came to in these launches: not a digest, popped by the tests)
            return {**d, "wlocal": persist.launch_knobs()["wlocal"]}
    finally:
        persist_bits.LAUNCHES = old


@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("part", list(PARTS))
def test_parts_equal_the_path_without_them(part, case, world):
    """Each part alone and all of them (the default): every arena word and every loss of WLOCAL=0."""
    want = dict(_digests(case, 0, WORLDS[world]))
    got = dict(_digests(case, PARTS[part], WORLDS[world]))
    # the two were really different launches: the kernel's knob word followed the environment (all parts when unset)
    assert (want.pop("wlocal"), got.pop("wlocal")) == (0, 7 if PARTS[part] is None else PARTS[part])
    assert set(got) == set(want) and len(want) > 4
    bad = sorted(k for k in want if got[k] != want[k])
    print(part, case, world, PLAN, "differing:", bad)
    assert not bad, bad
