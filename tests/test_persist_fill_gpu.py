"""The waits of the persistent flagship step (csrc/ops/mnist_persist.hip, position_wg) filled with work that is
ready early, against the bits of the unfilled schedule and of the parent build.

``HOPSX_PERSIST_FILL`` moves two pieces of a step to where a position workgroup waits anyway, one bit each:
1 the slice owners' lane-owned fc1 Adadelta, a chunk per poll of the progressive C gather (``<false>`` only, whatever
  is left runs behind the D publish as before; ``HOPSX_PERSIST_FILL_MAX`` caps the chunks inside the wait, so both ends
  of a split that otherwise depends on timing can be forced);
2 the next step's dropout keep mask, drawn at the head of the B wait instead of behind the fc1 update.
(A third part, D's conv2 weights held in registers over the next step's conv1, passed these checks and measured no
gain: it is not in the tree, profiles/r17_persist_fill_waits.txt.)

None of them changes a float operation's operands or order, so five steps (launches of 3 + 2, the plan of
tools/persist_bits.py) from numpy-drawn inputs must leave every arena word (fp32 master, both Adadelta
accumulators, bf16 shadow; one SHA-256 per parameter tensor and arena) and every step's (loss, correct) exactly as
the default schedule does, and the default as the parent commit's build did
(tests/golden/persist_parent_conv_bits.json, tests/golden/persist_parent_bits.json).  Equality of digests: no
tolerance.

A chunk that is skipped or run twice and a mask drawn for the wrong step change values, hence digests (each was
built once as a mutation and failed this file: profiles/r17_persist_fill_waits.txt).
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

GOLDEN_TENSORS = json.loads((ROOT / "tests" / "golden" / "persist_parent_conv_bits.json").read_text())
GOLDEN = json.loads((ROOT / "tests" / "golden" / "persist_parent_bits.json").read_text())
CASES = list(persist_bits.CASES)  # the model's own dropout rate (0.01) and 0.5, where the moved mask carries weight
ALL = 3  # every part: the default


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
def _digests(case: str, fill: int = ALL, prog: int = 3, fmax: int = -1, loopback: int = 0, launches=(3, 2)) -> dict:
    """Per-tensor digests of the plan `launches`; fmax < 0: HOPSX_PERSIST_FILL_MAX not set.  Computed once per
    setting and shared (the default is every test's reference)."""
    kv = {"HOPSX_PERSIST_FILL": fill, "HOPSX_PERSIST_PROG": prog}
    if fmax >= 0:
        kv["HOPSX_PERSIST_FILL_MAX"] = fmax
    old = persist_bits.LAUNCHES
    persist_bits.LAUNCHES = tuple(launches)
    try:
        with _knobs(**kv):
            return persist_bits.digests(persist_bits.CASES[case], loopback=loopback, per_tensor=True)
    finally:
        persist_bits.LAUNCHES = old


def _differing(got: dict, want: dict) -> list:
    assert set(got) == set(want)
    return sorted(k for k in want if got[k] != want[k])


def test_knob_geometry():
    """The chunks divide the 32 lane-owned updates, and the cap's range fits its four bits of the hand word."""
    n = persist.geometry()["fill_chunks"]
    assert 1 <= n <= 15 and 32 % n == 0


@pytest.mark.parametrize("prog", [3, 0], ids=["progressive", "flag_form"])
@pytest.mark.parametrize("case", CASES)
def test_default_keeps_parent_bits(case, prog):
    """Every part on (the default), both forms of C: tensor by tensor the parent build's bytes."""
    assert GOLDEN_TENSORS["launches"] == [3, 2]
    bad = _differing(_digests(case, ALL, prog), GOLDEN_TENSORS["digests"]["w1"][case])
    print(case, prog, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_default_keeps_parent_arena_bits(case):
    """The same run against the whole-arena digests of the parent (persist_parent_bits.json)."""
    with _knobs(HOPSX_PERSIST_FILL=ALL):
        got = persist_bits.digests(persist_bits.CASES[case])
    want = GOLDEN["digests"][case]
    bad = sorted(k for k in want if got.get(k) != want[k])
    print(case, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("prog", [3, 0], ids=["progressive", "flag_form"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fill", [0, 1, 2], ids=["none", "fc1_in_c_wait", "mask_in_b_wait"])
def test_each_part_alone_equals_default(fill, case, prog):
    """No part, and each single part, against every part: all arena words, every step's loss and correct count."""
    bad = _differing(_digests(case, fill, prog), _digests(case, ALL, prog))
    print(fill, case, prog, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fmax", ["none", "one", "all"])
def test_fill_max_forces_the_split(fmax, case):
    """Chunks inside the C wait capped at 0 (all left over: the old placement through the new path), at 1 (most
    left over) and at the chunk count (none left over when the wait is long enough): every chunk runs once."""
    n = {"none": 0, "one": 1, "all": persist.geometry()["fill_chunks"]}[fmax]
    bad = _differing(_digests(case, ALL, 3, n), _digests(case, ALL, 3))
    print(fmax, case, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_launch_of_one_step_then_two(case):
    """A launch of ONE step (no next step: no mask is drawn in its B wait, and the state it writes back carries
    whatever chunks ran inside the wait) and one of two, against the unfilled schedule of the same plan."""
    got = _digests(case, ALL, 3, launches=(1, 2))
    bad = _differing(got, _digests(case, 0, 3, launches=(1, 2)))
    print(case, "differing:", bad)
    assert not bad, bad
    assert got["out"] != _digests(case, ALL, 3)["out"]  # (3 steps' outputs, not 5: the plan was really the other one)


@pytest.mark.parametrize("case", CASES)
def test_loopback2_equals_default_and_parent(case):
    """The data-parallel instantiation playing two ranks in-process: it keeps its own placement of the fc1 update
    and shares the moved mask draw."""
    dflt = _digests(case, ALL, 3, loopback=2)
    bad = _differing(_digests(case, 0, 3, loopback=2), dflt)
    print(case, "none vs default, differing:", bad)
    assert not bad, bad
    bad = _differing(dflt, GOLDEN_TENSORS["digests"]["loopback2"][case])
    print(case, "default vs parent, differing:", bad)
    assert not bad, bad
