"""The heads' A-to-B chain of the persistent flagship step (csrc/ops/mnist_persist.hip, head_wg), re-scheduled,
against the bits of the default schedule and of the parent build.

``HOPSX_PERSIST_GATE_A`` puts a gate in front of the heads' A wait: wave 0 of a head first watches ONE 128-byte line
of the A flag row at a slow cadence (1: head i line i % 6; 2: every head line 0; 0: no gate), for at most
``HOPSX_PERSIST_GATE_A_US`` microseconds, and only then runs the unchanged wait on every flag.
``HOPSX_PERSIST_HEAD_CHAIN`` re-places work of the one-wave head, one bit each: 1 its operands (fc1 bias, fc2 weight
columns, fc2 bias) are read into registers at the top of the step instead of inside the chain, 2 its ten logits are
summed by ``wave_sum_tree`` (common.h: the pairing tree of ``wave_sum`` without its LDS round trips; on its own in
tests/test_wave_sum_tree_gpu.py).

None of this changes a producer, a payload, a flag, an epoch, a granule or a float operation's operands or order,
so five steps from numpy-drawn inputs (tools/persist_bits.py) must leave every arena word (fp32 master, both
Adadelta accumulators, bf16 shadow; one SHA-256 per parameter tensor and arena) and every step's (loss, correct)
exactly as the default does, and the default as the parent commit's build did
(tests/golden/persist_parent_conv_bits.json, tests/golden/persist_parent_bits.json).  Equality of digests: no
tolerance.

Operands read before the previous step's fc2 update has finished and rotations in the ascending order change values,
hence digests (each was built once as a mutation and failed this file: profiles/r18_persist_head_chain.txt).
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
CASES = list(persist_bits.CASES)  # both dropout cases
WORLDS = {"w1": 0, "loopback2": 2}  # one process, and the data-parallel instantiation playing two ranks
PLANS = [(3, 2), (1, 2)]  # launches: the golden files' plan, and one whose first launch is step 0 alone
KNOBS = ("HOPSX_PERSIST_GATE_A", "HOPSX_PERSIST_GATE_A_US", "HOPSX_PERSIST_HEAD_CHAIN")
# (gate, bound in us): every gate setting with the default bound, and once with a bound of 0, where the gate gives way
# after one look, long before the flags are there
GATES = {"gate0": (0, None), "gate1": (1, None), "gate2": (2, None), "gate1_0us": (1, 0)}


@contextlib.contextmanager
def _knobs(**kv):
    """Launch knobs for the launches inside the block (the host wrapper caches them: reload); a knob given as None
    is unset, i.e. at its default."""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
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
def _digests(case: str, gate=None, gate_us=None, chain=None, loopback: int = 0, launches=(3, 2)) -> dict:
    """Per-tensor digests of the plan `launches`; None: the knob is not set.  Computed once per setting and shared
    (the default, every knob unset, is every test's reference)."""
    old = persist_bits.LAUNCHES
    persist_bits.LAUNCHES = tuple(launches)
    try:
        with _knobs(**dict(zip(KNOBS, (gate, gate_us, chain)))):
            return persist_bits.digests(persist_bits.CASES[case], loopback=loopback, per_tensor=True)
    finally:
        persist_bits.LAUNCHES = old


def _differing(got: dict, want: dict) -> list:
    assert set(got) == set(want)
    return sorted(k for k in want if got[k] != want[k])


@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
def test_default_keeps_parent_bits(case, world):
    """Every knob at its default: tensor by tensor the parent build's bytes, both instantiations."""
    assert GOLDEN_TENSORS["launches"] == [3, 2]
    bad = _differing(_digests(case, loopback=WORLDS[world], launches=PLANS[0]), GOLDEN_TENSORS["digests"][world][case])
    print(case, world, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_default_keeps_parent_arena_bits(case):
    """The same run against the whole-arena digests of the parent (persist_parent_bits.json)."""
    with _knobs(**dict.fromkeys(KNOBS)):
        got = persist_bits.digests(persist_bits.CASES[case])
    want = GOLDEN["digests"][case]
    bad = sorted(k for k in want if got.get(k) != want[k])
    print(case, "differing:", bad)
    assert not bad, bad


@pytest.mark.parametrize("plan", PLANS, ids=["3+2", "1+2"])
@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gate", list(GATES))
def test_gate_settings_equal_default(gate, case, world, plan):
    """No gate, either gate, and a gate giving way at once: all arena words, every step's loss and correct
    count, in both instantiations and with step 0 as a launch of its own."""
    g, us = GATES[gate]
    want = _digests(case, loopback=WORLDS[world], launches=plan)
    bad = _differing(_digests(case, g, us, loopback=WORLDS[world], launches=plan), want)
    print(gate, case, world, plan, "differing:", bad)
    assert not bad, bad
    if plan != PLANS[0]:  # (3 steps' outputs, not 5: the plan was really the other one)
        assert want["out"] != _digests(case, loopback=WORLDS[world], launches=PLANS[0])["out"]


@pytest.mark.parametrize("world", list(WORLDS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("chain", [0, 1, 2, 3], ids=["neither", "registers", "tree", "both"])
def test_head_chain_parts_equal_default(chain, case, world, plan=PLANS[0]):
    """The head's operands read inside the chain or at the top of the step, its logits by wave_sum or
    wave_sum_tree: the same bits.  (From step 1 on the operands are the ones the previous step's fc2 update wrote.)"""
    bad = _differing(_digests(case, chain=chain, loopback=WORLDS[world], launches=plan),
                     _digests(case, loopback=WORLDS[world], launches=plan))
    print(chain, case, world, plan, "differing:", bad)
    assert not bad, bad
