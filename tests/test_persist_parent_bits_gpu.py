"""The persistent flagship step (csrc/ops/mnist_persist.hip) against the bits of its parent build.

A change that only re-schedules the position workgroups' local compute (when LDS operands are read, how long
they are held) keeps every float operation's operands and order, so five steps from numpy-drawn inputs must
leave exactly the bytes the parent commit's build left: SHA-256 of the master / Adadelta arenas and of the
per-step (loss, correct) outputs, recorded on that build by tools/persist_bits.py --record into
tests/golden/persist_parent_bits.json (the file names the commit).  Two dropout rates: the model's own 0.01 and
0.5, where the keep mask carries weight."""
import json
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import persist_bits  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "persist_parent_bits.json").read_text())


@pytest.mark.parametrize("case", list(persist_bits.CASES))
def test_persistent_step_keeps_parent_bits(case):
    """5 steps as launches of 3 + 2: every arena byte and every step's loss / correct count as on the parent."""
    assert GOLDEN["launches"] == list(persist_bits.LAUNCHES)
    got = persist_bits.digests(persist_bits.CASES[case])
    want = GOLDEN["digests"][case]
    print(case, got)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
