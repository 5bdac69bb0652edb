"""The v2 taxi step's Python runtime (runtime/taxi_step.py) against the bits of its parent build.

A change to where the runtime lives and how it keys its launch slots and graphs hands the kernel
(csrc/ops/taxi_step.hip) the same arguments in the same order of launches, so twelve steps from numpy-drawn
inputs and weights must leave exactly the bytes the parent commit's build left: SHA-256 of the master, the
Adagrad and FTRL arenas and the loss, recorded on that build by tools/taxi_bits.py --record into
tests/golden/taxi_parent_bits.json (the file names the commit).  Three paths at B = 13, 4 batches: direct
launches of 8 + 4 steps, graph replays (HOPSX_TAXI_DIRECT=0) and the data-parallel instantiation with one
process playing two ranks.  No v1 case: its float atomics have no fixed order."""
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
import taxi_bits  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "taxi_parent_bits.json").read_text())


@pytest.mark.parametrize("case", list(taxi_bits.CASES))
def test_taxi_step_keeps_parent_bits(case):
    assert (GOLDEN["batch"], GOLDEN["nbatch"], GOLDEN["steps"]) == (taxi_bits.B, taxi_bits.NB, taxi_bits.STEPS)
    got = taxi_bits.digests(case)
    want = GOLDEN["digests"][case]
    print(case, got)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
