"""common.h wave_sum_tree against wave_sum on the GPU (the probe kernel in csrc/ops/mnist_persist.hip): 256 rows of 64
values spanning 2^-29 .. 2^29 with zeros, -0, denormals and infinities, no NaN (tools/wave_sum_tree_emu.py); every lane
of every row bit for bit.  The lane swaps and row rotations of the tree are only a re-spelling of the xor shuffles if
this holds; the emulation of both trees is compared in tests/test_wave_sum_tree_cpu.py."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd.ops import _C  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import wave_sum_tree_emu as emu  # noqa: E402

ROWS = 256


def test_probe_bits_equal():
    x = emu.make_rows(ROWS)
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x).to(dev)
    ref = torch.full_like(xd, float("nan"))
    tree = torch.full_like(xd, float("nan"))
    e = _C.ext().wave_sum_probe(xd.data_ptr(), ROWS, ref.data_ptr(), tree.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert e == 0, e
    torch.cuda.synchronize()
    r, t = emu.bits(ref.cpu().numpy()), emu.bits(tree.cpu().numpy())
    assert not np.isnan(ref.cpu().numpy()).any()
    bad = np.flatnonzero((r != t).any(axis=1))
    print("rows differing:", bad.size, "of", ROWS)
    assert bad.size == 0, bad[:8]
    assert (r == r[:, :1]).all()  # every lane of a row holds the row's sum
