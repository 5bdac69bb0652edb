"""common.h wave_sum_tree pairs the 64 lanes exactly as wave_sum does: a numpy fp32 emulation of both trees, lane by
lane (tools/wave_sum_tree_emu.py), on 20,000 rows spanning 2^-29 .. 2^29 with zeros, -0, denormals and infinities.
Every lane of every row must hold the same bits; the rotations in the ascending order 1, 2, 4, 8 must NOT (the
control: the data can tell two pairing trees apart).  The kernel's own instructions are compared on the GPU in
tests/test_wave_sum_tree_gpu.py."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import wave_sum_tree_emu as emu  # noqa: E402

N = 20000


def test_data_has_every_kind():
    x = emu.make_rows(N)
    a = np.abs(x[np.isfinite(x) & (x != 0)])
    assert a.max() >= 2.0 ** 28 and a.min() < 2.0 ** -126  # large values and denormals
    assert ((x == 0) & ~np.signbit(x)).any() and ((x == 0) & np.signbit(x)).any()
    assert np.isposinf(x).any() and np.isneginf(x).any() and not np.isnan(x).any()
    assert not np.isnan(emu.wave_sum(x)).any()


def test_tree_equals_wave_sum_in_every_lane():
    x = emu.make_rows(N)
    ref, tree = emu.bits(emu.wave_sum(x)), emu.bits(emu.wave_sum_tree(x))
    bad = np.flatnonzero((ref != tree).any(axis=1))
    print("rows differing:", bad.size)
    assert bad.size == 0, bad[:8]
    assert (ref == ref[:, :1]).all()  # (and every lane of a row holds the same sum)


def test_ascending_rotations_differ():
    x = emu.make_rows(N)
    ref, asc = emu.bits(emu.wave_sum(x)), emu.bits(emu.wave_sum_tree(x, rot=(1, 2, 4, 8)))
    n = int((ref != asc).any(axis=1).sum())
    print("rows differing in the ascending order:", n, "of", N)
    assert n >= 1
