"""numpy fp32 emulation of the two 64-lane sums of csrc/ops/common.h, lane by lane, and the data both tests of
wave_sum_tree run on (tests/test_wave_sum_tree_cpu.py, tests/test_wave_sum_tree_gpu.py).

wave_sum:       six steps v[l] += v[l ^ o], o = 32, 16, 8, 4, 2, 1 (__shfl_xor).
wave_sum_tree:  the 32- and 16-steps as half / row swaps (the swapped lanes add with the operands exchanged), then
                DPP row rotations v[l] += v[row(l) + (l % 16 + R) % 16] for R = 8, 4, 2, 1.  After the 16-step a row's
                lanes hold values of period 16, after the 8-step of period 8, ...: the rotation by R reads the same
                operand as xor R, so every lane holds the same bits as in wave_sum.  In the ascending order
                1, 2, 4, 8 (common.h row_fold) the rotations pair other operands: the control that the tests can
                tell two trees apart."""
import numpy as np

LANE = np.arange(64)


def make_rows(n: int, seed: int = 18) -> np.ndarray:
    """[n][64] fp32: magnitudes 2^-29 .. 2^29 of either sign, with zeros, -0, denormals and, in every eighth row,
    infinities of ONE sign (so no sum is a NaN, whose payload no test should depend on)."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(1.0, 2.0, size=(n, 64)) * np.exp2(rng.integers(-29, 30, size=(n, 64)))).astype(np.float32)
    x *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(n, 64))
    kind = rng.integers(0, 16, size=(n, 64))
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    den = (rng.integers(1, 1 << 23, size=(n, 64)).astype(np.uint32) | (rng.integers(0, 2, size=(n, 64)).astype(np.uint32) << 31))
    x[kind == 2] = den.view(np.float32)[kind == 2]
    inf_rows = np.arange(n) % 8 == 7
    sign = np.where(np.arange(n) % 16 == 7, np.float32(-np.inf), np.float32(np.inf))
    m = (kind == 3) & inf_rows[:, None]
    x[m] = np.broadcast_to(sign[:, None], (n, 64))[m]
    assert not np.isnan(x).any()
    return x


def wave_sum(x: np.ndarray) -> np.ndarray:
    v = x.astype(np.float32).copy()
    with np.errstate(over="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, LANE ^ o]
    return v


def wave_sum_tree(x: np.ndarray, rot=(8, 4, 2, 1)) -> np.ndarray:
    v = x.astype(np.float32).copy()
    with np.errstate(over="ignore"):
        for o in (32, 16):
            other = v[:, LANE ^ o]
            # the lanes that received the partner's value in the first result add (partner + own)
            v = np.where((LANE & o) == 0, v + other, other + v)
        for r in rot:
            v = v + v[:, (LANE & 48) | ((LANE + r) & 15)]
    return v


def bits(v: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
