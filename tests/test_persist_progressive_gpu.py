"""The progressive fan-in of the persistent flagship step (csrc/ops/mnist_persist.hip ``gather_rows``:
hand-off C, the 169 conv-gradient partials -> each slice owner) against the flag form it replaces.

The progressive form loads the same rows into the same registers and sums them in the same fixed order;
only WHEN a row is loaded changes (as soon as its own flag is there, not after the last flag).  So a run
with ``HOPSX_PERSIST_PROG=3`` must equal a run with ``HOPSX_PERSIST_PROG=0`` in every word of the
parameters, both Adadelta states, every per-step loss, every correct count and the cursor; one row
loaded before its flag, or taken from the launch before, changes those bits.  Launch lengths 1, 2, 4
restart the step parity inside a slab that still holds an earlier launch's rows and flags; a 32-step
launch is the benchmark's shape.

The knob's bit 1 is C.  Bit 0 was the same form for hand-off A (the 169 fc1 partial rows -> each head),
which measured slower and is not in the tree (profiles/r9_persist_progressive.txt): the wrapper ignores
it, so 1 runs what 0 runs and 3 what 2 runs.  The cases stay: every value of the knob must give the flag
form's bits.

Reference workload: notebooks/ml/Distributed_Training/mirrored_strategy/
mirroredstrategy_mnist_example.ipynb:189-222.
"""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd import optim  # noqa: E402
from hops_examples_amd.models.mnist import MirroredMnistCNN  # noqa: E402
from hops_examples_amd.runtime import persist  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402

B = 32


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


def _setup(seed=0, nb=5, spl=32, loopback=0):
    """32 images, 5 resident batches (as tests/test_persist_tagged_gpu.py builds it)."""
    from hops_examples_amd.ops import functional as HF

    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    HF.seed_device_rng(11, dev)
    m = MirroredMnistCNN().to(dev)
    m.pool.salt = 7919
    ParamArena.from_module(m, dev)
    opt = optim.Adadelta(m, lr=1.0)
    g = torch.Generator().manual_seed(seed + 7)
    xs = torch.randint(0, 256, (nb, B, 28, 28, 1), dtype=torch.uint8, generator=g).to(dev)
    ys = torch.randint(0, 10, (nb, B), dtype=torch.int64, generator=g).to(dev)
    eng = persist.PersistentMnistStep(m, opt, steps_per_launch=spl, loopback=loopback)
    return eng, xs, ys


def _launches(eng, xs, ys, plan):
    """One launch per entry of ``plan``; returns [steps, 2] (loss, correct) of every step."""
    out = []
    for k in plan:
        eng.run_resident(xs, ys, k)
        torch.cuda.synchronize()
        eng.check()
        out.append(eng.losses(k).clone())
    return torch.cat(out)


def _state(eng):
    """Every parameter (fp32 master and the bf16 shadow) and both Adadelta states: the whole arena."""
    a = eng.arena
    return a.master.clone(), a.shadow.clone(), eng.s1.clone(), eng.s2.clone()


def _run(plan, seed=0, loopback=0, spl=32, **knobs):
    with _knobs(**knobs):
        eng, xs, ys = _setup(seed, spl=spl, loopback=loopback)
        try:
            out = _launches(eng, xs, ys, plan)
            return _state(eng), out, int(eng.cursor.item())
        finally:
            eng.close()


def _assert_same(r0, r1):
    (st0, out0, c0), (st1, out1, c1) = r0, r1
    assert c0 == c1
    assert torch.equal(out0, out1), (out0 - out1).abs().max()
    for x, y in zip(st0, st1):
        assert torch.equal(x, y)


SHORT = [1, 2, 4]  # 7 steps: odd launch lengths, so a launch starts on the parity the last one ended on
FULL = SHORT + [32]

_cache = {}


def _old(plan):
    """The flag form's result of ``plan`` (computed once, shared, never modified)."""
    key = tuple(plan)
    if key not in _cache:
        _cache[key] = _run(plan, HOPSX_PERSIST_PROG=0)
    return _cache[key]


def test_progressive_equals_flag_form_every_word():
    old = _old(FULL)
    assert old[1].shape == (7 + 32, 2)
    assert old[2] == (7 + 32) % 5
    _assert_same(old, _run(FULL, HOPSX_PERSIST_PROG=3))


@pytest.mark.parametrize("prog", [1, 2])
def test_each_part_alone_equals_flag_form(prog):
    """Each bit alone: 2 is C progressive, 1 (A's bit, ignored) the flag form."""
    _assert_same(_old(SHORT), _run(SHORT, HOPSX_PERSIST_PROG=prog))


@pytest.mark.parametrize("head1w", [0, 1])
def test_progressive_equals_flag_form_both_head_forms(head1w):
    old = _run(SHORT, HOPSX_PERSIST_PROG=0, HOPSX_PERSIST_HEAD1W=head1w)
    new = _run(SHORT, HOPSX_PERSIST_PROG=3, HOPSX_PERSIST_HEAD1W=head1w)
    _assert_same(old, new)


def test_progressive_equals_flag_form_data_parallel():
    """The DP instantiation (two loopback ranks, 6 steps as launches of 4 and 2), and the existing
    invariant that two loopback ranks are bit-identical to one."""
    plan = [4, 2]
    old = _run(plan, seed=1, loopback=2, spl=4, HOPSX_PERSIST_PROG=0)
    new = _run(plan, seed=1, loopback=2, spl=4, HOPSX_PERSIST_PROG=3)
    _assert_same(old, new)
    one = _run(plan, seed=1, loopback=0, spl=4, HOPSX_PERSIST_PROG=3)
    _assert_same(one, new)


def test_prog_0_is_the_flag_form():
    """The knob routes: with HOPSX_PERSIST_PROG=0 the owners' wait is the multi-wave flag poll, so its wave
    count (HOPSX_PERSIST_POLLW_C, 4 by default) still selects another path through wait_all, and the results
    stay equal (a sanity check only)."""
    _assert_same(_old(SHORT), _run(SHORT, HOPSX_PERSIST_PROG=0, HOPSX_PERSIST_POLLW_C=1))


def test_check_raises_and_clears_then_runs_clean():
    """The failure path without a failing launch: the error word is set by hand on an idle engine (the code
    a C wait would record: phase 3), flags and tags are filled with 1 (the epoch of a fresh engine's first
    step, so an uncleared flag would let the progressive form load a row that was never written).  check()
    must raise and clear; a following 3-step launch must equal a fresh engine's."""
    ref = _run([3], HOPSX_PERSIST_PROG=3)
    with _knobs(HOPSX_PERSIST_PROG=3):
        eng, xs, ys = _setup()
        try:
            g = eng.geom
            eng.tags.fill_(1)
            eng.flags[: g["flag_words"] - 2].fill_(1)  # (not the 64-bit epoch base behind the flag rows)
            eng.err.fill_(0x83001005 - (1 << 32))
            with pytest.raises(persist.PersistentError):
                eng.check()
            assert not bool(eng.flags.any()) and not bool(eng.tags.any())
            eng.err.zero_()
            out = _launches(eng, xs, ys, [3])
            _assert_same(ref, (_state(eng), out, int(eng.cursor.item())))
        finally:
            eng.close()
