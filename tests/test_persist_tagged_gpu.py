"""The tagged hand-off of the persistent flagship step (csrc/ops/mnist_persist.hip "tagged granules":
hop B, dh of the 32 images, heads -> positions) against the flag form it replaces.

The tagged form moves the same bits by another route: the head rounds dh to bf16 with the conversion
the positions used.  So a run with ``HOPSX_PERSIST_TAGGED=1`` must equal a run with
``HOPSX_PERSIST_TAGGED=0`` in every word of the parameters, both Adadelta states, every per-step loss
and every correct count; one stale or torn dh pair changes those bits.  Launch lengths 1, 2, 4 restart
the step parity inside a slot that still holds an earlier launch's tags; 32-step launches are the
benchmark's shape.

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
    """32 images, 5 resident batches (as tests/test_persist_gpu.py builds it)."""
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


def test_tagged_equals_flag_form_every_word():
    plan = SHORT + [32, 32, 32]
    old = _run(plan, HOPSX_PERSIST_TAGGED=0)
    new = _run(plan, HOPSX_PERSIST_TAGGED=1)
    assert old[1].shape == (7 + 96, 2)
    _assert_same(old, new)


def test_tagged_equals_flag_form_data_parallel():
    """The DP instantiation (two loopback ranks, 6 steps as launches of 4 and 2), and the existing
    invariant that two loopback ranks are bit-identical to one."""
    plan = [4, 2]
    old = _run(plan, seed=1, loopback=2, spl=4, HOPSX_PERSIST_TAGGED=0)
    new = _run(plan, seed=1, loopback=2, spl=4, HOPSX_PERSIST_TAGGED=1)
    _assert_same(old, new)
    one = _run(plan, seed=1, loopback=0, spl=4, HOPSX_PERSIST_TAGGED=1)
    _assert_same(one, new)


@pytest.mark.parametrize("head1w", [0, 1])
def test_tagged_equals_flag_form_both_head_forms(head1w):
    old = _run(SHORT, HOPSX_PERSIST_TAGGED=0, HOPSX_PERSIST_HEAD1W=head1w)
    new = _run(SHORT, HOPSX_PERSIST_TAGGED=1, HOPSX_PERSIST_HEAD1W=head1w)
    _assert_same(old, new)


def test_check_clears_tags_with_the_flags():
    """A failed launch leaves tags behind without advancing the epoch base: check() must clear them with the
    flags.  No launch fails here: the tag slabs are filled with 1 (the epoch of a fresh engine's first
    step, so an uncleared granule would be taken for that step's data) and the error word is set by hand."""
    ref = _run([3])
    with _knobs(HOPSX_PERSIST_TAGGED=1):
        eng, xs, ys = _setup()
        g = eng.geom
        assert eng.tags.numel() == g["tag_words"] == 2 * 32 * 64 * 2  # [parity][image][granule] 8-byte granules
        eng.tags.fill_(1)
        eng.flags[: g["flag_words"] - 2].fill_(1)  # (not the 64-bit epoch base behind the flag rows)
        eng.err.fill_(0x82001005 - (1 << 32))
        with pytest.raises(persist.PersistentError):
            eng.check()
        assert not bool(eng.flags.any()) and not bool(eng.tags.any())
        eng.err.zero_()
        out = _launches(eng, xs, ys, [3])
        _assert_same(ref, (_state(eng), out, int(eng.cursor.item())))
