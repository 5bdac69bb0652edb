"""The persistent step's launch fast path (runtime/persist.py _launch) must not launch with stale arguments:
a launch on the same epoch tensors after a change of anything _build_args reads (here the hand-off timeout
and the dropout salt) stores a new argument set; a launch with nothing changed stores nothing.  And the
extension refuses a slot id it never handed out.  One batch, one step per launch: the smallest shape."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from hops_examples_amd import optim  # noqa: E402
from hops_examples_amd.models.mnist import MirroredMnistCNN  # noqa: E402
from hops_examples_amd.ops import _C  # noqa: E402
from hops_examples_amd.runtime import persist  # noqa: E402
from hops_examples_amd.runtime.arena import ParamArena  # noqa: E402

B = 32
HIP_ERROR_INVALID_VALUE = 1


def _engine():
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    m = MirroredMnistCNN().to(dev)
    ParamArena.from_module(m, dev)
    opt = optim.Adadelta(m, lr=1.0)
    g = torch.Generator().manual_seed(7)
    xs = torch.randint(0, 256, (1, B, 28, 28, 1), dtype=torch.uint8, generator=g).to(dev)
    ys = torch.randint(0, 10, (1, B), dtype=torch.int64, generator=g).to(dev)
    eng = persist.PersistentMnistStep(m, opt, steps_per_launch=1)
    stored = []  # the (ptrs, iv, fv) of every argument set the engine stores
    store = eng._slots._store

    def spy(slot, *args):
        stored.append(args)
        return store(slot, *args)

    eng._slots._store = spy
    return m, eng, xs, ys, stored


def _step(eng, xs, ys):
    eng.run_resident(xs, ys, 1)
    torch.cuda.synchronize()
    eng.check()


def test_a_changed_launch_argument_is_stored_not_served_stale():
    m, eng, xs, ys, stored = _engine()
    steps0 = float(eng.opt.step_count.item())
    _step(eng, xs, ys)
    assert len(eng._slots) == 1 and len(stored) == 1
    _step(eng, xs, ys)  # nothing changed: the fast path, nothing stored
    assert len(eng._slots) == 1 and len(stored) == 1

    eng.timeout_ms += 1000
    _step(eng, xs, ys)
    assert len(eng._slots) == 2 and len(stored) == 2
    assert stored[-1][1][-2] == eng.timeout_ms  # iv: [..., timeout_ms, xfence]

    m.pool.salt = int(m.pool.salt) + 1
    _step(eng, xs, ys)
    assert len(eng._slots) == 3 and len(stored) == 3
    assert stored[-1][1][len(eng.offs) + 1] == m.pool.salt  # iv: offs + [nbatch, salt, ...]
    assert stored[-1][1][-2] == eng.timeout_ms

    _step(eng, xs, ys)  # and again nothing changed
    assert len(eng._slots) == 3 and len(stored) == 3
    assert float(eng.opt.step_count.item()) == steps0 + 5  # every one of the five launches ran its step


def test_a_slot_id_out_of_range_is_refused_without_a_launch():
    m, eng, xs, ys, stored = _engine()
    _step(eng, xs, ys)
    before = float(eng.opt.step_count.item())  # the kernel advances it by the launch's steps
    for sid in (1 << 20, -1):
        assert persist._ext().mnist_persist_slot(sid, _C.stream()) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert float(eng.opt.step_count.item()) == before
