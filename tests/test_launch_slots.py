"""runtime/launch_slots.py ArgSlots — the key -> argument-slot cache of the whole-step launches — against a
fake store that hands out consecutive ids (what the extension's <name>_store does for slot -1)."""
import pytest

from hops_examples_amd.runtime.launch_slots import ArgSlots, launch_shapes


class FakeStore:
    def __init__(self):
        self.calls = []  # (slot asked for, args)
        self.n = 0

    def __call__(self, slot, *args):
        self.calls.append((slot, args))
        if slot < 0:
            slot = self.n
            self.n += 1
        return slot


def _no_build():
    raise AssertionError("build() called on a hit")


def test_hit_returns_the_same_id_without_building():
    store = FakeStore()
    s = ArgSlots(store)
    a = s.get("a", lambda: ([1], [2], [3.0]))
    b = s.get("b", lambda: ([4], [5], [6.0]))
    assert (a, b) == (0, 1) and len(s) == 2
    assert store.calls == [(-1, ([1], [2], [3.0])), (-1, ([4], [5], [6.0]))]
    assert s.get("a", _no_build) == a and s.get("b", _no_build) == b
    assert len(store.calls) == 2 and len(s) == 2


def test_ninth_key_evicts_the_first_and_reuses_its_id():
    store, evicted = FakeStore(), []
    s = ArgSlots(store, on_evict=evicted.append)
    ids = [s.get(k, lambda k=k: ([k],)) for k in range(8)]
    assert ids == list(range(8)) and len(s) == 8 and evicted == []
    assert s.get(8, lambda: ([8],)) == ids[0]  # the oldest key's id, handed to the store for reuse
    assert store.calls[-1] == (ids[0], ([8],))
    assert evicted == [0] and len(s) == 8
    # the evicted key is a miss again (and evicts the next oldest); the survivors are still hits
    assert s.get(7, _no_build) == 7
    assert s.get(0, lambda: ([0],)) == ids[1] and evicted == [0, 1] and len(s) == 8


def test_capacity_is_a_parameter_and_on_evict_optional():
    store = FakeStore()
    s = ArgSlots(store, capacity=2)
    assert [s.get(k, lambda: ()) for k in "abc"] == [0, 1, 0] and len(s) == 2
    assert s.get("b", _no_build) == 1


@pytest.mark.parametrize("n,U,want", [(20, 8, {8, 4}), (8, 8, {8}), (3, 8, {3}), (16, 8, {8}), (0, 8, set())])
def test_launch_shapes(n, U, want):
    """n steps at U per launch: the full launch (or n, when smaller) and the remainder, never 0."""
    assert launch_shapes(n, U) == want
