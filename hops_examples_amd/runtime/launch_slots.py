"""Launch-argument slots of the whole-step kernels: the Python half of bindings.cpp's ``def_arg_slots``.

A whole-step launch takes three argument vectors.  Converting them on every launch would put that host work
inside the timed window while the GPU waits, so the extension keeps converted argument sets in numbered slots
(``<name>_store(slot, ...) -> slot``; ``<name>_slot(slot, stream)`` launches one).  ``ArgSlots`` keeps which
launch key lives in which slot: a run has a few launch shapes (warm-up, steps per launch, the remainder), so
a small capacity with oldest-first eviction is enough."""
from __future__ import annotations

from typing import Callable, Hashable, Optional


def launch_shapes(n: int, per_launch: int) -> set:
    """The step counts of the launches that run ``n`` steps at ``per_launch`` steps a launch: the full
    launch (or ``n`` itself when smaller) and the remainder."""
    return {min(n, per_launch), n % per_launch} - {0}


class ArgSlots:
    """key -> slot id of ``store``.  ``store(slot, *args) -> slot`` writes an argument set into ``slot``, or
    into a new slot when ``slot`` is -1."""

    def __init__(self, store: Callable[..., int], capacity: int = 8,
                 on_evict: Optional[Callable[[Hashable], None]] = None):
        self._store = store
        self.capacity = int(capacity)
        self.on_evict = on_evict
        self._ids: dict = {}  # insertion order = age

    def get(self, key: Hashable, build: Callable[[], tuple]) -> int:
        """The slot id of ``key``.  On a miss ``build()`` gives the arguments to store; when full, the oldest
        key is evicted (``on_evict(key)``) and its slot id reused."""
        sid = self._ids.get(key)
        if sid is None:
            free = -1
            if len(self._ids) >= self.capacity:
                old = next(iter(self._ids))
                free = self._ids.pop(old)
                if self.on_evict is not None:
                    self.on_evict(old)
            sid = self._store(free, *build())
            self._ids[key] = sid
        return sid

    def __len__(self) -> int:
        return len(self._ids)
