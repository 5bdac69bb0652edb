"""PeerExchange: one rank's uncached exchange buffer and flag page, and every peer's mapped next to them.

The data-parallel whole-step kernels (csrc/ops/mnist_persist.hip, csrc/ops/taxi_step.hip) push into the peers'
buffers and raise flag words in the peers' pages inside the launch.  Both set up alike: allocate, exchange the
IPC handles over the default process group, map every peer's, and agree on any failure collectively, so that no
rank goes on alone into a launch that would wait for a peer that has already raised."""
from __future__ import annotations

import torch


class PeerExchange:
    """``bufs`` / ``flags``: device addresses of every rank's exchange buffer / flag page, in rank order (this
    rank's own at ``rank``).  ``loopback``: ONE process plays every rank; the peers' buffers are its own and
    there is no collective.  ``name`` heads the error messages ("persistent", "taxi").

    A rank whose allocation fails still takes part in the handle exchange, and one that cannot map a peer in the
    second gather: every rank then closes what it holds and raises ``RuntimeError`` naming the failing ranks."""

    def __init__(self, device, buf_bytes: int, flag_words: int, world: int, rank: int, loopback: bool = False,
                 name: str = "peer"):
        import torch.distributed as dist

        from ..parallel import dist as hdist
        from ..parallel import oneshot

        self.device = torch.device(device)
        self.bufs: list[int] = []
        self.flags: list[int] = []
        self._owned: list[int] = []
        self._opened: list[int] = []
        hdist.register(self)  # ordered teardown (close: local) at shutdown / interpreter exit
        C = oneshot.ext()
        err = None
        try:
            buf, hb = C.alloc(int(buf_bytes), True)
            self._owned.append(buf)
            flg, hf = C.alloc(int(flag_words) * 4, True)
            self._owned.append(flg)
        except Exception as e:  # every rank must learn of it before the handle exchange
            err, hb, hf = repr(e), None, None
        if loopback:
            if err:
                self.close()
                raise RuntimeError(f"{name} DP exchange setup failed: {err}")
            self.bufs, self.flags = [buf] * world, [flg] * world
            return
        objs = [None] * world
        dist.all_gather_object(objs, (rank, None if err else bytes(hb), None if err else bytes(hf), err))
        bad = [(o[0], o[3]) for o in objs if o[3]]
        if bad:
            self.close()
            raise RuntimeError(f"{name} DP exchange setup failed on ranks {bad}")
        bufs, flags = [0] * world, [0] * world
        try:
            for r, b, f, _ in objs:
                if r == rank:
                    bufs[r], flags[r] = buf, flg
                else:
                    bufs[r] = C.open(b)
                    self._opened.append(bufs[r])
                    flags[r] = C.open(f)
                    self._opened.append(flags[r])
        except Exception as e:
            err = repr(e)
        oks = [None] * world
        dist.all_gather_object(oks, err)
        if any(oks):
            self.close()
            raise RuntimeError(f"{name} DP: mapping a peer's exchange buffer failed: {oks}")
        self.bufs, self.flags = bufs, flags

    def close(self) -> None:
        """Unmap the peers' buffers, free this rank's (on every rank, after the last launch has finished)."""
        if not self._owned and not self._opened:
            return
        from ..parallel import oneshot

        C = oneshot.ext()
        torch.cuda.synchronize(self.device)
        for p in self._opened:
            C.close(p)
        for p in self._owned:
            C.free(p)
        self._opened, self._owned, self.bufs, self.flags = [], [], [], []
