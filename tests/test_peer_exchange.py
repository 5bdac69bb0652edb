"""runtime/peer_exchange.py PeerExchange — the cross-rank exchange setup of the whole-step kernels — against a
recording fake of the P2P extension (alloc / open / close / free) and a scripted ``all_gather_object``."""
import pytest
import torch

from hops_examples_amd.parallel import dist as hdist
from hops_examples_amd.parallel import oneshot
from hops_examples_amd.runtime.peer_exchange import PeerExchange


class FakeExt:
    """Hands out addresses 0x1000, 0x2000, ...; a handle is the address in 8 bytes.  ``fail_alloc``: the
    number of the ``alloc`` call that raises."""

    def __init__(self, fail_alloc=None):
        self.log = []
        self.n = 0
        self.fail_alloc = fail_alloc
        self.allocs = 0

    def _addr(self):
        self.n += 1
        return 0x1000 * self.n

    def alloc(self, nbytes, uncached):
        self.allocs += 1
        if self.allocs == self.fail_alloc:
            raise RuntimeError("out of memory")
        p = self._addr()
        self.log.append(("alloc", p, nbytes, uncached))
        return p, p.to_bytes(8, "little")

    def open(self, handle):
        p = self._addr()
        self.log.append(("open", p, bytes(handle)))
        return p

    def close(self, p):
        self.log.append(("close", p))

    def free(self, p):
        self.log.append(("free", p))

    def ops(self, *names):
        return [e for e in self.log if e[0] in names]


@pytest.fixture
def fake(monkeypatch):
    ext = FakeExt()
    monkeypatch.setattr(oneshot, "ext", lambda: ext)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: ext.log.append(("sync",)))
    return ext


def _script_gathers(monkeypatch, *peers):
    """all_gather_object: this rank's object at its own rank (0), the scripted peer's at rank 1; one scripted
    answer per call.  Returns the list of what this rank sent."""
    sent, answers = [], list(peers)

    def gather(out, obj):
        sent.append(obj)
        out[0], out[1] = obj, answers.pop(0)

    monkeypatch.setattr(torch.distributed, "all_gather_object", gather)
    return sent


def test_loopback_three_ranks_are_the_own_buffers(fake):
    px = PeerExchange("cpu", 4096, 64, 3, 0, loopback=True, name="taxi")
    (_, buf, nb, unc), (_, flg, nf, _) = fake.ops("alloc")
    assert (nb, nf, unc) == (4096, 64 * 4, True)
    assert px.bufs == [buf] * 3 and px.flags == [flg] * 3
    assert not fake.ops("open")
    px.close()
    assert fake.log[-3:] == [("sync",), ("free", buf), ("free", flg)]
    n = len(fake.log)
    px.close()
    assert len(fake.log) == n


def test_two_ranks_open_the_peers_handles_once_and_close_before_free(fake, monkeypatch):
    sent = _script_gathers(monkeypatch, (1, b"peer-buf", b"peer-flg", None), None)
    px = PeerExchange("cpu", 4096, 64, 2, 0, name="taxi")
    buf, flg = [e[1] for e in fake.ops("alloc")]
    assert sent == [(0, buf.to_bytes(8, "little"), flg.to_bytes(8, "little"), None), None]
    opens = fake.ops("open")
    assert [e[2] for e in opens] == [b"peer-buf", b"peer-flg"]
    assert px.bufs == [buf, opens[0][1]] and px.flags == [flg, opens[1][1]]
    px.close()
    assert fake.log[-5:] == [("sync",), ("close", opens[0][1]), ("close", opens[1][1]), ("free", buf), ("free", flg)]


def test_a_peers_allocation_error_is_raised_on_this_rank(fake, monkeypatch):
    _script_gathers(monkeypatch, (1, None, None, "RuntimeError('out of memory')"))
    with pytest.raises(RuntimeError, match=r"persistent DP exchange setup failed on ranks \[\(1, .*out of memory"):
        PeerExchange("cpu", 4096, 64, 2, 0, name="persistent")
    buf, flg = [e[1] for e in fake.ops("alloc")]
    assert fake.ops("free") == [("free", buf), ("free", flg)] and not fake.ops("open")


def test_an_own_flag_page_failure_travels_in_the_gather(fake, monkeypatch):
    fake.fail_alloc = 2
    sent = _script_gathers(monkeypatch, (1, b"peer-buf", b"peer-flg", None))
    with pytest.raises(RuntimeError, match=r"taxi DP exchange setup failed on ranks \[\(0, .*out of memory"):
        PeerExchange("cpu", 4096, 64, 2, 0, name="taxi")
    assert sent[0][:3] == (0, None, None) and "out of memory" in sent[0][3]
    (_, buf, _, _), = fake.ops("alloc")
    assert fake.ops("free") == [("free", buf)] and not fake.ops("open")


def test_a_mapping_failure_is_agreed_in_the_second_gather(fake, monkeypatch):
    _script_gathers(monkeypatch, (1, b"peer-buf", b"peer-flg", None), "RuntimeError('no peer access')")
    with pytest.raises(RuntimeError, match="taxi DP: mapping a peer's exchange buffer failed.*no peer access"):
        PeerExchange("cpu", 4096, 64, 2, 0, name="taxi")
    assert len(fake.ops("close")) == 2 and len(fake.ops("free")) == 2


def test_registered_for_ordered_teardown(fake):
    px = PeerExchange("cpu", 4096, 64, 2, 0, loopback=True)
    assert any(order == hdist.ORDER_COMM and ref() is px for order, ref in hdist._RESOURCES)
    px.close()
