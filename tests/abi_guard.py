"""Guard-banded, poisoned device buffers for calling the C ABI (include/ge_hip.h) directly.

Every buffer an `Arena` hands out is ONE uint8 allocation laid out  guard | payload | guard :
  * both guards are GUARD (4096) bytes of 0xC3;
  * the payload starts 256-byte aligned and is EXACTLY the declared number of bytes -- the tail guard begins at byte
    `nbytes`, not at a rounded-up address, so a store one element past the end lands in it;
  * the payload is pre-filled with one byte (0x00 or 0xFF: the poison of outputs and workspaces) or with data.
Tables that an entry point updates in place are allocated the same way, so a write to row -1 or row N shows.

`Arena.call` goes straight through `_lib` with the argument order the wrappers use, on torch's current stream, and
returns the status code instead of raising.  `Arena.damage()` lists, per buffer and side, the first damaged guard offset
and the number of damaged bytes; `Arena.assert_intact()` names the buffer and the entry point.

What this design does NOT see: a stray write that lands more than 4 KiB away from the buffer it belongs to (it falls
outside both guards), a stray write that happens to store 0xC3, and any out-of-bounds READ.

Needs only torch and graphembeddings_amd._lib.
"""
import numpy as np
import torch

from graphembeddings_amd import _lib

GUARD = 4096
GUARD_BYTE = 0xC3
ALIGN = 256


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """One guarded buffer: `ptr` is the payload's device address, `nbytes` its exact size."""

    def __init__(self, name: str, nbytes: int, kind: str, shift: int = 0):
        """shift: bytes past the 256-byte boundary at which the payload starts (0 except for misaligned-table cases)."""
        self.name, self.nbytes, self.kind = name, int(nbytes), kind
        self.raw = torch.empty(GUARD + self.nbytes + GUARD + ALIGN - 1 + shift, dtype=torch.uint8, device="cuda")
        self.raw.fill_(GUARD_BYTE)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % ALIGN + shift
        self.ptr = self.raw.data_ptr() + self.off
        assert self.ptr % ALIGN == shift

    @property
    def payload(self) -> torch.Tensor:
        return self.raw[self.off:self.off + self.nbytes]

    def fill(self, byte: int) -> None:
        self.payload.fill_(int(byte))

    def put(self, array) -> None:
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.nbytes, (self.name, a.nbytes, self.nbytes)
        if a.nbytes:
            self.payload.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda())

    def get(self, dtype, shape=(-1,)) -> np.ndarray:
        """The payload as a host array of `dtype`."""
        return self.payload.cpu().numpy().copy().view(dtype).reshape(shape)

    def all_bytes_are(self, byte: int) -> bool:
        return self.nbytes == 0 or bool((self.payload == int(byte)).all())

    def guards(self):
        return (("head", self.raw[self.off - GUARD:self.off]),
                ("tail", self.raw[self.off + self.nbytes:self.off + self.nbytes + GUARD]))


class Arena:
    """The buffers of one ABI call.  kinds: "in" (data the call only reads), "out" (poisoned output), "ws" (poisoned
    workspace), "table" (data updated in place)."""

    def __init__(self, entry: str, poison: int = 0x00):
        self.entry, self.poison, self.bufs = entry, int(poison), []
        self.called = set()

    def __getitem__(self, name: str) -> Buf:
        for b in self.bufs:
            if b.name == name:
                return b
        raise KeyError(name)

    def _new(self, name, nbytes, kind, shift=0) -> Buf:
        b = Buf(name, nbytes, kind, shift)
        self.bufs.append(b)
        return b

    def data(self, name: str, array, kind: str = "in", shift: int = 0) -> Buf:
        a = np.ascontiguousarray(array)
        b = self._new(name, a.nbytes, kind, shift)
        b.put(a)
        return b

    def table(self, name: str, array) -> Buf:
        return self.data(name, array, kind="table")

    def out(self, name: str, nbytes: int) -> Buf:
        b = self._new(name, nbytes, "out")
        b.fill(self.poison)
        return b

    def ws(self, name: str, nbytes: int) -> Buf:
        b = self._new(name, nbytes, "ws")
        b.fill(self.poison)
        return b

    def call(self, name: str, *args) -> int:
        """The entry point's status code (0 = ok); arguments as the ctypes prototypes of _lib.SYMBOLS take them."""
        self.entry = name
        self.called.add(name)
        return int(getattr(_lib.load(), name)(*args))

    def damage(self):
        """[(buffer name, side, first damaged offset within the guard, damaged byte count)] after a synchronize."""
        torch.cuda.synchronize()
        found = []
        for b in self.bufs:
            for side, g in b.guards():
                bad = g != GUARD_BYTE
                n = int(bad.sum())
                if n:
                    first = int(torch.nonzero(bad)[0])
                    found.append((b.name, side, first if side == "tail" else first - GUARD, n))
        return found

    def assert_intact(self, what: str = "") -> None:
        dmg = self.damage()
        assert not dmg, "%s %s wrote outside its buffers: %s" % (
            self.entry, what, "; ".join("%s %s guard: %d bytes damaged, first at payload offset %s%d"
                                        % (n, s, c, "end+" if s == "tail" else "", o) for n, s, o, c in dmg))

    def outputs(self):
        """{name: payload bytes} of every output and every table updated in place (workspaces are scratch)."""
        torch.cuda.synchronize()
        return {b.name: b.payload.cpu().numpy().copy() for b in self.bufs if b.kind in ("out", "table")}

    def assert_outputs_poison(self, what: str = "") -> None:
        torch.cuda.synchronize()
        for b in self.bufs:
            if b.kind in ("out", "ws"):
                assert b.all_bytes_are(self.poison), "%s %s: refused call touched %s" % (self.entry, what, b.name)


def assert_bitwise_equal(entry: str, a: dict, b: dict) -> None:
    """(c): the outputs of the 0x00-poisoned and the 0xFF-poisoned run."""
    assert a.keys() == b.keys()
    for name in a:
        if not np.array_equal(a[name], b[name]):
            first = int(np.nonzero(a[name] != b[name])[0][0])
            raise AssertionError("%s: %s depends on what the outputs / workspace held before the call "
                                 "(first differing byte %d of %d)" % (entry, name, first, a[name].size))
