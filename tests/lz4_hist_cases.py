"""Inputs for the tests of the LZ4 HC encoder with history (TEST INFRASTRUCTURE, shared by test_wavesim_lz4_hist.py and
test_gpu_lz4_hist.py): ONE batch in one input buffer, every block with the bytes the caller put in front of it.  A block's history is
whatever lies below it in the buffer -- a dictionary placed there, or the block before it (a linked chain)."""
import numpy as np

from rust_compress_amd import synth

HISTS = (0, 1, 3, 4, 5, 4096, 65535, 65536)
LENS = (0, 1, 11, 12, 13, 64, 1000, 65536, 65537 + 300)      # the last: two segments, of which only the first sees the history
LEVELS = (1, 9, 12)
E_OUTPUT_TOO_SMALL = 2


def bound(n):
    return n + n // 255 + 20


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Batch:
    """names, in_off, lens, hist_len (as the caller passes it: 65536 allowed), caps and the buffer"""

    def __init__(self):
        self.buf = bytearray()
        self.names, self.in_off, self.lens, self.hist_len, self.caps = [], [], [], [], []

    def add(self, name, hist, block, front=b"", cap=None):
        """`front`, then the history, then the block"""
        self.buf += front + hist
        self._block(name, block, len(hist), cap)

    def add_chain(self, name, data, size):
        """`data` as linked blocks of `size` bytes: every block's history is all of the chain in front of it, at most 65536 bytes"""
        self.buf += b"\x3C"
        start = len(self.buf)
        for k, at in enumerate(range(0, len(data), size)):
            assert len(self.buf) == start + at
            self._block("%s[%d]" % (name, k), data[at:at + size], min(at, 65536))

    def _block(self, name, block, hist, cap=None):
        self.names.append(name)
        self.in_off.append(len(self.buf))
        self.lens.append(len(block))
        self.hist_len.append(hist)
        self.caps.append(bound(len(block)) if cap is None else cap)
        self.buf += block

    def array(self):
        return np.frombuffer(bytes(self.buf) + b"\0" * 16, np.uint8).copy()

    def index(self, name):
        return self.names.index(name)

    def block(self, i):
        return bytes(self.buf[self.in_off[i]:self.in_off[i] + self.lens[i]])

    def history(self, i):
        """the history the encoder may use: at most 65535 bytes"""
        h = min(self.hist_len[i], 65535)
        return bytes(self.buf[self.in_off[i] - h:self.in_off[i]])


_batch = None


def batch():
    global _batch
    if _batch is not None:
        return _batch
    B = Batch()
    # every history length with every block length, in text; leads of 1, 2 and 3 bytes: unaligned 4-byte loads at the history's start
    k = 0
    for h in HISTS:
        for n in LENS:
            t = synth.gen("text", h + n, 100 + k).tobytes()
            B.add("h%d n%d" % (h, n), t[:h], t[h:], front=b"\xC3" * (1 + k % 3))
            k += 1
    # a block that is a verbatim slice of a random history: from its first byte (distance exactly 65535 at position 0), from its last
    # bytes; without the history the block is incompressible
    r = rand(65535, 7)
    B.add("slice first", r, r[:1000], front=b"\xC3\xC3")
    B.add("slice last", r, r[-1000:], front=b"\xC3")
    # a source that runs over the boundary between history and block, at distance 1
    B.add("run", b"a" * 7, b"a" * 200, front=b"\xC3\xC3\xC3")
    # bait: the history holds the block's first half; the bytes in front of the history hold (bait x) or do not hold (bait y) the
    # whole block -- a match an out-of-bounds read would find and prefer.  Both must give the same bytes
    x = rand(1000, 8)
    short = x[:500] + rand(1500, 9)
    B.add("bait x", short, x, front=b"\xC3" + x)
    B.add("bait y", short, x, front=b"\xC3" + rand(1000, 10))
    # a chain of linked blocks whose histories overlap each other's inputs
    B.add_chain("chain", synth.gen("text", 15000, 77).tobytes(), 3000)
    # a slot too small for its block's bound, between good ones
    t = synth.gen("text", 6000, 78).tobytes()
    B.add("small slot", t[:3000], t[3000:], front=b"\xC3", cap=bound(3000) - 1)
    B.add("after small slot", t[:3000], t[3000:], front=b"\xC3\xC3")
    _batch = B
    return B
