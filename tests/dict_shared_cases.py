"""Inputs for the tests of the encoders behind shared dictionaries (TEST INFRASTRUCTURE, shared by test_wavesim_dict_shared.py and
test_gpu_dict_shared.py).  A Batch holds dictionaries and blocks and lays them out twice: SHARED -- every dictionary once, anywhere in
the buffer, blocks naming it by offset and length -- and REPLICATED -- every block with its dictionary directly in front of it, what
the history encoders take (the oracle)."""
import numpy as np

from rust_compress_amd import synth

LEVELS = {"lz4": (1, 9, 12), "deflate": (2, 6, 9)}
MAX_DICT = {"lz4": 65536, "deflate": 32768}
REACH = {"lz4": 65535, "deflate": 32768}
DICTS = {"lz4": (0, 1, 3, 4, 5, 258, 4096, 32767, 32768, 65535, 65536), "deflate": (0, 1, 3, 4, 5, 258, 4096, 32767, 32768)}
LENS = (0, 1, 3, 4, 5, 258, 259, 1000, 65536, 65836)
SEG = 65536
E_OUTPUT_TOO_SMALL = 2


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed):
    return synth.gen("text", n, seed).tobytes()


def bound(family, n, fmt=0):
    if family == "lz4":
        return n + n // 255 + 20
    return n + 11 * ((n + SEG - 1) // SEG) + 2 + (10 if fmt else 0)


def pack(family, length, dist):
    """the candidate word of a match"""
    return length << 16 | (dist if family == "lz4" else dist - 1)


class Batch:
    def __init__(self, family):
        self.family = family
        # (data, front, behind, after, within): `front` + data + `behind` in the buffer, before or after the blocks; or within = (handle,
        # start): no bytes of its own, the range that starts `start` bytes into dictionary `handle` (and may run into its `behind`)
        self.dicts = []
        self.names, self.blocks, self.of, self.caps = [], [], [], []

    def dict(self, data, front=b"\xC3", behind=b"\x3C\x3C", after=False):
        self.dicts.append((data, front, behind, after, None))
        return len(self.dicts) - 1

    def dict_within(self, handle, start, length):
        """a dictionary that is a range of another one's bytes in the buffer: it overlaps dictionary `handle` and differs from it"""
        data, _, behind, after, within = self.dicts[handle]
        assert within is None and start + length <= len(data) + len(behind)
        self.dicts.append(((data + behind)[start:start + length], b"", b"", after, (handle, start)))
        return len(self.dicts) - 1

    def add(self, name, block, d=None, cap=None):
        """block behind dictionary d (a handle of dict(), or None)"""
        self.names.append(name)
        self.blocks.append(block)
        self.of.append(d)
        self.caps.append(cap)

    def index(self, name):
        return self.names.index(name)

    def dictionary(self, i):
        return self.dicts[self.of[i]][0] if self.of[i] is not None else b""

    def history(self, i):
        """what counts of block i's dictionary"""
        return self.dictionary(i)[-REACH[self.family]:]

    def out_caps(self, fmt=0):
        return [bound(self.family, len(b), fmt) if c is None else c for b, c in zip(self.blocks, self.caps)]

    def reordered(self, order):
        B = Batch(self.family)
        B.dicts = list(self.dicts)
        for i in order:
            B.add(self.names[i], self.blocks[i], self.of[i], self.caps[i])
        return B

    def shared(self):
        """-> (buffer, in_off, lens, dict_off, dict_len): dictionaries placed once, half of them in front of the blocks and half behind"""
        buf, at = bytearray(), {}
        for after in (False, True):
            if after:
                self._in_off = []
                for b in self.blocks:
                    buf += b"\x5A"
                    self._in_off.append(len(buf))
                    buf += b
            for j, (data, front, behind, aft, within) in enumerate(self.dicts):
                if aft == after and within is None:
                    buf += front
                    at[j] = len(buf)
                    buf += data + behind
        for j, d in enumerate(self.dicts):
            if d[4] is not None:
                at[j] = at[d[4][0]] + d[4][1]
        d_off = [at[d] if d is not None else 0 for d in self.of]
        d_len = [len(self.dicts[d][0]) if d is not None else 0 for d in self.of]
        return np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy(), list(self._in_off), [len(b) for b in self.blocks], d_off, d_len

    def replicated(self):
        """-> (blocks, hists, fronts): the history encoders' layout, for sim_*_hist_run.encode(blocks, hists, level, front=fronts)"""
        hists = [self.dictionary(i) or None for i in range(len(self.blocks))]
        fronts = [b"\xC3" * (1 + i % 3) for i in range(len(self.blocks))]
        return list(self.blocks), hists, fronts


_cache = {}


def cases(family):
    """the case batch: the length grid, the spanning prefixes, the run, the slices, the two bait pairs, a slot that is too small"""
    if ("cases", family) in _cache:
        return _cache[("cases", family)]
    B = Batch(family)
    k = 0
    for h in DICTS[family]:
        for n in LENS:
            t = text(h + n, 100 + k)
            d = B.dict(t[:h], front=b"\xC3" * (1 + k % 3), after=bool(k & 1)) if h else None
            B.add("h%d n%d" % (h, n), t[h:], d)
            k += 1
    # a dictionary that ends in the first k bytes of P: the 4-byte prefixes of its last three positions reach into the block
    for k in (1, 2, 3):
        P = rand(40, 20 + k)
        d = B.dict(rand(500, 30 + k) + P[:k], front=b"\xC3" * k, after=k == 2)
        B.add("span %d" % k, P[k:] + rand(100, 40 + k) + P + rand(20, 50 + k), d)
    B.add("run", b"a" * 200, B.dict(b"a" * 7, front=b"\xC3\xC3\xC3", behind=b"bb"))
    r = rand(MAX_DICT[family] if family == "deflate" else 65535, 7)
    B.add("slice first", r[:1000], B.dict(r, front=b"\xC3\xC3"))
    B.add("slice last", r[-1000:], B.dict(r, front=b"\xC3", after=True))
    # bait behind the dictionary's end: a match that starts in the dictionary and runs past its last byte goes on in the block's first
    # bytes (100 bytes at distance 100, then Y against the block's own start: a mismatch), not in what follows the dictionary
    A, Y = rand(1000, 60), rand(60, 61)
    blk = A[-100:] + Y + rand(20, 62)
    B.add("end bait x", blk, B.dict(A, front=b"\xC3\xC3", behind=Y + b"\x3C"))
    B.add("end bait y", blk, B.dict(A, front=b"\xC3\xC3", behind=rand(60, 63) + b"\x3C", after=True))
    # bait in front of the dictionary: it holds (x) or does not hold (y) the whole block, the dictionary its first half
    x = rand(1000, 8)
    short = x[:500] + rand(1500, 9)
    B.add("front bait x", x, B.dict(short, front=b"\xC3" + x))
    B.add("front bait y", x, B.dict(short, front=b"\xC3" + rand(1000, 10), after=True))
    # a slot that is too small, between good ones, all three behind one dictionary
    t = text(9000, 78)
    d = B.dict(t[:3000], front=b"\xC3\xC3")
    B.add("before small slot", t[3000:6000], d)
    B.add("small slot", t[6000:], d, cap=bound(family, 3000) - 1 if family == "lz4" else 300)
    B.add("after small slot", t[6000:], d)
    _cache[("cases", family)] = B
    return B


def zlib_subset(B):
    """the blocks of the case batch the zlib form runs over: every block below 64 KiB, and three of the long ones -- one segment and
    two, with and without a dictionary (the Adler-32 of a stream of two segments is combined from theirs)"""
    long = ("h0 n65836", "h4096 n65536", "h32768 n65836")
    return [i for i, b in enumerate(B.blocks) if len(b) < 65536 or B.names[i] in long]


def sharing(family):
    """about 300 blocks of 200..2000 bytes of text, interleaved over three distinct dictionaries and none; two of the dictionaries are
    ranges of one text that overlap but differ (the second starts 100 bytes into the first and ends 100 bytes behind it).  The last two
    blocks are ONE record behind each of those two: its first 100 bytes are found only in the second range, its next 100 only in
    the first"""
    if ("sharing", family) in _cache:
        return _cache[("sharing", family)]
    B = Batch(family)
    t = text(9000, 300)
    d0 = B.dict(t[:8000], front=b"\xC3", behind=t[8000:] + b"\x3C")
    d1 = B.dict_within(d0, 100, 8000)
    d2 = B.dict(text(4096, 301), front=b"\xC3\xC3", after=True)
    rng = np.random.default_rng(302)
    for i in range(300):
        n = int(rng.integers(200, 2001))
        B.add("rec %d" % i, text(n, 400 + i), (d0, d1, d2, None)[i % 4])
    twin = t[8000:8100] + t[:100] + rand(40, 303)
    B.add("twin first", twin, d0)
    B.add("twin second", twin, d1)
    _cache[("sharing", family)] = B
    return B


def many(family, nblocks=8200, ndict=1030):
    """More work items than the grid-strided launches have workgroups (8192 for the segments, 1024 for the build): nblocks blocks of 16
    bytes, block i a copy of its dictionary, the 16 bytes at 16 * (i % ndict) of a random buffer behind the blocks.  A block whose
    dictionary was not built, or whose segment did not run, cannot hold its match.  -> (buffer, in_off, lens, dict_off, dict_len)"""
    R = rand(16 * ndict, 500)
    blocks = b"".join(R[16 * (i % ndict):16 * (i % ndict) + 16] for i in range(nblocks))
    buf = b"\xC3" + blocks + b"\x5A\x5A\x5A" + R + b"\0" * 16
    base = 1 + len(blocks) + 3
    return (np.frombuffer(buf, np.uint8).copy(), [1 + 16 * i for i in range(nblocks)], [16] * nblocks,
            [base + 16 * (i % ndict) for i in range(nblocks)], [16] * nblocks)
