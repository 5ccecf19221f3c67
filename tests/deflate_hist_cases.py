"""Inputs for the tests of the DEFLATE encoder and decoder with history (TEST INFRASTRUCTURE, shared by test_wavesim_deflate_hist.py
and test_gpu_deflate_hist.py).  Encode: ONE batch in one input buffer, every block with the bytes the caller put in front of it -- a
dictionary placed there, or the block before it (linked chunks).  Decode: streams written by libz with zdict= and hand-assembled
fixed-Huffman streams, each with the history the caller puts in front of its slot.  The oracle is Python's zlib (libz)."""
import zlib

import numpy as np

import hc_stages as H
from rust_compress_amd import synth

HISTS = (0, 1, 3, 4, 5, 258, 4096, 32767, 32768)
LENS = (0, 1, 3, 4, 5, 258, 259, 1000, 65536, 65536 + 300)   # the last: two segments, of which the second sees the first as its window
LEVELS = (2, 6, 9)
SEG = 65536
E_OUTPUT_TOO_SMALL, E_INVALID_HUFFMAN_CODE, E_EOF = 2, 15, 1
E_ZLIB_DICT, E_ZLIB_CHECKSUM, E_ZLIB_DICT_ID = 22, 24, 25


def bound(n):
    return n + 11 * ((n + SEG - 1) // SEG) + 2


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed):
    return synth.gen("text", n, seed).tobytes()


_grid = None


def grid():
    """[(history, block)] of every history length with every block length, one text each"""
    global _grid
    if _grid is None:
        _grid, k = [], 0
        for h in HISTS:
            for n in LENS:
                t = text(h + n, 100 + k)
                _grid.append((t[:h], t[h:]))
                k += 1
    return _grid


class Batch:
    """names, in_off, lens, hist_len, caps and the buffer"""

    def __init__(self):
        self.buf = bytearray()
        self.names, self.in_off, self.lens, self.hist_len, self.caps = [], [], [], [], []

    def add(self, name, hist, block, front=b"", cap=None):
        """`front`, then the history, then the block"""
        self.buf += front + hist
        self._block(name, block, len(hist), cap)

    def add_chain(self, name, data, size):
        """`data` as linked chunks of `size` bytes: every chunk's history is all of the chain in front of it, at most 32768 bytes"""
        self.buf += b"\x3C"
        start = len(self.buf)
        for k, at in enumerate(range(0, len(data), size)):
            assert len(self.buf) == start + at
            self._block("%s[%d]" % (name, k), data[at:at + size], min(at, 32768))

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
        return bytes(self.buf[self.in_off[i] - self.hist_len[i]:self.in_off[i]])


_batch = None


def batch():
    global _batch
    if _batch is not None:
        return _batch
    B = Batch()
    # every history length with every block length, in text; leads of 1, 2 and 3 bytes: unaligned 4-byte loads at the history's start
    for k, (h, b) in enumerate(grid()):
        B.add("h%d n%d" % (len(h), len(b)), h, b, front=b"\xC3" * (1 + k % 3))
    # a block that is a verbatim slice of a random history: from its first byte (distance exactly 32768 at position 0: DEFLATE's
    # largest, and the history's first byte IS within reach), from its last bytes; without the history the block is incompressible
    r = rand(32768, 7)
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
    # linked chunks whose histories overlap each other's inputs
    B.add_chain("chain", text(15000, 77), 3000)
    # a slot too small for its stream, between good ones (text of 3000 bytes never fits in 300)
    t = text(6000, 78)
    B.add("small slot", t[:3000], t[3000:], front=b"\xC3", cap=300)
    B.add("after small slot", t[:3000], t[3000:], front=b"\xC3\xC3")
    _batch = B
    return B


def many_batch():
    """More work items than the links grid holds workgroups (8192): 8200 empty blocks (a work item each, no segment) in front of twelve
    tiny blocks with history, whose history items are the grid's second round."""
    B = Batch()
    B.buf += b"\xC3"
    t = text(64 * 12, 79)
    for i in range(8200):
        B.add("empty %d" % i, b"", b"")
    for i in range(12):
        s = t[64 * i:64 * i + 64]
        B.add("tiny %d" % i, s[:40], s[20:60] + s[:24])       # (the block repeats its history)
    return B


def what_history_buys():
    """(records, dictionary, chunks): sixteen 2 KiB text records (seeds 0..15) behind 32 KiB of text (seed 99); 263 144 bytes of text
    (seed 5) as five chunks of 64 KiB, each primed with the 32 KiB before it"""
    recs = [text(2048, s) for s in range(16)]
    t = text(263144, 5)
    return recs, text(32768, 99), [t[a:a + SEG] for a in range(0, len(t), SEG)], t


# ------------------------------------------------------------------------------------------------------------------ decode: streams
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nb):                      # LSB first (extra bits, header fields)
        self.acc |= v << self.n
        self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nb):                     # a Huffman code: most significant bit first
        for k in range(nb - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def fixed_stream(tokens):
    """one final fixed-Huffman block of tokens: (0, byte) literals and (length, distance) matches"""
    w = _Bits()
    w.put(1, 1)
    w.put(1, 2)

    def lit(v):
        if v < 144:
            w.code(0x30 + v, 8)
        elif v < 256:
            w.code(0x190 + v - 144, 9)
        elif v < 280:
            w.code(v - 256, 7)
        else:
            w.code(0xC0 + v - 280, 8)
    for ln, x in tokens:
        if ln == 0:
            lit(x)
            continue
        k = H.LEN_SYM[ln]
        lit(257 + k)
        w.put(ln - H.LBASE[k], H.LEXTRA[k])
        ds = int(H.DIST_SYM[x])
        w.code(ds, 5)
        w.put(x - H.DBASE[ds], H.DEXTRA[ds])
    lit(256)
    return w.done()


def lz_apply(hist, tokens):
    """what the tokens decode to behind `hist`, or None when a distance points in front of the history"""
    buf = bytearray(hist)
    for ln, x in tokens:
        if ln == 0:
            buf.append(x)
            continue
        if x > len(buf) or x > 32768:
            return None
        for _ in range(ln):
            buf.append(buf[-x])
    return bytes(buf[len(hist):])


F2_NEAR = 112                                  # k_inflate2.hip: distances from here on are gathered from memory, not read from the ring


def far_gathers(tokens):
    """the slot positions at which the lane-per-stream decoder gathers 16 bytes of a far source: one gather per 16 bytes of a match
    at a distance >= F2_NEAR, the first at (the match's start - distance).  A negative position lies behind the slot's first byte
    (in the history or dictionary); one in -15 .. -1 is a gather that straddles position 0."""
    pos, at = 0, []
    for ln, x in tokens:
        if ln and x >= F2_NEAR:
            at += [pos - x + k for k in range(0, ln, 16)]
        pos += ln or 1
    return at


def libz_raw(hist, tokens_stream):
    """libz's answer to a raw stream behind `hist`: the bytes, or None (an error)"""
    d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
    try:
        return d.decompress(tokens_stream)
    except zlib.error:
        return None


def libz_stream(hist, blk, mode, wbits=-15):
    """blk compressed by libz behind the dictionary `hist`; mode: a level (0 stored, 1, 6, 9) or "fixed" (Z_FIXED at level 6)"""
    level, strat = (6, zlib.Z_FIXED) if mode == "fixed" else (mode, zlib.Z_DEFAULT_STRATEGY)
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strat, hist) if hist else zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strat)
    return c.compress(blk) + c.flush()


MODES = (0, 1, 6, 9, "fixed")
_dec = None


def first_match_tokens(d):
    """the first symbol a match of 258 bytes at distance d (all of its source behind position 0, or running over it), then a literal
    and a short match"""
    return [(258, d), (0, 65), (7, 2)]


def decode_cases():
    """[dict(name, stream, hist, cap, front, want (bytes or None), status)] of raw DEFLATE streams"""
    global _dec
    if _dec is not None:
        return _dec
    cs = []

    def add(name, stream, hist, want, status=0, cap=None, front=None):
        cs.append({"name": name, "stream": stream, "hist": hist, "want": want, "status": status,
                   "cap": (len(want) if want is not None else 0) if cap is None else cap, "front": front})
    for h, b in grid():
        for m in MODES:
            if len(b) > 1000 and m in (1, 9):                 # (the long blocks: stored, one dynamic and the fixed form)
                continue
            add("libz %s h%d n%d" % (m, len(h), len(b)), libz_stream(h, b, m), h, b)
    # hand-assembled: the first symbol a match of 258 bytes at a distance on both sides of F2_NEAR (112), from the history into the
    # stream (overlapping where the distance is short: 1, 2 and 3 repeat inside one 4-byte step and read the seeded ring alone); at
    # 113 a 16-byte gather of the source straddles the first byte of the slot
    hist = rand(300, 11)
    for d in (1, 2, 3, 111, 112, 113, 300):
        toks = first_match_tokens(d)
        add("first match d%d" % d, fixed_stream(toks), hist, lz_apply(hist, toks))
    # the reach: output so far + history, exactly; one more is an error
    hist = rand(100, 12)
    lits = [(0, 70 + i) for i in range(5)]
    add("reach end+hist", fixed_stream(lits + [(9, 105)]), hist, lz_apply(hist, lits + [(9, 105)]))
    add("reach end+hist+1", fixed_stream(lits + [(9, 106)]), hist, bytes(70 + i for i in range(5)), E_INVALID_HUFFMAN_CODE, cap=14)
    # ... into a bait in front of the history
    add("reach bait", fixed_stream([(9, 101)]), hist, b"", E_INVALID_HUFFMAN_CODE, cap=9, front=b"\xC3" + rand(64, 13))
    # DEFLATE's largest distance: all 32768 history bytes are within reach at position 0, and still the last 32768 bytes at position 1
    # (history bytes 1 .. 32767 and one byte of output); with 32767 bytes of history it points in front of them at position 0
    h32 = rand(32768, 14)
    add("d32768 h32768 p0", fixed_stream([(20, 32768)]), h32, h32[:20])
    add("d32768 h32768 p1", fixed_stream([(0, 9), (20, 32768)]), h32, b"\x09" + h32[1:21])
    add("d32768 h32767 p0", fixed_stream([(20, 32768)]), h32[1:], b"", E_INVALID_HUFFMAN_CODE, cap=20, front=b"\xC3\xC3" + h32[:1])
    add("d32768 h32767 p1", fixed_stream([(0, 9), (20, 32768)]), h32[1:], b"\x09" + h32[1:21])
    # a slot one byte short
    toks = [(0, 1), (0, 2), (40, 50)]
    add("slot short", fixed_stream(toks), hist, lz_apply(hist, toks)[:2], E_OUTPUT_TOO_SMALL, cap=41)
    # the same stream and history behind two different fronts
    toks = [(30, 100), (0, 5), (30, 131)]
    add("front x", fixed_stream(toks), hist, lz_apply(hist, toks), front=b"\xC3" + rand(200, 15))
    add("front y", fixed_stream(toks), hist, lz_apply(hist, toks), front=b"\xC3" + rand(200, 16))
    _dec = cs
    return cs


def zlib_decode_cases():
    """[dict(name, stream, hist, told (the hist_len the decoder gets), dict_id, want, status, in_used)] of zlib streams"""
    t = text(36000, 81)
    hist, blk = t[:32768], t[32768:]
    did = zlib.adler32(hist)
    z = libz_stream(hist, blk, 6, 15)
    plain = zlib.compress(blk, 6)
    bad = z[:-1] + bytes([z[-1] ^ 1])
    assert z[1] & 0x20 and z[2:6] == did.to_bytes(4, "big") and not plain[1] & 0x20
    mk = lambda name, s, told, i, want, st, used: {"name": name, "stream": s, "hist": hist, "told": told, "dict_id": i, "want": want,
                                                    "status": st, "in_used": used}
    return [mk("right id", z, len(hist), did, blk, 0, len(z)),
            mk("wrong id", z, len(hist), did ^ 0x100, b"", E_ZLIB_DICT_ID, 6),
            mk("fdict, no history", z, 0, did, b"", E_ZLIB_DICT, 2),
            mk("no fdict, a history", plain, len(hist), did, blk, 0, len(plain)),
            mk("trailer", bad, len(hist), did, blk, E_ZLIB_CHECKSUM, len(z)),
            mk("cut in the id", z[:5], len(hist), did, b"", E_EOF, 5),
            mk("short history", libz_stream(hist[-300:], blk, 9, 15), 300, zlib.adler32(hist[-300:]), blk, 0, None)]
