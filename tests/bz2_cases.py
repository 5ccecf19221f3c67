"""The inputs of the bzip2 tests (wave simulator and GPU) and their oracle: libbz2 through Python's bz2, read STRICTLY -- stream by stream,
every stream to its end, a following stream only where BZh1..BZh9 stands, every stream error raised (bz2.decompress drops a corrupt
second stream silently)."""
import bz2
import functools

import numpy as np

import bz2_craft as K
from rust_compress_amd import synth

OK, E_EOF, E_TOO_SMALL = 0, 1, 2
E_MAGIC, E_DATA, E_BLOCK_CRC, E_STREAM_CRC, E_RANDOMISED = 70, 71, 72, 73, 74


def _magic(b):
    return len(b) >= 4 and b[:3] == b"BZh" and 0x31 <= b[3] <= 0x39


def strict(blob):
    """-> (decoded bytes, bytes consumed up to the end of the last stream's padding); raises OSError / EOFError / ValueError"""
    pos, out, first = 0, [], True
    while first or _magic(blob[pos:pos + 4]):
        d = bz2.BZ2Decompressor()
        out.append(d.decompress(blob[pos:]))
        if not d.eof:
            raise EOFError("the input ends inside a stream")
        pos = len(blob) - len(d.unused_data)
        first = False
    return b"".join(out), pos


def expected(blob):
    """-> (data, in_used) or None where the strict oracle raises"""
    try:
        return strict(blob)
    except (OSError, EOFError, ValueError):
        return None


def text(n, seed=7):
    return synth.gen("text", n, seed).tobytes()


def _run_cases():
    """runs of exactly 3, 4, 5, 255, 256, 259, 260 and 600 equal bytes between other bytes"""
    return [("run%d" % k, bz2.compress(b"xy" + b"r" * k + b"z" + b"q" * k)) for k in (3, 4, 5, 255, 256, 259, 260, 600)]


def _crafted_runs():
    """what libbz2 never writes: a block that ends after four equal bytes with no count (libbz2 reads the count behind the block's end
    and rejects the block), a count of 255, a count equal to the run's own byte followed by that byte again, periodic texts"""
    out = []
    for name, t in (("end4", b"abc" + b"dddd"), ("count255", b"ab" + b"cccc" + bytes([255]) + b"de"),
                    ("count_own", b"k" + bytes([5]) * 4 + bytes([5]) + bytes([5]) * 3 + b"m"), ("periodic", b"abcab" * 6),
                    ("periodic1", b"z" * 3)):
        s, plain = K.stream(3, [K.block_from_text(t)])
        out.append(("craft_" + name, s))
    return out


def _crafted_tables():
    out = []
    t = b"the quick brown fox jumps over the lazy dog " * 3
    base = K.block_from_text(t)
    alpha = len(base["used"]) + 2
    nsym = len(base["symbols"]) + 1
    groups = (nsym + 49) // 50
    flat = max(1, (alpha - 1).bit_length())
    # 2 and 6 tables, every group of 50 on another one
    for ng in (2, 6):
        b = K.block_from_text(t, tables=[[flat] * alpha for _ in range(ng)], selectors=[g % ng for g in range(groups)])
        out.append(("tables%d" % ng, K.stream(9, [b])[0]))
    # lengths of 1 and 20: a two-byte alphabet (alphaSize 4) coded 1, 2, 20, 20 -- an INCOMPLETE table that libbz2 takes
    tiny = K.block_from_text(b"abab" * 5 + b"b")
    a = len(tiny["used"]) + 2
    assert a == 4
    freq = sorted(range(a), key=lambda s: -(list(tiny["symbols"]) + [a - 1]).count(s))
    lens = [0] * a
    for rank, s in enumerate(freq):
        lens[s] = (1, 2, 20, 20)[rank]
    out.append(("len_1_20_incomplete", K.stream(1, [dict(tiny, tables=[lens, lens])])[0]))
    # over-subscribed: the end-of-block symbol in 1 bit, then three codes of length 2 and two of length 3 (Kraft sum 3/2); only the
    # first two of length 2 can be written, and the data -- a run of the first used byte -- needs no other
    over = K.block([K.RUNA, K.RUNB], [0x61, 0x62, 0x63, 0x64], tables=[[2, 2, 2, 3, 3, 1]] * 2)
    out.append(("oversubscribed", K.stream(1, [over])[0]))
    # a selector >= nGroups; too few selectors; origPtr = nblock
    two = [[flat] * alpha, [flat] * alpha]
    b = K.block_from_text(t, tables=two, selectors=[0] * (groups - 1), selector_values=[2])
    b["kw"]["n_selectors"] = groups
    out.append(("selector_ge_ngroups", K.stream(9, [b])[0]))
    if groups > 1:
        b = K.block_from_text(t, tables=two, selectors=[0] * (groups - 1))
        out.append(("too_few_selectors", K.stream(9, [b])[0]))
    b = K.block_from_text(t)
    out.append(("origptr_eq_nblock", K.stream(9, [dict(b, orig=len(b["l"]))])[0]))
    b = K.block_from_text(t)
    out.append(("bad_block_crc", K.stream(9, [dict(b, crc=b["crc"] ^ 1)])[0]))
    out.append(("bad_stream_crc", K.stream(9, [b], combined=b["crc"] ^ 0x80)[0]))
    out.append(("no_stream_end", K.stream(9, [b], end=False)[0]))
    return out


@functools.lru_cache(None)
def marks_inside():
    """A block of 16 symbols with 4-bit codes (symbol = its nibble) whose symbol stream spells the block mark, and a second whose stream
    spells the stream-end mark; padding symbols in front are tried until the mark starts off a byte boundary and
    the walk from origPtr is one cycle (then every decoder reads the same text).  -> (file bytes, [bit of the false block mark, bit of
    the false end mark])"""
    used = list(range(0x30, 0x3E))                             # 14 bytes: alphaSize 16
    tables = [[4] * 16, [4] * 16]
    blocks, where = [], []
    w = K.Bits()
    w.put(int.from_bytes(b"BZh9", "big"), 32)
    for mark in (K.BLOCK_MARK, K.END_MARK):
        nib = [(mark >> (44 - 4 * i)) & 15 for i in range(12)]
        found = None
        for pad in range(0, 40):
            for tail in range(0, 12):
                for filler in (2, 3, 5, 7):
                    syms = [filler + (i % 3) for i in range(pad)] + nib + [2 + (i * 5) % 11 for i in range(tail)]
                    l = K.symbols_to_l(syms, used)
                    for orig in range(min(len(l), 6)):
                        b = K.block(syms, used, tables=tables, orig=orig)
                        if b["cycle"] != len(l):
                            continue
                        trial = K.Bits()
                        trial.v, trial.n = w.v, w.n
                        K.block_bits(trial, [], used, tables, b["selectors"], orig, 0)
                        start = trial.n - 4 + 4 * pad              # (the empty block's end-of-block nibble is where the symbols begin)
                        if start % 8 != 0:
                            found = (b, start)
                            break
                    if found:
                        break
                if found:
                    break
            if found:
                break
        assert found, "no crafted block spells the mark off a byte boundary"
        b, start = found
        K.block_bits(w, b["symbols"], b["used"], b["tables"], b["selectors"], b["orig"], b["crc"])
        blocks.append(b)
        where.append(start)
    comb = 0
    for b in blocks:
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ b["crc"]
    w.put(K.END_MARK, 48)
    w.put(comb, 32)
    w.pad()
    return w.bytes(), where


def randomised():
    """a block with the obsolete randomised bit set.  libbz2 still reads such blocks; this library refuses them with a status of their own,
    so the file is not part of the oracle comparison"""
    b = K.block_from_text(b"the quick brown fox jumps over the lazy dog " * 3)
    return K.stream(9, [dict(b, kw=dict(randomised=1))])[0]


def short_cycle():
    """THE KNOWN DIFFERENCE FROM libbz2: an L that is the BWT of nothing, whose cycle through origPtr (5 steps) does not divide the
    block's length (14).  libbz2 goes round the cycle forwards, the inverse BWT of this library backwards, and the texts differ; the
    CRC is libbz2's, so libbz2 takes the file and this library reports a block CRC.  No encoder writes such a block.
    -> (file bytes, what libbz2 decodes it to)"""
    b = K.block([1, 0, 3, 0, 3, 3, 4, 0, 3, 2, 1], [0x61, 0x62, 0x63, 0x64], orig=5)
    assert len(b["l"]) == 14 and b["cycle"] == 5
    return K.stream(1, [b])


@functools.lru_cache(None)
def two_block():
    """a two-block level-1 file: 100 001 bytes of text"""
    return bz2.compress(text(100001), 1)


@functools.lru_cache(None)
def named():
    """-> [(name, file bytes)]: sizes and levels, runs, tables, a mark inside data, streams, truncations"""
    t100, t250 = text(100001), text(250000, 8)
    c = [("empty", bz2.compress(b"")), ("one_byte", bz2.compress(b"q")), ("banana", bz2.compress(b"banana")),
         ("all256", bz2.compress(bytes(range(256)))),
         ("text100001_l1", two_block()), ("text250000_l1", bz2.compress(t250, 1)),
         ("text100001_l9", bz2.compress(t100, 9)), ("text250000_l9", bz2.compress(t250, 9)),
         ("zeros2m", bz2.compress(bytes(2 << 20)))]
    c += _run_cases() + _crafted_runs() + _crafted_tables()
    c.append(("marks_inside", marks_inside()[0]))
    s1, s9, s5 = bz2.compress(b"first stream " * 40, 1), bz2.compress(text(3000, 9), 9), bz2.compress(b"third" * 99, 5)
    c += [("three_streams", s1 + s9 + s5), ("stream_xyz", s9 + b"xyz"), ("stream_then_header", s9 + b"BZh9"),
          ("corrupt_second", s1 + s9[:40] + bytes([s9[40] ^ 0x10]) + s9[41:]), ("bad_magic", b"BZx9" + s9[4:]), ("bad_level", b"BZh0" + s9[4:]),
          ("short", b"BZ"), ("nothing", b"")]
    two = two_block()
    n = len(two)
    cuts = sorted(set([3, 4, 7, 9, 10, 14, 40, n // 4, n // 2 - 1, n // 2 + 3, (3 * n) // 4, n - 12, n - 9, n - 6, n - 3, n - 1]))
    assert len(cuts) == 16
    c += [("trunc%d" % k, two[:k]) for k in cuts]
    return c


@functools.lru_cache(None)
def flips(count=200, seed=2024):
    """the two-block file with `count` seeded single-bit flips -> [(bit, file bytes)]"""
    two = two_block()
    rng = np.random.default_rng(seed)
    out = []
    for bit in rng.choice(len(two) * 8, count, replace=False):
        b = bytearray(two)
        b[int(bit) // 8] ^= 0x80 >> (int(bit) % 8)
        out.append((int(bit), bytes(b)))
    return out


def mixed64():
    """about 64 mixed files for one call: every named input but the largest, and a few flips"""
    c = [(k, b) for k, b in named() if k not in ("text250000_l1", "text250000_l9")]
    c += [("flip%d" % bit, b) for bit, b in flips()[:6]]
    return c
