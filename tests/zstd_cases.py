"""The named inputs of the Zstandard tests: the golden frames of tests/golden/zstd (written once by tests/gen_zstd_golden.py with
libzstd 1.4.8; their raw inputs are recipes, not files), the crafted frames of tests/zstd_craft.py with what must become of each, the
single-bit flips, and mixed64().  Shared by the reference's tests, the wave simulator's and the GPU's."""
import json
import os
import random

import numpy as np

import zstd_craft as K
import zstd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "zstd")
FLIP_SEED = 20
FLIPS = 200
# flips on which the reference cannot agree with libzstd, by (file, bit), with the reason; at most 4
FLIPS_LEFT_OUT = {}


def raw_of(spec):
    """the raw bytes of a recipe: ["synth", kind, n, seed] | ["zeros", n] | ["rep", hex, times] | ["bits3", n, seed] | ["hex", hex]"""
    from rust_compress_amd import synth
    what = spec[0]
    if what == "synth":
        return bytes(synth.gen(spec[1], spec[2], spec[3]))
    if what == "zeros":
        return bytes(spec[1])
    if what == "rep":
        return bytes.fromhex(spec[1]) * spec[2]
    if what == "bits3":
        return bytes((np.asarray(synth.gen("rand", spec[1], spec[2])) % 3 == 0).astype(np.uint8))
    if what == "hex":
        return bytes.fromhex(spec[1])
    raise ValueError(what)


_golden = None


def golden():
    """-> list of dict(name, blob, raw, dict (bytes or None), needs)"""
    global _golden
    if _golden is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as fh:
            man = json.load(fh)
        _golden = []
        for e in man["frames"]:
            with open(os.path.join(GOLDEN, e["file"]), "rb") as fh:
                blob = fh.read()
            _golden.append(dict(name=e["name"], blob=blob, raw=raw_of(e["raw"]), dict=raw_of(e["dict"]) if e.get("dict") else None,
                                needs=e["needs"]))
    return _golden


def props(trace):
    """what a decode's trace (zstd_ref.decode(trace=)) says the frame reaches, as a set of words"""
    p = set()
    blocks = [t for t in trace if t[0] == "block"]
    p.add("blocks=%d" % len(blocks))
    for t in trace:
        if t[0] == "block":
            p.add(("raw_block", "rle_block", "compressed_block", "reserved_block")[t[1]])
            if t[1] == 0 and t[2] == 0:
                p.add("raw_block_of_0")
        elif t[0] == "lit":
            p.add({"raw": "lit_raw", "rle": "lit_rle"}.get(t[1]) or ("huf%d_%s" % (t[2], t[3]) if t[1] == "huffman" else "treeless%d" % t[2]))
        elif t[0] == "modes":
            for name, m in zip(("ll", "of", "ml"), t[1:]):
                p.add("%s_%s" % (name, ("predef", "rle", "fse", "repeat")[m]))
            if t[1:] == (0, 0, 0):
                p.add("three_predef")
            if t[1:] == (2, 2, 2):
                p.add("three_fse")
        elif t[0] == "nseq":
            p.add("nseq%d" % t[2])
        elif t[0] == "frame":
            p.add("fcs%d" % t[1])
            if t[2]:
                p.add("window")
            if t[3]:
                p.add("checksum")
        else:
            p.add(t[0])
    return p


# ---- crafted frames ----------------------------------------------------------------------------------------------------------------------
def _hist16():
    return bytes(range(65, 81))


def crafted():
    """-> list of dict(name, blob, dict, status, raw (None unless OK), used (the expected in_used, OK alone))"""
    out = []

    def ok(name, blob, raw, used=None, d=None):
        out.append(dict(name=name, blob=blob, dict=d, status="OK", raw=raw, used=len(blob) if used is None else used))

    def bad(name, blob, status, d=None):
        out.append(dict(name=name, blob=blob, dict=d, status=status, raw=None, used=0))

    h = _hist16()
    # literals "ab" x 0, a match of 3 at offset 16 - 3 + ... : one RLE-mode sequence block behind 16 raw bytes
    rle_lits = K.compressed(K.literals(1, b"z", 40), b"\x00", last=True)
    ok("rle_literals", K.frame([rle_lits], fcs=40, single=True), b"z" * 40)
    # all three tables in RLE mode: literal length code 2, offset code 3 (offsets 5..12), match length code 4 (7 bytes)
    seqs = K.rle_sequences(2, 3, 4, [(3, 0, 0), (0, 0, 0)])                     # offsets 8 and 5
    raw = bytearray(h)
    lit = b"0123"
    for i, off in enumerate((8, 5)):
        raw += lit[2 * i:2 * i + 2]
        for _ in range(7):
            raw.append(raw[-off])
    blk = K.compressed(K.literals(0, lit), seqs, last=True)
    ok("rle_tables", K.frame([K.block(0, h), blk], fcs=len(raw), single=True), bytes(raw))
    # 32 512 sequences of one bit each: literal length 0, match length 3, offset code 1 (the repeat offsets 8, 4, 1 in turn)
    n = 32512
    raw = bytearray(h)
    rep = [1, 4, 8]
    for _ in range(n):
        off = rep[2]
        rep = [off, rep[0], rep[1]]
        for _ in range(3):
            raw.append(raw[-off])
    big = K.compressed(K.literals(0, b""), K.rle_sequences(0, 1, 0, [(0, 0, 0)] * n), last=True)
    ok("three_byte_count", K.frame([K.block(0, h), big], fcs=len(raw)), bytes(raw))
    ok("zero_sequences", K.frame([K.compressed(K.literals(0, b"hello"), b"\x00", last=True)], fcs=5, single=True), b"hello")
    # a count of 0 sequences in two bytes is no short cut for libzstd: the modes byte must follow, and what follows that is not read
    hello = K.literals(0, b"hello")
    bad("two_byte_zero_count_without_modes", K.frame([K.compressed(hello, b"\x80\x00", last=True)], fcs=5, single=True), "E_ZSTD_DATA")
    ok("two_byte_zero_count_with_modes", K.frame([K.compressed(hello, b"\x80\x00\x00", last=True)], fcs=5, single=True), b"hello")
    ok("two_byte_zero_count_and_trailing_bytes", K.frame([K.compressed(hello, b"\x80\x00\x00\xaa\xbb", last=True)], fcs=5, single=True), b"hello")
    bad("one_byte_zero_count_and_trailing_bytes", K.frame([K.compressed(hello, b"\x00\xaa", last=True)], fcs=5, single=True), "E_ZSTD_DATA")
    ok("fcs_8_bytes", K.frame([K.block(0, b"eight", last=True)], fcs=5, fcs_bytes=8, single=True), b"eight")
    one = K.frame([K.block(0, b"first frame ", last=True)], fcs=12, single=True)
    two = K.frame([K.block(1, b"-", size=30, last=True)], window=0x00, checksum=True, raw=b"-" * 30)
    three = K.frame([K.block(0, b" third", last=True)], fcs=6, single=True)
    ok("two_frames", one + two, b"first frame " + b"-" * 30)
    ok("three_frames", one + two + three, b"first frame " + b"-" * 30 + b" third")
    ok("skippable_before_between_after", K.skippable(b"abc") + one + K.skippable(b"", 15) + two + K.skippable(b"\xff" * 9, 7),
       b"first frame " + b"-" * 30)
    ok("trailing_bytes", one + b"\x00\x01\x02\x03\x04", b"first frame ", used=len(one))
    ok("trailing_three_bytes", one + b"\x28\xb5\x2f", b"first frame ", used=len(one))
    # a sequence whose offset (40) lies beyond 4 literals and 16 bytes of history; a dictionary of 64 bytes reaches it
    far = K.frame([K.compressed(K.literals(0, b"wxyz"), K.rle_sequences(4, 5, 0, [(11, 0, 0)]), last=True)], fcs=7, single=True)
    d64 = bytes(range(100, 164))
    ok("offset_into_dictionary", far, b"wxyz" + d64[64 - 36:64 - 33], d=d64)
    bad("offset_beyond_history", far, "E_ZSTD_DATA")
    bad("offset_beyond_dictionary", far, "E_ZSTD_DATA", d=d64[:16])
    bad("reserved_header_bit", K.frame([K.block(0, b"x", last=True)], fcs=1, single=True, reserved=True), "E_ZSTD_HEADER")
    bad("window_too_large", K.frame([K.block(0, b"x", last=True)], window=0xB0), "E_ZSTD_HEADER")
    bad("block_type_3", K.frame([K.block(3, b"x", last=True)], fcs=1, single=True), "E_ZSTD_DATA")
    bad("block_over_maximum", K.frame([K.block(2, b"\x00" * 131072, last=True)], window=0x50), "E_ZSTD_DATA")
    bad("wrong_size", K.frame([K.block(0, b"four", last=True)], fcs=5, single=True), "E_ZSTD_DATA")
    bad("wrong_checksum", K.frame([K.block(0, b"sum", last=True)], fcs=3, single=True, checksum=True, raw=b"sum", bad_checksum=True), "E_ZSTD_CHECKSUM")
    bad("weights_no_power_of_two", K.frame([K.compressed(K.huffman_literals_header(2, 10, bytes([0x81, 0x31, 0x01, 0x01])), last=True)], fcs=10, single=True),
        "E_ZSTD_DATA")
    lits4 = K.literals(0, b"wxyz")
    zero_run = K.forward([(0, 4), (1, 5)] + [(3, 2)] * 16)                        # accuracy 5, a count of 0, then a run past symbol 35
    bad("distribution_zero_run_past_last_symbol", K.frame([K.compressed(lits4, b"\x01\x80" + zero_run + b"\x01", last=True)], fcs=7, single=True), "E_ZSTD_DATA")
    starved = K.forward([(0, 4), (32, 6)] + [(1, 1)] * 40)                        # accuracy 5: 31 of 32, then zeros until the symbols run out
    bad("distribution_runs_out_of_symbols", K.frame([K.compressed(lits4, b"\x01\x80" + starved + b"\x01", last=True)], fcs=7, single=True), "E_ZSTD_DATA")
    bad("accuracy_log_over_limit", K.frame([K.compressed(lits4, b"\x01\x80" + bytes([0x0F, 0, 0, 0]) + b"\x01", last=True)], fcs=7, single=True), "E_ZSTD_DATA")
    bad("treeless_without_table", K.frame([K.compressed(K.huffman_literals_header(3, 10, b"\x01\x01\x01"), last=True)], fcs=10, single=True), "E_ZSTD_DATA")
    bad("repeat_mode_without_table", K.frame([K.compressed(lits4, b"\x01\xC0\x01", last=True)], fcs=7, single=True), "E_ZSTD_DATA")
    left = K.frame([K.block(0, h), K.compressed(K.literals(0, b"0123"), K.rle_sequences(2, 3, 4, [(3, 0, 0), (0, 0, 0)], left_over=8), last=True)],
                   fcs=34, single=True)
    bad("bits_left_over", left, "E_ZSTD_DATA")
    bad("dictionary_id", K.frame([K.block(0, b"x", last=True)], fcs=1, single=True, dict_id=7), "E_ZSTD_DICT")
    good = K.frame([K.block(0, h), blk], fcs=34, single=True, checksum=True, raw=bytes(out[1]["raw"]))
    ok("good_frame_for_truncation", good, out[1]["raw"])
    for k in range(16):
        cut = 1 + (len(good) - 2) * k // 15                                    # 1 .. len - 1
        bad("truncated_%02d_at_%d" % (k, cut), good[:cut], "E_EOF")
    bad("three_byte_file", b"\x28\xb5\x2f", "E_EOF")
    bad("bad_magic", b"\x29\xb5\x2f\xfd" + good[4:], "E_ZSTD_MAGIC")
    return out


# ---- single-bit flips ----------------------------------------------------------------------------------------------------------------------
def flips(seed=FLIP_SEED, count=FLIPS):
    """count single-bit flips, from a fixed seed, in the golden frames below 4 KiB that carry no checksum -> list of dict(name, blob, file, bit)"""
    pool = [g for g in golden() if len(g["blob"]) < 4096 and "checksum" not in g["needs"] and g["dict"] is None]
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        g = pool[rng.randrange(len(pool))]
        bit = rng.randrange(8 * len(g["blob"]))
        b = bytearray(g["blob"])
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append(dict(name="%s^%d" % (g["name"], bit), blob=bytes(b), file=g["name"], bit=bit))
    return [f for f in out if (f["file"], f["bit"]) not in FLIPS_LEFT_OUT]


_expected = {}


def expected(blob, d=None):
    """the reference's outcome for a file, cached: (status name, bytes or None, out_len, in_used)"""
    key = (blob, d)
    if key not in _expected:
        _expected[key] = R.outcome(blob, d or b"")
    return _expected[key]


def mixed64():
    """about 64 files of mixed kinds, the failing ones between good ones; none decodes to more than 300 KB -> list of dict(name, blob, dict)"""
    good = [dict(name=g["name"], blob=g["blob"], dict=g["dict"]) for g in golden() if len(g["raw"]) <= 300000]
    crafts = [dict(name=c["name"], blob=c["blob"], dict=c["dict"]) for c in crafted() if c["name"] != "block_over_maximum"]
    bads = [c for c in crafts if expected(c["blob"], c["dict"])[0] != "OK"]
    goods = good + [c for c in crafts if expected(c["blob"], c["dict"])[0] == "OK"]
    fl = [dict(name=f["name"], blob=f["blob"], dict=None) for f in flips()[:12]]
    out, gi = [], 0
    for b in bads[:26] + fl:
        out.append(goods[gi % len(goods)])
        gi += 1
        out.append(b)
    while gi < len(goods):
        out.append(goods[gi])
        gi += 1
    return out[:72]
