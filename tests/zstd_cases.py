"""The named inputs of the Zstandard tests: the golden frames of tests/golden/zstd (written once by tests/gen_zstd_golden.py with
libzstd 1.4.8; their raw inputs are recipes, not files), the crafted frames of tests/zstd_craft.py with what must become of each, the
single-bit flips, and mixed64(); the edge cases that reach the format paths those leave out (edge_cases(), golden_more(),
REQUIRED_WORDS) and the mutations.  Shared by the reference's tests, the wave simulator's and the GPU's."""
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
    """the raw bytes of a recipe: ["synth", kind, n, seed] | ["zeros", n] | ["rep", hex, times] | ["bits3", n, seed] | ["hex", hex] |
    ["randmod", n, seed, m]"""
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
    if what == "randmod":                                            # ["randmod", n, seed, m]: synth rand % m
        return bytes((np.asarray(synth.gen("rand", spec[1], spec[2])) % spec[3]).astype(np.uint8))
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


# ---- edge cases: the format paths the golden and crafted frames leave out ---------------------------------------------------------------
def golden_more():
    """the golden frames added for the 5-byte Huffman literals header (manifest.json's "more"; golden() stays the first 19) -> as golden()"""
    global _golden_more
    if _golden_more is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as fh:
            man = json.load(fh)
        _golden_more = []
        for e in man["more"]:
            with open(os.path.join(GOLDEN, e["file"]), "rb") as fh:
                blob = fh.read()
            _golden_more.append(dict(name=e["name"], blob=blob, raw=raw_of(e["raw"]), dict=None, needs=e["needs"]))
    return _golden_more


_golden_more = None
_edge = None


def _blocks(blob):
    """the (type, payload) of every block of a file's first frame, by a walk over the headers"""
    fhd = blob[4]
    single, didf, fcsf = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    pos = 5 + (0 if single else 1) + (4 if didf == 3 else didf) + (single if fcsf == 0 else (2, 4, 8)[fcsf - 1])
    out = []
    while True:
        bh = int.from_bytes(blob[pos:pos + 3], "little")
        kind, size = (bh >> 1) & 3, bh >> 3
        out.append((kind, blob[pos + 3:pos + 3 + (1 if kind == 1 else size)]))
        pos += 3 + (1 if kind == 1 else size)
        if bh & 1:
            return out


def _treeless_of(blob):
    """the literals of a file's first block (Huffman, one stream, a 3-byte header) again as treeless literals: the same stream without
    its table -> (the literals section, their count)"""
    kind, blk = _blocks(blob)[0]
    h = int.from_bytes(blk[:3], "little")
    assert kind == 2 and h & 15 == 2                                 # compressed literals, one stream
    size, csize = (h >> 4) & 0x3FF, h >> 14
    body = blk[3:3 + csize]
    used = R.read_huffman(body)[2]
    return K.huffman_literals_header(3, size, body[used:]), size


def edge_cases():
    """-> list of dict(name, blob, dict, status, size (the decoded size, OK alone), caps (further (capacity, status) pairs, or ()))"""
    global _edge
    if _edge is not None:
        return _edge
    out = []

    def add(name, blob, status="OK", size=None, d=None, caps=()):
        assert (status == "OK") == (size is not None)
        out.append(dict(name=name, blob=blob, dict=d, status=status, size=size, caps=caps))

    h = _hist16()
    none = K.literals(0, b"")
    fr = lambda blocks, **kw: K.frame(blocks, window=0x50, **kw)
    # literal length 0, match length 3, offset 3: sequence k copies sequence k - 1, the last lane of a full batch hops 63 times
    for n in (63, 64, 65, 200):
        add("hop%d" % n, fr([K.block(0, h), K.compressed(none, K.rle_sequences(0, 2, 0, [(2, 0, 0)] * n), last=True)], fcs=16 + 3 * n), size=16 + 3 * n)
    # offset_value 3 behind no literals is rep0 - 1 = 0, read as 1
    add("rep0_minus_1_is_zero", fr([K.block(0, h), K.compressed(none, K.rle_sequences(0, 1, 0, [(1, 0, 0)]), last=True)], fcs=19), size=19)
    add("ll_code35", fr([K.compressed(K.literals(1, b"q", 100000), K.rle_sequences(35, 2, 0, [(2, 0, 30000)]), last=True)]), size=100003)
    add("ml_code52_max", fr([K.block(0, h), K.compressed(none, K.rle_sequences(0, 2, 52, [(2, 65535, 0)]), last=True)]), size=131090)
    add("ml_code52_off1", fr([K.block(0, h), K.compressed(none, K.rle_sequences(0, 2, 52, [(0, 1234, 0)]), last=True)]), size=66789)
    pat = bytes((i * 7 + (i >> 8)) & 255 for i in range(5000))
    add("raw_lit_3byte", fr([K.compressed(K.literals(0, pat), K.rle_sequences(25, 5, 3, [(9, 0, 10)] * 3), last=True)]), size=5018)
    add("lit_rle_1byte", fr([K.compressed(K.literals(1, b"r", 20), K.rle_sequences(5, 2, 0, [(2, 0, 0)]), last=True)]), size=23)
    for oc in (31, 30, 20):
        add("of_code%d" % oc, fr([K.block(0, h), K.compressed(none, K.rle_sequences(0, oc, 0, [(0, 0, 0)]), last=True)]), "E_ZSTD_DATA")
    # sequence counts at the edges of the ring of 64: one literal, four match bytes at the offsets 5 .. 12
    for n in (1, 63, 64, 65, 127, 128, 129):
        lits = bytes((i * 11 + 3) & 255 for i in range(2 * (n % 200 + 1)))
        seqs = K.rle_sequences(1, 3, 1, [((i * 5) % 8, 0, 0) for i in range(n)])
        add("ring%d" % n, fr([K.block(0, h), K.compressed(K.literals(0, lits), seqs, last=True)]), size=16 + len(lits) + 4 * n)
    # a match of 67 that starts 36 bytes into a dictionary of 64: dictionary, the four literals, then its own output
    d64 = bytes(range(100, 164))
    straddle = fr([K.compressed(K.literals(0, b"wxyz"), K.rle_sequences(4, 5, 40, [(11, 0, 0)]), last=True)])
    add("dict_straddle", straddle, size=71, d=d64)
    add("dict_straddle_without_dictionary", straddle, "E_ZSTD_DATA")
    # second frames that hold a compressed block: the repeat offsets, the tables and the history begin again
    by = {c["name"]: c for c in crafted()}
    gold = {g["name"]: g for g in golden()}
    rle_tables = by["rle_tables"]["blob"]
    again = fr([K.block(0, h), K.compressed(K.literals(0, b"0123"), K.rle_sequences(2, 0, 4, [(0, 0, 0)] * 2), last=True)])
    add("two_frames_rep_reset", rle_tables + again, size=68)
    far = by["offset_into_dictionary"]["blob"]
    add("far_second_frame", rle_tables + far, "E_ZSTD_DATA")             # the first frame's output is no history
    add("far_second_frame_with_dictionary", rle_tables + far, size=41, d=d64)
    t8000 = gold["text_8000_l19_w12"]["blob"]
    blocks = _blocks(t8000)
    assert [k for k, _ in blocks] == [2, 2]
    treeless = fr([K.block(2, blocks[1][1], last=True)])
    add("treeless_in_second_frame_alone", treeless, "E_ZSTD_DATA")
    add("treeless_in_second_frame", t8000 + treeless, "E_ZSTD_DATA")
    # the same two, built so that they WOULD decode with what the frame (or the file) before them left behind: the literals of
    # bits3_4000_l1's block as treeless literals and no sequences; rle_tables' sequences with its three tables in repeat mode
    bits3 = gold["bits3_4000_l1"]["blob"]
    lits, count = _treeless_of(bits3)
    borrowed = fr([K.compressed(lits, last=True)], fcs=count)
    add("treeless_with_the_table_of_the_frame_before", bits3 + borrowed, "E_ZSTD_DATA")
    add("treeless_with_the_table_of_the_file_before", borrowed, "E_ZSTD_DATA")
    repeat = fr([K.block(0, h), K.compressed(K.literals(0, b"0123"), K.rle_sequences(2, 3, 4, [(3, 0, 0), (0, 0, 0)], repeat=True), last=True)], fcs=34)
    add("repeat_mode_with_the_tables_of_the_frame_before", rle_tables + repeat, "E_ZSTD_DATA")
    add("repeat_mode_with_the_tables_of_the_file_before", repeat, "E_ZSTD_DATA")
    add("golden_twice", t8000 + t8000, size=16000)
    add("golden_mix", gold["text_5000_l3"]["blob"] + gold["runs_5000_l3"]["blob"] + gold["bits3_4000_l19"]["blob"], size=14000)
    # raw and RLE blocks beyond the block maximum of 128 KiB, which libzstd does not hold them to
    big = bytes((i * 13 + (i >> 7)) & 255 for i in range(200000))
    add("raw_block_131073", fr([K.block(0, big[:131073], last=True)]), size=131073)
    add("raw_block_200000", K.frame([K.block(0, big, last=True)], window=0x70), size=200000)
    add("rle_block_131073", fr([K.block(1, b"r", size=131073, last=True)]), size=131073)
    add("rle_block_2097151", K.frame([K.block(1, b"r", size=(1 << 21) - 1, last=True)], window=0x70), size=(1 << 21) - 1)
    # a wrong checksum in the first of two frames: reported where the first frame fits, left to the retry where it does not
    one = K.frame([K.block(0, b"the first sum is wrong", last=True)], fcs=22, single=True, checksum=True, raw=b"the first sum is wrong", bad_checksum=True)
    two = K.frame([K.block(1, b"+", size=40, last=True)], fcs=40, single=True, checksum=True, raw=b"+" * 40)
    add("bad_sum_then_overflow", one + two, "E_ZSTD_CHECKSUM", caps=((22, "E_ZSTD_CHECKSUM"), (21, "E_OUTPUT_TOO_SMALL")))
    _edge = out
    return out


# the words (props) that the golden frames, crafted() and edge_cases() must reach between them: one per path of k_zstd.hip that a test
# input has to keep reached, and every word a golden frame's `needs` names
REQUIRED_WORDS = frozenset(
    ["lithdr%d_%s" % (n, k) for n in (1, 2, 3) for k in ("raw", "rle")] + ["hufhdr3", "hufhdr4", "hufhdr5", "lit_full"] +
    ["rep%d%s" % (n, s) for n in (1, 2, 3) for s in ("", "_ll0")] +
    ["zero_as_1", "ll_bits>=8", "ml_bits>=14", "of_code>=20", "dict_straddle", "frame2_compressed", "weights_end_state1", "weights_end_state2"] +
    ["raw_block_of_0", "raw_block", "rle_block", "compressed_block", "lit_raw", "three_predef", "huf4_fse", "three_fse", "nseq2", "huf1_fse",
     "huf1_direct", "huf4_direct", "overlap", "blocks=2", "treeless4", "ll_repeat", "window", "blocks=3", "of_repeat", "blocks=40",
     "ml_repeat", "of_rle", "ll_rle", "treeless1", "checksum", "fcs4", "far", "fcs0", "dict"])


def capacity_sweep():
    """Slots that end inside a literal run, a match, a batch of 64 sequences or between frames: every OK file of edge_cases(), the golden
    frames that decode to fewer than 50 000 bytes and the OK entries of crafted(), once per capacity of {1, n - 1, n * 64 // 256,
    n * 65 // 256, n * 191 // 256, n * 193 // 256} for a decoded size n, and bad_sum_then_overflow at its two capacities
    -> list of dict(name, blob, dict, cap)"""
    files = [c for c in edge_cases() if c["status"] == "OK"] + [g for g in golden() if len(g["raw"]) < 50000] + \
            [c for c in crafted() if c["status"] == "OK"]
    out = []
    for c in files:
        n = expected(c["blob"], c["dict"])[2]
        caps = []
        for cap in (1, n - 1, n * 64 // 256, n * 65 // 256, n * 191 // 256, n * 193 // 256):
            if cap >= 0 and cap not in caps:
                caps.append(cap)
        out += [dict(name="%s@%d" % (c["name"], cap), blob=c["blob"], dict=c["dict"], cap=cap) for cap in caps]
    bad = [c for c in edge_cases() if c["name"] == "bad_sum_then_overflow"][0]
    out += [dict(name="%s@%d" % (bad["name"], cap), blob=bad["blob"], dict=None, cap=cap) for cap, _ in bad["caps"]]
    return out


PERSISTENT_FILES = 2 * 2048 + 64


def persistent_files(n=PERSISTENT_FILES, waves=2048):
    """n files for `waves` persistent waves: wave w decodes the files w, w + waves, w + 2 * waves in turn with one literal buffer, one set
    of tables in LDS and one set of counters, and file i is T[(i % waves) % len(T)][i // waves], each triple of T built so that what a
    file leaves behind would show in the next: a table that must not be inherited, a dictionary, a file cut short, another Huffman
    table, RLE literals before raw ones.  Every blob is under 2.5 KiB.  -> list of dict(name, blob, dict)"""
    by = {c["name"]: c for c in golden() + crafted() + edge_cases()}
    trunc = [c["name"] for c in crafted() if c["name"].startswith("truncated_")]
    T = [("runs_5000_l3", "treeless_without_table", "bits3_4000_l1"),              # a Huffman table, then treeless literals: still refused
         ("text_5000_l3", "repeat_mode_without_table", "rle_tables"),              # three FSE tables, then repeat mode: still refused
         ("text_5000_l3", "bits3_4000_l1", "treeless_with_the_table_of_the_file_before"),   # ... and the table that would decode them
         ("bits3_4000_l19", "rle_tables", "repeat_mode_with_the_tables_of_the_file_before"),
         ("bits3_4000_l1", "treeless_with_the_table_of_the_file_before", "rle_tables"),
         ("rle_tables", "repeat_mode_with_the_tables_of_the_file_before", "runs_5000_l3"),
         ("record_behind_dictionary", "offset_beyond_history", "offset_into_dictionary"),   # a dictionary, then none
         (trunc[9], "good_frame_for_truncation", trunc[14]),                       # cut short, then whole
         ("bits3_4000_l1", "bits3_4000_l19", "runs_5000_l3"),                      # one Huffman table, then another
         ("rle_literals", "ring63", "lit_rle_1byte"),                              # RLE literals, then raw ones
         ("text_3000_l19_w10", "treeless_in_second_frame_alone", "stream_no_size"),
         ("hop64", "rep0_minus_1_is_zero", "two_frames_rep_reset")]                # repeat offsets that must begin at 1, 4, 8
    assert all(len(by[name]["blob"]) < 2560 for t in T for name in t)
    return [dict(name=by[name]["name"], blob=by[name]["blob"], dict=by[name]["dict"]) for name in (T[(i % waves) % len(T)][i // waves] for i in range(n))]


# ---- mutations: bit flips, byte sets and deletions, checksummed frames included ---------------------------------------------------------
MUTATION_SEED = 777
MUTATIONS = 600
# mutations on which the reference cannot agree with libzstd, by their number k, with the reason; at most 4
MUTATIONS_LEFT_OUT = {}


def mutations(seed=MUTATION_SEED, count=MUTATIONS):
    """count mutated files from a fixed seed -> list of dict(name, blob, file, k).  The pool: the golden frames below 4 KiB without a
    dictionary, then the OK entries of crafted() below 4 KiB without one.  Mutation k is, by k % 3: one bit flipped; one byte set to
    0, 255, 128, 1 or anything; one to three bytes deleted."""
    pool = [(g["name"], g["blob"]) for g in golden() if len(g["blob"]) < 4096 and g["dict"] is None] + \
           [(c["name"], c["blob"]) for c in crafted() if c["status"] == "OK" and c["dict"] is None and len(c["blob"]) < 4096]
    rng = random.Random(seed)
    out = []
    for k in range(count):
        name, blob = pool[rng.randrange(len(pool))]
        b = bytearray(blob)
        if k % 3 == 0:
            bit = rng.randrange(8 * len(b))
            b[bit >> 3] ^= 1 << (bit & 7)
        elif k % 3 == 1:
            i = rng.randrange(len(b))
            b[i] = rng.choice([0, 255, 128, 1, rng.randrange(256)])
        else:
            i = rng.randrange(len(b))
            del b[i:min(len(b), i + rng.randrange(1, 4))]
        out.append(dict(name="%s#%d" % (name, k), blob=bytes(b), file=name, k=k))
    return [m for m in out if m["k"] not in MUTATIONS_LEFT_OUT]


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
