"""tests/zstd_ref.py, the plain-Python Zstandard decoder the other Zstandard tests take as their oracle, against the golden frames'
recipes, the crafted frames' expectations and -- where ctypes finds libzstd -- libzstd itself (1.4.8 wrote the golden frames): bytes
and accept / reject equal ZSTD_decompress / ZSTD_decompress_usingDict frame by frame, in_used comes from ZSTD_findFrameCompressedSize.  The same for the edge cases, the further golden frames and the 600 mutations of
tests/zstd_cases.py, and: every word of REQUIRED_WORDS is reached by a named input.
CPU only."""
import ctypes as C

import pytest

import zstd_cases as Z
import zstd_ref as R


def _libzstd():
    try:
        z = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    for f in ("ZSTD_decompress", "ZSTD_decompress_usingDict", "ZSTD_findFrameCompressedSize", "ZSTD_isError"):
        getattr(z, f).restype = C.c_size_t
    z.ZSTD_createDCtx.restype = C.c_void_p
    return z


LIB = _libzstd()
needs_lib = pytest.mark.skipif(LIB is None, reason="no libzstd.so.1 on this machine")


def lib_outcome(blob, d=None, cap=400000):
    """the file as the batch call defines it, decoded frame by frame with libzstd -> (accepted, bytes, in_used)"""
    pos, out, frames = 0, b"", 0
    dst = C.create_string_buffer(cap)
    dctx = C.c_void_p(LIB.ZSTD_createDCtx())
    try:
        while len(blob) - pos >= 4:
            magic = int.from_bytes(blob[pos:pos + 4], "little")
            if magic != R.MAGIC and magic & 0xFFFFFFF0 != 0x184D2A50:
                break
            rest = blob[pos:]
            size = LIB.ZSTD_findFrameCompressedSize(rest, C.c_size_t(len(rest)))
            if LIB.ZSTD_isError(C.c_size_t(size)):
                return False, None, 0
            n = LIB.ZSTD_decompress_usingDict(dctx, dst, C.c_size_t(cap), rest, C.c_size_t(size), d, C.c_size_t(len(d) if d else 0))
            if LIB.ZSTD_isError(C.c_size_t(n)):
                return False, None, 0
            out += dst.raw[:n]
            pos += size
            frames += 1
        return (True, out, pos) if frames else (False, None, 0)
    finally:
        LIB.ZSTD_freeDCtx(dctx)


def test_golden_frames_decode_to_their_recipes_and_reach_their_paths():
    assert len(Z.golden()) == 19
    for g in Z.golden():
        trace = []
        data, used = R.decode(g["blob"], g["dict"] or b"", trace=trace)
        assert data == g["raw"] and used == len(g["blob"]), g["name"]
        assert set(g["needs"]) <= Z.props(trace), g["name"]
        assert len(g["blob"]) < 100 * 1024


def test_the_dictionary_record_needs_its_dictionary():
    g = [g for g in Z.golden() if g["dict"]][0]
    assert Z.expected(g["blob"], None)[0] == "E_ZSTD_DATA"          # the offset beyond history


def test_crafted_frames_decode_or_are_refused_as_listed():
    names = [c["name"] for c in Z.crafted()]
    assert len(set(names)) == len(names)
    assert sum(1 for n in names if n.startswith("truncated_")) == 16
    for c in Z.crafted():
        st, data, out_len, used = Z.expected(c["blob"], c["dict"])
        assert st == c["status"], (c["name"], st)
        if st == "OK":
            assert data == bytes(c["raw"]) and used == c["used"], c["name"]


def test_three_byte_count_is_reached_under_100_kb():
    c = [c for c in Z.crafted() if c["name"] == "three_byte_count"][0]
    trace = []
    R.decode(c["blob"], trace=trace)
    assert ("nseq", 32512, 3) in trace and len(c["raw"]) < 100000


def test_size_query_and_capacity():
    g = [g for g in Z.golden() if g["name"] == "stream_no_size"][0]
    assert R.outcome(g["blob"], cap=0)[:3] == ("E_OUTPUT_TOO_SMALL", None, 6000)
    assert R.outcome(g["blob"], cap=6000)[0] == "OK"


def test_xxh64_known_values():
    assert R.xxh64(b"") == 0xEF46DB3751D8E999
    assert R.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert R.xxh64(b"abc") == 0x44BC2CF5AD770999
    assert R.xxh64(b"Nobody inspects the spammish repetition") == 0xFBCEA83C8A378BF1


@needs_lib
def test_golden_and_crafted_agree_with_libzstd():
    for c in [dict(name=g["name"], blob=g["blob"], dict=g["dict"]) for g in Z.golden()] + Z.crafted():
        st, data, out_len, used = Z.expected(c["blob"], c["dict"])
        ok, ldata, lused = lib_outcome(c["blob"], c["dict"])
        assert ok == (st == "OK"), (c["name"], st)
        if ok:
            assert ldata == data and lused == used, c["name"]


@needs_lib
def test_single_bit_flips_agree_with_libzstd():
    fl = Z.flips()
    assert len(Z.FLIPS_LEFT_OUT) <= 4 and len(fl) == Z.FLIPS - len(Z.FLIPS_LEFT_OUT)
    for f in fl:
        st, data, out_len, used = Z.expected(f["blob"])
        ok, ldata, lused = lib_outcome(f["blob"])
        assert ok == (st == "OK"), (f["name"], st)
        if ok:
            assert ldata == data and lused == used, f["name"]


# ---- the edge cases, the two further golden frames and the mutations --------------------------------------------------------------------
def _words(c):
    trace = []
    try:
        R.decode(c["blob"], c["dict"] or b"", trace=trace)
    except R.ZstdRefError:
        pass                                                        # (a refused file still reached what it reached)
    return Z.props(trace)


def test_the_further_golden_frames_decode_to_their_recipes_and_reach_their_paths():
    assert [g["name"] for g in Z.golden_more()] == ["rand200_20000_l3", "rand48_131072_l1"]
    for g in Z.golden_more():
        trace = []
        data, used = R.decode(g["blob"], trace=trace)
        assert data == g["raw"] and used == len(g["blob"]), g["name"]
        assert set(g["needs"]) <= Z.props(trace), g["name"]
        assert len(g["blob"]) < 100 * 1024
    assert ("lit", "huffman", 4, "fse") in trace and len(Z.golden_more()[1]["raw"]) == R.BLOCK_MAX      # one block, all of it literals


def test_every_required_word_is_reached_by_a_named_input():
    reached = set()
    for c in Z.golden() + Z.golden_more() + Z.crafted() + Z.edge_cases():
        reached |= _words(c)
    assert not Z.REQUIRED_WORDS - reached, sorted(Z.REQUIRED_WORDS - reached)
    needs = set(w for g in Z.golden() + Z.golden_more() for w in g["needs"])
    assert needs <= Z.REQUIRED_WORDS
    paths = ("lithdr1_raw lithdr2_raw lithdr3_raw lithdr1_rle lithdr2_rle lithdr3_rle hufhdr3 hufhdr4 hufhdr5 lit_full rep1 rep2 rep3 rep1_ll0 "
             "rep2_ll0 rep3_ll0 zero_as_1 ll_bits>=8 ml_bits>=14 of_code>=20 dict_straddle frame2_compressed weights_end_state1 "
             "weights_end_state2").split()
    assert set(paths) <= Z.REQUIRED_WORDS


def test_the_edge_cases_reach_the_paths_they_are_named_for():
    by = {c["name"]: _words(c) for c in Z.edge_cases()}
    for name, words in (("rep0_minus_1_is_zero", ["zero_as_1", "rep3_ll0"]), ("ll_code35", ["lithdr3_rle", "ll_bits>=8"]),
                        ("ml_code52_max", ["ml_bits>=14", "overlap"]), ("ml_code52_off1", ["ml_bits>=14", "overlap"]),
                        ("raw_lit_3byte", ["lithdr3_raw"]), ("lit_rle_1byte", ["lithdr1_rle"]), ("of_code31", ["of_code>=20"]),
                        ("of_code30", ["of_code>=20"]), ("of_code20", ["of_code>=20"]), ("dict_straddle", ["dict", "dict_straddle"]),
                        ("two_frames_rep_reset", ["frame2_compressed", "rep1"]), ("far_second_frame", ["frame2_compressed"]),
                        ("treeless_in_second_frame", ["frame2_compressed", "treeless4", "ll_repeat"]),
                        ("treeless_in_second_frame_alone", ["treeless4"]), ("golden_twice", ["frame2_compressed", "huf4_fse"]),
                        ("golden_mix", ["frame2_compressed", "huf1_fse", "huf4_direct"])):
        assert set(words) <= by[name], (name, sorted(by[name]))
    for n in (63, 64, 65, 200, 1, 127, 128, 129):
        for kind in ("hop", "ring"):
            if kind + str(n) in by:
                assert "nseq1" in by[kind + str(n)] or n >= 128 and "nseq2" in by[kind + str(n)]


def test_edge_cases_decode_or_are_refused_as_listed():
    names = [c["name"] for c in Z.edge_cases()]
    assert len(set(names)) == len(names) == 38
    for c in Z.edge_cases():
        st, data, out_len, used = Z.expected(c["blob"], c["dict"])
        assert st == c["status"], (c["name"], st)
        if st == "OK":
            assert out_len == c["size"] == len(data) and used == len(c["blob"]), c["name"]
        for cap, want in c["caps"]:
            assert R.outcome(c["blob"], c["dict"] or b"", cap)[0] == want, (c["name"], cap)
    by = {c["name"]: c for c in Z.edge_cases()}
    assert Z.expected(by["rep0_minus_1_is_zero"]["blob"])[1] == bytes(range(65, 81)) + b"PPP"
    h = bytes(range(65, 81))
    assert Z.expected(by["ml_code52_max"]["blob"])[1] == (h + b"NOP" * 43692)[:131090]          # one block that decodes to more than 128 KiB
    assert Z.expected(by["ml_code52_off1"]["blob"])[1] == h + b"P" * 66773
    d64 = bytes(range(100, 164))
    src = d64[28:] + b"wxyz"                                         # 40 bytes back from behind the literals
    assert Z.expected(by["dict_straddle"]["blob"], d64)[1] == b"wxyz" + (src * 2)[:67]
    assert Z.expected(by["two_frames_rep_reset"]["blob"])[1][34:] == h + b"01" + b"1" * 7 + b"23" + b"3" * 7   # rep0 is 1 again
    g = [g for g in Z.golden() if g["name"] == "text_8000_l19_w12"][0]
    assert Z.expected(by["golden_twice"]["blob"])[1] == g["raw"] * 2


def test_the_borrowed_table_cases_would_decode_with_what_the_frame_before_left():
    """what makes them tests of the reset: carried over, the Huffman table and the three sequence tables decode these blocks"""
    by = {c["name"]: c for c in Z.edge_cases()}
    gold = {g["name"]: g for g in Z.golden()}
    f = R._Frame(b"")
    f.block(Z._blocks(gold["bits3_4000_l1"]["blob"])[0][1])
    before = len(f.out)
    f.block(Z._blocks(by["treeless_with_the_table_of_the_file_before"]["blob"])[0][1])
    assert 0 < len(f.out) - before < 1024 and set(f.out[before:]) <= {0, 1}
    rle_tables = [c for c in Z.crafted() if c["name"] == "rle_tables"][0]
    f = R._Frame(b"")
    f.out += bytes(range(65, 81))
    f.block(Z._blocks(rle_tables["blob"])[1][1])
    assert bytes(f.out) == rle_tables["raw"]
    f.rep[:] = [1, 4, 8]
    del f.out[16:]
    f.block(Z._blocks(by["repeat_mode_with_the_tables_of_the_file_before"]["blob"])[1][1])
    assert bytes(f.out) == rle_tables["raw"]
    for name in ("treeless_with_the_table_of_the_file_before", "treeless_with_the_table_of_the_frame_before",
                 "repeat_mode_with_the_tables_of_the_file_before", "repeat_mode_with_the_tables_of_the_frame_before"):
        assert Z.expected(by[name]["blob"])[0] == "E_ZSTD_DATA"


def test_mutations_are_600_of_three_kinds_from_one_seed():
    mu = Z.mutations()
    assert len(Z.MUTATIONS_LEFT_OUT) <= 4 and len(mu) == Z.MUTATIONS - len(Z.MUTATIONS_LEFT_OUT) and Z.MUTATIONS == 600
    assert [m["blob"] for m in Z.mutations(count=90)] == [m["blob"] for m in mu if m["k"] < 90]       # a shorter run is a prefix
    assert any("_sum" in m["file"] or m["file"] in ("two_frames", "good_frame_for_truncation") for m in mu)   # checksummed frames are in the pool
    sts = set(Z.expected(m["blob"])[0] for m in mu)
    assert {"OK", "E_EOF", "E_ZSTD_MAGIC", "E_ZSTD_HEADER", "E_ZSTD_DATA", "E_ZSTD_CHECKSUM"} <= sts, sts


@needs_lib
def test_edge_cases_and_further_golden_frames_agree_with_libzstd():
    for c in Z.golden_more() + Z.edge_cases():
        st, data, out_len, used = Z.expected(c["blob"], c["dict"])
        ok, ldata, lused = lib_outcome(c["blob"], c["dict"], cap=1 << 21)
        assert ok == (st == "OK"), (c["name"], st)
        if ok:
            assert ldata == data and lused == used, c["name"]


@needs_lib
def test_mutations_agree_with_libzstd():
    mu = Z.mutations()
    assert len(Z.MUTATIONS_LEFT_OUT) <= 4 and len(mu) == Z.MUTATIONS - len(Z.MUTATIONS_LEFT_OUT)
    for m in mu:
        st, data, out_len, used = Z.expected(m["blob"])
        ok, ldata, lused = lib_outcome(m["blob"])
        assert ok == (st == "OK"), (m["name"], st)
        if ok:
            assert ldata == data and lused == used, m["name"]
