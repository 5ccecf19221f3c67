"""tests/zstd_ref.py, the plain-Python Zstandard decoder the other Zstandard tests take as their oracle, against the golden frames'
recipes, the crafted frames' expectations and -- where ctypes finds libzstd -- libzstd itself (1.4.8 wrote the golden frames): bytes
and accept / reject equal ZSTD_decompress / ZSTD_decompress_usingDict frame by frame, in_used comes from ZSTD_findFrameCompressedSize.
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
