"""CPU suite: the plain-Python reference of the LZ4 frame tests (tests/lz4_frame_ref.py) against the published known answers, the
liblz4-made fixtures of tests/golden/lz4_frame and -- where ctypes finds them -- libxxhash and liblz4 themselves."""
import ctypes as C
import struct

import numpy as np
import pytest

import lz4_frame_inputs as I
import lz4_frame_ref as R

XXH32_KAT = [(b"", 0x02CC5D05), (b"a", 0x550D7456), (b"abc", 0x32D153FF), (b"Nobody inspects the spammish repetition", 0xE2293B2F)]
HC_KAT = [(0x64, 0x40, 0xA7), (0x60, 0x40, 0x82), (0x64, 0x70, 0xB9), (0x60, 0x70, 0x73), (0x60, 0x50, 0xFB), (0x40, 0x40, 0xC0)]


@pytest.mark.parametrize("data,want", XXH32_KAT)
def test_xxh32_known_answers(data, want):
    assert R.xxh32(data) == want


@pytest.mark.parametrize("flg,bd,want", HC_KAT)
def test_header_checksum_known_answers(flg, bd, want):
    assert R.header_checksum(bytes([flg, bd])) == want


def test_xxh32_matches_libxxhash_where_installed():
    lib = I.load_lib("xxhash")
    rng = np.random.default_rng(1)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in list(range(0, 70)) + [255, 256, 257, 4095, 4096, 4097, 70001]]
    if lib is None:
        pytest.skip("libxxhash is not installed here: the fixtures' raw_xxh32 (libxxhash's values) are checked either way")
    lib.XXH32.restype = C.c_uint
    lib.XXH32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    for d in datas:
        for seed in (0, 0x9E3779B1):
            assert R.xxh32(d, seed) == lib.XXH32(d, len(d), seed), (len(d), seed)


@pytest.mark.parametrize("fx", I.fixtures(), ids=lambda f: f.name)
def test_reference_decodes_every_fixture_to_the_manifests_data(fx):
    frames = [f for f in R.parse(fx.blob) if not f.skippable]
    entries = [e for e in fx.frames if not e["skippable"]]
    assert len(frames) == len(entries)
    for f, e, raw in zip(frames, entries, fx.raws):
        got = R.decode_frame(f, fx.dictionary)
        assert len(got) == e["raw_len"] and got == raw
        assert R.xxh32(got) == e["raw_xxh32"]                    # (libxxhash's value, recorded when the fixture was made)
        p = e["prefs"]
        assert f.block_size_id == p["block_size_id"] and f.block_checksum == p["block_checksum"]
        assert f.has_content_checksum == p["content_checksum"] and (f.content_size is not None) == p["content_size"]
        assert f.dict_id == p["dict_id"]
        if len(f.blocks) > 1:
            assert f.independent == (not p["linked"])
    assert R.decode(fx.blob, fx.dictionary) == fx.raw


def test_the_fixture_set_covers_what_it_should():
    fx = {f.name: f for f in I.fixtures()}
    par = {n: [f for f in R.parse(x.blob)] for n, x in fx.items()}
    linked = [n for n, fr in par.items() if any(not f.skippable and not f.independent for f in fr)]
    assert len(linked) >= 4
    ids = {f.block_size_id for fr in par.values() for f in fr if not f.skippable}
    assert {4, 5} <= ids
    assert any(f.skippable for f in par["concat_skip"]) and sum(not f.skippable for f in par["concat_skip"]) == 2
    assert par["empty"][0].blocks == []
    assert all(s for s, _, _ in par["stored"][0].blocks) and par["stored"][0].blocks
    assert all(len(x.blob) < 100 << 10 for x in fx.values())


@pytest.mark.parametrize("name", ["linked_b4", "linked_b4_all", "linked_b5_hc", "dict_linked"])
def test_every_linked_fixture_really_uses_history(name):
    """at least one block holds a match whose offset is larger than what the block itself has produced at that point"""
    f = R.parse(I.fixture(name).blob)[0]
    assert not f.independent and len(f.blocks) >= 2
    uses = [R.block_uses_history(p) for s, p, _ in f.blocks if not s]
    assert any(uses[1:]), uses
    # and without the history the block does not decode
    k = 1 + uses[1:].index(True)
    with pytest.raises(R.BlockError):
        R.block_decode(f.blocks[k][1], b"")


def test_dictionary_fixtures_need_their_dictionary():
    for name in ("dict_linked", "dict_indep"):
        fx = I.fixture(name)
        f = R.parse(fx.blob)[0]
        assert R.block_uses_history(f.blocks[0][1])
        with pytest.raises(R.FrameError):
            R.decode_frame(f, None)


def test_build_parse_round_trip_and_error_kinds():
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, 150000, dtype=np.uint8).tobytes()
    blocks = [(True, raw[i:i + 65536]) for i in range(0, len(raw), 65536)]
    blob = R.build(blocks, 4, True, True, R.xxh32(raw), len(raw))
    assert R.decode(blob) == raw
    assert R.decode(blob + R.skippable(b"xyz", 3) + blob) == raw + raw

    def kind(b):
        with pytest.raises(R.FrameError) as e:
            R.decode(b)
        return e.value.kind
    flip = lambda b, at, bit=0: b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]
    assert kind(flip(blob, 14)) == "header_checksum"
    assert kind(flip(blob, 8)) == "header_checksum"               # the content size is under the header checksum
    assert kind(flip(blob, 30)) == "block_checksum"
    assert kind(flip(blob, len(blob) - 1)) == "content_checksum"
    assert kind(blob[:-3]) == "truncated" and kind(blob[:40]) == "truncated" and kind(blob[:5]) == "truncated"
    wrong = R.build(blocks, 4, True, True, R.xxh32(raw), len(raw) + 1)
    assert kind(wrong) == "content_size"
    big = R.build([(True, raw[:65537])], 4)
    assert kind(big) == "block_too_large"
    assert kind(struct.pack("<I", 0x12345678) + blob) == "magic"


def test_block_decoder_with_history_and_its_bounds():
    blocks, raws = I.random_chain(np.random.default_rng(5), 3, b"0123456789" * 50)
    hist = b"0123456789" * 50
    for b, r in zip(blocks, raws):
        assert R.block_decode(b, hist) == r
        hist += r
    import corpus
    one_past = corpus.lz4_stream([(b"abcd", 5, 4 + 10 + 1)], b"tail!")
    ok = corpus.lz4_stream([(b"abcd", 5, 4 + 10)], b"tail!")
    assert R.block_decode(ok, b"0123456789") == b"abcd" + b"01234" + b"tail!"
    with pytest.raises(R.BlockError) as e:
        R.block_decode(one_past, b"0123456789")
    assert e.value.kind == "malformed"
    with pytest.raises(R.BlockError):
        R.block_decode(corpus.lz4_stream([(b"abcd", 5, 0)], b"tail!"), b"0123456789")


def test_liblz4_decodes_what_the_reference_builds_where_installed():
    lz4 = I.load_lib("lz4")
    if lz4 is None:
        pytest.skip("liblz4 is not installed here")
    import oracle_py
    oracle_py.build()
    raw = I.make([["text", 100000, 5]])
    blocks = []
    for i in range(0, len(raw), 65536):
        c = oracle_py.lz4_encode_block(raw[i:i + 65536])
        blocks.append((False, c))
    blob = R.build(blocks, 4, True, True, R.xxh32(raw), len(raw))
    assert I.lz4f_decompress(lz4, blob) == raw
