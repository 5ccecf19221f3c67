"""CPU suite: the XXH32 kernel (k_xxh32.hip) and the linked LZ4 block decoder (k_lz4_linked.hip: k_lz4_decode_v4's decoder with history)
run UNMODIFIED on the wave64 simulator (tests/sim_lz4frame_run.py) and are checked against the plain-Python reference."""
import numpy as np
import pytest

import corpus
import lz4_frame_inputs as I
import lz4_frame_ref as R
import sim_lz4frame_run as S

OK, TOO_SMALL, MALFORMED, HISTORY = 0, 2, 3, 43


def test_xxh32_known_answers_on_the_simulator():
    datas = [b"", b"a", b"abc", b"Nobody inspects the spammish repetition"]
    h, used, st = S.xxh32(datas)
    assert [int(x) for x in h] == [0x02CC5D05, 0x550D7456, 0x32D153FF, 0xE2293B2F]
    assert list(st) == [0] * 4 and [int(u) for u in used] == [len(d) for d in datas]


@pytest.mark.parametrize("seed,lead", [(0, 0), (0x9E3779B1, 0), (0, 1), (7, 3)])
def test_xxh32_lengths_0_to_80_and_around_multiples_of_16(seed, lead):
    rng = np.random.default_rng(seed + lead)
    lens = list(range(0, 81))
    for m in (96, 128, 240, 256, 272, 496, 512, 528, 1024, 4096):      # stripes, and the kernel's 256-byte tiles
        lens += [m - 1, m, m + 1]
    lens += [5000, 70001]
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    h, used, st = S.xxh32(datas, seed, lead)
    assert not st.any()
    bad = [n for n, d, x in zip(lens, datas, h) if R.xxh32(d, seed) != int(x)]
    assert not bad, bad


def test_xxh32_streams_of_one_wave_may_differ_in_length():
    """sixteen streams share a wave: a long one among short and empty ones, and a batch that does not fill its last wave"""
    rng = np.random.default_rng(11)
    lens = [0, 3000, 15, 16, 0, 257, 1, 9000, 255, 256, 31, 32, 33, 0, 700, 17, 4, 600, 0]
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    h, _, st = S.xxh32(datas, 5, 1)
    assert not st.any() and [int(x) for x in h] == [R.xxh32(d, 5) for d in datas]


def _check_chain(out, off, raws, out_len):
    pos = off
    for r, n in zip(raws, out_len):
        assert int(n) == len(r)
        assert bytes(out[pos:pos + len(r)]) == r
        pos += len(r)
    return pos


def test_a_linked_chain_of_three_blocks():
    rng = np.random.default_rng(21)
    blocks, raws = I.random_chain(rng, 3)
    assert any(R.block_uses_history(b) for b in blocks[1:])
    total = sum(map(len, raws))
    st, out_len, in_used, eff, out, out_off, _ = S.decode_linked(blocks, [0, 1, 1], [total, 0, 0])
    assert list(st) == [OK] * 3
    end = _check_chain(out, int(out_off[0]), raws, out_len)
    assert [int(e) for e in eff] == [int(out_off[0]), int(out_off[0]) + len(raws[0]), int(out_off[0]) + len(raws[0]) + len(raws[1])]
    assert [int(u) for u in in_used] == [len(b) for b in blocks]
    assert (out[:int(out_off[0])] == 0xEE).all() and (out[end:] == 0xEE).all()       # nothing outside the head's slot


def test_a_dictionary_block_and_a_chain_behind_a_dictionary():
    rng = np.random.default_rng(22)
    d = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    blocks, raws = I.random_chain(rng, 2, d)
    assert R.block_uses_history(blocks[0])
    total = sum(map(len, raws))
    st, out_len, _, _, out, out_off, dict_off = S.decode_linked(blocks, [0, 1], [total + 9, 0], [d, None])
    assert list(st) == [OK, OK]
    end = _check_chain(out, int(out_off[0]), raws, out_len)
    assert bytes(out[int(dict_off[0]):int(out_off[0])]) == d                               # read, never written
    assert (out[:int(dict_off[0])] == 0xEE).all() and (out[end:] == 0xEE).all()


def test_mixed_batch_heads_chains_and_dictionaries():
    rng = np.random.default_rng(23)
    blocks, link, slots, dicts, want = [], [], [], [], []
    for length, dl in ((1, 0), (4, 700), (2, 0), (1, 70000), (3, 65536)):
        d = rng.integers(0, 256, dl, dtype=np.uint8).tobytes()
        bl, rw = I.random_chain(rng, length, d, nseq=(10, 40))
        total = sum(map(len, rw))
        for k in range(length):
            blocks.append(bl[k]); link.append(1 if k else 0); slots.append(total if not k else 0); dicts.append(d[-65536:] if not k else None)
        want.append(rw)
    st, out_len, _, _, out, out_off, _ = S.decode_linked(blocks, link, slots, dicts)
    assert not st.any()
    j = 0
    for rw in want:
        _check_chain(out, int(out_off[j]), rw, out_len[j:j + len(rw)])
        j += len(rw)


def test_an_offset_one_byte_past_the_history_and_the_rest_of_its_chain():
    d = bytes(range(10, 20))
    good = corpus.lz4_stream([(b"abcd", 5, 4 + 10)], b"tail!")                  # reaches the dictionary's first byte
    bad = corpus.lz4_stream([(b"abcd", 5, 4 + 10 + 1)], b"tail!")               # one byte further
    nxt = corpus.lz4_stream([(b"xy", 4, 3)], b"12345")
    # chain A: good, then one byte past produced + dictionary, then two more; chain B (no dictionary): untouched by A's failure
    past2 = corpus.lz4_stream([(b"abcd", 5, 4 + 14 + 10 + 1)], b"tail!")
    blocks = [good, past2, nxt, nxt, bad, good, nxt]
    link = [0, 1, 1, 1, 0, 0, 1]
    st, out_len, in_used, _, out, out_off, _ = S.decode_linked(blocks, link, [100, 0, 0, 0, 100, 100, 0], [d, None, None, None, d, d, None])
    assert list(st) == [OK, MALFORMED, HISTORY, HISTORY, MALFORMED, OK, OK]
    assert [int(x) for x in out_len] == [14, 0, 0, 0, 0, 14, 11]
    assert bytes(out[int(out_off[0]):int(out_off[0]) + 14]) == R.block_decode(good, d)
    assert bytes(out[int(out_off[5]):int(out_off[5]) + 25]) == R.block_decode(good, d) + R.block_decode(nxt, R.block_decode(good, d))
    # exactly at the bound it decodes
    at = corpus.lz4_stream([(b"abcd", 5, 4 + 14 + 10)], b"tail!")
    st2, ol2, _, _, out2, oo2, _ = S.decode_linked([good, at], [0, 1], [100, 0], [d, None])
    assert list(st2) == [OK, OK] and bytes(out2[int(oo2[0]) + 14:int(oo2[0]) + 28]) == R.block_decode(at, d + R.block_decode(good, d))
    # a zero offset
    z = corpus.lz4_stream([(b"abcd", 5, 0)], b"tail!")
    assert list(S.decode_linked([z], [0], [100], [d])[0]) == [MALFORMED]


def test_a_chain_one_byte_over_its_heads_capacity():
    rng = np.random.default_rng(25)
    blocks, raws = I.random_chain(rng, 3, nseq=(10, 30))
    total = sum(map(len, raws))
    st, out_len, _, _, out, out_off, _ = S.decode_linked(blocks + blocks, [0, 1, 1, 0, 1, 1], [total - 1, 0, 0, total, 0, 0])
    assert list(st) == [OK, OK, TOO_SMALL, OK, OK, OK]
    assert int(out_len[2]) == 0
    _check_chain(out, int(out_off[0]), raws[:2], out_len[:2])
    end = _check_chain(out, int(out_off[3]), raws, out_len[3:])
    assert (out[int(out_off[0]) + total - 1:int(out_off[3])] == 0xEE).all() and (out[end:] == 0xEE).all()


def test_real_linked_blocks_from_liblz4():
    """the second block of the dictionary fixture: 64 KiB of dictionary and of chain in front of it"""
    fx = I.fixture("dict_linked")
    f = R.parse(fx.blob)[0]
    blocks = [p for _, p, _ in f.blocks]
    st, out_len, _, _, out, out_off, _ = S.decode_linked(blocks, [0, 1], [len(fx.raw), 0], [fx.dictionary[-65536:], None])
    assert list(st) == [OK, OK]
    assert bytes(out[int(out_off[0]):int(out_off[0]) + len(fx.raw)]) == fx.raw
