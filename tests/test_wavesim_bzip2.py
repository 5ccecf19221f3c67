"""The bzip2 decoder (rcx_bzip2_decode_batch: k_bzip2.hip's kernels and launch loop, rcx_plan_bz2_chain, the inverse BWT they call) on the
wave64 simulator against libbz2 read strictly (tests/bz2_cases.py); the generator of crafted streams and the CRC identity in plain
Python.  No GPU needed."""
import bz2
import zlib

import numpy as np
import pytest

import bz2_cases as BC
import bz2_craft as K
import sim_bzip2_run as S


def check_against_oracle(names, blobs, r, caps):
    """status is nonzero exactly where the strict oracle raises; bytes, out_len and in_used are equal where it does not"""
    assert r["rc"] == 0, r["err"]
    for i, (name, blob) in enumerate(zip(names, blobs)):
        want = BC.expected(blob)
        st = int(r["status"][i])
        if want is None:
            assert st not in (BC.OK, BC.E_TOO_SMALL), (name, st)
            assert int(r["out_len"][i]) == 0 and int(r["in_used"][i]) == 0, name
        else:
            assert st == BC.OK, (name, st)
            assert int(r["out_len"][i]) == len(want[0]) and int(r["in_used"][i]) == want[1], name
            assert r["data"][i] == want[0], name
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])


def caps_for(blobs, spare=0):
    return [len(e[0]) + spare if e else 64 for e in map(BC.expected, blobs)]


@pytest.fixture(scope="module")
def named_run():
    names, blobs = zip(*BC.named())
    caps = caps_for(blobs)
    return names, blobs, caps, S.run(blobs, caps)


def test_named_inputs_against_the_strict_oracle(named_run):
    """every input of the issue's list in ONE call, slots of exactly the decoded size: empty and one byte, all 256 values, two and three
    blocks with bit-unaligned starts, runs on both sides of every count, 2 MiB of zeros, crafted tables and counts, concatenated
    streams, trailing bytes, 16 truncations"""
    names, blobs, caps, r = named_run
    check_against_oracle(names, blobs, r, caps)
    assert r["rounds"] == 1


def test_statuses_name_the_failure(named_run):
    names, blobs, caps, r = named_run
    st = dict(zip(names, (int(s) for s in r["status"])))
    assert st["stream_then_header"] == BC.E_EOF and st["no_stream_end"] == BC.E_EOF and st["nothing"] == BC.E_EOF and st["short"] == BC.E_EOF
    assert st["bad_magic"] == BC.E_MAGIC and st["bad_level"] == BC.E_MAGIC
    assert st["bad_block_crc"] == BC.E_BLOCK_CRC and st["bad_stream_crc"] == BC.E_STREAM_CRC
    for k in ("selector_ge_ngroups", "too_few_selectors", "origptr_eq_nblock", "craft_end4"):
        assert st[k] == BC.E_DATA, k
    assert st["trunc3"] == BC.E_EOF and st["trunc4"] == BC.E_EOF and st["trunc7"] == BC.E_EOF
    assert all(st[k] == BC.E_EOF for k in st if k.startswith("trunc")), {k: v for k, v in st.items() if k.startswith("trunc")}


def test_randomised_blocks_are_refused():
    r = S.run([BC.randomised(), bz2.compress(b"after")], [200, 5])
    assert list(r["status"]) == [BC.E_RANDOMISED, BC.OK] and r["data"][1] == b"after" and int(r["out_len"][0]) == 0


def test_a_mark_inside_data_is_reported_and_dropped():
    """the symbol stream of one block spells the block mark, that of the next the stream-end mark, off byte boundaries: the scan reports
    both, the walk passes them by, and libbz2 decodes the file"""
    blob, where = BC.marks_inside()
    want = BC.strict(blob)
    r = S.run([blob], [len(want[0])])
    assert r["rc"] == 0 and int(r["status"][0]) == BC.OK and r["data"][0] == want[0] and int(r["in_used"][0]) == want[1]
    assert where[0] % 8 and where[1] % 8
    blocks = [bit for f, bit, kind, _ in r["cands"] if kind == "block"]
    ends = [bit for f, bit, kind, _ in r["cands"] if kind == "end"]
    assert where[0] in blocks and len(blocks) == 3
    assert where[1] in ends and len(ends) == 2
    live = [bit for f, bit in r["live"]]
    assert len(live) == 2 and where[0] not in live and live == [b for b in blocks if b != where[0]]
    assert [c[1] for c in r["cands"]] == sorted(c[1] for c in r["cands"])


def test_size_query_and_exact_retry(named_run):
    """caps of 0: RCX_E_OUTPUT_TOO_SMALL with the exact size for every file that decodes to something, the failures unchanged, nothing
    written; the retry with those sizes fills the slots to the byte"""
    names, blobs, caps, full = named_run
    keep = [i for i, k in enumerate(names) if not k.startswith(("text250000", "trunc"))]
    names, blobs = [names[i] for i in keep], [blobs[i] for i in keep]
    q = S.run(blobs, [0] * len(blobs))
    assert q["rc"] == 0 and (q["out"] == 0xEE).all()
    sizes = []
    for i, blob in enumerate(blobs):
        want = BC.expected(blob)
        st = int(q["status"][i])
        if want is None:
            assert st == int(full["status"][keep[i]]) and int(q["out_len"][i]) == 0, names[i]
        elif len(want[0]) == 0:
            assert st == BC.OK and int(q["in_used"][i]) == want[1]
        else:
            assert st == BC.E_TOO_SMALL and int(q["out_len"][i]) == len(want[0]), names[i]
        sizes.append(int(q["out_len"][i]))
    check_against_oracle(names, blobs, S.run(blobs, sizes), sizes)
    one_short = [max(s - 1, 0) for s in sizes]
    r = S.run(blobs, one_short)
    assert all(int(r["status"][i]) == BC.E_TOO_SMALL and int(r["out_len"][i]) == s for i, s in enumerate(sizes) if s)
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])


def test_single_bit_flips(named_run):
    """the two-block level-1 file with 200 seeded single-bit flips: a nonzero status exactly where the strict oracle raises, the same bytes
    where it does not -- every flip compared"""
    fl = BC.flips()
    assert len(fl) == 200
    names, blobs = ["flip%d" % b for b, _ in fl], [b for _, b in fl]
    caps = caps_for(blobs, spare=3)
    r = S.run(blobs, caps)
    check_against_oracle(names, blobs, r, caps)
    assert sum(1 for b in blobs if BC.expected(b) is None) >= 190


def test_more_candidates_than_a_round():
    """600 small level-1 files in one call: two rounds of block candidates, the results those of one file at a time; the slots are sized
    by the level the headers name"""
    blobs = [bz2.compress(b"file %d " % i * (i % 7 + 1), 1) for i in range(600)]
    caps = caps_for(blobs)
    r = S.run(blobs, caps, round=512)
    check_against_oracle(["f%d" % i for i in range(600)], blobs, r, caps)
    assert r["rounds"] == 2 and r["scratch"] < (300 << 20)            # (level-9 slots alone would be 920 MB)
    one = S.run(blobs, caps)                                          # the library's own round size takes them at once
    assert one["rounds"] == 1 and one["data"] == r["data"] and list(one["in_used"]) == list(r["in_used"])


def test_refusals():
    """more files than a grid dimension takes, a round size out of range: refused by name before anything is launched"""
    r = S.run([b""] * 65536, [0] * 65536)
    assert r["rc"] == -1 and "65535" in r["err"] and r["launches"] == 0
    for bad in (1, 63, 4097):
        r = S.run([bz2.compress(b"x")], [1], round=bad)
        assert r["rc"] == -1 and "round" in r["err"] and r["launches"] == 0
    assert S.run([bz2.compress(b"x")], [1], round=64)["data"] == [b"x"]


def test_the_known_difference_from_libbz2():
    """a crafted L whose cycle through origPtr does not divide the block's length: libbz2 decodes it, this library reports a block CRC
    (DESIGN.md 3.20, step 4); the file beside it is not affected"""
    blob, plain = BC.short_cycle()
    assert BC.strict(blob)[0] == plain
    r = S.run([blob, bz2.compress(b"beside")], [len(plain), 6])
    assert list(r["status"]) == [BC.E_BLOCK_CRC, BC.OK] and int(r["out_len"][0]) == 0 and r["data"][1] == b"beside"


def test_crafted_streams_round_trip_through_libbz2():
    """bz2_craft.py's streams are what libbz2 reads: the model's text comes back (where libbz2 takes the block at all)"""
    for t in (b"banana", b"abracadabra" * 7, bytes(range(256)), b"ab" + b"cccc" + bytes([255]) + b"de", b"k" + bytes([5]) * 9 + b"m", b"abcab" * 6):
        s, plain = K.stream(5, [K.block_from_text(t)])
        assert bz2.decompress(s) == plain == K.unrle(t)
    s, plain = K.stream(2, [K.block_from_text(K.rle1(b"x" * 700 + b"yz")), K.block_from_text(b"second block")])
    assert bz2.decompress(s) == plain == b"x" * 700 + b"yz" + b"second block"
    syms = K.l_to_symbols(b"aaaaaaabbbab", b"ab")
    assert K.symbols_to_l(syms, b"ab") == b"aaaaaaabbbab"
    for k, blob in BC.named():
        if k in ("craft_count255", "craft_count_own", "craft_periodic", "tables2", "tables6", "len_1_20_incomplete", "oversubscribed", "marks_inside"):
            assert BC.expected(blob) is not None, k
    with pytest.raises(OSError):
        BC.strict(bz2.compress(b"one") + bz2.compress(b"two")[:-3] + b"\0\0\0")
    assert bz2.decompress(bz2.compress(b"one") + b"BZh9" + b"\0" * 20) == b"one"     # (what the strict helper is for)


def test_crc_identity():
    """crc_bz2(d) == bitrev32(crc32(bitrev8 of every byte of d)): what lets the block CRCs ride on CRC-32's x^n mod P combining"""
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 7, 64, 1000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert K.crc_bz2(d) == K.bitrev32(zlib.crc32(bytes(K.bitrev8(b) for b in d)))
    assert K.crc_bz2(b"123456789") == 0xFC891918
