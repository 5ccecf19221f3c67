"""CPU suite: the DEFLATE encoder (levels 2..9) and decoder with history (k_deflate_hc_hist.hip behind k_deflate_hc.hip,
k_inflate_hist.hip behind k_inflate2.hip, UNMODIFIED, on the wave64 simulator).  Encode: the chains and candidates are the plain
references' of tests/hc_stages.py taken over history || block, every stream is read by libz given the history as its dictionary,
no distance leaves block and history, without a history the bytes are the level encoder's.  Decode: libz's streams written with
zdict= and hand-assembled ones, with sentinels around every slot.  tests/deflate_hist_cases.py holds the inputs.  (On a GPU,
tests/test_gpu_deflate_hist.py checks the device's bytes against the simulator's.)"""
import zlib

import numpy as np
import pytest

import deflate_hist_cases as K
import hc_stages as H

LEVELS = K.LEVELS
WIN = 32768


@pytest.fixture(scope="module")
def S():
    import sim_deflate_hist_run as S
    S.build()
    return S


@pytest.fixture(scope="module")
def runs(S):
    B = K.batch()
    inb = B.array()
    jobs = {(lv, stop): ("run", (inb, B.in_off, B.lens, B.hist_len, lv), {"caps": B.caps, "stop_after": stop})
            for lv in sorted(LEVELS, reverse=True) for stop in (S.ALL, S.SEARCH)}
    res = dict(zip(jobs, S.run_many(list(jobs.values()))))
    for k, r in res.items():
        assert r[0] == 0, k
    return B, res


@pytest.fixture(scope="module")
def refs():
    """the reference chains of every history || block, and its reference candidates per depth.  ref_search ends a match at the
    multiples of 65536 of ITS input (a segment is a DEFLATE block), so every segment of the block is handed to it at such a
    multiple: zero bytes without links, the window (the 32768 bytes of history || block before the segment), the segment"""
    B = K.batch()
    virt = [B.history(i) + B.block(i) for i in range(len(B.names))]
    links = [H.ref_links(v, WIN) for v in virt]
    cands = {}

    def cand(i, depth):
        if (i, depth) not in cands:
            h, n, parts = B.hist_len[i], B.lens[i], []
            for s0 in range(0, n, K.SEG):
                e = h + min(s0 + K.SEG, n)
                w = min(WIN, h + s0)
                raw = bytes(K.SEG - w) + virt[i][h + s0 - w:e]
                lk = np.concatenate([np.zeros(K.SEG - w, np.uint16), links[i][h + s0 - w:e]])
                parts.append(H.ref_search(raw, lk, WIN, depth, 0)[K.SEG:])
            cands[(i, depth)] = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        return cands[(i, depth)]
    return links, cand


def test_cases_are_what_they_say(refs):
    B = K.batch()
    _, cand = refs
    i = B.index("slice first")
    c = cand(i, 256)                            # (at depth 4 the nearest member of a bucket of random data is rarely the match)
    assert B.hist_len[i] == 32768 and (int(c[0]) & 0xFFFF) + 1 == 32768 and int(c[0]) >> 16 == 258
    i = B.index("slice last")
    assert (int(cand(i, 256)[0]) & 0xFFFF) + 1 == 1000
    i = B.index("run")
    assert int(cand(i, 4)[0]) == (200 << 16 | 0)
    x, y = B.index("bait x"), B.index("bait y")
    assert B.block(x) == B.block(y) and B.history(x) == B.history(y) and B.hist_len[x] == 2000
    assert bytes(B.buf[B.in_off[x] - 3000:B.in_off[x] - 2000]) == B.block(x) != bytes(B.buf[B.in_off[y] - 3000:B.in_off[y] - 2000])
    c = cand(x, 256)                            # (what the history offers at position 400; the bytes in front of it: 258 there too)
    assert int(c[0]) == (258 << 16 | 1999) and 100 <= int(c[400]) >> 16 < 104 and (int(c[400]) & 0xFFFF) + 1 == 2000
    assert [B.hist_len[B.index("chain[%d]" % k)] for k in range(5)] == [0, 3000, 6000, 9000, 12000]
    assert set(K.HISTS) <= set(B.hist_len) and set(K.LENS) <= set(B.lens)
    assert {(B.in_off[i] - B.hist_len[i]) % 4 for i in range(len(K.HISTS) * len(K.LENS))} >= {1, 2, 3}


@pytest.mark.parametrize("level", LEVELS)
def test_chains(runs, refs, level):
    """the links of the history and of the block: the reference's over history || block"""
    B, res = runs
    links, _ = refs
    views = res[(level, 0xFFFFFFFF)][5]
    for i, name in enumerate(B.names):
        if views[i] is None:
            assert B.lens[i] == 0, name
            continue
        bad = np.flatnonzero(views[i]["link"] != links[i])
        assert not len(bad), (name, "link[%d] = %d, the reference %d" % (bad[0], views[i]["link"][bad[0]], links[i][bad[0]]))


@pytest.mark.parametrize("level", LEVELS)
def test_search(S, runs, refs, level):
    B, res = runs
    _, cand = refs
    views = res[(level, S.SEARCH)][5]
    for i, name in enumerate(B.names):
        if views[i] is None:
            continue
        want = cand(i, H.DH_DEPTH[level])
        bad = np.flatnonzero(views[i]["cand"] != want)
        assert not len(bad), (name, "cand[%d] = %#x, the reference %#x" % (bad[0], views[i]["cand"][bad[0]], want[bad[0]]))
    i = B.index("slice first")                  # all 32768 history bytes are within reach: the distance at position 0 is 32768
    if level == 9:
        assert (int(views[i]["cand"][0]) & 0xFFFF) + 1 == 32768


@pytest.mark.parametrize("level", LEVELS)
def test_streams(runs, level):
    """statuses; every stream is read by libz behind its history, and no distance leaves block and history"""
    B, res = runs
    rc, outs, st, out_len, in_used, _, out, out_off = res[(level, 0xFFFFFFFF)]
    used_history = 0
    for i, name in enumerate(B.names):
        if name == "small slot":
            assert st[i] == K.E_OUTPUT_TOO_SMALL and out_len[i] == 0 and in_used[i] == 0
            o = int(out_off[i])
            assert (out[o:o + B.caps[i]] == 0xEE).all(), "a slot that is too small was written to"
            continue
        hist, blk, n = B.history(i), B.block(i), B.lens[i]
        assert st[i] == 0 and in_used[i] == n and len(outs[i]) <= K.bound(n), name
        d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
        assert d.decompress(outs[i]) == blk and d.eof and not d.unused_data, name
        pos = 0
        for blkk in H.inflate_tokens(outs[i]):
            for ln, x in blkk["tokens"]:
                if ln:
                    assert 1 <= x <= min(32768, pos + len(hist)), (name, pos, x)
                    used_history += x > pos
                pos += ln or 1
        assert pos == n, name
    assert used_history >= 100
    assert outs[B.index("bait x")] == outs[B.index("bait y")]
    for name in ("slice first", "slice last"):                      # (incompressible without the history: more than 1000 bytes)
        assert len(outs[B.index(name)]) < 30, name


@pytest.mark.parametrize("level", LEVELS)
def test_bait_stages(S, runs, level):
    """the bytes in front of the history influence neither the chains nor the candidates"""
    B, res = runs
    x, y = B.index("bait x"), B.index("bait y")
    for stop in (0xFFFFFFFF, S.SEARCH):
        vx, vy = res[(level, stop)][5][x], res[(level, stop)][5][y]
        assert (vx["link"] == vy["link"]).all()
    assert (res[(level, S.SEARCH)][5][x]["cand"] == res[(level, S.SEARCH)][5][y]["cand"]).all()


def test_more_items_than_the_links_grid(S):
    B = K.many_batch()
    assert len(B.names) + sum(1 for n in B.lens if n) > 8192
    rc, outs, st, out_len, in_used, views, _, _ = S.run(B.array(), B.in_off, B.lens, B.hist_len, 2, caps=B.caps, fill=None)
    assert rc == 0 and not st.any()
    used = 0
    for i, name in enumerate(B.names):
        hist, blk = B.history(i), B.block(i)
        d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
        assert d.decompress(outs[i]) == blk, name
        if blk:
            assert (views[i]["link"] == H.ref_links(hist + blk, WIN)).all(), name
            used += len(outs[i]) < 40
    assert used == 12                                                # (64 bytes that repeat their history: a few matches)


@pytest.mark.parametrize("level", LEVELS)
def test_empty_histories_are_the_level_encoder(S, level):
    """with no history (hist_len null, or all 0) the bytes are sim_deflate_hc's at that level, raw and zlib"""
    import sim_deflate_hc_run as S0
    B = K.batch()
    pick = [i for i, nm in enumerate(B.names) if (nm.startswith("h0 ") and nm != "h0 n65536") or nm == "chain[0]"]
    raws = [B.block(i) for i in pick]
    for fmt in (0, 1):
        rc0, outs0, st0, ol0, iu0 = S0.encode(raws, fmt, level)
        assert rc0 == 0 and not st0.any()
        for null in (True, False):
            rc, outs, st, out_len, in_used, _, _, _ = S.encode(raws, [None] * len(raws), level, leads=3, fmt=fmt, null_hist=null,
                                                                 dict_id=[0] * len(raws))
            assert rc == 0 and not st.any() and outs == outs0 and (out_len == ol0).all() and (in_used == iu0).all(), (fmt, null)


@pytest.mark.parametrize("level", LEVELS)
def test_zlib_form(S, level):
    """FDICT, FLEVEL, FCHECK, DICTID and the Adler-32 of the block alone; libz reads the stream given the dictionary; a block without
    history in the same batch has no FDICT and is the plain level encoder's stream"""
    import sim_deflate_hc_run as S0
    t = K.text(40000, 82)
    long_dict = K.rand(5000, 83) + t[:32768]                         # (the decoder's dictionary may be longer than what counts)
    blocks = [t[32768:], t[33000:34000], b"", t[32768:], b"abc"]
    hists = [t[:32768], t[32000:33000], t[:100], None, b"abcabc"]
    ids = [zlib.adler32(long_dict), zlib.adler32(hists[1]), zlib.adler32(hists[2]), 0xDEADBEEF, zlib.adler32(hists[4])]
    rc, outs, st, out_len, in_used, _, out, out_off = S.encode(blocks, hists, level, leads=2, fmt=1, dict_id=ids)
    assert rc == 0 and not st.any()
    flevel = 1 if level <= 5 else 2 if level == 6 else 3
    for i, (b, h) in enumerate(zip(blocks, hists)):
        o = outs[i]
        assert o[0] == 0x78 and (o[0] * 256 + o[1]) % 31 == 0 and o[1] >> 6 == flevel, i
        assert o[-4:] == zlib.adler32(b).to_bytes(4, "big"), i
        if h:
            assert o[1] & 0x20 and o[2:6] == ids[i].to_bytes(4, "big"), i
            d = zlib.decompressobj(zdict=long_dict if i == 0 else h)
            assert d.decompress(o) == b and d.eof, i
            raw = zlib.decompressobj(-15, zdict=h)
            assert raw.decompress(o[6:-4]) == b, i
        else:
            assert not o[1] & 0x20 and zlib.decompress(o) == b, i
    rc0, outs0, st0, _, _ = S0.encode([blocks[3]], 1, level)
    assert outs[3] == outs0[0]
    # the raw stream of the same batch: the zlib form's DEFLATE data, byte for byte
    rc, raws, st, _, _, _, _, _ = S.encode(blocks, hists, level, leads=2)
    assert [o[6 if h else 2:-4] for o, h in zip(outs, hists)] == raws
    # a slot that holds the raw stream and not the ten bytes around it
    caps = [len(raws[0]) + 9, S.bound(1000, 1)]
    rc, outs2, st, out_len, _, _, out, out_off = S.encode(blocks[:2], hists[:2], level, leads=2, fmt=1, dict_id=ids[:2], caps=caps)
    assert list(st) == [K.E_OUTPUT_TOO_SMALL, 0] and out_len[0] == 0 and (out[:caps[0]] == 0xEE).all() and outs2[1] == outs[1]


@pytest.mark.parametrize("level", LEVELS)
def test_what_a_history_buys(S, level):
    """every record is smaller behind the dictionary than alone, and linked chunks total less than independent ones (libz alone meets
    both: 0.63-0.70 of the size per record, 0.92 of the total for the chunks at level 6)"""
    recs, dic, chunks, whole = K.what_history_buys()
    inb = np.frombuffer(b"\xC3" + whole + b"\0" * 16, np.uint8).copy()
    off = [1 + K.SEG * k for k in range(len(chunks))]
    lens = [len(c) for c in chunks]
    with_d, alone, linked, indep = S.run_many([("encode", (recs, [dic] * 16, level), {"leads": 1}),
                                               ("encode", (recs, [None] * 16, level), {"leads": 1}),
                                               ("run", (inb, off, lens, [min(32768, o - 1) for o in off], level), {}),
                                               ("run", (inb, off, lens, [0] * len(off), level), {})])
    assert not with_d[2].any() and not alone[2].any()
    a, b = [len(o) for o in with_d[1]], [len(o) for o in alone[1]]
    print("level %d records with dictionary %s alone %s" % (level, a, b))
    assert all(x < y for x, y in zip(a, b)), (a, b)
    assert not linked[2].any() and not indep[2].any()
    la, lb = sum(len(o) for o in linked[1]), sum(len(o) for o in indep[1])
    print("level %d chunks linked %d independent %d" % (level, la, lb))
    assert la < lb
    for k, o in enumerate(linked[1]):
        h = whole[max(0, K.SEG * k - 32768):K.SEG * k]
        d = zlib.decompressobj(-15, zdict=h) if h else zlib.decompressobj(-15)
        assert d.decompress(o) == chunks[k]


# ---------------------------------------------------------------------------------------------------------------------------- decode
@pytest.fixture(scope="module")
def decoded(S):
    cs = K.decode_cases()
    args = ([c["stream"] for c in cs], [c["hist"] for c in cs], [c["cap"] for c in cs])
    kw = {"fronts": [c["front"] for c in cs], "misalign": [i % 16 for i in range(len(cs))]}
    with_h, told_none, plain = S.run_many([("inflate", args, kw), ("inflate", args, dict(kw, hist_len=[0] * len(cs))),
                                           ("inflate", args, dict(kw, hist_kernel=False))])
    return cs, with_h, told_none, plain


def test_decode_cases_are_what_they_say():
    cs = {c["name"]: c for c in K.decode_cases()}
    assert {len(c["hist"]) for c in cs.values()} >= set(K.HISTS)
    for name, c in cs.items():                                        # libz is the oracle of the hand-assembled streams too
        if c["status"] in (0, K.E_INVALID_HUFFMAN_CODE):
            got = K.libz_raw(c["hist"], c["stream"])
            assert got == (c["want"] if c["status"] == 0 else None), name
    assert cs["d32768 h32768 p1"]["status"] == 0 and cs["d32768 h32767 p0"]["status"] == K.E_INVALID_HUFFMAN_CODE
    # distances 1, 2 and 3 at output position 0 (the seeded ring alone), and a far gather that straddles the slot's first byte (the
    # other fourteen splits: the "end residue" cases of dict_decode_cases.py, which test_wavesim_dict_decode.py runs through this kernel)
    assert all(cs["first match d%d" % d]["status"] == 0 and len(cs["first match d%d" % d]["hist"]) >= d for d in (1, 2, 3))
    assert -1 in K.far_gathers(K.first_match_tokens(113)) and cs["first match d113"]["status"] == 0


def test_decode(decoded):
    cs, (outs, out_len, in_used, st, flags), _, _ = decoded
    for i, c in enumerate(cs):
        assert st[i] == c["status"], (c["name"], st[i])
        assert outs[i] == c["want"] and out_len[i] == len(c["want"]), c["name"]
        assert flags[i] == 0, c["name"]
        if c["status"] == 0:
            assert in_used[i] == len(c["stream"]), c["name"]
        else:
            assert in_used[i] <= len(c["stream"]), c["name"]
    by = {c["name"]: i for i, c in enumerate(cs)}
    assert outs[by["front x"]] == outs[by["front y"]]


def test_decode_without_history_is_k_inflate2(decoded):
    """told no history, the kernel gives what k_inflate2 gives on the same streams: the bytes of those that need none, the same error
    (a distance beyond the output so far) at the same place for the others"""
    cs, _, a, b = decoded
    for k in range(5):
        assert (np.asarray(a[k]) == np.asarray(b[k])).all() if k else a[k] == b[k], k
    assert sum(1 for s in a[3] if s == K.E_INVALID_HUFFMAN_CODE) > 20 and sum(1 for s in a[3] if s == 0) > 30


def test_zlib_decode(S):
    cs = K.zlib_decode_cases()
    outs, out_len, in_used, st, flags = S.inflate([c["stream"] for c in cs], [c["hist"] for c in cs], [len(c["want"]) + 5 for c in cs],
                                                  zlib=True, dict_id=[c["dict_id"] for c in cs], hist_len=[c["told"] for c in cs],
                                                  misalign=[3 * i for i in range(len(cs))])
    for i, c in enumerate(cs):
        assert st[i] == c["status"] and outs[i] == c["want"], (c["name"], st[i], out_len[i])
        assert in_used[i] == (len(c["stream"]) if c["in_used"] is None else c["in_used"]), (c["name"], in_used[i])
    # without lengths: k_inflate2's answers
    a = S.inflate([c["stream"] for c in cs], [c["hist"] for c in cs], [len(c["want"]) + 5 for c in cs], zlib=True, hist_len=[0] * len(cs))
    b = S.inflate([c["stream"] for c in cs], [c["hist"] for c in cs], [len(c["want"]) + 5 for c in cs], zlib=True, hist_kernel=False)
    for k in range(5):
        assert (np.asarray(a[k]) == np.asarray(b[k])).all() if k else a[k] == b[k], k
    assert list(a[3][:3]) == [K.E_ZLIB_DICT] * 3


# ------------------------------------------------------------------------------------------------------------------------------- ABI
def test_abi():
    import ctypes as C
    from rust_compress_amd import _native as N
    L = N.lib()
    for name in ("rcx_deflate_encode_hist_batch", "rcx_zlib_encode_dict_batch", "rcx_deflate_hist_scratch_bytes", "rcx_inflate_hist_batch",
                 "rcx_zlib_decode_dict_batch"):
        assert hasattr(L, name), name
    assert L.rcx_status_string(25) == b"zlib dictionary id mismatch"
    assert L.rcx_deflate_hist_scratch_bytes(4, 65536) > L.rcx_deflate_level_scratch_bytes(4, 65536) + 4 * 131072
