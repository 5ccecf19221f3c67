"""CPU suite: the LZ4 HC encoder with history (k_lz4_hc.hip + k_lz4_hc_hist.hip, UNMODIFIED, on the wave64 simulator) against the
plain references of tests/hc_stages.py taken over history || block: the chains and candidates at the block's positions are the
reference's behind the history, every block decodes behind its history, and is no larger than the greedy parse over the reference's
candidates.  tests/lz4_hist_cases.py holds the batch.  (On a GPU, tests/test_gpu_lz4_hist.py checks the device's bytes against the
simulator's.)"""
import numpy as np
import pytest

import hc_stages as H
import lz4_frame_ref as F
import lz4_hist_cases as K

SEARCH = 4                                  # stop_after: plan, hist_plan, links, search (k_hc_parse overwrites cand)
ALL = 0xFFFFFFFF
LEVELS = K.LEVELS


@pytest.fixture(scope="module")
def runs():
    import sim_lz4hist_run as S
    B = K.batch()
    inb = B.array()
    jobs = {(lv, stop): ("run", (inb, B.in_off, B.lens, B.hist_len, lv), {"caps": B.caps, "stop_after": stop})
            for lv in sorted(LEVELS, reverse=True) for stop in (ALL, SEARCH)}
    res = dict(zip(jobs, S.run_many(list(jobs.values()))))
    for k, r in res.items():
        assert r[0] == 0, k
    return B, res


@pytest.fixture(scope="module")
def refs():
    """the reference chains of every history || block, and its reference candidates per depth"""
    B = K.batch()
    virt = [B.history(i) + B.block(i) for i in range(len(B.names))]
    links = [H.ref_links(v, H.HC_WIN) for v in virt]
    cands = {}

    def cand(i, depth):
        if (i, depth) not in cands:
            cands[(i, depth)] = H.ref_search(virt[i], links[i], H.HC_WIN, depth, 1)
        return cands[(i, depth)]
    return links, cand


def test_cases_are_what_they_say(refs):
    B = K.batch()
    _, cand = refs
    i = B.index("slice first")
    c = cand(i, 256)                            # (at depth 1 the nearest member of a bucket of random data is rarely the match)
    assert B.hist_len[i] == 65535 and int(c[65535]) & 0xFFFF == 65535 and int(c[65535]) >> 16 == 1000 - 5
    i = B.index("slice last")
    assert int(cand(i, 256)[65535]) & 0xFFFF == 1000
    i = B.index("run")
    assert int(cand(i, 1)[7]) == (195 << 16 | 1)
    x, y = B.index("bait x"), B.index("bait y")
    assert B.block(x) == B.block(y) and B.history(x) == B.history(y) and B.hist_len[x] == 2000
    assert bytes(B.buf[B.in_off[x] - 3000:B.in_off[x] - 2000]) == B.block(x) != bytes(B.buf[B.in_off[y] - 3000:B.in_off[y] - 2000])
    assert 500 <= int(cand(x, 256)[2000]) >> 16 < 504               # (what the history offers; the bytes in front of it: all 1000 - 5)
    assert [B.hist_len[B.index("chain[%d]" % k)] for k in range(5)] == [0, 3000, 6000, 9000, 12000]
    assert set(K.HISTS) <= set(B.hist_len) and set(K.LENS) <= set(B.lens)
    assert {(B.in_off[i] - B.hist_len[i]) % 4 for i in range(len(K.HISTS) * len(K.LENS))} >= {1, 2, 3}


@pytest.mark.parametrize("level", LEVELS)
def test_chains(runs, refs, level):
    """the links of the history and of the block: the reference's over history || block"""
    B, res = runs
    links, _ = refs
    views = res[(level, ALL)][5]
    for i, name in enumerate(B.names):
        if views[i] is None:
            assert B.lens[i] == 0 or name == "small slot", name
            continue
        bad = np.flatnonzero(views[i]["link"] != links[i])
        assert not len(bad), (name, "link[%d] = %d, the reference %d" % (bad[0], views[i]["link"][bad[0]], links[i][bad[0]]))


@pytest.mark.parametrize("level", LEVELS)
def test_search(runs, refs, level):
    B, res = runs
    _, cand = refs
    views = res[(level, SEARCH)][5]
    for i, name in enumerate(B.names):
        if views[i] is None:
            continue
        want = cand(i, H.HC_DEPTH[level])[len(B.history(i)):]
        bad = np.flatnonzero(views[i]["cand"] != want)
        assert not len(bad), (name, "cand[%d] = %#x, the reference %#x" % (bad[0], views[i]["cand"][bad[0]], want[bad[0]]))


@pytest.mark.parametrize("level", LEVELS)
def test_blocks(runs, refs, level):
    """statuses; every block decodes behind its history, keeps its offsets inside block and history, and is no larger than the greedy
    parse over the reference's candidates"""
    B, res = runs
    _, cand = refs
    rc, outs, st, out_len, in_used, _ = res[(level, ALL)]
    used_history = 0
    for i, name in enumerate(B.names):
        if name == "small slot":
            assert st[i] == K.E_OUTPUT_TOO_SMALL and out_len[i] == 0 and in_used[i] == 0
            continue
        hist, blk, n = B.history(i), B.block(i), B.lens[i]
        assert st[i] == 0 and in_used[i] == n, name
        assert F.block_decode(outs[i], prefix=hist) == blk, name
        for _, start, ln, dist in H.lz4_block_tokens(outs[i])[:-1]:
            assert 1 <= dist <= min(65535, start + len(hist)), (name, start, dist)
            used_history += dist > start
        greedy = H.ref_lz4_greedy_size(n, cand(i, H.HC_DEPTH[level])[len(hist):])
        assert len(outs[i]) <= greedy, (name, level, "the block has %d bytes, the greedy parse %d" % (len(outs[i]), greedy))
    assert used_history > 100
    assert outs[B.index("bait x")] == outs[B.index("bait y")]
    for name in ("slice first", "slice last"):                      # (incompressible without the history: 1005 bytes)
        assert len(outs[B.index(name)]) < 20, name


@pytest.mark.parametrize("level", LEVELS)
def test_bait_stages(runs, level):
    """the bytes in front of the history influence neither the chains nor the candidates"""
    B, res = runs
    x, y = B.index("bait x"), B.index("bait y")
    for stop in (ALL, SEARCH):
        vx, vy = res[(level, stop)][5][x], res[(level, stop)][5][y]
        assert (vx["link"] == vy["link"]).all()
    assert (res[(level, SEARCH)][5][x]["cand"] == res[(level, SEARCH)][5][y]["cand"]).all()


@pytest.mark.parametrize("level", LEVELS)
def test_empty_histories_are_the_hc_encoder(level):
    """with no history (hist_len null, or all 0) the bytes and the stage arrays are sim_lz4hc_run's"""
    import sim_lz4hc_run as S0
    import sim_lz4hist_run as S
    B = K.batch()
    pick = [i for i, nm in enumerate(B.names) if (nm.startswith("h0 ") and nm != "h0 n65536") or nm == "chain[0]"]      # (0 .. 1000 bytes, two segments)
    raws = [B.block(i) for i in pick]
    for stop0, stop in ((S0.ALL, S.ALL), (3, SEARCH)):
        rc0, outs0, st0, scratch, lay = S0.stages(raws, level, stop0, lead=3)
        want = H.lz4_views(raws, scratch, lay)
        assert rc0 == 0
        for null in (True, False):
            rc, outs, st, out_len, in_used, views = S.encode(raws, [None] * len(raws), level, leads=3, stop_after=stop, null_hist=null)
            assert rc == 0 and (st == st0).all()
            if stop == S.ALL:
                assert outs == outs0 and not st.any()
            for i, r in enumerate(raws):
                if not len(r):
                    assert views[i] is None
                    continue
                for key in ("link", "elen", "seg_nm", "seg_fm", "seg_le") if stop == S.ALL else ("link", "cand"):
                    assert (views[i][key] == want[i][key]).all(), (i, key, null)
