"""CPU suite: the stages of DEFLATE levels 2..9 (k_deflate_hc.hip, UNMODIFIED, on the wave64 simulator) against plain references of
what their header comments claim -- exact hash chains, the longest match within the depth, code lengths that are a complete code, a
min-cost parse, the cheapest block holding the parse's tokens.  The final bytes cannot show a kernel that is a little short of these
(the stream still decodes, a few per cent larger); the stage arrays in the scratch can.  tests/hc_stages.py reads them and holds the
references, tests/hc_inputs.py the inputs.  (On a GPU, tests/test_gpu_hc_stages.py checks the device's arrays against these.)"""
import zlib

import numpy as np
import pytest

import hc_inputs as I
import hc_stages as H

SEG = H.SEG
LEAD = 3                                    # bytes before every stream in the input buffer: odd offsets (unaligned 4-byte loads)
LINKS, SEARCH, PRICE, PARSE, PRICE2, PARSE2 = 2, 3, 4, 5, 6, 7      # stop_after: the launches of sim_deflate_hc_run.LAUNCHES
ALL = 0xFFFFFFFF
# (level, stop_after) of every simulator run: levels 2 and 6 whole (one pass: every stage array survives), level 9 up to its search,
# level 8 up to its first parse and whole (the second pass overwrites price, elen and pos)
CONFIGS = ((8, ALL), (8, PARSE), (6, ALL), (2, ALL), (9, SEARCH))


def batches():
    return {"edges": I.window_cases(H.DE_WIN, 0) + I.group_cases() + I.length_cases(258, H.DH_RING, 0) + I.small_cases()
            + I.depth_cases((4, 64, 256), 0),
            "sizes": I.size_cases(), "synth": I.synth_cases()}


@pytest.fixture(scope="module")
def runs():
    import sim_deflate_hc_run as S
    B = batches()
    jobs = {}
    for lv, stop in CONFIGS:                # (the slowest first)
        for name in ("synth", "sizes", "edges"):
            jobs[(name, lv, stop)] = ("stages", H.deflate_reduce, [c.raw for c in B[name]], lv, stop, LEAD)
    res = dict(zip(jobs, S.encode_many(list(jobs.values()))))
    for k, (rc, outs, st, views) in res.items():
        assert rc == 0 and (k[2] != ALL or not st.any()), k
    return B, res


@pytest.fixture(scope="module")
def refs():
    """the reference chains of every stream, and its reference candidates per depth"""
    B = batches()
    links = {(name, i): H.ref_links(c.raw, H.DE_WIN) for name, cs in B.items() for i, c in enumerate(cs)}
    cands = {}

    def cand(name, i, depth):
        if (name, i, depth) not in cands:
            cands[(name, i, depth)] = H.ref_search(B[name][i].raw, links[(name, i)], H.DE_WIN, depth, 0)
        return cands[(name, i, depth)]
    return links, cand


def _segments(raw):
    return [(s, raw[s:s + SEG]) for s in range(0, len(raw), SEG)]


def test_inputs_hit_their_edges(refs):
    links, cand = refs
    B = batches()
    for i, c in enumerate(B["edges"]):
        lk = links[("edges", i)]
        c.check_edges(lk, cand("edges", i, getattr(c, "depth", 4)), 0)
        if hasattr(c, "depth"):
            # the long match is entry c.entry of the walk: found to that depth, not one short of it; the level's depth lies on the
            # side the case names
            ln = lambda d: int(cand("edges", i, d)[c.p]) >> 16
            assert ln(c.entry) == 24 and (c.entry == 1 or ln(c.entry - 1) == 4), c.name
            assert ln(c.depth) == (24 if c.entry == c.depth else 4), c.name
    # the zeros: a 258-byte candidate at every position, so all four long-length lanes relax at every position and their arrivals
    # cross every multiple of the parse's ring
    z = cand("synth", 1, 4)
    assert (z[:SEG - 258] >> 16 == 258)[1:].all() and B["synth"][1].name == "zeros"


@pytest.mark.parametrize("level", (2, 6, 9))
def test_chains(runs, refs, level):
    B, res = runs
    links, _ = refs
    stop = SEARCH if level == 9 else ALL
    for name, cs in B.items():
        views = res[(name, level, stop)][3]
        for i, c in enumerate(cs):
            bad = np.flatnonzero(views[i]["link"] != links[(name, i)])
            assert not len(bad), (c.name, "link[%d] = %d, the reference %d" % (bad[0], views[i]["link"][bad[0]], links[(name, i)][bad[0]]))


@pytest.mark.parametrize("level", (2, 6, 9))
def test_search(runs, refs, level):
    B, res = runs
    _, cand = refs
    stop = SEARCH if level == 9 else ALL
    for name, cs in B.items():
        views = res[(name, level, stop)][3]
        for i, c in enumerate(cs):
            want = cand(name, i, H.DH_DEPTH[level])
            bad = np.flatnonzero(views[i]["cand"] != want)
            assert not len(bad), (c.name, "cand[%d] = %#x, the reference %#x" % (bad[0], views[i]["cand"][bad[0]], want[bad[0]]))


def _passes(res, name, level):
    """(pass, the parse the prices come from, views holding that pass's price and pos) of a level"""
    if level < 7:
        v = res[(name, level, ALL)][3]
        return [(1, [x["cand"] for x in v], v)]
    v1, v2 = res[(name, level, PARSE)][3], res[(name, level, ALL)][3]
    return [(1, [x["cand"] for x in v1], v1), (2, [x["pos"] for x in v1], v2)]


@pytest.mark.parametrize("level", (2, 6, 8))
def test_prices(runs, level):
    """Monotone in frequency: code lengths built by any Huffman construction, length-limited or not, never give a more frequent
    symbol a longer code; asserted for every symbol."""
    B, res = runs
    for name, cs in B.items():
        for npass, srcs, views in _passes(res, name, level):
            for i, c in enumerate(cs):
                for k, (s, seg) in enumerate(_segments(c.raw)):
                    f = H.histogram(seg, srcs[i][s:s + len(seg)])
                    H.check_prices(views[i]["price"][k], f, (c.name, level, npass, k))


@pytest.mark.parametrize("level", (2, 6, 8))
def test_parse_is_min_cost(runs, level):
    B, res = runs
    hit = 0
    for name, cs in B.items():
        for npass, _, views in _passes(res, name, level):
            for i, c in enumerate(cs):
                v = views[i]
                for k, (s, seg) in enumerate(_segments(c.raw)):
                    sl = slice(s, s + len(seg))
                    H.check_deflate_parse(seg, v["cand"][sl], v["pos"][sl], v["price"][k], (c.name, level, npass, k))
                    ml = v["pos"][sl] >> 16
                    hit += int((ml[H.walk(v["pos"][sl], len(seg))] >= 64).sum())
    assert hit > 100                         # (the parses do take matches from the long-match ring)


@pytest.mark.parametrize("level", (2, 6, 8))
def test_blocks_hold_the_parse_and_are_the_cheapest(runs, level):
    """Every segment's block: its tokens are the walk of pos (or every byte a literal, the fourth candidate of dh_block); seg_bits is
    its length; it is no larger than the stored form as dh_block counts it and, when dynamic, no larger than the same tokens under the
    fixed code.  (When fixed was chosen, that dynamic was not cheaper cannot be checked without the kernel's trees.)"""
    B, res = runs
    types = set()
    for name, cs in B.items():
        rc, outs, st, views = res[(name, level, ALL)]
        for i, c in enumerate(cs):
            assert zlib.decompress(outs[i], -15) == c.raw, c.name
            blocks = H.inflate_tokens(outs[i])
            v = views[i]
            for k, (s, seg) in enumerate(_segments(c.raw)):
                where = (c.name, level, k)
                typ, bits, L = int(v["seg_type"][k]), int(v["seg_bits"][k]), len(seg)
                types.add(typ)
                lits = [(0, x) for x in seg]
                stored = 8 * L + 42 * ((L + 65534) // 65535)
                if typ == 0:                                # stored: one block per 65535 bytes
                    got = []
                    while len(got) < L:
                        b = blocks.pop(0)
                        assert b["type"] == 0, where
                        got += b["tokens"]
                    assert got == lits, where
                    continue
                b = blocks.pop(0)
                assert b["type"] == typ and b["bits"] == bits, (where, b["type"], typ, b["bits"], bits)
                toks = H.parse_tokens(seg, v["pos"][s:s + L])
                assert b["tokens"] == toks or (typ == 2 and b["tokens"] == lits), where
                assert bits <= stored, (where, bits, stored)
                if typ == 2:
                    assert bits <= H.fixed_cost(b["tokens"]), (where, "dynamic %d bits, fixed %d" % (bits, H.fixed_cost(b["tokens"])))
                assert (k + 1 == (len(c.raw) + SEG - 1) // SEG) == bool(b["final"]), where
            if len(c.raw):
                assert not blocks, c.name
    assert types == {0, 1, 2}                # (the batch holds segments of every block type)
