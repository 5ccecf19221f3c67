"""CPU suite: the stages of the LZ4 high-compression encoder (k_lz4_hc.hip, UNMODIFIED, on the wave64 simulator) against plain
references of what its header comment claims -- exact hash chains, the longest match within the depth, a parse made of the search's
candidates that is no larger than the greedy parse over them and no smaller than a lower bound.  tests/hc_stages.py reads the stage
arrays and holds the references, tests/hc_inputs.py the inputs.  (On a GPU, tests/test_gpu_hc_stages.py checks the device's arrays
against these.)

The parse has no single exact reference: a literal run's length bytes make a literal's cost depend on the run it is in.  So it is held
from both sides.  The lower bound charges a literal 1 byte and a match 3 bytes plus its length bytes; it holds for the parse's pieces as
the arrival record lists them, before k_hc_parse joins adjacent pieces of one run into one match -- a join pays one token for a run
longer than HC_MAXM, which no single candidate allows, so the joined list may lie below the bound by exactly what the joins save, and
that is added back."""
import numpy as np
import pytest

import hc_inputs as I
import hc_stages as H

SEG = H.SEG
LEAD = 3                                    # bytes before every block in the input buffer: odd offsets (unaligned 4-byte loads)
SEARCH = 3                                  # stop_after: the launches of sim_lz4hc_run.LAUNCHES (k_hc_parse overwrites cand)
ALL = 0xFFFFFFFF
LEVELS = (12, 10, 9, 4, 1)                  # depths 256, 64, 24, 4, 1 (the slowest first)


def batches():
    return {"edges": I.window_cases(H.HC_WIN, 1) + I.group_cases() + I.length_cases(H.HC_MAXM, H.HC_RING, 1) + I.end_cases()
            + I.small_cases() + I.depth_cases((1, 4, 24, 64, 256), 1),
            "sizes": I.size_cases(), "synth": I.synth_cases() + [I.Case("z", b"z" * 100000)]}


@pytest.fixture(scope="module")
def runs():
    import sim_lz4hc_run as S
    B = batches()
    jobs = {}
    for lv in LEVELS:
        for stop in (ALL, SEARCH):
            for name in ("synth", "sizes", "edges"):
                jobs[(name, lv, stop)] = ("stages", H.lz4_reduce, [c.raw for c in B[name]], lv, stop, LEAD)
    res = dict(zip(jobs, S.encode_many(list(jobs.values()))))
    for k, (rc, outs, st, views) in res.items():
        assert rc == 0 and (k[2] != ALL or not st.any()), k
    return B, res


@pytest.fixture(scope="module")
def refs():
    """the reference chains of every block, and its reference candidates per depth"""
    B = batches()
    links = {(name, i): H.ref_links(c.raw, H.HC_WIN) for name, cs in B.items() for i, c in enumerate(cs)}
    cands = {}

    def cand(name, i, depth):
        if (name, i, depth) not in cands:
            cands[(name, i, depth)] = H.ref_search(B[name][i].raw, links[(name, i)], H.HC_WIN, depth, 1)
        return cands[(name, i, depth)]
    return links, cand


def test_inputs_hit_their_edges(refs):
    links, cand = refs
    B = batches()
    for i, c in enumerate(B["edges"]):
        c.check_edges(links[("edges", i)], cand("edges", i, getattr(c, "depth", 4)), 1)
        if hasattr(c, "depth"):
            # the long match is entry c.entry of the walk: found to that depth, not one short of it; the level's depth lies on the
            # side the case names
            ln = lambda d: int(cand("edges", i, d)[c.p]) >> 16
            assert ln(c.entry) == 24 and (c.entry == 1 or ln(c.entry - 1) == 4), c.name
            assert ln(c.depth) == (24 if c.entry == c.depth else 4), c.name
    assert sorted(set(c.depth for c in B["edges"] if hasattr(c, "depth"))) == sorted(H.HC_DEPTH[lv] for lv in LEVELS)


@pytest.mark.parametrize("level", LEVELS)
def test_chains(runs, refs, level):
    B, res = runs
    links, _ = refs
    for name, cs in B.items():
        views = res[(name, level, ALL)][3]
        for i, c in enumerate(cs):
            bad = np.flatnonzero(views[i]["link"] != links[(name, i)])
            assert not len(bad), (c.name, "link[%d] = %d, the reference %d" % (bad[0], views[i]["link"][bad[0]], links[(name, i)][bad[0]]))


@pytest.mark.parametrize("level", LEVELS)
def test_search(runs, refs, level):
    B, res = runs
    _, cand = refs
    for name, cs in B.items():
        views = res[(name, level, SEARCH)][3]
        for i, c in enumerate(cs):
            want = cand(name, i, H.HC_DEPTH[level])
            bad = np.flatnonzero(views[i]["cand"] != want)
            assert not len(bad), (c.name, "cand[%d] = %#x, the reference %#x" % (bad[0], views[i]["cand"][bad[0]], want[bad[0]]))


@pytest.mark.parametrize("level", LEVELS)
def test_parse(oracle, runs, level):
    """(a) every segment's match list is made of the candidates; the block holds exactly these matches; (b) the block is no larger
    than the greedy parse over the same candidates; (c) with what its joins save added back, no smaller than the lower bound."""
    B, res = runs
    joins = 0
    for name, cs in B.items():
        outs, full = res[(name, level, ALL)][1], res[(name, level, ALL)][3]
        cands = res[(name, level, SEARCH)][3]
        for i, c in enumerate(cs):
            raw, out, n = c.raw, outs[i], len(c.raw)
            assert oracle.lz4_decode_block(out, cap=max(n, 1)) == raw, c.name
            cand = cands[i]["cand"]
            listed, saved, bound = [], 0, 1
            for k, s in enumerate(range(0, n, SEG)):
                L = min(SEG, n - s)
                toks = full[i]["toks"][k]
                _, sv = H.check_lz4_parse(L, cand[s:s + L], full[i]["elen"][k], toks, (c.name, level, k))
                saved += sv
                bound += H.ref_lz4_min_cost(L, cand[s:s + L])
                listed += [(s + int(st), int(ln), int(d)) for st, ln, d in toks]
                if len(toks):
                    assert int(full[i]["seg_fm"][k]) == int(toks[0][0]) and int(full[i]["seg_le"][k]) == int(toks[-1][0] + toks[-1][1])
            emitted = [(st, ln, d) for _, st, ln, d in H.lz4_block_tokens(out)[:-1]]
            literals_only = 1 + H.lext(n) + n
            if emitted or not listed:
                assert emitted == listed, c.name                       # the block holds the parse's matches
            else:
                saved = 0                                              # (larger than the block as literals: k_hc_scan emits those)
                assert len(out) == literals_only, c.name
            joins += sum(ln > H.HC_MAXM for _, ln, _ in emitted)
            greedy = H.ref_lz4_greedy_size(n, cand)
            assert len(out) <= greedy, (c.name, level, "the block has %d bytes, the greedy parse %d" % (len(out), greedy))
            assert len(out) + saved >= bound, (c.name, level, "the block has %d bytes (+ %d joined), the bound is %d" % (len(out), saved, bound))
    assert joins >= 3                        # (runs longer than HC_MAXM are in the batch and come out joined)
