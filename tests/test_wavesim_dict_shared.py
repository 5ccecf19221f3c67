"""CPU suite: the encoders behind shared dictionaries (k_lz4_hc_dict.hip, k_deflate_hc_dict.hip and lz_dict.h, UNMODIFIED, with the
host's rcx_plan_dict, on the wave64 simulator) against the history encoders on the replicated layout (sim_lz4hist_run,
sim_deflate_hist_run: every block with its dictionary copied directly in front of it): every block's bytes, out_len, in_used and status
are equal.  tests/dict_shared_cases.py holds the batches.  (On a GPU, tests/test_gpu_dict_shared.py checks the device's bytes against
the simulator's.)"""
import struct
import zlib

import numpy as np
import pytest

import dict_shared_cases as K
import lz4_frame_ref as F

FAMILIES = ("lz4", "deflate")
FL = [(f, lv) for f in FAMILIES for lv in K.LEVELS[f]]
IDS = ["%s-%d" % fl for fl in FL]
ZL = K.LEVELS["deflate"]


def _oracle(family, blocks, hists, level, fronts, caps, fmt=0, dict_id=None):
    """the history encoder on the replicated layout -> (rc, outputs, status, out_len, in_used)"""
    if family == "lz4":
        import sim_lz4hist_run as S
        return S.encode(blocks, hists, level, front=fronts, caps=caps)[:5]
    import sim_deflate_hist_run as S
    return S.encode(blocks, hists, level, front=fronts, caps=caps, fmt=fmt, dict_id=dict_id)[:5]


def _shared(*a, **kw):
    import sim_dict_shared_run as S
    return S.run(*a, **kw)


def _job(j):
    return (_oracle if j[0] == "oracle" else _shared)(*j[1], **j[2])


def _run_jobs(jobs):
    """{key: ("oracle" | "shared", args, kwargs)} in forked worker processes -> {key: result}"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    import sim_deflate_hist_run
    import sim_dict_shared_run
    import sim_lz4hist_run
    sim_lz4hist_run.build(); sim_deflate_hist_run.build()
    for f in FAMILIES:
        sim_dict_shared_run.build(f)
    keys = list(jobs)
    with ProcessPoolExecutor(max(1, min(len(keys), sim_dict_shared_run.WORKERS)), mp_context=mp.get_context("fork")) as ex:
        return dict(zip(keys, ex.map(_job, [jobs[k] for k in keys])))


def _ids(B):
    return [zlib.adler32(B.dictionary(i)) if B.of[i] is not None else 0 for i in range(len(B.blocks))]


@pytest.fixture(scope="module")
def runs():
    """the case batch of each family at each level, behind shared dictionaries and through the history encoder; DEFLATE also in the
    zlib form"""
    jobs = {}
    for f, lv in FL:
        B = K.cases(f)
        inb, in_off, lens, d_off, d_len = B.shared()
        blocks, hists, fronts = B.replicated()
        jobs[("shared", f, lv)] = ("shared", (f, inb, in_off, lens, d_off, d_len, lv), {"caps": B.out_caps()})
        jobs[("oracle", f, lv)] = ("oracle", (f, blocks, hists, lv, fronts, B.out_caps()), {})
    B = K.cases("deflate")
    Z = B.reordered(K.zlib_subset(B))
    inb, in_off, lens, d_off, d_len = Z.shared()
    blocks, hists, fronts = Z.replicated()
    for lv in ZL:
        jobs[("shared", "zlib", lv)] = ("shared", ("deflate", inb, in_off, lens, d_off, d_len, lv), {"caps": Z.out_caps(1), "fmt": 1, "dict_id": _ids(Z)})
        jobs[("oracle", "zlib", lv)] = ("oracle", ("deflate", blocks, hists, lv, fronts, Z.out_caps(1)), {"fmt": 1, "dict_id": _ids(Z)})
    res = _run_jobs(jobs)
    for k, r in res.items():
        assert (r["rc"] if isinstance(r, dict) else r[0]) == 0, k
    return res


def _same(names, r, o):
    bad = [names[i] for i in range(len(names)) if r["outputs"][i] != o[1][i]]
    assert not bad, bad
    assert list(r["status"]) == list(o[2]) and list(r["out_len"]) == list(o[3]) and list(r["in_used"]) == list(o[4])


@pytest.mark.parametrize("family,level", FL, ids=IDS)
def test_every_block_is_the_history_encoders(runs, family, level):
    import sim_dict_shared_run as S
    B = K.cases(family)
    r = runs[("shared", family, level)]
    _same(B.names, r, runs[("oracle", family, level)])
    small = B.index("small slot")
    assert r["status"][small] == K.E_OUTPUT_TOO_SMALL and r["out_len"][small] == 0 and not np.delete(r["status"], small).any()
    assert S.untouched_outside(r)                                # (nothing of the small slot, nothing between the slots)
    assert r["outputs"][B.index("end bait x")] == r["outputs"][B.index("end bait y")]
    assert r["outputs"][B.index("front bait x")] == r["outputs"][B.index("front bait y")]
    assert r["outputs"][B.index("before small slot")] != r["outputs"][B.index("after small slot")]
    # equal ranges are one dictionary: the grid's, the three spans', the run's, two slices', four baits' and the small slot's
    assert r["ndict"] == len(B.dicts) and r["ndict"] < sum(d is not None for d in B.of)


@pytest.mark.parametrize("family,level", FL, ids=IDS)
def test_reference_decoders_read_every_block_behind_its_dictionary(runs, family, level):
    B = K.cases(family)
    r = runs[("shared", family, level)]
    for i, o in enumerate(r["outputs"]):
        if r["status"][i]:
            continue
        if family == "lz4":
            assert F.block_decode(o, prefix=B.history(i)) == B.blocks[i], B.names[i]
        else:
            d = zlib.decompressobj(-15, zdict=B.history(i)) if B.of[i] is not None else zlib.decompressobj(-15)
            assert d.decompress(o) == B.blocks[i] and d.eof and not d.unused_data, B.names[i]


@pytest.mark.parametrize("level", ZL)
def test_zlib_form(runs, level):
    B = K.cases("deflate")
    Z = B.reordered(K.zlib_subset(B))
    r, ids = runs[("shared", "zlib", level)], _ids(Z)
    _same(Z.names, r, runs[("oracle", "zlib", level)])
    raw = runs[("shared", "deflate", level)]
    flevel = 1 if level <= 5 else 2 if level == 6 else 3
    plain = {2: b"\x78\x5e", 6: b"\x78\x9c", 9: b"\x78\xda"}[level]
    for i, o in enumerate(r["outputs"]):
        if r["status"][i]:
            assert Z.names[i] == "small slot"
            continue
        body = raw["outputs"][B.index(Z.names[i])]               # the raw stream of the same block at the same level
        adler = struct.pack(">I", zlib.adler32(Z.blocks[i]))
        if Z.of[i] is None:
            # no dictionary: rcx_zlib_encode_level_batch's stream -- its two header bytes, the raw stream, the Adler-32
            assert o == plain + body + adler, Z.names[i]
            assert zlib.decompress(o) == Z.blocks[i]
        else:
            flg = flevel << 6 | 0x20
            flg += 31 - (0x7800 + flg) % 31
            assert o[:2] == bytes([0x78, flg]) and (o[0] << 8 | o[1]) % 31 == 0 and o[1] & 0x20, Z.names[i]
            assert o[2:6] == struct.pack(">I", ids[i]) and o[6:-4] == body and o[-4:] == adler, Z.names[i]
            d = zlib.decompressobj(zdict=Z.dictionary(i))
            assert d.decompress(o) == Z.blocks[i] and d.eof, Z.names[i]


# ------------------------------------------------------------------------------------------------------------------ the candidates
@pytest.fixture(scope="module")
def searched():
    """the spans and the end baits, stopped behind the search"""
    jobs = {}
    for f, lv in FL:
        B = K.cases(f)
        S = B.reordered([B.index(nm) for nm in ("span 1", "span 2", "span 3", "end bait x", "end bait y", "run")])
        inb, in_off, lens, d_off, d_len = S.shared()
        jobs[(f, lv)] = ("shared", (f, inb, in_off, lens, d_off, d_len, lv), {"stop_after": 4, "want_cand": True})
    return _run_jobs(jobs)


@pytest.mark.parametrize("family,level", FL, ids=IDS)
def test_matches_across_the_dictionarys_end(searched, family, level):
    c = searched[(family, level)]["cand"]
    for k in (1, 2, 3):
        # the dictionary ends in P[:k], the block holds P[k:], 100 bytes, P: P is found whole, 140 back, through a chain that passes
        # one of the dictionary's last three positions
        assert int(c[k - 1][140 - k]) == K.pack(family, 40, 140), (k, hex(int(c[k - 1][140 - k])))
    # the match runs past the dictionary's last byte into the block's first bytes, whatever follows the dictionary in memory
    assert int(c[3][0]) == int(c[4][0]) == K.pack(family, 100, 100)
    assert (c[3] == c[4]).all()
    # a run across the boundary at distance 1 (LZ4: the last 5 bytes are literals; DEFLATE: at most 258)
    assert int(c[5][0]) == K.pack(family, 195 if family == "lz4" else 200, 1)


# ------------------------------------------------------------------------------------------------------------------ sharing
ORDER_SEED = 7


@pytest.fixture(scope="module")
def shared_runs():
    jobs = {}
    for f, lv in FL:
        B = K.sharing(f)
        order = list(np.random.default_rng(ORDER_SEED).permutation(len(B.blocks)))
        for tag, L in (("a", B), ("b", B.reordered(order))):
            inb, in_off, lens, d_off, d_len = L.shared()
            jobs[("shared", f, lv, tag)] = ("shared", (f, inb, in_off, lens, d_off, d_len, lv), {"caps": L.out_caps()})
        blocks, hists, fronts = B.replicated()
        jobs[("oracle", f, lv)] = ("oracle", (f, blocks, hists, lv, fronts, B.out_caps()), {})
    return _run_jobs(jobs)


@pytest.mark.parametrize("family,level", FL, ids=IDS)
def test_blocks_that_share_dictionaries(shared_runs, family, level):
    B = K.sharing(family)
    a, b = shared_runs[("shared", family, level, "a")], shared_runs[("shared", family, level, "b")]
    assert a["rc"] == 0 and b["rc"] == 0 and not a["status"].any() and not b["status"].any()
    _same(B.names, a, shared_runs[("oracle", family, level)])
    assert a["ndict"] == b["ndict"] == 3                          # (two ranges that overlap but differ are two dictionaries)
    order = list(np.random.default_rng(ORDER_SEED).permutation(len(B.blocks)))
    assert [b["outputs"][k] for k in np.argsort(order)] == a["outputs"]      # the same bytes wherever the block stands in the batch
    # the overlapping ranges are not interchangeable: one record behind the one is not what it is behind the other (and each is what
    # the history encoder makes of it behind that range: _same above)
    x, y = B.index("twin first"), B.index("twin second")
    assert B.blocks[x] == B.blocks[y] and B.dictionary(x) != B.dictionary(y) and B.dictionary(x)[100:] == B.dictionary(y)[:-100]
    assert a["outputs"][x] != a["outputs"][y]


# ------------------------------------------------------------------------------------------------------------------ more work than workgroups
@pytest.mark.parametrize("family", FAMILIES)
def test_more_work_items_than_the_grids_hold(family):
    """8200 segments for launches of 8192 workgroups at the most, 1030 distinct dictionaries for a build launch of 1024: every block is
    a copy of its 16-byte dictionary, and a sample (both ends, both wrap-arounds) equals the history encoder's bytes"""
    import sim_dict_shared_run as S
    level = K.LEVELS[family][1]
    inb, in_off, lens, d_off, d_len = K.many(family)
    r = S.run(family, inb, in_off, lens, d_off, d_len, level)
    assert r["rc"] == 0 and not r["status"].any() and r["ndict"] == 1030
    sample = list(range(0, 12)) + list(range(1020, 1040)) + list(range(8186, 8200))
    blocks = [bytes(inb[in_off[i]:in_off[i] + 16]) for i in sample]
    o = _oracle(family, blocks, blocks, level, [b"\xC3"] * len(sample), [K.bound(family, 16)] * len(sample))
    assert [r["outputs"][i] for i in sample] == o[1]
    if family == "lz4":
        # one match of 11 bytes at distance 16 (the last 5 bytes are literals): 1 + 2 + 1 + 5 bytes
        assert set(int(x) for x in r["out_len"]) == {9}
        assert all(F.block_decode(r["outputs"][i], prefix=bytes(inb[d_off[i]:d_off[i] + 16])) == bytes(inb[in_off[i]:in_off[i] + 16])
                   for i in range(0, 8200, 41))
    else:
        assert len(set(int(x) for x in r["out_len"])) <= 3 and int(r["out_len"].max()) < 12
        for i in range(0, 8200, 41):
            d = zlib.decompressobj(-15, zdict=bytes(inb[d_off[i]:d_off[i] + 16]))
            assert d.decompress(r["outputs"][i]) == bytes(inb[in_off[i]:in_off[i] + 16])


def test_the_plan_refuses_what_the_abi_refuses():
    import sim_dict_shared_run as S
    inb = np.zeros(200000, np.uint8)
    for family in FAMILIES:
        ok = S.run(family, inb, [100000], [100], [10], [K.MAX_DICT[family]], K.LEVELS[family][0])
        assert ok["rc"] == 0 and ok["ndict"] == 1 and ok["span"] == 10 + K.MAX_DICT[family]
        assert S.run(family, inb, [100000], [100], [10], [K.MAX_DICT[family] + 1], K.LEVELS[family][0])["rc"] == -1
