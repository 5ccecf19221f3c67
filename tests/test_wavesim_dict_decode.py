"""CPU suite: the UNMODIFIED decoders behind shared dictionaries (k_lz4_dict.hip, k_inflate_dict.hip behind k_inflate2.hip, with the
host's rcx_plan_dict, on the wave64 simulator) against the history decoders on the replicated layout (k_lz4_linked through
sim_lz4frame_run, k_inflate_hist through sim_deflate_hist_run): bytes, out_len, in_used, status and flags, malformed streams included.
The batches are dict_decode_cases'; test_gpu_dict_decode.py runs the same ones on the device."""
import numpy as np
import pytest

import dict_decode_cases as DC
import sim_dict_decode_run as DR

_results = {}


def _both(batches):
    """[(shared result, history result)] of the batches, every decode a job of one pool; memoised by the batches' identity"""
    todo = [B for B in batches if id(B) not in _results]
    if todo:
        res = DR.run_many([DC.shared_job(B) for B in todo] + [DC.hist_job(B) for B in todo])
        for k, B in enumerate(todo):
            _results[id(B)] = (B, res[k], DC.hist_results(B, res[len(todo) + k]))
    return [_results[id(B)][1:] for B in batches]


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_case_batches_equal_the_history_kernels(family):
    batches = DC.case_batches(family)
    for B, (got, ref) in zip(batches, _both(batches)):
        assert got["rc"] == 0, got["err"]
        DC.check(B, got, ref)


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_the_cases_cover_what_they_claim(family):
    g0, g1, hand = DC.case_batches(family)[:3]
    # every dictionary length with every block length; a dictionary that ends at the buffer's last byte; both sides of the blocks
    for g in (g0, g1):
        buf, in_off, _, d_off, d_len = g.layout()
        assert max(o + l for o, l in zip(d_off, d_len)) == buf.size
        assert any(o and o < in_off[0] for o in d_off) and any(o > in_off[-1] for o in d_off)
        assert {int(l) for l in d_len} == set(DC.DICTS[family])
    got = [r[0] for r in _both([g0, g1])]
    assert {int(l) for r in got for l in r["out_len"]} >= set(DC.LENS)
    # the dictionary's end and the slots at every residue mod 16; a slot at offset 0
    _, _, _, d_off, d_len = hand.layout()
    ends = {(d_off[i] + d_len[i]) % 16 for i, nm in enumerate(hand.names) if nm.startswith("end residue")}
    assert ends == set(range(16))
    out_off = hand.slots()[0]
    assert {o % 16 for o in out_off} == set(range(16)) and out_off[0] == 0
    # the statuses the reach cases and the short slot are there for
    (h, _), = _both([hand])
    st = {nm: int(s) for nm, s in zip(hand.names, h["status"])}
    bad = DC.E_MALFORMED if family == "lz4" else DC.E_INVALID_HUFFMAN_CODE
    assert st["short slot"] == DC.E_OUTPUT_TOO_SMALL and st["before short slot"] == 0 and st["after short slot"] == 0
    if family == "lz4":
        assert st["reach end+dict"] == 0 and st["reach end+dict+1"] == bad and st["reach bait"] == bad and st["off65535 D65534 p0"] == bad
        assert st["off65535 D65535 p0"] == 0 and st["off65535 D65536 p0"] == 0 and st["off65535 D65534 p1"] == 0
    else:
        assert st["reach end+hist"] == 0 and st["reach end+hist+1"] == bad and st["reach bait"] == bad
        assert st["d32768 h32768 p0"] == 0 and st["d32768 h32767 p0"] == bad and st["d32768 h32767 p1"] == 0
    # the bait pair: equal outputs, equal to the reference
    x, y = hand.index("end bait x"), hand.index("end bait y")
    assert h["outputs"][x] == h["outputs"][y] == hand.want[x][1] and int(h["status"][x]) == 0
    # distances 1, 2 and 3 at output position 0: nothing but the seeded ring to read
    assert all(st["first match d%d" % d] == 0 and hand.want[hand.index("first match d%d" % d)][1] for d in (1, 2, 3))
    if family == "deflate":
        import deflate_hist_cases as DH
        # a 16-byte gather of a far source that straddles position 0, split after every count of dictionary bytes; both kernels take
        # it: _both() sends the batch through k_inflate_dict and, on the replicated layout, through k_inflate_hist
        splits = {-s for r in range(16) for s in DH.far_gathers(DH.first_match_tokens(112 + r)) if -16 < s < 0}
        assert splits == set(range(1, 16)) and all(st["end residue %d" % r] == 0 for r in range(16))
        # ... and whole gathers on both sides of it: from the dictionary alone (the first of every far match here), from the slot alone.
        # (A far source ends 96 bytes or more below the output's end, inside the slot: no case can make its gather pass the slot's
        # capacity, so the byte-wise tail of the slot policy has none.)
        at = DH.far_gathers(DH.first_match_tokens(112))
        assert at[0] == -112 and 0 in at
        # zlib: FDICT with a wrong DICTID and FDICT with no dictionary; a dictionary in use that ends at the buffer's last byte
        zl = DC.zlib_cases()
        (z, _), = _both([zl])
        zst = {nm: int(s) for nm, s in zip(zl.names, z["status"])}
        assert zst["wrong id"] == DH.E_ZLIB_DICT_ID and zst["fdict, no history"] == DH.E_ZLIB_DICT
        buf, _, _, d_off, d_len = zl.layout()
        i = zl.index("short history")
        assert d_off[i] + d_len[i] == buf.size and zst["short history"] == 0 and z["outputs"][i] == zl.want[i][1]
        assert DH.libz_raw(b"", zl.blocks[i][6:-4]) is None               # (without the dictionary libz cannot read it)


def test_zlib_cases_carry_their_statuses():
    B = DC.zlib_cases()
    (got, _), = _both([B])
    import deflate_hist_cases as DH
    cs = DH.zlib_decode_cases()
    assert [int(s) for s in got["status"]] == [c["status"] for c in cs]
    assert all(c["in_used"] is None or int(u) == c["in_used"] for c, u in zip(cs, got["in_used"]))


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_sharing_in_two_orders(family):
    A, Z = DC.sharing(family, 0), DC.sharing(family, 1)
    (a, ra), (z, rz) = _both([A, Z])
    DC.check(A, a, ra)
    DC.check(Z, z, rz)
    assert a["ndict"] == 3 and z["ndict"] == 3
    assert (a["status"] == 0).all()
    # a block's results do not depend on its place in the batch
    assert a["outputs"] == z["outputs"][::-1] and (a["in_used"] == z["in_used"][::-1]).all()


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_more_blocks_than_a_grid(family):
    B = DC.many(family)
    (got, ref), = _both([B])
    DC.check(B, got, ref)
    assert got["ndict"] == 1030 and (got["status"] == 0).all() and (got["out_len"] == 16).all()
    buf, _, _, d_off, d_len = B.layout()
    assert max(o + l for o, l in zip(d_off, d_len)) == buf.size


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_corrupted_streams_status_for_status(family):
    B = DC.corrupted(family)
    (got, ref), = _both([B])
    st = np.asarray(ref[0])
    print("%s: %d of %d fail by the history kernel" % (family, int((st != 0).sum()), st.size))
    assert int((st != 0).sum()) >= 20 and int((st == 0).sum()) >= 150          # (not all of one kind)
    DC.check(B, got, ref)


def test_a_dictionary_over_the_limit_names_the_block():
    for family, lim in (("lz4", 65536), ("deflate", 32768)):
        inb = np.zeros(lim + 8, np.uint8)
        r = DR.run(family, inb, [0, 1], [1, 1], [0, 0], [lim, lim + 1], [0, 8], [4, 4], 32)
        assert r["rc"] == -1 and "block 1" in r["err"] and str(lim) in r["err"], r["err"]
        assert DR.run(family, inb, [0, 1], [1, 1], [0, 0], [lim, lim], [0, 8], [4, 4], 32)["rc"] == 0
