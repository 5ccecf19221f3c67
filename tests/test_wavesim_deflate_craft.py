"""CPU suite: the table of hand-assembled DEFLATE streams (deflate_craft_cases.py) through the UNMODIFIED inflate kernels on the wave64
simulator: k_inflate3 + k_inflate2 (variants 0, 11), k_inflate2 alone at every streams-per-wave geometry (9, 2 .. 5), the first pass
alone (12, 10), raw / zlib / gzip framing, and k_inflate_hist / k_inflate_dict without and behind a history.  The reference is the
oracle, which test_deflate_craft.py holds against the token model, libz and the hand-stated statuses.  The simulator runs portable
versions of k_inflate3's ISA walks: only tests/test_gpu_deflate_craft.py runs those."""
import struct
import zlib

import pytest

import deflate_craft_cases as T
from rust_compress_amd import _native as N

PREFIX_STEP = 3                                 # the simulator's share of the prefixes: every third cut


def _rows(oracle):
    return T.table(oracle, T.SWEEP_SIM, PREFIX_STEP)


def _run(codec, variant, streams, caps):
    import simrun
    outs, out_len, used, st, aux = simrun.run(codec, variant, streams, caps, scratch_bytes=64 * len(streams) + 1024)     # (gzip: 48 bytes a member + the inflate path's own)
    return st, out_len, used, aux, outs


@pytest.mark.parametrize("variant", (0, 9, 2, 3, 4, 5, 11))
def test_raw(oracle, variant):
    rows = _rows(oracle)
    bad = T.mismatches(rows, *_run(N.INFLATE, variant, [r["stream"] for r in rows], [r["cap"] for r in rows]))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("variant", (12, 10))
def test_first_pass_alone(oracle, variant):
    """k_inflate3 without the second pass: a status is 0 or the hand-back; 0 only with the reference's results; every stream the
    reference refuses is handed back, every one it takes is accepted, the named exceptions apart"""
    rows = _rows(oracle)
    st, out_len, used, aux, outs = _run(N.INFLATE, variant, [r["stream"] for r in rows], [r["cap"] for r in rows])
    T.check_first_pass(rows, st, out_len, used, aux, outs)


@pytest.mark.parametrize("variant", (0, 9))
def test_zlib(oracle, variant):
    rows = _rows(oracle)
    zs = [b"\x78\x9c" + r["stream"] + struct.pack(">I", zlib.adler32(r["ref"][1]) ^ (i % 5 == 4)) for i, r in enumerate(rows)]   # (every fifth sum is wrong)
    ref = []
    for z, r in zip(zs, rows):
        out, used, flags, st = oracle.zlib_decode(z, cap=r["cap"], raise_on_error=False)
        ref.append((st, out, used, flags))
    assert {e[0] for e in ref} >= {0, T.E_ZLIB_CHECKSUM, T.E_EOF, T.E_NOT_ENOUGH_BITS}
    bad = T.mismatches(rows, *_run(N.ZLIB_DECODE, variant, zs, [r["cap"] for r in rows]), ref=ref)
    assert not bad, (len(bad), bad[:6])
    fr = [c for c in T.framed() if c["kind"] == "zlib"]
    st, out_len, used, _, outs = _run(N.ZLIB_DECODE, variant, [c["stream"] for c in fr], [len(c["want"]) for c in fr])
    assert [int(s) for s in st] == [c["status"] for c in fr] and outs == [c["want"] for c in fr]


def test_gzip(oracle):
    fr = [c for c in T.framed() if c["kind"] == "gzip"]
    for c in T.valid()[::7]:
        w = c["want"]
        fr.append({"name": c["name"], "stream": T.GZIP_HEAD + c["stream"] + struct.pack("<II", zlib.crc32(w), len(w)), "want": w, "status": 0})
    st, out_len, used, _, outs = _run(N.GZIP_DECODE, 0, [c["stream"] for c in fr], [len(c["want"]) for c in fr])
    bad = [c["name"] for i, c in enumerate(fr) if int(st[i]) != c["status"] or outs[i] != c["want"] or int(used[i]) != len(c["stream"])]
    assert not bad, bad


# ---- the history and dictionary kernels: their stream bodies are k_inflate2's f2_stored / f2_fixed / f2_dynamic, reached from kernels
# of their own
def _hist(rows, hists, caps=None):
    import sim_deflate_hist_run as S
    outs, out_len, used, st, flags = S.inflate([r["stream"] for r in rows], hists, caps or [r["cap"] for r in rows])
    return st, out_len, used, flags, outs


def _dict(rows, hist, caps=None):
    import dict_decode_cases as DC
    import sim_dict_decode_run as DR
    B = DC.DBatch("deflate")
    d = B.dict(hist) if hist else None
    for r, c in zip(rows, caps or [r["cap"] for r in rows]):
        B.rec(r["name"], r["stream"], d, c)
    got = DR.run(*DC.shared_job(B)[1])
    assert got["rc"] == 0, got["err"]
    out_off, cp, _ = B.slots()
    assert DR.only_slots_changed(got["out"], out_off, cp)
    return got["status"], got["out_len"], got["in_used"], got["flags"], got["outputs"]


@pytest.mark.parametrize("kernel", ("hist", "dict"))
def test_history_kernels_without_history(oracle, kernel):
    rows = _rows(oracle)
    got = _hist(rows, [None] * len(rows)) if kernel == "hist" else _dict(rows, b"")
    bad = T.mismatches(rows, *got)
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("nhist", (300, 32768))
@pytest.mark.parametrize("kernel", ("hist", "dict"))
def test_history_kernels_behind_a_history(oracle, kernel, nhist):
    hist = T.rand(nhist, 90 + nhist % 7)
    rows = _rows(oracle)
    extra = [{"name": n, "stream": s, "cap": c, "want": w} for n, s, c, w in T.into_history(hist)]
    rows = rows + extra
    ref = T.behind_history(oracle, rows, hist)
    for r, e in zip(extra, ref[-len(extra):]):                 # the token model over the history
        assert e == (0, r["want"], len(r["stream"]), 0), r["name"]
    got = _hist(rows, [hist] * len(rows)) if kernel == "hist" else _dict(rows, hist)
    bad = T.mismatches(rows, *got, ref=ref)
    assert not bad, (len(bad), bad[:6])
