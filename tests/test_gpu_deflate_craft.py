"""GPU suite: the WHOLE table of hand-assembled DEFLATE streams (deflate_craft_cases.py: both families, all 128 shifts of the position
sweep, every prefix) through the library on the device -- the only place where k_inflate3's hand-written ISA walks (rcx_inf_walk,
rcx_inf_hops, the rewalk) run; the simulator of tests/test_wavesim_deflate_craft.py has portable versions of them.  One batch per
variant.  The reference is the oracle, which tests/test_deflate_craft.py holds against the token model, libz and the hand-stated
statuses."""
import struct
import zlib

import pytest

import deflate_craft_cases as T
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows(oracle):
    return T.table(oracle, T.SWEEP_ALL, 1)


def _got(res):
    return res.status, res.out_len, res.in_used, res.aux, res.outputs


def _inflate(ctx, variant, rows):
    ctx.set_variant(N.INFLATE, variant)
    try:
        return _got(ctx.inflate([r["stream"] for r in rows], [r["cap"] for r in rows]))
    finally:
        ctx.set_variant(N.INFLATE, 0)


@pytest.mark.parametrize("variant", sorted(set(N.INFLATE_VARIANTS) - {10} | {2, 3, 4, 5}))
def test_raw(ctx, rows, variant):
    bad = T.mismatches(rows, *_inflate(ctx, variant, rows))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("variant", (12, 10))
def test_first_pass_alone(ctx, rows, variant):
    """k_inflate3 without the second pass, as tests/test_wavesim_deflate_craft.py on the simulator: the same check, so the same
    accepted set -- or the ISA walks and the portable ones disagree"""
    T.check_first_pass(rows, *_inflate(ctx, variant, rows))


def test_zlib(ctx, oracle, rows):
    zs = [b"\x78\x9c" + r["stream"] + struct.pack(">I", zlib.adler32(r["ref"][1]) ^ (i % 5 == 4)) for i, r in enumerate(rows)]   # (every fifth sum is wrong)
    ref = []
    for z, r in zip(zs, rows):
        out, used, flags, st = oracle.zlib_decode(z, cap=r["cap"], raise_on_error=False)
        ref.append((st, out, used, flags))
    bad = T.mismatches(rows, *_got(ctx.zlib_decode(zs, [r["cap"] for r in rows])), ref=ref)
    assert not bad, (len(bad), bad[:6])
    fr = [c for c in T.framed() if c["kind"] == "zlib"]
    res = ctx.zlib_decode([c["stream"] for c in fr], [len(c["want"]) for c in fr])
    assert [int(s) for s in res.status] == [c["status"] for c in fr] and res.outputs == [c["want"] for c in fr]


def test_gzip(ctx, rows):
    """no oracle for gzip: the framed cases' hand-stated statuses; every valid case in a member (bytes, and in_used = header + stream
    + trailer); every invalid one with the status of its raw stream"""
    fr = [c for c in T.framed() if c["kind"] == "gzip"]
    res = ctx.gzip_decode([c["stream"] for c in fr], [len(c["want"]) for c in fr])
    assert [int(s) for s in res.status] == [c["status"] for c in fr] and res.outputs == [c["want"] for c in fr]
    gz, ref = [], []
    for r in rows:
        st, out, used, flags = r["ref"]
        gz.append(T.GZIP_HEAD + r["stream"] + (struct.pack("<II", zlib.crc32(out), len(out)) if st == 0 and used == len(r["stream"]) else b""))
    res = ctx.gzip_decode(gz, [r["cap"] for r in rows])
    bad = []
    for i, r in enumerate(rows):
        st, out, used, flags = r["ref"]
        if st == 0 and used != len(r["stream"]):      # (a cut stream with a tail that decodes: its trailer is the tail's bytes)
            continue
        want = (st, out, used + 10 + (8 if st == 0 else 0)) if st == 0 else (st,)
        got = (int(res.status[i]), res.outputs[i], int(res.in_used[i]))[:len(want)]
        if got != want:
            bad.append((r["name"], got[0], want[0]))
    assert not bad, (len(bad), bad[:6])


# ---- rcx_inflate_hist_batch (k_inflate_hist) and rcx_inflate_shared_batch (k_inflate_dict)
def _hist(ctx, rows, hist):
    return _got(ctx.inflate_hist_blocks([r["stream"] for r in rows], [hist or None] * len(rows), [r["cap"] for r in rows]))


def _dict(ctx, rows, hist):
    return _got(ctx.inflate_dict_blocks([r["stream"] for r in rows], [hist or None] * len(rows), [r["cap"] for r in rows]))


@pytest.mark.parametrize("call", (_hist, _dict))
def test_history_kernels_without_history(ctx, rows, call):
    bad = T.mismatches(rows, *call(ctx, rows, b""))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("nhist", (300, 32768))
@pytest.mark.parametrize("call", (_hist, _dict))
def test_history_kernels_behind_a_history(ctx, oracle, rows, call, nhist):
    hist = T.rand(nhist, 90 + nhist % 7)
    extra = [{"name": n, "stream": s, "cap": c, "want": w} for n, s, c, w in T.into_history(hist)]
    rows = rows + extra
    ref = T.behind_history(oracle, rows, hist)
    for r, e in zip(extra, ref[-len(extra):]):                 # the token model over the history
        assert e == (0, r["want"], len(r["stream"]), 0), r["name"]
    bad = T.mismatches(rows, *call(ctx, rows, hist), ref=ref)
    assert not bad, (len(bad), bad[:6])
