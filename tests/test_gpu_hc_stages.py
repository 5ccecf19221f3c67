"""GPU: the stage arrays of the two high-compression encoders (k_deflate_hc.hip, k_lz4_hc.hip) on the device -- chains, candidates,
prices, arrivals, parses, match lists, block types and sizes -- equal the wave simulator's for the same batch, entry for entry where an
entry is defined.  tests/test_wavesim_deflate_stages.py and test_wavesim_lz4hc_stages.py hold the simulator's arrays to plain
references; this carries those checks onto the hardware and sees what the final bytes hide.  The chain and search references run on
the device's arrays directly at one level.  And every kernel's loop over segments runs a second time: batches of more segments than
the largest grid."""
import zlib

import numpy as np
import pytest

import hc_stages as H
from rust_compress_amd import synth
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

SEG = H.SEG
LEAD = 3
ALL = 0xFFFFFFFF
DEFLATE_LEVELS = (9, 6, 2)
LZ4_LEVELS = (12, 9, 1)


def _device_run(ctx, codec, level, raws, caps, sb):
    """a device-resident launch in a scratch of the test's own, prefilled with 0x5A -> (status, outputs, the scratch on the host, its
    device address)"""
    import torch
    from rust_compress_amd.api import DeviceBatch
    dev = torch.device("cuda")
    n = len(raws)
    buf, offs = H.pack(raws, LEAD)
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    inb = torch.tensor(np.frombuffer(buf, np.uint8).copy(), device=dev)
    out_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    outb = torch.full((int(sum(caps)) + 16,), 0xEE, dtype=torch.uint8, device=dev)
    db = DeviceBatch(inb, T(offs), T([len(r) for r in raws]), outb, T(out_off), T(caps))
    scratch = torch.full((sb,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()                                      # (the context launches on a stream of its own)
    assert N.lib().rcx_ctx_set_param(ctx._h, codec, level) == 0
    try:
        ctx.launch_dev(codec, db, scratch)
        torch.cuda.synchronize()
    finally:
        assert N.lib().rcx_ctx_set_param(ctx._h, codec, 0) == 0
    st, ol, ob = db.status.cpu().numpy(), db.out_len.cpu().numpy(), outb.cpu().numpy()
    outs = [bytes(ob[int(out_off[i]):int(out_off[i]) + int(ol[i])]) for i in range(n)]
    return st, outs, scratch.cpu().numpy(), scratch.data_ptr()


def _eq(a, b, what):
    bad = np.flatnonzero(np.asarray(a) != np.asarray(b))
    assert not len(bad), (what, "entry %d: the device has %#x, the simulator %#x" % (bad[0], np.asarray(a)[bad[0]], np.asarray(b)[bad[0]]))


@pytest.fixture(scope="module")
def deflate_sim():
    import sim_deflate_hc_run as S
    import test_wavesim_deflate_stages as W
    B = W.batches()
    jobs = {(name, lv): ("stages", H.deflate_reduce, [c.raw for c in B[name]], lv, ALL, LEAD)
            for lv in DEFLATE_LEVELS for name in ("synth", "sizes", "edges")}
    return B, dict(zip(jobs, S.encode_many(list(jobs.values()))))


@pytest.mark.parametrize("level", DEFLATE_LEVELS)
def test_deflate_stage_arrays_equal_the_simulator(ctx, deflate_sim, level):
    import sim_deflate_hc_run as S
    B, sim = deflate_sim
    names = ("edges", "sizes", "synth")
    cases = [c for name in names for c in B[name]]
    raws = [c.raw for c in cases]
    want_outs = [o for name in names for o in sim[(name, level)][1]]
    want = [v for name in names for v in sim[(name, level)][3]]
    caps = [int(N.lib().rcx_deflate_compression_bound(len(r))) for r in raws]
    sb = int(N.lib().rcx_deflate_level_scratch_bytes(len(raws), max(map(len, raws))))
    st, outs, scratch, addr = _device_run(ctx, N.DEFLATE_ENCODE, level, raws, caps, sb)
    assert not st.any()
    got = H.deflate_views(raws, scratch, S.layout(addr, sb, len(raws)))
    for c, r, g, w, o, wo in zip(cases, raws, got, want, outs, want_outs):
        assert zlib.decompress(o, -15) == r and o == wo, c.name
        _eq(g["link"], w["link"], (c.name, "link"))
        _eq(g["cand"], w["cand"], (c.name, "cand"))
        _eq(g["price"].ravel(), w["price"].ravel(), (c.name, "price"))
        _eq(g["seg_type"], w["seg_type"], (c.name, "seg_type"))
        _eq(g["seg_bits"], w["seg_bits"], (c.name, "seg_bits"))
        for k, s in enumerate(range(0, len(r), SEG)):
            L = min(SEG, len(r) - s)
            _eq(g["elen"][k][:L + 1], w["elen"][k][:L + 1], (c.name, "elen", k))
            starts = H.walk(w["pos"][s:s + L], L)                  # pos is defined at the token starts of the parse
            _eq(g["pos"][s:s + L][starts], w["pos"][s:s + L][starts], (c.name, "pos", k))
        if level == 6:                                              # the references, directly on the device's arrays
            lk = H.ref_links(r, H.DE_WIN)
            _eq(g["link"], lk, (c.name, "link against the reference"))
            _eq(g["cand"], H.ref_search(r, lk, H.DE_WIN, H.DH_DEPTH[6], 0), (c.name, "cand against the reference"))


@pytest.fixture(scope="module")
def lz4_sim():
    import sim_lz4hc_run as S
    import test_wavesim_lz4hc_stages as W
    B = W.batches()
    jobs = {(name, lv): ("stages", H.lz4_reduce, [c.raw for c in B[name]], lv, ALL, LEAD)
            for lv in LZ4_LEVELS for name in ("synth", "sizes", "edges")}
    return B, dict(zip(jobs, S.encode_many(list(jobs.values()))))


@pytest.mark.parametrize("level", LZ4_LEVELS)
def test_lz4_stage_arrays_equal_the_simulator(ctx, oracle, lz4_sim, level):
    import sim_lz4hc_run as S
    B, sim = lz4_sim
    names = ("edges", "sizes", "synth")
    cases = [c for name in names for c in B[name]]
    raws = [c.raw for c in cases]
    want_outs = [o for name in names for o in sim[(name, level)][1]]
    want = [v for name in names for v in sim[(name, level)][3]]
    caps = [int(N.lib().rcx_lz4_compression_bound(len(r))) for r in raws]
    sb = int(N.lib().rcx_lz4_hc_scratch_bytes(len(raws), max(map(len, raws))))
    st, outs, scratch, addr = _device_run(ctx, N.LZ4_ENCODE, level, raws, caps, sb)
    assert not st.any()
    got = H.lz4_views(raws, scratch, S.layout(addr, sb, len(raws)))
    for c, r, g, w, o, wo in zip(cases, raws, got, want, outs, want_outs):
        assert oracle.lz4_decode_block(o, cap=max(len(r), 1)) == r and o == wo, c.name
        _eq(g["link"], w["link"], (c.name, "link"))
        for key in ("seg_nm", "seg_fm", "seg_le"):
            _eq(g[key], w[key], (c.name, key))
        lk = H.ref_links(r, H.HC_WIN) if level == 9 else None
        cd = H.ref_search(r, lk, H.HC_WIN, H.HC_DEPTH[9], 1) if level == 9 else None
        for k, s in enumerate(range(0, len(r), SEG)):
            L = min(SEG, len(r) - s)
            _eq(g["elen"][k][:L + 1], w["elen"][k][:L + 1], (c.name, "elen", k))
            _eq(g["toks"][k].ravel(), w["toks"][k].ravel(), (c.name, "match list", k))
            if level == 9:                                          # the references, directly on the device's arrays: the match list
                keep = min(L, 2 * (H.HC_TOKCAP - len(g["toks"][k])))   # lies over the end of the segment's candidates
                _eq(g["cand"][s:s + keep], cd[s:s + keep], (c.name, "cand against the reference", k))
        if level == 9:
            _eq(g["link"], lk, (c.name, "link against the reference"))


def _short_streams(n):
    """n streams of 100..700 bytes cut from one buffer per kind: as many segments as streams, a few MiB in all"""
    kinds = [synth.gen(k, 1 << 20, 50 + i).tobytes() for i, k in enumerate(("text", "words", "dna4", "runs", "rand"))] + [b"\0" * (1 << 20)]
    rng = np.random.default_rng(77)
    lens, offs = rng.integers(100, 701, n), rng.integers(0, (1 << 20) - 701, n)
    return [kinds[i % len(kinds)][int(o):int(o) + int(l)] for i, (o, l) in enumerate(zip(offs, lens))]


N_STRIDE = 9000                              # more segments than the largest grid (8192): workgroups take a second segment


@pytest.mark.parametrize("level", (2, 7))
def test_deflate_more_segments_than_the_grid(ctx, level):
    raws = _short_streams(N_STRIDE)
    res = ctx.deflate_encode(raws, level=level)
    assert not np.asarray(res.status).any()
    for r, e in zip(raws, res.outputs):
        assert zlib.decompress(e, -15) == r
    for lo in range(0, N_STRIDE, 1024):
        assert ctx.deflate_encode(raws[lo:lo + 1024], level=level).outputs == res.outputs[lo:lo + 1024], lo


def test_lz4_hc_more_segments_than_the_grid(ctx, oracle):
    raws = _short_streams(N_STRIDE)
    res = ctx.lz4_encode_hc_blocks(raws, 9)
    assert not np.asarray(res.status).any()
    for r, e in zip(raws, res.outputs):
        assert oracle.lz4_decode_block(e, cap=len(r)) == r
    for lo in range(0, N_STRIDE, 1024):
        assert ctx.lz4_encode_hc_blocks(raws[lo:lo + 1024], 9).outputs == res.outputs[lo:lo + 1024], lo
