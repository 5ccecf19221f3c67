"""GPU parity: the parser wave's segment links (k_lz4_decode_v8.hip, run_parser8 step 2) on hand-built blocks whose links all fail
(tests/lz4_link_cases.py) -- bytes, out_len, in_used and status against the oracle, through the device-resident launch the benchmark
uses (every input misalignment) and through the host-memory batch call."""
import numpy as np
import pytest

import lz4_link_cases as K
from rust_compress_amd import _native as N
from rust_compress_amd import batch as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expect(oracle):
    """oracle results, computed once per block and shared"""
    memo = {}

    def ex(blob, cap):
        key = (blob, cap)
        if key not in memo:
            memo[key] = oracle.lz4_decode_block(blob, cap=cap, raise_on_error=False)
        return memo[key]
    return ex


def _valid(expect, blobs):
    """every hand-built block is a valid stream for the oracle; -> its decoded bytes"""
    raws = []
    for i, b in enumerate(blobs):
        out, st = expect(b, 65536)
        assert st == 0, (i, st, len(b))
        assert len(out) <= 65536
        raws.append(out)
    return raws


def _launch(ctx, blobs, caps, mis=0):
    """one device-resident launch, every block's input `mis` bytes off a 16-byte boundary -> (outputs, out_len, in_used, status)"""
    import torch
    import rust_compress_amd as R
    base, off, lens = B.pack(blobs)
    base = np.concatenate([np.zeros(mis, np.uint8), base, np.zeros(64, np.uint8)])
    off = off + np.uint64(mis)
    total, ooff, ocap = B.layout(caps)
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    db = R.DeviceBatch.from_host(base, off, lens, total, ooff, ocap, dev)
    ctx.launch_dev(N.LZ4_DECODE, db)
    torch.cuda.synchronize()
    n = len(blobs)
    out = db.out_base.cpu().numpy()
    out_len, in_used, st = db.out_len[:n].cpu().numpy(), db.in_used[:n].cpu().numpy(), db.status[:n].cpu().numpy()
    return [bytes(out[int(o): int(o) + int(l)]) for o, l in zip(ooff, out_len)], out_len, in_used, st


def _check_ok(ctx, blobs, raws, mis):
    outs, out_len, in_used, st = _launch(ctx, blobs, [len(r) for r in raws], mis)
    assert not st.any(), (mis, np.nonzero(st)[0])
    assert outs == raws, mis
    assert list(out_len) == [len(r) for r in raws]
    assert list(in_used) == [len(b) for b in blobs]


def _check_status(ctx, expect, blobs, caps, mis=0):
    outs, out_len, in_used, st = _launch(ctx, blobs, caps, mis)
    for i, (b, c) in enumerate(zip(blobs, caps)):
        eo, es = expect(b, c)
        assert es == st[i], (i, es, st[i])
        if es == 0:
            assert eo == outs[i] and out_len[i] == len(eo) and in_used[i] == len(b), i


def test_phase_locked_every_link_fails(ctx, expect):
    """periods 3, 4, 5 and 7, every true phase, input misalignments 0-15"""
    blobs = K.phase_blocks()
    raws = _valid(expect, blobs)
    for mis in range(16):
        _check_ok(ctx, blobs, raws, mis)
    res = ctx.lz4_decode_blocks(blobs, [len(r) for r in raws]).check()           # the host-memory call (its kernel keeps a head start of its own)
    assert res.outputs == raws and list(res.in_used) == [len(b) for b in blobs] and list(res.out_len) == [len(r) for r in raws]


def test_general_tokens_in_repaired_segments(ctx, expect):
    """literal runs of 15 / 16 / 270 / 600 bytes and match extensions of one byte and of several 0xff, started in, spanning and jumping over failed
    segments and a chunk edge"""
    blobs = K.general_blocks()
    raws = _valid(expect, blobs)
    for mis in (0, 1, 6, 15):
        _check_ok(ctx, blobs, raws, mis)
    res = ctx.lz4_decode_blocks(blobs, [len(r) for r in raws]).check()
    assert res.outputs == raws and list(res.in_used) == [len(b) for b in blobs]


def test_edges(ctx, expect):
    """compressed lengths 1, 19-21, 63-65, 4095-4097, 4096 + 63..65, 8191-8193; ragged last segments of every length with the links failing up to
    segment nseg - 1 and from segment k0 + 1 on; chunks that are one giant token; too little room"""
    blobs = K.edge_blocks() + K.giant_blocks()
    lens = {len(b) for b in blobs}
    for n in (1, 19, 20, 21, 63, 64, 65) + K.EDGE_LENGTHS:
        assert n in lens
    raws = _valid(expect, blobs)
    for mis in (0, 3, 5, 10, 15):
        _check_ok(ctx, blobs, raws, mis)
    rng = np.random.default_rng(4)
    caps = [int(rng.integers(0, len(r) + 1)) for r in raws]
    _check_status(ctx, expect, blobs, caps)


@pytest.mark.parametrize("kind", ["truncated", "mutated"])
def test_malformed_status_for_status(ctx, expect, kind):
    base = K.phase_blocks()[:2] + K.general_blocks()[::9] + K.edge_blocks()[7::5] + K.giant_blocks()[3:5]
    _valid(expect, base)
    cut, mut = K.malformed(base, 200, 17)
    blobs = cut if kind == "truncated" else mut
    assert len(blobs) == 200
    for mis in (0, 3):
        _check_status(ctx, expect, blobs, [65536] * len(blobs), mis)
