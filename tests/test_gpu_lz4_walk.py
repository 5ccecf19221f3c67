"""GPU parity: the parser's hand-written token walk (k_lz4_decode_v8.hip: walk_steps2 and its reads, RCX_WALK_READ) -- the hand-built
blocks of tests/lz4_walk_cases.py through the shipped library (and, with it, the batch header in whichever form RCX_HDR_PACK builds).

The wave simulator builds without the inline assembly, so this file is the check of the step itself: the two aligned qword reads, the
choice of the step's three dwords by bit 2 of the token's address, the byte read for a match-length extension beyond the eight bytes in
hand, the reads of a chunk's last token into the staged slack, and the hand-over to the portable loop 19 bytes in front of the block's
end.  A token's LDS address is its block position + the input's misalignment + the head start (mod 8), so every block is decoded at all
sixteen input misalignments: each token passes through all eight read phases, and the segment grid moves across the tokens.
Bytes, out_len, in_used and status are the oracle's; so are the statuses of the same blocks cut short inside a token."""
import numpy as np
import pytest
import torch

from rust_compress_amd import _native as N
import lz4_walk_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return [K.build(*c) for c in K.CASES]


def _decode(ctx, jobs):
    """jobs: (blob, input misalignment, cap) -> status, out_len, in_used, outputs: one launch, every block's input at its misalignment"""
    from rust_compress_amd.api import DeviceBatch
    dev = torch.device("cuda")
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    in_off, ooff, pos, total = [], [], 0, 0
    for blob, mis, cap in jobs:
        pos = ((pos + 15) & ~15) + 16 + mis                 # (a gap: no block's staged rows are its neighbour's bytes by accident of layout)
        in_off.append(pos)
        pos += len(blob)
        ooff.append(total)
        total += (cap + 64 + 255) & ~255
    host_in = np.full(pos + 64, 0xFF, np.uint8)             # between the blocks: bytes that read as "the extension goes on"
    for (blob, _, _), o in zip(jobs, in_off):
        host_in[o: o + len(blob)] = np.frombuffer(blob, np.uint8)
    inb = torch.tensor(host_in, device=dev)
    assert inb.data_ptr() % 16 == 0
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    db = DeviceBatch(inb, T(in_off), T([len(j[0]) for j in jobs]), out, T(ooff), T([j[2] for j in jobs]))
    torch.cuda.synchronize()                                # (the context launches on a stream of its own)
    ctx.launch_dev(N.LZ4_DECODE, db)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    status, out_len, in_used = db.status.cpu().numpy(), db.out_len.cpu().numpy(), db.in_used.cpu().numpy()
    outs = [host[o: o + int(l)].tobytes() for o, l in zip(ooff, out_len)]
    return status, out_len, in_used, outs


def test_every_block_at_every_input_misalignment(ctx, oracle, cases):
    jobs = [(c.blob, mis, len(c.raw)) for mis in range(16) for c in cases]
    status, out_len, in_used, outs = _decode(ctx, jobs)
    for i, (blob, mis, cap) in enumerate(jobs):
        eo, es = oracle.lz4_decode_block(blob, cap=cap, raise_on_error=False)
        eu = len(blob)                                      # (a well-formed block is consumed to its last byte)
        c = cases[i % len(cases)]
        assert es == 0 and eo == c.raw and eu == len(blob)
        what = (K.CASES[i % len(cases)], mis)
        assert int(status[i]) == es, what
        assert int(out_len[i]) == len(eo) and int(in_used[i]) == eu, what
        assert outs[i] == eo, what


def test_blocks_cut_short_inside_a_token(ctx, oracle, cases):
    """each block ended inside a token with a length extension (behind the token byte, in front of the match-length extension, in front
    of the token's last byte): the cuts of a token are spread over the blocks -- they differ in their bytes and tails, not in where their
    tokens stand -- every block keeps the cuts of its own tail, and the misalignment steps with the cut"""
    jobs = []
    for ci, c in enumerate(cases):
        cuts = K.cuts(c)
        mine = set(cuts[ci::len(cases)]) | set(n for n in cuts if n > len(c.blob) - 24)
        for k, n in enumerate(sorted(mine)):
            jobs.append((c.blob[:n], (k + ci) % 16, len(c.raw)))
    assert 200 <= len(jobs) <= 600, len(jobs)
    status, out_len, in_used, outs = _decode(ctx, jobs)
    nerr = 0
    for i, (blob, mis, cap) in enumerate(jobs):
        eo, es = oracle.lz4_decode_block(blob, cap=cap, raise_on_error=False)
        eu = len(blob)                                      # (a well-formed block is consumed to its last byte)
        assert int(status[i]) == es, (i, len(blob), mis, es, int(status[i]))
        if es == 0:
            assert int(out_len[i]) == len(eo) and int(in_used[i]) == eu and outs[i] == eo, (i, len(blob), mis)
        else:
            nerr += 1
    assert nerr > len(jobs) // 2                            # (a cut behind a token's literals can be a well-formed last token)
