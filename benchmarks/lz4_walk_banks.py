"""LDS bank model of the LZ4 parser's token walk (k_lz4_decode_v8.hip: run_parser8's step 1, walk_steps2).  CPU only.

    python benchmarks/lz4_walk_banks.py                     the table of docs/LAB_NOTEBOOK.md, "Walk reads"
    python benchmarks/lz4_walk_banks.py --reads 2 --seg 64 --pre 128 [--inmis 3] [--kind text] [--blocks 8]

What is modelled.  The parser stages a chunk of 64 segments linearly in LDS (stage8: cbuf + 16 j) and walks all segments at once, a lane
per segment: lane l starts PRE bytes in front of its segment (the lane that holds the block's true cursor starts there), every lane takes
one token a step, in lockstep, until no lane is inside its bound (its segment's end, or the block's last 19 bytes); `exec` stays
narrowed, so a lane past its bound reads no more.  A step reads the token's bytes with

    --reads 3    three ds_read_b32 at a4 = ad & ~3, a4 + 4, a4 + 8       (RCX_WALK_READ 3)
    --reads 2    two ds_read_b64 at a8 = ad & ~7, a8 + 8                  (RCX_WALK_READ 2)

The bank rule and the lane groups are those of the hardware guide's LDS table (MI355X_MICROARCH.md, "LDS [CDNA4]": `ds_read_b32` and
`ds_read_b64` are both served in two groups of 32 lanes, {0-31} and {32-63}, one LDS cycle a group when conflict-free; the bank of byte
address a is (a / 4) mod 32 for `ds_read_b32` and (a / 4) mod 64 for `ds_read_b64`; identical addresses broadcast, and each further
distinct address on a busy bank adds a cycle -- `SQ_LDS_BANK_CONFLICT` counts the extra cycles, `SQ_LDS_IDX_ACTIVE` all of them).  So the
cost of one read for one group is the largest number of distinct dword addresses that fall on one bank, 0 for a group with no lane
left; "conflict-free" is 1 for every group with a lane.  The byte read for a match-length extension beyond the eight bytes in hand
(`ds_read_u8`) is counted apart: it is the same under either shape.

Figures are per BATCH OF 56 TOKENS (the headline's 5488 tokens a block in 98 batches), the unit of the profiles' per-batch counters.
The input is the benchmark's: G-text blocks of 64 KiB from synth.gen_blocks, compressed by the oracle's block encoder."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np

NSEG = 64                                                   # lanes = segments a chunk
TOKENS_A_BATCH = 56
CBUF_BASE = 0                                               # LDS address of the staged chunk: 16-byte aligned, which is all the banks see of it


def next_tok(buf, p, n):
    """where the token after the one at p starts (n: there is none) -- the kernel's next_tok, which never leaves the block on garbage"""
    t = buf[p]; q = p + 1
    L = t >> 4
    if L == 15:
        while True:
            if q >= n:
                return n, 0
            x = buf[q]; q += 1; L += x
            if x != 255:
                break
    if L >= n - q:
        return n, 0
    q += L
    if n - q < 2:
        return n, 0
    hop = q + 2 - p
    q += 2
    far = 0
    if (t & 15) == 15:
        far = 1 if hop > 7 else 0                           # the extension byte lies beyond the eight bytes in hand: a ds_read_u8
        while True:
            if q >= n:
                return n, far
            x = buf[q]; q += 1
            if x != 255:
                break
    return q, far


def group_cost(addrs, width, nbanks):
    """LDS cycles of one read for one 32-lane group: addrs = the lanes' (aligned) byte addresses, width = dwords a lane"""
    if not addrs:
        return 0
    per_bank = {}
    for a in set(addrs):
        for k in range(width):
            d = a // 4 + k
            per_bank.setdefault(d % nbanks, set()).add(d)
    return max(len(s) for s in per_bank.values())


def step_cost(ads, reads):
    """(cycles, conflict-free cycles) of one step's reads: ads = {lane: LDS address of its token}"""
    cyc = free = 0
    for lo in (0, 32):
        g = [a for l, a in ads.items() if lo <= l < lo + 32]
        if not g:
            continue
        if reads == 3:
            for k in range(3):
                cyc += group_cost([(a & ~3) + 4 * k for a in g], 1, 32); free += 1
        else:
            for k in range(2):
                cyc += group_cost([(a & ~7) + 8 * k for a in g], 2, 64); free += 1
    return cyc, free


def walk_block(buf, reads, segb, pre, inmis):
    """-> dict of totals for one block: steps, read cycles, conflict-free cycles, tokens, byte reads"""
    n = len(buf)
    ch = segb * NSEG
    tot = dict(steps=0, cycles=0, free=0, tokens=0, u8=0, start_cycles=0, chunks=0)
    # the true walk: every token start
    starts, p = [], 0
    while p < n:
        starts.append(p)
        p, _ = next_tok(buf, p, n)
    tot["tokens"] = len(starts)
    starts.append(n)
    si = 0
    c, cs = 0, -inmis
    while c < n:
        cbase = cs - pre
        nseg = NSEG if n - cs >= ch else (n - cs + segb - 1) // segb
        k0 = (c - cs) // segb
        nx, _ = next_tok(buf, c, n)
        giant = nx >= n or nx >= cs + ch
        pos, bound = {}, {}
        if not giant and n >= 20:
            for l in range(k0, nseg):
                s = cs + segb * l
                e = min(s + segb, n)
                pos[l] = c if l == k0 else max(s - pre, 0)
                bound[l] = min(e, n - 19)
        first = True
        while True:
            act = {l: p for l, p in pos.items() if p < bound[l]}
            if not act:
                break
            cyc, free = step_cost({l: p - cbase + CBUF_BASE for l, p in act.items()}, reads)
            tot["steps"] += 1; tot["cycles"] += cyc; tot["free"] += free
            if first:
                tot["start_cycles"] += cyc; first = False
            for l, p in act.items():
                q, far = next_tok(buf, p, n)
                pos[l] = q; tot["u8"] += far
            for l in list(pos):                              # (exec stays narrowed)
                if pos[l] >= bound[l]:
                    del pos[l], bound[l]
        tot["chunks"] += 1
        while starts[si] < cs + ch and starts[si] < n:      # the true cursor enters the next chunk at the first token start behind this one
            si += 1
        c = starts[si]
        ncs = cs + ch                                       # (run_parser8: a token that jumps over a whole chunk takes the chunk grid with it)
        if c < n and c >= ncs + ch:
            ncs = ((c + inmis) & ~15) - inmis
        cs = ncs
    return tot


def blocks(kind, nblocks, block_bytes, seed):
    import oracle_py as O
    from rust_compress_amd import synth
    O.build()
    raw = synth.gen_blocks(kind, nblocks, block_bytes, seed)
    return [O.lz4_encode_block(raw[i * block_bytes:(i + 1) * block_bytes].tobytes()) for i in range(nblocks)]


def model(blobs, reads, segb, pre, inmis=0):
    keys = ("steps", "cycles", "free", "tokens", "u8", "start_cycles", "chunks")
    t = dict.fromkeys(keys, 0)
    for b in blobs:
        r = walk_block(np.frombuffer(b, np.uint8).tolist(), reads, segb, pre, inmis)
        for k in keys:
            t[k] += r[k]
    nb = len(blobs)
    batches = t["tokens"] / TOKENS_A_BATCH
    return dict(reads=reads, seg=segb, pre=pre, cycles_a_batch=t["cycles"] / batches, free_a_batch=t["free"] / batches,
                conflicts_a_batch=(t["cycles"] - t["free"]) / batches, steps_a_block=t["steps"] / nb, tokens_a_block=t["tokens"] / nb,
                reads_a_batch=t["steps"] * reads / batches, u8_a_batch=t["u8"] / batches, first_step_cycles=t["start_cycles"] / max(1, t["chunks"]))


def row(m):
    what = "3 x ds_read_b32" if m["reads"] == 3 else "2 x ds_read_b64"
    return "| %s | %d / %d | %.1f (conflict-free: %.1f, conflicts: %.1f) | %.1f | %.2f | %.1f | %.2f |" % (
        what, m["seg"], m["pre"], m["cycles_a_batch"], m["free_a_batch"], m["conflicts_a_batch"], m["steps_a_block"], m["reads_a_batch"],
        m["first_step_cycles"], m["u8_a_batch"])


HEAD = ("| walk reads | segment / head start | LDS-array cycles a batch of 56 tokens | steps a block | read instructions a batch | cycles of a chunk's first step | ds_read_u8 a batch |\n"
        "|---|---|---|---|---|---|---|")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, choices=(2, 3), help="read shape; without it: the notebook's table")
    ap.add_argument("--seg", type=int, default=64, help="segment size, bytes (a lane's share of a chunk)")
    ap.add_argument("--pre", type=int, default=128, help="head start of a guessing lane, bytes")
    ap.add_argument("--inmis", type=int, default=0, help="the input's misalignment mod 16")
    ap.add_argument("--kind", default="text")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block-bytes", type=int, default=65536)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4C5A3401)
    a = ap.parse_args()
    blobs = blocks(a.kind, a.blocks, a.block_bytes, a.seed)
    print("%d blocks of %d bytes, G-%s, compressed to %.0f bytes a block; input misalignment %d" % (a.blocks, a.block_bytes, a.kind, sum(map(len, blobs)) / len(blobs), a.inmis))
    print(HEAD)
    shapes = [(a.reads, a.seg, a.pre)] if a.reads else [(3, 64, 128), (3, 60, 128), (2, 64, 128), (2, 56, 128), (2, 60, 128)]
    for reads, seg, pre in shapes:
        if (seg * NSEG) % 16 or pre % 16:
            sys.exit("a chunk and the head start are multiples of 16 bytes (staging is 16 bytes a lane)")
        print(row(model(blobs, reads, seg, pre, a.inmis)))


if __name__ == "__main__":
    main()
