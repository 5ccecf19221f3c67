#!/usr/bin/env python3
"""Rates of the two device calls behind rust_compress_amd.lz4frame, device-resident data (RCX_MEM_DEVICE), one JSON line each:

  (a) rcx_xxh32_batch          4096 x 64 KiB blocks; one 256 MiB stream (the per-stream serial bound)
  (b) rcx_lz4_decode_linked_batch
        4096 independent 64 KiB blocks (link all zero) against rcx_lz4_decode_batch on the same blocks, calls alternating
        256 chains of 16 linked ~64 KiB blocks (16 launches, one per depth)

Both are *_batch calls: synchronous, the small descriptor arrays travel with every call.  A time is the host clock around one call
(it ends in a stream synchronise), so it holds the descriptor copies and the launches, not the kernels alone; GiB/s = bytes hashed or
bytes decoded / that time.  REPS calls after WARM warm-up calls; min, median and max are reported: the spread is the reader's to judge.

The linked chains: the project has no linked ENCODER, so a chain is made from one 1 MiB block of the greedy encoder (its matches reach
back 65535 bytes whatever the block's size), cut at sequence boundaries into 16 pieces of about 64 KiB, each ended by an empty
last-literals token -- piece k's matches reach into pieces before it exactly as a linked frame's blocks do.  TEMPLATES such streams,
repeated to 256 chains at distinct addresses; every chain's output is compared with the text it came from.
NB / CHAINS / BIG_MIB / REPS in the environment shrink the runs; --out FILE appends the lines to FILE."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import rust_compress_amd as R  # noqa: E402
from rust_compress_amd import _native as N, synth  # noqa: E402

BLOCK = 65536
NB = int(os.environ.get("NB", "4096"))
CHAINS, DEPTH, TEMPLATES = int(os.environ.get("CHAINS", "256")), 16, 4
BIG = int(os.environ.get("BIG_MIB", "256")) << 20
REPS, WARM = int(os.environ.get("REPS", "10")), 2
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda", 0)
ctx = R.Context(0)
lib = N.lib()
p = lambda a: a.ctypes.data


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_min": round(ms[0], 4), "ms_median": round(med, 4), "ms_max": round(ms[-1], 4), "reps": len(ms),
            "gib_per_s_median": round(nbytes / 2**30 / med * 1e3, 3), "gib_per_s_best": round(nbytes / 2**30 / ms[0] * 1e3, 3)}


def call(fn, reps=REPS, warm=WARM):
    out = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn()
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, lib.rcx_last_error(ctx._h)
        if i >= warm:
            out.append(dt)
    return out


class Dev:
    """a device-memory rcx_batch over torch buffers; the descriptor arrays are host numpy arrays"""

    def __init__(self, d_in, in_off, in_len, d_out=None, out_off=None, out_cap=None):
        n = len(in_off)
        self.n = n
        self.in_off, self.in_len = np.ascontiguousarray(in_off, np.uint64), np.ascontiguousarray(in_len, np.uint64)
        self.out_off = np.ascontiguousarray(out_off if out_off is not None else np.zeros(n), np.uint64)
        self.out_cap = np.ascontiguousarray(out_cap if out_cap is not None else np.zeros(n), np.uint64)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.keep = (d_in, d_out)
        self.b = N.Batch(d_in.data_ptr(), p(self.in_off), p(self.in_len), d_out.data_ptr() if d_out is not None else None, p(self.out_off),
                         p(self.out_cap), p(self.out_len), p(self.in_used), p(self.status), n, N.MEM_DEVICE)


# ---------------------------------------------------------------------------------------------------------------- (a) XXH32
def xxh32_rates():
    data = torch.from_numpy(synth.gen_blocks("text", NB, BLOCK, 0x4C5A)).to(dev)
    b = Dev(data, np.arange(NB) * BLOCK, [BLOCK] * NB)
    h = np.zeros(NB, np.uint32)
    ms = call(lambda: lib.rcx_xxh32_batch(ctx._h, C.byref(b.b), C.c_uint32(0), C.c_void_p(p(h))))
    assert not b.status.any()
    emit(dict({"bench": "xxh32_batch", "blocks": NB, "block_bytes": BLOCK}, **stats(ms, NB * BLOCK)))
    del data
    big = torch.from_numpy(np.resize(synth.gen("text", 4 << 20, 3), BIG)).to(dev)
    b1 = Dev(big, [0], [BIG])
    h1 = np.zeros(1, np.uint32)
    ms = call(lambda: lib.rcx_xxh32_batch(ctx._h, C.byref(b1.b), C.c_uint32(0), C.c_void_p(p(h1))), reps=max(REPS // 3, 3), warm=1)
    emit(dict({"bench": "xxh32_single_stream", "bytes": BIG, "hash": "%08x" % int(h1[0])}, **stats(ms, BIG)))


# ---------------------------------------------------------------------------------------------------------------- (b) linked decode
def decode_independent():
    raw = synth.gen_blocks("text", NB, BLOCK, 0x4C5A)
    enc = ctx.lz4_encode_blocks([raw[i * BLOCK:(i + 1) * BLOCK].tobytes() for i in range(NB)]).check()
    lens = np.array([len(e) for e in enc.outputs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    d_in = torch.from_numpy(np.frombuffer(b"".join(enc.outputs) + b"\0" * 64, np.uint8).copy()).to(dev)
    d_raw = torch.from_numpy(raw).to(dev)
    outs = [torch.zeros(NB * BLOCK + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
    plain = Dev(d_in, offs, lens, outs[0], np.arange(NB) * BLOCK, [BLOCK] * NB)
    linked = Dev(d_in, offs, lens, outs[1], np.arange(NB) * BLOCK, [BLOCK] * NB)
    link = np.zeros(NB, np.uint8)
    f_plain = lambda: lib.rcx_lz4_decode_batch(ctx._h, C.byref(plain.b))
    f_link = lambda: lib.rcx_lz4_decode_linked_batch(ctx._h, C.byref(linked.b), C.c_void_p(p(link)), None)
    for _ in range(WARM):
        call(f_plain, 1, 0); call(f_link, 1, 0)
    tp, tl = [], []
    for _ in range(REPS):                                          # alternating: both see the same machine
        tp += call(f_plain, 1, 0)
        tl += call(f_link, 1, 0)
    for b, o in ((plain, outs[0]), (linked, outs[1])):
        assert not b.status.any() and torch.equal(o[:NB * BLOCK], d_raw)
    emit(dict({"bench": "lz4_decode_batch", "blocks": NB, "block_bytes": BLOCK, "kind": "text"}, **stats(tp, NB * BLOCK)))
    emit(dict({"bench": "lz4_decode_linked_batch_independent", "blocks": NB, "block_bytes": BLOCK, "kind": "text"}, **stats(tl, NB * BLOCK)))


def cut_chain(block, raw_len, pieces):
    """one LZ4 block -> `pieces` linked blocks, cut at sequence boundaries near every raw_len / pieces bytes -> [(block bytes, raw bytes)]"""
    n, q, produced, start, start_raw, out = len(block), 0, 0, 0, 0, []
    step = raw_len // pieces
    while q < n:
        t = block[q]
        s = q + 1
        L = t >> 4
        if L == 15:
            while True:
                x = block[s]; s += 1; L += x
                if x != 255:
                    break
        s += L
        produced += L
        if s >= n:                                                 # the block's own last sequence
            out.append((block[start:n], produced - start_raw))
            break
        s += 2
        M = t & 15
        if M == 15:
            while True:
                x = block[s]; s += 1; M += x
                if x != 255:
                    break
        produced += M + 4
        q = s
        if len(out) < pieces - 1 and produced >= (len(out) + 1) * step:
            out.append((block[start:q] + b"\x00", produced - start_raw))
            start, start_raw = q, produced
    return out


def decode_chains():
    stream = DEPTH * BLOCK
    raws = [synth.gen("text", stream, 0x51 + i).tobytes() for i in range(TEMPLATES)]
    enc = ctx.lz4_encode_blocks(raws).check().outputs
    chains = [cut_chain(e, stream, DEPTH) for e in enc]
    assert all(len(c) == DEPTH and sum(r for _, r in c) == stream for c in chains)
    buf, in_off, in_len, link, out_off, out_cap = bytearray(), [], [], [], [], []
    for c in range(CHAINS):
        for k, (blk, _) in enumerate(chains[c % TEMPLATES]):
            in_off.append(len(buf)); in_len.append(len(blk)); link.append(1 if k else 0)
            out_off.append(c * stream if not k else 0); out_cap.append(stream if not k else 0)
            buf += blk
    d_in = torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 64, np.uint8).copy()).to(dev)
    d_out = torch.zeros(CHAINS * stream + 64, dtype=torch.uint8, device=dev)
    b = Dev(d_in, in_off, in_len, d_out, out_off, out_cap)
    lk = np.array(link, np.uint8)
    ms = call(lambda: lib.rcx_lz4_decode_linked_batch(ctx._h, C.byref(b.b), C.c_void_p(p(lk)), None))
    assert not b.status.any(), b.status[:40]
    got = d_out.cpu().numpy()
    for c in range(CHAINS):
        assert got[c * stream:(c + 1) * stream].tobytes() == raws[c % TEMPLATES], c
    emit(dict({"bench": "lz4_decode_linked_batch_chains", "chains": CHAINS, "depth": DEPTH, "launches": DEPTH, "block_bytes": BLOCK,
               "kind": "text", "compressed_bytes": len(buf)}, **stats(ms, CHAINS * stream)))


if __name__ == "__main__":
    emit({"bench": "lz4_frame_rate", "device": torch.cuda.get_device_name(0), "reps": REPS, "warm": WARM})
    xxh32_rates()
    decode_independent()
    decode_chains()
    ctx.close()
