#!/usr/bin/env python3
"""DEFLATE encode rate and ratio per compression level (extension: the reference has no DEFLATE encoder).  For every level 1..9: raw
DEFLATE through rcx_launch_dev with the level as the codec parameter, event-timed (the best of TIMED launches after one warm-up), input
GiB/s and ratio, for 4096 x 64 KiB G-text / G-words / G-runs / G-rand and one 256 MiB G-text stream; Python's zlib at the same level
on 16 threads on the same data (the 256 MiB stream in 16 MiB pieces) for comparison; a sample of streams checked with Python's zlib.
The per-kernel split: run this under
    rocprofv3 --kernel-trace --stats -d <dir> -- python benchmarks/deflate_level_rate.py
Arguments: the levels (default 1..9).  NB / BIG_MIB / THREADS / TIMED / KINDS (comma-separated) / CPU=0 in the environment shrink
the runs."""
import os, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rust_compress_amd as R
from rust_compress_amd import _native as N, synth

BLOCK, NB = 65536, int(os.environ.get("NB", "4096"))
BIG = int(os.environ.get("BIG_MIB", "256")) << 20
THREADS = int(os.environ.get("THREADS", "16"))
TIMED = int(os.environ.get("TIMED", "3"))
KINDS = os.environ.get("KINDS", "text,words,runs,rand,big-text").split(",")
CPU = os.environ.get("CPU", "1") != "0"
dev = torch.device("cuda", 0)
ctx = R.Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def gpu(raw_h, lens, level):
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    caps = np.array([R.api.deflate_bound(int(x)) for x in lens], np.int64)
    caps = (caps + 15) & ~15
    ooff = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    raw = torch.from_numpy(raw_h).to(dev)
    b = R.DeviceBatch(raw, i64(offs), i64(lens), torch.zeros(int(caps.sum()) + 64, dtype=torch.uint8, device=dev), i64(ooff), i64(caps))
    scratch = torch.empty(int(N.lib().rcx_deflate_level_scratch_bytes(n, int(max(lens)))), dtype=torch.uint8, device=dev)
    assert N.lib().rcx_ctx_set_param(ctx._h, N.DEFLATE_ENCODE, level) == 0
    try:
        ctx.launch_dev(N.DEFLATE_ENCODE, b, scratch); torch.cuda.synchronize()
        assert int(b.status.abs().max()) == 0
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(TIMED + 1)]
        for i in range(TIMED):
            ev[i].record(); ctx.launch_dev(N.DEFLATE_ENCODE, b, scratch)
        ev[TIMED].record(); torch.cuda.synchronize()
    finally:
        N.lib().rcx_ctx_set_param(ctx._h, N.DEFLATE_ENCODE, 0)
    ms = min(ev[i].elapsed_time(ev[i + 1]) for i in range(TIMED))
    ol = b.out_len[:n].cpu().numpy()
    ob = b.out_base.cpu().numpy()
    for i in sorted({0, n // 2, n - 1}):
        e = ob[ooff[i]:ooff[i] + ol[i]].tobytes()
        assert zlib.decompress(e, -15) == raw_h[offs[i]:offs[i] + lens[i]].tobytes()
    del raw, scratch, b
    return ms, float(ol.sum())


def cpu_zlib(raw_h, lens, level):
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    mv = memoryview(raw_h)
    if len(lens) == 1:                                   # one stream: 16 MiB pieces (what a parallel CPU encoder would do)
        piece = 16 << 20
        parts = [(o, min(piece, int(lens[0]) - o)) for o in range(0, int(lens[0]), piece)]
    else:
        parts = [(int(offs[i]), int(lens[i])) for i in range(len(lens))]

    def one(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(c.compress(mv[parts[i][0]:parts[i][0] + parts[i][1]]) + c.flush())
    t = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        total = sum(ex.map(one, range(len(parts))))
    return (time.perf_counter() - t) * 1e3, float(total)


data = {}
for kind in KINDS:
    if kind == "big-text":
        data[kind] = (synth.gen_blocks("text", BIG // BLOCK, BLOCK, 0x4C5A), np.array([BIG], np.int64))
    else:
        data[kind] = (synth.gen_blocks(kind, NB, BLOCK, 0x4C5A), np.full(NB, BLOCK, np.int64))
for level in [int(x) for x in sys.argv[1:]] or range(1, 10):
    for kind in KINDS:
        raw_h, lens = data[kind]
        ms, out = gpu(raw_h, lens, level)
        gib = raw_h.size / 2**30
        line = "level %d %-9s GPU %9.3f ms %8.2f GiB/s ratio %.3f" % (level, kind, ms, gib / ms * 1e3, raw_h.size / out)
        if CPU:
            cms, cout = cpu_zlib(raw_h, lens, level)
            line += " | CPU zlib -%d x%d %9.1f ms %6.3f GiB/s ratio %.3f" % (level, THREADS, cms, gib / cms * 1e3, raw_h.size / cout)
        print(line, flush=True)
