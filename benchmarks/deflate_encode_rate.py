#!/usr/bin/env python3
"""DEFLATE encode rate (extension: the reference has no DEFLATE encoder).  Raw DEFLATE through rcx_launch_dev, event-timed, input GiB/s
and ratio for 4096 x 64 KiB G-text / G-words / G-rand and one 256 MiB G-text stream (that one also as zlib and gzip: their Adler-32 /
CRC-32 give ONE wave to a stream); CPU zlib level 1 on 16 threads on the same data for comparison; the host-memory entry point on the
G-text batch (its copies in and out, and the output span copied in first); a sample of streams checked with Python's zlib.  The per-kernel split: run this under
    rocprofv3 --kernel-trace --stats -d <dir> -- python benchmarks/deflate_encode_rate.py
NB / BIG_MIB / THREADS in the environment shrink the runs."""
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
dev = torch.device("cuda", 0)
ctx = R.Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def gpu(raw_h, lens, codec=N.DEFLATE_ENCODE):
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    caps = np.array([R.api.deflate_bound(int(x)) + 18 for x in lens], np.int64)
    caps = (caps + 15) & ~15
    ooff = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    raw = torch.from_numpy(raw_h).to(dev)
    b = R.DeviceBatch(raw, i64(offs), i64(lens), torch.zeros(int(caps.sum()) + 64, dtype=torch.uint8, device=dev), i64(ooff), i64(caps))
    scratch = torch.empty(ctx.scratch_bytes(codec, n, int(max(lens))), dtype=torch.uint8, device=dev)
    ctx.launch_dev(codec, b, scratch); torch.cuda.synchronize()
    assert int(b.status.abs().max()) == 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for i in range(3):
        ev[i].record(); ctx.launch_dev(codec, b, scratch)
    ev[3].record(); torch.cuda.synchronize()
    ms = min(ev[i].elapsed_time(ev[i + 1]) for i in range(3))
    ol = b.out_len[:n].cpu().numpy()
    ob = b.out_base.cpu().numpy()
    for i in sorted({0, n // 2, n - 1}):
        e = ob[ooff[i]:ooff[i] + ol[i]].tobytes()
        wb = {N.DEFLATE_ENCODE: -15, N.ZLIB_ENCODE: 15, N.GZIP_ENCODE: 31}[codec]
        assert zlib.decompress(e, wb) == raw_h[offs[i]:offs[i] + lens[i]].tobytes()
    del raw, scratch, b
    return ms, float(ol.sum())


def host(raw_h, lens):
    """rcx_deflate_encode_batch from pageable host memory: ms a call (the best of three) and GiB/s of input"""
    import ctypes as C
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    caps = np.array([R.api.deflate_bound(int(x)) for x in lens], np.uint64)
    ooff = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    out = np.zeros(int(caps.sum()), np.uint8)
    ol, used, st = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    ln = np.ascontiguousarray(lens, np.uint64)
    p = lambda a: a.ctypes.data
    b = N.Batch(p(raw_h), p(offs), p(ln), p(out), p(ooff), p(caps), p(ol), p(used), p(st), n, N.MEM_HOST)
    best = 1e30
    for _ in range(3):
        t = time.perf_counter()
        assert N.lib().rcx_deflate_encode_batch(ctx._h, C.byref(b)) == 0
        best = min(best, (time.perf_counter() - t) * 1e3)
    assert not st.any()
    return best


def cpu_zlib1(raw_h, lens):
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    mv = memoryview(raw_h)
    def one(i):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(c.compress(mv[offs[i]:offs[i] + lens[i]]) + c.flush())
    if len(lens) == 1:                                   # one stream: 16 threads on 16 MiB pieces (what a parallel CPU encoder would do)
        piece = 16 << 20
        pieces = [(o, min(piece, lens[0] - o)) for o in range(0, int(lens[0]), piece)]
        def one(i):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            return len(c.compress(mv[pieces[i][0]:pieces[i][0] + pieces[i][1]]) + c.flush())
        idx = range(len(pieces))
    else:
        idx = range(len(lens))
    t = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        total = sum(ex.map(one, idx))
    return (time.perf_counter() - t) * 1e3, float(total)


for kind in sys.argv[1:] or ["text", "words", "rand", "big-text", "big-text-zlib", "big-text-gzip", "host-text"]:
    if kind.startswith("big-text-"):
        raw_h = synth.gen_blocks("text", BIG // BLOCK, BLOCK, 0x4C5A); lens = np.array([BIG], np.int64)
        ms, out = gpu(raw_h, lens, N.ZLIB_ENCODE if kind.endswith("zlib") else N.GZIP_ENCODE)
        print("%-13s GPU %9.3f ms %8.2f GiB/s ratio %.3f" % (kind, ms, raw_h.size / 2**30 / ms * 1e3, raw_h.size / out), flush=True)
        continue
    if kind == "host-text":
        raw_h = synth.gen_blocks("text", NB, BLOCK, 0x4C5A); lens = np.full(NB, BLOCK, np.int64)
        ms = host(raw_h, lens)
        print("%-13s host memory in and out %9.3f ms %8.2f GiB/s" % (kind, ms, raw_h.size / 2**30 / ms * 1e3), flush=True)
        continue
    if kind == "big-text":
        raw_h = synth.gen_blocks("text", BIG // BLOCK, BLOCK, 0x4C5A); lens = np.array([BIG], np.int64)
    else:
        raw_h = synth.gen_blocks(kind, NB, BLOCK, 0x4C5A); lens = np.full(NB, BLOCK, np.int64)
    ms, out = gpu(raw_h, lens)
    cms, cout = cpu_zlib1(raw_h, lens)
    gib = raw_h.size / 2**30
    print("%-13s GPU %9.3f ms %8.2f GiB/s ratio %.3f | CPU zlib -1 x%d %9.1f ms %6.2f GiB/s ratio %.3f" % (
        kind, ms, gib / ms * 1e3, raw_h.size / out, THREADS, cms, gib / cms * 1e3, raw_h.size / cout), flush=True)
