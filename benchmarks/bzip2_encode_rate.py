#!/usr/bin/env python3
"""What writing bzip2 costs (rcx_bzip2_encode_batch).  One JSON line per measurement:

  small_files   FILES files of 64 KiB of G-text each (level 9: one block a file)
  big_files     BIG files of 4 MiB of G-text each (level 9: five blocks a file)
  one_file      ONE file of ONE_MIB MiB of G-text (level 9)
  libbz2        the same workloads through Python's bz2.compress(level 9) on THREADS host threads, one file a thread (one_file on one
                thread), the baseline to report against, HOST_REPS times

A time is the host clock around one synchronous call (descriptor copies, staging and the launch loop with its read-backs included), REPS
calls after WARM warm-up calls, device-resident and from pageable host memory; min, median and max are reported, and rates are INPUT bytes
per second.  Every file of the last call is read back by libbz2 and compared with its text, and the total size is reported against
libbz2's.  There is no gate on a time.  FILES / BIG / ONE_MIB / REPS / HOST_REPS / LEGS in the environment shrink the runs; --out FILE
appends the lines to FILE; --once runs each device leg one time (for a profiler); ROUND in the environment sets the blocks a round
(rcx_ctx_set_param(ctx, RCX_BZIP2_ENCODE, r), 0 = the library's default)."""
import bz2
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rust_compress_amd import synth  # noqa: E402

FILES, BIG, ONE_MIB = int(os.environ.get("FILES", "4096")), int(os.environ.get("BIG", "256")), int(os.environ.get("ONE_MIB", "256"))
REPS, HOST_REPS, WARM = int(os.environ.get("REPS", "10")), int(os.environ.get("HOST_REPS", "3")), 1
THREADS = int(os.environ.get("THREADS", "16"))
LEGS = [x for x in os.environ.get("LEGS", "small_files,big_files,one_file").split(",") if x]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
ONCE, NO_HOST = "--once" in sys.argv, "--no-libbz2" in sys.argv
ROUND = int(os.environ.get("ROUND", "0"))
LEVEL = 9
RCX_BZIP2_ENCODE = 47
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
    return {"ms_min": round(ms[0], 3), "ms_median": round(med, 3), "ms_max": round(ms[-1], 3), "reps": len(ms),
            "input_mib_per_s_median": round(nbytes / 2**20 / med * 1e3, 1)}


def workload(leg):
    if leg == "small_files":
        raw = synth.gen_blocks("text", FILES, 65536, 0xB200)
        return [raw[i * 65536:(i + 1) * 65536].tobytes() for i in range(FILES)]
    if leg == "big_files":
        return [synth.gen_blocks("text", 64, 65536, 0xB300 + i).tobytes() for i in range(BIG)]
    return [synth.gen_blocks("text", ONE_MIB * 16, 65536, 0xB400).tobytes()]


def host_leg(leg, texts):
    """-> libbz2's total size"""
    threads = 1 if leg == "one_file" else THREADS
    ms, outs = [], []
    for r in range(HOST_REPS):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            outs = list(ex.map(lambda t: bz2.compress(t, LEVEL), texts))
        ms.append((time.perf_counter() - t0) * 1e3)
    total = sum(map(len, outs))
    emit(dict({"bench": "libbz2_python", "workload": leg, "threads": threads, "files": len(texts), "compressed_bytes": total},
              **stats(ms, sum(map(len, texts)))))
    return total


def device_leg(leg, texts, where):
    """-> the encoder's total size"""
    import torch
    import rust_compress_amd as R
    from rust_compress_amd import _native as N
    global ctx
    if ctx is None:
        ctx = R.Context(0)
    lib = N.lib()
    assert lib.rcx_ctx_set_param(ctx._h, RCX_BZIP2_ENCODE, ROUND) == 0
    n = len(texts)
    in_len = np.array([len(t) for t in texts], np.uint64)
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
    inb = np.frombuffer(b"".join(texts) + b"\0" * 16, np.uint8)
    out_cap = (in_len + in_len // np.uint64(64) + np.uint64(1024)).astype(np.uint64)          # the first capacity include/rcx.h names
    out_off = np.concatenate([[0], np.cumsum(out_cap)[:-1]]).astype(np.uint64)
    total = int(out_cap.sum())
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    if where == "device":
        d_in, d_out = torch.from_numpy(inb.copy()).cuda(), torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        b = N.Batch(d_in.data_ptr(), p(in_off), p(in_len), d_out.data_ptr(), p(out_off), p(out_cap), p(out_len), p(in_used), p(status), n, N.MEM_DEVICE)
    else:
        h_out = np.zeros(total + 16, np.uint8)
        b = N.Batch(p(inb), p(in_off), p(in_len), p(h_out), p(out_off), p(out_cap), p(out_len), p(in_used), p(status), n, N.MEM_HOST)
    ms = []
    for r in range(1 if ONCE else WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rcx_bzip2_encode_batch(ctx._h, C.byref(b), LEVEL)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and not status.any(), (rc, lib.rcx_last_error(ctx._h), status[:8])
        if ONCE or r >= WARM:
            ms.append(dt)
    o = d_out.cpu().numpy() if where == "device" else h_out
    streams = [o[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
    with ThreadPoolExecutor(THREADS) as ex:
        back = list(ex.map(bz2.decompress, streams))
    assert (in_used == in_len).all() and all(x == t for x, t in zip(back, texts)), "libbz2 does not read the text back"
    size = int(out_len.sum())
    emit(dict({"bench": "rcx_bzip2_encode_batch", "workload": leg, "memory": where, "level": LEVEL, "blocks_a_round": ROUND or 1024, "files": n,
               "input_bytes": int(in_len.sum()), "compressed_bytes": size},
              **stats(ms, int(in_len.sum()))))
    return size


ctx = None
if __name__ == "__main__":
    import torch
    emit({"bench": "bzip2_encode_rate", "reps": REPS, "host_reps": HOST_REPS, "warm": WARM, "device": torch.cuda.get_device_name(0), "threads": THREADS})
    for leg in LEGS:
        t0 = time.perf_counter()
        texts = workload(leg)
        emit({"bench": "workload", "workload": leg, "files": len(texts), "seconds_to_make": round(time.perf_counter() - t0, 1)})
        ours = None
        for where in ("device",) if ONCE else ("device", "host"):
            ours = device_leg(leg, texts, where)
        if not ONCE and not NO_HOST:
            theirs = host_leg(leg, texts)
            emit({"bench": "size_against_libbz2", "workload": leg, "ours": ours, "libbz2": theirs, "ratio": round(ours / theirs, 5)})
    if ctx is not None:
        ctx.close()
