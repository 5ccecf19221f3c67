#!/usr/bin/env python3
"""What reading bzip2 costs (rcx_bzip2_decode_batch).  One JSON line per measurement:

  small_files   FILES files of one 64 KiB G-text block each (level 9)
  big_files     BIG level-9 files of 4 MiB of G-text each (five blocks a file)
  one_file      ONE level-9 file of ONE_MIB MiB of G-text
  libbz2        the same workloads through Python's bz2 on THREADS host threads, one file a thread (one_file on one thread), the baseline to
                report against

A time is the host clock around one synchronous call (descriptor copies, staging and the launch loop with its read-backs included), REPS
calls after WARM warm-up calls, device-resident and from pageable host memory; min, median and max are reported, and rates are DECODED bytes
per second.  Every call's bytes are compared with the text.  There is no gate on a time.  FILES / BIG / ONE_MIB / REPS / LEGS in the
environment shrink the runs; --out FILE appends the lines to FILE; --once runs each device leg one time (for a profiler); --sweep times
the first two workloads, device-resident, at 512, 1024, 1536 and 2048 block candidates a round (rcx_ctx_set_param(ctx, RCX_BZIP2_DECODE, r);
ROUND in the environment sets it for the other legs, 0 = the library's default)."""
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
REPS, WARM = int(os.environ.get("REPS", "10")), 1
THREADS = int(os.environ.get("THREADS", "16"))
LEGS = [x for x in os.environ.get("LEGS", "small_files,big_files,one_file").split(",") if x]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
ONCE, NO_HOST, SWEEP = "--once" in sys.argv, "--no-libbz2" in sys.argv, "--sweep" in sys.argv
ROUND = int(os.environ.get("ROUND", "0"))
RCX_BZIP2_DECODE = 46
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
            "decoded_mib_per_s_median": round(nbytes / 2**20 / med * 1e3, 1)}


def workload(leg):
    """-> (texts, files): the plain texts and their .bz2 files, compressed on THREADS threads (bz2 releases the interpreter lock)"""
    if leg == "small_files":
        raw = synth.gen_blocks("text", FILES, 65536, 0xB200)
        texts = [raw[i * 65536:(i + 1) * 65536].tobytes() for i in range(FILES)]
    elif leg == "big_files":
        texts = [synth.gen_blocks("text", 64, 65536, 0xB300 + i).tobytes() for i in range(BIG)]
    else:
        texts = [synth.gen_blocks("text", ONE_MIB * 16, 65536, 0xB400).tobytes()]
    with ThreadPoolExecutor(THREADS) as ex:
        files = list(ex.map(lambda t: bz2.compress(t, 9), texts))
    return texts, files


def host_leg(leg, texts, files):
    threads = 1 if leg == "one_file" else THREADS
    ms = []
    for r in range(REPS):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            outs = list(ex.map(bz2.decompress, files))
        ms.append((time.perf_counter() - t0) * 1e3)
        assert all(len(o) == len(t) for o, t in zip(outs, texts))
    emit(dict({"bench": "libbz2_python", "workload": leg, "threads": threads, "files": len(files), "compressed_bytes": sum(map(len, files))},
              **stats(ms, sum(map(len, texts)))))


def device_leg(leg, texts, files, where, round=None, reps=None):
    import torch
    import rust_compress_amd as R
    from rust_compress_amd import _native as N
    global ctx
    if ctx is None:
        ctx = R.Context(0)
    lib = N.lib()
    round = ROUND if round is None else round
    assert lib.rcx_ctx_set_param(ctx._h, RCX_BZIP2_DECODE, round) == 0
    n = len(files)
    in_len = np.array([len(f) for f in files], np.uint64)
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
    inb = np.frombuffer(b"".join(files) + b"\0" * 16, np.uint8)
    out_cap = np.array([len(t) for t in texts], np.uint64)
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
    for r in range(1 if ONCE else WARM + (reps or REPS)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rcx_bzip2_decode_batch(ctx._h, C.byref(b))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and not status.any(), (rc, lib.rcx_last_error(ctx._h), status[:8])
        if ONCE or r >= WARM:
            ms.append(dt)
    o = d_out.cpu().numpy() if where == "device" else h_out
    want = np.frombuffer(b"".join(texts), np.uint8)
    assert (out_len == out_cap).all() and (in_used == in_len).all() and np.array_equal(o[:total], want), "decoded bytes differ from the text"
    emit(dict({"bench": "round_sweep" if reps else "rcx_bzip2_decode_batch", "workload": leg, "memory": where, "candidates_a_round": round or 1536, "files": n, "compressed_bytes": int(in_len.sum()),
               "decoded_bytes": total, "blocks": int(sum((len(t) + 899999) // 900000 for t in texts))}, **stats(ms, total)))


ctx = None
if __name__ == "__main__":
    import torch
    emit({"bench": "bzip2_decode_rate", "reps": REPS, "warm": WARM, "device": torch.cuda.get_device_name(0), "threads": THREADS})
    for leg in LEGS:
        t0 = time.perf_counter()
        texts, files = workload(leg)
        emit({"bench": "workload", "workload": leg, "files": len(files), "seconds_to_make": round(time.perf_counter() - t0, 1)})
        if SWEEP:
            if leg != "one_file":
                for r in (512, 1024, 1536, 2048):
                    device_leg(leg, texts, files, "device", round=r, reps=5)
            continue
        for where in ("device",) if ONCE else ("device", "host"):
            device_leg(leg, texts, files, where)
        if not ONCE and not NO_HOST:
            host_leg(leg, texts, files)
    if ctx is not None:
        ctx.close()
