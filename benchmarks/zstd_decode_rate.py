#!/usr/bin/env python3
"""What reading Zstandard costs (rcx_zstd_decode_batch).  One JSON line per measurement:

  frames        FILES frames of 64 KiB of G-text each, level 3
  records       RECORDS records of 2 KiB of G-text behind ONE 32 KiB raw-content dictionary, level 3
  one_frame     ONE frame of ONE_MIB MiB of G-text, level 3: a serial chain of 128 KiB blocks on one wave, measured to state the limit
  libzstd       the same files through ZSTD_decompressDCtx / ZSTD_decompress_usingDDict on THREADS host threads (one_frame on one thread),
                the comparison: a small C helper the script builds (pthreads; one foreign call a measurement; every thread loops over
                its files; output buffers, contexts and the digested dictionary are made outside the timed region) -- only where
                ctypes finds libzstd.so.1 and a C compiler on the machine this runs on.  Where it does not, nothing can be
                compressed either: the committed golden frames (tests/golden/zstd) are replicated across the batch, every line says
                "inputs": "golden_replicated", and the host comparison is null

A time is the host clock around one synchronous call (descriptor copies and staging included), the median of REPS calls after WARM
warm-up calls, device-resident and from pageable host memory; rates are DECODED bytes per second.  Every call's bytes are compared
with the text.  There is no gate on a time.  With RCX_AB=1 in the environment (the A/B library) every device-resident leg also times
a size query (capacities of 0: everything but the copies) and the profiling launch that ends a block behind its literals, and reports
the literal / sequence / execution shares of the call from the three.

With RCX_AB=1 the device-resident leg also times the executor built first (a sequence at a time, variant 2) against the shipped,
flattened one, alternating, REPS calls each.

Every step of every leg -- device-resident, pageable host memory, libzstd -- runs in a child process of its own under its own
`timeout`, one after the other, and the first one that fails ends the run.
FILES / RECORDS / ONE_MIB / REPS / LEGS in the environment shrink the runs; --out FILE appends the lines to FILE."""
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rust_compress_amd import synth  # noqa: E402

FILES, RECORDS, ONE_MIB = int(os.environ.get("FILES", "4096")), int(os.environ.get("RECORDS", "65535")), int(os.environ.get("ONE_MIB", "256"))
REPS, WARM = int(os.environ.get("REPS", "10")), 1
THREADS = int(os.environ.get("THREADS", "16"))
LEGS = [x for x in os.environ.get("LEGS", "frames,records,one_frame").split(",") if x]
LIMIT = {"frames": 240, "records": 240, "one_frame": 560}          # seconds a step (a 256 MiB frame takes 17 s a call)
STEPS = ("device", "host", "libzstd")
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
RCX_ZSTD_DECODE = 48
p = lambda a: a.ctypes.data


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def libzstd():
    try:
        z = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    for f in ("ZSTD_compress", "ZSTD_compressBound", "ZSTD_decompress", "ZSTD_decompress_usingDict", "ZSTD_compress_usingDict", "ZSTD_isError"):
        getattr(z, f).restype = C.c_size_t
    z.ZSTD_createCCtx.restype = C.c_void_p
    z.ZSTD_createDCtx.restype = C.c_void_p
    return z


def workload(leg, z):
    """-> (texts, files, dictionary or None, how the inputs were made)"""
    if z is None:                                             # no compressor here: the committed frames, replicated
        import zstd_cases as Z
        if leg == "records":
            pool = [g for g in Z.golden() if g["dict"]]
        elif leg == "one_frame":
            pool = [g for g in Z.golden() if g["name"] == "text_300000_l3_sum"]
        else:
            pool = [g for g in Z.golden() if g["name"] in ("text_40000_l19_w10", "text_5000_l3", "words_20000_l1_w10", "runs_40000_l3_w10")]
        n = {"frames": FILES, "records": RECORDS, "one_frame": 1}[leg]
        picks = [pool[i % len(pool)] for i in range(n)]
        return [g["raw"] for g in picks], [g["blob"] for g in picks], pool[0]["dict"], "golden_replicated"
    d = None
    if leg == "frames":
        raw = synth.gen_blocks("text", FILES, 65536, 0x2500)
        texts = [raw[i * 65536:(i + 1) * 65536].tobytes() for i in range(FILES)]
    elif leg == "records":
        d = synth.gen("text", 32768, 1).tobytes()
        raw = synth.gen_blocks("text", (RECORDS * 2048 + 65535) // 65536, 65536, 0x2600)
        texts = [raw[i * 2048:(i + 1) * 2048].tobytes() for i in range(RECORDS)]
    else:
        texts = [synth.gen_blocks("text", ONE_MIB * 16, 65536, 0x2700).tobytes()]

    def comp(t):
        cap = z.ZSTD_compressBound(C.c_size_t(len(t)))
        dst = C.create_string_buffer(cap)
        if d is None:
            n = z.ZSTD_compress(dst, C.c_size_t(cap), t, C.c_size_t(len(t)), 3)
        else:
            cctx = C.c_void_p(z.ZSTD_createCCtx())
            n = z.ZSTD_compress_usingDict(cctx, dst, C.c_size_t(cap), t, C.c_size_t(len(t)), d, C.c_size_t(len(d)), 3)
            z.ZSTD_freeCCtx(cctx)
        assert not z.ZSTD_isError(C.c_size_t(n))
        return dst.raw[:n]
    with ThreadPoolExecutor(THREADS) as ex:                   # (ctypes releases the interpreter lock around a foreign call)
        files = list(ex.map(comp, texts))
    return texts, files, d, "libzstd_level_3"


def stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_min": round(ms[0], 3), "ms_median": round(med, 3), "ms_max": round(ms[-1], 3), "reps": len(ms),
            "decoded_mib_per_s_median": round(nbytes / 2**20 / med * 1e3, 1)}


HELPER = r"""
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>
typedef struct ZSTD_DCtx_s ZSTD_DCtx;
typedef struct ZSTD_DDict_s ZSTD_DDict;
ZSTD_DCtx* ZSTD_createDCtx(void);
size_t ZSTD_freeDCtx(ZSTD_DCtx*);
ZSTD_DDict* ZSTD_createDDict(const void*, size_t);
size_t ZSTD_freeDDict(ZSTD_DDict*);
size_t ZSTD_decompressDCtx(ZSTD_DCtx*, void*, size_t, const void*, size_t);
size_t ZSTD_decompress_usingDDict(ZSTD_DCtx*, void*, size_t, const void*, size_t, const ZSTD_DDict*);
typedef struct { const uint8_t* base; const uint64_t* off; const uint64_t* len; const uint64_t* raw; uint32_t n, first, step;
                 ZSTD_DCtx* dctx; const ZSTD_DDict* dd; uint8_t* dst; size_t cap; uint32_t bad; } job;
static void* work(void* p)
{
    job* j = (job*)p;
    for (uint32_t i = j->first; i < j->n; i += j->step) {
        const size_t r = j->dd ? ZSTD_decompress_usingDDict(j->dctx, j->dst, j->cap, j->base + j->off[i], j->len[i], j->dd)
                               : ZSTD_decompressDCtx(j->dctx, j->dst, j->cap, j->base + j->off[i], j->len[i]);
        if (r != j->raw[i]) j->bad++;
    }
    return 0;
}
/* ms[r]: the wall time of decoding all n files on `threads` threads, thread t taking files t, t + threads, ...; -> files that failed */
int host_decode(const uint8_t* base, const uint64_t* off, const uint64_t* len, const uint64_t* raw, uint32_t n, const uint8_t* dict,
                uint64_t dlen, size_t cap, int threads, int reps, double* ms)
{
    job* js = (job*)calloc(threads, sizeof(job));
    pthread_t* th = (pthread_t*)calloc(threads, sizeof(pthread_t));
    ZSTD_DDict* dd = dlen ? ZSTD_createDDict(dict, dlen) : 0;
    uint32_t bad = 0;
    for (int t = 0; t < threads; t++) {
        job j = {base, off, len, raw, n, (uint32_t)t, (uint32_t)threads, ZSTD_createDCtx(), dd, (uint8_t*)malloc(cap + 64), cap, 0};
        js[t] = j;
    }
    for (int r = 0; r < reps; r++) {
        struct timespec a, b;
        clock_gettime(CLOCK_MONOTONIC, &a);
        for (int t = 1; t < threads; t++) pthread_create(&th[t], 0, work, &js[t]);
        work(&js[0]);
        for (int t = 1; t < threads; t++) pthread_join(th[t], 0);
        clock_gettime(CLOCK_MONOTONIC, &b);
        ms[r] = (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) / 1e6;
    }
    for (int t = 0; t < threads; t++) { bad += js[t].bad; ZSTD_freeDCtx(js[t].dctx); free(js[t].dst); }
    if (dd) ZSTD_freeDDict(dd);
    free(js); free(th);
    return (int)bad;
}
"""


def helper():
    """the C helper as a ctypes library, or None where it cannot be built"""
    import tempfile
    tmp = tempfile.mkdtemp(prefix="zstd_host_")
    src, out = os.path.join(tmp, "host_decode.c"), os.path.join(tmp, "libhost_decode.so")
    with open(src, "w") as fh:
        fh.write(HELPER)
    try:
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-pthread", "-o", out, src, "-l:libzstd.so.1"])
        return C.CDLL(out)
    except (OSError, subprocess.CalledProcessError):
        return None


def host_leg(leg, z, texts, files, d):
    h = helper() if z is not None else None
    if h is None:
        return None
    threads = 1 if leg == "one_frame" else THREADS
    n = len(files)
    in_len = np.array([len(f) for f in files], np.uint64)
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
    inb = np.frombuffer(b"".join(files) + b"\0" * 16, np.uint8)
    raw = np.array([len(t) for t in texts], np.uint64)
    dd = np.frombuffer(d, np.uint8) if d else np.zeros(1, np.uint8)
    ms = np.zeros(WARM + REPS, np.float64)
    bad = h.host_decode(C.c_void_p(p(inb)), C.c_void_p(p(in_off)), C.c_void_p(p(in_len)), C.c_void_p(p(raw)), n, C.c_void_p(p(dd)),
                        C.c_uint64(len(d) if d else 0), C.c_size_t(int(raw.max())), threads, WARM + REPS, C.c_void_p(p(ms)))
    assert bad == 0, bad
    rec = dict({"bench": "libzstd", "workload": leg, "threads": threads, "files": n, "harness": "C helper, pthreads, DCtx and DDict reused"},
               **stats(list(ms[WARM:]), sum(map(len, texts))))
    emit(rec)
    return rec["ms_median"]


def device_leg(leg, texts, files, d, where, made):
    import torch
    import rust_compress_amd as R
    from rust_compress_amd import _native as N
    ctx = R.Context(0)
    lib = N.lib()
    n = len(files)
    head = d or b""
    in_len = np.array([len(f) for f in files], np.uint64)
    in_off = (np.concatenate([[0], np.cumsum(in_len)[:-1]]) + len(head)).astype(np.uint64)
    inb = np.frombuffer(head + b"".join(files) + b"\0" * 16, np.uint8)
    d_off, d_len = (np.zeros(n, np.uint64), np.full(n, len(head), np.uint64)) if d else (None, None)
    out_cap = np.array([len(t) for t in texts], np.uint64)
    out_off = np.concatenate([[0], np.cumsum(out_cap)[:-1]]).astype(np.uint64)
    total = int(out_cap.sum())
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    if where == "device":
        t_in, t_out = torch.from_numpy(inb.copy()).cuda(), torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        base_in, base_out, mem = t_in.data_ptr(), t_out.data_ptr(), N.MEM_DEVICE
    else:
        h_out = np.zeros(total + 16, np.uint8)
        base_in, base_out, mem = p(inb), p(h_out), N.MEM_HOST
    zero = np.zeros(n, np.uint64)

    def timed(caps, variant, check):
        assert lib.rcx_ctx_set_variant(ctx._h, RCX_ZSTD_DECODE, variant) == 0
        b = N.Batch(base_in, p(in_off), p(in_len), base_out, p(out_off), p(caps), p(out_len), p(in_used), p(status), n, mem)
        ms = []
        for r in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.rcx_zstd_decode_batch(ctx._h, C.byref(b), C.c_void_p(p(d_off) if d else None), C.c_void_p(p(d_len) if d else None))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.rcx_last_error(ctx._h))
            check()
            if r >= WARM:
                ms.append(dt)
        assert lib.rcx_ctx_set_variant(ctx._h, RCX_ZSTD_DECODE, 0) == 0
        return ms

    def full():
        assert not status.any() and (out_len == out_cap).all() and (in_used == in_len).all(), status[:8]
    ms = timed(out_cap, 0, full)
    o = t_out.cpu().numpy() if where == "device" else h_out
    assert np.array_equal(o[:total], np.frombuffer(b"".join(texts), np.uint8)), "decoded bytes differ from the text"
    rec = dict({"bench": "rcx_zstd_decode_batch", "workload": leg, "memory": where, "inputs": made, "files": n, "compressed_bytes": int(in_len.sum()),
                "decoded_bytes": total}, **stats(ms, total))
    if N.AB and where == "device":                            # the stages' shares: the literal stage alone, everything but the copies, everything

        def query():
            assert (status == 2).all() and (out_len == out_cap).all()
        q = sorted(timed(zero, 0, query))[REPS // 2]
        lit = sorted(timed(zero, 1, lambda: None))[REPS // 2]
        t = rec["ms_median"]
        rec.update({"ms_size_query": round(q, 3), "ms_literals_only": round(lit, 3), "share_literals": round(lit / t, 3),
                    "share_sequences_and_tables": round((q - lit) / t, 3), "share_execution": round((t - q) / t, 3)})
        a, b = [], []
        for r in range(REPS):                                 # the lever: the executor that takes a sequence at a time and the shipped, flattened one, alternating
            a += timed(out_cap, 2, full)[-1:]
            b += timed(out_cap, 0, full)[-1:]
        o2 = t_out.cpu().numpy()
        assert np.array_equal(o2[:total], np.frombuffer(b"".join(texts), np.uint8)), "the bytes differ from the text"
        rec.update({"lever_plain_ms": [round(x, 3) for x in a], "lever_flat_ms": [round(x, 3) for x in b],
                    "lever_plain_median": round(sorted(a)[len(a) // 2], 3), "lever_flat_median": round(sorted(b)[len(b) // 2], 3)})
    emit(rec)
    ctx.close()
    return rec["ms_median"]


def child(leg, step):
    z = libzstd()
    t0 = time.perf_counter()
    texts, files, d, made = workload(leg, z)
    emit({"bench": "workload", "workload": leg, "step": step, "inputs": made, "files": len(files), "seconds_to_make": round(time.perf_counter() - t0, 1)})
    if step == "libzstd":
        ms = host_leg(leg, z, texts, files, d)
    else:
        ms = device_leg(leg, texts, files, d, step, made)
    emit({"bench": "step", "workload": leg, "step": step, "inputs": made, "ms_median": ms})


if __name__ == "__main__":
    if "--leg" in sys.argv:
        child(sys.argv[sys.argv.index("--leg") + 1], sys.argv[sys.argv.index("--step") + 1])
        sys.exit(0)
    emit({"bench": "zstd_decode_rate", "reps": REPS, "warm": WARM, "threads": THREADS, "legs": LEGS})
    for leg in LEGS:                                          # a child a step, each under its own time limit; the first failure ends the run
        got = {}
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(LIMIT[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--step", step] + (["--out", OUT] if OUT else [])
            run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(run.stdout)
            sys.stdout.flush()
            if run.returncode != 0:
                emit({"bench": "zstd_decode_rate", "failed": leg, "step": step, "exit": run.returncode})
                sys.exit(run.returncode)
            last = json.loads(run.stdout.strip().splitlines()[-1])
            got[step], made = last["ms_median"], last["inputs"]
        host = got["libzstd"]
        emit({"bench": "zstd_vs_host", "workload": leg, "inputs": made, "rcx_device_ms": got["device"], "rcx_host_memory_ms": got["host"],
              "libzstd_ms": host, "libzstd_threads": None if host is None else (1 if leg == "one_frame" else THREADS),
              "rcx_faster": None if host is None else bool(got["device"] < host)})
