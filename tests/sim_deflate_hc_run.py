"""Builds and drives tests/sim_deflate_hc/sim_deflate_hc.cpp: the DEFLATE encoder kernels of every level on the wave64 simulator
(TEST INFRASTRUCTURE)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "sim_deflate_hc", "build", "libsim_deflate_hc.so")
_lib = None


def build():
    src = os.path.join(HERE, "sim_deflate_hc", "sim_deflate_hc.cpp")
    ws = os.path.join(HERE, "wavesim")
    csrc = os.path.join(ROOT, "rust_compress_amd", "csrc")
    deps = [src, os.path.join(ws, "wavesim.h"), os.path.join(ws, "wavesim.cpp"), os.path.join(csrc, "k_deflate_encode.hip"),
            os.path.join(csrc, "k_deflate_hc.hip"), os.path.join(csrc, "rcx_dev.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = OUT + ".%d" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-x", "c++", "-include", os.path.join(ws, "wavesim.h"),
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-attributes",
                           "-o", tmp, src, os.path.join(ws, "wavesim.cpp")])
    os.replace(tmp, OUT)
    return OUT


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def encode(raws, fmt, level, caps=None, scratch_bytes=0, full=False):
    """fmt 0 raw DEFLATE / 1 zlib / 2 gzip at level 1..9 -> (rc, outputs, status, out_len, in_used) (full: + the output buffer and
    out_off); caps default to the bound (+ framing); the output buffer starts filled with 0xEE."""
    n = len(raws)
    in_off = np.zeros(max(n, 1), np.uint64)
    in_len = np.array([len(r) for r in raws] or [0], np.uint64)
    o = 0
    for i, r in enumerate(raws):
        in_off[i] = o
        o += len(r)
    inb = np.frombuffer(b"".join(raws) + b"\0" * 16, np.uint8).copy()
    if caps is None:
        from rust_compress_amd import _native as N
        caps = [int(N.lib().rcx_deflate_compression_bound(len(r))) + (0, 6, 18)[fmt] for r in raws]
    out_cap = np.array(caps or [0], np.uint64)
    out_off = np.zeros(max(n, 1), np.uint64)
    o = 0
    for i, c in enumerate(caps):
        out_off[i] = o
        o += c
    out = np.full(o + 16, 0xEE, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_deflate_hc_encode(fmt, level, P(inb), P(in_off), P(in_len), P(out), P(out_off), P(out_cap), P(out_len), P(in_used),
                                     P(st), n, C.c_uint64(scratch_bytes))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    if full:
        return rc, outs, st[:n], out_len[:n], in_used[:n], out, out_off[:n]
    return rc, outs, st[:n], out_len[:n], in_used[:n]


def _job(args):
    return encode(*args)


def encode_many(jobs, workers=None):
    """encode(*job) for every job, in forked worker processes (the simulator runs one launch at a time per process): a list of the
    results in the jobs' order."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    build()
    workers = workers or max(1, min(len(jobs), os.cpu_count() or 1))
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        return list(ex.map(_job, jobs))
