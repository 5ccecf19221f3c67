"""Builds and drives tests/sim_lz4hc/sim_lz4hc.cpp: the LZ4 high-compression encoder kernels on the wave64 simulator (TEST
INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_lz4hc", "build", "libsim_lz4hc.so")
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_lz4hc", "sim_lz4hc.cpp"), ("k_lz4_hc.hip", "lz_match.h", "rcx_dev.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def bound(n):
    return n + n // 255 + 20


def encode(raws, level, caps=None, scratch_bytes=0, fill=0xEE):
    """-> (rc, outputs, status, out_len, in_used, out buffer, out_off); caps default to the LZ4 compression bound."""
    n = len(raws)
    in_off = np.zeros(max(n, 1), np.uint64)
    in_len = np.array([len(r) for r in raws] or [0], np.uint64)
    o = 0
    for i, r in enumerate(raws):
        in_off[i] = o
        o += len(r)
    inb = np.frombuffer(b"".join(raws) + b"\0" * 16, np.uint8).copy()
    if caps is None:
        caps = [bound(len(r)) for r in raws]
    out_cap = np.array(caps or [0], np.uint64)
    out_off = np.zeros(max(n, 1), np.uint64)
    o = 0
    for i, c in enumerate(caps):
        out_off[i] = o
        o += c
    out = np.full(o + 16, fill, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_lz4hc_encode(level, P(inb), P(in_off), P(in_len), P(out), P(out_off), P(out_cap), P(out_len), P(in_used), P(st), n,
                                C.c_uint64(scratch_bytes))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    return rc, outs, st[:n], out_len[:n], in_used[:n], out, out_off[:n]


LAYOUT = ("link", "cand", "elen", "seg_first", "seg_nm", "seg_fm", "seg_le", "cap")
LAUNCHES = ("plan", "links", "search", "parse", "scan", "place")     # kernel launches of an encode, in order (stop_after counts them)
ALL = 0xFFFFFFFF


def layout(base, nbytes, n):
    """{array: byte offset} (and "cap": segments) of an HC scratch of nbytes bytes at the address `base` for n blocks, from the
    kernels' own hc_carve."""
    lay = np.zeros(len(LAYOUT), np.uint64)
    lib().sim_lz4hc_layout(C.c_uint64(base), C.c_uint64(nbytes), C.c_uint32(n), C.c_void_p(lay.ctypes.data))
    return {k: int(v) for k, v in zip(LAYOUT, lay)}


def scratch_bytes_for(n, segs):
    f = lib().sim_lz4hc_scratch_bytes
    f.restype = C.c_uint64
    return int(f(C.c_uint32(n), C.c_uint64(segs)))


def stages(raws, level, stop_after=ALL, lead=0, fill=0xA5):
    """An encode at `level` of which the first stop_after kernel launches run (LAUNCHES; ALL: the whole encode), in a scratch filled
    with `fill`.  `lead` bytes of padding precede every block in the input buffer.  -> (rc, outputs, status, scratch, layout): the
    scratch as a uint8 array and layout(...) of it; tests/hc_stages.py cuts it into per-block views."""
    n = len(raws)
    in_off = np.zeros(max(n, 1), np.uint64)
    in_len = np.array([len(r) for r in raws] or [0], np.uint64)
    buf = bytearray()
    for i, r in enumerate(raws):
        buf += b"\xC3" * lead
        in_off[i] = len(buf)
        buf += r
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy()
    out_cap = np.array([bound(len(r)) for r in raws] or [0], np.uint64)
    out_off = np.concatenate([[0], np.cumsum(out_cap)[:-1]]).astype(np.uint64)
    out = np.full(int(out_cap.sum()) + 16, 0xEE, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    sb = scratch_bytes_for(n, sum((len(r) + 65535) // 65536 for r in raws))
    scratch = np.full(sb + 64, fill, np.uint8)
    lay = np.zeros(len(LAYOUT), np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_lz4hc_stages(level, P(inb), P(in_off), P(in_len), P(out), P(out_off), P(out_cap), P(out_len), P(in_used), P(st), n,
                                C.c_uint32(stop_after), P(scratch), C.c_uint64(sb), P(lay))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    return rc, outs, st[:n], scratch, {k: int(v) for k, v in zip(LAYOUT, lay)}


def _job(args):
    """a job is encode's arguments, or ("stages", reduce, ...): reduce(raws, stages(...)) -- what the worker sends back (a function
    of a module the workers can import), so that whole scratches do not travel between processes"""
    if args and isinstance(args[0], str) and args[0] == "stages":
        return args[1](args[2], stages(*args[2:]))
    return encode(*args)


def encode_many(jobs, workers=None):
    """encode(*job) or the stages job for every job, in forked worker processes (the simulator runs one launch at a time per process):
    a list of the results in the jobs' order."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    build()
    workers = workers or max(1, min(len(jobs), os.cpu_count() or 1))
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        return list(ex.map(_job, jobs))
