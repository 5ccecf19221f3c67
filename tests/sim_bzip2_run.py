"""Builds and drives tests/sim_bzip2/sim_bzip2.cpp: the bzip2 decoder's kernels and launch loop, the host's chain plan and the inverse BWT
they call, on the wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_bzip2", "build", "libsim_bzip2.so")
KINDS = {0: "block", 1: "end", 2: "head"}
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_bzip2", "sim_bzip2.cpp"),
                     ("k_bzip2.hip", "k_bwt_inverse.hip", "k_crc32.hip", "rcx_dev.h", "rcx_plan.h"), ("-Wno-unused-but-set-variable",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def layout(blobs, caps):
    """The batch both the simulator and the GPU tests decode: the files three bytes apart behind one byte of 0x5A, the slots five bytes
    apart in a buffer of 0xEE.  -> (inb, in_off, in_len, out, out_off, out_cap)"""
    n = len(blobs)
    in_len = np.array([len(b) for b in blobs], np.uint64)
    in_off = (np.concatenate([[0], np.cumsum(in_len + np.uint64(3))[:-1]]) + 1).astype(np.uint64)
    inb = np.full(int(in_off[-1] + in_len[-1]) + 16, 0x5A, np.uint8)
    for o, b in zip(in_off, blobs):
        inb[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    out_cap = np.array(caps, np.uint64)
    out_off = (np.concatenate([[0], np.cumsum(out_cap + np.uint64(5))[:-1]]) + 5).astype(np.uint64)
    out = np.full(int(out_off[-1] + out_cap[-1]) + 16, 0xEE, np.uint8)
    assert n == len(caps)
    return inb, in_off, in_len, out, out_off, out_cap


def run(blobs, caps, round=0):
    """One call over the files `blobs` with slot capacities `caps` (round: block candidates a round, 0 = the library's choice) -> dict(rc, err, data, out_len, in_used, status, out, out_off,
    out_cap, launches, rounds, scratch, cands, live): cands a list of (file, bit, kind, extra), live a list of (file, bit) in stream order."""
    n = len(blobs)
    inb, in_off, in_len, out, out_off, out_cap = layout(blobs, caps)
    out_len = np.full(n, 0x7777, np.uint64)
    in_used = np.full(n, 0x7777, np.uint64)
    st = np.full(n, -1, np.int32)
    info = np.zeros(5, np.uint64)
    err = C.create_string_buffer(512)
    rc = lib().sim_bzip2_decode(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(st), n, round,
                                _p(info), err, 512)
    cands = np.zeros(4 * int(info[2]) + 4, np.uint64)
    live = np.zeros(2 * int(info[3]) + 2, np.uint64)
    lib().sim_bzip2_trace(_p(cands), _p(live))
    data = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) if st[i] == 0 else None for i in range(n)]
    return dict(rc=rc, err=err.value.decode(), data=data, out_len=out_len, in_used=in_used, status=st, out=out, out_off=out_off,
                out_cap=out_cap, launches=int(info[0]), rounds=int(info[1]), scratch=int(info[4]),
                cands=[(int(cands[4 * i]), int(cands[4 * i + 1]), KINDS[int(cands[4 * i + 2])], int(cands[4 * i + 3])) for i in range(int(info[2]))],
                live=[(int(live[2 * i]), int(live[2 * i + 1])) for i in range(int(info[3]))])


def untouched_outside(out, out_off, out_cap):
    """every byte outside the slots is the sentinel"""
    mask = np.ones(out.size, bool)
    for o, c in zip(out_off, out_cap):
        mask[int(o):int(o) + int(c)] = False
    return bool((out[mask] == 0xEE).all())
