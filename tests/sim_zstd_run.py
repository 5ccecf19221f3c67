"""Builds and drives tests/sim_zstd/sim_zstd.cpp: the Zstandard decoder's kernel and the host's rcx_plan_zstd on the wave64 simulator
(TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_zstd", "build", "libsim_zstd.so")
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_zstd", "sim_zstd.cpp"),
                     ("k_zstd.hip", "k_xxh64.hip", "rcx_dev.h", "rcx_plan.h"), ("-Wno-unused-but-set-variable",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def layout(blobs, caps, dicts=None):
    """The batch both the simulator and the GPU tests decode: every distinct dictionary once at the front, then the files three bytes
    apart behind one byte of 0x5A; the slots five bytes apart in a buffer of 0xEE.  dicts: None, or one entry (bytes or None) per file.
    -> (inb, in_off, in_len, d_off, d_len, out, out_off, out_cap); d_off / d_len None without dicts"""
    n = len(blobs)
    assert n == len(caps) and n
    front, at = bytearray(b"\x5a"), {}
    d_off = d_len = None
    if dicts is not None:
        d_off, d_len = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for i, d in enumerate(dicts):
            if d:
                if d not in at:
                    at[d] = len(front)
                    front += d + b"\x5a"
                d_off[i], d_len[i] = at[d], len(d)
    in_len = np.array([len(b) for b in blobs], np.uint64)
    in_off = (np.concatenate([[0], np.cumsum(in_len + np.uint64(3))[:-1]]) + len(front)).astype(np.uint64)
    inb = np.full(int(in_off[-1] + in_len[-1]) + 16, 0x5A, np.uint8)
    inb[:len(front)] = np.frombuffer(bytes(front), np.uint8)
    for o, b in zip(in_off, blobs):
        inb[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    out_cap = np.array(caps, np.uint64)
    out_off = (np.concatenate([[0], np.cumsum(out_cap + np.uint64(5))[:-1]]) + 5).astype(np.uint64)
    out = np.full(int(out_off[-1] + out_cap[-1]) + 16, 0xEE, np.uint8)
    return inb, in_off, in_len, d_off, d_len, out, out_off, out_cap


def run(blobs, caps, dicts=None, waves=0, variant=0):
    """One call over the files `blobs` with slot capacities `caps` -> dict(rc, err, data, out_len, in_used, status, out, out_off, out_cap,
    waves, scratch, span); data[i] is None for a file whose status is not RCX_OK."""
    n = len(blobs)
    inb, in_off, in_len, d_off, d_len, out, out_off, out_cap = layout(blobs, caps, dicts)
    out_len = np.full(n, 0x7777, np.uint64)
    in_used = np.full(n, 0x7777, np.uint64)
    st = np.full(n, -1, np.int32)
    info = np.zeros(3, np.uint64)
    err = C.create_string_buffer(512)
    lib().sim_zstd_variant(variant)                      # 0: the shipped form; 2: the executor that takes a sequence at a time (an A/B variant)
    rc = lib().sim_zstd_decode(_p(inb), _p(in_off), _p(in_len), _p(d_off), _p(d_len), _p(out), _p(out_off), _p(out_cap), _p(out_len),
                               _p(in_used), _p(st), n, waves, _p(info), err, 512)
    data = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) if st[i] == 0 else None for i in range(n)]
    return dict(rc=rc, err=err.value.decode(), data=data, out_len=out_len, in_used=in_used, status=st, out=out, out_off=out_off,
                out_cap=out_cap, waves=int(info[0]), scratch=int(info[1]), span=int(info[2]))


def xxh64(blobs, seed=0):
    n = len(blobs)
    in_len = np.array([len(b) for b in blobs], np.uint64)
    in_off = (np.concatenate([[0], np.cumsum(in_len + np.uint64(3))[:-1]]) + 1).astype(np.uint64)
    inb = np.zeros(int(in_off[-1] + in_len[-1]) + 16, np.uint8)
    for o, b in zip(in_off, blobs):
        inb[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    h = np.zeros(n, np.uint64)
    lib().sim_xxh64(_p(inb), _p(in_off), _p(in_len), n, C.c_uint64(seed), _p(h))
    return [int(x) for x in h]


def untouched_outside(out, out_off, out_cap):
    """every byte outside the slots is the sentinel"""
    mask = np.ones(out.size, bool)
    for o, c in zip(out_off, out_cap):
        mask[int(o):int(o) + int(c)] = False
    return bool((out[mask] == 0xEE).all())
