"""Builds and drives tests/sim_deflate/sim_deflate.cpp: the DEFLATE encoder kernels on the wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_deflate", "build", "libsim_deflate.so")
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_deflate", "sim_deflate.cpp"), ("k_deflate_encode.hip", "lz_match.h", "rcx_dev.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def encode(raws, fmt, caps=None):
    """fmt 0 raw DEFLATE / 1 zlib / 2 gzip -> (outputs, status, out_len, in_used); caps default to the bound (+ framing)."""
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
    rc = lib().sim_deflate_encode(fmt, P(inb), P(in_off), P(in_len), P(out), P(out_off), P(out_cap), P(out_len), P(in_used), P(st), n)
    assert rc == 0
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    return outs, st[:n], out_len[:n], in_used[:n]
