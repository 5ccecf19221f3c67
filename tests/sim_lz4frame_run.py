"""Builds and drives tests/sim_lz4frame/sim_lz4frame.cpp: the XXH32 kernel and the linked LZ4 block decoder on the wave64 simulator
(TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_lz4frame", "build", "libsim_lz4frame.so")
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_lz4frame", "sim_lz4frame.cpp"),
                     ("k_xxh32.hip", "k_lz4_linked.hip", "k_lz4_decode_v4.hip", "rcx_dev.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def xxh32(blobs, seed=0, lead=0):
    """XXH32 of every blob; `lead` bytes of padding precede each one in the input buffer (odd alignments).  -> (hashes, in_used, status)"""
    n = len(blobs)
    buf = bytearray()
    in_off = np.zeros(max(n, 1), np.uint64)
    for i, r in enumerate(blobs):
        buf += b"\xC3" * lead
        in_off[i] = len(buf)
        buf += r
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy()
    in_len = np.array([len(r) for r in blobs] or [0], np.uint64)
    h = np.zeros(max(n, 1), np.uint32)
    used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    lib().sim_xxh32(_p(inb), _p(in_off), _p(in_len), n, C.c_uint32(seed), _p(h), _p(used), _p(st))
    return h[:n], used[:n], st[:n]


def plan(link):
    """The chains of a batch as rcx_lz4_decode_linked_batch lays them out: (order, rounds_off, head)."""
    n = len(link)
    head = np.zeros(n, np.uint32)
    depth = np.zeros(n, np.uint32)
    for i in range(n):
        head[i] = head[i - 1] if link[i] else i
        depth[i] = depth[i - 1] + 1 if link[i] else 0
    order = np.argsort(depth, kind="stable").astype(np.uint32)
    nr = int(depth.max()) + 1
    rounds = np.zeros(nr + 1, np.uint32)
    for d in depth:
        rounds[int(d) + 1] += 1
    return order, np.cumsum(rounds).astype(np.uint32), head


def decode_linked(blocks, link, slots, dicts=None, sentinel=0xEE, pad=64):
    """blocks: compressed blocks; link[i]: 1 = continues block i - 1; slots[i]: the output capacity of chain head i (ignored for linked
    blocks); dicts[i]: the dictionary in front of head i's slot (or None).  Every head's region is laid out as
    [pad sentinels | dictionary | slot | pad sentinels].  -> (status, out_len, in_used, eff, out buffer, out_off, dict_off)"""
    n = len(blocks)
    dicts = dicts or [b""] * n
    in_off = np.zeros(n, np.uint64)
    buf = bytearray()
    for i, r in enumerate(blocks):
        in_off[i] = len(buf)
        buf += r
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy()
    in_len = np.array([len(r) for r in blocks], np.uint64)
    out_off = np.zeros(n, np.uint64)
    out_cap = np.zeros(n, np.uint64)
    dcount = np.zeros(n, np.uint32)
    dict_off = np.zeros(n, np.uint64)
    img = bytearray()
    for i in range(n):
        if link[i]:
            out_off[i] = 0xDEAD0000          # ignored by the library
            out_cap[i] = 7
            continue
        img += bytes([sentinel]) * pad
        dict_off[i] = len(img)
        img += dicts[i] or b""
        dcount[i] = len(dicts[i] or b"")
        out_off[i] = len(img)
        out_cap[i] = slots[i]
        img += bytes([sentinel]) * slots[i]
    img += bytes([sentinel]) * pad
    out = np.frombuffer(bytes(img), np.uint8).copy()
    order, rounds, head = plan(link)
    out_len = np.zeros(n, np.uint64)
    in_used = np.zeros(n, np.uint64)
    st = np.full(n, -1, np.int32)
    eff = np.zeros(n, np.uint64)
    lib().sim_lz4_decode_linked(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(st), n,
                                _p(order), _p(rounds), len(rounds) - 1, _p(head), _p(dcount), _p(eff))
    return st, out_len, in_used, eff, out, out_off, dict_off
