"""Builds and drives tests/sim_bzip2_enc/sim_bzip2_enc.cpp: the bzip2 encoder's kernels and launch loop, the host's plan and the suffix
sorter they call, on the wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from sim_bzip2_run import layout, untouched_outside            # noqa: F401  (the batch both the simulator and the GPU tests run)

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_bzip2_enc", "build", "libsim_bzip2_enc.so")
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_bzip2_enc", "sim_bzip2_enc.cpp"),
                     ("k_bzip2_enc.hip", "k_bwt.hip", "k_bwt_sort.hip", "k_crc32.hip", "rcx_dev.h", "rcx_plan.h"), ("-Wno-unused-but-set-variable",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def run(datas, caps, level=9, chunk=None, round=0, stages=True):
    """One call over the files `datas` with slot capacities `caps` (chunk: input bytes a block, None = the level's; round: blocks a
    round, 0 = the library's choice) -> dict(rc, err, data, out_len, in_used, status, out, out_off, out_cap, launches, rounds, scratch,
    blocks): blocks a list of dicts with every stage of a block (file, off, len, t, l, orig, crc, symbols, tables, selectors, used, bits)."""
    n = len(datas)
    inb, in_off, in_len, out, out_off, out_cap = layout(datas, caps)
    out_len = np.full(n, 0x7777, np.uint64)
    in_used = np.full(n, 0x7777, np.uint64)
    st = np.full(n, -1, np.int32)
    info = np.zeros(4, np.uint64)
    err = C.create_string_buffer(512)
    chunk = 100000 * level - 19 if chunk is None else chunk
    rc = lib().sim_bzip2_encode(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(st), n,
                                C.c_int(level), C.c_uint32(chunk), C.c_uint32(round), _p(info), err, 512)
    blocks = []
    nblk = int(info[2])
    if rc == 0 and stages and nblk:
        sizes = np.zeros(12 * nblk, np.uint64)
        lib().sim_bzip2_enc_sizes(_p(sizes))
        for i in range(nblk):
            f, off, ln, bn, nmtf, nsel, ng, alpha, orig, crc, bits, head = (int(x) for x in sizes[12 * i:12 * i + 12])
            tt = np.zeros(2 * bn, np.uint8)
            l = np.zeros(bn, np.uint8)
            syms = np.zeros(nmtf, np.uint16)
            lens = np.zeros(6 * 258, np.uint8)
            sel = np.zeros(nsel, np.uint8)
            used = np.zeros(8, np.uint32)
            lib().sim_bzip2_enc_block(i, _p(tt), _p(l), _p(syms), _p(lens), _p(sel), _p(used))
            blocks.append(dict(file=f, off=off, len=ln, t=tt[:bn].tobytes(), tt=tt.tobytes(), l=l.tobytes(), orig=orig, crc=crc,
                               symbols=[int(x) for x in syms], tables=[[int(x) for x in lens[258 * t:258 * t + alpha]] for t in range(ng)],
                               selectors=[int(x) for x in sel], used=[b for b in range(256) if used[b >> 5] >> (b & 31) & 1], bits=bits,
                               head_bits=head))
    data = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) if st[i] == 0 else None for i in range(n)]
    return dict(rc=rc, err=err.value.decode(), data=data, out_len=out_len, in_used=in_used, status=st, out=out, out_off=out_off,
                out_cap=out_cap, launches=int(info[0]), rounds=int(info[1]), scratch=int(info[3]), blocks=blocks)
