"""CPU suite: the parser wave's segment links (k_lz4_decode_v8.hip, run_parser8 step 2) on the wave64 simulator -- a failed link is
repaired over a pre-decoded hop table of the segment (RCX_HOP_WALK), general-path tokens hand over to next_tok_c.  The hand-built
blocks of tests/lz4_link_cases.py make every link fail; bytes, out_len, in_used and status must be the oracle's, at the shipped head
start (RCX_V8_PRE) and, through A/B builds of the same sources, at 32 and 128."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lz4_link_cases as K

LZ4_DECODE = 0
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "wavesim")
CSRC = os.path.join(HERE, "..", "rust_compress_amd", "csrc")

PRES = (None, 32, 128)                 # None: the library tests/wavesim/build.py makes, the shipped defaults


def _ab_lib(pre):
    """the simulator build of the same sources with another head start (tests/wavesim/build.py's command line + -DRCX_V8_PRE)"""
    out = os.path.join(SIM, "build", "libwavesim_kernels_pre%d.so" % pre)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SIM, "sim_kernels.cpp"), os.path.join(SIM, "wavesim.cpp")]
    deps = srcs + [os.path.join(SIM, "wavesim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fno-gnu-unique", "-x", "c++", "-include", os.path.join(SIM, "wavesim.h"),
                               "-Wall", "-DRCX_V8_WHY_STATS", "-DRCX_V8_PRE=%d" % pre, "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                               "-Wno-attributes", "-o", tmp] + srcs)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module", params=PRES, ids=lambda p: "shipped" if p is None else "pre%d" % p)
def sim(request):
    """simrun.run bound to one build of the kernels; .stats() -> the simulator's counters since the last call"""
    import simrun
    shipped = simrun.lib()
    lib = shipped
    if request.param is not None:
        lib = C.CDLL(_ab_lib(request.param))
        lib.sim_launch.argtypes = shipped.sim_launch.argtypes
    lib.sim_stats.restype = C.POINTER(C.c_ulonglong)

    class Sim:
        def run(self, blobs, caps, **kw):
            simrun._lib = lib
            try:
                return simrun.run(LZ4_DECODE, 0, blobs, caps, **kw)
            finally:
                simrun._lib = shipped

        def stats(self):
            p = lib.sim_stats()
            v = [int(p[i]) for i in range(32)]
            for i in range(32):
                p[i] = 0
            return v
    return Sim()


@pytest.fixture(scope="module")
def expect(oracle):
    """oracle results, computed once per block and shared"""
    memo = {}

    def ex(blob, cap):
        key = (blob, cap)
        if key not in memo:
            memo[key] = oracle.lz4_decode_block(blob, cap=cap, raise_on_error=False)
        return memo[key]
    return ex


def _valid(expect, blobs):
    """every hand-built block is a valid stream for the oracle; -> its decoded bytes"""
    raws = []
    for i, b in enumerate(blobs):
        out, st = expect(b, 65536)
        assert st == 0, (i, st, len(b))
        assert len(out) <= 65536
        raws.append(out)
    return raws


def _check_ok(sim, blobs, raws, mis):
    outs, out_len, in_used, st, _ = sim.run(blobs, [len(r) for r in raws], in_misalign=mis)
    assert not st.any(), np.nonzero(st)[0]
    assert outs == raws
    assert list(out_len) == [len(r) for r in raws]
    assert list(in_used) == [len(b) for b in blobs]


def _check_status(sim, expect, blobs, caps, mis=0):
    outs, out_len, in_used, st, _ = sim.run(blobs, caps, in_misalign=mis)
    for i, (b, c) in enumerate(zip(blobs, caps)):
        eo, es = expect(b, c)
        assert es == st[i], (i, es, st[i])
        if es == 0:
            assert eo == outs[i] and out_len[i] == len(eo) and in_used[i] == len(b), i


def test_phase_locked_every_link_fails(sim, expect):
    """periods 3, 4, 5 and 7, every true phase, input misalignments 0-15 (the chunk grid follows the misalignment, the segment grid with
    it).  The links DO fail: the simulator counts the repairs, their hops and the tokens left to next_tok_c."""
    blobs = K.phase_blocks()
    raws = _valid(expect, blobs)
    sim.stats()
    decoded = 0
    for mis in range(16):
        sel = [i for i in range(len(blobs)) if mis < 4 or (i + mis) % 4 == 0]      # every block at misalignments 0-3, a quarter of them at each other
        _check_ok(sim, [blobs[i] for i in sel], [raws[i] for i in sel], mis)
        decoded += len(sel)
    s = sim.stats()
    fails, hops, general = s[7] & 0xffffffff, s[7] >> 32, s[19]
    print("repaired links %d, hops %d, general tokens %d" % (fails, hops, general))
    assert fails > 2000 and hops > 8 * fails
    # the only general-path tokens behind the opening run lie in a block's last 20 bytes: seven of three bytes or more at the most, and the tail
    assert general <= 8 * decoded


def test_general_tokens_in_repaired_segments(sim, expect):
    """literal runs of 15 / 16 / 270 / 600 bytes and match extensions of one byte and of several 0xff, started in, spanning and jumping over failed
    segments and a chunk edge (tests/lz4_link_cases.py: placements); two misalignments, so that a placement whose phase agrees with the
    guesses at one disagrees at the other"""
    blobs = K.general_blocks()
    raws = _valid(expect, blobs)
    sim.stats()
    for mis in (0, 1):
        _check_ok(sim, blobs, raws, mis)
    s = sim.stats()
    assert (s[7] & 0xffffffff) > 1000 and s[19] > 100, s


def test_edges(sim, expect):
    """compressed lengths 1, 19-21, 63-65, 4095-4097, 4096 + 63..65, 8191-8193; ragged last segments of every length with the links failing up to
    segment nseg - 1 and from segment k0 + 1 on; chunks that are one giant token"""
    blobs = K.edge_blocks() + K.giant_blocks()
    lens = {len(b) for b in blobs}
    for n in (1, 19, 20, 21, 63, 64, 65) + K.EDGE_LENGTHS:
        assert n in lens
    raws = _valid(expect, blobs)
    for mis in (0, 5, 15):
        _check_ok(sim, blobs, raws, mis)
    # too little room: the oracle's statuses
    rng = np.random.default_rng(4)
    caps = [int(rng.integers(0, len(r) + 1)) for r in raws]
    _check_status(sim, expect, blobs, caps)


@pytest.mark.parametrize("kind", ["truncated", "mutated"])
def test_malformed_status_for_status(sim, expect, kind):
    base = K.phase_blocks()[:2] + K.general_blocks()[::9] + K.edge_blocks()[7::5] + K.giant_blocks()[3:5]
    _valid(expect, base)
    cut, mut = K.malformed(base, 200, 17)
    blobs = cut if kind == "truncated" else mut
    assert len(blobs) == 200
    _check_status(sim, expect, blobs, [65536] * len(blobs), mis=3)
