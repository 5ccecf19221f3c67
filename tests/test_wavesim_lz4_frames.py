"""CPU suite: emit6's frame stores (k_lz4_emit6.hip: store_frame, the mask table's row stride RCX_X6_MROW, four atomics where no
lane reaches a frame's fifth dword RCX_X6_NW4) on the wave64 simulator.  The hand-built blocks of tests/lz4_frame_cases.py -- every
misalignment x length per kind of store, the batches the four-or-five choice turns on, neighbours that share a boundary dword,
emit5's frame stores -- must decode to the oracle's bytes, out_len, in_used and status: with the library tests/wavesim/build.py makes
(the shipped switches) and, through A/B builds of the same sources, at each row stride (8, 9, 12) and with the choice on and off.

The simulator stores a frame byte by byte and never reads the mask table: what it checks is the lengths, misalignments and frame
pointers every store is handed, that the table fits its allocation at each stride, and -- its store drops, as the GPU's would,
whatever lies beyond the dwords a store was told to write -- that no store is told `four` when a lane needs five.  The GPU's
hand-written paths are checked by tests/test_gpu_lz4_frames.py alone.

The A/B builds count (RCX_X6_FRAME_STATS) emit6's frame stores and those in which no lane reaches the fifth dword; the last test
reports the share on the benchmark's text blocks."""
import ctypes as C
import os
import subprocess

import pytest

import lz4_frame_cases as K
from rust_compress_amd import synth

LZ4_DECODE = 0
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "wavesim")
CSRC = os.path.join(HERE, "..", "rust_compress_amd", "csrc")
MIS = ((0, 0), (1, 1), (2, 7), (13, 3), (3, 14))            # input / output buffer misalignments: every output residue mod 4

BUILDS = (None, (12, 3), (9, 0), (8, 3), (12, 0))           # None: the shipped switches; (RCX_X6_MROW, RCX_X6_NW4)
FOUR_SHARE_TEXT = 0.437                                     # measured below on two text blocks: frame stores with no lane at the fifth dword


def _ab_lib(mrow, nw4):
    """the simulator build of the same sources at another row stride / choice, with the frame-store counters (tests/wavesim/build.py's
    command line + the switches)"""
    out = os.path.join(SIM, "build", "libwavesim_kernels_m%dn%d.so" % (mrow, nw4))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SIM, "sim_kernels.cpp"), os.path.join(SIM, "wavesim.cpp")]
    deps = srcs + [os.path.join(SIM, "wavesim.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fno-gnu-unique", "-x", "c++", "-include", os.path.join(SIM, "wavesim.h"),
                               "-Wall", "-DRCX_V8_WHY_STATS", "-DRCX_X6_FRAME_STATS", "-DRCX_X6_MROW=%d" % mrow, "-DRCX_X6_NW4=%d" % nw4,
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-attributes", "-o", tmp] + srcs)
        os.replace(tmp, out)
    return out


class Sim:
    """simrun.run bound to one build of the kernels; .stats() -> the simulator's 32 counters, .frames() -> (frame stores, those of them
    with no lane at the fifth dword, gathered matches), all since the last call"""

    def __init__(self, build):
        import simrun
        self.simrun = simrun
        self.shipped = simrun.lib()
        self.lib = self.shipped
        if build is not None:
            self.lib = C.CDLL(_ab_lib(*build))
            self.lib.sim_launch.argtypes = self.shipped.sim_launch.argtypes
            self.lib.rcx_x6_frame_stats.restype = C.POINTER(C.c_ulonglong)
        self.lib.sim_stats.restype = C.POINTER(C.c_ulonglong)
        self.counts = build is not None

    def run(self, blobs, caps, **kw):
        self.simrun._lib = self.lib
        try:
            return self.simrun.run(LZ4_DECODE, 0, blobs, caps, **kw)
        finally:
            self.simrun._lib = self.shipped

    def stats(self):
        p = self.lib.sim_stats()
        v = [int(p[i]) for i in range(32)]
        for i in range(32):
            p[i] = 0
        return v

    def frames(self):
        p = self.lib.rcx_x6_frame_stats()
        v = (int(p[0]), int(p[1]), int(p[2]))
        p[0] = p[1] = p[2] = 0
        return v


@pytest.fixture(scope="module", params=BUILDS, ids=lambda b: "shipped" if b is None else "mrow%d_nw4_%d" % b)
def sim(request):
    return Sim(request.param)


@pytest.fixture(scope="module")
def built(oracle):
    """the blocks and the oracle's bytes, once"""
    memo = {}

    def get(case):
        if case not in memo:
            blob, b, want = case()
            raw = oracle.lz4_decode_block(blob, cap=b.pos + 24)
            assert len(raw) == b.pos + 24
            memo[case] = (blob, b, want, raw)
        return memo[case]
    return get


@pytest.mark.parametrize("case", K.CASES, ids=lambda f: f.__name__[4:])
def test_frame_cases_decode_as_the_oracle(sim, built, case):
    blob, b, want, raw = built(case)
    for mis in MIS:
        sim.stats()
        outs, out_len, in_used, status, _ = sim.run([blob], [len(raw)], in_misalign=mis[0], out_misalign=mis[1])
        assert not status.any(), (mis, status)
        assert outs == [raw], mis
        assert list(out_len) == [len(raw)] and list(in_used) == [len(blob)], mis
        st = sim.stats()
        # every batch but the block's first and last -- and those built to go through emit5 -- went through emit6, none fell back
        n5 = 2 + want.get("emit5", 0)
        assert (st[8], st[9]) == (b.n_batches - n5, n5), (mis, st[8], st[9], b.n_batches)
        # ... and the matches took the store they were built for: early lanes (slot 15), window matches copied in the rounds, runs among
        # them (slot 16), gathered matches (the A/B builds' counter)
        assert st[15] >= want.get("early", 0), (mis, st[15])
        assert st[16] >= want.get("rounds", 0), (mis, st[16])
        if sim.counts:
            assert sim.frames()[2] >= want.get("far", 0), mis


@pytest.mark.parametrize("case", K.FIFTH_CASES, ids=lambda f: f.__name__[4:])
def test_the_fifth_dword_batches_take_the_branch_they_were_built_for(built, case):
    """the blocks built for the four-or-five choice: every store with a lane at the fifth dword is one of the frames built to be the
    only such lane of its batch -- those of them that the buffer's alignment puts at a >= 2 -- and every other store of the block
    goes without; in the block of quiet batches no store at all has one"""
    s = Sim((12, 3))
    blob, b, want, raw = built(case)
    for mis in MIS:
        s.frames()
        outs, _, _, status, _ = s.run([blob], [len(raw)], in_misalign=mis[0], out_misalign=mis[1])
        assert not status.any() and outs == [raw]
        stores, four, _ = s.frames()
        expect = sum(((p + mis[1]) & 3) + 15 > 16 for p in want["fifth"])
        print("%s, output misalignment %d: %d frame stores, %d of them with a fifth dword (built: %d)" % (case.__name__, mis[1], stores, stores - four, expect))
        assert stores > 0 and stores - four == expect, (mis, stores, four, expect)
        assert not want["fifth"] or 0 < expect < len(want["fifth"])


def test_text_blocks_share_of_stores_without_a_fifth_dword(oracle):
    """the statistic the choice rests on, reported: on text blocks (the benchmark's distribution) the share of emit6's frame stores in
    which no lane reaches the fifth dword.  The inputs are seeded and the figure is exact; 5 % of slack for a change elsewhere in the
    executor."""
    s = Sim((12, 3))
    raws = [synth.gen("text", 65536, 21 + i).tobytes() for i in range(2)]
    blobs = [oracle.lz4_encode_block(r) for r in raws]
    s.frames(); s.stats()
    outs, _, in_used, status, _ = s.run(blobs, [len(r) for r in raws])
    assert not status.any() and outs == raws and list(in_used) == [len(x) for x in blobs]
    stores, four, _ = s.frames()
    st = s.stats()
    print("text: %d plain batches, %d frame stores (%.2f a batch), %d without a fifth dword (%.4f)" % (st[8], stores, stores / st[8], four, four / stores))
    assert st[8] > 100 and stores > 3 * st[8]
    assert abs(four / stores - FOUR_SHARE_TEXT) < 0.05 * FOUR_SHARE_TEXT, (stores, four, four / stores)
