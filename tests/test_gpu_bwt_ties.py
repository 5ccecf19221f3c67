"""GPU: the suffix sorter (k_bwt.hip + k_bwt_sort.hip) where its groups tie deep and come in every size class -- the tie-group case
table (tests/bwt_tie_cases.py; tests/test_sa_check.py proves what it covers), 256 KiB blocks with LCPs near their length, the
2^24-byte switch of the key width with planted ties, and the bzip2 encoder, which sorts every block doubled.

No oracle here (its qsort over memcmp does not finish on these inputs): the exported suffix array must pass the certificate of
tests/sa_check.py, (L, origin) must be the transform that follows from the certified array, and the inverse transform must return
the input."""
import bz2
import ctypes as C
import time

import numpy as np
import pytest

import bwt_tie_cases as TC
import sa_check as S
from rust_compress_amd import _native as N
from rust_compress_amd import batch as B

pytestmark = pytest.mark.gpu


def _call(ctx, fn_name, blocks, caps, mem):
    """One raw batch call with the blocks and the slots in host or in device memory (the descriptors and the origins are the caller's
    host arrays either way: tests/test_gpu_layout.py, call_raw) -> (outputs, origins)"""
    import torch
    n = len(blocks)
    base, off, lens = B.pack(blocks)
    total, ooff, ocap = B.layout(caps)
    out = np.zeros(total + 64, np.uint8)
    p = lambda a: a.ctypes.data
    if mem == "device":
        ti, to = torch.from_numpy(base).to("cuda:0"), torch.from_numpy(out).to("cuda:0")
        ip, op = ti.data_ptr(), to.data_ptr()
    else:
        ip, op = p(base), p(out)
    out_len, in_used, status, aux = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -9, np.int32), np.zeros(n, np.uint32)
    b = N.Batch(ip, p(off), p(lens), op, p(ooff), p(ocap), p(out_len), p(in_used), p(status), n, N.MEM_DEVICE if mem == "device" else N.MEM_HOST)
    rc = getattr(N.lib(), fn_name)(ctx._h, C.byref(b), C.c_void_p(p(aux)))
    assert rc == 0, (fn_name, mem, rc, N.lib().rcx_last_error(ctx._h))
    if mem == "device":
        torch.cuda.synchronize()
        out = to.cpu().numpy()
    assert not status.any() and out_len.tolist() == list(caps), (fn_name, mem, status.tolist())
    return B.unpack(out, ooff, out_len), aux


def _sort_and_check(ctx, blocks, tag, mem="host", inverse=True):
    """suffixes and transform of one batch: certificate, (L, origin) from the certified array, the inverse transform.  -> seconds the
    three GPU calls took"""
    t0 = time.perf_counter()
    sas, og_sa = _call(ctx, "rcx_bwt_suffixes_batch", blocks, [4 * len(b) for b in blocks], mem)
    Ls, og = _call(ctx, "rcx_bwt_forward_batch", blocks, [len(b) for b in blocks], mem)
    gpu = time.perf_counter() - t0
    for i, (T, sa, L) in enumerate(zip(blocks, sas, Ls)):
        S.assert_block(T, sa, L, og[i], (tag, mem, i))
        assert not T or int(og_sa[i]) == int(og[i]), (tag, mem, i)
    if inverse:
        nz = [i for i, T in enumerate(blocks) if T]
        t0 = time.perf_counter()
        inv = ctx.bwt_inverse([Ls[i] for i in nz], [int(og[i]) for i in nz]).check()
        gpu += time.perf_counter() - t0
        assert inv.outputs == [blocks[i] for i in nz], (tag, mem)
    print("%s (%s): %d bytes, GPU calls %.3f s" % (tag, mem, sum(len(b) for b in blocks), gpu))
    return gpu


CASES = [n for n, _ in TC.case_table()]


@pytest.mark.parametrize("mem", ("host", "device"))
@pytest.mark.parametrize("name", CASES)
def test_case_table(ctx, name, mem):
    _sort_and_check(ctx, list(dict(TC.case_table())[name]), name, mem)


@pytest.mark.parametrize("name", CASES)
def test_case_table_three_blocks_a_pass(ctx, name):
    """BWT_FORWARD variant 3: at most three blocks per sorting pass.  The groups lie at other places in the windows (the pass's array
    starts again every three blocks) and the per-pass state is rebuilt pass after pass; the certificate needs no model of that."""
    try:
        ctx.set_variant(N.BWT_FORWARD, 3); ctx.set_variant(N.BWT_SUFFIXES, 3)
        for mem in ("host", "device"):
            _sort_and_check(ctx, list(dict(TC.case_table())[name]), name + "/3", mem, inverse=False)
    finally:
        ctx.set_variant(N.BWT_FORWARD, 0); ctx.set_variant(N.BWT_SUFFIXES, 0)


BLOCK = 262144
DEEP = {"periodic251": lambda: TC.periodic(251, BLOCK // 251 + 1, 0, 200, 31)[:BLOCK], "fibonacci": lambda: TC.fibonacci(BLOCK),
        "thue_morse": lambda: TC.thue_morse(BLOCK), "zeros": lambda: bytes(BLOCK), "abab": lambda: b"ab" * (BLOCK // 2)}


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_block_of_the_products_size(ctx, name):
    """one 256 KiB block whose groups stay alive until h passes its longest repeat: 14 doubling rounds and more"""
    T = DEEP[name]()
    assert len(T) == BLOCK
    _sort_and_check(ctx, [T], name)


def test_64_copies_of_one_periodic_block(ctx):
    T = TC.periodic(29, 4096 // 29 + 1, 0, 5, 32)[:4096]
    _sort_and_check(ctx, [T] * 64, "64 x periodic 4 KiB")


def _planted_random(n, seed):
    """random bytes over 64 symbols with planted repeats: 40 copies of a 3000-symbol word, 300 of a 600-symbol one, 2100 of a 100-symbol
    one (groups for the one-wave sort, the workgroup sort and the partition that stand from depth 17 to 32 and far beyond), and 9 and
    20 copies of two 200-symbol words (the dense passes' two sorts)."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 64, n, dtype=np.uint8) + 32
    plan = [(40, 3000), (300, 600), (2100, 100), (9, 200), (20, 200)]
    slots = rng.permutation(n // 4096 - 1)[: sum(g for g, _ in plan)] * 4096 + rng.integers(0, 1000, sum(g for g, _ in plan))
    k = 0
    for g, wlen in plan:
        W = rng.integers(0, 64, wlen, dtype=np.uint8) + 32
        for _ in range(g):
            T[slots[k]: slots[k] + wlen] = W
            k += 1
    return T


@pytest.mark.parametrize("n", ((1 << 24) - 1, 1 << 24))
def test_key_width_switch_with_planted_ties(ctx, n):
    """2^24 - 1 bytes: the largest local rank the 32-bit keys pack under a 6-bit group id; 2^24: the first block of the 64-bit keys.
    Each in a call of its own, so that the block's length alone picks the key width.  The planted repeats give the kernels of the rounds
    >= 1 (k_bws_partition, k_bws_local_wave, k_bws_local_wg, k_bws_dense, in the width the block takes) groups of every size class:
    asserted on the certified array at depths 17 and 32."""
    Ta = _planted_random(n, 5 + (n & 1))
    T = Ta.tobytes()
    t0 = time.perf_counter()
    sa = np.frombuffer(ctx.bwt_suffixes([T]).check().outputs[0], dtype="<u4")
    t1 = time.perf_counter()
    fw = ctx.bwt_forward([T]).check()
    t2 = time.perf_counter()
    print("n = %d: bwt_suffixes %.3f s, bwt_forward %.3f s (host-memory calls: the copies included)" % (n, t1 - t0, t2 - t1))
    fault = S.suffix_array_fault(Ta, sa)
    assert fault is None, fault
    eL, eo = S.bwt_from_sa(Ta, sa)
    assert fw.outputs[0] == eL and int(fw.aux[0]) == eo
    t = S.ties(Ta, sa)
    s0, z0 = t.groups(17)
    s1, z1 = t.groups(32)
    enc = np.searchsorted(s0, s1, side="right") - 1
    got = {S.classify(a, z)[0] for a, z, z17 in zip(s1.tolist(), z1.tolist(), z0[enc].tolist()) if S.classify(a, z)[0] == S.classify(a, z17)[0]}
    assert got == set(S.CLASSES), got
    inv = ctx.bwt_inverse([eL], [eo]).check()
    assert inv.outputs[0] == T


BZ_FILES = {"periodic251": lambda: TC.periodic(251, 400, 0, 200, 41)[:100_000], "periodic37": lambda: TC.periodic(37, 2703, 0, 4, 42)[:100_000],
            "periodic3": lambda: TC.periodic(3, 33334, 0, 3, 43)[:100_000], "thue_morse": lambda: TC.thue_morse(100_000)}


@pytest.mark.parametrize("level", (1, 9))
def test_bzip2_encode_of_deep_ties(ctx, level):
    """The bzip2 encoder sorts every block doubled (rotations, not suffixes), so the ties of these files go twice as deep as in the
    transform's own tests.  The serial reference encoder of tests/bz2_enc_ref.py is too slow on such inputs, so the streams are not
    compared byte for byte: Python's bz2 and the GPU decoder must both return the input."""
    files = [BZ_FILES[k]() for k in sorted(BZ_FILES)]
    assert all(len(f) == 100_000 for f in files)
    enc = ctx.bzip2_encode(files, [len(f) + len(f) // 64 + 1024 for f in files], level).check()
    for f, z in zip(files, enc.outputs):
        assert bz2.decompress(z) == f, level
    dec = ctx.bzip2_decode(enc.outputs, [len(f) for f in files]).check()
    assert dec.outputs == files, level
