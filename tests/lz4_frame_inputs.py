"""Inputs shared by the LZ4 frame tests: the liblz4-made fixtures of tests/golden/lz4_frame (tests/gen_lz4_frame_golden.py) with their raw
data regenerated from the manifest, and hand-built chains of linked LZ4 blocks whose expected bytes come from tests/lz4_frame_ref.py."""
import ctypes as C
import ctypes.util
import json
import os

import numpy as np

import corpus
import lz4_frame_ref as R
from rust_compress_amd import synth

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_frame")


def make(spec):
    return b"".join(synth.gen(k, n, seed).tobytes() for k, n, seed in spec)


class Fixture:
    """name, blob, dictionary (bytes or None), frames (the manifest's entries), raw (the content of all frames, concatenated)"""


_FIX = None


def fixtures():
    global _FIX
    if _FIX is None:
        _FIX = []
        for e in json.load(open(os.path.join(DIR, "manifest.json"))):
            f = Fixture()
            f.name, f.frames = e["name"], e["frames"]
            f.blob = open(os.path.join(DIR, e["file"]), "rb").read()
            assert len(f.blob) == e["bytes"]
            f.dictionary = make(e["dictionary"]) if e["dictionary"] else None
            f.raws = [make(fr["raw"]) for fr in e["frames"] if not fr["skippable"]]
            f.raw = b"".join(f.raws)
            _FIX.append(f)
    return _FIX


def fixture(name):
    return [f for f in fixtures() if f.name == name][0]


def random_chain(rng, nblocks, dictionary=b"", nseq=(20, 120), far=0.5):
    """A chain of `nblocks` linked LZ4 blocks behind `dictionary`: random literals, matches whose offsets reach anywhere into the history
    (dictionary + the chain so far, at most 65535 back) -- with probability `far` beyond the block's own bytes when there is any history
    -- and now and then long or self-overlapping.  -> (blocks, the bytes each block decodes to, by the reference decoder)."""
    blocks, raws = [], []
    hist = bytes(dictionary)[-65536:]
    for _ in range(nblocks):
        seqs, produced = [], 0
        for _ in range(int(rng.integers(nseq[0], nseq[1]))):
            L = int(rng.choice([0, 0, 1, 2, 3, 6, 14, 15, 16, 40, 300]))
            if produced == 0 and not hist and L == 0:
                L = 1
            lit = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            produced += L
            reach = min(len(hist) + produced, 65535)
            if len(hist) and rng.random() < far:
                off = int(rng.integers(produced + 1, reach + 1)) if reach > produced else reach
            else:
                off = int(rng.integers(1, max(min(produced, 65535), 1) + 1)) if produced else int(rng.integers(1, reach + 1))
            if rng.random() < 0.1:
                off = min(reach, int(rng.choice([1, 2, 3, 15, 16, 17, 33])))
            M = int(rng.choice([4, 5, 8, 18, 19, 20, 64, 65, 70, 300, 1100])) if rng.random() < 0.15 else int(rng.integers(4, 19))
            seqs.append((lit, M, off))
            produced += M
        tail = rng.integers(0, 256, int(rng.choice([0, 1, 5, 12, 40])), dtype=np.uint8).tobytes()
        b = corpus.lz4_stream(seqs, tail)
        raw = R.block_decode(b, hist)
        blocks.append(b)
        raws.append(raw)
        hist = (hist + raw)[-65536:]
    return blocks, raws


def load_lib(name):
    """the system's lib<name> through ctypes, or None where it is not installed (the GPU machine may have neither liblz4 nor libxxhash)"""
    path = ctypes.util.find_library(name)
    try:
        return C.CDLL(path) if path else None
    except OSError:
        return None


def lz4f_decompress(lz4, blob):
    """LZ4F_decompress of a whole frame -> bytes; raises ValueError with liblz4's error name"""
    lz4.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lz4.LZ4F_createDecompressionContext.restype = C.c_size_t
    lz4.LZ4F_decompress.restype = C.c_size_t
    lz4.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    lz4.LZ4F_isError.argtypes = [C.c_size_t]
    lz4.LZ4F_getErrorName.argtypes = [C.c_size_t]
    lz4.LZ4F_getErrorName.restype = C.c_char_p
    lz4.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    d = C.c_void_p()
    assert not lz4.LZ4F_isError(lz4.LZ4F_createDecompressionContext(C.byref(d), 100))
    out = bytearray()
    dst = C.create_string_buffer(1 << 20)
    pos = 0
    try:
        while True:
            dn, sn = C.c_size_t(len(dst)), C.c_size_t(len(blob) - pos)
            src = C.create_string_buffer(blob[pos:], len(blob) - pos) if pos < len(blob) else None
            r = lz4.LZ4F_decompress(d, dst, C.byref(dn), src, C.byref(sn), None)
            if lz4.LZ4F_isError(r):
                raise ValueError(lz4.LZ4F_getErrorName(r).decode())
            out += dst.raw[:dn.value]
            pos += sn.value
            if r == 0 and pos >= len(blob):
                return bytes(out)
            if dn.value == 0 and sn.value == 0:
                raise ValueError("truncated")
    finally:
        lz4.LZ4F_freeDecompressionContext(d)
