"""Records what the Python host layer (rust_compress_amd/api.py, lz4frame.py, bzip2.py, zstd.py) hands to librcx.so and what it makes of the
answers, with a STAND-IN for the library: no GPU, no librcx.so, no torch.  tests/test_api_marshal.py replays the same cases and compares
them with tests/golden/api_marshal.json for equality.

    python tests/gen_api_marshal_golden.py          rewrites the recording from the rust_compress_amd that is first on sys.path

The recording pins the marshalling: it is regenerated only when a method is meant to hand over something else.

The stand-in (StandIn) answers every rcx_*_batch entry point.  It reads the rcx_batch through ctypes and records the function name, nblocks
and mem, which of the nine pointers are null, the n entries of in_off / in_len / out_off / out_cap, the input buffer up to the highest byte a
block or a dictionary range names, the output buffer up to the highest slot end AS IT IS BEFORE THE CALL (histories are preloaded there), and
every extra argument (EXTRA below: scalars as integers, arrays by content).  Then it writes results back so that the unpacking and the retry
loops run:

    block i wants 3 * in_len[i] + 1 output bytes (an input that starts with NIL: 0 bytes -- "a file that decodes to nothing", the only way a
    slot of capacity 0 ever fits)
    out_cap[i] >= want      status 0, out_len = want, in_used = in_len, the bytes (i + j) & 255 in the slot
    out_cap[i] <  want      RCX_E_OUTPUT_TOO_SMALL, out_len = want
    an input that starts with BAD      RCX_E_MALFORMED, out_len = 0
    the checksum entry points (NO_OUTPUT) have no slots: status 0, in_used = in_len
    flag, checksum, origin and hash arrays get i + 1
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "api_marshal.json")

E_OUTPUT_TOO_SMALL, E_MALFORMED = 2, 3
U8, U32, U64 = np.uint8, np.uint32, np.uint64
# include/rcx.h: what follows (rcx_ctx*, const rcx_batch*).  "int": a scalar; (name, "in" | "out", element type, "n" | "samples"): an array of
# nblocks entries, or of one entry per sample of every corpus (rcx_dict_train_batch's sample_len)
_PLAIN = ("lz4_decode", "lz4_encode", "deflate_encode", "zlib_encode", "gzip_encode", "mtf_encode", "mtf_decode", "dc_encode", "dc_encode_ctx",
          "ari_byte_encode", "ari_byte_decode", "ari_proxy_encode", "ari_proxy_decode", "ari_apm_encode", "ari_apm_decode", "rle_encode",
          "rle_decode", "bzip2_decode")
_DICT = [("dict_off", "in", U64, "n"), ("dict_len", "in", U64, "n")]
_FLAGS, _HIST, _ID = ("flags", "out", U32, "n"), ("hist_len", "in", U64, "n"), ("dict_id", "in", U32, "n")
EXTRA = {"rcx_%s_batch" % k: [] for k in _PLAIN}
EXTRA.update({"rcx_%s_batch" % k: ["int"] for k in ("lz4_encode_hc", "deflate_encode_level", "zlib_encode_level", "gzip_encode_level",
                                                    "ari_binary_encode", "ari_binary_decode", "bzip2_encode")})
EXTRA.update({"rcx_%s_batch" % k: [(w, "out", U32, "n")] for k, w in (("inflate", "flags"), ("zlib_decode", "flags"), ("gzip_decode", "flags"),
                                                                     ("adler32", "adler"), ("crc32", "crc"), ("bwt_forward", "origin"),
                                                                     ("bwt_suffixes", "origin"))})
EXTRA.update({"rcx_%s_batch" % k: [("origin", "in", U32, "n")] for k in ("bwt_inversion_table", "bwt_inverse", "bwt_inverse_minimal")})
EXTRA.update({"rcx_%s_batch" % k: [("n_out", "in", U64, "n")] for k in ("dc_decode", "dc_decode_ctx")})
EXTRA.update({
    "rcx_xxh32_batch": ["int", ("hash", "out", U32, "n")],
    "rcx_xxh64_batch": ["int", ("hash", "out", U64, "n")],
    "rcx_lz4_decode_linked_batch": [("link", "in", U8, "n"), ("dict_len", "in", U64, "n")],
    "rcx_lz4_encode_hc_hist_batch": ["int", _HIST],
    "rcx_deflate_encode_hist_batch": ["int", _HIST],
    "rcx_zlib_encode_dict_batch": ["int", _HIST, _ID],
    "rcx_inflate_hist_batch": [_FLAGS, _HIST],
    "rcx_zlib_decode_dict_batch": [_FLAGS, _HIST, _ID],
    "rcx_lz4_encode_hc_shared_batch": ["int"] + _DICT,
    "rcx_deflate_encode_shared_batch": ["int"] + _DICT,
    "rcx_zlib_encode_shared_batch": ["int"] + _DICT + [_ID],
    "rcx_lz4_decode_shared_batch": _DICT,
    "rcx_inflate_shared_batch": [_FLAGS] + _DICT,
    "rcx_zlib_decode_shared_batch": [_FLAGS] + _DICT + [_ID],
    "rcx_zstd_decode_batch": _DICT,
    "rcx_dict_train_batch": [("nsamples", "in", U32, "n"), ("sample_len", "in", U64, "samples"), "int", "int", "int"],
})
NO_OUTPUT = ("rcx_adler32_batch", "rcx_crc32_batch", "rcx_xxh32_batch", "rcx_xxh64_batch")
POINTERS = ("in_base", "in_off", "in_len", "out_base", "out_off", "out_cap", "out_len", "in_used", "status")


def _buf(b):
    """bytes -> hex; {"zeros": length} for eight or more bytes that are all 0; for a long buffer its length, SHA-256 and both ends"""
    b = bytes(b)
    if len(b) >= 8 and not any(b):
        return {"zeros": len(b)}
    if len(b) <= 40:
        return b.hex()
    return {"len": len(b), "sha256": hashlib.sha256(b).hexdigest(), "head": b[:12].hex(), "tail": b[-12:].hex()}


def _value(a):
    """a ctypes scalar, a ctypes pointer or a Python int -> int or None"""
    return getattr(a, "value", a)


def _read(ptr, dtype, count):
    if ptr is None:
        return None
    return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype).copy()


def _write(ptr, values, dtype):
    if ptr is not None and len(values):
        a = np.asarray(values, dtype)
        C.memmove(ptr, a.tobytes(), a.nbytes)


class StandIn:
    """what stands in for rust_compress_amd._native.lib() (the module's docstring)"""

    def __init__(self):
        self.calls = []

    # ---- the functions that take no batch: fixed, simple formulas
    def rcx_ctx_create(self, device, handle):
        handle._obj.value = 0x1000
        return 0

    def rcx_ctx_destroy(self, handle):
        pass

    def rcx_last_error(self, handle):
        return b"stand-in error"

    def rcx_status_string(self, status):
        return b"status %d" % status

    def rcx_lz4_compression_bound(self, n):
        return n + n // 255 + 16

    def rcx_deflate_compression_bound(self, n):
        return n + 64

    def rcx_ari_byte_encode_bound(self, n):
        return 2 * n + 32

    def rcx_rle_encode_bound(self, n):
        return 2 * n + 2

    def __getattr__(self, name):
        if name not in EXTRA:
            raise AttributeError(name)
        return lambda handle, batch, *extra: self._batch(name, getattr(batch, "_obj", None) or batch.contents, extra)

    def _batch(self, name, b, extra):
        n = int(b.nblocks)
        ptr = {k: getattr(b, k) for k in POINTERS}
        rec = {"fn": name, "nblocks": n, "mem": int(b.mem), "null": [k for k in POINTERS if ptr[k] is None]}
        arr = {k: _read(ptr[k], U64, n) for k in ("in_off", "in_len", "out_off", "out_cap")}
        for k, a in arr.items():
            rec[k] = None if a is None else a.tolist()
        spec = EXTRA[name]
        assert len(extra) == len(spec), "%s: %d extra arguments, include/rcx.h has %d" % (name, len(extra), len(spec))
        in_end = max([int(o) + int(l) for o, l in zip(arr["in_off"], arr["in_len"])] or [0])
        rec["extra"], outs, given = [], [], {}
        for a, s in zip(extra, spec):
            if s == "int":
                rec["extra"].append(int(_value(a)))
                continue
            what, way, dtype, count = s
            p = _value(a)
            count = n if count == "n" else int(sum(given["nsamples"]))
            if way == "out":
                rec["extra"].append([what, "null" if p is None else "out"])
                outs.append((p, dtype))
            else:
                given[what] = _read(p, dtype, count)
                rec["extra"].append([what, None if p is None else given[what].tolist()])
        if given.get("dict_off") is not None and given.get("dict_len") is not None:
            in_end = max([in_end] + [int(o) + int(l) for o, l in zip(given["dict_off"], given["dict_len"])])
        rec["in"] = None if ptr["in_base"] is None else _buf(C.string_at(ptr["in_base"], in_end))
        slots = name not in NO_OUTPUT and ptr["out_base"] is not None
        if ptr["out_base"] is not None and arr["out_off"] is not None and arr["out_cap"] is not None:
            out_end = max([int(o) + int(c) for o, c in zip(arr["out_off"], arr["out_cap"])] or [0])
            rec["out_before"] = _buf(C.string_at(ptr["out_base"], out_end))
        self.calls.append(rec)

        out_len, in_used, status = [0] * n, [0] * n, [0] * n
        for i in range(n):
            off, ln = int(arr["in_off"][i]), int(arr["in_len"][i])
            head = C.string_at(ptr["in_base"] + off, min(ln, 3))
            want = 0 if head == b"NIL" else 3 * ln + 1
            if head == b"BAD":
                status[i] = E_MALFORMED
            elif not slots:
                in_used[i] = ln
            elif int(arr["out_cap"][i]) < want:
                status[i], out_len[i] = E_OUTPUT_TOO_SMALL, want
            else:
                out_len[i], in_used[i] = want, ln
                C.memmove(ptr["out_base"] + int(arr["out_off"][i]), bytes((i + j) & 255 for j in range(want)), want)
        _write(ptr["out_len"], out_len, U64)
        _write(ptr["in_used"], in_used, U64)
        _write(ptr["status"], status, np.int32)
        for p, dtype in outs:
            _write(p, [i + 1 for i in range(n)], dtype)
        return 0


def _ser(x):
    """a result of the layer -> what JSON holds"""
    if isinstance(x, (bytes, bytearray)):
        return _buf(x)
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype), "v": x.tolist()}
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, BaseException):
        d = {"exc": type(x).__name__, "msg": str(x)}
        if hasattr(x, "results"):
            d["results"] = _ser(x.results)
        return d
    if isinstance(x, (list, tuple)):
        return [_ser(v) for v in x]
    if hasattr(x, "outputs") and hasattr(x, "in_used"):                # api.Result
        return {k: _ser(getattr(x, k)) for k in ("outputs", "out_len", "in_used", "status", "aux")}
    assert x is None or isinstance(x, (int, str, bool)), type(x)
    return x


def _ramp(n, step):
    """n bytes that repeat nowhere near a clamp: which 64 KiB (32 KiB) of them were taken shows in the buffer's hash"""
    return bytes((i * step + (i >> 8)) & 255 for i in range(n))


def _zst(declared):
    """a .zst file of one single-segment frame that DECLARES `declared` bytes (one byte of Frame_Content_Size) and holds one empty raw block:
    zstd.declared_size reads it; the stand-in decodes nothing"""
    return bytes.fromhex("28b52ffd") + bytes([0x20, declared]) + bytes([1, 0, 0])


def _lz4_frames():
    """two blobs for lz4frame.decode_frames whose header checksum byte is the 0 that the stand-in's hashes (i + 1) give: an independent frame
    of a compressed and a stored block, and a linked frame of a compressed and a stored block (whose second block has no slot of its own: the
    stand-in, which knows nothing of links, fails it)"""
    def frame(flg, blocks):
        out = bytes.fromhex("04224d18") + bytes([flg, 0x40, 0])
        for stored, payload in blocks:
            out += (len(payload) | (0x80000000 if stored else 0)).to_bytes(4, "little") + payload
        return out + b"\0\0\0\0"
    return [frame(0x60, [(False, b"\x11ab"), (True, b"stored")]), frame(0x40, [(False, b"\x22cde"), (True, b"lit")])]


def cases(R):
    """-> [(name, callable(ctx))]: every call of the host layer that the recording pins.  R: the rust_compress_amd under test"""
    from rust_compress_amd import bzip2, lz4frame, zstd
    blobs = [b"hello world", b"", b"xyz" * 5]
    bad = [b"fits", b"BAD file", b"NIL", b"needs a second call"]
    caps = [64, 1, 9]                                                  # (the last one is too small)
    H = [b"history-0", None, b"h2"]
    D = [b"dict-A", None, b"dict-A"]                                   # a repeated dictionary: it lies in the buffer once
    h70, h40 = _ramp(70000, 7), _ramp(40000, 11)
    base = np.frombuffer(b"DDDDDDDDblock-0block-1!" + b"\0" * 16, np.uint8)
    off, lens, hist, d_off, d_len = [8, 15], [7, 8], [8, 7], [0, 2], [8, 0]
    empty = np.zeros(0, np.uint8)
    out = []

    def add(name, fn):
        out.append((name, fn))

    def each(method, *args, **kw):
        add("%s(%s)" % (method, ", ".join(["..."] * len(args) + ["%s=%s" % (k, v if isinstance(v, (int, bool, type(None))) else "...") for k, v in kw.items()])
                                 + " #%d" % len(out)), lambda c: getattr(c, method)(*args, **kw))

    # ---- the plain path
    each("lz4_decode_blocks", blobs, caps)
    each("lz4_decode_blocks", [], [])
    each("lz4_decode_blocks", [b"BAD block", b"ok"], [64, 64])
    each("lz4_encode_blocks", blobs)
    each("lz4_encode_hc_blocks", blobs)
    each("lz4_encode_hc_blocks", blobs, level=12, caps=caps)
    each("inflate", blobs, caps)
    each("inflate", [], [])
    each("zlib_decode", blobs, caps)
    each("gzip_decode", blobs, caps)
    each("adler32", blobs)
    each("adler32", [])
    each("crc32", blobs)
    for level in (1, 6):
        for m in ("deflate_encode", "zlib_encode", "gzip_encode"):
            each(m, blobs, level=level)
            each(m, blobs, caps=caps, level=level)
    each("deflate_encode", [], level=1)
    each("deflate_encode", [], level=6)
    each("bwt_forward", blobs)
    each("bwt_suffixes", blobs)
    each("bwt_inversion_table", blobs, [3, 0, 14])
    each("bwt_inverse", blobs, [3, 0, 14])
    each("bwt_inverse_minimal", blobs, [3, 0, 14])
    each("mtf_encode", blobs)
    each("mtf_decode", blobs)
    each("dc_encode", blobs)
    each("dc_decode", blobs, [40, 1, 7])
    each("dc_encode_ctx", blobs)
    each("dc_decode_ctx", [b"w" * 1040, b"", b"xyz" * 5], [40, 1, 7])
    each("ari_byte_encode", blobs)
    each("ari_byte_decode", blobs, caps)
    each("ari_binary_encode", blobs, 5)
    each("ari_binary_decode", blobs, 5, [40, 1, 7])
    each("ari_proxy_encode", blobs)
    each("ari_proxy_decode", blobs, [40, 1, 7])
    each("ari_apm_encode", blobs)
    each("ari_apm_decode", blobs, [40, 1, 7])
    each("rle_encode", blobs)
    each("rle_decode", blobs, caps)
    each("bzip2_decode", blobs, caps)
    each("bzip2_decode", [], [])
    each("bzip2_encode", blobs, caps)
    each("bzip2_encode", blobs, [64, 64, 64], level=3)
    each("bzip2_encode", [], [])

    # ---- history in front of the block (encode) or of the slot (decode)
    for m in ("lz4_encode_hc_hist", "deflate_encode_hist"):
        each(m, base, off, lens, hist)
        each(m, base, off, lens, None, level=4, caps=[64, 9])
        each(m, base, np.array(off, np.uint32), np.array(lens, np.int64), np.array(hist, np.uint16))
        each(m, empty, [0, 0], [0, 0], [0, 0])
        each(m, empty, [], [], [])
        each(m, empty, [], [], None)
        each(m, base, off, lens, [8])
    for m, long in (("lz4_encode_hc_hist_blocks", h70), ("deflate_encode_hist_blocks", h40)):
        each(m, blobs, H)
        each(m, blobs, H, level=3, caps=caps)
        each(m, blobs, [long, None, long])
        each(m, [], [])
        each(m, blobs, H[:2])
    each("inflate_hist_blocks", blobs, H, caps)
    each("inflate_hist_blocks", blobs, [h40, None, h40], caps)
    each("inflate_hist_blocks", [], [], [])
    each("inflate_hist_blocks", blobs, H[:2], caps)

    # ---- dictionaries anywhere in the input buffer
    for m in ("lz4_encode_hc_shared", "deflate_encode_shared"):
        each(m, base, off, lens, d_off, d_len)
        each(m, base, off, lens, None, None, level=4, caps=[64, 9])
        each(m, empty, [], [], [], [])
        each(m, empty, [], [], None, None)
        each(m, base, off, lens, d_off, None)
        each(m, base, off, lens, None, d_len)
        each(m, base, off, lens, d_off, [8])
    for m in ("lz4_decode_shared", "inflate_shared"):
        each(m, base, off, lens, d_off, d_len, [64, 9])
        each(m, base, off, lens, None, None, [64, 9])
        each(m, empty, [], [], [], [], [])
        each(m, empty, [0], [0], None, None, [4])
        each(m, base, off, lens, d_off, None, [64, 9])
        each(m, base, off, lens, [0], d_len, [64, 9])
    for m, long in (("lz4_encode_hc_dict_blocks", h70), ("deflate_encode_dict_blocks", h40)):
        each(m, blobs, b"one for all")
        each(m, blobs, D, level=5, caps=caps)
        each(m, blobs, [long, None, long])
        each(m, [], b"nobody's")
        each(m, blobs, D[:2])
    for m, long in (("lz4_decode_dict_blocks", h70), ("inflate_dict_blocks", h40)):
        each(m, blobs, b"one for all", caps)
        each(m, blobs, D, caps)
        each(m, blobs, [long, None, long], caps)
        each(m, [], b"nobody's", [])
        each(m, blobs, D[:2], caps)

    # ---- zlib with a preset dictionary: in front of every block / slot, or shared
    for zd in (None, b"preset", D):
        each("zlib_encode", blobs, level=6, zdict=zd)
        each("zlib_encode", blobs, caps=caps, level=6, zdict=zd)
        each("zlib_decode", blobs, caps, zdict=zd)
    each("zlib_encode", blobs, level=6, zdict=D, shared=True)
    each("zlib_encode", blobs, caps=caps, level=6, zdict=b"preset", shared=True)
    each("zlib_decode", blobs, caps, zdict=D, shared=True)
    each("zlib_encode", blobs, level=6, zdict=[h40, None, h40])
    each("zlib_encode", blobs, level=6, zdict=[h40, None, h40], shared=True)
    each("zlib_decode", blobs, caps, zdict=[h40, None, h40])
    each("zlib_decode", blobs, caps, zdict=[h40, None, h40], shared=True)
    for shared in (False, True):
        each("zlib_encode", [], level=6, zdict=b"preset", shared=shared)
        each("zlib_decode", [], [], zdict=b"preset", shared=shared)
        each("zlib_encode", blobs, level=6, zdict=D[:2], shared=shared)
        each("zlib_decode", blobs, caps, zdict=D[:2], shared=shared)

    # ---- the trainer
    each("train_dictionaries", [[b"abc", b"de"], []], [32, 8])
    each("train_dictionaries", [[b"abc", b"de"], []], [32, 8], k=16, d=6, f=10)
    each("train_dictionaries", [[b"abc", b"de"], []], [4, 8])                 # a capacity too small: the call raises BlockError
    each("train_dictionaries", [], [])
    each("train_dictionaries", [[b"abc"]], [32, 8])
    each("train_dictionary", [b"sample one", b"", b"sample three"], 128)

    # ---- whole files, hashes
    for dictionary in (None, b"raw content", D):
        each("zstd_decode", blobs, caps, dictionary)
    each("zstd_decode", [], [])
    each("zstd_decode", [], [], b"raw content")
    each("zstd_decode", blobs, caps, D[:2])
    each("xxh64", blobs)
    each("xxh64", blobs, seed=-1)
    each("xxh64", blobs, seed=(1 << 64) + 5)
    each("xxh64", [])

    # ---- lz4frame
    cat = np.frombuffer(b"0123456789abcdef" + b"\0", np.uint8)
    add("lz4frame.xxh32_many", lambda c: lz4frame.xxh32_many(cat, [0, 4, 16], [4, 12, 0], 7, c))
    add("lz4frame.xxh32_many(uint64 offsets)", lambda c: lz4frame.xxh32_many(cat, np.array([0, 4], np.uint64), [4, 12], ctx=c))
    add("lz4frame.xxh32_many(n = 0)", lambda c: lz4frame.xxh32_many(cat, [], [], 0, c))
    add("lz4frame.xxh32_many(empty base)", lambda c: lz4frame.xxh32_many(empty, [0], [0], 0, c))
    add("lz4frame.xxh32", lambda c: lz4frame.xxh32(b"one buffer", 3, c))
    for dictionary in (None, b"frame dictionary"):
        add("lz4frame.decode_frames(dictionary=%s)" % (dictionary and "..."),
            lambda c, d=dictionary: lz4frame.decode_frames(_lz4_frames(), d, verify=False, return_exceptions=True, ctx=c))
    add("lz4frame.decode_frames(nothing to decode)", lambda c: lz4frame.decode_frames([b""], ctx=c))

    # ---- the exact-size retry: bzip2.decode_many, bzip2.encode_many, zstd.decode_many
    for rex in (False, True):
        for used in (False, True):
            add("bzip2.decode_many(return_exceptions=%s, with_used=%s)" % (rex, used),
                lambda c, rex=rex, used=used: bzip2.decode_many(bad, ctx=c, return_exceptions=rex, with_used=used))
    add("bzip2.decode_many(all fit)", lambda c: bzip2.decode_many([b"NIL", b"NIL2"], ctx=c, with_used=True))
    add("bzip2.decode_many(none fails)", lambda c: bzip2.decode_many([b"a", b"NIL", b"bc"], ctx=c))
    add("bzip2.decode_many(n = 0)", lambda c: bzip2.decode_many([], ctx=c))
    big = b"q" * 600                                                    # 3 * 600 + 1 > 600 + 600 / 64 + 1024: the second call
    add("bzip2.encode_many", lambda c: bzip2.encode_many([b"fits", big, b"", big[:550]], 5, ctx=c))
    add("bzip2.encode_many(all fit)", lambda c: bzip2.encode_many([b"fits", b""], ctx=c))
    add("bzip2.encode_many(BAD)", lambda c: bzip2.encode_many([b"fits", big, b"BAD data"], ctx=c))
    add("bzip2.encode_many(BAD alone)", lambda c: bzip2.encode_many([b"BAD data"], ctx=c))
    add("bzip2.encode_many(n = 0)", lambda c: bzip2.encode_many([], ctx=c))
    add("bzip2.encode_many(level 0)", lambda c: bzip2.encode_many([b"x"], 0, ctx=c))
    files = [_zst(100), b"BAD file", _zst(5), b"NIL", b"no frame: sized by the call"]
    for dictionary in (None, b"raw content", [b"d0", None, b"d2", b"d0", b"d2"]):
        for rex, used in ((False, False), (False, True), (True, False), (True, True)) if dictionary is None else ((False, False), (True, True)):
            add("zstd.decode_many(dictionary=%s, return_exceptions=%s, with_used=%s)" % (type(dictionary).__name__, rex, used),
                lambda c, d=dictionary, rex=rex, used=used: zstd.decode_many(files, d, ctx=c, return_exceptions=rex, with_used=used))
    add("zstd.decode_many(all fit)", lambda c: zstd.decode_many([_zst(100), b"NIL"], b"raw content", ctx=c, with_used=True))
    add("zstd.decode_many(a dictionary list too short)", lambda c: zstd.decode_many(files, [b"d0"], ctx=c, return_exceptions=True))
    add("zstd.decode_many(n = 0)", lambda c: zstd.decode_many([], ctx=c))
    return out


def record(stand_in):
    """-> {case: {"calls": what the library was handed, "result" | "raises": what came back}}.  rust_compress_amd._native.lib must already
    answer with stand_in (the test: monkeypatch; the generator: main below)"""
    import rust_compress_amd as R
    ctx = R.Context()
    rec = {}
    for name, fn in cases(R):
        assert name not in rec, name
        stand_in.calls = []
        try:
            got = {"result": _ser(fn(ctx))}
        except Exception as e:                                          # (ValueError, BlockError, CompressError and its kin: type and message)
            got = {"raises": _ser(e)}
        rec[name] = dict(calls=stand_in.calls, **got)
    ctx.close()
    return rec


def dumps(rec):
    """one case per line"""
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rec.items()) + "\n}\n"


def main():
    sys.path.append(os.path.dirname(HERE))                             # (last: a rust_compress_amd put on the path by the caller comes first)
    import rust_compress_amd._native as N
    stand_in = StandIn()
    real, N.lib = N.lib, lambda: stand_in
    try:
        text = dumps(record(stand_in))
    finally:
        N.lib = real
    with open(GOLDEN, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes, from %s" % (GOLDEN, text.count("\n") - 2, len(text), os.path.dirname(N.__file__)))


if __name__ == "__main__":
    main()
