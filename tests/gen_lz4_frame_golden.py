"""Writes tests/golden/lz4_frame/: small LZ4 frames made by the system's liblz4 (LZ4F_compressFrame, LZ4F_compressFrame_usingCDict,
through ctypes) and manifest.json with each frame's preferences, its raw length and raw XXH32 (libxxhash).  The raw inputs come from
rust_compress_amd.synth and are not stored: the manifest names the generator calls (`raw`, `dictionary`: lists of [kind, bytes, seed]
whose outputs are concatenated).  Run once, by hand, where liblz4.so.1 and libxxhash.so.0 are installed:
    python tests/gen_lz4_frame_golden.py
TEST INFRASTRUCTURE; the tests read the files, never this script's libraries (tests/test_lz4_frame_ref.py cross-checks against them
only where ctypes finds them)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from rust_compress_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "golden", "lz4_frame")
LIMIT = 100 << 10


class FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class Preferences(C.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


def libs():
    lz4 = C.CDLL("liblz4.so.1")
    xxh = C.CDLL("libxxhash.so.0")
    lz4.LZ4F_compressFrameBound.restype = C.c_size_t
    lz4.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    lz4.LZ4F_compressFrame.restype = C.c_size_t
    lz4.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lz4.LZ4F_isError.argtypes = [C.c_size_t]
    lz4.LZ4F_createCDict.restype = C.c_void_p
    lz4.LZ4F_createCDict.argtypes = [C.c_void_p, C.c_size_t]
    lz4.LZ4F_freeCDict.argtypes = [C.c_void_p]
    lz4.LZ4F_createCompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lz4.LZ4F_createCompressionContext.restype = C.c_size_t
    lz4.LZ4F_freeCompressionContext.argtypes = [C.c_void_p]
    lz4.LZ4F_compressFrame_usingCDict.restype = C.c_size_t
    lz4.LZ4F_compressFrame_usingCDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    xxh.XXH32.restype = C.c_uint
    xxh.XXH32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    return lz4, xxh


def make(spec):
    return b"".join(synth.gen(k, n, seed).tobytes() for k, n, seed in spec)


def prefs(p):
    pr = Preferences()
    pr.frameInfo.blockSizeID = p["block_size_id"]
    pr.frameInfo.blockMode = 0 if p["linked"] else 1
    pr.frameInfo.contentChecksumFlag = int(p["content_checksum"])
    pr.frameInfo.blockChecksumFlag = int(p["block_checksum"])
    pr.frameInfo.contentSize = 1 if p["content_size"] else 0        # (LZ4F_compressFrame replaces a non-zero value by the source size)
    pr.frameInfo.dictID = p.get("dict_id") or 0
    pr.compressionLevel = p["level"]
    return pr


def compress(lz4, raw, p, dictionary=None):
    pr = prefs(p)
    cap = lz4.LZ4F_compressFrameBound(len(raw), C.byref(pr))
    dst = C.create_string_buffer(cap)
    if dictionary is None:
        n = lz4.LZ4F_compressFrame(dst, cap, raw, len(raw), C.byref(pr))
    else:
        cctx = C.c_void_p()
        assert not lz4.LZ4F_isError(lz4.LZ4F_createCompressionContext(C.byref(cctx), 100))
        cd = lz4.LZ4F_createCDict(dictionary, len(dictionary))
        n = lz4.LZ4F_compressFrame_usingCDict(cctx, dst, cap, raw, len(raw), cd, C.byref(pr))
        lz4.LZ4F_freeCDict(cd)
        lz4.LZ4F_freeCompressionContext(cctx)
    assert not lz4.LZ4F_isError(n), n
    return dst.raw[:n]


def P(linked, bid, bc=False, cc=False, cs=False, level=0, dict_id=None):
    return {"linked": linked, "block_size_id": bid, "block_checksum": bc, "content_checksum": cc, "content_size": cs, "level": level,
            "dict_id": dict_id}


# name -> (frames: [(raw spec, preferences) or ("skip", user bytes)], dictionary spec)
FIXTURES = [
    ("linked_b4", [([["text", 200000, 7001]], P(True, 4, cc=True))], None),
    ("linked_b4_all", [([["words", 150000, 7002]], P(True, 4, bc=True, cc=True, cs=True))], None),
    ("linked_b5_hc", [([["text", 200000, 7003], ["runs", 150000, 7004]], P(True, 5, cc=True, level=9))], None),
    ("indep_b4_plain", [([["text", 150000, 7005]], P(False, 4))], None),
    ("indep_b5_bc_cs", [([["text", 180000, 7006], ["runs", 120000, 7007]], P(False, 5, bc=True, cs=True))], None),
    ("dict_linked", [([["text", 100000, 7008]], P(True, 4, cc=True, dict_id=0x1234ABCD))], [["text", 70000, 7009]]),
    ("dict_indep", [([["text", 140000, 7010]], P(False, 4, cc=True, bc=True, dict_id=0x1234ABCD))], [["text", 70000, 7009]]),
    ("empty", [([], P(True, 4, cc=True))], None),
    ("stored", [([["rand", 70000, 7011]], P(True, 4, bc=True, cc=True, cs=True))], None),
    ("concat_skip", [([["text", 30000, 7012]], P(True, 4, cc=True)), ("skip", "skippable user data"),
                     ([["runs", 40000, 7013]], P(False, 4, cc=True, cs=True))], None),
]


def main():
    lz4, xxh = libs()
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    for name, frames, dspec in FIXTURES:
        d = make(dspec) if dspec else None
        blob, entries = b"", []
        for fr in frames:
            if fr[0] == "skip":
                user = fr[1].encode()
                blob += (0x184D2A53).to_bytes(4, "little") + len(user).to_bytes(4, "little") + user
                entries.append({"skippable": True, "user_len": len(user)})
                continue
            spec, p = fr
            raw = make(spec)
            blob += compress(lz4, raw, p, d)
            entries.append({"skippable": False, "raw": spec, "raw_len": len(raw), "raw_xxh32": int(xxh.XXH32(raw, len(raw), 0)), "prefs": p})
        assert len(blob) < LIMIT, (name, len(blob))
        with open(os.path.join(OUT, name + ".lz4"), "wb") as f:
            f.write(blob)
        manifest.append({"name": name, "file": name + ".lz4", "bytes": len(blob), "dictionary": dspec, "frames": entries})
        print("%-16s %6d bytes" % (name, len(blob)))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
