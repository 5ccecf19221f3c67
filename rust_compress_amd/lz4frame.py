"""Standard LZ4 frames (lz4_Frame_format.md): what the `lz4` tool, liblz4's LZ4F_* and python-lz4 read and write.

`compress.lz4.Decoder` / `Encoder` mirror the reference crate's frame types quirk for quirk (a header checksum of 0, two zero words
at the end, no checksum ever verified, no linked blocks) and nothing outside this project exchanges files with them.  This module
is the conforming codec beside them: framing on the host, bytes on the device, MANY FRAMES PER CALL (one block alone loses to a
host thread; a batch does not):

    decode_frames(blobs)   every block of every frame through ONE rcx_lz4_decode_linked_batch call (linked blocks and dictionaries
                           are that call's history), every block checksum through one rcx_xxh32_batch call, every content
                           checksum through another
    encode_frames(blobs)   independent blocks from the greedy encoder (level=None) or the high-compression one (level 1..12), or --
                           with a level -- linked blocks and blocks behind a dictionary (rcx_lz4_encode_hc_hist_batch: every block
                           of every frame in ONE call); checksums from rcx_xxh32_batch
    Decoder(r) / Encoder(w)   the buffered stream classes in the style of compress.py

There is no CPU path: the parsing is Python, every decoded, encoded or hashed byte comes from the device.
"""
import ctypes as C
import struct

import numpy as np

from . import _native as N
from . import compress as _compress
from .compress import CompressError

MAGIC = 0x184D2204
SKIP_LO, SKIP_HI = 0x184D2A50, 0x184D2A5F
BLOCK_MAX = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
DICT_MAX = 64 << 10


class FrameError(CompressError):
    """A frame that cannot be decoded.  index: the blob's position in the batch; frame: the frame's number inside that blob (a blob
    may hold several frames back to back); what: one word for the check that failed (the subclasses below)."""
    what = "frame"

    def __init__(self, index, frame, detail="", status=N.E_MALFORMED):
        self.index, self.frame, self.detail = index, frame, detail
        CompressError.__init__(self, status, "lz4 frame %d of blob %d: %s%s" % (frame, index, self.what.replace("_", " "), (": " + detail) if detail else ""))


class FrameFormatError(FrameError):          # magic, version, reserved bits, block-size id
    what = "format"


class HeaderChecksumError(FrameError):
    what = "header_checksum"


class BlockChecksumError(FrameError):
    what = "block_checksum"


class ContentChecksumError(FrameError):
    what = "content_checksum"


class ContentSizeError(FrameError):
    what = "content_size"


class BlockTooLargeError(FrameError):
    what = "block_too_large"


class TruncatedError(FrameError):
    what = "truncated"


class BlockDataError(FrameError):            # the LZ4 block itself: the device's status for it
    what = "block_data"


class FrameTooLargeError(FrameError):        # a linked frame that may decode to 4 GiB or more: more than one chain of a call holds
    what = "frame_too_large"


class DictionaryError(FrameError):           # the frame names a dictionary and none was given
    what = "dictionary"


class FramesFailed(CompressError):
    """decode_frames without return_exceptions: some blobs failed.  results: one entry per blob, bytes or the blob's FrameError;
    errors: the FrameErrors alone."""

    def __init__(self, results):
        self.results = results
        self.errors = [r for r in results if isinstance(r, Exception)]
        CompressError.__init__(self, self.errors[0].status, "%d of %d blobs failed; the first: %s" % (len(self.errors), len(results), self.errors[0]))


def xxh32_many(base, offs, lens, seed=0, ctx=None):
    """XXH32 of base[offs[i] : offs[i] + lens[i]] for every i in one rcx_xxh32_batch call -> numpy uint32 array.  base: a numpy uint8 array."""
    n = len(offs)
    if n == 0:
        return np.zeros(0, np.uint32)
    ctx = ctx or _compress.context()
    h = np.zeros(n, np.uint32)
    ctx._batch("rcx_xxh32_batch", base, offs, lens, None, C.c_uint32(seed), h)
    return h


def xxh32(data, seed=0, ctx=None):
    """XXH32 of one buffer, on the device (a single stream is a serial chain there: use xxh32_many for rate)."""
    a = np.frombuffer(bytes(data), np.uint8)
    return int(xxh32_many(a, [0], [a.size], seed, ctx)[0])


def header_checksum(descriptor, ctx=None):
    return (xxh32(descriptor, 0, ctx) >> 8) & 0xFF


# ---------------------------------------------------------------------------------------------------------------- parsing (host)
class _Frame:
    __slots__ = ("independent", "block_checksum", "content_checksum", "content_size", "dict_id", "block_max", "blocks", "desc", "hc", "error")


def _parse_blob(blob, index):
    """-> list of _Frame of one blob (skippable frames dropped).  Offsets are relative to the blob.  The header checksum is NOT checked
    here: the descriptor's range is recorded and hashed with every other header of the batch.  Parsing stops at the first frame that
    cannot be parsed: that frame is the list's last one and carries the FrameError in .error (the frames before it are still decoded
    and checked, and an error of theirs -- or a bad header checksum of this one -- is what the blob reports: what a reader that goes
    through the blob in order would have met first)."""
    frames = []
    try:
        _parse_into(frames, blob, index)
    except FrameError as e:
        if not frames or frames[-1].error is not False:         # (the error came before this frame's header was complete)
            f = _Frame()
            f.desc = None
            frames.append(f)
        frames[-1].error = e
        frames[-1].blocks = []
    return frames


def _parse_into(frames, blob, index):
    pos, n, k = 0, len(blob), 0

    def need(cnt, what):
        if n - pos < cnt:
            raise TruncatedError(index, k, "in the %s at byte %d" % (what, pos), N.E_EOF)
    while pos < n:
        need(4, "magic")
        magic = struct.unpack_from("<I", blob, pos)[0]
        pos += 4
        if SKIP_LO <= magic <= SKIP_HI:
            need(4, "skippable frame's size")
            size = struct.unpack_from("<I", blob, pos)[0]
            pos += 4
            need(size, "skippable frame")
            pos += size
            continue
        if magic != MAGIC:
            raise FrameFormatError(index, k, "magic %08x" % magic, N.E_LZ4_MAGIC)
        need(2, "frame descriptor")
        f = _Frame()
        d0 = pos
        flg, bd = blob[pos], blob[pos + 1]
        pos += 2
        if flg >> 6 != 1:
            raise FrameFormatError(index, k, "version %d" % (flg >> 6), N.E_LZ4_VERSION)
        if flg & 2 or bd & 0x8F:
            raise FrameFormatError(index, k, "reserved bits set (FLG %02x BD %02x)" % (flg, bd))
        if (bd >> 4) < 4:
            raise FrameFormatError(index, k, "block-size id %d" % (bd >> 4))
        f.independent, f.block_checksum = bool(flg & 0x20), bool(flg & 0x10)
        f.block_max = BLOCK_MAX[bd >> 4]
        f.content_size = f.dict_id = f.content_checksum = None
        if flg & 8:
            need(8, "content size")
            f.content_size = struct.unpack_from("<Q", blob, pos)[0]
            pos += 8
        if flg & 1:
            need(4, "dictionary id")
            f.dict_id = struct.unpack_from("<I", blob, pos)[0]
            pos += 4
        need(1, "header checksum")
        f.desc, f.hc = (d0, pos - d0), blob[pos]
        pos += 1
        f.error = False                      # (False: being parsed; None: complete)
        frames.append(f)
        f.blocks = []                        # (stored?, offset, size, checksum or None)
        while True:
            need(4, "block size")
            w = struct.unpack_from("<I", blob, pos)[0]
            pos += 4
            if w == 0:
                break
            size = w & 0x7FFFFFFF
            if size > f.block_max:
                raise BlockTooLargeError(index, k, "block %d: %d bytes, the frame's maximum is %d" % (len(f.blocks), size, f.block_max))
            need(size, "block %d" % len(f.blocks))
            at = pos
            pos += size
            ck = None
            if f.block_checksum:
                need(4, "block checksum")
                ck = struct.unpack_from("<I", blob, pos)[0]
                pos += 4
            f.blocks.append((bool(w >> 31), at, size, ck))
        if flg & 4:
            need(4, "content checksum")
            f.content_checksum = struct.unpack_from("<I", blob, pos)[0]
            pos += 4
        f.error = None
        k += 1


def _literal_block(payload):
    """`payload` as an LZ4 block of literals alone: how a STORED block of a linked frame joins its chain on the device (the blocks
    behind it may copy from its bytes, and where those land is only known there)."""
    n = len(payload)
    out = bytearray([min(n, 15) << 4])
    if n >= 15:
        v = n - 15
        out += b"\xff" * (v // 255)
        out.append(v % 255)
    return bytes(out) + payload


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_frames(blobs, dictionary=None, verify=True, return_exceptions=False, ctx=None):
    """Decodes every blob -- one or more LZ4 frames back to back, skippable frames (magic 184D2A50..5F) between them skipped -- to its
    content: a list of bytes, one per blob.

    dictionary: bytes, or None.  Its last 64 KiB are the history in front of every frame's first block (block-linked frames) or of
        every block (block-independent frames).  A frame that carries a dictionary id and gets no dictionary fails (DictionaryError).
    verify=False skips the CONTENT checksum only (one stream per frame: the slow one for a single large frame).  Header checksums,
        block checksums and the content size are always checked.
    Failures are FrameError subclasses (HeaderChecksumError, BlockChecksumError, ContentChecksumError, ContentSizeError,
        BlockTooLargeError, TruncatedError, FrameFormatError, BlockDataError, FrameTooLargeError, DictionaryError) that name the blob,
        the frame inside it and what failed; a blob with several failing frames reports the first of them in reading order.  A blob that fails does not stop the others: with return_exceptions=True its entry in the result is the
        exception; otherwise the call decodes everything, then raises FramesFailed, whose .results is that same list."""
    ctx = ctx or _compress.context()
    blobs = [bytes(b) for b in blobs]
    nb = len(blobs)
    results = [None] * nb
    dct = bytes(dictionary)[-DICT_MAX:] if dictionary else b""
    parsed = []
    for i, blob in enumerate(blobs):
        fr = _parse_blob(blob, i)
        for k, f in enumerate(fr):
            if f.error is None and f.dict_id is not None and not dct:
                f.error, f.blocks = DictionaryError(i, k, "the frame needs dictionary %08x" % f.dict_id), []
                del fr[k + 1:]
                break
        parsed.append(fr)

    # one input buffer: the blobs back to back, then the stored blocks of linked frames as literal-only blocks
    base_of = np.zeros(nb + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=base_of[1:])
    extra = bytearray()
    extra_base = int(base_of[-1])
    in_off, in_len, link, dlen, out_off, out_cap = [], [], [], [], [], []
    hash_off, hash_len, hash_want, hash_who = [], [], [], []            # header and block checksums: one call
    frames = []                                                        # (blob, frame no, _Frame, pieces, head block or None)
    cur = 0
    dict_at = []
    for i, fr in enumerate(parsed):
        if results[i] is not None:
            continue
        for k, f in enumerate(fr):
            if f.desc is not None:
                hash_off.append(int(base_of[i]) + f.desc[0]); hash_len.append(f.desc[1]); hash_want.append(f.hc); hash_who.append((i, k, -1))
            if f.error is not None:                                # the frame at which parsing stopped: its header is checked, no more
                frames.append((i, k, f, None))
                break
            pieces, head = [], None
            # what the frame's blocks can decode to: a stored block its size, a compressed one at most 255 bytes per byte (a match-length
            # extension byte) and the frame's maximum; a linked frame's chain shares one slot of their sum -- one byte past the content
            # size where the header gives one, so that a longer content shows
            bounds = [size if stored else min(f.block_max, 255 * size) for stored, _, size, _ in f.blocks]
            chain_cap = sum(bounds)
            if f.content_size is not None:
                chain_cap = min(chain_cap, f.content_size + 1)
            if not f.independent and chain_cap >= 1 << 32:
                f.error = FrameTooLargeError(i, k, "a linked frame of up to %d bytes; one chain holds less than 4 GiB" % chain_cap)
                frames.append((i, k, f, None))
                break
            for bno, (stored, at, size, ck) in enumerate(f.blocks):
                if ck is not None:
                    hash_off.append(int(base_of[i]) + at); hash_len.append(size); hash_want.append(ck); hash_who.append((i, k, bno))
                if stored and f.independent:
                    pieces.append(("host", at, size))
                    continue
                j = len(in_off)
                if stored:
                    lb = _literal_block(blobs[i][at:at + size])
                    in_off.append(extra_base + len(extra)); in_len.append(len(lb))
                    extra += lb
                else:
                    in_off.append(int(base_of[i]) + at); in_len.append(size)
                if f.independent or head is None:
                    if dct:
                        dict_at.append(cur)
                        cur += len(dct)
                    cap = bounds[bno] if f.independent else chain_cap
                    link.append(0); dlen.append(len(dct)); out_off.append(cur); out_cap.append(cap)
                    cur += cap
                    if not f.independent:
                        head = j
                else:
                    link.append(1); dlen.append(0); out_off.append(0); out_cap.append(0)
                pieces.append(("dev", j, bno))
            frames.append((i, k, f, pieces))
    inbuf = np.frombuffer(b"".join(blobs) + bytes(extra) + b"\0" * 16, np.uint8)

    # header and block checksums
    herr = {}                                                          # (blob, frame) -> its first checksum error
    if hash_off:
        got = xxh32_many(inbuf, hash_off, hash_len, 0, ctx)
        for (i, k, bno), g, w in zip(hash_who, got, hash_want):
            if bno < 0 and ((int(g) >> 8) & 0xFF) != w:
                herr.setdefault((i, k), HeaderChecksumError(i, k, "%02x in the frame, %02x computed" % (w, (int(g) >> 8) & 0xFF)))
            elif bno >= 0 and int(g) != w:
                herr.setdefault((i, k), BlockChecksumError(i, k, "block %d" % bno))

    # every compressed block of every frame: one call
    n = len(in_off)
    out = np.zeros(cur + 16, np.uint8)
    if dct:
        d = np.frombuffer(dct, np.uint8)
        for at in dict_at:
            out[at:at + d.size] = d
    if n:
        res = ctx._batch("rcx_lz4_decode_linked_batch", inbuf, in_off, in_len, (out, out_off, out_cap), np.array(link, np.uint8), np.array(dlen, np.uint64),
                         unpack=False)
        out_len, status = res.out_len, res.status

    def head_of(j):
        while link[j]:
            j -= 1
        return j

    # contents: a linked frame's chain is contiguous behind its head; independent blocks sit in their own slots
    # (a blob's frames come in order: the first one that fails is the blob's result, and the frames behind it are not looked at)
    contents = {}
    for i, k, f, pieces in frames:
        if results[i] is not None:
            continue
        if (i, k) in herr or pieces is None:
            results[i] = herr.get((i, k)) or f.error
            continue
        parts, pos, bad = [], None, None
        for pc in pieces:
            if pc[0] == "host":
                parts.append(blobs[i][pc[1]:pc[1] + pc[2]])
                continue
            j, bno = pc[1], pc[2]
            if status[j] == N.E_OUTPUT_TOO_SMALL and not f.independent and f.content_size is not None and out_cap[head_of(j)] == f.content_size + 1:
                bad = ContentSizeError(i, k, "block %d takes the content past the %d bytes the frame says" % (bno, f.content_size))
                break
            if status[j] == N.E_OUTPUT_TOO_SMALL and f.independent and out_cap[j] == f.block_max:
                bad = BlockTooLargeError(i, k, "block %d decodes to more than the frame's maximum of %d bytes" % (bno, f.block_max))
                break
            if status[j] != 0:
                bad = BlockDataError(i, k, "block %d: %s" % (bno, N.lib().rcx_status_string(int(status[j])).decode()), int(status[j]))
                break
            ln = int(out_len[j])
            if ln > f.block_max:
                bad = BlockTooLargeError(i, k, "block %d decodes to %d bytes, the frame's maximum is %d" % (bno, ln, f.block_max))
                break
            if link[j] == 0:
                pos = out_off[j]
            parts.append(out[pos:pos + ln].tobytes())
            pos += ln
        if bad is not None:
            results[i] = bad
            continue
        content = b"".join(parts)
        if f.content_size is not None and f.content_size != len(content):
            results[i] = ContentSizeError(i, k, "%d bytes decoded, the frame says %d" % (len(content), f.content_size))
            continue
        contents[(i, k)] = content

    # content checksums: one call
    if verify:
        # (of every frame that decoded, also in front of a frame that failed: its checksum error would have come first)
        todo = [(i, k, f) for i, k, f, pc in frames if (i, k) in contents and f.content_checksum is not None]
        if todo:
            lens = [len(contents[(i, k)]) for i, k, _ in todo]
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if lens else []
            cat = np.frombuffer(b"".join(contents[(i, k)] for i, k, _ in todo) + b"\0", np.uint8)
            got = xxh32_many(cat, offs, lens, 0, ctx)
            for (i, k, f), g in zip(todo, got):
                if int(g) != f.content_checksum and (not isinstance(results[i], FrameError) or k < results[i].frame):
                    results[i] = (ContentChecksumError(i, k, "%08x in the frame, %08x computed" % (f.content_checksum, int(g))))

    for i in range(nb):
        if results[i] is None:
            results[i] = b"".join(contents[(i, k)] for k in range(len(parsed[i])))
    if not return_exceptions and any(isinstance(r, Exception) for r in results):
        raise FramesFailed(results)
    return results


# ---------------------------------------------------------------------------------------------------------------- encode
def _block_size_id(block_size):
    if block_size in BLOCK_MAX:
        return block_size
    for k, v in BLOCK_MAX.items():
        if v == block_size:
            return k
    raise ValueError("block_size must be 64 KiB, 256 KiB, 1 MiB or 4 MiB (or the format's id 4..7)")


def _encode_with_history(ctx, blobs, bmax, level, linked, dct):
    """Every block of every blob through ONE rcx_lz4_encode_hc_hist_batch call.  The staging buffer holds, linked: each frame as
    dictionary || blob, and block k's history is what lies in front of it there (the dictionary and the frame's bytes before it, at most
    64 KiB); independent blocks behind a dictionary: the dictionary in front of every block.  -> the blocks' LZ4 bytes, in order"""
    buf, off, lens, hist = bytearray(), [], [], []
    for blob in blobs:
        if linked:
            buf += dct
            start = len(buf)
            buf += blob
        for at in range(0, len(blob), bmax):
            n = min(bmax, len(blob) - at)
            if linked:
                off.append(start + at)
                hist.append(min(DICT_MAX, len(dct) + at))
            else:
                buf += dct
                off.append(len(buf))
                hist.append(len(dct))
                buf += blob[at:at + n]
            lens.append(n)
    if not off:
        return []
    base = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8)
    return ctx.lz4_encode_hc_hist(base, off, lens, hist, int(level)).check().outputs


def encode_frames(blobs, level=None, block_size=64 << 10, block_checksum=False, content_checksum=True, content_size=True, ctx=None,
                  linked=False, dictionary=None, dict_id=None):
    """One LZ4 frame per blob.  level=None: the greedy block encoder (rcx_lz4_encode_batch); 1..12: the high-compression one
    (rcx_lz4_encode_hc_batch).  A block that compression does not shrink is stored.  block_size: 64 KiB, 256 KiB, 1 MiB or 4 MiB (or
    the id 4..7).  The header checksum, the optional block checksums (of each block as written) and the optional content checksum
    come from rcx_xxh32_batch; the frame ends with one EndMark.  Every block of every blob is compressed by one call.

    linked=True writes block-linked frames (what the `lz4` tool writes by default): a block's matches reach up to 64 KiB back into the
        frame's earlier blocks -- also into a stored one's bytes.  All blocks are still encoded at once: history is input.
    dictionary: bytes whose last 64 KiB are the history in front of every frame's first block (linked) or of every block
        (independent); decode_frames and LZ4F_decompress_usingDict want the same bytes.  dict_id: written as the header's dictionary
        id when given.
    linked and dictionary need a level (rcx_lz4_encode_hc_hist_batch): the greedy encoder has no history."""
    ctx = ctx or _compress.context()
    bid = _block_size_id(block_size)
    bmax = BLOCK_MAX[bid]
    blobs = [bytes(b) for b in blobs]
    dct = bytes(dictionary)[-DICT_MAX:] if dictionary else b""
    if (linked or dct) and level is None:
        raise ValueError("linked blocks and dictionaries need the high-compression encoder: choose a level from 1 to 12")
    raws, owner = [], []
    for i, blob in enumerate(blobs):
        for at in range(0, len(blob), bmax):
            raws.append(blob[at:at + bmax])
            owner.append(i)
    if linked or dct:
        comp = _encode_with_history(ctx, blobs, bmax, level, linked, dct)
    elif raws:
        res = (ctx.lz4_encode_blocks(raws) if level is None else ctx.lz4_encode_hc_blocks(raws, int(level))).check()
        comp = res.outputs
    else:
        comp = []
    written = [(False, c) if len(c) < len(r) else (True, r) for r, c in zip(raws, comp)]
    # descriptors first: their checksums, the blocks' and the contents' go through one call
    descs = []
    for blob in blobs:
        flg = 0x40 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | (8 if content_size else 0) | (4 if content_checksum else 0) \
            | (1 if dict_id is not None else 0)
        descs.append(bytes([flg, bid << 4]) + (struct.pack("<Q", len(blob)) if content_size else b"")
                     + (struct.pack("<I", dict_id) if dict_id is not None else b""))
    regions = list(descs)
    if block_checksum:
        regions += [w[1] for w in written]
    if content_checksum:
        regions += blobs
    lens = [len(r) for r in regions]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if lens else []
    hashes = xxh32_many(np.frombuffer(b"".join(regions) + b"\0", np.uint8), offs, lens, 0, ctx)
    nb = len(blobs)
    bh = hashes[nb:nb + len(written)] if block_checksum else None
    ch = hashes[len(hashes) - nb:] if content_checksum else None
    outs = [bytearray(struct.pack("<I", MAGIC) + descs[i] + bytes([(int(hashes[i]) >> 8) & 0xFF])) for i in range(nb)]
    for j, (stored, payload) in enumerate(written):
        o = outs[owner[j]]
        o += struct.pack("<I", len(payload) | (0x80000000 if stored else 0)) + payload
        if block_checksum:
            o += struct.pack("<I", int(bh[j]))
    for i in range(nb):
        outs[i] += struct.pack("<I", 0)
        if content_checksum:
            outs[i] += struct.pack("<I", int(ch[i]))
    return [bytes(o) for o in outs]


# ---------------------------------------------------------------------------------------------------------------- stream classes
class Decoder(_compress._BufferedDecoder):
    """Reads standard LZ4 frames from `r` (every frame up to the reader's end, their contents back to back): read(n), read_to_end(),
    eof(), finish() as the decoders of compress.py.  Raises the FrameError of the first frame that fails."""

    def __init__(self, r, dictionary=None, verify=True):
        _compress._BufferedDecoder.__init__(self, r)
        self._dictionary, self._verify = dictionary, verify

    def _decode_all(self, raw):
        res = decode_frames([raw], self._dictionary, self._verify, return_exceptions=True)[0]
        if isinstance(res, Exception):
            raise res
        return res


class Encoder:
    """Collects what is written and, at finish(), writes it to `w` as one standard LZ4 frame (encode_frames' options) -> w."""

    def __init__(self, w, level=None, block_size=64 << 10, block_checksum=False, content_checksum=True, content_size=True,
                 linked=False, dictionary=None, dict_id=None):
        self.w = w
        self._buf = bytearray()
        self._opts = dict(level=level, block_size=block_size, block_checksum=block_checksum, content_checksum=content_checksum, content_size=content_size,
                          linked=linked, dictionary=dictionary, dict_id=dict_id)
        if (linked or dictionary) and level is None:
            raise ValueError("linked blocks and dictionaries need the high-compression encoder: choose a level from 1 to 12")

    def write(self, buf):
        self._buf += buf
        return len(buf)

    def flush(self):
        pass

    def finish(self):
        self.w.write(encode_frames([bytes(self._buf)], **self._opts)[0])
        self._buf = bytearray()
        return self.w
