"""Zstandard files (.zst) as zstd / libzstd write them (RFC 8878), MANY FILES PER CALL.  Reading only.

    decode_many(blobs)   every file through rcx_zstd_decode_batch: one wave per file takes its frames and blocks in order -- FSE and
                         Huffman tables, literals, sequences, the copies -- on the device.  Two calls at the most: the first with the
                         capacities the frame headers declare (0 for a file with a frame that declares none), the second for the
                         files that reported a size
    Decoder(r)           the buffered stream class in the style of compress.py: every frame up to the reader's end or up to the first
                         bytes that are no frame, which go back to the reader

A file is one or more concatenated frames; skippable frames are skipped; bytes behind the last frame that are no magic are left alone.
dictionary: raw content (what train_dictionary returns), history in front of every frame.  A frame that names a Dictionary_ID needs a
formatted dictionary, which is not supported.  There is no CPU path."""
from . import _native as N
from . import compress as _compress
from .api import _per_blob
from .compress import CompressError

MAGIC = 0xFD2FB528


class ZstdError(CompressError):
    """A file that cannot be decoded.  index: the blob's position in the batch; what: one word for the check that failed."""
    what = "zstd"

    def __init__(self, index, status):
        self.index = index
        CompressError.__init__(self, status, "zstd file %d: %s (%s)" % (index, self.what.replace("_", " "), N.lib().rcx_status_string(int(status)).decode()))


class MagicError(ZstdError):               # the first 4 bytes are no frame
    what = "magic"


class HeaderError(ZstdError):              # a reserved header bit, a window beyond 2^31
    what = "header"


class DataError(ZstdError):                # everything else the format calls corrupt
    what = "data"


class ChecksumError(ZstdError):
    what = "checksum"


class DictionaryError(ZstdError):          # the frame names a Dictionary_ID: a formatted dictionary is needed
    what = "dictionary"


class TruncatedError(ZstdError):           # the input ends inside a frame
    what = "truncated"


_BY_STATUS = {N.E_ZSTD_MAGIC: MagicError, N.E_ZSTD_HEADER: HeaderError, N.E_ZSTD_DATA: DataError, N.E_ZSTD_CHECKSUM: ChecksumError,
              N.E_ZSTD_DICT: DictionaryError, N.E_EOF: TruncatedError}


class FilesFailed(CompressError):
    """decode_many without return_exceptions: results holds every file's bytes or its ZstdError"""

    def __init__(self, results):
        self.results = results
        first = next(r for r in results if isinstance(r, Exception))
        CompressError.__init__(self, first.status, str(first))


def _error(index, status):
    return _BY_STATUS.get(int(status), ZstdError)(index, int(status))


def declared_size(blob):
    """-> the sum of the Frame_Content_Size fields of the file's frames, found by a walk over the frame and block headers alone, or
    None where a frame declares no size, the sum is 4 GiB or more, or the walk runs into something it cannot read (the call will say
    what)."""
    b = bytes(blob)
    pos, total, frames = 0, 0, 0
    while len(b) - pos >= 4:
        magic = int.from_bytes(b[pos:pos + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if len(b) - pos < 8:
                return None
            pos += 8 + int.from_bytes(b[pos + 4:pos + 8], "little")
            frames += 1
            continue
        if magic != MAGIC:
            break
        if len(b) - pos < 5:
            return None
        fhd = b[pos + 4]
        single, fcsf, didf = (fhd >> 5) & 1, fhd >> 6, fhd & 3
        at = pos + 5 + (0 if single else 1) + (4 if didf == 3 else didf)
        size = (1 if single else 0) if fcsf == 0 else (2, 4, 8)[fcsf - 1]
        if not size or len(b) < at + size:
            return None
        total += int.from_bytes(b[at:at + size], "little") + (256 if size == 2 else 0)
        pos = at + size
        while True:
            if len(b) - pos < 3:
                return None
            bh = int.from_bytes(b[pos:pos + 3], "little")
            pos += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
            if bh & 1:
                break
        pos += 4 if fhd & 4 else 0
        frames += 1
    return total if frames and total < (1 << 32) else None


def decode_many(blobs, dictionary=None, ctx=None, return_exceptions=False, with_used=False):
    """-> the decoded bytes of every file (with_used: (bytes, bytes consumed) pairs).  A file that fails raises FilesFailed, or, with
    return_exceptions, has its typed ZstdError in its place."""
    ctx = ctx or _compress.context()
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    if n == 0:
        return []
    dicts = None if dictionary is None else _per_blob(dictionary, n)
    # a declared size is taken for the first call's slot only where it is plausible for the file's length (an RLE block makes 2 MiB of
    # 4 bytes, a match 64 KiB of a few bits: 64 MiB or 1024 times the file, whichever is more); beyond that the call sizes the file
    # itself, so a few hostile bytes cannot ask for a slot of 4 GiB before anything has been checked
    def first_cap(b):
        size = declared_size(b) or 0
        return size if size <= max(64 << 20, 1024 * len(b)) else 0
    got = _compress._exact_retry(lambda idx, caps: ctx.zstd_decode([blobs[i] for i in idx], caps, dicts and [dicts[i] for i in idx]),
                                 [first_cap(b) for b in blobs])
    results = [_error(i, st) if st else ((out, used) if with_used else out) for i, (st, out, used) in enumerate(got)]
    if not return_exceptions and any(isinstance(r, Exception) for r in results):
        raise FilesFailed(results)
    return results


class Decoder(_compress._BufferedDecoder):
    """Reads a .zst file from `r`: read(n), read_to_end(), eof(), finish() as the decoders of compress.py.  Raises the ZstdError of
    the first frame that fails; bytes behind the last frame go back to the reader."""

    def __init__(self, r, dictionary=None):
        _compress._BufferedDecoder.__init__(self, r)
        self.dictionary = dictionary

    def _decode_all(self, raw):
        res = decode_many([raw], self.dictionary, return_exceptions=True, with_used=True)[0]
        if isinstance(res, Exception):
            raise res
        self.consumed = res[1]
        return res[0]
