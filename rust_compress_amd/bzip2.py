"""bzip2 files (.bz2) as bzip2 / libbz2 write and read them, MANY FILES PER CALL.

    decode_many(blobs)   every block of every file through rcx_bzip2_decode_batch: a scan for the block marks, one wave per block for the
                         Huffman / MTF stage, the inverse BWT, the run-length undo and the CRCs, all on the device.  Two calls: the
                         first with capacities of 0 returns the exact sizes (and every error), the second decodes into them
    Decoder(r)           the buffered stream class in the style of compress.py: every stream up to the reader's end or up to the
                         first bytes that are no stream header, which go back to the reader

    encode_many(datas)   every file as one stream through rcx_bzip2_encode_batch: the run-length step, a suffix sort of every block
                         doubled, MTF, the table fit and the bit packing, all on the device.  One call with capacities of
                         n + n / 64 + 1024, one retry for the files that report a larger size
    Encoder(w)           the buffering stream class in the style of compress.py's DEFLATE encoders: one stream at finish()

A file that is read is one or more concatenated streams; bytes behind the last stream that do not begin with BZh1..BZh9 are left alone.
A file that is written is one stream whose bytes are those of the specification in DESIGN.md 3.21, not libbz2's (every bzip2 reader
reads them).  There is no CPU path."""
from . import _native as N
from . import compress as _compress
from .compress import CompressError


class Bzip2Error(CompressError):
    """A file that cannot be decoded.  index: the blob's position in the batch; what: one word for the check that failed."""
    what = "bzip2"

    def __init__(self, index, status):
        self.index = index
        CompressError.__init__(self, status, "bzip2 file %d: %s (%s)" % (index, self.what.replace("_", " "), N.lib().rcx_status_string(int(status)).decode()))


class MagicError(Bzip2Error):              # the first 4 bytes are not BZh1..BZh9
    what = "magic"


class DataError(Bzip2Error):               # a malformed block or stream structure
    what = "data"


class BlockChecksumError(Bzip2Error):
    what = "block_checksum"


class StreamChecksumError(Bzip2Error):
    what = "stream_checksum"


class RandomisedError(Bzip2Error):         # the obsolete randomised bit: not supported
    what = "randomised"


class TruncatedError(Bzip2Error):          # the input ends inside a stream
    what = "truncated"


_BY_STATUS = {N.E_BZ2_MAGIC: MagicError, N.E_BZ2_DATA: DataError, N.E_BZ2_BLOCK_CRC: BlockChecksumError, N.E_BZ2_STREAM_CRC: StreamChecksumError,
              N.E_BZ2_RANDOMISED: RandomisedError, N.E_EOF: TruncatedError}


class FilesFailed(CompressError):
    """decode_many without return_exceptions: results holds every file's bytes or its Bzip2Error"""

    def __init__(self, results):
        self.results = results
        first = next(r for r in results if isinstance(r, Exception))
        CompressError.__init__(self, first.status, str(first))


def _error(index, status):
    return _BY_STATUS.get(int(status), Bzip2Error)(index, int(status))


def decode_many(blobs, ctx=None, return_exceptions=False, with_used=False):
    """-> the decoded bytes of every file (with_used: (bytes, bytes consumed) pairs).  A file that fails raises FilesFailed, or, with
    return_exceptions, has its typed Bzip2Error in its place."""
    ctx = ctx or _compress.context()
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    if n == 0:
        return []
    got = _compress._exact_retry(lambda idx, caps: ctx.bzip2_decode([blobs[i] for i in idx], caps), [0] * n)      # (capacities of 0: a size query)
    results = [_error(i, st) if st else ((out, used) if with_used else out) for i, (st, out, used) in enumerate(got)]
    if not return_exceptions and any(isinstance(r, Exception) for r in results):
        raise FilesFailed(results)
    return results


class Decoder(_compress._BufferedDecoder):
    """Reads a .bz2 file from `r`: read(n), read_to_end(), eof(), finish() as the decoders of compress.py.  Raises the Bzip2Error of
    the first stream that fails; bytes behind the last stream go back to the reader."""

    def _decode_all(self, raw):
        res = decode_many([raw], return_exceptions=True, with_used=True)[0]
        if isinstance(res, Exception):
            raise res
        self.consumed = res[1]
        return res[0]


def _level(level):
    if not 1 <= int(level) <= 9:
        raise ValueError("bzip2 level must be 1..9")
    return int(level)


def encode_many(datas, level=9, ctx=None):
    """-> one .bz2 stream per input, at level 1..9 (blocks of 100 000 x level bytes).  There is no bound to size the slots with: the first
    call offers n + n / 64 + 1024 bytes each, and a file that needs more says how much and is encoded again."""
    level = _level(level)
    ctx = ctx or _compress.context()
    datas = [bytes(d) for d in datas]
    if not datas:
        return []
    def check(i, st, but=0):
        if st and st != but:
            raise CompressError(st, "bzip2 file %d: %s" % (i, N.lib().rcx_status_string(st).decode()))

    def call(idx, caps):
        res = ctx.bzip2_encode([datas[i] for i in idx], caps, level)
        for i, st in zip(idx, res.status):                  # a file that fails ends it at once: nothing is encoded again for the others
            check(i, int(st), but=N.E_OUTPUT_TOO_SMALL)
        return res
    got = _compress._exact_retry(call, [len(d) + len(d) // 64 + 1024 for d in datas])
    for i, (st, _, _) in enumerate(got):
        check(i, st)
    return [out for _, out, _ in got]


class Encoder:
    """Writes a .bz2 file to `w`.  Shaped like compress.py's DEFLATE encoders: write() only buffers, and finish() encodes everything as
    ONE stream in one batch call, writes it to the writer and returns the writer.  level: 1..9; anything else raises ValueError."""

    def __init__(self, w, level=9):
        self.w = w
        self.buf = bytearray()
        self.level = _level(level)

    def write(self, buf):
        self.buf += bytes(buf)
        return len(buf)

    def flush(self):
        pass

    def finish(self):
        out = encode_many([bytes(self.buf)], self.level)[0]
        self.buf = bytearray()
        self.w.write(out)
        return self.w
