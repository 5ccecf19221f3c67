"""rust_compress_amd -- MI355X-native (gfx950) block-codec engine behind the `compress::*` hot path.

Only what the path needs lives here: csrc/ (HIP kernels + the C-ABI of include/rcx.h), the ctypes
binding, the batch API, the stream-codec mirror of the reference interface (compress.py), the standard
LZ4 frame codec (lz4frame.py), the bzip2 reader and writer (bzip2.py), the Zstandard reader (zstd.py) and the synthetic data generators.  There is no CPU fallback: the HIP library must be built and a GPU present.
"""
from . import _native  # noqa: F401
from .api import BlockError, Context, DeviceBatch, RcxError, Result  # noqa: F401
from . import lz4frame  # noqa: F401
from . import bzip2  # noqa: F401
from . import zstd  # noqa: F401

__all__ = ["Context", "DeviceBatch", "Result", "BlockError", "RcxError", "lz4frame", "bzip2", "zstd"]
