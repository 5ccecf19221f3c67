//! RFC 1951 decoder (reference: src/flate.rs:164-193, 453-488).  Batch semantics: the stream is decoded to BFINAL in one
//! call; `flags & RCX_W_EMPTY_BLOCK_MIDSTREAM` reports the reference's `Ok(0)` quirk (:474-476) instead of acting it out.
use crate::rcx_sys::*;
use crate::{decode_many_with, grow_decode, run_batch, Buffered, TailReader};
use std::io::{self, Read, Write};
use std::os::raw::c_int;

pub struct Decoder<R: Read> {
    /// `pub r: R` (flate.rs:166), left exactly after the DEFLATE stream once it is decoded (:250-260 reads byte by byte)
    pub r: TailReader<R>,
    buf: Buffered,
    pub flags: u32,
}

impl<R: Read> Decoder<R> {
    pub fn new(r: R) -> Decoder<R> {
        Decoder { r: TailReader::new(r), buf: Buffered::new(), flags: 0 }
    }
    /// :453-458: the final block has been served completely
    pub fn eof(&mut self) -> bool {
        self.buf.eof()
    }
    /// :460-465
    pub fn reset(&mut self) {
        self.buf.reset()
    }
}

impl<R: Read> Read for Decoder<R> {
    fn read(&mut self, dst: &mut [u8]) -> io::Result<usize> {
        let flags = &mut self.flags;
        self.buf.ensure(&mut self.r, |raw| {
            let r = grow_decode(raw, 4 * raw.len() as u64, |c, b, f| unsafe { rcx_inflate_batch(c, b, f) })?;
            *flags = r.aux[0];
            Ok((r.out[0].clone(), Some(r.in_used[0] as usize)))
        })?;
        Ok(self.buf.serve(dst))
    }
}

/// Many raw DEFLATE streams through ONE batch call (the reference decodes one deflate block per `read()`, flate.rs:468-488: on the
/// GPU a stream is one wave's work, so a caller with many streams hands them over together).  -> per stream (decoded bytes, input
/// bytes used, flags); the first stream that fails returns what its `Decoder` would.
pub fn decode_many(streams: &[&[u8]]) -> io::Result<Vec<(Vec<u8>, usize, u32)>> {
    decode_many_with(streams, |c, b, f| unsafe { rcx_inflate_batch(c, b, f) })
}

/// Extension (the reference has no DEFLATE encoder): the whole input as ONE stream.  `write` only buffers -- there is no incremental
/// state across calls -- and `finish` encodes everything in one batch call, writes it to `w` and returns the writer.
pub struct Encoder<W: Write> {
    w: W,
    buf: Vec<u8>,
    level: u32,
}

impl<W: Write> Encoder<W> {
    pub fn new(w: W) -> Encoder<W> {
        Encoder { w, buf: Vec::new(), level: 0 }
    }
    /// Extension: compression level 1..9 (`rcx_deflate_encode_level_batch`; 1 makes the bytes of `new`).  Panics on a level outside 1..9.
    pub fn with_level(w: W, level: u32) -> Encoder<W> {
        assert!((1..=9).contains(&level), "deflate level must be 1..9");
        Encoder { level, ..Encoder::new(w) }
    }
    pub fn finish(mut self) -> (W, io::Result<()>) {
        let cap = unsafe { rcx_deflate_compression_bound(self.buf.len() as u64) };
        let level = self.level as c_int;
        let r = run_batch(&[&self.buf[..]], &[cap], |c, b, _| unsafe {
            if level == 0 { rcx_deflate_encode_batch(c, b) } else { rcx_deflate_encode_level_batch(c, b, level) }
        })
        .check();
        let res = match r {
            Ok(r) => self.w.write_all(&r.out[0]),
            Err(e) => Err(e),
        };
        (self.w, res)
    }
}

impl<W: Write> Write for Encoder<W> {
    fn write(&mut self, buf: &[u8]) -> io::Result<usize> {
        self.buf.extend_from_slice(buf);
        Ok(buf.len())
    }
    fn flush(&mut self) -> io::Result<()> {
        Ok(())
    }
}
