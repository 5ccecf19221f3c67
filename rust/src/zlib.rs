//! RFC 1950 decoder (reference: src/zlib.rs:32-127): CMF/FLG checks, DEFLATE, Adler-32 trailer -- all on the device.
use crate::rcx_sys::*;
use crate::{decode_many_with, grow_decode, run_batch, Buffered, TailReader};
use std::io::{self, Read, Write};
use std::os::raw::c_int;

pub struct Decoder<R: Read> {
    r: TailReader<R>,
    buf: Buffered,
}

impl<R: Read> Decoder<R> {
    /// zlib.rs:42-49
    pub fn new(r: R) -> Decoder<R> {
        Decoder { r: TailReader::new(r), buf: Buffered::new() }
    }
    /// zlib.rs:51-53: the reader, positioned exactly after the 4-byte Adler-32 trailer
    pub fn unwrap(self) -> TailReader<R> {
        self.r
    }
}

impl<R: Read> Read for Decoder<R> {
    fn read(&mut self, dst: &mut [u8]) -> io::Result<usize> {
        self.buf.ensure(&mut self.r, |raw| {
            let r = grow_decode(raw, 4 * raw.len() as u64, |c, b, f| unsafe { rcx_zlib_decode_batch(c, b, f) })?;
            Ok((r.out[0].clone(), Some(r.in_used[0] as usize)))
        })?;
        Ok(self.buf.serve(dst))
    }
}

/// Many zlib members through ONE batch call, every member's Adler-32 checked on the device.  -> per member (decoded bytes, input
/// bytes used); the first member that fails returns what its `Decoder` would.
pub fn decode_many(members: &[&[u8]]) -> io::Result<Vec<(Vec<u8>, usize)>> {
    Ok(decode_many_with(members, |c, b, f| unsafe { rcx_zlib_decode_batch(c, b, f) })?.into_iter().map(|(o, u, _)| (o, u)).collect())
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
    /// Extension: compression level 1..9 (`rcx_zlib_encode_level_batch`; 1 makes the bytes of `new`).  Panics on a level outside 1..9.
    pub fn with_level(w: W, level: u32) -> Encoder<W> {
        assert!((1..=9).contains(&level), "deflate level must be 1..9");
        Encoder { level, ..Encoder::new(w) }
    }
    pub fn finish(mut self) -> (W, io::Result<()>) {
        let cap = unsafe { rcx_deflate_compression_bound(self.buf.len() as u64) } + 6;
        let level = self.level as c_int;
        let r = run_batch(&[&self.buf[..]], &[cap], |c, b, _| unsafe {
            if level == 0 { rcx_zlib_encode_batch(c, b) } else { rcx_zlib_encode_level_batch(c, b, level) }
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
