// compress.hpp -- C++17 host-side mirror of the reference crate's per-algorithm Reader/Writer surface
// (`compress::*`, rusty-shell/rust-compress) over the batch C-ABI of include/rcx.h.
//
// The reference is Rust and no Rust toolchain exists in this image, so the host side above the C-ABI is
// written in C++ with the SAME names, argument meaning and error behaviour (INTEGRATION.md shows the Rust
// binding a maintainer would add).  A reader R is anything with `size_t read(uint8_t* dst, size_t n)`
// (returns 0 at end of stream, like std::io::Read); a writer W anything with `void write(const uint8_t*,
// size_t)`.  Decoders buffer their whole input, parse the framing on the host and make ONE batch FFI call
// per stream; `read()` then serves the decoded bytes in whatever chunk sizes the caller asks for.
//
//   compress::lz4::{Decoder,Encoder,decode_block,encode_block,compression_bound}   src/lz4.rs
//   compress::flate::Decoder, compress::zlib::Decoder, compress::Adler32           src/flate.rs, zlib.rs, adler.rs
//   compress::flate::Encoder, compress::zlib::Encoder (extension: the reference has no DEFLATE encoder)
//   compress::bwt::{Encoder,Decoder,encode_simple,decode_simple}, bwt::mtf, bwt::dc src/bwt/*.rs
//   compress::entropy::ari::{ByteEncoder,ByteDecoder}                              src/entropy/ari/table.rs
//   compress::entropy::ari::{RangeEncoder,Model,Encoder,Decoder,table,bin,apm}     src/entropy/ari/*.rs (ari_symbol.hpp)
//   compress::rle::{Encoder,Decoder}                                               src/rle.rs
#pragma once
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rcx.h"
#include "ari_symbol.hpp"     // entropy::ari::{RangeEncoder, Model, Encoder, Decoder, table, bin, apm}: the per-symbol surface, host code

namespace compress {
namespace detail { constexpr uint64_t MAX_BLOCK = 0xFFFFFFFFull; }    // the kernels index a block with 32 bits (run_batch rejects a larger slot)

enum class ErrorKind { InvalidInput, UnexpectedEof, Other, Panic };

struct io_error : std::runtime_error {          // std::io::Error
    ErrorKind kind; int status;
    io_error(ErrorKind k, int st, const std::string& m) : std::runtime_error(m), kind(k), status(st) {}
};

inline void raise_status(int st)
{
    if (st == RCX_OK) return;
    const std::string msg = rcx_status_string(st);
    if (st == RCX_E_EOF) throw io_error(ErrorKind::UnexpectedEof, st, msg);
    if (st == RCX_E_MALFORMED || st == RCX_E_OUTPUT_TOO_SMALL) throw io_error(ErrorKind::Panic, st, msg);
    if (st == RCX_E_RLE_LONG_RUN) throw io_error(ErrorKind::Other, st, msg);
    throw io_error(ErrorKind::InvalidInput, st, msg);
}

// ---- plumbing --------------------------------------------------------------------------------------
class Context {                                   // one rcx_ctx; no CPU fallback: throws without a GPU
public:
    explicit Context(int device = -1)
    {
        const int rc = rcx_ctx_create(device, &h_);
        if (rc != RCX_RC_OK) throw std::runtime_error("rcx_ctx_create failed (no HIP device? there is no CPU fallback)");
    }
    ~Context() { rcx_ctx_destroy(h_); }
    Context(const Context&) = delete;
    rcx_ctx* get() const { return h_; }
    static Context& global() { static Context c; return c; }
private:
    rcx_ctx* h_ = nullptr;
};

struct BatchResult {
    std::vector<std::vector<uint8_t>> out;
    std::vector<uint64_t> in_used;
    std::vector<int32_t> status;
    std::vector<uint32_t> aux;
};

// Pack blobs into one host buffer, call a batch entry point, unpack.  `call` gets (ctx, &batch).
template <class Call>
BatchResult run_batch(const std::vector<std::vector<uint8_t>>& blobs, const std::vector<uint64_t>& caps, Call call)
{
    const uint32_t n = (uint32_t)blobs.size();
    std::vector<uint64_t> in_off(n), in_len(n), out_off(n), out_cap(n), out_len(n), in_used(n);
    std::vector<int32_t> status(n);
    uint64_t it = 0, ot = 0;
    for (uint32_t i = 0; i < n; i++) {
        in_off[i] = it; in_len[i] = blobs[i].size(); it += (blobs[i].size() + 15) & ~15ull;
        out_off[i] = ot; out_cap[i] = caps[i]; ot += (caps[i] + 15) & ~15ull;
    }
    std::vector<uint8_t> in(it + 16), out(ot + 16);
    for (uint32_t i = 0; i < n; i++) if (!blobs[i].empty()) std::memcpy(in.data() + in_off[i], blobs[i].data(), blobs[i].size());
    rcx_batch b{in.data(), in_off.data(), in_len.data(), out.data(), out_off.data(), out_cap.data(), out_len.data(),
                in_used.data(), status.data(), n, RCX_MEM_HOST};
    BatchResult r;
    r.aux.assign(n, 0);
    const int rc = call(Context::global().get(), &b, r.aux.data());
    if (rc != RCX_RC_OK) throw std::runtime_error(std::string("rcx batch call failed: ") + rcx_last_error(Context::global().get()));
    r.out.resize(n);
    for (uint32_t i = 0; i < n; i++) r.out[i].assign(out.begin() + out_off[i], out.begin() + out_off[i] + out_len[i]);
    r.in_used = in_used; r.status = status;
    return r;
}
inline void check(const BatchResult& r) { for (int st : r.status) raise_status(st); }

// ---- more than one GPU from a host that is not Python -----------------------------------------------------------------
// Blocks are independent in every codec (lz4.rs:445-456, bwt/mod.rs:373-401, ari/test.rs:52-89), so a batch shards by
// contiguous block ranges balanced by output bytes -- the partition of rust_compress_amd/dist.py -- and needs no collective:
// one rcx_ctx per device (a context binds one device, include/rcx.h), one host thread per context (a context is
// thread-compatible, not thread-safe), every range staged to and from its own GPU by the library's host-memory path.
// `devices` may name a device more than once (two ranges on one GPU); the result is block for block what run_batch returns.
inline std::vector<size_t> partition(const std::vector<uint64_t>& weights, size_t parts)
{
    std::vector<size_t> bounds(parts + 1, weights.size());
    bounds[0] = 0;
    long double total = 0, run = 0;
    for (uint64_t w : weights) total += (long double)w;
    size_t g = 1;
    for (size_t i = 0; i < weights.size() && g < parts; i++) {
        while (g < parts && run >= total * g / parts) bounds[g++] = i;
        run += (long double)weights[i];
    }
    return bounds;
}
template <class Call>
BatchResult run_batch_devices(const std::vector<int>& devices, const std::vector<std::vector<uint8_t>>& blobs, const std::vector<uint64_t>& caps, Call call)
{
    const size_t G = devices.size(), n = blobs.size();
    if (G == 0) throw std::runtime_error("run_batch_devices: no device");
    const std::vector<size_t> bounds = partition(caps, G);
    std::vector<BatchResult> part(G);
    std::vector<std::string> err(G);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++)
        th.emplace_back([&, g] {
            try {
                const size_t a = bounds[g], b = bounds[g + 1];
                if (a == b) return;
                Context ctx(devices[g]);
                const uint32_t m = (uint32_t)(b - a);
                std::vector<uint64_t> in_off(m), in_len(m), out_off(m), out_cap(m), out_len(m), in_used(m);
                std::vector<int32_t> status(m);
                uint64_t it = 0, ot = 0;
                for (uint32_t i = 0; i < m; i++) {
                    in_off[i] = it; in_len[i] = blobs[a + i].size(); it += (blobs[a + i].size() + 15) & ~15ull;
                    out_off[i] = ot; out_cap[i] = caps[a + i]; ot += (caps[a + i] + 15) & ~15ull;
                }
                std::vector<uint8_t> in(it + 16), out(ot + 16);
                for (uint32_t i = 0; i < m; i++) if (!blobs[a + i].empty()) std::memcpy(in.data() + in_off[i], blobs[a + i].data(), blobs[a + i].size());
                rcx_batch bt{in.data(), in_off.data(), in_len.data(), out.data(), out_off.data(), out_cap.data(), out_len.data(), in_used.data(), status.data(), m, RCX_MEM_HOST};
                BatchResult& r = part[g];
                r.aux.assign(m, 0);
                if (call(ctx.get(), &bt, r.aux.data()) != RCX_RC_OK) { err[g] = std::string("rcx batch call failed: ") + rcx_last_error(ctx.get()); return; }
                r.out.resize(m);
                for (uint32_t i = 0; i < m; i++) r.out[i].assign(out.begin() + out_off[i], out.begin() + out_off[i] + out_len[i]);
                r.in_used = in_used; r.status = status;
            } catch (const std::exception& e) { err[g] = e.what(); }
        });
    for (auto& t : th) t.join();
    BatchResult all;
    for (size_t g = 0; g < G; g++) {
        if (!err[g].empty()) throw std::runtime_error("device " + std::to_string(devices[g]) + ": " + err[g]);
        all.out.insert(all.out.end(), part[g].out.begin(), part[g].out.end());
        all.in_used.insert(all.in_used.end(), part[g].in_used.begin(), part[g].in_used.end());
        all.status.insert(all.status.end(), part[g].status.begin(), part[g].status.end());
        all.aux.insert(all.aux.end(), part[g].aux.begin(), part[g].aux.end());
    }
    if (all.out.size() != n) throw std::runtime_error("run_batch_devices: lost blocks");
    return all;
}

struct SliceReader {                              // BufReader::new(&[u8])
    const uint8_t* p; size_t n, pos = 0;
    SliceReader(const uint8_t* d, size_t len) : p(d), n(len) {}
    explicit SliceReader(const std::vector<uint8_t>& v) : p(v.data()), n(v.size()) {}
    size_t read(uint8_t* dst, size_t k) { k = k < n - pos ? k : n - pos; std::memcpy(dst, p + pos, k); pos += k; return k; }
};
struct VecWriter {                                // BufWriter::new(Vec::new())
    std::vector<uint8_t> v;
    void write(const uint8_t* d, size_t n) { v.insert(v.end(), d, d + n); }
};
// A reader that takes bytes back.  The batch decoders read ahead (a stream's end is only known once it is decoded); the
// reference's decoders stop reading exactly at the end of their stream (flate.rs:250-260, ari/mod.rs:289-292) and its tests
// rely on it (ari/test.rs:52-89).  Every Decoder keeps its reader as TailReader<R> `r` and hands the bytes behind its stream
// back, so `decoder.r` / finish() / unwrap() is a reader positioned exactly after the stream.
template <class R>
struct TailReader {
    R inner; std::vector<uint8_t> tail; size_t tpos = 0;
    explicit TailReader(R r) : inner(std::move(r)) {}
    size_t read(uint8_t* dst, size_t n)
    {
        size_t k = 0;
        if (tpos < tail.size()) { k = n < tail.size() - tpos ? n : tail.size() - tpos; std::memcpy(dst, tail.data() + tpos, k); tpos += k; }
        if (k < n) k += inner.read(dst + k, n - k);
        return k;
    }
    void unread(const uint8_t* p, size_t n)
    {
        if (!n) return;
        std::vector<uint8_t> t(p, p + n);
        t.insert(t.end(), tail.begin() + tpos, tail.end());
        tail.swap(t); tpos = 0;
    }
};
template <class R> std::vector<uint8_t> read_all(R& r)
{
    std::vector<uint8_t> v; uint8_t buf[65536]; size_t k;
    while ((k = r.read(buf, sizeof buf)) != 0) v.insert(v.end(), buf, buf + k);
    return v;
}
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }

// common part of every buffered decoder: decode everything on first read, then serve chunks
template <class R, class Derived>
class BufferedDecoder {
public:
    TailReader<R> r;                              // `pub r: R`, left exactly after the stream once it is decoded
    explicit BufferedDecoder(R rd) : r(std::move(rd)) {}
    size_t read(uint8_t* dst, size_t n)
    {
        ensure();
        const size_t k = n < out_.size() - pos_ ? n : out_.size() - pos_;
        std::memcpy(dst, out_.data() + pos_, k);
        pos_ += k;
        return k;
    }
    std::vector<uint8_t> read_to_end() { ensure(); std::vector<uint8_t> v(out_.begin() + pos_, out_.end()); pos_ = out_.size(); return v; }
    bool eof() { ensure(); return pos_ == out_.size(); }
    void reset() { done_ = false; out_.clear(); pos_ = 0; }
    static constexpr size_t TO_EOF = ~(size_t)0;
    size_t consumed = TO_EOF;                     // input bytes this stream used (in_used); TO_EOF: the format runs to the reader's end
    TailReader<R>& finish() { ensure(); return r; }   // the reader, positioned exactly after this stream
    TailReader<R>& unwrap() { return finish(); }
protected:
    void ensure()
    {
        if (done_) return;
        consumed = TO_EOF;
        raw_ = read_all(r); out_ = static_cast<Derived*>(this)->decode_all(raw_); pos_ = 0; done_ = true;
        if (consumed != TO_EOF && consumed < raw_.size()) { r.unread(raw_.data() + consumed, raw_.size() - consumed); raw_.resize(consumed); }
    }
    std::vector<uint8_t> raw_, out_; size_t pos_ = 0; bool done_ = false;
};

// ---- lz4 ---------------------------------------------------------------------------------------------
namespace lz4 {
inline std::optional<uint32_t> compression_bound(uint32_t size)                      // lz4.rs:175-181
{
    const uint64_t v = rcx_lz4_compression_bound(size);
    return v ? std::optional<uint32_t>((uint32_t)v) : std::nullopt;
}
inline size_t decode_block(const std::vector<uint8_t>& input, std::vector<uint8_t>& output)   // lz4.rs:602-611
{
    // the reference grows its Vec as the block decodes (:148-161): slots grow 8x until the block fits (a kernel stops at a full
    // slot, so the failed attempts together cost a seventh of the one that fits)
    // (the last attempt is the largest slot a block may have, 2^32 - 1 bytes: past it the block's own status is the answer)
    for (uint64_t cap = std::min<uint64_t>(detail::MAX_BLOCK, std::max<uint64_t>(1u << 16, 8 * input.size()));; cap = std::min<uint64_t>(cap * 8, detail::MAX_BLOCK)) {
        auto r = run_batch({input}, {cap}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_lz4_decode_batch(c, b); });
        if (r.status[0] == RCX_E_OUTPUT_TOO_SMALL && cap < detail::MAX_BLOCK) continue;
        check(r);
        output.insert(output.end(), r.out[0].begin(), r.out[0].end());
        return r.out[0].size();
    }
}
inline size_t encode_block(const std::vector<uint8_t>& input, std::vector<uint8_t>& output)   // lz4.rs:616-627
{
    auto r = run_batch({input}, {rcx_lz4_compression_bound(input.size()) + 1}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_lz4_encode_batch(c, b); });
    if (r.status[0] == RCX_E_LZ4_INPUT_TOO_LARGE) return 0;
    check(r);
    output.insert(output.end(), r.out[0].begin(), r.out[0].end());
    return r.out[0].size();
}
// extension: one block from the high-compression encoder (levels 1..12: rcx_lz4_encode_hc_batch); decode_block reads it.  0 when
// compression_bound is None; a level outside 1..12 throws (RCX_RC_BAD_ARG).
inline size_t encode_block_hc(const std::vector<uint8_t>& input, std::vector<uint8_t>& output, int level = 9)
{
    auto r = run_batch({input}, {rcx_lz4_compression_bound(input.size()) + 1}, [level](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_lz4_encode_hc_batch(c, b, level); });
    if (r.status[0] == RCX_E_LZ4_INPUT_TOO_LARGE) return 0;
    check(r);
    output.insert(output.end(), r.out[0].begin(), r.out[0].end());
    return r.out[0].size();
}
}  // namespace lz4
namespace detail {
struct Lz4Frame { std::vector<std::pair<bool, std::vector<uint8_t>>> parts; size_t consumed = 0, max_block = 0; };   // (stored?, payload)
inline Lz4Frame lz4_parse_frame(const std::vector<uint8_t>& d)                       // the host framing of lz4.rs:316-500
{
    Lz4Frame f;
    size_t p = 0; const size_t n = d.size();
    auto need = [&](size_t k) { if (n - p < k) raise_status(RCX_E_EOF); };
    need(4);
    if (le32(&d[p]) != 0x184d2204u) throw io_error(ErrorKind::InvalidInput, RCX_E_LZ4_MAGIC, "");   // :365-367
    p += 4;
    uint8_t flg = p < n ? d[p] : 0, bd = p + 1 < n ? d[p + 1] : 0;               // :369-372
    p = p + 2 < n ? p + 2 : n;
    if ((flg >> 6) != 1) throw io_error(ErrorKind::InvalidInput, RCX_E_LZ4_VERSION, "");           // :375-377
    const bool blk_ck = flg & 0x10, ssize = flg & 0x08, preset = flg & 0x01;
    static const size_t MAXS[8] = {0, 0, 0, 0, 64u << 10, 256u << 10, 1u << 20, 4u << 20};
    f.max_block = MAXS[(bd >> 4) & 7];
    if (ssize) { need(8); p += 8; }
    if (preset) raise_status(RCX_E_MALFORMED);                                    // :407 assert!
    need(1); p += 1;                                                              // header checksum ignored, :417
    for (;;) {
        need(4);
        const uint32_t v = le32(&d[p]); p += 4;
        if (v == 0) break;
        const size_t amt = v & 0x7fffffffu;
        need(amt);
        f.parts.emplace_back((v & 0x80000000u) != 0, std::vector<uint8_t>(d.begin() + p, d.begin() + p + amt));
        p += amt;
        if (blk_ck) { need(4); p += 4; }
    }
    f.consumed = p;                                                               // (the content checksum is never read)
    return f;
}
// a conforming frame's blocks decode to at most max_block bytes: that is every block's slot; only a block that does not
// fit is decoded again with a larger one (the reference would grow its Vec)
inline std::vector<std::vector<uint8_t>> lz4_decode_frames(const std::vector<const Lz4Frame*>& fs)
{
    std::vector<std::vector<uint8_t>> comp; std::vector<uint64_t> caps;
    for (const Lz4Frame* f : fs) for (auto& pr : f->parts) if (!pr.first) { comp.push_back(pr.second); caps.push_back(std::max<size_t>(f->max_block, 1u << 16)); }
    BatchResult r;
    if (!comp.empty()) {
        r = run_batch(comp, caps, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_lz4_decode_batch(c, b); });
        for (size_t i = 0; i < comp.size(); i++)
            if (r.status[i] == RCX_E_OUTPUT_TOO_SMALL) { std::vector<uint8_t> o; lz4::decode_block(comp[i], o); r.out[i] = std::move(o); r.status[i] = RCX_OK; }
        check(r);
    }
    std::vector<std::vector<uint8_t>> outs(fs.size());
    size_t ci = 0;
    for (size_t k = 0; k < fs.size(); k++)
        for (auto& pr : fs[k]->parts) { const auto& src = pr.first ? pr.second : r.out[ci++]; outs[k].insert(outs[k].end(), src.begin(), src.end()); }
    return outs;
}
}  // namespace detail
namespace lz4 {
template <class R>
class Decoder : public BufferedDecoder<R, Decoder<R>> {                              // lz4.rs:316-500
public:
    using BufferedDecoder<R, Decoder<R>>::BufferedDecoder;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    {
        detail::Lz4Frame f = detail::lz4_parse_frame(d);
        this->consumed = f.consumed;
        std::vector<std::vector<uint8_t>> outs = detail::lz4_decode_frames({&f});
        return std::move(outs[0]);
    }
};
// Several frames, ONE batch call for every compressed block of every frame (a single 64 KiB block alone on the GPU takes six times what
// one host thread needs, eight or more together take less: INTEGRATION.md).  -> the decoded frames; consumed[i]: bytes frame i used.
inline std::vector<std::vector<uint8_t>> decode_many(const std::vector<std::vector<uint8_t>>& frames, std::vector<size_t>* consumed = nullptr)
{
    std::vector<detail::Lz4Frame> fs; fs.reserve(frames.size());
    for (const auto& d : frames) fs.push_back(detail::lz4_parse_frame(d));
    std::vector<const detail::Lz4Frame*> ps; for (auto& f : fs) ps.push_back(&f);
    if (consumed) { consumed->clear(); for (auto& f : fs) consumed->push_back(f.consumed); }
    return detail::lz4_decode_frames(ps);
}
template <class W>
class Encoder {                                                                       // lz4.rs:505-597 (stored blocks)
public:
    // level 0: the reference's frame, every block stored.  1..12 (extension): the full blocks are held and encoded by the
    // high-compression encoder in one batch call at flush() / finish(); a block is written compressed where that is smaller
    explicit Encoder(W w, int level = 0) : w_(std::move(w)), level_(level) {}
    size_t write(const uint8_t* buf, size_t n)
    {
        if (!wrote_header_) { const uint8_t h[7] = {0x04, 0x22, 0x4d, 0x18, 0x60, 0x50, 0x00}; w_.write(h, 7); wrote_header_ = true; }
        while (n) {
            const size_t amt = std::min(limit_ - buf_.size(), n);
            buf_.insert(buf_.end(), buf, buf + amt);
            if (buf_.size() == limit_) encode_block();
            buf += amt; n -= amt;
        }
        return 0;                                                                     // Ok(0) quirk, :588
    }
    void flush() { if (!buf_.empty()) encode_block(); write_held(); }
    W finish() { flush(); const uint8_t z[8] = {0}; w_.write(z, 8); return std::move(w_); }
private:
    void encode_block()
    {
        if (level_) { held_.push_back(std::move(buf_)); buf_.clear(); return; }
        std::vector<uint8_t> h; put32(h, (uint32_t)buf_.size() | 0x80000000u); w_.write(h.data(), 4); w_.write(buf_.data(), buf_.size()); buf_.clear();
    }
    void write_held()
    {
        if (held_.empty()) return;
        std::vector<uint64_t> caps;
        for (const auto& b : held_) caps.push_back(rcx_lz4_compression_bound(b.size()));
        const int level = level_;
        auto r = run_batch(held_, caps, [level](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_lz4_encode_hc_batch(c, b, level); });
        check(r);
        for (size_t i = 0; i < held_.size(); i++) {
            const bool comp = r.out[i].size() < held_[i].size();
            const std::vector<uint8_t>& d = comp ? r.out[i] : held_[i];
            std::vector<uint8_t> h; put32(h, (uint32_t)d.size() | (comp ? 0u : 0x80000000u));
            w_.write(h.data(), 4); w_.write(d.data(), d.size());
        }
        held_.clear();
    }
    W w_; std::vector<uint8_t> buf_; bool wrote_header_ = false; size_t limit_ = 256 * 1024; int level_ = 0;
    std::vector<std::vector<uint8_t>> held_;
};
}  // namespace lz4

// ---- flate / zlib / Adler32 ------------------------------------------------------------------------------
namespace detail {
template <class Fn> std::vector<uint8_t> grow_decode(const std::vector<uint8_t>& d, size_t& consumed, Fn fn, uint32_t* flags = nullptr)
{
    for (uint64_t cap = std::min<uint64_t>(MAX_BLOCK, std::max<uint64_t>(1u << 16, 4 * d.size()));; cap = std::min<uint64_t>(cap * 8, MAX_BLOCK)) {
        auto r = run_batch({d}, {cap}, fn);
        if (r.status[0] == RCX_E_OUTPUT_TOO_SMALL && cap < MAX_BLOCK) continue;
        check(r);
        consumed = r.in_used[0];
        if (flags) *flags = r.aux[0];
        return r.out[0];
    }
}
// several streams of one kind through ONE batch call; the slots that were too small once more, eight times larger, together
struct ManyResult { std::vector<std::vector<uint8_t>> out; std::vector<size_t> consumed; std::vector<uint32_t> flags; };
template <class Fn> ManyResult decode_many(const std::vector<std::vector<uint8_t>>& streams, Fn fn)
{
    ManyResult m;
    const size_t n = streams.size();
    m.out.resize(n); m.consumed.assign(n, 0); m.flags.assign(n, 0);
    if (!n) return m;
    std::vector<size_t> idx(n);
    uint64_t cap = 1u << 16;
    for (size_t i = 0; i < n; i++) { idx[i] = i; cap = std::max<uint64_t>(cap, 4 * streams[i].size()); }
    cap = std::min<uint64_t>(cap, MAX_BLOCK);
    std::vector<int> status(n, RCX_OK);
    for (;;) {
        std::vector<std::vector<uint8_t>> blobs; std::vector<uint64_t> caps(idx.size(), cap);
        for (size_t i : idx) blobs.push_back(streams[i]);
        auto r = run_batch(blobs, caps, fn);
        std::vector<size_t> redo;
        for (size_t j = 0; j < idx.size(); j++) {
            const size_t i = idx[j];
            status[i] = r.status[j];
            if (r.status[j] == RCX_E_OUTPUT_TOO_SMALL && cap < MAX_BLOCK) { redo.push_back(i); continue; }
            m.out[i] = std::move(r.out[j]); m.consumed[i] = r.in_used[j]; m.flags[i] = r.aux[j];
        }
        if (redo.empty()) break;
        idx.swap(redo);
        cap = std::min<uint64_t>(cap * 8, MAX_BLOCK);
    }
    for (int st : status) raise_status(st);                                       // the first stream that failed, as its own Decoder would
    return m;
}
// the DEFLATE encoders (extension: the reference has none): the whole input as ONE stream at finish(); write() only buffers.
// level 0 (the default): the level-1 encoder's bytes; 1..9: rcx_*_encode_level_batch; anything else throws (RCX_RC_BAD_ARG) at finish()
template <class W, int (*Call)(rcx_ctx*, const rcx_batch*), int (*CallLevel)(rcx_ctx*, const rcx_batch*, int), uint64_t Framing>
class OneShotEncoder {
public:
    explicit OneShotEncoder(W w, int level = 0) : w_(std::move(w)), level_(level) {}
    size_t write(const uint8_t* p, size_t n) { buf_.insert(buf_.end(), p, p + n); return n; }
    void write_all(const uint8_t* p, size_t n) { write(p, n); }
    W finish()
    {
        const int level = level_;
        auto r = run_batch({buf_}, {rcx_deflate_compression_bound(buf_.size()) + Framing}, [level](rcx_ctx* c, rcx_batch* b, uint32_t*) {
            return level ? CallLevel(c, b, level) : Call(c, b);
        });
        check(r);
        w_.write(r.out[0].data(), r.out[0].size());
        buf_.clear();
        return std::move(w_);
    }
private:
    W w_; std::vector<uint8_t> buf_; int level_ = 0;
};
}  // namespace detail
namespace flate {
template <class W> using Encoder = detail::OneShotEncoder<W, rcx_deflate_encode_batch, rcx_deflate_encode_level_batch, 0>;   // one raw DEFLATE stream (RFC 1951)
// many raw DEFLATE streams, ONE batch call (the reference decodes one deflate block per read(), flate.rs:468-488: a stream is one wave's work
// on the GPU -- a caller with many streams hands them over together)
inline detail::ManyResult decode_many(const std::vector<std::vector<uint8_t>>& streams)
{ return detail::decode_many(streams, [](rcx_ctx* c, rcx_batch* b, uint32_t* f) { return rcx_inflate_batch(c, b, f); }); }
template <class R>
class Decoder : public BufferedDecoder<R, Decoder<R>> {                              // flate.rs:164-488
public:
    using BufferedDecoder<R, Decoder<R>>::BufferedDecoder;
    uint32_t flags = 0;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    { return detail::grow_decode(d, this->consumed, [](rcx_ctx* c, rcx_batch* b, uint32_t* f) { return rcx_inflate_batch(c, b, f); }, &flags); }
};
}  // namespace flate
namespace zlib {
template <class W> using Encoder = detail::OneShotEncoder<W, rcx_zlib_encode_batch, rcx_zlib_encode_level_batch, 6>;      // one zlib stream (RFC 1950)
inline detail::ManyResult decode_many(const std::vector<std::vector<uint8_t>>& members)      // every member's Adler-32 checked on the device
{ return detail::decode_many(members, [](rcx_ctx* c, rcx_batch* b, uint32_t* f) { return rcx_zlib_decode_batch(c, b, f); }); }
template <class R>
class Decoder : public BufferedDecoder<R, Decoder<R>> {                              // zlib.rs:32-127
public:
    using BufferedDecoder<R, Decoder<R>>::BufferedDecoder;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    { return detail::grow_decode(d, this->consumed, [](rcx_ctx* c, rcx_batch* b, uint32_t* f) { return rcx_zlib_decode_batch(c, b, f); }); }
};
}  // namespace zlib
class Adler32 {                                                                       // checksum/adler.rs:22-51
public:
    void feed(const uint8_t* p, size_t n) { data_.insert(data_.end(), p, p + n); }
    uint32_t result() const
    {
        auto r = run_batch({data_}, {0}, [](rcx_ctx* c, rcx_batch* b, uint32_t* a) { return rcx_adler32_batch(c, b, a); });
        return r.aux[0];
    }
    void reset() { data_.clear(); }
private:
    std::vector<uint8_t> data_;
};

// ---- bwt ------------------------------------------------------------------------------------------------
namespace bwt {
inline std::pair<std::vector<uint8_t>, size_t> encode_simple(const std::vector<uint8_t>& input)   // bwt/mod.rs:214-219
{
    auto r = run_batch({input}, {input.size()}, [](rcx_ctx* c, rcx_batch* b, uint32_t* o) { return rcx_bwt_forward_batch(c, b, o); });
    check(r);
    return {r.out[0], r.aux[0]};
}
// bwt/mod.rs:136-166: fills suf_array (at least input.size() entries, as the reference indexes it) with the sorted suffixes
inline void compute_suffixes(const std::vector<uint8_t>& input, std::vector<uint32_t>& suf_array)
{
    if (suf_array.size() < input.size()) throw io_error(ErrorKind::Panic, RCX_E_OUTPUT_TOO_SMALL, "compute_suffixes: suf_array is shorter than the input");
    auto r = run_batch({input}, {4 * (uint64_t)input.size()}, [](rcx_ctx* c, rcx_batch* b, uint32_t* o) { return rcx_bwt_suffixes_batch(c, b, o); });
    check(r);
    if (!input.empty()) memcpy(suf_array.data(), r.out[0].data(), 4 * input.size());
}
// bwt/mod.rs:223-239: fills table (exactly input.size() entries: assert_eq!, :224) with the inversion jump table
inline void compute_inversion_table(const std::vector<uint8_t>& input, size_t origin, std::vector<uint32_t>& table)
{
    if (table.size() != input.size()) throw io_error(ErrorKind::Panic, RCX_E_MALFORMED, "compute_inversion_table: input.len() != table.len()");
    if (origin >= input.size()) throw io_error(ErrorKind::Panic, RCX_E_MALFORMED, "compute_inversion_table: origin out of range");
    uint32_t og = (uint32_t)origin;
    auto r = run_batch({input}, {4 * (uint64_t)input.size()}, [&](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_bwt_inversion_table_batch(c, b, &og); });
    check(r);
    memcpy(table.data(), r.out[0].data(), 4 * input.size());
}
inline std::vector<uint8_t> decode_simple(const std::vector<uint8_t>& input, size_t origin)       // bwt/mod.rs:291-294
{
    if (input.empty()) return {};
    uint32_t og = (uint32_t)origin;
    auto r = run_batch({input}, {input.size()}, [&](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_bwt_inverse_batch(c, b, &og); });
    check(r);
    return r.out[0];
}
template <class W>
class Encoder {                                                                       // bwt/mod.rs:437-518
public:
    Encoder(W w, size_t block_size) : w_(std::move(w)), bs_(block_size) {}
    size_t write(const uint8_t* buf, size_t n)
    {
        if (!wrote_header_) { std::vector<uint8_t> h; put32(h, (uint32_t)bs_); w_.write(h.data(), 4); wrote_header_ = true; }
        buf_.insert(buf_.end(), buf, buf + n);
        return 0;                                                                     // Ok(0) quirk, :507
    }
    void flush()                                                                      // :511-518: the buffered blocks and the partial one, ONE batch call
    {
        std::vector<std::vector<uint8_t>> blocks; std::vector<uint64_t> caps;
        const size_t bs = std::max<size_t>(bs_, 1);
        for (size_t i = 0; i < buf_.size(); i += bs) { blocks.emplace_back(buf_.begin() + i, buf_.begin() + std::min(buf_.size(), i + bs)); caps.push_back(blocks.back().size()); }
        if (!blocks.empty()) {
            auto r = run_batch(blocks, caps, [](rcx_ctx* c, rcx_batch* b, uint32_t* o) { return rcx_bwt_forward_batch(c, b, o); });
            check(r);
            for (size_t i = 0; i < blocks.size(); i++) {
                std::vector<uint8_t> h; put32(h, (uint32_t)blocks[i].size()); w_.write(h.data(), 4);
                w_.write(r.out[i].data(), r.out[i].size());
                h.clear(); put32(h, r.aux[i]); w_.write(h.data(), 4);
            }
        }
        buf_.clear();
    }
    W finish() { flush(); return std::move(w_); }                                     // :485-489
private:
    W w_; size_t bs_; std::vector<uint8_t> buf_; bool wrote_header_ = false;
};
template <class R>
class Decoder : public BufferedDecoder<R, Decoder<R>> {                              // bwt/mod.rs:321-432
public:
    Decoder(R r, bool extra_mem) : BufferedDecoder<R, Decoder<R>>(std::move(r)), extra_memory(extra_mem) {}
    bool extra_memory; size_t max_block_size = 0;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    {
        size_t p = 0; const size_t n = d.size();
        if (n - p < 4) raise_status(RCX_E_EOF);                                       // :369
        max_block_size = le32(&d[p]); p += 4;
        std::vector<std::vector<uint8_t>> Ls; std::vector<uint64_t> caps; std::vector<uint32_t> origins;
        while (n - p >= 4) {                                                          // EOF at a block boundary ends, :374-377
            const size_t bn = le32(&d[p]); p += 4;
            if (n - p < bn) raise_status(RCX_E_EOF);
            Ls.emplace_back(d.begin() + p, d.begin() + p + bn); p += bn;
            if (n - p < 4) raise_status(RCX_E_EOF);
            origins.push_back(le32(&d[p])); p += 4;
            if (bn == 0 && extra_memory) raise_status(RCX_E_MALFORMED);               // :230 panic (decode_minimal: only if origin != 0, :300-302)
            caps.push_back(bn);
        }
        std::vector<uint8_t> out;
        if (Ls.empty()) return out;
        // extra_mem = false is the reference's decode_minimal (:298-315, :397-399), reproduced as it computes (not an inverse in general)
        auto r = run_batch(Ls, caps, [&](rcx_ctx* c, rcx_batch* b, uint32_t*) {
            return extra_memory ? rcx_bwt_inverse_batch(c, b, origins.data()) : rcx_bwt_inverse_minimal_batch(c, b, origins.data()); });
        check(r);
        for (auto& o : r.out) out.insert(out.end(), o.begin(), o.end());
        return out;
    }
};
namespace mtf {
inline std::vector<uint8_t> encode(const std::vector<uint8_t>& in)                   // mtf::Encoder over a whole stream, mtf.rs:95-129
{ auto r = run_batch({in}, {in.size()}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_mtf_encode_batch(c, b); }); check(r); return r.out[0]; }
inline std::vector<uint8_t> decode(const std::vector<uint8_t>& in)                   // mtf::Decoder, mtf.rs:133-169
{ auto r = run_batch({in}, {in.size()}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_mtf_decode_batch(c, b); }); check(r); return r.out[0]; }
}  // namespace mtf
namespace dc {
inline std::vector<uint32_t> encode_simple(const std::vector<uint8_t>& in)           // dc.rs:153-159
{
    auto r = run_batch({in}, {4 * (256 + in.size())}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_dc_encode_batch(c, b); });
    check(r);
    std::vector<uint32_t> w(r.out[0].size() / 4);
    for (size_t i = 0; i < w.size(); i++) w[i] = le32(&r.out[0][4 * i]);
    return w;
}
inline std::vector<uint8_t> decode_simple(size_t n, const std::vector<uint32_t>& distances)   // dc.rs:236-252
{
    std::vector<uint8_t> blob; for (uint32_t x : distances) put32(blob, x);
    uint64_t nn = n;
    auto r = run_batch({blob}, {n}, [&](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_dc_decode_batch(c, b, &nn); });
    check(r);
    return r.out[0];
}
struct Context { uint8_t symbol, last_rank; size_t distance_limit;                  // dc.rs:40-58
                 bool operator==(const Context& o) const { return symbol == o.symbol && last_rank == o.last_rank && distance_limit == o.distance_limit; } };
struct Encoded { std::vector<uint32_t> init; std::vector<std::pair<uint32_t, Context>> pairs; };
// dc.rs:110-149 in batch-backed form: the initial positions (:83-86) and the (distance, Context) pairs the iterator yields (:88-103)
inline Encoded encode(const std::vector<uint8_t>& in)
{
    const size_t n = in.size();
    auto r = run_batch({in}, {4 * (256 + n) + 8 * n}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_dc_encode_ctx_batch(c, b); });
    check(r);
    const auto& o = r.out[0];
    const size_t k = (o.size() - 4 * (256 + n)) / 8, cb = 4 * (256 + n);
    Encoded e;
    for (size_t s = 0; s < 256; s++) e.init.push_back(le32(&o[4 * s]));
    for (size_t j = 0; j < k; j++) e.pairs.push_back({le32(&o[4 * (256 + j)]), Context{o[cb + 8 * j], o[cb + 8 * j + 1], le32(&o[cb + 8 * j + 4])}});
    return e;
}
// dc.rs:162-233 in batch-backed form: the decoded block and the Context handed to the distance callback before each read (:208)
inline std::pair<std::vector<uint8_t>, std::vector<Context>> decode(const std::vector<uint32_t>& init, const std::vector<uint32_t>& distances, size_t n)
{
    std::vector<uint8_t> blob; for (uint32_t x : init) put32(blob, x); for (uint32_t x : distances) put32(blob, x);
    uint64_t nn = n;
    const size_t co = (n + 7) & ~(size_t)7;
    auto r = run_batch({blob}, {co + 8 * distances.size()}, [&](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_dc_decode_ctx_batch(c, b, &nn); });
    check(r);
    const auto& o = r.out[0];
    std::vector<Context> cx;
    for (size_t p = co; p + 8 <= o.size(); p += 8) cx.push_back(Context{o[p], o[p + 1], le32(&o[p + 4])});
    return {std::vector<uint8_t>(o.begin(), o.begin() + n), cx};
}
}  // namespace dc
}  // namespace bwt

// ---- entropy::ari ----------------------------------------------------------------------------------------
namespace entropy { namespace ari {
template <class W>
class ByteEncoder {                                                                   // table.rs:185-224
public:
    explicit ByteEncoder(W w) : w_(std::move(w)) {}
    size_t write(const uint8_t* p, size_t n) { buf_.insert(buf_.end(), p, p + n); return n; }
    W finish()
    {
        auto r = run_batch({buf_}, {rcx_ari_byte_encode_bound(buf_.size())}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_ari_byte_encode_batch(c, b); });
        check(r);
        w_.write(r.out[0].data(), r.out[0].size());
        return std::move(w_);
    }
private:
    W w_; std::vector<uint8_t> buf_;
};
template <class R>
class ByteDecoder : public BufferedDecoder<R, ByteDecoder<R>> {                      // table.rs:229-273
public:
    using BufferedDecoder<R, ByteDecoder<R>>::BufferedDecoder;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    { return detail::grow_decode(d, this->consumed, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_ari_byte_decode_batch(c, b); }); }
    // finish() (BufferedDecoder): the reader ends exactly after this stream (mod.rs:289-292)
};
}}  // namespace entropy::ari

// ---- rle ------------------------------------------------------------------------------------------------
namespace rle {
template <class W>
class Encoder {                                                                       // rle.rs:40-123 (one-shot write_all + finish)
public:
    explicit Encoder(W w) : w_(std::move(w)) {}
    void write_all(const uint8_t* p, size_t n) { buf_.insert(buf_.end(), p, p + n); }
    W finish()
    {
        auto r = run_batch({buf_}, {rcx_rle_encode_bound(buf_.size())}, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_rle_encode_batch(c, b); });
        check(r);
        w_.write(r.out[0].data(), r.out[0].size());
        return std::move(w_);
    }
private:
    W w_; std::vector<uint8_t> buf_;
};
template <class R>
class Decoder : public BufferedDecoder<R, Decoder<R>> {                              // rle.rs:176-281
public:
    using BufferedDecoder<R, Decoder<R>>::BufferedDecoder;
    std::vector<uint8_t> decode_all(const std::vector<uint8_t>& d)
    { return detail::grow_decode(d, this->consumed, [](rcx_ctx* c, rcx_batch* b, uint32_t*) { return rcx_rle_decode_batch(c, b); }); }
};
}  // namespace rle

}  // namespace compress
