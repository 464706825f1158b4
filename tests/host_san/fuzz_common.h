// fuzz_common.h -- what the sanitizer programs of tests/host_san share: a fixed random generator, heap blocks of an exact size (so
// that AddressSanitizer sees an overrun of one byte), a failure report that names seed and iteration, and the PNG mutant generator.
//
// Which checksums the PNG reader (csrc/io_png.hip) verifies, read from its code: it verifies NO chunk CRC-32.  The Adler-32 of the
// zlib stream is verified by zlib's inflate, and only when inflate reaches the stream's trailer, which it does when the stream holds
// exactly the scanlines' bytes; a stream that holds more is accepted once the scanlines are full.  So byte mutations of a file end in
// inflate's own checks almost every time; the mutations that reach the unfilter code are the ones made here on the INFLATED scanlines,
// which are deflated again (compress2 writes a matching Adler-32) into one IDAT chunk whose length and CRC are recomputed.  The CRCs
// are repaired all the same, so that the files stay honest if the reader one day checks them.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include <sanitizer/common_interface_defs.h>

#include "../../include/kbnet_hip.h"

typedef std::vector<unsigned char> Bytes;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull) { next(); next(); }
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    uint32_t below(uint32_t n) { return n ? (uint32_t)((next() >> 11) % n) : 0; }     // [0, n)
    int range(int lo, int hi) { return lo + (int)below((uint32_t)(hi - lo + 1)); }    // [lo, hi]
};

// ---- where a failure happened
static const char* g_program = "?";
static const char* g_stage = "";
static uint64_t g_seed = 0;
static long long g_iteration = 0;
static void where(FILE* f) { fprintf(f, "%s: stage '%s', seed %llu, iteration %lld\n", g_program, g_stage, (unsigned long long)g_seed, g_iteration); }
static void on_death() { fprintf(stderr, "the sanitizer report above: "); where(stderr); }
[[noreturn]] static void fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("FAIL: ");
    vprintf(fmt, ap);
    va_end(ap);
    printf("\n");
    where(stdout);
    fflush(stdout);
    exit(1);
}
#define REQUIRE(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

// ---- a heap block of exactly n bytes
struct Block {
    unsigned char* p;
    size_t n;
    explicit Block(size_t bytes, int fill = 0xA5) : p((unsigned char*)malloc(bytes)), n(bytes) {
        if (bytes && !p) fail("out of memory (%zu bytes)", bytes);
        if (bytes) memset(p, fill, bytes);
    }
    explicit Block(const Bytes& b) : p((unsigned char*)malloc(b.size())), n(b.size()) {
        if (n) memcpy(p, b.data(), n);
    }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block() { free(p); }
    bool all(int value) const {
        for (size_t i = 0; i < n; ++i)
            if (p[i] != (unsigned char)value) return false;
        return true;
    }
};

static Bytes read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) fail("cannot read %s", path);
    Bytes b;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

// ---- PNG files taken apart and put together again
static uint32_t be32(const unsigned char* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
static void put32(Bytes& b, uint32_t v) { b.push_back(v >> 24); b.push_back(v >> 16 & 255); b.push_back(v >> 8 & 255); b.push_back(v & 255); }
static void put_chunk(Bytes& out, const char* type, const Bytes& data) {
    put32(out, (uint32_t)data.size());
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data.begin(), data.end());
    put32(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), out.data() + at, (uInt)(out.size() - at)));
}

struct Png {
    Bytes ihdr;                     // 13 bytes
    Bytes plte;                     // empty when the file has none
    Bytes raw;                      // the inflated scanlines: height x (filter byte + stride)
    int width() const { return (int)be32(ihdr.data()); }
    int height() const { return (int)be32(ihdr.data() + 4); }
    int depth() const { return ihdr[8]; }
    int colour() const { return ihdr[9]; }
    size_t stride() const {         // bytes of a scanline without its filter byte, as the reader computes them
        const int channels = colour() == 2 ? 3 : (colour() == 6 ? 4 : (colour() == 4 ? 2 : 1));
        return (size_t)width() * channels * (depth() / 8 ? depth() / 8 : 1);
    }
};

static Png png_parse(const Bytes& file) {    // a fixture: well-formed
    Png p;
    Bytes z;
    size_t pos = 8;
    while (pos + 12 <= file.size()) {
        const size_t len = be32(file.data() + pos);
        const unsigned char* type = file.data() + pos + 4;
        const unsigned char* data = type + 4;
        if (pos + 12 + len > file.size()) fail("a fixture PNG is damaged");
        if (!memcmp(type, "IHDR", 4)) p.ihdr.assign(data, data + len);
        if (!memcmp(type, "PLTE", 4)) p.plte.assign(data, data + len);
        if (!memcmp(type, "IDAT", 4)) z.insert(z.end(), data, data + len);
        pos += 12 + len;
    }
    if (p.ihdr.size() != 13) fail("a fixture PNG has no IHDR");
    p.raw.resize((size_t)p.height() * (p.stride() + 1));
    uLongf n = (uLongf)p.raw.size();
    if (uncompress(p.raw.data(), &n, z.data(), (uLong)z.size()) != Z_OK || n != p.raw.size()) fail("a fixture PNG does not inflate");
    return p;
}

static Bytes png_build(const Png& p, int level = 6) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    Bytes out(sig, sig + 8);
    put_chunk(out, "IHDR", p.ihdr);
    if (!p.plte.empty()) put_chunk(out, "PLTE", p.plte);
    Bytes z(compressBound((uLong)p.raw.size()));
    uLongf zn = (uLongf)z.size();
    if (compress2(z.data(), &zn, p.raw.data(), (uLong)p.raw.size(), level) != Z_OK) fail("compress2");
    z.resize(zn);
    put_chunk(out, "IDAT", z);
    put_chunk(out, "IEND", Bytes());
    return out;
}

// png_fuzz.py's six kinds of byte mutation, on the file
static Bytes png_mutate_bytes(const Bytes& file, Rng& r) {
    Bytes d = file;
    switch (r.below(6)) {
        case 0: d.resize(r.below((uint32_t)d.size())); break;
        case 1: for (int i = r.range(1, 7); i > 0; --i) d[r.below((uint32_t)d.size())] = (unsigned char)r.below(256); break;
        case 2: d[16 + r.below(13)] = (unsigned char)r.below(256); break;
        case 3: {   // a chunk length
            std::vector<size_t> chunks;
            for (size_t pos = 8; pos + 8 <= d.size(); pos += 12 + (size_t)be32(d.data() + pos)) chunks.push_back(pos);
            const uint32_t values[6] = {0, 1, 0x7fffffffu, 0xffffffffu, (uint32_t)d.size(), (uint32_t)r.next()};
            const uint32_t v = values[r.below(6)];
            unsigned char* at = d.data() + chunks[r.below((uint32_t)chunks.size())];
            at[0] = v >> 24; at[1] = v >> 16 & 255; at[2] = v >> 8 & 255; at[3] = v & 255;
            break;
        }
        case 4: {   // huge dimensions
            const uint32_t values[6] = {0, 1, 65535, 1u << 20, 0x7fffffffu, 0xffffffffu};
            const uint32_t w = values[r.below(6)], h = values[r.below(5)];
            unsigned char* at = d.data() + 16;
            at[0] = w >> 24; at[1] = w >> 16 & 255; at[2] = w >> 8 & 255; at[3] = w & 255;
            at[4] = h >> 24; at[5] = h >> 16 & 255; at[6] = h >> 8 & 255; at[7] = h & 255;
            break;
        }
        default: for (int i = r.range(1, 63); i > 0; --i) d.push_back((unsigned char)r.below(256)); break;
    }
    return d;
}

// Mutations behind the checksums: on the inflated scanlines and the IHDR fields, the file rebuilt with length, CRC and Adler-32 right.
// kind 0 .. PNG_DEEP_KINDS - 1; `v`: a value some kinds take (the filter type)
constexpr int PNG_DEEP_KINDS = 9;
static Bytes png_mutate_deep(const Png& src, int kind, int v, Rng& r) {
    Png p = src;
    const size_t row = p.stride() + 1;
    const int h = p.height();
    auto set32 = [&](int at, uint32_t x) { p.ihdr[at] = x >> 24; p.ihdr[at + 1] = x >> 16 & 255; p.ihdr[at + 2] = x >> 8 & 255; p.ihdr[at + 3] = x & 255; };
    auto random_lines = [&]() {   // scanlines of the size the (new) header asks for: every filter type, random bytes
        const size_t n = (size_t)p.height() * (p.stride() + 1);
        if (n > (1u << 22)) return;
        p.raw.resize(n);
        for (size_t i = 0; i < n; ++i) p.raw[i] = (unsigned char)r.below(256);
        for (int y = 0; y < p.height(); ++y) p.raw[(size_t)y * (p.stride() + 1)] = (unsigned char)r.below(5);
    };
    switch (kind) {
        case 0: p.raw[0] = (unsigned char)v; break;                                          // the first row's filter type
        case 1: p.raw[(size_t)r.below((uint32_t)h) * row] = (unsigned char)v; break;        // some row's
        case 2: for (int i = r.range(1, 8); i > 0; --i) p.raw[r.below((uint32_t)p.raw.size())] ^= (unsigned char)(1u << r.below(8)); break;
        case 3: random_lines(); break;
        case 4: {                                                                            // shorter or longer by 1 or by a row
            const long long delta[4] = {-1, 1, -(long long)row, (long long)row};
            const long long n = (long long)p.raw.size() + delta[r.below(4)];
            p.raw.resize((size_t)(n < 0 ? 0 : n), (unsigned char)r.below(5));
            break;
        }
        case 5: { const int depths[6] = {0, 1, 2, 4, 8, 16}; p.ihdr[8] = (unsigned char)depths[r.below(6)]; if (r.below(2)) random_lines(); break; }
        case 6: { const int colours[7] = {0, 2, 3, 4, 6, 1, 7}; p.ihdr[9] = (unsigned char)colours[r.below(7)]; if (r.below(2)) random_lines(); break; }
        case 7: p.ihdr[12] = (unsigned char)r.range(1, 2); break;                            // interlace
        default: {                                                                           // width, height +- 1
            if (r.below(2)) set32(0, (uint32_t)(p.width() + (r.below(2) ? 1 : -1)));
            else set32(4, (uint32_t)(p.height() + (r.below(2) ? 1 : -1)));
            if (r.below(2)) random_lines();
            break;
        }
    }
    return png_build(p, r.below(2) ? 1 : 6);
}
