// codec_fuzz -- the host codecs between untrusted bytes and the device, csrc/frame_pack.hip and csrc/io_png.hip, in a build with
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_sanitizers_cpu.py builds and runs it; nothing else is linked).
// Deterministic: fixed seeds, and every failure names its stage, seed and iteration.  Every file handed to the library lives in a
// heap block of exactly file_bytes bytes and every output in a block of exactly the size passed: an overrun of one byte is a report.
//
// Packed frames (format version 1, csrc/frame_pack.h).  For every input:
//   1. kbn_frame_decode answers KBN_OK exactly when kbn_frame_check does, given a big enough output;
//   2. kbn_frame_info succeeds whenever check does, with the geometry decode then fills;
//   3. an accepted file, decoded into exactly W H C bits / 8 bytes, re-encodes to a file check accepts and that decodes to the same;
//   4. with samples_bytes one short decode refuses and writes nothing.
// Inputs: encoded frames; byte mutations and structure-aware ones of them; files no encoder of ours writes but the format allows
// (header bytes wider than needed, nonzero pad bits, wholly random field bits under random header bytes), which check must accept.
//
// PNG: see fuzz_common.h for which checksums the reader verifies and what follows for the mutations.
// usage: codec_fuzz [--scale PERCENT] PNG...
#include <limits.h>

#include <algorithm>

#include "fuzz_common.h"

static long long g_accepted = 0, g_refused = 0, g_noncanonical = 0, g_illegal = 0, g_illegal_accepted = 0;

// ================================================================================================ packed frames
struct Geo { int w, h, c, bits; };
static const Geo GEOS[] = {{1, 1, 1, 8}, {15, 1, 3, 8}, {16, 8, 1, 16}, {17, 9, 4, 8}, {129, 17, 3, 8}, {43, 25, 1, 16}, {120, 24, 3, 8}};
// contents: 0 noise, 1 constant, 2 sparse (1 sample in 20 set), 3 wrap (0 beside 2^bits - 1)

static size_t samples_bytes(const Geo& g) { return (size_t)g.w * g.h * g.c * (g.bits / 8); }
static unsigned get_sample(const Bytes& s, const Geo& g, size_t i) {
    if (g.bits == 8) return s[i];
    uint16_t v;
    memcpy(&v, s.data() + 2 * i, 2);
    return v;
}
static void put_sample(Bytes& s, const Geo& g, size_t i, unsigned v) {
    if (g.bits == 8) { s[i] = (unsigned char)v; return; }
    const uint16_t u = (uint16_t)v;
    memcpy(s.data() + 2 * i, &u, 2);
}

static Bytes make_content(const Geo& g, int content, Rng& r) {
    Bytes s(samples_bytes(g));
    const unsigned top = (1u << g.bits) - 1u;
    const unsigned constant = r.below(top + 1);
    for (size_t i = 0; i < (size_t)g.w * g.h * g.c; ++i) {
        unsigned v;
        switch (content) {
            case 0: v = r.below(top + 1); break;
            case 1: v = constant; break;
            case 2: v = r.below(20) == 0 ? 1 + r.below(top) : 0; break;
            default: { const unsigned three[3] = {0, top, (top + 1) / 2}; v = three[r.below(3)]; break; }
        }
        put_sample(s, g, i, v);
    }
    return s;
}

// kbn_frame_encode into a block of exactly its bound; one byte less is refused
static Bytes encode(const Bytes& samples, const Geo& g) {
    const size_t bound = kbn_frame_encode_bound(g.w, g.h, g.c, g.bits);
    REQUIRE(bound != 0, "kbn_frame_encode_bound(%d, %d, %d, %d) = 0", g.w, g.h, g.c, g.bits);
    Block in(samples), out(bound);
    size_t n = (size_t)-1;
    int rc = kbn_frame_encode(in.p, g.w, g.h, g.c, g.bits, out.p, bound, &n);
    REQUIRE(rc == KBN_OK && n <= bound, "kbn_frame_encode: status %d, %zu bytes, bound %zu", rc, n, bound);
    Block small(bound - 1);
    size_t m = 12345;
    rc = kbn_frame_encode(in.p, g.w, g.h, g.c, g.bits, small.p, bound - 1, &m);
    REQUIRE(rc == KBN_ERR_WORKSPACE, "kbn_frame_encode with capacity bound - 1: status %d, not KBN_ERR_WORKSPACE", rc);
    REQUIRE(small.all(0xA5) && m == 12345, "a refused kbn_frame_encode wrote");
    return Bytes(out.p, out.p + n);
}

// properties 1 - 4 for one input; true when it was accepted.  `expect`: samples the file must decode to, or null
//   `must_refuse`: the format forbids the file (a header byte above `bits`); decode runs before that is asserted, so that what a
//   too lenient check lets through also meets the sanitizers
static bool frame_properties(const Bytes& file, const Bytes* expect = nullptr, bool must_accept = false, bool must_refuse = false) {
    Block f(file);
    const int checked = kbn_frame_check(f.p, f.n);
    int w = -1, h = -1, c = -1, bits = -1;
    const int informed = kbn_frame_info(f.p, f.n, &w, &h, &c, &bits);
    if (must_refuse && informed == KBN_OK) {
        Block out((size_t)w * h * c * (bits / 8));
        const int rc = kbn_frame_decode(f.p, f.n, out.p, out.n);
        if (checked == KBN_OK || rc == KBN_OK) {      // reported when the stage ends: the files behind this one still meet the sanitizers
            ++g_illegal_accepted;
            return false;
        }
    }
    if (checked != KBN_OK) {
        REQUIRE(!must_accept, "kbn_frame_check refuses (status %d) a file the format allows", checked);
        // property 1: what check refuses decode refuses, and writes nothing -- into what the header asks for, where that is sane
        const unsigned long long asked = informed == KBN_OK ? (unsigned long long)w * h * c * (bits / 8) : 0;
        Block out(asked >= 1 && asked <= (1ull << 20) ? (size_t)asked : (size_t)4096);
        const int rc = kbn_frame_decode(f.p, f.n, out.p, out.n);
        REQUIRE(rc != KBN_OK, "kbn_frame_decode accepts a file kbn_frame_check refuses (status %d)", checked);
        REQUIRE(out.all(0xA5), "kbn_frame_decode wrote for a file it refused");
        ++g_refused;
        return false;
    }
    REQUIRE(informed == KBN_OK, "kbn_frame_info refuses (status %d) a file kbn_frame_check accepts", informed);      // property 2
    REQUIRE(w >= 1 && h >= 1 && (c == 1 || c == 3 || c == 4) && (bits == 8 || bits == 16), "kbn_frame_info: geometry %d x %d x %d, %d bits", w, h, c, bits);
    // an accepted file holds a header byte for every segment of every plane: its geometry cannot be much larger than the file
    const unsigned long long need = (unsigned long long)w * h * c * (bits / 8);
    REQUIRE(need <= 64ull * 2 * f.n, "kbn_frame_check accepts %zu bytes as a frame of %llu sample bytes", f.n, need);
    const Geo g{w, h, c, bits};
    Block out((size_t)need);
    int rc = kbn_frame_decode(f.p, f.n, out.p, out.n);       // properties 1 and 2: the geometry of info is what decode fills
    REQUIRE(rc == KBN_OK, "kbn_frame_decode refuses (status %d) a file kbn_frame_check accepts", rc);
    if (expect) REQUIRE(expect->size() == out.n && memcmp(expect->data(), out.p, out.n) == 0, "the file does not decode to the samples it was built from");
    {                                                         // decode wrote every sample: a second decode over another fill agrees
        Block again((size_t)need, 0x5A);
        rc = kbn_frame_decode(f.p, f.n, again.p, again.n);
        REQUIRE(rc == KBN_OK && memcmp(again.p, out.p, out.n) == 0, "kbn_frame_decode left samples unwritten");
    }
    {                                                         // property 4
        Block small((size_t)need - 1);
        rc = kbn_frame_decode(f.p, f.n, small.p, small.n);
        REQUIRE(rc != KBN_OK, "kbn_frame_decode accepts samples_bytes one short");
        REQUIRE(small.all(0xA5), "kbn_frame_decode with samples_bytes one short wrote");
    }
    {                                                         // property 3
        const Bytes samples(out.p, out.p + out.n);
        const Bytes again = encode(samples, g);
        Block e(again);
        REQUIRE(kbn_frame_check(e.p, e.n) == KBN_OK, "kbn_frame_check refuses what kbn_frame_encode wrote");
        Block back((size_t)need);
        rc = kbn_frame_decode(e.p, e.n, back.p, back.n);
        REQUIRE(rc == KBN_OK && memcmp(back.p, out.p, out.n) == 0, "decode -> encode -> decode changes the samples");
    }
    ++g_accepted;
    return true;
}

// ---- the layout of a file of ours, for the structure-aware mutations
struct Parsed {
    Geo g;
    size_t groups, segments, entries, table_end, start;
    std::vector<uint32_t> table;      // entries + 1
};
static uint32_t le32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static void set_le(Bytes& f, size_t at, int bytes, uint64_t v) { for (int i = 0; i < bytes; ++i) f[at + i] = (unsigned char)(v >> (8 * i)); }
static uint64_t get_le(const Bytes& f, size_t at, int bytes) { uint64_t v = 0; for (int i = 0; i < bytes; ++i) v |= (uint64_t)f[at + i] << (8 * i); return v; }
static Parsed parse(const Bytes& f, const Geo& g) {
    Parsed p;
    p.g = g;
    p.groups = ((size_t)g.h + 7) / 8;
    p.segments = ((size_t)g.w + 15) / 16;
    p.entries = p.groups * g.c;
    p.table_end = 32 + 4 * (p.entries + 1);
    p.start = (p.table_end + 15) / 16 * 16;
    for (size_t e = 0; e <= p.entries; ++e) p.table.push_back(le32(f.data() + 32 + 4 * e));
    return p;
}
static unsigned seg_bytes(int n, int b, int bits, bool left) { return (unsigned)((left ? bits + (n - 1) * b : n * b) + 7) / 8; }

// every structure-aware mutant of `f`, each through the properties
static void structural(const Bytes& f, const Geo& g, Rng& r) {
    const Parsed p = parse(f, g);
    auto run = [&](const Bytes& m) { ++g_iteration; frame_properties(m); };
    struct Field { size_t at; int bytes; };
    const Field fields[7] = {{8, 4}, {12, 4}, {16, 2}, {18, 2}, {20, 2}, {22, 2}, {24, 8}};
    for (const Field& fd : fields) {
        const uint64_t now = get_le(f, fd.at, fd.bytes);
        const uint64_t values[7] = {0, 1, 0x7fffffffull, 0x80000000ull, 0xffffffffull, now + 1, now - 1};
        for (uint64_t v : values) { Bytes m = f; set_le(m, fd.at, fd.bytes, v); run(m); }
    }
    const size_t last = 32 + 4 * p.entries;
    for (int d = -1; d <= 1; d += 2) { Bytes m = f; set_le(m, last, 4, (uint64_t)p.table.back() + d); run(m); }
    for (int d = -1; d <= 1; d += 2) {      // payload_bytes and the table's last entry together
        Bytes m = f; set_le(m, last, 4, (uint64_t)p.table.back() + d); set_le(m, 24, 8, (uint64_t)p.table.back() + d); run(m);
    }
    for (size_t e = 0; e + 1 <= p.entries; ++e) {
        Bytes m = f; set_le(m, 32 + 4 * e, 4, p.table[e + 1]); set_le(m, 32 + 4 * (e + 1), 4, p.table[e]); run(m);       // neighbours swapped
        m = f; set_le(m, 32 + 4 * e, 4, p.table[e + 1]); run(m);                                                          // made equal
        m = f; set_le(m, 32 + 4 * (e + 1), 4, p.table[e]); run(m);
        m = f; set_le(m, 32 + 4 * e, 4, (uint64_t)p.table.back() + 1 + r.below(64)); run(m);                              // past payload_bytes
        m = f; set_le(m, 32 + 4 * e, 4, 0xffffffffull - r.below(4)); run(m);
    }
    for (int i = 0; i < 8 && p.entries >= 2; ++i) {      // any two entries
        const size_t a = r.below((uint32_t)p.entries + 1), b = r.below((uint32_t)p.entries + 1);
        Bytes m = f; set_le(m, 32 + 4 * a, 4, p.table[b]); set_le(m, 32 + 4 * b, 4, p.table[a]); run(m);
    }
    for (size_t e = 0; e < p.entries; ++e) {             // header bytes: b +- 1, bits, bits + 1, 255 (the sizes no longer fit, or b is illegal)
        const size_t rows = std::min<size_t>(8, (size_t)g.h - e / g.c * 8), heads = rows * p.segments;
        for (size_t i = 0; i < heads; ++i) {
            if (heads > 64 && r.below((uint32_t)(heads / 32)) != 0 && i != 0 && i + 1 != heads) continue;      // a sample of the long ones
            const size_t at = p.start + p.table[e] + i;
            const int b = f[at];
            for (int v : {b + 1, b - 1, g.bits, g.bits + 1, 255}) {
                if (v < 0) continue;
                Bytes m = f; m[at] = (unsigned char)v; run(m);
            }
        }
    }
    for (size_t at = p.table_end; at < p.start; ++at) { Bytes m = f; m[at] = (unsigned char)(1 + r.below(255)); run(m); }
    std::vector<size_t> bounds = {32, p.table_end, p.start, f.size()};
    for (size_t e = 0; e <= p.entries; ++e) bounds.push_back(p.start + p.table[e]);
    for (size_t b : bounds)
        for (int d = -1; d <= 1; ++d) {
            const long long n = (long long)b + d;
            if (n < 0) continue;
            Bytes m = f;
            m.resize((size_t)n, (unsigned char)r.below(256));      // truncated, or a byte longer
            run(m);
        }
    for (int n = 1; n <= 64; ++n) { Bytes m = f; for (int i = 0; i < n; ++i) m.push_back((unsigned char)r.below(256)); run(m); }
    // the payload cut at the start of a (group, plane), inside its header bytes and right behind them, and the table and payload_bytes
    // repaired to say so: every size the header states is then true, and the planes from there on are short or empty
    for (size_t e = 0; e < p.entries; ++e) {
        const size_t rows = std::min<size_t>(8, (size_t)g.h - e / g.c * 8), heads = rows * p.segments;
        for (size_t cut : {(size_t)p.table[e], (size_t)p.table[e] + heads / 2, (size_t)p.table[e] + heads - 1, (size_t)p.table[e] + heads}) {
            Bytes m = f;
            m.resize(p.start + cut);
            for (size_t j = 0; j <= p.entries; ++j)
                if (p.table[j] > cut) set_le(m, 32 + 4 * j, 4, cut);
            set_le(m, 24, 8, cut);
            run(m);
            // ... and the same file with one inner entry left where it was, or pushed farther, above the new payload_bytes: the
            // plane in front of it then claims room for its header bytes that the file does not have.  check_file reads a plane's
            // header bytes before it looks at the next entry, so only `hi > payload_bytes` stands between this file and that read
            for (size_t j = e + 1; j < p.entries; ++j) {
                if (j > e + 2 && j + 1 != p.entries) continue;      // the next entry, the one after it, the last inner one
                for (uint64_t v : {(uint64_t)p.table[j], (uint64_t)cut + heads + 1000, (uint64_t)0xfffffff0u}) {
                    if (v <= cut) continue;
                    Bytes n = m;
                    set_le(n, 32 + 4 * j, 4, v);
                    run(n);
                }
            }
        }
    }
}

// byte mutations as tests/png_fuzz.py makes them
static Bytes frame_mutate_bytes(const Bytes& f, const Parsed& p, Rng& r) {
    Bytes d = f;
    switch (r.below(6)) {
        case 0: d.resize(r.below((uint32_t)d.size())); break;
        case 1: for (int i = r.range(1, 7); i > 0; --i) d[r.below((uint32_t)d.size())] = (unsigned char)r.below(256); break;
        case 2: d[8 + r.below(24)] = (unsigned char)r.below(256); break;                       // a header field
        case 3: {                                                                              // a table entry
            const uint32_t values[6] = {0, 1, 0x7fffffffu, 0xffffffffu, (uint32_t)d.size(), (uint32_t)r.next()};
            set_le(d, 32 + 4 * r.below((uint32_t)p.entries + 1), 4, values[r.below(6)]);
            break;
        }
        case 4: {                                                                              // huge dimensions
            const uint32_t values[6] = {0, 1, 65535, 1u << 20, 0x7fffffffu, 0xffffffffu};
            set_le(d, 8, 4, values[r.below(6)]);
            set_le(d, 12, 4, values[r.below(6)]);
            break;
        }
        default: for (int i = r.range(1, 63); i > 0; --i) d.push_back((unsigned char)r.below(256)); break;
    }
    return d;
}

// ---- files the format allows and no encoder of ours writes
struct BitSink {
    Bytes& out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint64_t v, int bits) {
        acc |= v << n;
        n += bits;
        while (n >= 8) { out.push_back((unsigned char)acc); acc >>= 8; n -= 8; }
    }
    void pad(unsigned fill) { if (n) put(fill & ((1u << (8 - n)) - 1u), 8 - n); }
};
static unsigned zigzag_of(unsigned a, unsigned pred, int bits) {   // the field a sample leaves behind its predictor
    const unsigned mask = (1u << bits) - 1u, u = (a - pred) & mask;
    const long long d = (u >> (bits - 1)) ? (long long)u - (long long)mask - 1 : (long long)u;
    return d >= 0 ? (unsigned)(2 * d) : (unsigned)(-2 * d - 1);
}
static int width_of(unsigned v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }
static Bytes assemble(const Geo& g, const std::vector<Bytes>& parts) {
    const size_t entries = parts.size(), table_end = 32 + 4 * (entries + 1), start = (table_end + 15) / 16 * 16;
    Bytes f(start, 0);
    memcpy(f.data(), "KBNFRM1", 8);
    set_le(f, 8, 4, (uint64_t)g.w); set_le(f, 12, 4, (uint64_t)g.h); set_le(f, 16, 2, (uint64_t)g.c); set_le(f, 18, 2, (uint64_t)g.bits);
    set_le(f, 20, 2, 8); set_le(f, 22, 2, 16);
    size_t at = 0;
    for (size_t e = 0; e < entries; ++e) { set_le(f, 32 + 4 * e, 4, at); at += parts[e].size(); f.insert(f.end(), parts[e].begin(), parts[e].end()); }
    set_le(f, 32 + 4 * entries, 4, at);
    set_le(f, 24, 8, at);
    return f;
}
// mode 0: the canonical file (must equal the library's); 1: every b = bits; 2: b random in [needed, bits] and random pad bits
static Bytes build_from_samples(const Bytes& s, const Geo& g, int mode, Rng& r) {
    const size_t groups = ((size_t)g.h + 7) / 8, segments = ((size_t)g.w + 15) / 16;
    std::vector<Bytes> parts;
    for (size_t grp = 0; grp < groups; ++grp)
        for (int plane = 0; plane < g.c; ++plane) {
            const int rows = (int)std::min<size_t>(8, (size_t)g.h - grp * 8);
            Bytes heads, data;
            BitSink sink{data};
            for (int row = 0; row < rows; ++row)
                for (size_t k = 0; k < segments; ++k) {
                    const int n = (int)std::min<size_t>(16, (size_t)g.w - k * 16);
                    const size_t y = grp * 8 + row;
                    unsigned z[16], most = 0;
                    for (int i = row == 0 ? 1 : 0; i < n; ++i) {
                        const size_t x = k * 16 + i;
                        const unsigned a = get_sample(s, g, (y * g.w + x) * g.c + plane);
                        const unsigned pred = row == 0 ? get_sample(s, g, (y * g.w + x - 1) * g.c + plane) : get_sample(s, g, ((y - 1) * g.w + x) * g.c + plane);
                        z[i] = zigzag_of(a, pred, g.bits);
                        most |= z[i];
                    }
                    const int needed = width_of(most);
                    const int b = mode == 0 ? needed : (mode == 1 ? g.bits : r.range(needed, g.bits));
                    heads.push_back((unsigned char)b);
                    if (row == 0) sink.put(get_sample(s, g, (y * g.w + k * 16) * g.c + plane), g.bits);
                    for (int i = row == 0 ? 1 : 0; i < n; ++i) sink.put(z[i], b);
                    sink.pad(mode == 2 ? (unsigned)r.next() : 0u);
                }
            heads.insert(heads.end(), data.begin(), data.end());
            parts.push_back(heads);
        }
    return assemble(g, parts);
}
// random header bytes in [0, bits], every field and pad bit random, the table from the segments' sizes
// `illegal` > 0: one header byte is `illegal` (above `bits`) instead, its segment sized as frame_pack.h sizes it: a file that must be refused
static Bytes build_random(const Geo& g, Rng& r, int illegal = 0) {
    const size_t groups = ((size_t)g.h + 7) / 8, segments = ((size_t)g.w + 15) / 16;
    std::vector<Bytes> parts;
    const size_t bad_part = r.below((uint32_t)(groups * g.c));
    for (size_t grp = 0; grp < groups; ++grp)
        for (int plane = 0; plane < g.c; ++plane) {
            const int rows = (int)std::min<size_t>(8, (size_t)g.h - grp * 8);
            Bytes part;
            size_t bytes = 0;
            const size_t bad = illegal && parts.size() == bad_part ? r.below((uint32_t)(rows * segments)) : (size_t)-1;
            for (int row = 0; row < rows; ++row)
                for (size_t k = 0; k < segments; ++k) {
                    const int b = part.size() == bad ? illegal : r.range(0, g.bits);
                    part.push_back((unsigned char)b);
                    bytes += seg_bytes((int)std::min<size_t>(16, (size_t)g.w - k * 16), b, g.bits, row == 0);
                }
            for (size_t i = 0; i < bytes; ++i) part.push_back((unsigned char)r.below(256));
            parts.push_back(part);
        }
    return assemble(g, parts);
}

static void fuzz_frames(int scale) {
    const int n_geos = (int)(sizeof GEOS / sizeof GEOS[0]);
    for (int gi = 0; gi < n_geos; ++gi)
        for (int content = 0; content < 4; ++content) {
            const Geo g = GEOS[gi];
            g_seed = 1000 + 10 * gi + content;
            g_iteration = 0;
            Rng r(g_seed);
            const Bytes samples = make_content(g, content, r);
            g_stage = "packed: encode and its bound";
            const Bytes file = encode(samples, g);
            REQUIRE(file == build_from_samples(samples, g, 0, r), "the canonical builder of this program and kbn_frame_encode disagree");
            REQUIRE(frame_properties(file, &samples, true), "an encoded frame is refused");
            g_stage = "packed: structure-aware mutations";
            structural(file, g, r);
            g_stage = "packed: byte mutations";
            const Parsed p = parse(file, g);
            for (int i = 0; i < 15 * scale; ++i) { ++g_iteration; frame_properties(frame_mutate_bytes(file, p, r)); }
            g_stage = "packed: accepted non-canonical files";
            for (int i = 0; i < 3 * scale; ++i) {
                ++g_iteration;
                const Bytes wide = build_from_samples(samples, g, 1 + i % 2, r);
                frame_properties(wide, &samples, true);
                frame_properties(build_random(g, r), nullptr, true);
                g_noncanonical += 2;
                const int too_wide[6] = {255, 64, 33, 32, 31, g.bits + 1};      // the widest first: fields a 64-bit reader cannot hold
                if (i % 4 == 0) frame_properties(build_random(g, r, too_wide[i / 4 % 6]), nullptr, false, true), ++g_illegal;
            }
        }
    g_stage = "packed: files with a header byte above their bits";
    REQUIRE(g_illegal_accepted == 0, "%lld of %lld files with a header byte above their bits were accepted", g_illegal_accepted, g_illegal);
}

// ================================================================================================ PNG
static long long g_png_decoded = 0, g_png_refused = 0, g_png_deep_decoded = 0, g_png_deep = 0;

// one file through kbn_png_info and kbn_png_decode, `pixels_bytes` exactly the need, one less, or a random smaller value
static bool png_properties(const Bytes& file, Rng& r) {
    Block f(file);
    int w = -1, h = -1, c = -1, depth = -1;
    const int informed = kbn_png_info(f.p, f.n, &w, &h, &c, &depth);
    if (informed != KBN_OK) {
        Block out(64);
        REQUIRE(kbn_png_decode(f.p, f.n, out.p, out.n) != KBN_OK, "kbn_png_decode accepts a file kbn_png_info refuses");
        REQUIRE(out.all(0xA5), "kbn_png_decode wrote for a file kbn_png_info refuses");
        ++g_png_refused;
        return false;
    }
    REQUIRE(w >= 1 && h >= 1 && w <= 32767 && h <= 32767 && (c == 1 || c == 3 || c == 4) && (depth == 8 || depth == 16), "kbn_png_info: %d x %d x %d, depth %d", w, h, c, depth);
    const unsigned long long need = (unsigned long long)w * h * c * (depth / 8);
    const int mode = need > (1ull << 24) ? 2 : (int)r.below(4);       // huge headers over small files: never allocate what they ask for
    if (mode >= 2) {                                                  // too small an output: refused, nothing written
        const size_t size = mode == 2 ? (size_t)r.below((uint32_t)std::min<unsigned long long>(need, 4096)) : (size_t)need - 1;
        Block out(size);
        REQUIRE(kbn_png_decode(f.p, f.n, out.p, out.n) != KBN_OK, "kbn_png_decode accepts pixels_bytes %zu below the need %llu", size, need);
        REQUIRE(out.all(0xA5), "a kbn_png_decode refused for its pixels_bytes wrote");
        ++g_png_refused;
        return false;
    }
    Block out((size_t)need);
    const int rc = kbn_png_decode(f.p, f.n, out.p, out.n);
    if (rc == KBN_OK) {
        Block again((size_t)need, 0x5A);                               // every pixel written: a second decode over another fill agrees
        REQUIRE(kbn_png_decode(f.p, f.n, again.p, again.n) == KBN_OK && memcmp(again.p, out.p, out.n) == 0, "kbn_png_decode left pixels unwritten");
    }
    ++(rc == KBN_OK ? g_png_decoded : g_png_refused);
    return rc == KBN_OK;
}

static void fuzz_png(const std::vector<Bytes>& files, int scale) {
    for (size_t fi = 0; fi < files.size(); ++fi) {
        g_seed = 5000 + fi;
        g_iteration = 0;
        Rng r(g_seed);
        g_stage = "png: the fixture as it is";
        const Png png = png_parse(files[fi]);
        {
            Block f(files[fi]);
            int w, h, c, depth;
            REQUIRE(kbn_png_info(f.p, f.n, &w, &h, &c, &depth) == KBN_OK, "a fixture is refused");
            Block a((size_t)w * h * c * (depth / 8)), b(a.n);
            REQUIRE(kbn_png_decode(f.p, f.n, a.p, a.n) == KBN_OK, "a fixture is refused");
            Block rebuilt(png_build(png));                               // the rebuilt file is the same picture
            REQUIRE(kbn_png_decode(rebuilt.p, rebuilt.n, b.p, b.n) == KBN_OK && memcmp(a.p, b.p, a.n) == 0, "a rebuilt fixture decodes differently");
        }
        g_stage = "png: byte mutations";
        for (int i = 0; i < 12 * scale; ++i) { ++g_iteration; png_properties(png_mutate_bytes(files[fi], r), r); }
        g_stage = "png: filter types 0 .. 255 behind the checksums";
        for (int kind = 0; kind < 2; ++kind)
            for (int v = 0; v < 256; ++v) { ++g_iteration; ++g_png_deep; g_png_deep_decoded += png_properties(png_mutate_deep(png, kind, v, r), r); }
        g_stage = "png: scanline and IHDR mutations behind the checksums";
        for (int i = 0; i < 6 * scale; ++i) {
            ++g_iteration;
            ++g_png_deep;
            g_png_deep_decoded += png_properties(png_mutate_deep(png, 2 + (int)r.below(PNG_DEEP_KINDS - 2), (int)r.below(256), r), r);
        }
    }
}

// the three encoders: blocks of exactly their bound, every level, decoded again; one byte less is refused
static void png_encoders() {
    g_stage = "png: encoders";
    g_seed = 9000;
    g_iteration = 0;
    Rng r(g_seed);
    const int shapes[8][2] = {{1, 1}, {3, 1}, {2, 1300}, {97, 33}, {1, 3}, {1300, 2}, {33, 97}, {16, 16}};      // width, height
    for (const auto& shape : shapes)
        for (int kind = 0; kind < 3; ++kind)             // gray16, rgb8, gray8
            for (int content = 0; content < 2; ++content)
                for (int level = -1; level <= 9; ++level) {
                    ++g_iteration;
                    const int w = shape[0], h = shape[1];
                    const size_t bytes = (size_t)w * h * (kind == 0 ? 2 : (kind == 1 ? 3 : 1));
                    Block pixels(bytes, 0x3C);
                    if (content == 0) for (size_t i = 0; i < bytes; ++i) pixels.p[i] = (unsigned char)r.below(256);
                    const size_t bound = kind == 0 ? kbn_png_encode_gray16_bound(w, h) : (kind == 1 ? kbn_png_encode_rgb8_bound(w, h) : kbn_png_encode_gray8_bound(w, h));
                    REQUIRE(bound != 0, "a PNG encoder's bound is 0 for %d x %d", w, h);
                    auto run = [&](unsigned char* out, size_t capacity, size_t* n) {
                        return kind == 0 ? kbn_png_encode_gray16((const unsigned short*)pixels.p, w, h, out, capacity, n, level)
                             : kind == 1 ? kbn_png_encode_rgb8(pixels.p, w, h, out, capacity, n, level) : kbn_png_encode_gray8(pixels.p, w, h, out, capacity, n, level);
                    };
                    Block out(bound);
                    size_t n = (size_t)-1;
                    int rc = run(out.p, bound, &n);
                    REQUIRE(rc == KBN_OK && n <= bound, "PNG encoder %d, level %d, %d x %d: status %d, %zu bytes, bound %zu", kind, level, w, h, rc, n, bound);
                    Block small(bound - 1);
                    size_t m = 12345;
                    rc = run(small.p, bound - 1, &m);
                    REQUIRE(rc == KBN_ERR_WORKSPACE && m == 12345 && small.all(0xA5), "PNG encoder %d with capacity bound - 1: status %d", kind, rc);
                    Block file(Bytes(out.p, out.p + n)), back(bytes);
                    int iw, ih, ic, id;
                    REQUIRE(kbn_png_info(file.p, file.n, &iw, &ih, &ic, &id) == KBN_OK && iw == w && ih == h && ic == (kind == 1 ? 3 : 1) && id == (kind == 0 ? 16 : 8),
                            "PNG encoder %d: kbn_png_info of its file disagrees", kind);
                    rc = kbn_png_decode(file.p, file.n, back.p, back.n);
                    REQUIRE(rc == KBN_OK && memcmp(back.p, pixels.p, bytes) == 0, "PNG encoder %d, level %d, %d x %d: the file decodes differently (status %d)", kind, level, w, h, rc);
                }
    // levels outside the ABI's are refused
    unsigned char px[6] = {0}, out[256];
    size_t n;
    REQUIRE(kbn_png_encode_gray8(px, 1, 1, out, sizeof out, &n, 10) != KBN_OK && kbn_png_encode_gray8(px, 1, 1, out, sizeof out, &n, -2) != KBN_OK, "a level outside -1 .. 9 is accepted");
}

int main(int argc, char** argv) {
    g_program = "codec_fuzz";
    setvbuf(stdout, nullptr, _IOLBF, 0);
    __sanitizer_set_death_callback(on_death);
    int scale = 100;
    std::vector<Bytes> pngs;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--scale") && i + 1 < argc) scale = atoi(argv[++i]);
        else pngs.push_back(read_file(argv[i]));
    }
    if (scale < 1) scale = 1;
    fuzz_frames(scale);
    const long long frames = g_accepted + g_refused;
    printf("codec_fuzz packed: %lld inputs, %lld accepted (%lld of them non-canonical by construction), %lld refused\n", frames, g_accepted, g_noncanonical, g_refused);
    g_stage = "packed: the share of accepted inputs";
    REQUIRE(10 * g_accepted >= frames, "fewer than a tenth of the inputs were accepted");
    if (!pngs.empty()) {
        fuzz_png(pngs, scale);
        png_encoders();
        printf("codec_fuzz png: %zu fixtures, %lld inputs, %lld decoded, %lld refused; behind the checksums %lld inputs, %lld decoded; %lld encoder cases\n", pngs.size(),
               g_png_decoded + g_png_refused, g_png_decoded, g_png_refused, g_png_deep, g_png_deep_decoded, g_iteration);
        g_stage = "png: the share of inputs that reach the unfilter code";
        REQUIRE(g_png_deep_decoded * 20 >= g_png_deep, "fewer than a twentieth of the deep mutants decoded");
    } else {
        printf("codec_fuzz png: no fixture given, skipped\n");
    }
    printf("codec_fuzz: ok\n");
    return 0;
}
