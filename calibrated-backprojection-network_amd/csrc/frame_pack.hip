// frame_pack.hip -- HOST side of the packed frame store: the container the loaders read in place of PNG files, whose
// decoding is data-parallel (csrc/unpack_packed.hip decodes it on the device).  No GPU work here: kbn_frame_info, kbn_frame_encode
// (+ _bound), kbn_frame_decode and kbn_frame_check, all thread-safe.  The layout is written down in frame_pack.h.
//
// kbn_frame_check is the gate between a file and the device decoder: after it has accepted a file, every address that decoder
// derives from the file's table and header bytes lies inside the file, whatever the field bits hold.
#include <cstring>
#include <vector>

#include "frame_pack.h"
#include "kbn_common.h"

namespace kbn {
namespace fp {

static const unsigned char MAGIC[8] = {'K', 'B', 'N', 'F', 'R', 'M', '1', 0};

static inline uint32_t rd16(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t rd32(const unsigned char* p) { return rd16(p) | rd16(p + 2) << 16; }
static inline uint64_t rd64(const unsigned char* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
static inline void wr16(unsigned char* p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); }
static inline void wr32(unsigned char* p, uint32_t v) { wr16(p, v); wr16(p + 2, v >> 16); }
static inline void wr64(unsigned char* p, uint64_t v) { wr32(p, (uint32_t)v); wr32(p + 4, (uint32_t)(v >> 32)); }

struct Layout {
    int w, h, c, bits;
    uint64_t payload_bytes, groups, segments /* of a row */, start /* of the payload */;
};

static bool geometry_ok(long long w, long long h, int c, int bits) {
    return w >= 1 && h >= 1 && w <= 0x7fffffffLL && h <= 0x7fffffffLL && (c == 1 || c == 3 || c == 4) && (bits == 8 || bits == 16);
}

static void fill_layout(Layout& L, int w, int h, int c, int bits) {
    L.w = w; L.h = h; L.c = c; L.bits = bits;
    L.groups = ((uint64_t)h + FP_ROWS - 1) / FP_ROWS;
    L.segments = ((uint64_t)w + FP_SEG - 1) / FP_SEG;
    L.start = payload_start(L.groups, (unsigned)c);
}

static int parse_header(const unsigned char* file, size_t file_bytes, Layout& L) {
    if (!file || file_bytes < (size_t)FP_HEADER) return KBN_ERR_INVALID_ARGUMENT;
    if (std::memcmp(file, MAGIC, 8) != 0) return KBN_ERR_INVALID_ARGUMENT;
    const uint32_t w = rd32(file + 8), h = rd32(file + 12), c = rd16(file + 16), bits = rd16(file + 18);
    if (rd16(file + 20) != (uint32_t)FP_ROWS || rd16(file + 22) != (uint32_t)FP_SEG) return KBN_ERR_UNSUPPORTED;
    if (w < 1 || h < 1 || w > 0x7fffffffu || h > 0x7fffffffu) return KBN_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(w, h, (int)c, (int)bits)) return KBN_ERR_UNSUPPORTED;
    fill_layout(L, (int)w, (int)h, (int)c, (int)bits);
    L.payload_bytes = rd64(file + 24);
    return KBN_OK;
}

template <typename T>
static inline int residual(T a, T pred, int bits) {   // the signed representative of a - pred mod 2^bits
    const unsigned mask = (1u << bits) - 1u;
    const unsigned u = ((unsigned)a - (unsigned)pred) & mask;
    return u >> (bits - 1) ? (int)u - (int)(mask + 1u) : (int)u;
}

static inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

struct BitWriter {
    unsigned char* p;
    uint64_t acc = 0;
    int n = 0;
    void put(unsigned v, int bits) {
        acc |= (uint64_t)v << n;
        n += bits;
        while (n >= 8) { *p++ = (unsigned char)acc; acc >>= 8; n -= 8; }
    }
    void pad() { if (n) { *p++ = (unsigned char)acc; acc = 0; n = 0; } }
};

struct BitReader {
    const unsigned char* p;
    uint64_t acc = 0;
    int n = 0;
    unsigned get(int bits) {   // the caller stays inside the segment: kbn_frame_check has sized it
        while (n < bits) { acc |= (uint64_t)*p++ << n; n += 8; }
        const unsigned v = (unsigned)(acc & ((1ull << bits) - 1ull));
        acc >>= bits; n -= bits;
        return v;
    }
};

template <typename T>
static size_t encode_plane_group(const T* samples, const Layout& L, uint64_t g, int plane, unsigned char* out) {
    const int rows = (int)std::min<uint64_t>(FP_ROWS, (uint64_t)L.h - g * FP_ROWS);
    const size_t pitch = (size_t)L.w * L.c;
    unsigned char* head = out;
    BitWriter bw{out + (size_t)rows * L.segments};
    unsigned z[FP_SEG];
    for (int r = 0; r < rows; ++r) {
        const T* row = samples + (g * FP_ROWS + r) * pitch + plane;
        for (uint64_t k = 0; k < L.segments; ++k) {
            const int n = (int)std::min<uint64_t>(FP_SEG, (uint64_t)L.w - k * FP_SEG);
            const T* s = row + k * FP_SEG * L.c;
            unsigned most = 0;
            for (int i = r == 0 ? 1 : 0; i < n; ++i) {
                const T pred = r == 0 ? s[(size_t)(i - 1) * L.c] : *(s + (size_t)i * L.c - pitch);
                z[i] = zigzag(residual<T>(s[(size_t)i * L.c], pred, L.bits));
                most |= z[i];
            }
            const int b = bit_length(most);
            *head++ = (unsigned char)b;
            if (r == 0) bw.put(s[0], L.bits);
            if (b)
                for (int i = r == 0 ? 1 : 0; i < n; ++i) bw.put(z[i], b);
            bw.pad();
        }
    }
    return (size_t)(bw.p - out);
}

template <typename T>
static void decode_plane_group(const unsigned char* in, const Layout& L, uint64_t g, int plane, T* samples) {
    const int rows = (int)std::min<uint64_t>(FP_ROWS, (uint64_t)L.h - g * FP_ROWS);
    const size_t pitch = (size_t)L.w * L.c;
    const unsigned mask = (1u << L.bits) - 1u;
    const unsigned char* head = in;
    const unsigned char* data = in + (size_t)rows * L.segments;
    for (int r = 0; r < rows; ++r) {
        T* row = samples + (g * FP_ROWS + r) * pitch + plane;
        for (uint64_t k = 0; k < L.segments; ++k) {
            const int n = (int)std::min<uint64_t>(FP_SEG, (uint64_t)L.w - k * FP_SEG);
            const int b = *head++;
            T* s = row + k * FP_SEG * L.c;
            BitReader br{data};
            if (r == 0) s[0] = (T)br.get(L.bits);
            for (int i = r == 0 ? 1 : 0; i < n; ++i) {
                const int d = b ? unzigzag(br.get(b)) : 0;
                const unsigned pred = r == 0 ? s[(size_t)(i - 1) * L.c] : *(s + (size_t)i * L.c - pitch);
                s[(size_t)i * L.c] = (T)((pred + (unsigned)d) & mask);
            }
            data += segment_bytes(n, b, L.bits, r == 0);
        }
    }
}

static int check_file(const unsigned char* file, size_t file_bytes, Layout& L) {
    const int st = parse_header(file, file_bytes, L);
    if (st != KBN_OK) return st;
    if (L.start > file_bytes || L.payload_bytes != file_bytes - L.start || L.payload_bytes > 0xffffffffull) return KBN_ERR_INVALID_ARGUMENT;
    const uint64_t entries = L.groups * L.c;
    for (uint64_t at = FP_HEADER + 4 * (entries + 1); at < L.start; ++at)
        if (file[at]) return KBN_ERR_INVALID_ARGUMENT;
    const unsigned char* table = file + FP_HEADER;
    const unsigned char* payload = file + L.start;
    if (rd32(table) != 0 || rd32(table + 4 * entries) != L.payload_bytes) return KBN_ERR_INVALID_ARGUMENT;
    const int last_n = (int)((uint64_t)L.w - (L.segments - 1) * FP_SEG);
    for (uint64_t e = 0; e < entries; ++e) {
        const uint64_t lo = rd32(table + 4 * e), hi = rd32(table + 4 * (e + 1));
        if (lo > hi || hi > L.payload_bytes) return KBN_ERR_INVALID_ARGUMENT;
        const uint64_t g = e / L.c;
        const uint64_t rows = std::min<uint64_t>(FP_ROWS, (uint64_t)L.h - g * FP_ROWS);
        const uint64_t heads = rows * L.segments;
        if (hi - lo < heads) return KBN_ERR_INVALID_ARGUMENT;
        const unsigned char* head = payload + lo;
        uint64_t bytes = heads;
        for (uint64_t r = 0; r < rows; ++r)
            for (uint64_t k = 0; k < L.segments; ++k) {
                const int b = *head++;
                if (b > L.bits) return KBN_ERR_INVALID_ARGUMENT;
                bytes += segment_bytes(k + 1 == L.segments ? last_n : FP_SEG, b, L.bits, r == 0);
            }
        if (bytes != hi - lo) return KBN_ERR_INVALID_ARGUMENT;
    }
    return KBN_OK;
}

}  // namespace fp
}  // namespace kbn

extern "C" int kbn_frame_info(const unsigned char* file, size_t file_bytes, int* width, int* height, int* channels, int* bits) {
    using namespace kbn::fp;
    if (!width || !height || !channels || !bits) return KBN_ERR_INVALID_ARGUMENT;
    Layout L;
    const int st = parse_header(file, file_bytes, L);
    if (st != KBN_OK) return st;
    *width = L.w; *height = L.h; *channels = L.c; *bits = L.bits;
    return KBN_OK;
}

extern "C" size_t kbn_frame_encode_bound(int width, int height, int channels, int bits) {
    using namespace kbn::fp;
    if (!geometry_ok(width, height, channels, bits)) return 0;
    Layout L;
    fill_layout(L, width, height, channels, bits);
    // a header byte a segment, and no segment takes more than its samples do raw
    const uint64_t row = L.segments + ((uint64_t)width * bits + 7) / 8 + L.segments;
    const unsigned __int128 bound = (unsigned __int128)row * (uint64_t)height * channels + L.start;   // past 64 bits for sides near 2^31
    return bound > KBN_MAX_SIZE_BYTES ? 0 : (size_t)bound;
}

extern "C" int kbn_frame_encode(const void* samples, int width, int height, int channels, int bits, unsigned char* out,
                                size_t out_capacity, size_t* out_bytes) {
    using namespace kbn::fp;
    if (!samples || !out || !out_bytes) return KBN_ERR_INVALID_ARGUMENT;
    if (width < 1 || height < 1) return KBN_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(width, height, channels, bits)) return KBN_ERR_UNSUPPORTED;
    const size_t bound = kbn_frame_encode_bound(width, height, channels, bits);
    if (bound == 0) return KBN_ERR_UNSUPPORTED;              // no size_t holds it: 0 is a refusal, not "any capacity will do"
    if (out_capacity < bound) return KBN_ERR_WORKSPACE;
    if (bound > 0xffffffffull) return KBN_ERR_UNSUPPORTED;   // the table's offsets are 32-bit
    Layout L;
    fill_layout(L, width, height, channels, bits);
    std::memset(out, 0, (size_t)L.start);
    std::memcpy(out, MAGIC, 8);
    wr32(out + 8, (uint32_t)width); wr32(out + 12, (uint32_t)height);
    wr16(out + 16, (uint32_t)channels); wr16(out + 18, (uint32_t)bits);
    wr16(out + 20, FP_ROWS); wr16(out + 22, FP_SEG);
    unsigned char* payload = out + L.start;
    size_t at = 0;
    uint64_t e = 0;
    for (uint64_t g = 0; g < L.groups; ++g)
        for (int plane = 0; plane < channels; ++plane, ++e) {
            wr32(out + FP_HEADER + 4 * e, (uint32_t)at);
            at += bits == 16 ? encode_plane_group(static_cast<const unsigned short*>(samples), L, g, plane, payload + at)
                             : encode_plane_group(static_cast<const unsigned char*>(samples), L, g, plane, payload + at);
        }
    wr32(out + FP_HEADER + 4 * e, (uint32_t)at);
    wr64(out + 24, at);
    *out_bytes = (size_t)L.start + at;
    return KBN_OK;
}

extern "C" int kbn_frame_check(const unsigned char* file, size_t file_bytes) {
    kbn::fp::Layout L;
    return kbn::fp::check_file(file, file_bytes, L);
}

extern "C" int kbn_frame_decode(const unsigned char* file, size_t file_bytes, void* samples, size_t samples_bytes) {
    using namespace kbn::fp;
    if (!samples) return KBN_ERR_INVALID_ARGUMENT;
    Layout L;
    const int st = check_file(file, file_bytes, L);
    if (st != KBN_OK) return st;
    if (samples_bytes < (uint64_t)L.w * L.h * L.c * (L.bits / 8)) return KBN_ERR_INVALID_ARGUMENT;
    uint64_t e = 0;
    for (uint64_t g = 0; g < L.groups; ++g)
        for (int plane = 0; plane < L.c; ++plane, ++e) {
            const unsigned char* in = file + L.start + rd32(file + FP_HEADER + 4 * e);
            if (L.bits == 16) decode_plane_group(in, L, g, plane, static_cast<unsigned short*>(samples));
            else decode_plane_group(in, L, g, plane, static_cast<unsigned char*>(samples));
        }
    return KBN_OK;
}
