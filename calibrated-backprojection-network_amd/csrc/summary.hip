// summary.hip -- the training loop's image summaries (kbn_summary_panel_forward): one launch writes one finished panel of the
// reference's KBNetModel.log_summary (src/kbnet_model.py:417-650), i.e. the 3 x Hg x Wg fp32 tensor that
//     torchvision.utils.make_grid(torch.cat(rows, dim=2), nrow=n_display)
// returns, where every row is torch.cat([left, right], dim=3) of two N x 3 x H x W cells.  The reference copies each tensor to the
// host, colourises frame by frame through matplotlib, concatenates on the CPU and builds the grid there.
//
// Layout.  `frames` (B) tiles of 3 x (R H) x (2 W) side by side, R rows of a left and a right cell each.  B > 1: make_grid's
// padding = 2, pad_value = 0 -- the panel is 3 x (R H + 4) x (B (2 W + 2) + 2), tile k at row 2, column k (2 W + 2) + 2, everything
// else 0.  B == 1: the tile itself (torchvision returns a single image as it is).  The kernel writes EVERY element of the panel,
// padding and zero cells included: no memset, no second launch.
//
// Cells (reference expressions, each operation rounded on its own in fp32; no fast-math flag on this file, IEEE division):
//   COPY        a 3-channel image as it is
//   ZERO        0
//   PHOTO_ERR   inferno(x), x = (((|a0 - b0| + |a1 - b1|) + |a2 - b2|) / 3) / 0.10f       a, b 3-channel images
//   DEPTH       viridis(d / max_predict_depth)                                           d a 1-channel map
//   REL_ERR     inferno(x), x = (v == 1 ? (|out - ref| + 1e-8f) / (ref + 1e-8f) : v) / 0.05f       out, ref, v 1-channel maps
// Colour lookup = matplotlib's Colormap.__call__ on float32 data: t = x * 256 in fp32; t < 0 -> entry 0; t >= 256 (+inf too) ->
// entry 255; otherwise entry (int)t; NaN -> (0, 0, 0).  The two 256 x 3 tables (colormaps.h, generated from matplotlib) are staged
// into LDS once a workgroup (6 KB): the lookups diverge across the lanes of a wave.  The cell records follow them there (1 KB): a
// lane picks its cell, left or right, by an index of its own.
//
// Work.  An item is four consecutive pixels of one cell row when W % 4 == 0 (else one pixel), all three channels; a cell whose
// sources have unit element stride, strides that are multiples of 4 and 16-byte aligned pointers reads them with 16-byte loads, any
// other cell with scalar loads.  The panel's columns start at 2 (mod 2 W + 2), so its stores are 16-, 8- or 4-byte ones by the
// address.  A panel row is a run of 256-item chunks; the workgroups stride over all chunks of all rows.  The row records (source
// pointers and strides) travel BY VALUE in the kernel arguments: no device table, no allocation, no host synchronisation.
#include <math.h>

#include "colormaps.h"
#include "kbn_common.h"

namespace kbn {

constexpr int SUM_THREADS = 256;
constexpr int SUM_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups: each stages the tables once and strides over the chunks

enum { CELL_ZERO = KBN_SUMMARY_CELL_ZERO, CELL_COPY = KBN_SUMMARY_CELL_COPY, CELL_PHOTO_ERR = KBN_SUMMARY_CELL_PHOTO_ERR,
       CELL_DEPTH = KBN_SUMMARY_CELL_DEPTH, CELL_REL_ERR = KBN_SUMMARY_CELL_REL_ERR };

struct SumSource {
    const float* data;
    long long sn, sc, sh, sw;   // element strides
};
struct SumCell {
    SumSource src[3];
    int kind;
    int vec;   // 16-byte loads: see the file comment
};
struct SumParams {
    SumCell cell[KBN_SUMMARY_MAX_ROWS][2];   // [row][left, right]
    float* panel;
    int rows, frames, height, width;
    int pad;                    // 2 when frames > 1, else 0
    int panel_height, panel_width;
    float max_predict_depth;
};
static_assert(sizeof(SumParams) <= 3584, "the records must fit the kernel-argument segment");

// matplotlib's Colormap.__call__ for one float32 value -> the entry's offset in a table, or -1 for NaN (the "bad" colour, 0 0 0)
__device__ __forceinline__ int colormap_entry(float x) {
    const float t = __fmul_rn(x, 256.0f);
    if (t != t) return -1;
    if (t < 0.f) return 0;
    if (t >= 256.f) return COLORMAP_ENTRIES - 1;
    return (int)t;
}

// PIX pixels (4 with 16-byte loads where the cell allows, else scalar loads) of channel `c` of frame `b`, row y, from column x
template <int PIX>
__device__ __forceinline__ void load_pixels(const SumSource& s, bool vec, int b, int c, int y, int x, float (&v)[PIX]) {
    const float* row = s.data + (long long)b * s.sn + (long long)c * s.sc + (long long)y * s.sh;
    if constexpr (PIX == 4) {
        if (vec) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(row + x);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < PIX; ++i) v[i] = row[(long long)(x + i) * s.sw];
}

// PIX consecutive values of one panel row: the widest stores the address allows
template <int PIX>
__device__ __forceinline__ void store_pixels(float* dst, const float (&v)[PIX]) {
    if constexpr (PIX == 4) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
        if ((a & 15) == 0) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        } else if ((a & 7) == 0) {
            *reinterpret_cast<f32x2*>(dst) = f32x2{v[0], v[1]};
            *reinterpret_cast<f32x2*>(dst + 2) = f32x2{v[2], v[3]};
        } else {
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
    } else {
        dst[0] = v[0];
    }
}

// One item: PIX pixels of cell `cl` (frame b, cell row y, from cell column x) -> the three channel planes at dst
template <int PIX>
__device__ __forceinline__ void cell_item(const SumParams& p, const SumCell& cl, const float* lut, int b, int y, int x, float* dst,
                                          long long plane) {
    float out[3][PIX];
    if (cl.kind == CELL_ZERO) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < PIX; ++i) out[c][i] = 0.f;
    } else if (cl.kind == CELL_COPY) {
#pragma unroll
        for (int c = 0; c < 3; ++c) load_pixels<PIX>(cl.src[0], cl.vec, b, c, y, x, out[c]);
    } else {
        float value[PIX];
        const float* table = lut;   // viridis first, inferno behind it
        if (cl.kind == CELL_DEPTH) {
            float d[PIX];
            load_pixels<PIX>(cl.src[0], cl.vec, b, 0, y, x, d);
#pragma unroll
            for (int i = 0; i < PIX; ++i) value[i] = __fdiv_rn(d[i], p.max_predict_depth);
        } else if (cl.kind == CELL_PHOTO_ERR) {
            table = lut + COLORMAP_ENTRIES * 3;
            float sum[PIX];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float a[PIX], r[PIX];
                load_pixels<PIX>(cl.src[0], cl.vec, b, c, y, x, a);
                load_pixels<PIX>(cl.src[1], cl.vec, b, c, y, x, r);
#pragma unroll
                for (int i = 0; i < PIX; ++i) {
                    const float e = fabsf(__fsub_rn(a[i], r[i]));
                    sum[i] = c == 0 ? e : __fadd_rn(sum[i], e);
                }
            }
#pragma unroll
            for (int i = 0; i < PIX; ++i) value[i] = __fdiv_rn(__fdiv_rn(sum[i], 3.0f), 0.10f);
        } else {   // CELL_REL_ERR
            table = lut + COLORMAP_ENTRIES * 3;
            float o[PIX], r[PIX], m[PIX];
            load_pixels<PIX>(cl.src[0], cl.vec, b, 0, y, x, o);
            load_pixels<PIX>(cl.src[1], cl.vec, b, 0, y, x, r);
            load_pixels<PIX>(cl.src[2], cl.vec, b, 0, y, x, m);
#pragma unroll
            for (int i = 0; i < PIX; ++i) {
                const float rel = __fdiv_rn(__fadd_rn(fabsf(__fsub_rn(o[i], r[i])), 1e-8f), __fadd_rn(r[i], 1e-8f));
                value[i] = __fdiv_rn(m[i] == 1.0f ? rel : m[i], 0.05f);
            }
        }
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
            const int entry = colormap_entry(value[i]);
            const float* rgb = table + 3 * (entry < 0 ? 0 : entry);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c][i] = entry < 0 ? 0.f : rgb[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_pixels<PIX>(dst + c * plane, out[c]);
}

template <int PIX>
__global__ __launch_bounds__(SUM_THREADS) void summary_panel_kernel(const SumParams p) {
    __shared__ float lut[2 * COLORMAP_ENTRIES * 3];
    for (int i = threadIdx.x; i < COLORMAP_ENTRIES * 3; i += SUM_THREADS) {
        lut[i] = k_colormap_viridis[i];
        lut[COLORMAP_ENTRIES * 3 + i] = k_colormap_inferno[i];
    }
    // the cell records beside the tables: an item picks its cell by a per-lane index (left or right), which registers cannot serve
    __shared__ SumCell cells[KBN_SUMMARY_MAX_ROWS][2];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < KBN_SUMMARY_MAX_ROWS; ++r) { cells[r][0] = p.cell[r][0]; cells[r][1] = p.cell[r][1]; }
    }
    __syncthreads();
    const int W = p.width, H = p.height, Wg = p.panel_width, Hg = p.panel_height, pad = p.pad;
    const long long plane = (long long)Hg * Wg;
    const int cell_items = W / PIX;                   // items of one cell row
    const int tile_items = 2 * cell_items;            // of one tile row
    const int row_items = p.frames * tile_items + (pad ? p.frames + 1 : 0);   // + a two-column padding strip in front of each tile and behind the last
    const int pad_row_items = pad ? Wg : 0;           // a padding row: one pixel an item
    const int chunks_x = (max(row_items, pad_row_items) + SUM_THREADS - 1) / SUM_THREADS;
    const long long chunks = (long long)Hg * chunks_x;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int y = (int)(chunk / chunks_x);        // panel row: the same in every thread
        const int item = (int)(chunk - (long long)y * chunks_x) * SUM_THREADS + threadIdx.x;
        float* out_row = p.panel + (long long)y * Wg;
        if (y < pad || y >= Hg - pad) {               // make_grid's top and bottom padding rows
            if (item < pad_row_items) {
                out_row[item] = 0.f; out_row[plane + item] = 0.f; out_row[2 * plane + item] = 0.f;
            }
            continue;
        }
        if (item >= row_items) continue;
        const int ty = y - pad, r = ty / H, cy = ty - r * H;   // the tile's row -> cell row r, row cy inside it
        if (item < p.frames * tile_items) {
            const int b = item / tile_items, q = item - b * tile_items;
            const int side = q >= cell_items, cx = (q - side * cell_items) * PIX;
            float* dst = out_row + pad + (long long)b * (2 * W + pad) + side * W + cx;
            cell_item<PIX>(p, cells[r][side], lut, b, cy, cx, dst, plane);
        } else {                                      // the two padding columns in front of tile j (j == frames: behind the last tile)
            const int j = item - p.frames * tile_items;
            float* dst = out_row + (long long)j * (2 * W + pad);
#pragma unroll
            for (int c = 0; c < 3; ++c) { dst[c * plane] = 0.f; dst[c * plane + 1] = 0.f; }
        }
    }
}

// kb.summary.colorize: the lookup alone, n x 1 x H x W -> n x 3 x H x W (dense), one pixel a thread
__global__ __launch_bounds__(SUM_THREADS) void summary_colorize_kernel(const float* x, long long sn, long long sh, long long sw, int height,
                                                                       int width, int colormap, float* out) {
    __shared__ float lut[COLORMAP_ENTRIES * 3];
    const float* table = colormap == KBN_SUMMARY_COLORMAP_INFERNO ? k_colormap_inferno : k_colormap_viridis;
    for (int i = threadIdx.x; i < COLORMAP_ENTRIES * 3; i += SUM_THREADS) lut[i] = table[i];
    __syncthreads();
    const long long pixels = (long long)height * width;
    const float* frame = x + (long long)blockIdx.y * sn;
    float* dst = out + 3 * pixels * blockIdx.y;
    for (long long i = (long long)blockIdx.x * SUM_THREADS + threadIdx.x; i < pixels; i += (long long)gridDim.x * SUM_THREADS) {
        const long long y = i / width, xx = i - y * width;
        const int entry = colormap_entry(frame[y * sh + xx * sw]);
        const float* rgb = lut + 3 * (entry < 0 ? 0 : entry);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c * pixels + i] = entry < 0 ? 0.f : rgb[c];
    }
}

}  // namespace kbn

extern "C" {

int kbn_summary_colorize_forward(const float* x, long long stride_n, long long stride_h, long long stride_w, int n, int height, int width,
                                 int colormap, float* out, kbn_stream_t stream) {
    using namespace kbn;
    if (!x || !out || n < 1 || n > 65535 || height < 1 || width < 1 || stride_n < 0 || stride_h < 0 || stride_w < 0) return KBN_ERR_INVALID_ARGUMENT;
    if (colormap != KBN_SUMMARY_COLORMAP_VIRIDIS && colormap != KBN_SUMMARY_COLORMAP_INFERNO) return KBN_ERR_UNSUPPORTED;
    const long long blocks = ((long long)height * width + SUM_THREADS - 1) / SUM_THREADS;
    const dim3 grid((unsigned)std::min<long long>(blocks, std::max(1, SUM_MAX_BLOCKS / n)), (unsigned)n);
    hipLaunchKernelGGL(summary_colorize_kernel, grid, dim3(SUM_THREADS), 0, (hipStream_t)stream, x, stride_n, stride_h, stride_w, height, width,
                       colormap, out);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_summary_panel_forward(const kbn_summary_row* rows, int n_rows, int frames, int height, int width, float max_predict_depth,
                              float* panel, kbn_stream_t stream) {
    using namespace kbn;
    if (!rows || !panel || n_rows < 2 || n_rows > KBN_SUMMARY_MAX_ROWS || frames < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    const int pad = frames > 1 ? 2 : 0;
    const long long Hg = (long long)n_rows * height + 2 * pad, Wg = (long long)frames * (2ll * width + pad) + pad;
    if (3 * Hg * Wg > 0x7fffffffll) return KBN_ERR_UNSUPPORTED;   // items and panel columns are 32-bit
    if (max_predict_depth != max_predict_depth) return KBN_ERR_INVALID_ARGUMENT;
    SumParams p;
    p.panel = panel;
    p.rows = n_rows; p.frames = frames; p.height = height; p.width = width; p.pad = pad;
    p.panel_height = (int)Hg; p.panel_width = (int)Wg;
    p.max_predict_depth = max_predict_depth;
    for (int r = 0; r < KBN_SUMMARY_MAX_ROWS; ++r)
        for (int side = 0; side < 2; ++side) {
            SumCell& c = p.cell[r][side];
            c.kind = CELL_ZERO; c.vec = 0;
            for (SumSource& s : c.src) s = SumSource{nullptr, 0, 0, 0, 0};
            if (r >= n_rows) continue;
            const kbn_summary_cell& g = side ? rows[r].right : rows[r].left;
            // the left cell shows a tensor (an image or a colourised depth), the right one an error map or nothing
            const bool kind_fits = side ? (g.kind == CELL_ZERO || g.kind == CELL_PHOTO_ERR || g.kind == CELL_REL_ERR)
                                        : (g.kind == CELL_COPY || g.kind == CELL_DEPTH);
            if (!kind_fits) return KBN_ERR_INVALID_ARGUMENT;
            c.kind = g.kind;
            const int used = g.kind == CELL_ZERO ? 0 : g.kind == CELL_COPY || g.kind == CELL_DEPTH ? 1 : g.kind == CELL_PHOTO_ERR ? 2 : 3;
            const int channels = g.kind == CELL_COPY || g.kind == CELL_PHOTO_ERR ? 3 : 1;
            bool vec = width % 4 == 0;
            for (int i = 0; i < used; ++i) {
                const kbn_summary_source& s = g.src[i];
                if (!s.data || s.stride_n < 0 || s.stride_c < 0 || s.stride_h < 0 || s.stride_w < 0) return KBN_ERR_INVALID_ARGUMENT;
                if (s.channels != channels) return KBN_ERR_UNSUPPORTED;   // the reference's cat fails on these too
                c.src[i] = SumSource{s.data, s.stride_n, s.stride_c, s.stride_h, s.stride_w};
                vec = vec && s.stride_w == 1 && ((s.stride_n | s.stride_c | s.stride_h) & 3) == 0 && (reinterpret_cast<uintptr_t>(s.data) & 15) == 0;
            }
            c.vec = vec && used > 0;
        }
    const bool quads = width % 4 == 0;
    const long long tile_items = 2ll * (quads ? width / 4 : width);
    const long long row_items = std::max<long long>(frames * tile_items + (pad ? frames + 1 : 0), pad ? Wg : 0);   // as the kernel counts them
    const long long chunks = Hg * ((row_items + SUM_THREADS - 1) / SUM_THREADS);
    const dim3 grid((unsigned)std::min<long long>(chunks, SUM_MAX_BLOCKS));
    if (quads) hipLaunchKernelGGL(summary_panel_kernel<4>, grid, dim3(SUM_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(summary_panel_kernel<1>, grid, dim3(SUM_THREADS), 0, (hipStream_t)stream, p);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // extern "C"
