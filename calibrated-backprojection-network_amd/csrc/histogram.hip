// histogram.hip -- TensorBoard's default histogram (kbn_histogram_forward): what SummaryWriter.add_histogram(bins='tensorflow')
// computes on the host -- np.histogram(values.astype(float), bins=edges) with min, max, sum and values.dot(values) -- in one pass
// over an fp32 device tensor.  The reference's log_summary hands add_histogram image-sized tensors (the output depth, the sparse
// depth); the writer copies them to the host, waits for the device and histograms them in NumPy.
//
// Edges.  774 positive fp64 edges P[k] (1e-12 multiplied by 1.1 again and again; built by the caller, handed over as a device buffer),
// mirrored negative, 0 between: E[0 .. 1548], E[774] = 0, E[775 + k] = P[k], E[773 - k] = -P[k]; 1548 bins.  A value x, widened to
// fp64 (exact) and compared in fp64, is counted in bin i when E[i] <= x < E[i + 1]; the last bin is closed on the right; values
// outside [E[0], E[1548]], NaN and +-inf are counted nowhere.  With a = |x|:
//   x >= 0 (-0 too):  j  = #{k : P[k] <= a}                ->  bin 774 + j;   j  == 774: bin 1547 when a == P[773], else none
//   x <  0:           j' = #{k : P[k] <  a}                ->  bin 773 - j';  j' == 774: none
// Both counts come from one branch-free binary search (10 probes) of the table staged in LDS, so a value AT an edge lands where
// NumPy's comparison puts it.
//
// Plan.  Launch 1: a workgroup of 256 threads stages the table (6192 B) and clears 1548 integer bins (6192 B) in LDS, then strides
// over 16-byte quads of the 16-byte aligned middle of the tensor (up to three head and three tail elements are read one by one by
// workgroup 0).  A thread counts runs of one bin in a register and adds a run with ONE integer LDS atomic (sparse depth maps are
// mostly runs of 0).  At the end a workgroup adds its non-empty bins to the global counts with integer atomics -- order-independent
// -- and writes ONE record {min, max, sum, sum of squares} (fp64; reduced over the threads through LDS in a fixed tree) into the
// workspace.  Launch 2: one workgroup folds the records in a fixed order into stats[4].  No float atomics, no flag between
// workgroups: two runs give the same bits.  min and max ignore nothing: NaN propagates (np.min / np.max); sum and sum of squares run
// over ALL values, as values.sum() and values.dot(values) do.
#include <math.h>

#include "kbn_common.h"

namespace kbn {

constexpr int HIST_THREADS = 256;
constexpr int HIST_EDGES = KBN_HISTOGRAM_POSITIVE_EDGES;   // 774
constexpr int HIST_BINS = KBN_HISTOGRAM_BINS;              // 1548
constexpr int HIST_MAX_BLOCKS = 1024;                      // records the workspace holds: 4 workgroups a CU
constexpr int HIST_BLOCK_ELEMENTS = HIST_THREADS * 16;     // a workgroup takes at least four quads a thread (one or two measured the same)
static_assert(HIST_BINS == 2 * HIST_EDGES, "bins");
static_assert((size_t)HIST_MAX_BLOCKS * 4 * sizeof(double) == KBN_HISTOGRAM_WORKSPACE_BYTES, "workspace");

struct HistStats {
    double mn, mx, sum, sq;
};

// np.min / np.max: a NaN, once seen, stays (x < NaN is false for every x)
__device__ __forceinline__ void fold_min(double& a, double b) { if (b < a || b != b) a = b; }
__device__ __forceinline__ void fold_max(double& a, double b) { if (b > a || b != b) a = b; }

// the bin of one value, or -1 (see the file comment)
__device__ __forceinline__ int bin_of(const double* edges, float v) {
    const double x = (double)v;
    if (x != x) return -1;
    const bool negative = x < 0.0;
    const double a = fabs(x);
    int j = 0;   // #{k : P[k] <= a}, or #{k : P[k] < a} for a negative value
#pragma unroll
    for (int step = 512; step >= 1; step >>= 1) {
        const int probe = j + step;            // P[0 .. probe - 1] all pass <=> P[probe - 1] passes (P increases)
        if (probe <= HIST_EDGES) {
            const double e = edges[probe - 1];
            if (negative ? e < a : e <= a) j = probe;
        }
    }
    if (negative) return j == HIST_EDGES ? -1 : HIST_EDGES - 1 - j;
    if (j == HIST_EDGES) return a == edges[HIST_EDGES - 1] ? HIST_BINS - 1 : -1;
    return HIST_EDGES + j;
}

struct HistThread {
    HistStats s;
    int bin, run;   // the current run: `run` values of bin `bin` not yet added
};

__device__ __forceinline__ void take(HistThread& t, unsigned* bins, float v, int b) {
    const double x = (double)v;
    fold_min(t.s.mn, x);
    fold_max(t.s.mx, x);
    t.s.sum += x;
    t.s.sq += x * x;
    if (b != t.bin) {
        if (t.run > 0) atomicAdd(&bins[t.bin], (unsigned)t.run);   // t.run > 0 only with t.bin >= 0
        t.bin = b;
        t.run = 0;
    }
    t.run += b >= 0;
}

__global__ __launch_bounds__(HIST_THREADS) void histogram_kernel(const float* __restrict__ x, long long n, long long head, long long quads,
                                                                 const double* __restrict__ positive_edges, unsigned* __restrict__ counts,
                                                                 HistStats* __restrict__ records) {
    __shared__ double edges[HIST_EDGES];
    __shared__ unsigned bins[HIST_BINS];
    __shared__ HistStats fold[HIST_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < HIST_EDGES; i += HIST_THREADS) edges[i] = positive_edges[i];
    for (int i = tid; i < HIST_BINS; i += HIST_THREADS) bins[i] = 0u;
    __syncthreads();

    HistThread t;
    t.s = HistStats{INFINITY, -INFINITY, 0.0, 0.0};
    t.bin = -1;
    t.run = 0;
    // the aligned middle: quads [0, quads) start at element `head`
    const f32x4* middle = reinterpret_cast<const f32x4*>(x + head);
    for (long long q = (long long)blockIdx.x * HIST_THREADS + tid; q < quads; q += (long long)gridDim.x * HIST_THREADS) {
        const f32x4 v = middle[q];
        // the four searches first: they are independent chains of LDS reads, and the runs below must be taken in order
        const int b0 = bin_of(edges, v[0]), b1 = bin_of(edges, v[1]), b2 = bin_of(edges, v[2]), b3 = bin_of(edges, v[3]);
        take(t, bins, v[0], b0);
        take(t, bins, v[1], b1);
        take(t, bins, v[2], b2);
        take(t, bins, v[3], b3);
    }
    // up to three elements in front of the middle and three behind it
    if (blockIdx.x == 0) {
        const long long tail = head + 4 * quads;
        if (tid < head) take(t, bins, x[tid], bin_of(edges, x[tid]));
        else if (tid >= 4 && tail + (tid - 4) < n) take(t, bins, x[tail + (tid - 4)], bin_of(edges, x[tail + (tid - 4)]));
    }
    if (t.run > 0) atomicAdd(&bins[t.bin], (unsigned)t.run);

    fold[tid] = t.s;
    __syncthreads();
    for (int s = HIST_THREADS / 2; s >= 1; s >>= 1) {   // a fixed tree: the same bits every run
        if (tid < s) {
            HistStats a = fold[tid];
            const HistStats b = fold[tid + s];
            fold_min(a.mn, b.mn);
            fold_max(a.mx, b.mx);
            a.sum += b.sum;
            a.sq += b.sq;
            fold[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) records[blockIdx.x] = fold[0];
    for (int i = tid; i < HIST_BINS; i += HIST_THREADS) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&counts[i], c);
    }
}

// the records of all workgroups -> stats[4], in a fixed order
__global__ __launch_bounds__(HIST_THREADS) void histogram_stats_kernel(const HistStats* __restrict__ records, int n_records,
                                                                       double* __restrict__ stats) {
    __shared__ HistStats fold[HIST_THREADS];
    const int tid = threadIdx.x;
    HistStats a{INFINITY, -INFINITY, 0.0, 0.0};
    for (int i = tid; i < n_records; i += HIST_THREADS) {
        const HistStats b = records[i];
        fold_min(a.mn, b.mn);
        fold_max(a.mx, b.mx);
        a.sum += b.sum;
        a.sq += b.sq;
    }
    fold[tid] = a;
    __syncthreads();
    for (int s = HIST_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            HistStats c = fold[tid];
            const HistStats b = fold[tid + s];
            fold_min(c.mn, b.mn);
            fold_max(c.mx, b.mx);
            c.sum += b.sum;
            c.sq += b.sq;
            fold[tid] = c;
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[0] = fold[0].mn;
        stats[1] = fold[0].mx;
        stats[2] = fold[0].sum;
        stats[3] = fold[0].sq;
    }
}

}  // namespace kbn

extern "C" {

int kbn_histogram_forward(const float* x, long long n, const double* positive_edges, int* counts, double* stats, void* workspace,
                          size_t workspace_bytes, kbn_stream_t stream) {
    using namespace kbn;
    if (!x || !positive_edges || !counts || !stats || !workspace || n < 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(positive_edges) & 7) || (reinterpret_cast<uintptr_t>(stats) & 7) ||
        (reinterpret_cast<uintptr_t>(counts) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return KBN_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < KBN_HISTOGRAM_WORKSPACE_BYTES) return KBN_ERR_WORKSPACE;
    if (n > 0x7fffffffll) return KBN_ERR_UNSUPPORTED;   // the counts are 32-bit
    // elements in front of the first 16-byte boundary (0 .. 3), then whole quads, then 0 .. 3 elements
    const long long head = std::min<long long>(n, (long long)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4));
    const long long quads = (n - head) / 4;
    const int blocks = (int)std::min<long long>((n + HIST_BLOCK_ELEMENTS - 1) / HIST_BLOCK_ELEMENTS, HIST_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, HIST_BINS * sizeof(int), s) != hipSuccess) return KBN_ERR_LAUNCH;
    HistStats* records = static_cast<HistStats*>(workspace);
    hipLaunchKernelGGL(histogram_kernel, dim3(blocks), dim3(HIST_THREADS), 0, s, x, n, head, quads, positive_edges,
                       reinterpret_cast<unsigned*>(counts), records);
    KBN_CHECK_LAUNCH();
    hipLaunchKernelGGL(histogram_stats_kernel, dim3(1), dim3(HIST_THREADS), 0, s, records, blocks, stats);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // extern "C"
