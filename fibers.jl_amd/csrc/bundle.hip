// bundle.hip — what a tractogram needs before it can be worked on per bundle, on gfx950: every line brought to K points equidistant in
// arc length (fibd_str_resample), the MDF distance of every line to a set of model bundles with the nearest model and the orientation
// (fibd_str_assign), and the per-bundle sums of the oriented lines (fibd_str_centroids).  Not in the reference: the definitions are the
// "Bundle tools" section of include/fibers_hip.h.  Resample reads packed lines as fibd_stream_run / fibd_stream_pack leave them.
//
// Kernels
//   ls_block / ls_totals / ls_apply <TmItem>   (line_scan.inc, tm_lines.inc) the offset scan and its verdict on npts; *status_dev starts at 0 / -1
//   bd_resample<G>    lines of at most BD_SHORT_MAX points, G lanes per line, G segments per round.  NO storage for the cumulative
//                     lengths: in a round every lane computes the length of its segment, then the group runs the float64 running sum
//                     through its G lanes in sequence (shuffles), so that lane g holds [c_i, c_{i+1}) of its segment -- the same
//                     values, bit for bit, in the pass that finds T and in the pass that emits.  A lane emits the rows k whose t_k
//                     falls inside its interval (the last segment also takes what lies beyond).  c is non-decreasing because it is a
//                     sequence of additions of non-negative terms: every row has exactly one owner, two runs give the same bytes.
//   bd_resample_long  the same code with a whole wave per line (G = 64) for the lines bd_resample leaves out; a workgroup looks at
//                     TM_BLOCK counts at a time, a lane each, and where none is long that is all it does
//   bd_assign         a lane per line, the models through LDS in tiles of BD_TILE_POINTS points (60 KB: two workgroups per CU); BD_MT
//                     models at a time, their 2 x BD_MT float64 sums in registers, so that a point of the line is loaded once per
//                     2 x BD_MT norms; every lane of a wave reads the same model point (an LDS broadcast)
//   bd_centroids      a workgroup takes BD_CENT_LINES lines; the bundles go through LDS in windows of as many as fit in
//                     BD_CENT_DOUBLES float64 cells; a wave adds a line into its bundle's cells (LDS atomics), then the cells of the
//                     bundles that got a line are added to global memory, one float64 vector atomic per cell and workgroup
//   bd_centroids_direct   more windows than BD_CENT_MAX_WINDOWS (many bundles, few lines each): global atomics straight away
#include "common.h"

#include <algorithm>

// every distance is defined as float64 operations rounded one by one (include/fibers_hip.h): nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "tm_lines.inc"                                        // TM_BLOCK, the offset scan (tm_offsets), tm_check_lines
constexpr int BD_RESAMPLE_G = 16;                              // lanes per line of bd_resample
constexpr int BD_SHORT_MAX = 1024;                             // points of a line bd_resample takes; longer lines: bd_resample_long
constexpr int BD_LONG_GRID = 1024;
constexpr int BD_K_MAX = 256;
constexpr uint32_t BD_NAN = 0x7FC00000u;
constexpr int BD_TILE_POINTS = 5120;                           // model points per LDS tile of bd_assign (61 440 bytes)
constexpr int BD_MT = 8;                                       // models whose sums a lane of bd_assign keeps in registers
constexpr int BD_CENT_LINES = 1024;                            // lines per workgroup of bd_centroids
constexpr int BD_CENT_DOUBLES = 6144;                          // float64 cells of its LDS window (48 KB)
constexpr int BD_CENT_MAX_WINDOWS = 16;

// |(a - b) o r| in float64, the term of tm_stats' length with a and b as they are passed (include/fibers_hip.h)
__device__ __forceinline__ double bd_norm(double ax, double ay, double az, double bx, double by, double bz, double rx, double ry, double rz) {
    const double ux = (ax - bx) * rx, uy = (ay - by) * ry, uz = (az - bz) * rz;
    return sqrt(ux * ux + uy * uy + uz * uz);
}

// ---- resample --------------------------------------------------------------------------------------------------------------------
// One round of the running sum: lane g of the group contributes l (0 beyond the line's last segment); on return [cs, ce) is the
// interval of its segment and `carry` the sum after the round's last lane.  Sequential in the lanes: c_{i+1} = c_i + l_i.
template <int G>
__device__ __forceinline__ void bd_round(double l, int g, double &carry, double &cs, double &ce) {
    double v = carry;
    cs = ce = v;
#pragma unroll
    for (int j = 0; j < G; j++) {
        const double lj = __shfl(l, j, G);
        if (j == g) cs = v;
        v += lj;
        if (j == g) ce = v;
    }
    carry = v;
}

template <int G>
__device__ __forceinline__ double bd_segment(const float *p, int i, int n, double rx, double ry, double rz) {
    if (i + 1 >= n) return 0.0;
    const float *a = p + 3 * (int64_t)i;
    return bd_norm((double)a[3], (double)a[4], (double)a[5], (double)a[0], (double)a[1], (double)a[2], rx, ry, rz);
}

// the K rows of one line, by the G lanes of a group (g = 0 .. G-1; the whole group arrives here together)
template <int G>
__device__ __forceinline__ void bd_resample_line(const float *p, int n, double rx, double ry, double rz, int K, bool flip, uint32_t *out, int g) {
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(p);
    if (n <= 1) {                                               // no points: NaN rows; one point: copies of it, bit for bit
        for (int w = g; w < 3 * K; w += G) out[w] = n == 0 ? BD_NAN : pw[w % 3];
        return;
    }
    double T = 0.0, cs, ce;
    for (int base = 0; base < n - 1; base += G) bd_round<G>(bd_segment<G>(p, base + g, n, rx, ry, rz), g, T, cs, ce);
    if (!(fabs(T) <= 1.79769313486231570815e308)) {             // NaN or Inf
        for (int w = g; w < 3 * K; w += G) out[w] = BD_NAN;
        return;
    }
    if (g < 3) {                                                // the two ends are copies
        out[(flip ? 3 * (K - 1) : 0) + g] = pw[g];
        out[(flip ? 0 : 3 * (K - 1)) + g] = pw[3 * (int64_t)(n - 1) + g];
    }
    const double km1 = (double)(K - 1);
    double carry = 0.0;
    for (int base = 0; base < n - 1; base += G) {
        const int i = base + g;
        bd_round<G>(bd_segment<G>(p, i, n, rx, ry, rz), g, carry, cs, ce);
        if (i > n - 2) continue;
        const bool last = i == n - 2;
        int k = 1;
        if (T > 0.0) {                                          // an estimate of the first row at or behind cs, then made exact
            const double kf = cs / T * km1;
            k = kf >= km1 ? K - 1 : (int)kf;
            if (k < 1) k = 1;
        }
        while (k > 1 && (T * (double)(k - 1)) / km1 >= cs) k--;
        while (k <= K - 2 && (T * (double)k) / km1 < cs) k++;
        for (; k <= K - 2; k++) {
            const double t = (T * (double)k) / km1;
            if (!last && !(t < ce)) break;
            const double den = ce - cs;
            double a = 0.0;
            if (den > 0.0) { a = (t - cs) / den; a = a < 0.0 ? 0.0 : a > 1.0 ? 1.0 : a; }
            const float *q = p + 3 * (int64_t)i;
            float *row = reinterpret_cast<float *>(out) + 3 * (flip ? K - 1 - k : k);
            for (int c = 0; c < 3; c++) {
                const double p0 = (double)q[c], p1 = (double)q[3 + c];
                row[c] = (float)(p0 + a * (p1 - p0));
            }
        }
    }
}

template <int G>
__global__ __launch_bounds__(TM_BLOCK) void bd_resample(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines, float rx, float ry,
                                                        float rz, int K, const uint8_t *flip, const TmHead *head, uint32_t *out, int64_t *status) {
    if (!head->ok) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = nlines;
    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    if (line >= nlines) return;                                 // (whole groups leave together)
    const int n = npts[line];
    if (n > BD_SHORT_MAX) return;                               // bd_resample_long's
    bd_resample_line<G>(xyz + 3 * off[line], n, (double)rx, (double)ry, (double)rz, K, flip && flip[line], out + (int64_t)3 * K * line, g);
}

__global__ __launch_bounds__(TM_BLOCK) void bd_resample_long(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines, float rx, float ry,
                                                             float rz, int K, const uint8_t *flip, const TmHead *head, uint32_t *out) {
    __shared__ int32_t s_npts[TM_BLOCK];
    if (!head->ok) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile0 = (int64_t)blockIdx.x * TM_BLOCK; tile0 < nlines; tile0 += (int64_t)gridDim.x * TM_BLOCK) {
        const int mine = tile0 + threadIdx.x < nlines ? npts[tile0 + threadIdx.x] : 0;
        if (!__syncthreads_or(mine > BD_SHORT_MAX)) continue;
        s_npts[threadIdx.x] = mine;
        __syncthreads();
        for (int t = wave; t < TM_BLOCK; t += TM_BLOCK / 64) {  // a wave per long line
            const int n = s_npts[t];
            if (n <= BD_SHORT_MAX) continue;                    // (uniform over the wave)
            const int64_t line = tile0 + t;
            bd_resample_line<64>(xyz + 3 * off[line], n, (double)rx, (double)ry, (double)rz, K, flip && flip[line], out + (int64_t)3 * K * line, lane);
        }
        __syncthreads();                                        // (s_npts is rewritten for the next tile)
    }
}

// ---- assign ----------------------------------------------------------------------------------------------------------------------
// A lane per line; the models of a tile lie in LDS as they lie in memory.  For BD_MT models at a time the two k-sums of every model
// run in registers, k from 0 upwards: sequential float64 sums, as the header defines them.
__global__ __launch_bounds__(TM_BLOCK) void bd_assign(const float *lines, int64_t nlines, int K, const float *models, int nmodels, int tile_models,
                                                      float rx, float ry, float rz, float thresh, int32_t *label, float *dist, uint8_t *flip,
                                                      float *dist_all) {
    __shared__ float s_m[3 * BD_TILE_POINTS];
    const int64_t line = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    const bool valid = line < nlines;
    const float *a = lines + (int64_t)3 * K * (valid ? line : nlines - 1);
    const double dx = (double)rx, dy = (double)ry, dz = (double)rz, dK = (double)K;
    double best = 0.0;
    int bestm = -1, bestf = 0;
    for (int m0 = 0; m0 < nmodels; m0 += tile_models) {
        const int tm = min(tile_models, nmodels - m0);
        __syncthreads();                                        // (the tile before this one has been read)
        for (int w = threadIdx.x; w < 3 * K * tm; w += TM_BLOCK) s_m[w] = models[(int64_t)3 * K * m0 + w];
        __syncthreads();
        for (int c0 = 0; c0 < tm; c0 += BD_MT) {
            double sd[BD_MT], sf[BD_MT];
            int mo[BD_MT];                                      // (a chunk's missing models repeat its last one; their sums are dropped)
#pragma unroll
            for (int j = 0; j < BD_MT; j++) { sd[j] = 0.0; sf[j] = 0.0; mo[j] = 3 * K * min(c0 + j, tm - 1); }
            for (int k = 0; k < K; k++) {
                const double ax = (double)a[3 * k], ay = (double)a[3 * k + 1], az = (double)a[3 * k + 2];
                const int kr = 3 * (K - 1 - k);
#pragma unroll
                for (int j = 0; j < BD_MT; j++) {
                    const float *m = s_m + mo[j];
                    sd[j] += bd_norm(ax, ay, az, (double)m[3 * k], (double)m[3 * k + 1], (double)m[3 * k + 2], dx, dy, dz);
                    sf[j] += bd_norm(ax, ay, az, (double)m[kr], (double)m[kr + 1], (double)m[kr + 2], dx, dy, dz);
                }
            }
#pragma unroll
            for (int j = 0; j < BD_MT; j++) {
                if (c0 + j >= tm) break;
                const double dd = sd[j] / dK, df = sf[j] / dK;
                const int f = df < dd;
                const double d = f ? df : dd;
                if (valid && dist_all) dist_all[line * nmodels + m0 + c0 + j] = d == d ? (float)d : __uint_as_float(BD_NAN);
                if (d == d && (bestm < 0 || d < best)) { best = d; bestm = m0 + c0 + j; bestf = f; }       // (a NaN is larger than everything)
            }
        }
    }
    if (!valid) return;
    dist[line] = bestm >= 0 ? (float)best : __uint_as_float(BD_NAN);
    label[line] = bestm >= 0 && best <= (double)thresh ? bestm : -1;
    flip[line] = (uint8_t)bestf;
}

// ---- centroids -------------------------------------------------------------------------------------------------------------------
// A workgroup takes BD_CENT_LINES lines, a wave a line at a time, a lane a component.  Window by window of `slots` bundles: the
// lines whose label lies in the window are added into LDS, then the cells of the bundles that got a line go to global memory.
__global__ __launch_bounds__(TM_BLOCK) void bd_centroids(const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip, int nmodels,
                                                         int slots, double *sums, uint32_t *counts) {
    __shared__ double s_sum[BD_CENT_DOUBLES];
    __shared__ uint32_t s_cnt[BD_CENT_DOUBLES / 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K3 = 3 * K;
    const int64_t l0 = (int64_t)blockIdx.x * BD_CENT_LINES, l1 = min(l0 + BD_CENT_LINES, nlines);
    for (int b0 = 0; b0 < nmodels; b0 += slots) {
        const int nb = min(slots, nmodels - b0);
        for (int w = threadIdx.x; w < nb * K3; w += TM_BLOCK) s_sum[w] = 0.0;
        for (int w = threadIdx.x; w < nb; w += TM_BLOCK) s_cnt[w] = 0;
        __syncthreads();
        for (int64_t line = l0 + wave; line < l1; line += TM_BLOCK / 64) {
            const int lab = label[line];                        // (uniform over the wave)
            if (lab < b0 || lab >= b0 + nb) continue;
            const int b = lab - b0;
            const bool f = flip && flip[line];
            const float *src = lines + line * K3;
            for (int e = lane; e < K3; e += 64) {
                const int k = e / 3, c = e - 3 * k;
                atomicAdd(&s_sum[b * K3 + e], (double)src[3 * (f ? K - 1 - k : k) + c]);
            }
            if (lane == 0) atomicAdd(&s_cnt[b], 1u);
        }
        __syncthreads();
        for (int w = threadIdx.x; w < nb * K3; w += TM_BLOCK)
            if (s_cnt[w / K3]) atomicAdd(sums + (int64_t)b0 * K3 + w, s_sum[w]);
        for (int w = threadIdx.x; w < nb; w += TM_BLOCK)
            if (s_cnt[w]) atomicAdd(counts + b0 + w, s_cnt[w]);
        __syncthreads();                                        // (the window is zero-filled again)
    }
}

__global__ __launch_bounds__(TM_BLOCK) void bd_centroids_direct(const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip,
                                                                int nmodels, double *sums, uint32_t *counts) {
    const int lane = threadIdx.x & 63, K3 = 3 * K;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) >> 6;      // a wave per line
    if (line >= nlines) return;
    const int b = label[line];
    if (b < 0 || b >= nmodels) return;
    const bool f = flip && flip[line];
    const float *src = lines + line * K3;
    for (int e = lane; e < K3; e += 64) {
        const int k = e / 3, c = e - 3 * k;
        atomicAdd(sums + (int64_t)b * K3 + e, (double)src[3 * (f ? K - 1 - k : k) + c]);
    }
    if (lane == 0) atomicAdd(counts + b, 1u);
}

int bd_check_rows(const float *lines, int64_t nlines, int K) {
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    FIB_CHECK(K >= 1 && K <= BD_K_MAX, FIB_ERR_UNSUPPORTED, "lines of 1 to %d points each, not %d", BD_K_MAX, K);
    FIB_CHECK(nlines == 0 || lines, FIB_ERR_INVALID, "NULL lines");
    FIB_CHECK((reinterpret_cast<uintptr_t>(lines) & 3) == 0, FIB_ERR_INVALID, "lines must be 4-byte aligned");
    FIB_CHECK(nlines < ((int64_t)1 << 31) * 2, FIB_ERR_UNSUPPORTED, "too many lines");
    return FIB_OK;
}

}  // namespace

extern "C" int fibd_str_resample(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], int K,
                                 const uint8_t *flip, float *out, int64_t *status_dev, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(K >= 2 && K <= BD_K_MAX, FIB_ERR_UNSUPPORTED, "fibd_str_resample gives 2 to %d points per line, not %d", BD_K_MAX, K);
    FIB_CHECK(volres && status_dev, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_CHECK(nlines == 0 || out, FIB_ERR_INVALID, "NULL out");
    FIB_CHECK((reinterpret_cast<uintptr_t>(out) & 3) == 0, FIB_ERR_INVALID, "out must be 4-byte aligned");
    FIB_CHECK(fib::cdiv(nlines * BD_RESAMPLE_G, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_resample", st);
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, status_dev, st, w));          // (*status_dev = 0, or -1 for a refused input)
    if (nlines == 0) return FIB_OK;
    hipLaunchKernelGGL(bd_resample<BD_RESAMPLE_G>, dim3((unsigned)fib::cdiv(nlines * BD_RESAMPLE_G, TM_BLOCK)), dim3(TM_BLOCK), 0, st, xyz, npts, w.off,
                       nlines, volres[0], volres[1], volres[2], K, flip, w.head, reinterpret_cast<uint32_t *>(out), status_dev);
    hipLaunchKernelGGL(bd_resample_long, dim3((unsigned)std::min<int64_t>(fib::cdiv(nlines, TM_BLOCK), BD_LONG_GRID)), dim3(TM_BLOCK), 0, st, xyz, npts,
                       w.off, nlines, volres[0], volres[1], volres[2], K, flip, w.head, reinterpret_cast<uint32_t *>(out));
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_assign(const float *lines, int64_t nlines, int K, const float *models, int nmodels, const float volres[3],
                               float thresh_mm, int32_t *label, float *dist, uint8_t *flip, float *dist_all, void *stream) try {
    FIB_RC(bd_check_rows(lines, nlines, K));
    FIB_CHECK(nmodels >= 1 && nmodels < (1 << 24), FIB_ERR_INVALID, "the number of models must be between 1 and 2^24 - 1");
    FIB_CHECK(models && volres, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK((reinterpret_cast<uintptr_t>(models) & 3) == 0, FIB_ERR_INVALID, "models must be 4-byte aligned");
    FIB_CHECK(nlines == 0 || (label && dist && flip), FIB_ERR_INVALID, "NULL output");
    FIB_CHECK(fib::cdiv(nlines, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    if (nlines == 0) return FIB_OK;
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_assign", st);
    const int tile_models = std::min(nmodels, BD_TILE_POINTS / K);
    hipLaunchKernelGGL(bd_assign, dim3((unsigned)fib::cdiv(nlines, TM_BLOCK)), dim3(TM_BLOCK), 0, st, lines, nlines, K, models, nmodels, tile_models,
                       volres[0], volres[1], volres[2], thresh_mm, label, dist, flip, dist_all);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_centroids(const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip, int nmodels,
                                  int flags, double *sums, uint32_t *counts, void *stream) try {
    FIB_CHECK((flags & ~FIB_CENTROIDS_ACCUMULATE) == 0, FIB_ERR_INVALID, "unknown centroid flags 0x%x", flags);
    FIB_RC(bd_check_rows(lines, nlines, K));
    FIB_CHECK(nmodels >= 1 && nmodels < (1 << 24), FIB_ERR_INVALID, "the number of models must be between 1 and 2^24 - 1");
    FIB_CHECK(sums && counts && (nlines == 0 || label), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(fib::cdiv(nlines * 64, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_centroids", st);
    const size_t cells = (size_t)nmodels * 3 * (size_t)K;
    if (!(flags & FIB_CENTROIDS_ACCUMULATE)) {
        FIB_HIP(hipMemsetAsync(sums, 0, sizeof(double) * cells, st));
        FIB_HIP(hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)nmodels, st));
    }
    if (nlines == 0) return FIB_OK;
    const int slots = BD_CENT_DOUBLES / (3 * K);
    if (fib::cdiv(nmodels, slots) <= BD_CENT_MAX_WINDOWS)
        hipLaunchKernelGGL(bd_centroids, dim3((unsigned)fib::cdiv(nlines, BD_CENT_LINES)), dim3(TM_BLOCK), 0, st, lines, nlines, K, label, flip, nmodels,
                           slots, sums, counts);
    else
        hipLaunchKernelGGL(bd_centroids_direct, dim3((unsigned)fib::cdiv(nlines * 64, TM_BLOCK)), dim3(TM_BLOCK), 0, st, lines, nlines, K, label, flip,
                           nmodels, sums, counts);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
