// tractmap.hip — what a tractogram says about the volume it was traced in, on gfx950: path-density maps (fibd_str_density), the
// scalar maps sampled along every line (fibd_str_sample) and per-line length / mean (fibd_str_stats).  Not in the reference: the
// definitions are the "Tract maps" section of include/fibers_hip.h.  Inputs are packed lines as fibd_stream_run / fibd_stream_pack
// leave them: xyz float32 [npoints][3] (any 4-byte boundary), npts int32 [nlines].
//
// Kernels
//   ls_block / ls_totals / ls_apply <TmItem>   (line_scan.inc; the Item is in tm_lines.inc, shared with tractsel.hip and bundle.hip)
//                     exclusive int64 scan of npts -> first point of every line; the totals kernel also
//                     judges the input (a negative count, or a sum that is not npoints) and publishes the verdict in device memory:
//                     the kernels behind it read it and add nothing to a refused input (no host round trip)
//   tm_density_points (mode 0)   a flat pass over the points, no line structure: a wave takes 64 consecutive points, merges runs of
//                     equal voxels (ballot of the run heads) and adds the run length with ONE vector atomic per run
//   tm_density_lines  (mode 1)   G lanes per line, G points per round; the voxels of the line so far lie in an LDS tile and a run head
//                     is counted only if no earlier point of the line has its voxel (an exact comparison against ALL of them).
//                     Lines longer than the tile are left to
//   tm_density_lines_long        one workgroup per long line: an LDS bitmap over 2^18 voxels at a time, the line is passed once per
//                     window between its smallest and largest voxel; the lane whose atomic OR sets a bit adds 1.  Exact for any length.
//   tm_density_ends   (mode 2)   a lane per line
//   tm_sample         256 points per workgroup: voxel indices into LDS, then the [256][nframes] block of the output is written as
//                     consecutive floats (whole rows of consecutive points) with the gather done per element
//   tm_stats          G lanes per line: float64 terms, a strided partial sum per lane, a butterfly over the group
#include "common.h"

#include <algorithm>

// the statistics are defined as float64 operations rounded one by one (include/fibers_hip.h): nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "tm_lines.inc"                                        // TM_BLOCK, tm_voxel, the offset scan (tm_offsets), tm_check_lines
constexpr int TM_LINES_G = 16;                                 // lanes per line of tm_density_lines (profiles/tract_maps/README.md)
constexpr int TM_LINES_TILE = 256;                             // points of a line its LDS tile holds; longer lines: tm_density_lines_long
constexpr int TM_LONG_BITS = 1 << 18;                          // voxels per window of the long-line bitmap (32 KB of LDS)
constexpr int TM_LONG_GRID = 1024;
constexpr int TM_STATS_G = 16;                                 // lanes per line of tm_stats
constexpr int TM_POINTS_PER_BLOCK = 2048;                      // tm_density_points: 8 wave tiles of 64 points per wave

__device__ __forceinline__ void tm_add_outside(int64_t *n_outside, int64_t n) {
    if (n) atomicAdd(reinterpret_cast<unsigned long long *>(n_outside), (unsigned long long)n);
}

// ---- density ---------------------------------------------------------------------------------------------------------------------
// mode 0.  A wave's tile is 64 consecutive points; a run of equal voxels inside the tile is one atomic add of its length.
__global__ __launch_bounds__(TM_BLOCK) void tm_density_points(const float *xyz, int64_t npoints, int nx, int ny, int nz, const TmHead *head,
                                                              uint32_t *D, int64_t *n_outside) {
    if (!head->ok) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t block0 = (int64_t)blockIdx.x * TM_POINTS_PER_BLOCK;
    int outside = 0;
    for (int t = wave; t < TM_POINTS_PER_BLOCK / 64; t += TM_BLOCK / 64) {
        const int64_t p = block0 + t * 64 + lane;
        if (block0 + t * 64 >= npoints) break;
        const bool valid = p < npoints;
        const int64_t v = valid ? tm_voxel_at(xyz, p, nx, ny, nz) : -2;
        const int64_t prev = __shfl_up(v, 1);
        const bool head_of_run = lane == 0 || v != prev;
        const uint64_t heads = __ballot(head_of_run);
        outside += valid && v < 0;
        if (head_of_run && v >= 0) {
            const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
            const int len = above ? __ffsll((unsigned long long)above) : 64 - lane;
            atomicAdd(D + v, (unsigned)len);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) outside += __shfl_xor(outside, d);
    if (lane == 0) tm_add_outside(n_outside, outside);
}

// mode 1, lines of at most TM_LINES_TILE points: G lanes per line.  Round r takes points [G r, G r + G) of the line; their voxels go
// into the line's LDS tile, and the head of a run of equal voxels is counted iff NO earlier point of the line has its voxel.
template <int G>
__global__ __launch_bounds__(64) void tm_density_lines(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines,
                                                       int nx, int ny, int nz, const TmHead *head, uint32_t *D, int64_t *n_outside) {
    __shared__ __attribute__((aligned(16))) int32_t s_tile[64 / G][TM_LINES_TILE];
    if (!head->ok) return;
    const int lane = threadIdx.x, g = lane % G, grp = lane / G;
    const int64_t line = (int64_t)blockIdx.x * (64 / G) + grp;
    int n = 0;
    int64_t first = 0;
    if (line < nlines) { n = npts[line]; first = off[line]; }
    if (n > TM_LINES_TILE) n = 0;                               // tm_density_lines_long's
    int32_t *tile = s_tile[grp];
    int outside = 0;
    int32_t carry = -2;                                         // voxel of the point before this round's first
    for (int base = 0; __any(base < n); base += G) {            // (one wave per workgroup: the barrier below is the wave's own)
        const int k = base + g;
        const bool valid = k < n;
        const int32_t v = valid ? (int32_t)tm_voxel_at(xyz, first + k, nx, ny, nz) : -2;
        int32_t prev = __shfl_up(v, 1, G);
        if (g == 0) prev = carry;
        carry = __shfl(v, G - 1, G);
        if (valid) tile[k] = v;
        outside += valid && v < 0;
        __syncthreads();
        if (valid && v >= 0 && v != prev) {
            bool seen = false;
            int i = 0;
            for (; i + 4 <= k; i += 4) {
                const int4 t = *reinterpret_cast<const int4 *>(tile + i);
                seen |= t.x == v | t.y == v | t.z == v | t.w == v;
            }
            for (; i < k; i++) seen |= tile[i] == v;
            if (!seen) atomicAdd(D + v, 1u);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) outside += __shfl_xor(outside, d);
    if (lane == 0) tm_add_outside(n_outside, outside);
}

// mode 1, lines of more than TM_LINES_TILE points: a workgroup per line, a bitmap of TM_LONG_BITS voxels in LDS.  The line is passed
// once per window of voxel indices between its smallest and its largest; whoever sets a bit first adds 1.
__global__ __launch_bounds__(TM_BLOCK) void tm_density_lines_long(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines,
                                                                  int nx, int ny, int nz, const TmHead *head, uint32_t *D, int64_t *n_outside) {
    __shared__ uint32_t s_bits[TM_LONG_BITS / 32];
    __shared__ int s_lo, s_hi, s_out;
    __shared__ int32_t s_npts[TM_BLOCK];
    if (!head->ok) return;
    // the workgroup looks at TM_BLOCK counts at a time, a lane each: where none is long (every tile of the tracer's own output) that is all
    for (int64_t tile0 = (int64_t)blockIdx.x * TM_BLOCK; tile0 < nlines; tile0 += (int64_t)gridDim.x * TM_BLOCK) {
        const int mine = tile0 + threadIdx.x < nlines ? npts[tile0 + threadIdx.x] : 0;
        if (!__syncthreads_or(mine > TM_LINES_TILE)) continue;
        s_npts[threadIdx.x] = mine;
        __syncthreads();
        for (int t = 0; t < TM_BLOCK; t++) {
            const int n = s_npts[t];
            if (n <= TM_LINES_TILE) continue;                   // (uniform over the workgroup)
            const int64_t first = off[tile0 + t];
            if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; s_out = 0; }
            __syncthreads();
            int lo = 0x7fffffff, hi = -1, outside = 0;
            for (int k = threadIdx.x; k < n; k += TM_BLOCK) {
                const int v = (int)tm_voxel_at(xyz, first + k, nx, ny, nz);
                if (v < 0) outside++; else { lo = min(lo, v); hi = max(hi, v); }
            }
            if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
            if (outside) atomicAdd(&s_out, outside);
            __syncthreads();
            const int vlo = s_lo, vhi = s_hi;
            if (threadIdx.x == 0) tm_add_outside(n_outside, s_out);
            for (int64_t w0 = vlo; w0 <= vhi; w0 += TM_LONG_BITS) {  // (no window at all when every point is outside: vhi = -1)
                const int nbits = (int)min((int64_t)TM_LONG_BITS, (int64_t)vhi - w0 + 1);
                for (int i = threadIdx.x; i < (nbits + 31) / 32; i += TM_BLOCK) s_bits[i] = 0;
                __syncthreads();
                for (int k = threadIdx.x; k < n; k += TM_BLOCK) {
                    const int64_t v = tm_voxel_at(xyz, first + k, nx, ny, nz);
                    if (v < w0 || v >= w0 + nbits) continue;
                    const int bit = (int)(v - w0);
                    const uint32_t m = 1u << (bit & 31);
                    if (!(atomicOr(&s_bits[bit >> 5], m) & m)) atomicAdd(D + v, 1u);
                }
                __syncthreads();
            }
            __syncthreads();                                    // (s_lo / s_hi / s_out are rewritten for the next line)
        }
        __syncthreads();                                        // (s_npts is rewritten for the next tile)
    }
}

// mode 2: a lane per line
__global__ __launch_bounds__(TM_BLOCK) void tm_density_ends(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines,
                                                            int nx, int ny, int nz, const TmHead *head, uint32_t *D, int64_t *n_outside) {
    if (!head->ok) return;
    const int64_t line = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    int outside = 0;
    if (line < nlines) {
        const int n = npts[line];
        if (n >= 1) {
            const int64_t first = off[line];
            const int64_t a = tm_voxel_at(xyz, first, nx, ny, nz), b = tm_voxel_at(xyz, first + n - 1, nx, ny, nz);
            if (a >= 0) atomicAdd(D + a, 1u); else outside++;
            if (b >= 0) atomicAdd(D + b, 1u); else outside++;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) outside += __shfl_xor(outside, d);
    if ((threadIdx.x & 63) == 0) tm_add_outside(n_outside, outside);
}

// ---- sample ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void tm_sample(const float *xyz, int64_t npoints, const float *vol, int nx, int ny, int nz, int nframes,
                                                      float outside, float *S) {
    __shared__ int64_t s_vox[TM_BLOCK];
    const int64_t p0 = (int64_t)blockIdx.x * TM_BLOCK, p = p0 + threadIdx.x;
    s_vox[threadIdx.x] = p < npoints ? tm_voxel_at(xyz, p, nx, ny, nz) : -1;
    __syncthreads();
    const int64_t nvox = (int64_t)nx * ny * nz;
    const unsigned here = (unsigned)min((int64_t)TM_BLOCK, npoints - p0), nout = here * (unsigned)nframes;
    float *out = S + p0 * nframes;
    for (unsigned e = threadIdx.x; e < nout; e += TM_BLOCK) {   // consecutive lanes, consecutive floats of [here][nframes]
        const unsigned pt = e / (unsigned)nframes, f = e - pt * (unsigned)nframes;
        const int64_t v = s_vox[pt];
        out[e] = v >= 0 ? vol[(int64_t)f * nvox + v] : outside;
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ double tm_group_sum(double s) {
    for (int d = G / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, G);
    return s;
}

// G lanes per line.  props[line][0] = length in mm, [1 + c] = mean of scalar column c; float64 terms, rounded to float32 once.
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void tm_stats(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines,
                                                     float rx, float ry, float rz, const float *scalars, int ns, const TmHead *head, float *props) {
    if (!head->ok) return;
    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    if (line >= nlines) return;                                 // (whole groups leave together)
    const int n = npts[line];
    const int64_t first = off[line];
    const double dx = (double)rx, dy = (double)ry, dz = (double)rz;
    double len = 0.0;
    for (int k = g; k + 1 < n; k += G) {
        const float *a = xyz + 3 * (first + k);
        const double ux = ((double)a[3] - (double)a[0]) * dx, uy = ((double)a[4] - (double)a[1]) * dy, uz = ((double)a[5] - (double)a[2]) * dz;
        len += sqrt(ux * ux + uy * uy + uz * uz);
    }
    len = tm_group_sum<G>(len);
    float *row = props + line * (1 + ns);
    if (g == 0) row[0] = (float)len;
    for (int c = 0; c < ns; c++) {
        double s = 0.0;
        for (int k = g; k < n; k += G) s += (double)scalars[(first + k) * ns + c];
        s = tm_group_sum<G>(s);
        if (g == 0) row[1 + c] = (float)(s / (double)n);
    }
}

template <int G>
void tm_launch_lines(const float *xyz, const int32_t *npts, const TmWork &w, int64_t nlines, int nx, int ny, int nz, uint32_t *density,
                     int64_t *n_outside, hipStream_t st) {
    hipLaunchKernelGGL(tm_density_lines<G>, dim3((unsigned)fib::cdiv(nlines, 64 / G)), dim3(64), 0, st, xyz, npts, w.off, nlines, nx, ny, nz, w.head,
                       density, n_outside);
}

}  // namespace

extern "C" int fibd_str_work_size(int64_t nlines, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    *bytes = tm_work_bytes(nlines);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_density(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int mode,
                                uint32_t *density, int64_t *n_outside_dev, void *work, size_t work_bytes, void *stream) try {
    const int what = mode & ~FIB_DENSITY_ACCUMULATE;
    FIB_CHECK(what == FIB_DENSITY_POINTS || what == FIB_DENSITY_LINES || what == FIB_DENSITY_ENDPOINTS, FIB_ERR_INVALID, "unknown density mode %d", mode);
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(density && n_outside_dev, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    const int64_t nvox = (int64_t)nx * ny * nz;
    FIB_CHECK(what != FIB_DENSITY_LINES || nvox < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "FIB_DENSITY_LINES takes volumes of fewer than 2^31 voxels");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof(what == FIB_DENSITY_POINTS ? "str_density_points" : what == FIB_DENSITY_LINES ? "str_density_lines" : "str_density_ends", st);
    if (!(mode & FIB_DENSITY_ACCUMULATE)) FIB_HIP(hipMemsetAsync(density, 0, sizeof(uint32_t) * (size_t)nvox, st));
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, n_outside_dev, st, w));
    if (nlines == 0 || npoints == 0) return FIB_OK;
    if (what == FIB_DENSITY_POINTS)
        hipLaunchKernelGGL(tm_density_points, dim3((unsigned)fib::cdiv(npoints, TM_POINTS_PER_BLOCK)), dim3(TM_BLOCK), 0, st, xyz, npoints, nx, ny, nz,
                           w.head, density, n_outside_dev);
    else if (what == FIB_DENSITY_LINES) {
        int g = TM_LINES_G;
#ifdef FIB_AB_VARIANTS                                          // the lane mapping's A/B partners (tools/tract_maps_time.py, diagnostic build only)
        if (const char *e = fib::ab_env("FIBERS_TM_LINES_G")) g = atoi(e);
        if (g == 8) tm_launch_lines<8>(xyz, npts, w, nlines, nx, ny, nz, density, n_outside_dev, st);
        else if (g == 32) tm_launch_lines<32>(xyz, npts, w, nlines, nx, ny, nz, density, n_outside_dev, st);
        else if (g == 64) tm_launch_lines<64>(xyz, npts, w, nlines, nx, ny, nz, density, n_outside_dev, st);
        else
#endif
        { (void)g; tm_launch_lines<TM_LINES_G>(xyz, npts, w, nlines, nx, ny, nz, density, n_outside_dev, st); }
        hipLaunchKernelGGL(tm_density_lines_long, dim3((unsigned)std::min<int64_t>(fib::cdiv(nlines, TM_BLOCK), TM_LONG_GRID)), dim3(TM_BLOCK), 0, st, xyz, npts, w.off,
                           nlines, nx, ny, nz, w.head, density, n_outside_dev);
    } else
        hipLaunchKernelGGL(tm_density_ends, dim3((unsigned)fib::cdiv(nlines, TM_BLOCK)), dim3(TM_BLOCK), 0, st, xyz, npts, w.off, nlines, nx, ny, nz,
                           w.head, density, n_outside_dev);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_sample(const float *xyz, int64_t npoints, const float *vol, int nx, int ny, int nz, int nframes, float outside,
                               float *scalars, void *stream) try {
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(nframes <= (1 << 20), FIB_ERR_UNSUPPORTED, "more than 2^20 frames");
    if (npoints == 0) return FIB_OK;
    FIB_CHECK(xyz && vol && scalars, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK((reinterpret_cast<uintptr_t>(xyz) & 3) == 0, FIB_ERR_INVALID, "points must be 4-byte aligned");
    FIB_CHECK(fib::cdiv(npoints, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many points");
    fib::ProfScope prof("str_sample", (hipStream_t)stream);
    hipLaunchKernelGGL(tm_sample, dim3((unsigned)fib::cdiv(npoints, TM_BLOCK)), dim3(TM_BLOCK), 0, (hipStream_t)stream, xyz, npoints, vol, nx, ny, nz,
                       nframes, outside, scalars);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_stats(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], const float *scalars,
                              int nscalars, float *props, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(volres, FIB_ERR_INVALID, "NULL volres");
    FIB_CHECK(nscalars >= 0 && (nscalars == 0 || npoints == 0 || scalars), FIB_ERR_INVALID, "nscalars columns need a scalars array");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_CHECK(nlines == 0 || props, FIB_ERR_INVALID, "NULL props");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_stats", st);
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, nullptr, st, w));
    if (nlines == 0) return FIB_OK;
    hipLaunchKernelGGL(tm_stats<TM_STATS_G>, dim3((unsigned)fib::cdiv(nlines * TM_STATS_G, TM_BLOCK)), dim3(TM_BLOCK), 0, st, xyz, npts, w.off, nlines,
                       volres[0], volres[1], volres[2], scalars, nscalars, w.head, props);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
