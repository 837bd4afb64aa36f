// volmask.hip — dwi_mask (median-Otsu brain mask), the volume median filter and the connected components of a mask.  Not in the
// reference; the definition is the section "Brain mask" of include/fibers_hip.h, and tests/mask_ref.py restates it in NumPy: every
// step is a selection, an integer count or a comparison, so the kernels are held to that restatement bit for bit.
//
// float32 values are ordered by the ordered-uint key of their bit pattern (vm_key; the key of odf_post_kernel's maximum).
//   vm_mean_*        mean of the chosen frames: a float64 sequential sum in the list's order, one division, one rounding
//   vm_median<R>     a tile and its halo as keys in LDS; the rank-(n/2) key by bisection on the 32 key bits, counting over the window
//                    (R = 1, 2) or over the window's sorted y-z columns, which x-neighbours share (R = 3)
//   vm_minmax / vm_hist / vm_otsu / vm_threshold     finite extremes by atomics, 256 LDS counters a workgroup, the integer Otsu in one wave
//   vm_cc_*          label equivalence: union by atomicMin on a parent array whose entries only decrease; no workgroup waits for another
//   vm_dilate        7-point stencil
#include <algorithm>

#include "common.h"

namespace {

constexpr int VM_T = 256;                                   // threads of every one-lane-per-voxel kernel
constexpr int64_t VM_MAXVOX = (int64_t)1 << 27;             // Otsu's d = s0 c1 - s1 c0 stays inside int64
constexpr int VM_UNION_CAP = 1 << 20;                       // retries of one union (each retry means another lane lowered a root)

__host__ __device__ inline unsigned vm_key(unsigned b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__host__ __device__ inline unsigned vm_unkey(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }
__device__ inline bool vm_finite(unsigned b) { return (b & 0x7f800000u) != 0x7f800000u; }

// a count of lanes: one LDS add per wave, one global atomic per workgroup.  Every thread of the workgroup must come here.
__device__ inline void vm_count(unsigned long long *dst, bool pred) {
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const unsigned long long b = __ballot(pred);
    if (b && __lane_id() == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(&total, (unsigned)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(dst, (unsigned long long)total);
}

// ---- mean of frames --------------------------------------------------------------------------------------------------------------
constexpr int VM_LIST = 64;
struct VmFrames { int n; int idx[VM_LIST]; };

// mode A: the frames by list, summed and finalised in one launch
__global__ __launch_bounds__(VM_T) void vm_mean_frames_kernel(const float *__restrict__ dwi, int64_t stride, VmFrames fr, int64_t n, float *__restrict__ b0) {
    const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int f = 0; f < fr.n; f++) s += (double)dwi[(int64_t)fr.idx[f] * stride + i];
    b0[i] = (float)(s / (double)fr.n);
}
// mode B: nf frames [nf][n] added to the float64 buffer (first: it starts from zero), finalised by vm_mean_fin_kernel
__global__ __launch_bounds__(VM_T) void vm_mean_acc_kernel(double *__restrict__ acc, const float *__restrict__ frames, int64_t n, int nf, int first) {
    const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
    if (i >= n) return;
    double s = first ? 0.0 : acc[i];
    for (int f = 0; f < nf; f++) s += (double)frames[(int64_t)f * n + i];
    acc[i] = s;
}
__global__ __launch_bounds__(VM_T) void vm_mean_fin_kernel(const double *__restrict__ acc, int count, int64_t n, float *__restrict__ b0) {
    const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
    if (i < n) b0[i] = (float)(acc[i] / (double)count);
}

// ---- median ----------------------------------------------------------------------------------------------------------------------
// A workgroup stages its 32 x 8 x 8 tile with a halo of R as keys (coordinates clamped into the volume: edge replication, and the
// same code for a volume smaller than the tile).  A lane owns one (x, y) of the tile and takes its eight z four at a time: the four
// windows share 2R of their 2R + 1 planes, so a round reads (2R + 4)(2R + 1)^2 keys for four voxels.  The rank-(n/2) key is built from
// its top bit down: bit b stays set when fewer than rank + 1 keys lie below the prefix with it set.  32 rounds, no branch on the data.
constexpr int VM_TX = 32, VM_TY = 8, VM_TZ = 8, VM_ZV = 4;

template <int R>
__global__ __launch_bounds__(VM_TX * VM_TY) void vm_median_kernel(const float *__restrict__ in, float *__restrict__ out, int nx, int ny, int nz) {
    constexpr int W = 2 * R + 1, LX = VM_TX + 2 * R, LY = VM_TY + 2 * R, LZ = VM_TZ + 2 * R, RANK = W * W * W / 2;
    __shared__ unsigned s[LZ * LY * LX];
    const int x0 = blockIdx.x * VM_TX, y0 = blockIdx.y * VM_TY, z0 = blockIdx.z * VM_TZ;
    const unsigned *bits = reinterpret_cast<const unsigned *>(in);
    for (int i = threadIdx.x; i < LZ * LY * LX; i += VM_TX * VM_TY) {
        const int lx = i % LX, ly = (i / LX) % LY, lz = i / (LX * LY);
        const int gx = min(max(x0 - R + lx, 0), nx - 1), gy = min(max(y0 - R + ly, 0), ny - 1), gz = min(max(z0 - R + lz, 0), nz - 1);
        s[i] = vm_key(bits[((int64_t)gz * ny + gy) * nx + gx]);
    }
    __syncthreads();
    const int tx = threadIdx.x % VM_TX, ty = threadIdx.x / VM_TX;
    const int x = x0 + tx, y = y0 + ty;
    for (int zg = 0; zg < VM_TZ && z0 + zg < nz; zg += VM_ZV) {
        unsigned res[VM_ZV];
#pragma unroll
        for (int j = 0; j < VM_ZV; j++) res[j] = 0;
        const unsigned *col = s + (zg * LY + ty) * LX + tx;
        for (int bit = 31; bit >= 0; bit--) {
            unsigned t[VM_ZV], cnt[VM_ZV];
#pragma unroll
            for (int j = 0; j < VM_ZV; j++) { t[j] = res[j] | (1u << bit); cnt[j] = 0; }
#pragma unroll
            for (int p = 0; p < W + VM_ZV - 1; p++)
#pragma unroll
                for (int dy = 0; dy < W; dy++)
#pragma unroll
                    for (int dx = 0; dx < W; dx++) {
                        const unsigned k = col[(p * LY + dy) * LX + dx];
#pragma unroll
                        for (int j = 0; j < VM_ZV; j++)
                            if (p >= j && p < j + W) cnt[j] += k < t[j] ? 1u : 0u;
                    }
#pragma unroll
            for (int j = 0; j < VM_ZV; j++) if (cnt[j] <= (unsigned)RANK) res[j] = t[j];
        }
#pragma unroll
        for (int j = 0; j < VM_ZV; j++) {
            const int z = z0 + zg + j;
            if (x < nx && y < ny && z < nz) reinterpret_cast<unsigned *>(out)[((int64_t)z * ny + y) * nx + x] = vm_unkey(res[j]);
        }
    }
}

// The second scheme: work shared between x-neighbours.  The 2R + 1 windows that overlap in x are made of the same y-z columns of
// (2R + 1)^2 keys, so each column of a 32 x 4 x TZ tile and its x-halo is sorted once (odd-even transposition in registers) into LDS,
// and a voxel's median is the rank-(n/2) key of its 2R + 1 sorted columns: the same 32 rounds on the key bits, each count a binary
// search per column.  Measured on an MI355X, a pass over 140^3 (tools/mask_time.py, profiles/mask/): bisection 0.19 / 0.85 / 4.0 ms at
// R = 1 / 2 / 3, sorted columns 0.21 / 0.94 / 1.8 ms.  So the library runs bisection at R = 1 and 2 and sorted columns at R = 3 (there
// the bisection kernel holds 490 keys a lane and needs all 512 registers); the other instantiations are the A/B partners of the
// diagnostic build (FIBERS_MEDIAN_SCHEME = bisect | columns forces one scheme at every radius).
template <int R>
__global__ __launch_bounds__(256) void vm_median_cols_kernel(const float *__restrict__ in, float *__restrict__ out, int nx, int ny, int nz) {
    constexpr int W = 2 * R + 1, N2 = W * W, TY = 4, TZ = R == 3 ? 2 : 4, LX = VM_TX + 2 * R, LY = TY + 2 * R, LZ = TZ + 2 * R;
    constexpr int NCOL = LX * TY * TZ, RANK = W * W * W / 2, TOP = N2 >= 32 ? 32 : (N2 >= 16 ? 16 : 8);
    extern __shared__ unsigned vm_lds[];
    unsigned *s = vm_lds, *sorted = vm_lds + LZ * LY * LX;
    const int x0 = blockIdx.x * VM_TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
    const unsigned *bits = reinterpret_cast<const unsigned *>(in);
    for (int i = threadIdx.x; i < LZ * LY * LX; i += 256) {
        const int lx = i % LX, ly = (i / LX) % LY, lz = i / (LX * LY);
        const int gx = min(max(x0 - R + lx, 0), nx - 1), gy = min(max(y0 - R + ly, 0), ny - 1), gz = min(max(z0 - R + lz, 0), nz - 1);
        s[i] = vm_key(bits[((int64_t)gz * ny + gy) * nx + gx]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NCOL; c += 256) {
        const int lx = c % LX, ty = (c / LX) % TY, tz = c / (LX * TY);
        unsigned k[N2];
#pragma unroll
        for (int dz = 0; dz < W; dz++)
#pragma unroll
            for (int dy = 0; dy < W; dy++) k[dz * W + dy] = s[((tz + dz) * LY + ty + dy) * LX + lx];
#pragma unroll
        for (int round = 0; round < N2; round++)
#pragma unroll
            for (int i = round & 1; i + 1 < N2; i += 2) {
                const unsigned a = min(k[i], k[i + 1]), b = max(k[i], k[i + 1]);
                k[i] = a; k[i + 1] = b;
            }
#pragma unroll
        for (int j = 0; j < N2; j++) sorted[c * N2 + j] = k[j];
    }
    __syncthreads();
    for (int v = threadIdx.x; v < VM_TX * TY * TZ; v += 256) {
        const int tx = v % VM_TX, ty = (v / VM_TX) % TY, tz = v / (VM_TX * TY);
        const unsigned *cols = sorted + (size_t)(tx + LX * (ty + TY * tz)) * N2;
        unsigned res = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const unsigned t = res | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int d = 0; d < W; d++) {
                const unsigned *L = cols + d * N2;
                int pos = 0;                                 // the number of keys of the column below t
#pragma unroll
                for (int step = TOP; step >= 1; step >>= 1) {
                    const int q = pos + step;
                    if (q <= N2 && L[min(q, N2) - 1] < t) pos = q;
                }
                cnt += pos;
            }
            if (cnt <= RANK) res = t;
        }
        const int x = x0 + tx, y = y0 + ty, z = z0 + tz;
        if (x < nx && y < ny && z < nz) reinterpret_cast<unsigned *>(out)[((int64_t)z * ny + y) * nx + x] = vm_unkey(res);
    }
}
template <int R>
int vm_median_cols_launch(const float *src, float *dst, int nx, int ny, int nz, hipStream_t st) {
    constexpr int W = 2 * R + 1, TY = 4, TZ = R == 3 ? 2 : 4, LX = VM_TX + 2 * R;
    constexpr size_t lds = sizeof(unsigned) * ((TZ + 2 * R) * (TY + 2 * R) * LX + LX * TY * TZ * W * W);
    const dim3 grid((unsigned)fib::cdiv(nx, VM_TX), (unsigned)fib::cdiv(ny, TY), (unsigned)fib::cdiv(nz, TZ));
    FIB_CHECK(grid.y <= 65535 && grid.z <= 65535, FIB_ERR_UNSUPPORTED, "vol_median: ny and nz may be at most %d", 65535 * TZ);
    FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vm_median_cols_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(vm_median_cols_kernel<R>, grid, dim3(256), lds, st, src, dst, nx, ny, nz);
    return FIB_OK;
}
template <int R>
int vm_median_bisect_launch(const float *src, float *dst, int nx, int ny, int nz, hipStream_t st) {
    const dim3 grid((unsigned)fib::cdiv(nx, VM_TX), (unsigned)fib::cdiv(ny, VM_TY), (unsigned)fib::cdiv(nz, VM_TZ));
    FIB_CHECK(grid.y <= 65535 && grid.z <= 65535, FIB_ERR_UNSUPPORTED, "vol_median: ny and nz may be at most %d", 65535 * VM_TY);
    hipLaunchKernelGGL(vm_median_kernel<R>, grid, dim3(VM_TX * VM_TY), 0, st, src, dst, nx, ny, nz);
    return FIB_OK;
}
// one pass: bisection at radius 1 and 2, sorted columns at 3
int vm_median_pass(const float *src, float *dst, int nx, int ny, int nz, int radius, hipStream_t st) {
#ifdef FIB_AB_VARIANTS
    if (const char *e = fib::ab_env("FIBERS_MEDIAN_SCHEME")) {
        if (!strcmp(e, "columns"))
            return radius == 1 ? vm_median_cols_launch<1>(src, dst, nx, ny, nz, st) : radius == 2 ? vm_median_cols_launch<2>(src, dst, nx, ny, nz, st)
                                                                                                  : vm_median_cols_launch<3>(src, dst, nx, ny, nz, st);
        if (!strcmp(e, "bisect"))
            return radius == 1 ? vm_median_bisect_launch<1>(src, dst, nx, ny, nz, st) : radius == 2 ? vm_median_bisect_launch<2>(src, dst, nx, ny, nz, st)
                                                                                                    : vm_median_bisect_launch<3>(src, dst, nx, ny, nz, st);
    }
#endif
    return radius == 1 ? vm_median_bisect_launch<1>(src, dst, nx, ny, nz, st) : radius == 2 ? vm_median_bisect_launch<2>(src, dst, nx, ny, nz, st)
                                                                                            : vm_median_cols_launch<3>(src, dst, nx, ny, nz, st);
}

// ---- histogram and Otsu ----------------------------------------------------------------------------------------------------------
struct VmHead {                       // the head of a workspace (zeroed at the start of a call)
    unsigned long long hist[256];
    unsigned nkmin, kmax;             // max of ~key and max of key over the finite values: both 0 while there is none
    unsigned long long winner;        // (count << 32) | ~label
    unsigned long long pad[5];
};
static_assert(sizeof(VmHead) == 2048 + 56, "VmHead");
constexpr size_t VM_HEAD = 2112;      // sizeof(VmHead) rounded to 64

__device__ inline int vm_bin(float v, float lo, float hi) {
    const double t = ((double)v - (double)lo) / ((double)hi - (double)lo) * 256.0;
    const long long b = (long long)floor(t);
    return (int)(b < 255 ? b : 255);
}

__global__ __launch_bounds__(VM_T) void vm_minmax_kernel(const float *__restrict__ v, int64_t n, VmHead *head) {
    __shared__ unsigned sm[2];
    if (threadIdx.x < 2) sm[threadIdx.x] = 0;
    __syncthreads();
    unsigned a = 0, b = 0;
    for (int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * VM_T) {
        const unsigned u = __float_as_uint(v[i]);
        if (vm_finite(u)) { const unsigned k = vm_key(u); a = max(a, ~k); b = max(b, k); }
    }
    if (b) { atomicMax(&sm[0], a); atomicMax(&sm[1], b); }        // (a finite value's key is never 0)
    __syncthreads();
    if (threadIdx.x == 0 && sm[1]) { atomicMax(&head->nkmin, sm[0]); atomicMax(&head->kmax, sm[1]); }
}

__global__ __launch_bounds__(VM_T) void vm_hist_kernel(const float *__restrict__ v, int64_t n, VmHead *head) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned kmin = ~head->nkmin, kmax = head->kmax;
    const float lo = __uint_as_float(vm_unkey(kmin)), hi = __uint_as_float(vm_unkey(kmax));
    if (kmin > kmax || lo == hi) return;                            // (uniform: no finite value, or one value)
    for (int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * VM_T) {
        const float f = v[i];
        if (vm_finite(__float_as_uint(f))) atomicAdd(&h[vm_bin(f, lo, hi)], 1);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&head->hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// one wave; lane l holds candidates k = 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void vm_otsu_kernel(const VmHead *head, fib_mask_info *info) {
    const int lane = threadIdx.x;
    const unsigned kmin = ~head->nkmin, kmax = head->kmax;
    const bool any = kmin <= kmax;
    const float lo = any ? __uint_as_float(vm_unkey(kmin)) : 0.f, hi = any ? __uint_as_float(vm_unkey(kmax)) : 0.f;
    long long h[4], c = 0, s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { h[j] = (long long)head->hist[4 * lane + j]; c += h[j]; s += (long long)(4 * lane + j) * h[j]; }
    long long ci = c, si = s;                                       // inclusive sums across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long cu = __shfl_up(ci, o), su = __shfl_up(si, o);
        if (lane >= o) { ci += cu; si += su; }
    }
    const long long C = __shfl(ci, 63), S = __shfl(si, 63);
    long long c0 = ci - c, s0 = si - s;
    double best = -1.0;
    int bestk = 1 << 30;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int k = 4 * lane + j;
        c0 += h[j]; s0 += (long long)k * h[j];
        const long long c1 = C - c0, s1 = S - s0;
        if (k <= 254 && c0 > 0 && c1 > 0) {
            const long long d = s0 * c1 - s1 * c0;
            const double crit = ((double)d * (double)d) / ((double)c0 * (double)c1);
            if (crit > best) { best = crit; bestk = k; }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int ok = __shfl_xor(bestk, o);
        if (ob > best || (ob == best && ok < bestk)) { best = ob; bestk = ok; }
    }
    if (lane == 0) {
        const bool degenerate = !any || lo == hi || best < 0.0;
        info->status = degenerate ? 1 : 0;
        info->kstar = degenerate ? -1 : bestk;
        info->lo = lo; info->hi = hi;
        info->threshold = degenerate ? 0.0 : __dadd_rn((double)lo, __dmul_rn((double)(bestk + 1), (double)hi - (double)lo) / 256.0);
    }
}

__global__ __launch_bounds__(VM_T) void vm_threshold_kernel(const float *__restrict__ v, int64_t n, fib_mask_info *info, uint8_t *__restrict__ m) {
    const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
    bool above = false;
    if (i < n && info->status == 0) {
        const float f = v[i];
        above = vm_finite(__float_as_uint(f)) && vm_bin(f, info->lo, info->hi) > info->kstar;
    }
    if (i < n) m[i] = above ? 1 : 0;
    vm_count(reinterpret_cast<unsigned long long *>(&info->n_above), above);
}

// ---- components ------------------------------------------------------------------------------------------------------------------
// P[i] <= i always and entries only decrease, so a chain of parents strictly descends and ends at a root; a union lowers the larger
// root onto the smaller by atomicMin and follows whoever got there first.  Nothing here waits: a lane that loses a race has a smaller
// value to go on with.  The caps are never reached by a descending chain (find: at most n steps); reaching one sets status = -1.
__device__ inline int vm_load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ inline int vm_find(const int *P, int i, int cap, fib_mask_info *info) {
    int p = vm_load(P + i);
    for (int it = 0; p != i; it++) {
        if (it >= cap) { info->status = -1; break; }
        i = p; p = vm_load(P + i);
    }
    return i;
}

__device__ inline void vm_union(int *P, int a, int b, int cap, fib_mask_info *info) {
    for (int it = 0;; it++) {
        if (it >= VM_UNION_CAP) { info->status = -1; return; }
        a = vm_find(P, a, cap, info); b = vm_find(P, b, cap, info);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }              // a > b: a's root goes under b
        const int old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;                                                    // someone lowered a first: go on from there
    }
}

#define VM_FG(i) ((m[i] != 0) != (invert != 0))

__global__ __launch_bounds__(VM_T) void vm_cc_init_kernel(const uint8_t *__restrict__ m, int invert, int n, int *__restrict__ P, int *__restrict__ cnt) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    if (i >= n) return;
    P[i] = VM_FG(i) ? i : -1;
    cnt[i] = 0;
}
__global__ __launch_bounds__(VM_T) void vm_cc_merge_kernel(const uint8_t *__restrict__ m, int invert, int nx, int ny, int nz, int *P, fib_mask_info *info) {
    const int n = nx * ny * nz, i = blockIdx.x * VM_T + threadIdx.x;
    if (i >= n || !VM_FG(i)) return;
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny);
    if (x > 0 && VM_FG(i - 1)) vm_union(P, i, i - 1, n, info);
    if (y > 0 && VM_FG(i - nx)) vm_union(P, i, i - nx, n, info);
    if (z > 0 && VM_FG(i - nx * ny)) vm_union(P, i, i - nx * ny, n, info);
}
// every voxel points at its root; its component's size on the root (one atomic a wave where the wave is in one component)
__global__ __launch_bounds__(VM_T) void vm_cc_flatten_kernel(int n, int *P, int *cnt, fib_mask_info *info) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    int root = -1;
    if (i < n && vm_load(P + i) >= 0) { root = vm_find(P, i, n, info); P[i] = root; }
    if (root < 0) return;
    const int first = __builtin_amdgcn_readfirstlane(root);
    const unsigned long long same = __ballot(root == first);
    if (root != first) atomicAdd(cnt + root, 1);
    else if (__lane_id() == (unsigned)(__ffsll((long long)same) - 1)) atomicAdd(cnt + root, (int)__popcll(same));
}
__global__ __launch_bounds__(VM_T) void vm_cc_roots_kernel(int n, const int *__restrict__ P, const int *__restrict__ cnt, VmHead *head, fib_mask_info *info) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    const bool root = i < n && P[i] == i;
    if (root) atomicMax(&head->winner, ((unsigned long long)(unsigned)cnt[i] << 32) | (unsigned)~(unsigned)(i + 1));
    vm_count(reinterpret_cast<unsigned long long *>(&info->n_components), root);
}
__global__ __launch_bounds__(VM_T) void vm_cc_select_kernel(int n, const int *__restrict__ P, const VmHead *head, int keep_largest, uint8_t *__restrict__ sel, fib_mask_info *info) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    const unsigned win = ~(unsigned)(head->winner & 0xffffffffu);  // the winner's label (0xffffffff: there is no component)
    const bool in = i < n && P[i] >= 0 && (!keep_largest || (unsigned)(P[i] + 1) == win);
    if (i < n) sel[i] = in ? 1 : 0;
    vm_count(reinterpret_cast<unsigned long long *>(&info->n_kept), in);
}
// holes: the flattened components of the complement; a root's size (>= 1) gives way to -1 where one of its voxels is on a face
__global__ __launch_bounds__(VM_T) void vm_cc_face_kernel(int nx, int ny, int nz, const int *__restrict__ P, int *flag) {
    const int n = nx * ny * nz, i = blockIdx.x * VM_T + threadIdx.x;
    if (i >= n || P[i] < 0) return;
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny);
    if (x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1) flag[P[i]] = -1;
}
__global__ __launch_bounds__(VM_T) void vm_cc_fill_kernel(int n, const int *__restrict__ P, const int *__restrict__ flag, uint8_t *sel, fib_mask_info *info) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    const bool fill = i < n && P[i] >= 0 && flag[P[i]] > 0;
    if (fill) sel[i] = 1;
    vm_count(reinterpret_cast<unsigned long long *>(&info->n_filled), fill);
}
__global__ __launch_bounds__(VM_T) void vm_cc_labels_kernel(int n, const int *__restrict__ P, const uint8_t *__restrict__ sel, int32_t *__restrict__ labels) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    if (i < n) labels[i] = sel[i] && P[i] >= 0 ? P[i] + 1 : 0;
}

__global__ __launch_bounds__(VM_T) void vm_dilate_kernel(const uint8_t *__restrict__ m, int nx, int ny, int nz, uint8_t *__restrict__ out) {
    const int n = nx * ny * nz, i = blockIdx.x * VM_T + threadIdx.x;
    if (i >= n) return;
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny), p = nx * ny;
    uint8_t v = m[i];
    if (x > 0) v |= m[i - 1];
    if (x < nx - 1) v |= m[i + 1];
    if (y > 0) v |= m[i - nx];
    if (y < ny - 1) v |= m[i + nx];
    if (z > 0) v |= m[i - p];
    if (z < nz - 1) v |= m[i + p];
    out[i] = v ? 1 : 0;
}
// a mask leaves the workspace (out may be NULL) and is counted
__global__ __launch_bounds__(VM_T) void vm_finish_kernel(const uint8_t *__restrict__ m, int n, uint8_t *__restrict__ out, int64_t *count) {
    const int i = blockIdx.x * VM_T + threadIdx.x;
    const bool in = i < n && m[i] != 0;
    if (i < n && out) out[i] = in ? 1 : 0;
    vm_count(reinterpret_cast<unsigned long long *>(count), in);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline unsigned vm_blocks(int64_t n) { return (unsigned)fib::cdiv(n, VM_T); }
inline size_t vm_up(size_t b) { return (b + 63) & ~(size_t)63; }

int vm_dims(int nx, int ny, int nz, int64_t *n) {
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    *n = (int64_t)nx * ny * nz;
    return FIB_OK;
}
int vm_median_args(int radius, int numpass) {
    FIB_CHECK(radius >= 1 && radius <= 3, FIB_ERR_INVALID, "the median's radius must be 1, 2 or 3, not %d", radius);
    FIB_CHECK(numpass >= 0, FIB_ERR_INVALID, "numpass must not be negative (%d)", numpass);
    return FIB_OK;
}
int vm_work_ok(const void *work, size_t work_bytes, size_t need, const char *name) {
    FIB_CHECK(work != nullptr, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "workspace of %zu bytes, %zu needed (%s)", work_bytes, need, name);
    FIB_CHECK(reinterpret_cast<uintptr_t>(work) % 8 == 0, FIB_ERR_INVALID, "the workspace must be 8-byte aligned");
    return FIB_OK;
}

// the workspace of the components: head | parent int32 [n] | count / face flag int32 [n] | selected uint8 [n]
struct CcWork {
    VmHead *head; int *P, *cnt; uint8_t *sel;
    static size_t bytes(int64_t n) { return VM_HEAD + 2 * vm_up(4 * (size_t)n) + vm_up((size_t)n); }
    CcWork(void *w, int64_t n) {
        char *c = static_cast<char *>(w);
        head = reinterpret_cast<VmHead *>(c); c += VM_HEAD;
        P = reinterpret_cast<int *>(c); c += vm_up(4 * (size_t)n);
        cnt = reinterpret_cast<int *>(c); c += vm_up(4 * (size_t)n);
        sel = reinterpret_cast<uint8_t *>(c);
    }
};
// the workspace of dwi_mask: the components' | b0 float [n] | median float [n] | its scratch float [n] | mask uint8 [n]; the float64
// sums of the mean lie over parent and count, which begin their lives after the mean is final
struct MaskWork {
    CcWork cc; float *b0, *med, *med2; uint8_t *m1; double *acc;
    static size_t bytes(int64_t n) { return CcWork::bytes(n) + 3 * vm_up(4 * (size_t)n) + vm_up((size_t)n); }
    MaskWork(void *w, int64_t n) : cc(w, n) {
        char *c = static_cast<char *>(w) + CcWork::bytes(n);
        b0 = reinterpret_cast<float *>(c); c += vm_up(4 * (size_t)n);
        med = reinterpret_cast<float *>(c); c += vm_up(4 * (size_t)n);
        med2 = reinterpret_cast<float *>(c); c += vm_up(4 * (size_t)n);
        m1 = reinterpret_cast<uint8_t *>(c);
        acc = reinterpret_cast<double *>(cc.P);
    }
};

// numpass passes from `in` to `out` (numpass >= 1), alternating through `tmp` so that the last one lands in out
int vm_median_run(const float *in, int nx, int ny, int nz, int radius, int numpass, float *out, float *tmp, hipStream_t st) {
    const float *src = in;
    for (int p = 1; p <= numpass; p++) {
        float *dst = (numpass - p) % 2 == 0 ? out : tmp;
        fib::ProfScope prof("vm_median", st);
        FIB_RC(vm_median_pass(src, dst, nx, ny, nz, radius, st));
        FIB_HIP(hipGetLastError());
        src = dst;
    }
    return FIB_OK;
}

// components of (m != 0) != invert into w.P (flattened) with sizes in w.cnt
int vm_cc_label(const uint8_t *m, int invert, int nx, int ny, int nz, const CcWork &w, fib_mask_info *info, hipStream_t st) {
    const int n = nx * ny * nz;
    const dim3 g(vm_blocks(n)), b(VM_T);
    fib::ProfScope prof("vm_cc_label", st);
    hipLaunchKernelGGL(vm_cc_init_kernel, g, b, 0, st, m, invert, n, w.P, w.cnt);
    hipLaunchKernelGGL(vm_cc_merge_kernel, g, b, 0, st, m, invert, nx, ny, nz, w.P, info);
    hipLaunchKernelGGL(vm_cc_flatten_kernel, g, b, 0, st, n, w.P, w.cnt, info);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

// mask `m` (nonzero = inside) -> w.sel: components, the largest kept, holes filled; labels (or NULL) of the result's components.
// info's counters must be zero on entry; w.head->winner too.
int vm_components_run(const uint8_t *m, int nx, int ny, int nz, int flags, int32_t *labels, const CcWork &w, fib_mask_info *info, hipStream_t st) {
    const int n = nx * ny * nz;
    const dim3 g(vm_blocks(n)), b(VM_T);
    FIB_RC(vm_cc_label(m, 0, nx, ny, nz, w, info, st));
    hipLaunchKernelGGL(vm_cc_roots_kernel, g, b, 0, st, n, w.P, w.cnt, w.head, info);
    hipLaunchKernelGGL(vm_cc_select_kernel, g, b, 0, st, n, w.P, w.head, (flags & FIB_MASK_KEEP_LARGEST) ? 1 : 0, w.sel, info);
    if (labels && !(flags & FIB_MASK_FILL_HOLES)) hipLaunchKernelGGL(vm_cc_labels_kernel, g, b, 0, st, n, w.P, w.sel, labels);
    if (flags & FIB_MASK_FILL_HOLES) {
        FIB_RC(vm_cc_label(w.sel, 1, nx, ny, nz, w, info, st));
        fib::ProfScope prof("vm_cc_fill", st);
        hipLaunchKernelGGL(vm_cc_face_kernel, g, b, 0, st, nx, ny, nz, w.P, w.cnt);
        hipLaunchKernelGGL(vm_cc_fill_kernel, g, b, 0, st, n, w.P, w.cnt, w.sel, info);
        if (labels) {                                       // (labels are of the result's components: once more over the filled mask)
            FIB_RC(vm_cc_label(w.sel, 0, nx, ny, nz, w, info, st));
            hipLaunchKernelGGL(vm_cc_labels_kernel, g, b, 0, st, n, w.P, w.sel, labels);
        }
    }
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

// b0 (final, in w.b0 or the caller's) -> mask
int vm_mask_run(const float *b0, int nx, int ny, int nz, const fib_mask_params *p, uint8_t *mask, fib_mask_info *info, const MaskWork &w, hipStream_t st) {
    const int64_t n = (int64_t)nx * ny * nz;
    const dim3 g(vm_blocks(n)), b(VM_T);
    const float *v = b0;
    if (p->numpass > 0) { FIB_RC(vm_median_run(b0, nx, ny, nz, p->radius, p->numpass, w.med, w.med2, st)); v = w.med; }
    const unsigned gs = std::min<unsigned>(vm_blocks(n), 2048);
    {
        fib::ProfScope prof("vm_minmax_hist", st);
        hipLaunchKernelGGL(vm_minmax_kernel, dim3(gs), b, 0, st, v, n, w.cc.head);
        hipLaunchKernelGGL(vm_hist_kernel, dim3(gs), b, 0, st, v, n, w.cc.head);
    }
    {
        fib::ProfScope prof("vm_otsu", st);
        hipLaunchKernelGGL(vm_otsu_kernel, dim3(1), dim3(64), 0, st, w.cc.head, info);
    }
    {
        fib::ProfScope prof("vm_threshold", st);
        hipLaunchKernelGGL(vm_threshold_kernel, g, b, 0, st, v, n, info, w.m1);
    }
    FIB_HIP(hipGetLastError());
    FIB_RC(vm_components_run(w.m1, nx, ny, nz, p->flags, nullptr, w.cc, info, st));
    uint8_t *cur = w.cc.sel, *other = w.m1;
    {
        fib::ProfScope prof("vm_dilate", st);
        for (int d = 0; d < p->dilate; d++) {
            hipLaunchKernelGGL(vm_dilate_kernel, g, b, 0, st, cur, nx, ny, nz, other);
            std::swap(cur, other);
        }
        hipLaunchKernelGGL(vm_finish_kernel, g, b, 0, st, cur, (int)n, mask, &info->n_mask);
    }
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

int vm_params(const fib_mask_params *p) {
    FIB_CHECK(p != nullptr, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(p->radius >= 1 && p->radius <= 3, FIB_ERR_INVALID, "dwi_mask: the median's radius must be 1, 2 or 3, not %d", p->radius);
    FIB_CHECK(p->numpass >= 0, FIB_ERR_INVALID, "dwi_mask: numpass must not be negative (%d)", p->numpass);
    FIB_CHECK(p->dilate >= 0, FIB_ERR_INVALID, "dwi_mask: dilate must not be negative (%d)", p->dilate);
    FIB_CHECK((p->flags & ~(FIB_MASK_KEEP_LARGEST | FIB_MASK_FILL_HOLES)) == 0, FIB_ERR_INVALID, "dwi_mask: unknown flags 0x%x", p->flags);
    return FIB_OK;
}

int vm_start(void *work, fib_mask_info *info, hipStream_t st) {
    FIB_HIP(hipMemsetAsync(work, 0, VM_HEAD, st));
    FIB_HIP(hipMemsetAsync(info, 0, sizeof(fib_mask_info), st));
    return FIB_OK;
}

}  // namespace

// ---- what fib_dwi_mask is made of (common.h) -------------------------------------------------------------------------------------
namespace fib {
int vm_mean_add(void *work, const float *frames, int64_t nvox, int nf, bool first, hipStream_t st) {
    MaskWork w(work, nvox);
    fib::ProfScope prof("vm_mean_frames", st);
    hipLaunchKernelGGL(vm_mean_acc_kernel, dim3(vm_blocks(nvox)), dim3(VM_T), 0, st, w.acc, frames, nvox, nf, first ? 1 : 0);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}
int vm_mask_finish(void *work, int count, int nx, int ny, int nz, const fib_mask_params *p, uint8_t *mask, float *b0, fib_mask_info *info,
                   hipStream_t st) {
    const int64_t n = (int64_t)nx * ny * nz;
    MaskWork w(work, n);
    float *mean = b0 ? b0 : w.b0;
    hipLaunchKernelGGL(vm_mean_fin_kernel, dim3(vm_blocks(n)), dim3(VM_T), 0, st, w.acc, count, n, mean);
    FIB_HIP(hipGetLastError());
    FIB_RC(vm_start(work, info, st));                       // (the head lies in front of the sums)
    return vm_mask_run(mean, nx, ny, nz, p, mask, info, w, st);
}
}  // namespace fib

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int fib_dwi_mask_check(int nx, int ny, int nz, int nvol, const int32_t *frames, int nframes, const fib_mask_params *params) try {
    int64_t n;
    FIB_RC(vm_dims(nx, ny, nz, &n));
    FIB_CHECK(nvol >= 1, FIB_ERR_INVALID, "dwi_mask: the series must have at least one frame, not %d", nvol);
    FIB_RC(vm_params(params));
    FIB_CHECK(frames != nullptr && nframes >= 1, FIB_ERR_INVALID, "dwi_mask: the frame list is empty");
    for (int f = 0; f < nframes; f++)
        FIB_CHECK(frames[f] >= 0 && frames[f] < nvol, FIB_ERR_INVALID, "dwi_mask: frame %d (entry %d of the list) is outside [0, %d)", frames[f], f, nvol);
    FIB_CHECK(n <= VM_MAXVOX, FIB_ERR_UNSUPPORTED, "dwi_mask: %lld voxels; the limit is 2^27 (the integer Otsu criterion must stay inside int64)",
              (long long)n);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_vol_median_work_size(int nx, int ny, int nz, int numpass, size_t *bytes) try {
    int64_t n;
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(vm_dims(nx, ny, nz, &n));
    FIB_CHECK(numpass >= 0, FIB_ERR_INVALID, "numpass must not be negative (%d)", numpass);
    *bytes = numpass >= 2 ? vm_up(4 * (size_t)n) : 64;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_vol_median(const float *in, int nx, int ny, int nz, int radius, int numpass, float *out, void *work, size_t work_bytes,
                               void *stream) try {
    int64_t n;
    size_t need;
    FIB_CHECK(in && out, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(vm_dims(nx, ny, nz, &n));
    FIB_RC(vm_median_args(radius, numpass));
    FIB_CHECK(in != out, FIB_ERR_INVALID, "vol_median: in and out must not be the same buffer");
    FIB_RC(fibd_vol_median_work_size(nx, ny, nz, numpass, &need));
    FIB_RC(vm_work_ok(work, work_bytes, need, "fibd_vol_median_work_size"));
    const hipStream_t st = (hipStream_t)stream;
    if (numpass == 0) {
        FIB_HIP(hipMemcpyAsync(out, in, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, st));
        return FIB_OK;
    }
    return vm_median_run(in, nx, ny, nz, radius, numpass, out, static_cast<float *>(work), st);
} FIB_API_CATCH

extern "C" int fibd_mask_components_work_size(int nx, int ny, int nz, size_t *bytes) try {
    int64_t n;
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(vm_dims(nx, ny, nz, &n));
    FIB_CHECK(n <= VM_MAXVOX, FIB_ERR_UNSUPPORTED, "mask_components: %lld voxels; the limit is 2^27", (long long)n);
    *bytes = CcWork::bytes(n);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_mask_components(const uint8_t *mask, int nx, int ny, int nz, int flags, int32_t *labels, uint8_t *out_mask, fib_mask_info *info,
                                    void *work, size_t work_bytes, void *stream) try {
    size_t need;
    FIB_CHECK(mask && info, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(fibd_mask_components_work_size(nx, ny, nz, &need));
    FIB_CHECK((flags & ~(FIB_MASK_KEEP_LARGEST | FIB_MASK_FILL_HOLES)) == 0, FIB_ERR_INVALID, "mask_components: unknown flags 0x%x", flags);
    FIB_RC(vm_work_ok(work, work_bytes, need, "fibd_mask_components_work_size"));
    const hipStream_t st = (hipStream_t)stream;
    const int n = nx * ny * nz;
    CcWork w(work, n);
    FIB_RC(vm_start(work, info, st));
    hipLaunchKernelGGL(vm_finish_kernel, dim3(vm_blocks(n)), dim3(VM_T), 0, st, mask, n, (uint8_t *)nullptr, &info->n_above);
    FIB_RC(vm_components_run(mask, nx, ny, nz, flags, labels, w, info, st));
    hipLaunchKernelGGL(vm_finish_kernel, dim3(vm_blocks(n)), dim3(VM_T), 0, st, w.sel, n, out_mask, &info->n_mask);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dwi_mask_work_size(int nx, int ny, int nz, size_t *bytes) try {
    int64_t n;
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(vm_dims(nx, ny, nz, &n));
    FIB_CHECK(n <= VM_MAXVOX, FIB_ERR_UNSUPPORTED, "dwi_mask: %lld voxels; the limit is 2^27 (the integer Otsu criterion must stay inside int64)",
              (long long)n);
    *bytes = MaskWork::bytes(n);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dwi_mask(const float *dwi, int64_t frame_stride, int nvol, const int32_t *frames, int nframes, int nx, int ny, int nz,
                             const fib_mask_params *params, uint8_t *mask, float *b0, fib_mask_info *info, void *work, size_t work_bytes,
                             void *stream) try {
    size_t need;
    FIB_CHECK(dwi && mask && info, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(fib_dwi_mask_check(nx, ny, nz, nvol, frames, nframes, params));
    const int64_t n = (int64_t)nx * ny * nz;
    FIB_CHECK(frame_stride >= n, FIB_ERR_INVALID, "dwi_mask: a frame stride of %lld for frames of %lld voxels", (long long)frame_stride, (long long)n);
    FIB_RC(fibd_dwi_mask_work_size(nx, ny, nz, &need));
    FIB_RC(vm_work_ok(work, work_bytes, need, "fibd_dwi_mask_work_size"));
    const hipStream_t st = (hipStream_t)stream;
    MaskWork w(work, n);
    float *mean = b0 ? b0 : w.b0;
    if (nframes <= VM_LIST) {                                // mode A: the list travels in the kernel's arguments
        VmFrames fr;
        fr.n = nframes;
        for (int f = 0; f < VM_LIST; f++) fr.idx[f] = f < nframes ? frames[f] : 0;
        fib::ProfScope prof("vm_mean_frames", st);
        hipLaunchKernelGGL(vm_mean_frames_kernel, dim3(vm_blocks(n)), dim3(VM_T), 0, st, dwi, frame_stride, fr, n, mean);
        FIB_HIP(hipGetLastError());
    } else {                                                 // mode B, a frame a launch
        for (int f = 0; f < nframes; f++) FIB_RC(fib::vm_mean_add(work, dwi + (int64_t)frames[f] * frame_stride, n, 1, f == 0, st));
        hipLaunchKernelGGL(vm_mean_fin_kernel, dim3(vm_blocks(n)), dim3(VM_T), 0, st, w.acc, nframes, n, mean);
        FIB_HIP(hipGetLastError());
    }
    FIB_RC(vm_start(work, info, st));
    return vm_mask_run(mean, nx, ny, nz, params, mask, info, w, st);
} FIB_API_CATCH
