// fixel.hip — tractogram weights on gfx950: every line gets a weight so that the weighted track density of every fibre population
// ("fixel": one peak in one voxel) matches that peak's amplitude.  Not in the reference: the definitions are the "Tractogram weights"
// section of include/fibers_hip.h.  Inputs are packed lines (xyz float32 [npoints][3], npts int32 [nlines]) and the peak field as
// fibd_stream_field takes it (ovec[k] planar [3][nvox], f[k] [nvox]).  Every sum that decides a weight is an INTEGER sum (weights in
// units of 2^-20, amplitudes quantised once), so the atomic adds may arrive in any order and two runs give the same bytes.
//
// Kernels
//   ls_block / ls_totals / ls_apply <TmItem>   (line_scan.inc, tm_lines.inc) the first point of every line and the verdict on npts
//   fx_max / fx_quantise   the largest amplitude of an existing fixel (atomic max on the bits of positive floats), then Aq and its sum
//   fx_assign       G lanes per line: tangent, the best-aligned existing fixel of the point's voxel, the cone test -> int32 id per point
//   fx_td           G lanes per line, G points per round: a run of equal ids inside the round is ONE vector atomic add of q * length
//                   on uint64 (a line at q = 0 adds nothing)
//   fx_update       G lanes per line: D_s (and N_s on the first call) gathered through the ids, a butterfly over the group, the ISRA
//                   update of q in float64 on lane 0; counts the gathered TDq >= 2^44
//   fx_sum_td / fx_mu      the sum of the initial TDq, then mu (one lane)
//   fx_cost / fx_cost_final   a fixed grid's strided float64 partial sums, then ONE wave adds them in a fixed order (the same bytes
//                   on every run, and in the device and the host form)
//   fx_output       weights, the clamp / zero counts;  fx_td_output: the fitted density as float32
#include "common.h"

#include <algorithm>

// every float32 / float64 operation of the definitions is rounded on its own: nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "tm_lines.inc"                                        // TM_BLOCK, tm_voxel, the offset scan (tm_offsets), tm_check_lines

constexpr int FX_G = 16;                                       // lanes per line of fx_assign / fx_td / fx_update
constexpr int FX_COST_GRID = 256;                              // workgroups of fx_cost: the number of partial sums, fixed
constexpr uint64_t FX_TD_LIMIT = (uint64_t)1 << 44;
static_assert(sizeof(double) * FX_COST_GRID == FIB_FIXEL_COST_WORK_BYTES, "the size the header states");
constexpr uint32_t FX_Q_ONE = 1u << 20, FX_Q_CLAMP = 0xffffffffu;

// the state of a fit in device memory: FIB_FIXEL_STATE_SLOTS slots of 8 bytes (include/fibers_hip.h)
struct FxState {
    double a_scale, mu;
    uint64_t sum_aq, sum_td0, fmax_bits;
    int64_t n_unassigned, n_lines_without, n_clamp, n_zero, overflow;
    int64_t reserved[6];
};
static_assert(sizeof(FxState) == 8 * FIB_FIXEL_STATE_SLOTS, "the layout the header states");

struct FxField {                                               // the peak field, by value
    const float *ovec[3], *f[3];
    const uint8_t *mask;
    int64_t nvox;
    int nvec;
    float f_thresh;
};

// fixel (k, v) exists: mask, a finite amplitude above the threshold, a finite direction that is not zero
__device__ __forceinline__ bool fx_exists(const FxField &fld, int k, int64_t v, float &ux, float &uy, float &uz) {
    if (fld.mask && !fld.mask[v]) return false;
    const float a = fld.f[k][v];
    if (!(isfinite(a) && a > fld.f_thresh)) return false;
    ux = fld.ovec[k][v]; uy = fld.ovec[k][fld.nvox + v]; uz = fld.ovec[k][2 * fld.nvox + v];
    return isfinite(ux) && isfinite(uy) && isfinite(uz) && !(ux == 0.0f && uy == 0.0f && uz == 0.0f);
}

template <int G>
__device__ __forceinline__ int64_t fx_group_sum(int64_t s) {
    for (int d = G / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, G);
    return s;
}

// ---- quantise --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void fx_max(const FxField fld, FxState *st) {
    const int64_t nfix = fld.nvox * fld.nvec;
    uint32_t best = 0;
    for (int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < nfix; i += (int64_t)gridDim.x * TM_BLOCK) {
        const int k = (int)(i / fld.nvox);
        const int64_t v = i - (int64_t)k * fld.nvox;
        float ux, uy, uz;
        if (fx_exists(fld, k, v, ux, uy, uz)) best = max(best, __float_as_uint(fld.f[k][v]));   // (amplitudes above f_thresh >= 0: positive)
    }
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(reinterpret_cast<unsigned long long *>(&st->fmax_bits), (unsigned long long)best);
}

__global__ __launch_bounds__(TM_BLOCK) void fx_quantise(const FxField fld, FxState *st, uint64_t *aq) {
    const int64_t nfix = fld.nvox * fld.nvec;
    const uint32_t bits = (uint32_t)st->fmax_bits;
    const double a_scale = bits ? 1073741824.0 / (double)__uint_as_float(bits) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->a_scale = a_scale;
    int64_t sum = 0;
    for (int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < nfix; i += (int64_t)gridDim.x * TM_BLOCK) {
        const int k = (int)(i / fld.nvox);
        const int64_t v = i - (int64_t)k * fld.nvox;
        float ux, uy, uz;
        uint64_t q = 0;
        if (fx_exists(fld, k, v, ux, uy, uz)) q = (uint64_t)rint((double)fld.f[k][v] * a_scale);
        aq[i] = q;
        sum += (int64_t)q;
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long *>(&st->sum_aq), (unsigned long long)sum);
}

// ---- assign ----------------------------------------------------------------------------------------------------------------------
// G lanes per line; lane g takes points g, g + G, ... of its line.  counts[0] += unassigned points, counts[1] += lines without an
// assigned point (empty lines included).
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void fx_assign(const FxField fld, const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines,
                                                      int nx, int ny, int nz, float cos2, const TmHead *head, int32_t *ids, int64_t *counts) {
    if (!head->ok) return;
    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    if (line >= nlines) return;                                 // (whole groups leave together)
    const int n = npts[line];
    const int64_t first = off[line];
    int64_t unassigned = 0, assigned = 0;
    for (int k = g; k < n; k += G) {
        int32_t id = -1;
        if (n >= 2) {
            const float *p = xyz + 3 * (first + k);
            const float *a = k > 0 ? p - 3 : p, *b = k < n - 1 ? p + 3 : p;
            const int64_t v = tm_voxel(p[0], p[1], p[2], nx, ny, nz);
            const float tx = b[0] - a[0], ty = b[1] - a[1], tz = b[2] - a[2];
            const bool usable = isfinite(tx) && isfinite(ty) && isfinite(tz) && !(tx == 0.0f && ty == 0.0f && tz == 0.0f);
            if (v >= 0 && usable) {
                float best = -1.0f, bd = 0.0f;
                int bk = -1;
                for (int kk = 0; kk < fld.nvec; kk++) {
                    float ux, uy, uz;
                    if (!fx_exists(fld, kk, v, ux, uy, uz)) continue;
                    const float d = (tx * ux + ty * uy) + tz * uz;
                    const float ad = fabsf(d);
                    if (ad > best) { best = ad; bd = d; bk = kk; }   // (a NaN is never larger; a tie keeps the smaller k)
                }
                if (bk >= 0) {
                    const float tt = (tx * tx + ty * ty) + tz * tz;
                    if (bd * bd >= cos2 * tt) id = (int32_t)((int64_t)bk * fld.nvox + v);
                }
            }
        }
        ids[first + k] = id;
        if (id < 0) unassigned++; else assigned++;
    }
    unassigned = fx_group_sum<G>(unassigned);
    assigned = fx_group_sum<G>(assigned);
    if (g == 0) {
        if (unassigned) atomicAdd(reinterpret_cast<unsigned long long *>(counts), (unsigned long long)unassigned);
        if (!assigned) atomicAdd(reinterpret_cast<unsigned long long *>(counts + 1), 1ull);
    }
}

// ---- scatter ---------------------------------------------------------------------------------------------------------------------
// G lanes per line, round r takes points [G r, G r + G) of the line; a run of equal ids inside a round is one atomic add.
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void fx_td(const int32_t *ids, const int32_t *npts, const int64_t *off, int64_t nlines, const uint32_t *q,
                                                  int64_t nfix, const TmHead *head, uint64_t *tdq) {
    if (!head->ok) return;
    const int lane = threadIdx.x & 63, g = lane % G, gbase = lane - g;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    int n = 0;
    int64_t first = 0;
    uint64_t w = 0;
    if (line < nlines) { n = npts[line]; first = off[line]; w = q[line]; }
    if (w == 0) n = 0;                                          // (adds nothing)
    for (int base = 0; __any(base < n); base += G) {            // (the wave stays together: the ballot below is over all 64 lanes)
        const int k = base + g;
        int32_t id = k < n ? ids[first + k] : -2;
        if (id >= nfix) id = -1;                                // (ids are the caller's in fibd_fixel_td: nothing is added out of bounds)
        const int32_t prev = __shfl_up(id, 1, G);
        const bool head_of_run = g == 0 || id != prev;
        const uint64_t heads = (__ballot(head_of_run) >> gbase) & ((1ull << G) - 1);
        if (head_of_run && id >= 0) {
            const uint64_t above = heads >> (g + 1);
            const int len = above ? __ffsll((unsigned long long)above) : G - g;
            atomicAdd(reinterpret_cast<unsigned long long *>(tdq + id), (unsigned long long)(w * (uint64_t)len));
        }
    }
}

// ---- update ----------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void fx_update(const int32_t *ids, const int32_t *npts, const int64_t *off, int64_t nlines, const uint64_t *aq,
                                                      const uint64_t *tdq, int64_t nfix, int first_call, const TmHead *head, FxState *st, uint64_t *nline, uint32_t *q) {
    if (!head->ok) return;
    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    if (line >= nlines) return;                                 // (whole groups leave together)
    const int n = npts[line];
    const int64_t first = off[line];
    int64_t D = 0, N = 0, over = 0, assigned = 0;               // (two's complement: the sums are those of uint64)
    for (int k = g; k < n; k += G) {
        const int32_t id = ids[first + k];
        if (id < 0 || id >= nfix) continue;
        const uint64_t t = tdq[id];
        D += (int64_t)t;
        over += t >= FX_TD_LIMIT;
        assigned++;
        if (first_call) N += (int64_t)aq[id];
    }
    D = fx_group_sum<G>(D);
    over = fx_group_sum<G>(over);
    assigned = fx_group_sum<G>(assigned);
    if (first_call) N = fx_group_sum<G>(N);
    if (g != 0) return;
    if (over) atomicAdd(reinterpret_cast<unsigned long long *>(&st->overflow), (unsigned long long)over);
    if (first_call) nline[line] = (uint64_t)N; else N = (int64_t)nline[line];
    uint32_t qn = 0;
    if (assigned && D != 0) {
        const double w = (double)q[line] * 0x1p-20;
        const double A = (double)(uint64_t)N / st->a_scale;
        const double B = (double)(uint64_t)D * 0x1p-20;
        const double C = st->mu * B;
        const double wn = (w * A) / C;
        qn = (uint32_t)rint(fmin(wn, 4096.0 - 0x1p-20) * 0x1p20);
    }
    q[line] = qn;
}

// ---- mu, cost, outputs -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void fx_sum_td(const uint64_t *tdq, int64_t nfix, FxState *st) {
    int64_t sum = 0;
    for (int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < nfix; i += (int64_t)gridDim.x * TM_BLOCK) sum += (int64_t)tdq[i];
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long *>(&st->sum_td0), (unsigned long long)sum);
}

__global__ void fx_mu(FxState *st) {
    const double a = st->a_scale;
    const uint64_t t = st->sum_td0;
    st->mu = (a > 0.0 && t) ? ((double)st->sum_aq / a) / ((double)t * 0x1p-20) : 0.0;
}

__global__ __launch_bounds__(TM_BLOCK) void fx_cost(const uint64_t *aq, const uint64_t *tdq, int64_t nfix, const FxState *st, double *partial) {
    __shared__ double s_sum[TM_BLOCK / 64];
    const double a = st->a_scale, mu = st->mu;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < nfix; i += (int64_t)gridDim.x * TM_BLOCK) {
        const uint64_t A = aq[i];
        const double x = mu * ((double)tdq[i] * 0x1p-20), y = A ? (double)A / a : 0.0, r = x - y;
        sum += r * r;
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < TM_BLOCK / 64; w++) t += s_sum[w];
        partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void fx_cost_final(const double *partial, double *cost) {
    double sum = 0.0;
    for (int i = threadIdx.x; i < FX_COST_GRID; i += 64) sum += partial[i];
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (threadIdx.x == 0) *cost = sum;
}

__global__ __launch_bounds__(TM_BLOCK) void fx_output(const uint32_t *q, int64_t nlines, float *weights, FxState *st) {
    const int64_t l = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    int64_t clamp = 0, zero = 0;
    if (l < nlines) {
        const uint32_t v = q[l];
        weights[l] = (float)v * 0x1p-20f;
        clamp = v == FX_Q_CLAMP; zero = v == 0;
    }
    for (int d = 32; d >= 1; d >>= 1) { clamp += __shfl_xor(clamp, d); zero += __shfl_xor(zero, d); }
    if ((threadIdx.x & 63) == 0) {
        if (clamp) atomicAdd(reinterpret_cast<unsigned long long *>(&st->n_clamp), (unsigned long long)clamp);
        if (zero) atomicAdd(reinterpret_cast<unsigned long long *>(&st->n_zero), (unsigned long long)zero);
    }
}

__global__ __launch_bounds__(TM_BLOCK) void fx_td_output(const uint64_t *tdq, int64_t nfix, const FxState *st, float *td) {
    const int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (i < nfix) td[i] = (float)(((double)tdq[i] * 0x1p-20) * st->mu);
}

__global__ __launch_bounds__(TM_BLOCK) void fx_fill(uint32_t *q, int64_t n, uint32_t v) {
    const int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (i < n) q[i] = v;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
unsigned fx_grid(int64_t n, int64_t per_block, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min(fib::cdiv(n, per_block), cap)); }

int fx_field(int32_t nvec, int64_t nvox, const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, FxField &fld) {
    FIB_CHECK(nvec >= 1 && nvec <= 3, FIB_ERR_INVALID, "nvec must be 1, 2 or 3, not %d", nvec);
    FIB_CHECK(nvox > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nvox * nvec < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "fixel ids are int32: nvec * nvox must stay below 2^31");
    FIB_CHECK(ovec && f, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(f_thresh >= 0.0f, FIB_ERR_INVALID, "f_thresh must not be negative (amplitudes are positive)");   // (NaN fails too)
    fld = FxField{};
    for (int k = 0; k < nvec; k++) {
        FIB_CHECK(ovec[k] && f[k], FIB_ERR_INVALID, "peak %d is NULL", k);
        fld.ovec[k] = ovec[k]; fld.f[k] = f[k];
    }
    fld.mask = mask; fld.nvox = nvox; fld.nvec = nvec; fld.f_thresh = f_thresh;
    return FIB_OK;
}

int fx_check_lines(const void *ids, const int32_t *npts, int64_t nlines, int64_t npoints) {
    FIB_RC(tm_check_lines(nullptr, npts, nlines, 0));
    FIB_CHECK(npoints >= 0 && npoints < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the weights take fewer than 2^31 points");
    FIB_CHECK(npoints == 0 || ids, FIB_ERR_INVALID, "NULL ids");
    return FIB_OK;
}

unsigned fx_line_grid(int64_t nlines) { return (unsigned)fib::cdiv(nlines * FX_G, TM_BLOCK); }

// the steps on a scan that has been made (w): what the entry points and the driver share
void fx_quantise_launch(const FxField &fld, FxState *st, uint64_t *aq, hipStream_t s) {
    const unsigned grid = fx_grid(fld.nvox * fld.nvec, TM_BLOCK, 4096);
    hipLaunchKernelGGL(fx_max, dim3(grid), dim3(TM_BLOCK), 0, s, fld, st);
    hipLaunchKernelGGL(fx_quantise, dim3(grid), dim3(TM_BLOCK), 0, s, fld, st, aq);
}
void fx_td_launch(const int32_t *ids, const int32_t *npts, const TmWork &w, int64_t nlines, const uint32_t *q, int64_t nfix, uint64_t *tdq, hipStream_t s) {
    if (nlines) hipLaunchKernelGGL(fx_td<FX_G>, dim3(fx_line_grid(nlines)), dim3(TM_BLOCK), 0, s, ids, npts, w.off, nlines, q, nfix, w.head, tdq);
}
void fx_update_launch(const int32_t *ids, const int32_t *npts, const TmWork &w, int64_t nlines, const uint64_t *aq, const uint64_t *tdq, int64_t nfix, int first,
                      FxState *st, uint64_t *nline, uint32_t *q, hipStream_t s) {
    if (nlines) hipLaunchKernelGGL(fx_update<FX_G>, dim3(fx_line_grid(nlines)), dim3(TM_BLOCK), 0, s, ids, npts, w.off, nlines, aq, tdq, nfix, first, w.head,
                                   st, nline, q);
}
void fx_cost_launch(const uint64_t *aq, const uint64_t *tdq, int64_t nfix, const FxState *st, double *partial, double *cost, hipStream_t s) {
    hipLaunchKernelGGL(fx_cost, dim3(FX_COST_GRID), dim3(TM_BLOCK), 0, s, aq, tdq, nfix, st, partial);
    hipLaunchKernelGGL(fx_cost_final, dim3(1), dim3(64), 0, s, partial, cost);
}

size_t fx_align(size_t b) { return (b + 15) & ~(size_t)15; }

// the work area of fibd_str_weights: [scan | partial sums of the cost | Aq | TDq | N_s | ids]
struct FxWork {
    size_t scan, partial, aq, tdq, nline, ids, total;
    FxWork(int64_t nlines, int64_t npoints, int64_t nfix) {
        scan = 0;
        partial = scan + fx_align(tm_work_bytes(nlines));
        aq = partial + fx_align(sizeof(double) * FX_COST_GRID);
        tdq = aq + fx_align(sizeof(uint64_t) * (size_t)nfix);
        nline = tdq + fx_align(sizeof(uint64_t) * (size_t)nfix);
        ids = nline + fx_align(sizeof(uint64_t) * (size_t)std::max<int64_t>(nlines, 1));
        total = ids + fx_align(sizeof(int32_t) * (size_t)std::max<int64_t>(npoints, 1));
    }
};

}  // namespace

extern "C" int fibd_fixel_quantise(int32_t nvec, int64_t nvox, const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh,
                                   uint64_t *aq, void *state, void *stream) try {
    FxField fld;
    FIB_RC(fx_field(nvec, nvox, ovec, f, mask, f_thresh, fld));
    FIB_CHECK(aq && state, FIB_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_quantise", s);
    FIB_HIP(hipMemsetAsync(state, 0, sizeof(FxState), s));
    fx_quantise_launch(fld, reinterpret_cast<FxState *>(state), aq, s);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_assign(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int32_t nvec,
                                 const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2, int32_t *ids,
                                 int64_t *counts, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FxField fld;
    FIB_RC(fx_field(nvec, (int64_t)nx * ny * nz, ovec, f, mask, f_thresh, fld));
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_RC(fx_check_lines(ids, npts, nlines, npoints));
    FIB_CHECK(counts, FIB_ERR_INVALID, "NULL counts");
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_assign", s);
    FIB_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, counts, s, w));
    if (nlines) hipLaunchKernelGGL(fx_assign<FX_G>, dim3(fx_line_grid(nlines)), dim3(TM_BLOCK), 0, s, fld, xyz, npts, w.off, nlines, nx, ny, nz, cos2,
                                   w.head, ids, counts);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_td(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint32_t *q, int64_t nfixels,
                             uint64_t *tdq, void *work, size_t work_bytes, void *stream) try {
    FIB_RC(fx_check_lines(ids, npts, nlines, npoints));
    FIB_CHECK(nfixels > 0 && nfixels < ((int64_t)1 << 31), FIB_ERR_INVALID, "nfixels must be between 1 and 2^31 - 1");
    FIB_CHECK(tdq && (nlines == 0 || q), FIB_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_td", s);
    FIB_HIP(hipMemsetAsync(tdq, 0, sizeof(uint64_t) * (size_t)nfixels, s));
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, nullptr, s, w));
    fx_td_launch(ids, npts, w, nlines, q, nfixels, tdq, s);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_mu(const uint64_t *tdq, int64_t nfixels, void *state, void *stream) try {
    FIB_CHECK(tdq && state && nfixels > 0, FIB_ERR_INVALID, "NULL argument or no fixels");
    hipStream_t s = (hipStream_t)stream;
    FxState *st = reinterpret_cast<FxState *>(state);
    FIB_HIP(hipMemsetAsync(&st->sum_td0, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(fx_sum_td, dim3(fx_grid(nfixels, TM_BLOCK, 4096)), dim3(TM_BLOCK), 0, s, tdq, nfixels, st);
    hipLaunchKernelGGL(fx_mu, dim3(1), dim3(1), 0, s, st);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_update(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint64_t *aq, const uint64_t *tdq,
                                 int64_t nfixels, int first, void *state, uint64_t *nline, uint32_t *q, void *work, size_t work_bytes, void *stream) try {
    FIB_RC(fx_check_lines(ids, npts, nlines, npoints));
    FIB_CHECK(aq && tdq && state && (nlines == 0 || (nline && q)), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nfixels > 0 && nfixels < ((int64_t)1 << 31), FIB_ERR_INVALID, "nfixels must be between 1 and 2^31 - 1");
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_update", s);
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, nullptr, s, w));
    fx_update_launch(ids, npts, w, nlines, aq, tdq, nfixels, first != 0, reinterpret_cast<FxState *>(state), nline, q, s);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_cost(const uint64_t *aq, const uint64_t *tdq, int64_t nfixels, const void *state, double *cost, void *work, size_t work_bytes,
                               void *stream) try {
    FIB_CHECK(aq && tdq && state && cost && nfixels > 0, FIB_ERR_INVALID, "NULL argument or no fixels");
    FIB_RC(ls_check_work(work, work_bytes, sizeof(double) * FX_COST_GRID, "FIB_FIXEL_COST_WORK_BYTES"));
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_cost", s);
    fx_cost_launch(aq, tdq, nfixels, reinterpret_cast<const FxState *>(state), reinterpret_cast<double *>(work), cost, s);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_fixel_output(const uint32_t *q, int64_t nlines, const uint64_t *tdq, int64_t nfixels, void *state, float *weights, float *td,
                                 void *stream) try {
    FIB_CHECK(nlines >= 0 && nfixels >= 0, FIB_ERR_INVALID, "nlines and nfixels must not be negative");
    FIB_CHECK(state && (nlines == 0 || (q && weights)) && (nfixels == 0 || (tdq && td)), FIB_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    FxState *st = reinterpret_cast<FxState *>(state);
    FIB_HIP(hipMemsetAsync(&st->n_clamp, 0, 2 * sizeof(int64_t), s));
    if (nlines) hipLaunchKernelGGL(fx_output, dim3((unsigned)fib::cdiv(nlines, TM_BLOCK)), dim3(TM_BLOCK), 0, s, q, nlines, weights, st);
    if (nfixels) hipLaunchKernelGGL(fx_td_output, dim3((unsigned)fib::cdiv(nfixels, TM_BLOCK)), dim3(TM_BLOCK), 0, s, tdq, nfixels, st, td);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_weights_work_size(int64_t nlines, int64_t npoints, int32_t nvec, int64_t nvox, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nlines >= 0 && npoints >= 0 && nvec >= 1 && nvec <= 3 && nvox > 0, FIB_ERR_INVALID, "sizes must not be negative, nvec 1 to 3");
    *bytes = FxWork(nlines, npoints, nvox * nvec).total;
    return FIB_OK;
} FIB_API_CATCH

// the iterations on ids that have been made: q holds the start weights.  Shared by fibd_str_weights and (through fibd_fixel_fit) the host form
extern "C" int fibd_fixel_fit(const int32_t *ids, const int32_t *npts, int64_t nlines, int64_t npoints, const uint64_t *aq, int64_t nfixels, int niter,
                              uint32_t *q, float *weights, float *td, double *cost, void *state, uint64_t *tdq, uint64_t *nline, void *work,
                              size_t work_bytes, void *stream) try {
    FIB_RC(fx_check_lines(ids, npts, nlines, npoints));
    FIB_CHECK(niter >= 0, FIB_ERR_INVALID, "niter must not be negative");
    FIB_CHECK(nfixels > 0 && nfixels < ((int64_t)1 << 31), FIB_ERR_INVALID, "nfixels must be between 1 and 2^31 - 1");
    FIB_CHECK(aq && td && cost && state && tdq && (nlines == 0 || (q && weights && nline)), FIB_ERR_INVALID, "NULL argument");
    const size_t scan_bytes = fx_align(tm_work_bytes(nlines));
    FIB_RC(ls_check_work(work, work_bytes, scan_bytes + sizeof(double) * FX_COST_GRID, "fibd_fixel_fit_work_size"));
    hipStream_t s = (hipStream_t)stream;
    fib::ProfScope prof("fixel_fit", s);
    FxState *st = reinterpret_cast<FxState *>(state);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<char *>(work) + scan_bytes);
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, nullptr, s, w));
    const size_t td_bytes = sizeof(uint64_t) * (size_t)nfixels;
    FIB_HIP(hipMemsetAsync(tdq, 0, td_bytes, s));
    fx_td_launch(ids, npts, w, nlines, q, nfixels, tdq, s);
    FIB_HIP(hipMemsetAsync(&st->sum_td0, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(fx_sum_td, dim3(fx_grid(nfixels, TM_BLOCK, 4096)), dim3(TM_BLOCK), 0, s, tdq, nfixels, st);
    hipLaunchKernelGGL(fx_mu, dim3(1), dim3(1), 0, s, st);
    fx_cost_launch(aq, tdq, nfixels, st, partial, cost, s);
    for (int it = 0; it < niter; it++) {
        fx_update_launch(ids, npts, w, nlines, aq, tdq, nfixels, it == 0, st, nline, q, s);
        FIB_HIP(hipMemsetAsync(tdq, 0, td_bytes, s));
        fx_td_launch(ids, npts, w, nlines, q, nfixels, tdq, s);
        fx_cost_launch(aq, tdq, nfixels, st, partial, cost + it + 1, s);
    }
    FIB_HIP(hipGetLastError());
    return fibd_fixel_output(q, nlines, tdq, nfixels, state, weights, td, stream);
} FIB_API_CATCH

extern "C" int fibd_fixel_fit_work_size(int64_t nlines, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    *bytes = fx_align(tm_work_bytes(nlines)) + sizeof(double) * FX_COST_GRID;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_weights(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, int32_t nvec,
                                const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2, int niter,
                                const uint32_t *q0, uint32_t *q, float *weights, float *td, double *cost, void *state, void *work, size_t work_bytes,
                                void *stream) try {
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nvec >= 1 && nvec <= 3, FIB_ERR_INVALID, "nvec must be 1, 2 or 3, not %d", nvec);
    FIB_CHECK(nlines >= 0 && npoints >= 0 && niter >= 0, FIB_ERR_INVALID, "nlines, npoints and niter must not be negative");
    const int64_t nvox = (int64_t)nx * ny * nz, nfix = nvox * nvec;
    const FxWork lay(nlines, npoints, nfix);
    FIB_RC(ls_check_work(work, work_bytes, lay.total, "fibd_str_weights_work_size"));
    FIB_CHECK(state && td && cost && (nlines == 0 || (q && weights)), FIB_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    char *base = reinterpret_cast<char *>(work);
    uint64_t *aq = reinterpret_cast<uint64_t *>(base + lay.aq), *tdq = reinterpret_cast<uint64_t *>(base + lay.tdq);
    uint64_t *nline = reinterpret_cast<uint64_t *>(base + lay.nline);
    int32_t *ids = reinterpret_cast<int32_t *>(base + lay.ids);
    FxState *st = reinterpret_cast<FxState *>(state);
    FIB_RC(fibd_fixel_quantise(nvec, nvox, ovec, f, mask, f_thresh, aq, state, stream));
    FIB_RC(fibd_fixel_assign(xyz, npts, nlines, npoints, nx, ny, nz, nvec, ovec, f, mask, f_thresh, cos2, ids, &st->n_unassigned, work, lay.partial, stream));
    if (nlines) {
        if (q0) FIB_HIP(hipMemcpyAsync(q, q0, sizeof(uint32_t) * (size_t)nlines, hipMemcpyDeviceToDevice, s));
        else hipLaunchKernelGGL(fx_fill, dim3((unsigned)fib::cdiv(nlines, TM_BLOCK)), dim3(TM_BLOCK), 0, s, q, nlines, FX_Q_ONE);
    }
    return fibd_fixel_fit(ids, npts, nlines, npoints, aq, nfix, niter, q, weights, td, cost, state, tdq, nline, work, lay.aq, stream);
} FIB_API_CATCH
