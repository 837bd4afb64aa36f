// nlreg.hip — non-linear registration on gfx950 ("Non-linear registration", include/fibers_hip.h): a single-contrast, multi-resolution,
// additive demons estimator of the displacement field that warp.hip applies, and the Jacobian map that checks it.  Not in the
// reference.  tests/nlreg_ref.py restates every definition in NumPy and the kernels are held to that bit for bit: the field sample is
// warp.hip's (warp_sample.inc), the pull-back and the trilinear value are volxform.hip's (xfm_apply.inc, vol_sample.inc), the pyramid and
// the ranges are register.hip's (fibd_vol_halve, fibd_vol_range).
//
// Every kernel has one thread per voxel of the field's grid on vx_kernel's tile (four neighbouring x-row segments, a wave each) and no
// kernel waits for another workgroup.  nl_step_kernel: the moving sample through the current field, the fixed gradient, the force, the
// updated field, and the workgroup's {sum of diff^2, count} into its own slot of the workspace; nl_cost_kernel adds the slots in a fixed
// order.  nl_smooth_kernel<AXIS>: one pass of the separable Gaussian; three launches make fibd_warp_smooth.  The field is the packed
// float4 form: a 16-byte load or store per lane and voxel.
#include "common.h"

#include <algorithm>
#include <cmath>

// the sample, the gradient, the force, the taps' sum and the determinant are sequences of separately rounded float32 operations
#pragma clang fp contract(off)

namespace {

#include "xfm_apply.inc"
#include "vol_sample.inc"
#include "warp_sample.inc"

constexpr int NL_MAX_DIM = 1 << 24;                            // every size is exact in float32
constexpr int NL_T = 256, NL_BX = 64, NL_BY = 4;               // a workgroup: 64 x 4 voxels of a plane
constexpr int NL_MAX_RADIUS = 12;                              // ceil(3 sigma) at the largest sigma, 4
constexpr int NL_MAX_LEVELS = 4;

struct NlCost { double ssd; uint64_t count; };                 // what a step leaves: the sum of diff^2 and the voxels it ran over
struct NlMat3 { float m[9]; };
struct NlTaps { float w[2 * NL_MAX_RADIUS + 1]; int r; };
struct NlNorm { float lo_f, s_f, lo_m, s_m; };                 // n(v) = (v - lo) * s of the fixed and of the moving level volume
static_assert(sizeof(NlCost) == 16, "the cost slots are 16 bytes apart");

__device__ __forceinline__ bool nl_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float nl_norm(float v, float lo, float s) { return (v - lo) * s; }

// the difference rule along an axis of size n at index i, from the values at i - 1, i and i + 1 (each read at its clamped index):
// central in the interior, one-sided on the two faces, 0 on an axis of size 1
__device__ __forceinline__ float nl_dif(float a, float b, float c, int i, int n) {
    return n == 1 ? 0.f : (i == 0 ? c - b : (i == n - 1 ? b - a : (c - a) * 0.5f));
}

// the voxel of a thread on the flat grid over (x segment, y tile, z)
__device__ __forceinline__ bool nl_voxel(int nx, int ny, unsigned nsx, unsigned nsy, int &i, int &j, int &k) {
    const unsigned b = blockIdx.x, bx = b % nsx, r = b / nsx, by = r % nsy;
    k = (int)(r / nsy);
    i = (int)(bx * NL_BX) + (int)(threadIdx.x % NL_BX);
    j = (int)(by * NL_BY) + (int)(threadIdx.x / NL_BX);
    return i < nx && j < ny;
}

// ---- one demons iteration -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NL_T) void nl_step_kernel(const float *__restrict__ fixed, int nx, int ny, int nz, const float *__restrict__ moving,
                                                       int nxm, int nym, int nzm, const NlNorm N, const XfmMat to_ras, const XfmMat from_ras,
                                                       const NlMat3 T, float kappa, const float4 *__restrict__ din, float4 *__restrict__ dout,
                                                       NlCost *__restrict__ partial, unsigned nsx, unsigned nsy) {
    __shared__ double s_ssd[NL_T / 64];
    __shared__ unsigned s_cnt[NL_T / 64];
    int i, j, k;
    double ssd = 0.0;
    bool counted = false;
    if (nl_voxel(nx, ny, nsx, nsy, i, j, k)) {
        const int64_t sy = nx, sz = (int64_t)nx * ny, o = (int64_t)i + sy * j + sz * k;
        const WarpField W{din, nx, ny, nz};
        const float4 d = din[o];
        float ux = 0.f, uy = 0.f, uz = 0.f;
        // the moving sample: fibd_warp_volume's position with to_field the identity (q is the voxel itself)
        const float3 x = xfm_point(to_ras, (float)i, (float)j, (float)k);
        const float3 s = wp_sample(W, make_float3((float)i, (float)j, (float)k));
        const float3 p = xfm_point(from_ras, x.x + s.x, x.y + s.y, x.z + s.z);
        if (vx_inside(p, nxm, nym, nzm)) {
            const float m = nl_norm(vx_cell_value(vx_cell(p, nxm, nym, nzm), moving), N.lo_m, N.s_m);
            const float *F = fixed + o;
            const float f = nl_norm(F[0], N.lo_f, N.s_f);
            const float fxa = nl_norm(F[i > 0 ? -1 : 0], N.lo_f, N.s_f), fxc = nl_norm(F[i < nx - 1 ? 1 : 0], N.lo_f, N.s_f);
            const float fya = nl_norm(F[j > 0 ? -sy : 0], N.lo_f, N.s_f), fyc = nl_norm(F[j < ny - 1 ? sy : 0], N.lo_f, N.s_f);
            const float fza = nl_norm(F[k > 0 ? -sz : 0], N.lo_f, N.s_f), fzc = nl_norm(F[k < nz - 1 ? sz : 0], N.lo_f, N.s_f);
            const float v0 = nl_dif(fxa, f, fxc, i, nx), v1 = nl_dif(fya, f, fyc, j, ny), v2 = nl_dif(fza, f, fzc, k, nz);
            const float g0 = (T.m[0] * v0 + T.m[1] * v1) + T.m[2] * v2;
            const float g1 = (T.m[3] * v0 + T.m[4] * v1) + T.m[5] * v2;
            const float g2 = (T.m[6] * v0 + T.m[7] * v1) + T.m[8] * v2;
            const float diff = f - m;
            const float sq = diff * diff;
            const float den = ((g0 * g0 + g1 * g1) + g2 * g2) + sq * kappa;
            if (nl_finite(f) && nl_finite(m) && nl_finite(g0) && nl_finite(g1) && nl_finite(g2) && nl_finite(den) && den != 0.f) {
                const float q = diff / den;
                ux = q * g0; uy = q * g1; uz = q * g2;
                ssd = (double)sq;
                counted = true;
            }
        }
        dout[o] = make_float4(d.x + ux, d.y + uy, d.z + uz, 0.f);
    }
    // the workgroup's partial: lanes in a fixed tree, then the four waves in their order
    const unsigned cnt = (unsigned)__popcll(__ballot(counted));
    for (int off = 32; off > 0; off >>= 1) ssd = ssd + __shfl_down(ssd, off, 64);
    if (threadIdx.x % 64 == 0) { s_ssd[threadIdx.x / 64] = ssd; s_cnt[threadIdx.x / 64] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        NlCost c;
        c.ssd = ((s_ssd[0] + s_ssd[1]) + s_ssd[2]) + s_ssd[3];
        c.count = (uint64_t)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        partial[blockIdx.x] = c;
    }
}
static_assert(NL_T == 256 && NL_BX * NL_BY == NL_T, "the partial adds four waves");

// the sum of the workgroups' partials, by one workgroup in a fixed order (so a run gives the same bits every time)
__global__ __launch_bounds__(NL_T) void nl_cost_kernel(const NlCost *__restrict__ partial, int64_t n, NlCost *__restrict__ out) {
    __shared__ double s_ssd[NL_T];
    __shared__ unsigned long long s_cnt[NL_T];
    double ssd = 0.0;
    unsigned long long cnt = 0;
    for (int64_t b = threadIdx.x; b < n; b += NL_T) { ssd = ssd + partial[b].ssd; cnt += partial[b].count; }
    s_ssd[threadIdx.x] = ssd; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = NL_T / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { s_ssd[threadIdx.x] = s_ssd[threadIdx.x] + s_ssd[threadIdx.x + h]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out->ssd = s_ssd[0]; out->count = s_cnt[0]; }
}

// ---- regularisation: one pass of the separable Gaussian along AXIS --------------------------------------------------------------------
template <int AXIS>
__global__ __launch_bounds__(NL_T) void nl_smooth_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, int nx, int ny, int nz,
                                                         const NlTaps K, unsigned nsx, unsigned nsy) {
    int i, j, k;
    if (!nl_voxel(nx, ny, nsx, nsy, i, j, k)) return;
    const int64_t o = (int64_t)i + (int64_t)nx * ((int64_t)j + (int64_t)ny * k);
    const int n = AXIS == 0 ? nx : (AXIS == 1 ? ny : nz), c = AXIS == 0 ? i : (AXIS == 1 ? j : k);
    const int64_t stride = AXIS == 0 ? 1 : (AXIS == 1 ? (int64_t)nx : (int64_t)nx * ny);
    const float4 *row = in + (o - stride * c);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int t = -K.r; t <= K.r; t++) {
        const int e = min(max(c + t, 0), n - 1);                   // the edge value continues beyond the grid
        const float4 v = row[stride * e];
        const float w = K.w[t + K.r];
        ax = ax + w * v.x; ay = ay + w * v.y; az = az + w * v.z;
    }
    out[o] = make_float4(ax, ay, az, 0.f);
}

// ---- between levels: fine voxel y takes S(0.5 y - 0.25) of the coarse field ----------------------------------------------------------
__global__ __launch_bounds__(NL_T) void nl_upsample_kernel(const WarpField C, float4 *__restrict__ out, int nx, int ny, int nz, unsigned nsx,
                                                           unsigned nsy) {
    int i, j, k;
    if (!nl_voxel(nx, ny, nsx, nsy, i, j, k)) return;
    const float3 s = wp_sample(C, make_float3(0.5f * (float)i - 0.25f, 0.5f * (float)j - 0.25f, 0.5f * (float)k - 0.25f));
    out[(int64_t)i + (int64_t)nx * ((int64_t)j + (int64_t)ny * k)] = make_float4(s.x, s.y, s.z, 0.f);
}

__global__ __launch_bounds__(NL_T) void nl_unpack_kernel(const float4 *__restrict__ packed, int64_t nvox, float *__restrict__ disp) {
    const int64_t v = (int64_t)blockIdx.x * NL_T + threadIdx.x;
    if (v >= nvox) return;
    const float4 d = packed[v];
    disp[v] = d.x; disp[nvox + v] = d.y; disp[2 * nvox + v] = d.z;
}

// ---- the Jacobian map: det(I + dd/dx) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NL_T) void nl_jacobian_kernel(const float4 *__restrict__ d, int nx, int ny, int nz, const NlMat3 Li,
                                                           float *__restrict__ out, unsigned nsx, unsigned nsy) {
    int i, j, k;
    if (!nl_voxel(nx, ny, nsx, nsy, i, j, k)) return;
    const int64_t sy = nx, sz = (int64_t)nx * ny, o = (int64_t)i + sy * j + sz * k;
    const float4 b = d[o];
    const float4 xa = d[o + (i > 0 ? -1 : 0)], xc = d[o + (i < nx - 1 ? 1 : 0)];
    const float4 ya = d[o + (j > 0 ? -sy : 0)], yc = d[o + (j < ny - 1 ? sy : 0)];
    const float4 za = d[o + (k > 0 ? -sz : 0)], zc = d[o + (k < nz - 1 ? sz : 0)];
    // D[c][k] = dd_c / dvox_k, then G[c][r] = sum_k D[c][k] Linv[k][r] in k order
    const float D[3][3] = {{nl_dif(xa.x, b.x, xc.x, i, nx), nl_dif(ya.x, b.x, yc.x, j, ny), nl_dif(za.x, b.x, zc.x, k, nz)},
                           {nl_dif(xa.y, b.y, xc.y, i, nx), nl_dif(ya.y, b.y, yc.y, j, ny), nl_dif(za.y, b.y, zc.y, k, nz)},
                           {nl_dif(xa.z, b.z, xc.z, i, nx), nl_dif(ya.z, b.z, yc.z, j, ny), nl_dif(za.z, b.z, zc.z, k, nz)}};
    float J[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float g = (D[c][0] * Li.m[r] + D[c][1] * Li.m[3 + r]) + D[c][2] * Li.m[6 + r];
            J[c][r] = c == r ? 1.f + g : g;
        }
    const float m0 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const float m1 = J[1][0] * J[2][2] - J[1][2] * J[2][0];
    const float m2 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    out[o] = (J[0][0] * m0 - J[0][1] * m1) + J[0][2] * m2;
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------
bool nl_apart(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x + na <= y || y + nb <= x;
}
bool nl_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int nl_field_check(const void *packed, int nx, int ny, int nz) {
    FIB_CHECK(packed, FIB_ERR_INVALID, "NULL field");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    FIB_CHECK(std::max({nx, ny, nz}) <= NL_MAX_DIM, FIB_ERR_UNSUPPORTED, "a field dimension above 2^24");
    FIB_CHECK(nl_aligned(packed, 16), FIB_ERR_INVALID, "the packed field must be 16-byte aligned");
    return FIB_OK;
}

// the flat grid over (x segment, y tile, z) of a field
int nl_grid(int nx, int ny, int nz, unsigned &nsx, unsigned &nsy, int64_t &nblocks) {
    nsx = (unsigned)fib::cdiv(nx, NL_BX); nsy = (unsigned)fib::cdiv(ny, NL_BY);
    nblocks = (int64_t)nsx * nsy * nz;
    FIB_CHECK(nblocks < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the field needs 2^31 workgroups or more");
    return FIB_OK;
}

int nl_sigma_check(float sigma) {
    FIB_CHECK(sigma >= 0.f && sigma <= 4.f, FIB_ERR_INVALID, "sigma %g outside [0, 4]", (double)sigma);      // (a NaN fails)
    return FIB_OK;
}

XfmMat nl_mat(const float m[16]) {
    XfmMat X;
    memcpy(X.m, m, sizeof X.m);
    return X;
}
NlMat3 nl_mat3(const float m[9]) {
    NlMat3 X;
    memcpy(X.m, m, sizeof X.m);
    return X;
}

int nl_taps(float sigma, NlTaps &K) {
    memset(&K, 0, sizeof K);
    FIB_RC(fib::host_gauss_taps(sigma, NL_MAX_RADIUS, &K.r, K.w));
    return FIB_OK;
}

// the three passes on checked arguments: x: in -> out, y: out -> tmp, z: tmp -> out
int nl_smooth(const float4 *in, int nx, int ny, int nz, const NlTaps &K, float4 *out, float4 *tmp, hipStream_t st) {
    unsigned nsx, nsy;
    int64_t nb;
    FIB_RC(nl_grid(nx, ny, nz, nsx, nsy, nb));
    hipLaunchKernelGGL(nl_smooth_kernel<0>, dim3((unsigned)nb), dim3(NL_T), 0, st, in, out, nx, ny, nz, K, nsx, nsy);
    hipLaunchKernelGGL(nl_smooth_kernel<1>, dim3((unsigned)nb), dim3(NL_T), 0, st, static_cast<const float4 *>(out), tmp, nx, ny, nz, K, nsx, nsy);
    hipLaunchKernelGGL(nl_smooth_kernel<2>, dim3((unsigned)nb), dim3(NL_T), 0, st, static_cast<const float4 *>(tmp), out, nx, ny, nz, K, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

}  // namespace

extern "C" int fibd_nlreg_step_work_size(int nx, int ny, int nz, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    FIB_CHECK(std::max({nx, ny, nz}) <= NL_MAX_DIM, FIB_ERR_UNSUPPORTED, "a field dimension above 2^24");
    unsigned nsx, nsy;
    int64_t nb;
    FIB_RC(nl_grid(nx, ny, nz, nsx, nsy, nb));
    *bytes = sizeof(NlCost) * (size_t)nb;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_nlreg_step(const float *fixed, int nxf, int nyf, int nzf, const float *moving, int nxm, int nym, int nzm, const float norm[4],
                               const float to_ras[16], const float from_ras[16], const float T[9], float kappa, const void *packed, void *out,
                               void *cost, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(fixed && moving && norm && to_ras && from_ras && T && out && cost && work, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(nl_field_check(packed, nxf, nyf, nzf));
    FIB_CHECK(nxm > 0 && nym > 0 && nzm > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(std::max({nxm, nym, nzm}) <= NL_MAX_DIM, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    FIB_CHECK(nl_aligned(out, 16), FIB_ERR_INVALID, "the packed field must be 16-byte aligned");
    FIB_CHECK(nl_aligned(fixed, 4) && nl_aligned(moving, 4), FIB_ERR_INVALID, "volumes must be 4-byte aligned");
    FIB_CHECK(nl_aligned(cost, 8) && nl_aligned(work, 8), FIB_ERR_INVALID, "cost and work must be 8-byte aligned");
    size_t need = 0;
    FIB_RC(fibd_nlreg_step_work_size(nxf, nyf, nzf, &need));
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "workspace of %zu bytes, fibd_nlreg_step_work_size asks for %zu", work_bytes, need);
    const uint64_t nvf = (uint64_t)nxf * nyf * nzf, bf = 4 * nvf, bm = 4ull * (uint64_t)nxm * nym * nzm, bp = 16 * nvf;
    // a gather: every output word may be another thread's input, and the partials are written while the volumes are read
    FIB_CHECK(nl_apart(out, bp, packed, bp) && nl_apart(out, bp, fixed, bf) && nl_apart(out, bp, moving, bm) && nl_apart(out, bp, work, need) &&
              nl_apart(out, bp, cost, 16) && nl_apart(work, need, packed, bp) && nl_apart(work, need, fixed, bf) && nl_apart(work, need, moving, bm) &&
              nl_apart(work, need, cost, 16) && nl_apart(cost, 16, packed, bp) && nl_apart(cost, 16, fixed, bf) && nl_apart(cost, 16, moving, bm),
              FIB_ERR_INVALID, "out, cost and work must not overlap the field, the volumes or each other");
    unsigned nsx, nsy;
    int64_t nb;
    FIB_RC(nl_grid(nxf, nyf, nzf, nsx, nsy, nb));
    hipStream_t st = (hipStream_t)stream;
    const NlNorm N{norm[0], norm[1], norm[2], norm[3]};
    fib::ProfScope prof("nlreg_step", st);
    hipLaunchKernelGGL(nl_step_kernel, dim3((unsigned)nb), dim3(NL_T), 0, st, fixed, nxf, nyf, nzf, moving, nxm, nym, nzm, N, nl_mat(to_ras),
                       nl_mat(from_ras), nl_mat3(T), kappa, static_cast<const float4 *>(packed), static_cast<float4 *>(out),
                       static_cast<NlCost *>(work), nsx, nsy);
    hipLaunchKernelGGL(nl_cost_kernel, dim3(1), dim3(NL_T), 0, st, static_cast<const NlCost *>(work), nb, static_cast<NlCost *>(cost));
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_smooth(const void *packed, int nx, int ny, int nz, float sigma, void *out, void *work, size_t work_bytes, void *stream) try {
    FIB_RC(nl_field_check(packed, nx, ny, nz));
    FIB_CHECK(out && work, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(nl_sigma_check(sigma));
    FIB_CHECK(nl_aligned(out, 16) && nl_aligned(work, 16), FIB_ERR_INVALID, "the packed fields and the workspace must be 16-byte aligned");
    const uint64_t bp = 16ull * (uint64_t)nx * ny * nz;
    FIB_CHECK(work_bytes >= bp, FIB_ERR_INVALID, "workspace of %zu bytes, a packed field of %llu bytes is needed", work_bytes, (unsigned long long)bp);
    FIB_CHECK(nl_apart(out, bp, packed, bp) && nl_apart(work, bp, packed, bp) && nl_apart(out, bp, work, bp), FIB_ERR_INVALID,
              "the field, out and work must not overlap");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("warp_smooth", st);
    if (sigma == 0.f) {                                         // no smoothing: the field as it is
        FIB_HIP(hipMemcpyAsync(out, packed, bp, hipMemcpyDeviceToDevice, st));
        return FIB_OK;
    }
    NlTaps K;
    FIB_RC(nl_taps(sigma, K));
    return nl_smooth(static_cast<const float4 *>(packed), nx, ny, nz, K, static_cast<float4 *>(out), static_cast<float4 *>(work), st);
} FIB_API_CATCH

extern "C" int fibd_warp_upsample(const void *coarse, int cx, int cy, int cz, void *out, int nx, int ny, int nz, void *stream) try {
    FIB_RC(nl_field_check(coarse, cx, cy, cz));
    FIB_RC(nl_field_check(out, nx, ny, nz));
    FIB_CHECK(nl_apart(coarse, 16ull * (uint64_t)cx * cy * cz, out, 16ull * (uint64_t)nx * ny * nz), FIB_ERR_INVALID, "the coarse field and out must not overlap");
    unsigned nsx, nsy;
    int64_t nb;
    FIB_RC(nl_grid(nx, ny, nz, nsx, nsy, nb));
    const WarpField C{static_cast<const float4 *>(coarse), cx, cy, cz};
    fib::ProfScope prof("warp_upsample", (hipStream_t)stream);
    hipLaunchKernelGGL(nl_upsample_kernel, dim3((unsigned)nb), dim3(NL_T), 0, (hipStream_t)stream, C, static_cast<float4 *>(out), nx, ny, nz, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_unpack(const void *packed, int nx, int ny, int nz, float *disp, void *stream) try {
    FIB_RC(nl_field_check(packed, nx, ny, nz));
    FIB_CHECK(disp, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nl_aligned(disp, 4), FIB_ERR_INVALID, "the field must be 4-byte aligned");
    const int64_t nvox = (int64_t)nx * ny * nz;
    FIB_CHECK(nl_apart(disp, 12ull * (uint64_t)nvox, packed, 16ull * (uint64_t)nvox), FIB_ERR_INVALID, "disp and packed must not overlap");
    FIB_CHECK(fib::cdiv(nvox, NL_T) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the field needs 2^31 workgroups or more");
    fib::ProfScope prof("warp_unpack", (hipStream_t)stream);
    hipLaunchKernelGGL(nl_unpack_kernel, dim3((unsigned)fib::cdiv(nvox, NL_T)), dim3(NL_T), 0, (hipStream_t)stream, static_cast<const float4 *>(packed),
                       nvox, disp);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_jacobian(const void *packed, int nx, int ny, int nz, const float linv[9], float *out, void *stream) try {
    FIB_RC(nl_field_check(packed, nx, ny, nz));
    FIB_CHECK(linv && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nl_aligned(out, 4), FIB_ERR_INVALID, "out must be 4-byte aligned");
    const uint64_t nvox = (uint64_t)nx * ny * nz;
    FIB_CHECK(nl_apart(out, 4 * nvox, packed, 16 * nvox), FIB_ERR_INVALID, "out must not overlap the field");
    unsigned nsx, nsy;
    int64_t nb;
    FIB_RC(nl_grid(nx, ny, nz, nsx, nsy, nb));
    fib::ProfScope prof("warp_jacobian", (hipStream_t)stream);
    hipLaunchKernelGGL(nl_jacobian_kernel, dim3((unsigned)nb), dim3(NL_T), 0, (hipStream_t)stream, static_cast<const float4 *>(packed), nx, ny, nz,
                       nl_mat3(linv), out, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

// ---- the whole pyramid on device-resident volumes -------------------------------------------------------------------------------------
namespace {

// the workspace of fibd_nlreg_run: pyramid levels 1 .. levels - 1 of both volumes, a range per level and volume, three packed fields of
// the level-0 size (the current field, the stepped one, the smoothing's middle pass), the workgroups' partials and the costs of a level
struct NlLayout {
    int fs[NL_MAX_LEVELS][3], ms[NL_MAX_LEVELS][3], maxit = 0;
    size_t fixed[NL_MAX_LEVELS], moving[NL_MAX_LEVELS], rf[NL_MAX_LEVELS], rm[NL_MAX_LEVELS], field[3], partial, cost, total;
    NlLayout(const int32_t *fsize, const int32_t *msize, int levels, const int32_t *niter) {
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
        for (int l = 0; l < levels; l++) {
            for (int c = 0; c < 3; c++) { fs[l][c] = l ? (fs[l - 1][c] + 1) / 2 : fsize[c]; ms[l][c] = l ? (ms[l - 1][c] + 1) / 2 : msize[c]; }
            fixed[l] = l ? take(4 * fvox(l)) : 0;
            moving[l] = l ? take(4 * mvox(l)) : 0;
            rf[l] = take(16);
            rm[l] = take(16);
            maxit = std::max(maxit, (int)niter[l]);
        }
        for (int b = 0; b < 3; b++) field[b] = take(16 * fvox(0));
        partial = take(sizeof(NlCost) * (size_t)(fib::cdiv(fs[0][0], NL_BX) * fib::cdiv(fs[0][1], NL_BY) * fs[0][2]));
        cost = take(sizeof(NlCost) * (size_t)std::max(maxit, 1));
        total = at;
    }
    size_t fvox(int l) const { return (size_t)fs[l][0] * fs[l][1] * fs[l][2]; }
    size_t mvox(int l) const { return (size_t)ms[l][0] * ms[l][1] * ms[l][2]; }
};

int nl_run_checks(const int32_t *fsize, const int32_t *msize, int levels, const int32_t *niter) {
    FIB_CHECK(fsize && msize && niter, FIB_ERR_INVALID, "NULL argument");
    for (int c = 0; c < 3; c++) FIB_CHECK(fsize[c] > 0 && msize[c] > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    for (int c = 0; c < 3; c++) FIB_CHECK(fsize[c] <= NL_MAX_DIM && msize[c] <= NL_MAX_DIM, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    FIB_CHECK(levels >= 1 && levels <= NL_MAX_LEVELS, FIB_ERR_INVALID, "levels must lie in 1 .. %d, not %d", NL_MAX_LEVELS, levels);
    for (int l = 0; l < levels; l++) FIB_CHECK(niter[l] >= 0, FIB_ERR_INVALID, "niter must not be negative");
    unsigned nsx, nsy;
    int64_t nb;
    return nl_grid(fsize[0], fsize[1], fsize[2], nsx, nsy, nb);
}

struct RegRange { float lo, hi, scale; uint32_t nfinite; };     // what fibd_vol_range leaves (register.hip)

}  // namespace

extern "C" int fibd_nlreg_work_size(const int32_t fixed_size[3], const int32_t moving_size[3], int levels, const int32_t *niter, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(nl_run_checks(fixed_size, moving_size, levels, niter));
    *bytes = NlLayout(fixed_size, moving_size, levels, niter).total;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_nlreg_run(const float *fixed, const int32_t fixed_size[3], const float fixed_vox2ras[16], const float *moving,
                              const int32_t moving_size[3], const float moving_vox2ras[16], const float *post, int levels, const int32_t *niter,
                              float sigma, float step, void *field, double *cost, int64_t *count, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(fixed && fixed_vox2ras && moving && moving_vox2ras && field && work, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(nl_run_checks(fixed_size, moving_size, levels, niter));
    FIB_RC(nl_sigma_check(sigma));
    const NlLayout lay(fixed_size, moving_size, levels, niter);
    FIB_CHECK(work_bytes >= lay.total && nl_aligned(work, 16), FIB_ERR_INVALID,
              "a 16-byte aligned workspace of fibd_nlreg_work_size = %zu bytes is needed, not %zu", lay.total, work_bytes);
    FIB_CHECK(nl_aligned(field, 16), FIB_ERR_INVALID, "the packed field must be 16-byte aligned");
    FIB_CHECK(nl_aligned(fixed, 4) && nl_aligned(moving, 4), FIB_ERR_INVALID, "volumes must be 4-byte aligned");
    const uint64_t bf = 4ull * lay.fvox(0), bm = 4ull * lay.mvox(0), bp = 16ull * lay.fvox(0);
    FIB_CHECK(nl_apart(work, lay.total, fixed, bf) && nl_apart(work, lay.total, moving, bm) && nl_apart(work, lay.total, field, bp) &&
              nl_apart(field, bp, fixed, bf) && nl_apart(field, bp, moving, bm), FIB_ERR_INVALID,
              "the field and work must not overlap the volumes or each other");
    // the matrices of every level (host, float64, rounded once); the refusals of step and of singular matrices come before any launch
    struct Level { float to_ras[16], from_ras[16], T[9], kappa; } lv[NL_MAX_LEVELS];
    for (int l = 0; l < levels; l++) FIB_RC(fib_nlreg_level(fixed_vox2ras, moving_vox2ras, post, l, step, lv[l].to_ras, lv[l].from_ras, lv[l].T, &lv[l].kappa));
    NlTaps K;
    FIB_RC(nl_taps(sigma, K));
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(work);
    auto fx = [&](int l) { return l ? reinterpret_cast<const float *>(w + lay.fixed[l]) : fixed; };
    auto mv = [&](int l) { return l ? reinterpret_cast<const float *>(w + lay.moving[l]) : moving; };
    // the pyramids and the ranges; the ranges come back once: a level volume without two distinct finite values is refused
    for (int l = 0; l < levels; l++) {
        if (l) {
            FIB_RC(fibd_vol_halve(fx(l - 1), lay.fs[l - 1][0], lay.fs[l - 1][1], lay.fs[l - 1][2], 1, reinterpret_cast<float *>(w + lay.fixed[l]), st));
            FIB_RC(fibd_vol_halve(mv(l - 1), lay.ms[l - 1][0], lay.ms[l - 1][1], lay.ms[l - 1][2], 1, reinterpret_cast<float *>(w + lay.moving[l]), st));
        }
        FIB_RC(fibd_vol_range(fx(l), (int64_t)lay.fvox(l), 1, FIB_REG_MIN_BINS, w + lay.rf[l], st));
        FIB_RC(fibd_vol_range(mv(l), (int64_t)lay.mvox(l), 1, FIB_REG_MIN_BINS, w + lay.rm[l], st));
    }
    RegRange rng[NL_MAX_LEVELS][2];
    for (int l = 0; l < levels; l++) {
        FIB_HIP(hipMemcpyAsync(&rng[l][0], w + lay.rf[l], 16, hipMemcpyDeviceToHost, st));
        FIB_HIP(hipMemcpyAsync(&rng[l][1], w + lay.rm[l], 16, hipMemcpyDeviceToHost, st));
    }
    FIB_HIP(hipStreamSynchronize(st));
    float norm[NL_MAX_LEVELS][4];
    for (int l = 0; l < levels; l++)
        for (int v = 0; v < 2; v++) {
            const RegRange &r = rng[l][v];
            FIB_CHECK(r.nfinite > 0 && r.hi != r.lo, FIB_ERR_INVALID, "constant volume: the %s volume at level %d has no two distinct finite values",
                      v ? "moving" : "fixed", l);
            norm[l][2 * v] = r.lo;
            norm[l][2 * v + 1] = 1.f / (r.hi - r.lo);
        }
    const size_t width = (size_t)std::max(lay.maxit, 1);       // a row of cost and count; what no iteration fills stays NaN and 0
    if (cost) for (size_t e = 0; e < (size_t)levels * width; e++) cost[e] = std::nan("");
    if (count) for (size_t e = 0; e < (size_t)levels * width; e++) count[e] = 0;
    float4 *A = reinterpret_cast<float4 *>(w + lay.field[0]), *B = reinterpret_cast<float4 *>(w + lay.field[1]),
           *C = reinterpret_cast<float4 *>(w + lay.field[2]);
    NlCost *d_cost = reinterpret_cast<NlCost *>(w + lay.cost);
    std::vector<NlCost> h_cost(width);
    const size_t partial_bytes = lay.cost - lay.partial;
    for (int l = levels - 1, row = 0; l >= 0; l--, row++) {
        const int nx = lay.fs[l][0], ny = lay.fs[l][1], nz = lay.fs[l][2];
        if (l == levels - 1) {
            FIB_HIP(hipMemsetAsync(A, 0, 16 * lay.fvox(l), st));                       // the coarsest level starts from zero
        } else {
            FIB_RC(fibd_warp_upsample(A, lay.fs[l + 1][0], lay.fs[l + 1][1], lay.fs[l + 1][2], B, nx, ny, nz, st));
            std::swap(A, B);
        }
        const int n = niter[row];
        for (int it = 0; it < n; it++) {
            FIB_RC(fibd_nlreg_step(fx(l), nx, ny, nz, mv(l), lay.ms[l][0], lay.ms[l][1], lay.ms[l][2], norm[l], lv[l].to_ras, lv[l].from_ras, lv[l].T,
                                   lv[l].kappa, A, B, d_cost + it, w + lay.partial, partial_bytes, st));
            if (sigma > 0.f) {
                fib::ProfScope prof("warp_smooth", st);
                FIB_RC(nl_smooth(B, nx, ny, nz, K, A, C, st));
            } else {
                std::swap(A, B);
            }
        }
        if (n && (cost || count)) {                              // one wait per level, for its costs
            FIB_HIP(hipMemcpyAsync(h_cost.data(), d_cost, sizeof(NlCost) * (size_t)n, hipMemcpyDeviceToHost, st));
            FIB_HIP(hipStreamSynchronize(st));
            for (int it = 0; it < n; it++) {
                const size_t e = (size_t)row * width + it;
                if (cost) cost[e] = h_cost[it].count ? h_cost[it].ssd / (double)h_cost[it].count : std::nan("");
                if (count) count[e] = (int64_t)h_cost[it].count;
            }
        }
    }
    FIB_HIP(hipMemcpyAsync(field, A, bp, hipMemcpyDeviceToDevice, st));
    return FIB_OK;
} FIB_API_CATCH
