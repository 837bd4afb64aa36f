// warp.hip — non-linear warps on gfx950: a displacement field (mm, RAS) on a grid of its own applied to points (fibd_warp_points) and
// to volumes (fibd_warp_volume), and inverted by fixed-point iteration (fibd_warp_invert).  Not in the reference: the definitions are
// the "Non-linear warps" section of include/fibers_hip.h.  The non-linear sibling of xform.hip and volxform.hip: the matrices are
// applied by xfm_point (xfm_apply.inc), a warped volume is sampled by vx_sample (vol_sample.inc) and the field by wp_sample
// (warp_sample.inc, shared with nlreg.hip).
//
// The field's device form is float4 [nvox] = (dx, dy, dz, 0), made once by fibd_warp_pack (the tracer's precedent, stream.hip): the
// sample S(q) is 8 aligned 16-byte gathers instead of 24 scalar ones.  All three users are gather kernels with one thread per point or
// output voxel; the field is the large operand (182 x 218 x 182 packed: 115 MB) and lives in L2 / the Infinity Cache, so what bounds them
// is the gather rate, not arithmetic (profiles/warp/README.md).  Offsets are 64-bit; points and volumes may start at any 4-byte
// boundary (single-word loads and stores), the packed field at any 16-byte boundary.
#include "common.h"

#include <algorithm>

// the matrices, the sample and the iteration are sequences of separately rounded float32 operations: nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "xfm_apply.inc"
#include "vol_sample.inc"
#include "warp_sample.inc"

constexpr int WP_MAX_DIM = 1 << 24;                            // every size is exact in float32 (the clamp compares floats)
constexpr int WP_BLOCK = 256;

// the warp of a point of caller coordinates: to RAS and to field voxels, the sample, the sum, back to caller coordinates
__device__ __forceinline__ float3 wp_point(const WarpField &W, const XfmMat &to_ras, const XfmMat &to_field, const XfmMat &from_ras, float px,
                                           float py, float pz) {
    const float3 x = xfm_point(to_ras, px, py, pz);
    const float3 d = wp_sample(W, xfm_point(to_field, px, py, pz));
    return xfm_point(from_ras, x.x + d.x, x.y + d.y, x.z + d.z);
}

__global__ __launch_bounds__(WP_BLOCK) void wp_pack_kernel(const float *__restrict__ disp, int64_t nvox, float4 *__restrict__ packed) {
    const int64_t v = (int64_t)blockIdx.x * WP_BLOCK + threadIdx.x;
    if (v < nvox) packed[v] = make_float4(disp[v], disp[nvox + v], disp[2 * nvox + v], 0.f);
}

// (no __restrict__ on the points: out may be xyz itself; a thread reads its point before it writes it)
__global__ __launch_bounds__(WP_BLOCK) void wp_points_kernel(const WarpField W, const XfmMat to_ras, const XfmMat to_field, const XfmMat from_ras,
                                                             const float *xyz, float *out, int64_t npoints) {
    const int64_t p = (int64_t)blockIdx.x * WP_BLOCK + threadIdx.x;
    if (p >= npoints) return;
    const float3 r = wp_point(W, to_ras, to_field, from_ras, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]);
    out[3 * p] = r.x; out[3 * p + 1] = r.y; out[3 * p + 2] = r.z;
}

// the tile of vx_kernel<64, 4, .> (volxform.hip): four neighbouring x-row segments, a wave each
template <int BX, int BY, int UNROLL>
__global__ __launch_bounds__(BX * BY) void wp_volume_kernel(const WarpField W, const XfmMat to_ras, const XfmMat to_field, const XfmMat from_ras,
                                                            const uint32_t *__restrict__ vol, int nxi, int nyi, int nzi, int nframes, int interp,
                                                            uint32_t fill, uint32_t *__restrict__ out, int nxo, int nyo, int nzo, unsigned nsx,
                                                            unsigned nsy) {
    const unsigned b = blockIdx.x, bx = b % nsx, r = b / nsx, by = r % nsy, k = r / nsy;
    const int i = (int)(bx * BX) + (int)(threadIdx.x % BX), j = (int)(by * BY) + (int)(threadIdx.x / BX);
    if (i >= nxo || j >= nyo) return;
    const int64_t nvo = (int64_t)nxo * nyo * nzo;
    uint32_t *dst = out + ((int64_t)i + (int64_t)nxo * ((int64_t)j + (int64_t)nyo * k));
    vx_sample<UNROLL>(wp_point(W, to_ras, to_field, from_ras, (float)i, (float)j, (float)k), vol, nxi, nyi, nzi, nframes, interp, fill, dst, nvo);
}

__device__ __forceinline__ bool wp_same_bits(const float3 a, const float3 b) {
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) && __float_as_uint(a.z) == __float_as_uint(b.z);
}

// x <- y - S(x), niter times from x = y.  The loop is left when an iterate repeats bit for bit: every later one is the same.
template <int BX, int BY>
__global__ __launch_bounds__(BX * BY) void wp_invert_kernel(const WarpField W, const XfmMat out_to_ras, const XfmMat ras_to_field, int niter,
                                                            float *__restrict__ inv, float *__restrict__ err, int nxo, int nyo, int nzo, unsigned nsx,
                                                            unsigned nsy) {
    const unsigned b = blockIdx.x, bx = b % nsx, r = b / nsx, by = r % nsy, k = r / nsy;
    const int i = (int)(bx * BX) + (int)(threadIdx.x % BX), j = (int)(by * BY) + (int)(threadIdx.x / BX);
    if (i >= nxo || j >= nyo) return;
    const int64_t nvo = (int64_t)nxo * nyo * nzo, o = (int64_t)i + (int64_t)nxo * ((int64_t)j + (int64_t)nyo * k);
    const float3 y = xfm_point(out_to_ras, (float)i, (float)j, (float)k);
    float3 x = y;
    for (int it = 0; it < niter; it++) {
        const float3 d = wp_sample(W, xfm_point(ras_to_field, x.x, x.y, x.z));
        const float3 xn = make_float3(y.x - d.x, y.y - d.y, y.z - d.z);
        const bool same = wp_same_bits(xn, x);
        x = xn;
        if (same) break;
    }
    inv[o] = x.x - y.x; inv[nvo + o] = x.y - y.y; inv[2 * nvo + o] = x.z - y.z;
    if (err) {
        const float3 d = wp_sample(W, xfm_point(ras_to_field, x.x, x.y, x.z));
        const float rx = (x.x + d.x) - y.x, ry = (x.y + d.y) - y.y, rz = (x.z + d.z) - y.z;
        float e = fmaxf(fmaxf(fabsf(rx), fabsf(ry)), fabsf(rz));           // (fmaxf drops a NaN operand: it is put back)
        if (rx != rx || ry != ry || rz != rz) e = __builtin_nanf("");
        err[o] = e;
    }
}

int wp_field_check(const void *packed, int nx, int ny, int nz) {
    FIB_CHECK(packed, FIB_ERR_INVALID, "NULL field");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    FIB_CHECK(std::max({nx, ny, nz}) <= WP_MAX_DIM, FIB_ERR_UNSUPPORTED, "a field dimension above 2^24");
    FIB_CHECK((reinterpret_cast<uintptr_t>(packed) & 15) == 0, FIB_ERR_INVALID, "the packed field must be 16-byte aligned");
    return FIB_OK;
}

bool wp_disjoint(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa + na <= pb || pb + nb <= pa;
}

XfmMat wp_mat(const float m[16]) {
    XfmMat X;
    memcpy(X.m, m, sizeof X.m);
    return X;
}

}  // namespace

extern "C" int fibd_warp_pack(const float *disp, int nx, int ny, int nz, void *packed, void *stream) try {
    FIB_CHECK(disp, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(wp_field_check(packed, nx, ny, nz));
    FIB_CHECK((reinterpret_cast<uintptr_t>(disp) & 3) == 0, FIB_ERR_INVALID, "the field must be 4-byte aligned");
    const int64_t nvox = (int64_t)nx * ny * nz;
    FIB_CHECK(wp_disjoint(disp, 12ull * (uint64_t)nvox, packed, 16ull * (uint64_t)nvox), FIB_ERR_INVALID, "disp and packed must not overlap");
    FIB_CHECK(fib::cdiv(nvox, WP_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the field needs 2^31 workgroups or more");
    fib::ProfScope prof("warp_pack", (hipStream_t)stream);
    hipLaunchKernelGGL(wp_pack_kernel, dim3((unsigned)fib::cdiv(nvox, WP_BLOCK)), dim3(WP_BLOCK), 0, (hipStream_t)stream, disp, nvox,
                       static_cast<float4 *>(packed));
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_points(const void *packed, int nx, int ny, int nz, const float to_ras[16], const float to_field[16], const float from_ras[16],
                                const float *xyz, float *out, int64_t npoints, void *stream) try {
    FIB_RC(wp_field_check(packed, nx, ny, nz));
    FIB_CHECK(to_ras && to_field && from_ras, FIB_ERR_INVALID, "NULL matrix");
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    if (npoints == 0) return FIB_OK;
    FIB_CHECK(xyz && out, FIB_ERR_INVALID, "NULL argument");
    const uintptr_t ai = reinterpret_cast<uintptr_t>(xyz), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK((ai & 3) == 0 && (ao & 3) == 0, FIB_ERR_INVALID, "points must be 4-byte aligned");
    // in place or not at all: a partial overlap would let one thread's stores reach another thread's loads
    FIB_CHECK(ai == ao || wp_disjoint(xyz, 12ull * (uint64_t)npoints, out, 12ull * (uint64_t)npoints), FIB_ERR_INVALID,
              "xyz and out must be the same array or not overlap");
    FIB_CHECK(wp_disjoint(packed, 16ull * (uint64_t)nx * ny * nz, out, 12ull * (uint64_t)npoints), FIB_ERR_INVALID, "out must not overlap the field");
    FIB_CHECK(fib::cdiv(npoints, WP_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the points need 2^31 workgroups or more");
    const WarpField W{static_cast<const float4 *>(packed), nx, ny, nz};
    fib::ProfScope prof("warp_points", (hipStream_t)stream);
    hipLaunchKernelGGL(wp_points_kernel, dim3((unsigned)fib::cdiv(npoints, WP_BLOCK)), dim3(WP_BLOCK), 0, (hipStream_t)stream, W, wp_mat(to_ras),
                       wp_mat(to_field), wp_mat(from_ras), xyz, out, npoints);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_volume(const void *packed, int nx, int ny, int nz, const float to_ras[16], const float to_field[16], const float from_ras[16],
                                const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits, void *out, int nxo, int nyo,
                                int nzo, void *stream) try {
    FIB_RC(wp_field_check(packed, nx, ny, nz));
    FIB_CHECK(to_ras && to_field && from_ras && vol && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nxi > 0 && nyi > 0 && nzi > 0 && nxo > 0 && nyo > 0 && nzo > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(interp == FIB_VOL_NEAREST || interp == FIB_VOL_TRILINEAR, FIB_ERR_INVALID, "unknown interpolation %d", interp);
    FIB_CHECK(std::max({nxi, nyi, nzi, nxo, nyo, nzo}) <= WP_MAX_DIM, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    FIB_CHECK(((reinterpret_cast<uintptr_t>(vol) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, FIB_ERR_INVALID, "volumes must be 4-byte aligned");
    const uint64_t bi = 4ull * (uint64_t)nxi * nyi * nzi * nframes, bo = 4ull * (uint64_t)nxo * nyo * nzo * nframes;
    // a gather: any output word may be read as another thread's input, so there is no in-place form
    FIB_CHECK(wp_disjoint(vol, bi, out, bo), FIB_ERR_INVALID, "vol and out must not overlap");
    FIB_CHECK(wp_disjoint(packed, 16ull * (uint64_t)nx * ny * nz, out, bo), FIB_ERR_INVALID, "out must not overlap the field");
    constexpr int BX = 64, BY = 4;
    const unsigned nsx = (unsigned)fib::cdiv(nxo, BX), nsy = (unsigned)fib::cdiv(nyo, BY);
    FIB_CHECK(fib::cdiv(nxo, BX) * fib::cdiv(nyo, BY) * nzo < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the output volume needs 2^31 workgroups or more");
    const WarpField W{static_cast<const float4 *>(packed), nx, ny, nz};
    const dim3 grid(nsx * nsy * (unsigned)nzo), block(BX * BY);        // a flat grid over (x segment, y tile, z): no 65535 limit on ny or nz
    const uint32_t *src = static_cast<const uint32_t *>(vol);
    uint32_t *dst = static_cast<uint32_t *>(out);
    fib::ProfScope prof("warp_volume", (hipStream_t)stream);
    if (nframes >= 4)
        hipLaunchKernelGGL((wp_volume_kernel<BX, BY, 4>), grid, block, 0, (hipStream_t)stream, W, wp_mat(to_ras), wp_mat(to_field), wp_mat(from_ras), src,
                           nxi, nyi, nzi, nframes, interp, (uint32_t)outside_bits, dst, nxo, nyo, nzo, nsx, nsy);
    else
        hipLaunchKernelGGL((wp_volume_kernel<BX, BY, 1>), grid, block, 0, (hipStream_t)stream, W, wp_mat(to_ras), wp_mat(to_field), wp_mat(from_ras), src,
                           nxi, nyi, nzi, nframes, interp, (uint32_t)outside_bits, dst, nxo, nyo, nzo, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_warp_invert(const void *packed, int nx, int ny, int nz, const float out_to_ras[16], const float ras_to_field[16], int niter,
                                float *inv, float *err, int nxo, int nyo, int nzo, void *stream) try {
    FIB_RC(wp_field_check(packed, nx, ny, nz));
    FIB_CHECK(out_to_ras && ras_to_field && inv, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(niter >= 0, FIB_ERR_INVALID, "niter must not be negative");
    FIB_CHECK(nxo > 0 && nyo > 0 && nzo > 0, FIB_ERR_INVALID, "the output dimensions must be positive");
    FIB_CHECK(std::max({nxo, nyo, nzo}) <= WP_MAX_DIM, FIB_ERR_UNSUPPORTED, "an output dimension above 2^24");
    FIB_CHECK(((reinterpret_cast<uintptr_t>(inv) | reinterpret_cast<uintptr_t>(err)) & 3) == 0, FIB_ERR_INVALID, "inv and err must be 4-byte aligned");
    const uint64_t nvo = (uint64_t)nxo * nyo * nzo, bf = 16ull * (uint64_t)nx * ny * nz;
    FIB_CHECK(wp_disjoint(packed, bf, inv, 12 * nvo) && (!err || (wp_disjoint(packed, bf, err, 4 * nvo) && wp_disjoint(inv, 12 * nvo, err, 4 * nvo))),
              FIB_ERR_INVALID, "the field, inv and err must not overlap");
    constexpr int BX = 64, BY = 4;
    const unsigned nsx = (unsigned)fib::cdiv(nxo, BX), nsy = (unsigned)fib::cdiv(nyo, BY);
    FIB_CHECK(fib::cdiv(nxo, BX) * fib::cdiv(nyo, BY) * nzo < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the output volume needs 2^31 workgroups or more");
    const WarpField W{static_cast<const float4 *>(packed), nx, ny, nz};
    fib::ProfScope prof("warp_invert", (hipStream_t)stream);
    hipLaunchKernelGGL((wp_invert_kernel<BX, BY>), dim3(nsx * nsy * (unsigned)nzo), dim3(BX * BY), 0, (hipStream_t)stream, W, wp_mat(out_to_ras),
                       wp_mat(ras_to_field), niter, inv, err, nxo, nyo, nzo, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
