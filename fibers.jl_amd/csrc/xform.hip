// xform.hip — xfm_apply (util.jl:385-420) on gfx950: the projective 4x4 vox2vox of an `Xform` applied to packed float32 points
// [npoints][3] in HBM (fibd_xfm_apply).  The arithmetic is xfm_point (xfm_apply.inc): the reference's loop, float32, no contraction.
//
// A copy kernel: 24 B per point and a dozen flops.  A lane takes 4 points = 48 B = three 16-byte loads and three 16-byte stores.
// Points may start at any 4-byte boundary (a view that starts at point 1 is 12 B off): the first h < 4 points, chosen so that the
// rest starts 16-byte aligned in `in` and in `out`, and the last (npoints - h) % 4 go through the scalar lanes of block 0.  When
// `in` and `out` are misaligned differently (no h aligns both) every point takes the scalar path.
#include "common.h"

#include <algorithm>

// xfm_apply! is a sequence of separately rounded float32 operations (Julia does not contract): nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "xfm_apply.inc"

constexpr int XF_BLOCK = 256;

__device__ __forceinline__ void xfm_one(const XfmMat &X, const float *in, float *out, int64_t p) {
    const float3 r = xfm_point(X, in[3 * p], in[3 * p + 1], in[3 * p + 2]);
    out[3 * p] = r.x; out[3 * p + 1] = r.y; out[3 * p + 2] = r.z;
}

// quads [0, nquad) of points starting at point h (16-byte aligned in both arrays); block 0 also does the h head points and the
// `tail` points after the last quad
__global__ __launch_bounds__(XF_BLOCK) void xfm_apply_kernel(const XfmMat X, const float *in, float *out, int64_t h, int64_t nquad, int tail) {
    const int64_t q = (int64_t)blockIdx.x * XF_BLOCK + threadIdx.x;
    if (q < nquad) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 *src = reinterpret_cast<const f4 *>(in + 3 * h) + 3 * q;
        f4 *dst = reinterpret_cast<f4 *>(out + 3 * h) + 3 * q;
        // plain loads and stores: the non-temporal forms were measured slower here (C4's points: 0.742 ms against 0.586, profiles/xform/)
        const f4 a = src[0], b = src[1], c = src[2];
        const float3 p0 = xfm_point(X, a.x, a.y, a.z), p1 = xfm_point(X, a.w, b.x, b.y);
        const float3 p2 = xfm_point(X, b.z, b.w, c.x), p3 = xfm_point(X, c.y, c.z, c.w);
        const f4 u = {p0.x, p0.y, p0.z, p1.x}, v = {p1.y, p1.z, p2.x, p2.y}, w = {p2.z, p3.x, p3.y, p3.z};
        dst[0] = u; dst[1] = v; dst[2] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x >= XF_BLOCK - 8) {   // (the last wave: its quads are the grid's fewest when nquad is small)
        const int t = threadIdx.x - (XF_BLOCK - 8);
        if (t < h) xfm_one(X, in, out, t);
        else if (t >= 4 && t - 4 < tail) xfm_one(X, in, out, h + 4 * nquad + (t - 4));
    }
}

// every point on its own (in and out misaligned against each other)
__global__ __launch_bounds__(XF_BLOCK) void xfm_apply_scalar_kernel(const XfmMat X, const float *in, float *out, int64_t npoints) {
    const int64_t p = (int64_t)blockIdx.x * XF_BLOCK + threadIdx.x;
    if (p < npoints) xfm_one(X, in, out, p);
}

}  // namespace

extern "C" int fibd_xfm_apply(const float vox2vox[16], const float *in, float *out, int64_t npoints, void *stream) try {
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    if (npoints == 0) return FIB_OK;
    FIB_CHECK(vox2vox && in && out, FIB_ERR_INVALID, "NULL argument");
    const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK((ai & 3) == 0 && (ao & 3) == 0, FIB_ERR_INVALID, "points must be 4-byte aligned");
    // in place or not at all: a partial overlap would let one lane's stores reach another lane's loads
    FIB_CHECK(ai == ao || ai + 12 * (uint64_t)npoints <= ao || ao + 12 * (uint64_t)npoints <= ai, FIB_ERR_INVALID,
              "in and out must be the same array or not overlap");
    XfmMat X;
    memcpy(X.m, vox2vox, sizeof X.m);
    fib::ProfScope prof("xfm_apply", (hipStream_t)stream);
    if (((ai ^ ao) & 15) == 0) {
        int64_t h = 0;                                          // 12 h = -in (mod 16): h = 0, 1, 2, 3 for in = 0, 4, 8, 12 (mod 16)
        while (((ai + 12 * h) & 15) != 0) h++;
        if (h > npoints) h = npoints;
        const int64_t nquad = (npoints - h) / 4;
        const int tail = (int)(npoints - h - 4 * nquad);
        hipLaunchKernelGGL(xfm_apply_kernel, dim3((unsigned)std::max<int64_t>(1, fib::cdiv(nquad, XF_BLOCK))), dim3(XF_BLOCK), 0,
                           (hipStream_t)stream, X, in, out, h, nquad, tail);
    } else
        hipLaunchKernelGGL(xfm_apply_scalar_kernel, dim3((unsigned)fib::cdiv(npoints, XF_BLOCK)), dim3(XF_BLOCK), 0, (hipStream_t)stream,
                           X, in, out, npoints);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
