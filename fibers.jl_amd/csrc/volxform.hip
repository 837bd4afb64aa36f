// volxform.hip — a volume moved through an `Xform` on gfx950 (fibd_vol_xform): every output voxel is pulled back through the
// output -> input matrix (xfm_point, xfm_apply.inc) and the input volume is sampled there, nearest voxel (32-bit words copied
// untouched) or trilinear (float32).  Not in the reference: the definitions are the "Volume resampling" section of
// include/fibers_hip.h.  Volumes are planar [nframes][nz][ny][nx], x fastest, 0-based voxel coordinates.
//
// A gather kernel (the sampler itself is vol_sample.inc, shared with warp.hip): one thread per output voxel, x along the lanes, so a wave's stores are consecutive words and its gathers follow
// one straight line through the input.  Coordinates, the inside test, the 8 offsets and the 3 weight pairs are made once and reused
// for every frame.  Offsets are 64-bit (a DWI series on an anatomical grid passes 2^31 elements).  Stores are single words: `out` may
// start at any 4-byte boundary and no head or tail is needed.
//
// Workgroup shape: vx_kernel<64, 4, .> is a tile of four neighbouring x-row segments, a wave each (L2 locality under rotation); it was
// measured against vx_kernel<256, 1, .>, a segment of one x-row, which stays as its A/B partner in the diagnostic build
// (FIBERS_VOL_XFORM_TILE=0, tools/vol_xform_time.py).  The numbers are in profiles/vol_xform/README.md.
#include "common.h"

#include <algorithm>

// the pull-back and the interpolation are sequences of separately rounded float32 operations: nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "xfm_apply.inc"

#include "vol_sample.inc"

constexpr int VX_MAX_DIM = 1 << 24;                            // every size is exact in float32 (the inside test compares floats)

// UNROLL frames of the sampler's loop go together (vol_sample.inc): 4 for a series (116 VGPRs, 4 waves per SIMD), 1 for a volume of
// fewer than 4 frames (62 VGPRs, 8 waves per SIMD); profiles/vol_xform/README.md has both measured
template <int BX, int BY, int UNROLL>
__global__ __launch_bounds__(BX * BY) void vx_kernel(const XfmMat M, const uint32_t *__restrict__ vol, int nxi, int nyi, int nzi, int nframes,
                                                     int interp, uint32_t fill, uint32_t *__restrict__ out, int nxo, int nyo, int nzo, unsigned nsx, unsigned nsy) {
    const unsigned b = blockIdx.x, bx = b % nsx, r = b / nsx, by = r % nsy, k = r / nsy;
    const int i = (int)(bx * BX) + (int)(threadIdx.x % BX), j = (int)(by * BY) + (int)(threadIdx.x / BX);
    if (i >= nxo || j >= nyo) return;
    const int64_t nvo = (int64_t)nxo * nyo * nzo;
    uint32_t *dst = out + ((int64_t)i + (int64_t)nxo * ((int64_t)j + (int64_t)nyo * k));
    vx_sample<UNROLL>(xfm_point(M, (float)i, (float)j, (float)k), vol, nxi, nyi, nzi, nframes, interp, fill, dst, nvo);
}

template <int BX, int BY>
void vx_launch(const XfmMat &M, const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, uint32_t fill, void *out, int nxo, int nyo,
               int nzo, hipStream_t st) {
    const unsigned nsx = (unsigned)fib::cdiv(nxo, BX), nsy = (unsigned)fib::cdiv(nyo, BY);
    // a flat grid over (x segment, y tile, z): no 65535 limit on ny or nz
    const dim3 grid(nsx * nsy * (unsigned)nzo), block(BX * BY);
    const uint32_t *src = static_cast<const uint32_t *>(vol);
    uint32_t *dst = static_cast<uint32_t *>(out);
    if (nframes >= 4) hipLaunchKernelGGL((vx_kernel<BX, BY, 4>), grid, block, 0, st, M, src, nxi, nyi, nzi, nframes, interp, fill, dst, nxo, nyo, nzo, nsx, nsy);
    else hipLaunchKernelGGL((vx_kernel<BX, BY, 1>), grid, block, 0, st, M, src, nxi, nyi, nzi, nframes, interp, fill, dst, nxo, nyo, nzo, nsx, nsy);
}

}  // namespace

extern "C" int fibd_vol_xform(const float out2in[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits,
                              void *out, int nxo, int nyo, int nzo, void *stream) try {
    FIB_CHECK(out2in && vol && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nxi > 0 && nyi > 0 && nzi > 0 && nxo > 0 && nyo > 0 && nzo > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(interp == FIB_VOL_NEAREST || interp == FIB_VOL_TRILINEAR, FIB_ERR_INVALID, "unknown interpolation %d", interp);
    FIB_CHECK(std::max({nxi, nyi, nzi, nxo, nyo, nzo}) <= VX_MAX_DIM, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    const uintptr_t ai = reinterpret_cast<uintptr_t>(vol), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK((ai & 3) == 0 && (ao & 3) == 0, FIB_ERR_INVALID, "volumes must be 4-byte aligned");
    const uint64_t bi = 4ull * (uint64_t)nxi * nyi * nzi * nframes, bo = 4ull * (uint64_t)nxo * nyo * nzo * nframes;
    // a gather: any output word may be read as another thread's input, so there is no in-place form
    FIB_CHECK(ai + bi <= ao || ao + bo <= ai, FIB_ERR_INVALID, "vol and out must not overlap");
    XfmMat M;
    memcpy(M.m, out2in, sizeof M.m);
    bool tile = true;
    if (const char *e = fib::ab_env("FIBERS_VOL_XFORM_TILE")) tile = e[0] != '0';
    const int bx = tile ? 64 : 256, by = tile ? 4 : 1;
    FIB_CHECK(fib::cdiv(nxo, bx) * fib::cdiv(nyo, by) * nzo < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the output volume needs 2^31 workgroups or more");
    fib::ProfScope prof("vol_xform", (hipStream_t)stream);
    if (tile) vx_launch<64, 4>(M, vol, nxi, nyi, nzi, nframes, interp, (uint32_t)outside_bits, out, nxo, nyo, nzo, (hipStream_t)stream);
    else vx_launch<256, 1>(M, vol, nxi, nyi, nzi, nframes, interp, (uint32_t)outside_bits, out, nxo, nyo, nzo, (hipStream_t)stream);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
