// vol_sample.inc — the sampler of the "Volume resampling" contract (include/fibers_hip.h), shared by volxform.hip (fibd_vol_xform: p
// comes from one matrix) and warp.hip (fibd_warp_volume: p comes through a displacement field).  One output voxel: the INSIDE rule
// on the float values of p, then FIB_VOL_NEAREST (32-bit words copied untouched) or FIB_VOL_TRILINEAR (float32, x pairs, then y, then
// z) for every frame with the same p, indices and weights.  The including file has `#pragma clang fp contract(off)` in effect: every
// multiply and add below is a separately rounded float32 operation.  Offsets are 64-bit; `dst` is the voxel's word in frame 0 of the
// output, whose frames are nvo words apart.

__device__ __forceinline__ int vx_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// UNROLL frames of the loop go together: 4 for a series (the loads of four frames are in flight at once), 1 for a volume of fewer than
// 4 frames; profiles/vol_xform/README.md has both measured
template <int UNROLL>
__device__ __forceinline__ void vx_sample(const float3 p, const uint32_t *__restrict__ vol, int nxi, int nyi, int nzi, int nframes, int interp,
                                          uint32_t fill, uint32_t *__restrict__ dst, int64_t nvo) {
    const int64_t nvi = (int64_t)nxi * nyi * nzi;
    const float rx = rintf(p.x), ry = rintf(p.y), rz = rintf(p.z);
    // tested on the float values: NaN fails every comparison, -0.0 passes, and nothing is converted to an integer before
    const bool inside = rx >= 0.f && rx <= (float)(nxi - 1) && ry >= 0.f && ry <= (float)(nyi - 1) && rz >= 0.f && rz <= (float)(nzi - 1);
    if (!inside) {
        for (int f = 0; f < nframes; f++) dst[(int64_t)f * nvo] = fill;
        return;
    }
    if (interp == FIB_VOL_NEAREST) {
        const uint32_t *src = vol + ((int64_t)(int)rx + (int64_t)nxi * ((int64_t)(int)ry + (int64_t)nyi * (int)rz));
#pragma unroll UNROLL
        for (int f = 0; f < nframes; f++) dst[(int64_t)f * nvo] = src[(int64_t)f * nvi];
        return;
    }
    // trilinear: floor in [-1, n - 1] here (rint(p) is inside), both neighbours clamped into the volume
    const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
    const float fx = p.x - flx, fy = p.y - fly, fz = p.z - flz;
    const float gx = 1.f - fx, gy = 1.f - fy, gz = 1.f - fz;
    const int x0 = vx_clamp((int)flx, nxi), x1 = vx_clamp((int)flx + 1, nxi);
    const int64_t y0 = (int64_t)nxi * vx_clamp((int)fly, nyi), y1 = (int64_t)nxi * vx_clamp((int)fly + 1, nyi);
    const int64_t z0 = (int64_t)nxi * nyi * vx_clamp((int)flz, nzi), z1 = (int64_t)nxi * nyi * vx_clamp((int)flz + 1, nzi);
    const int64_t o000 = x0 + y0 + z0, o100 = x1 + y0 + z0, o010 = x0 + y1 + z0, o110 = x1 + y1 + z0;
    const int64_t o001 = x0 + y0 + z1, o101 = x1 + y0 + z1, o011 = x0 + y1 + z1, o111 = x1 + y1 + z1;
    const float *__restrict__ v = reinterpret_cast<const float *>(vol);
    float *__restrict__ d = reinterpret_cast<float *>(dst);
#pragma unroll UNROLL                                          // (vol and out do not overlap: the loads of UNROLL frames go out together)
    for (int f = 0; f < nframes; f++, v += nvi) {
        const float c00 = gx * v[o000] + fx * v[o100], c10 = gx * v[o010] + fx * v[o110];
        const float c01 = gx * v[o001] + fx * v[o101], c11 = gx * v[o011] + fx * v[o111];
        const float c0 = gy * c00 + fy * c10;
        const float c1 = gy * c01 + fy * c11;
        d[(int64_t)f * nvo] = gz * c0 + fz * c1;
    }
}
