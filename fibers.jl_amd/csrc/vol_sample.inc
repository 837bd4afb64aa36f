// vol_sample.inc — the sampler of the "Volume resampling" contract (include/fibers_hip.h), shared by volxform.hip (fibd_vol_xform: p
// comes from one matrix) and warp.hip (fibd_warp_volume: p comes through a displacement field).  One output voxel: the INSIDE rule
// on the float values of p, then FIB_VOL_NEAREST (32-bit words copied untouched) or FIB_VOL_TRILINEAR (float32, x pairs, then y, then
// z) for every frame with the same p, indices and weights.  The including file has `#pragma clang fp contract(off)` in effect: every
// multiply and add below is a separately rounded float32 operation.  Offsets are 64-bit; `dst` is the voxel's word in frame 0 of the
// output, whose frames are nvo words apart.

__device__ __forceinline__ int vx_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The INSIDE rule on the rounded coordinates (the float values of rint(p_c)): NaN fails every comparison, -0.0 passes, and nothing is
// converted to an integer before.  vx_inside is the rule alone, for a caller that skips outside samples (register.hip).
__device__ __forceinline__ bool vx_inside_rounded(float rx, float ry, float rz, int nxi, int nyi, int nzi) {
    return rx >= 0.f && rx <= (float)(nxi - 1) && ry >= 0.f && ry <= (float)(nyi - 1) && rz >= 0.f && rz <= (float)(nzi - 1);
}
__device__ __forceinline__ bool vx_inside(const float3 p, int nxi, int nyi, int nzi) {
    return vx_inside_rounded(rintf(p.x), rintf(p.y), rintf(p.z), nxi, nyi, nzi);
}

// FIB_VOL_TRILINEAR in its two steps, the one definition of its operation order.  vx_cell: the 8 offsets and the 3 weight pairs of an
// inside p (floor in [-1, n - 1] there, both neighbours clamped into the volume), the same for every frame.  vx_cell_value: one frame's
// value, x pairs, then y, then z.
struct VxCell {
    int64_t o000, o100, o010, o110, o001, o101, o011, o111;
    float fx, fy, fz, gx, gy, gz;
};
__device__ __forceinline__ VxCell vx_cell(const float3 p, int nxi, int nyi, int nzi) {
    VxCell c;
    const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
    c.fx = p.x - flx; c.fy = p.y - fly; c.fz = p.z - flz;
    c.gx = 1.f - c.fx; c.gy = 1.f - c.fy; c.gz = 1.f - c.fz;
    const int x0 = vx_clamp((int)flx, nxi), x1 = vx_clamp((int)flx + 1, nxi);
    const int64_t y0 = (int64_t)nxi * vx_clamp((int)fly, nyi), y1 = (int64_t)nxi * vx_clamp((int)fly + 1, nyi);
    const int64_t z0 = (int64_t)nxi * nyi * vx_clamp((int)flz, nzi), z1 = (int64_t)nxi * nyi * vx_clamp((int)flz + 1, nzi);
    c.o000 = x0 + y0 + z0; c.o100 = x1 + y0 + z0; c.o010 = x0 + y1 + z0; c.o110 = x1 + y1 + z0;
    c.o001 = x0 + y0 + z1; c.o101 = x1 + y0 + z1; c.o011 = x0 + y1 + z1; c.o111 = x1 + y1 + z1;
    return c;
}
__device__ __forceinline__ float vx_cell_value(const VxCell &c, const float *__restrict__ v) {
    const float c00 = c.gx * v[c.o000] + c.fx * v[c.o100], c10 = c.gx * v[c.o010] + c.fx * v[c.o110];
    const float c01 = c.gx * v[c.o001] + c.fx * v[c.o101], c11 = c.gx * v[c.o011] + c.fx * v[c.o111];
    const float c0 = c.gy * c00 + c.fy * c10;
    const float c1 = c.gy * c01 + c.fy * c11;
    return c.gz * c0 + c.fz * c1;
}

// UNROLL frames of the loop go together: 4 for a series (the loads of four frames are in flight at once), 1 for a volume of fewer than
// 4 frames; profiles/vol_xform/README.md has both measured
template <int UNROLL>
__device__ __forceinline__ void vx_sample(const float3 p, const uint32_t *__restrict__ vol, int nxi, int nyi, int nzi, int nframes, int interp,
                                          uint32_t fill, uint32_t *__restrict__ dst, int64_t nvo) {
    const int64_t nvi = (int64_t)nxi * nyi * nzi;
    const float rx = rintf(p.x), ry = rintf(p.y), rz = rintf(p.z);
    if (!vx_inside_rounded(rx, ry, rz, nxi, nyi, nzi)) {
        for (int f = 0; f < nframes; f++) dst[(int64_t)f * nvo] = fill;
        return;
    }
    if (interp == FIB_VOL_NEAREST) {
        const uint32_t *src = vol + ((int64_t)(int)rx + (int64_t)nxi * ((int64_t)(int)ry + (int64_t)nyi * (int)rz));
#pragma unroll UNROLL
        for (int f = 0; f < nframes; f++) dst[(int64_t)f * nvo] = src[(int64_t)f * nvi];
        return;
    }
    const VxCell c = vx_cell(p, nxi, nyi, nzi);
    const float *__restrict__ v = reinterpret_cast<const float *>(vol);
    float *__restrict__ d = reinterpret_cast<float *>(dst);
#pragma unroll UNROLL                                          // (vol and out do not overlap: the loads of UNROLL frames go out together)
    for (int f = 0; f < nframes; f++, v += nvi) d[(int64_t)f * nvo] = vx_cell_value(c, v);
}
