// warp_sample.inc — the field sample S(q) of the "Non-linear warps" contract (include/fibers_hip.h), shared by warp.hip (the warp of
// points and volumes, the inverse) and nlreg.hip (the demons step, the upsampling between levels).  The packed field is float4 [nvox] =
// (dx, dy, dz, 0), 16-byte aligned.  The including file has `#pragma clang fp contract(off)` in effect: every multiply and add below is a
// separately rounded float32 operation.  Offsets are 64-bit.

struct WarpField { const float4 *f; int nx, ny, nz; };

// one component of q: the clamp (the edge displacement continues beyond the grid: +-Inf clamp, -0.0 passes), then floor and fraction
__device__ __forceinline__ void wp_axis(float q, int n, int &i0, int &i1, float &f, float &g) {
    const float hi = (float)(n - 1);
    const float qc = q < 0.f ? 0.f : (q > hi ? hi : q);
    const float fl = floorf(qc);
    i0 = (int)fl;
    f = qc - fl;
    g = 1.f - f;
    i1 = min(i0 + 1, n - 1);
}

__device__ __forceinline__ float wp_lerp3(float gx, float fx, float gy, float fy, float gz, float fz, float v000, float v100, float v010, float v110,
                                          float v001, float v101, float v011, float v111) {
    const float c00 = gx * v000 + fx * v100, c10 = gx * v010 + fx * v110;
    const float c01 = gx * v001 + fx * v101, c11 = gx * v011 + fx * v111;
    const float c0 = gy * c00 + fy * c10;
    const float c1 = gy * c01 + fy * c11;
    return gz * c0 + fz * c1;
}

// S(q): q in field-voxel coordinates (0-based).  A NaN in any component gives three NaNs (nothing is converted to an integer then).
__device__ __forceinline__ float3 wp_sample(const WarpField &W, const float3 q) {
    if (q.x != q.x || q.y != q.y || q.z != q.z) {
        const float n = __builtin_nanf("");
        return make_float3(n, n, n);
    }
    int x0, x1, y0, y1, z0, z1;
    float fx, gx, fy, gy, fz, gz;
    wp_axis(q.x, W.nx, x0, x1, fx, gx);
    wp_axis(q.y, W.ny, y0, y1, fy, gy);
    wp_axis(q.z, W.nz, z0, z1, fz, gz);
    const int64_t r0 = (int64_t)W.nx * y0, r1 = (int64_t)W.nx * y1;
    const int64_t s0 = (int64_t)W.nx * W.ny * z0, s1 = (int64_t)W.nx * W.ny * z1;
    const float4 v000 = W.f[x0 + r0 + s0], v100 = W.f[x1 + r0 + s0], v010 = W.f[x0 + r1 + s0], v110 = W.f[x1 + r1 + s0];
    const float4 v001 = W.f[x0 + r0 + s1], v101 = W.f[x1 + r0 + s1], v011 = W.f[x0 + r1 + s1], v111 = W.f[x1 + r1 + s1];
    return make_float3(wp_lerp3(gx, fx, gy, fy, gz, fz, v000.x, v100.x, v010.x, v110.x, v001.x, v101.x, v011.x, v111.x),
                       wp_lerp3(gx, fx, gy, fy, gz, fz, v000.y, v100.y, v010.y, v110.y, v001.y, v101.y, v011.y, v111.y),
                       wp_lerp3(gx, fx, gy, fy, gz, fz, v000.z, v100.z, v010.z, v110.z, v001.z, v101.z, v011.z, v111.z));
}
