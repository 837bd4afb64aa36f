// xfm_apply.inc — the per-point projective 4x4 apply of xfm_apply! (util.jl:401-420), shared by xform.hip (fibd_xfm_apply) and
// the .trk epilogue of the pack kernels in stream.hip (fibd_stream_pack_trk_xfm).  The including file has `#pragma clang fp
// contract(off)` in effect: every multiply and add below is a separately rounded float32 operation, in the reference's order, and
// the division is IEEE (correctly rounded).  The division is kept for affine matrices too: a non-finite input makes out_aff NaN and
// the reference then returns NaN in all three coordinates.

// vox2vox, row-major: m[4 * i + j] = vox2vox[i + 1, j + 1] (include/fibers_hip.h)
struct XfmMat { float m[16]; };

__device__ __forceinline__ float3 xfm_point(const XfmMat &X, float x, float y, float z) {
    const float *m = X.m;
    float aff = 0.f;                                    // out_aff = Tx(0); out_aff += vox2vox[4, j] * inpoint[k+j]; += vox2vox[4, 4]
    aff = aff + m[12] * x; aff = aff + m[13] * y; aff = aff + m[14] * z; aff = aff + m[15];
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {                       // out_lin = Tx(0); out_lin += vox2vox[i, j] * inpoint[k+j]; += vox2vox[i, 4]
        float lin = 0.f;
        lin = lin + m[4 * i] * x; lin = lin + m[4 * i + 1] * y; lin = lin + m[4 * i + 2] * z; lin = lin + m[4 * i + 3];
        o[i] = lin / aff;
    }
    return make_float3(o[0], o[1], o[2]);
}
