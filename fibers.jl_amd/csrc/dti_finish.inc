// dti_finish.inc — a fitted tensor's ten output fields, shared by the DTI fit (dti.hip) and the kurtosis fit (dki.hip).
// Included inside an anonymous namespace after sym3_eigen.inc, under `#pragma clang fp contract(off)`.

// dti_maps, dti.jl:325-335
__device__ __forceinline__ void dti_maps(float e1, float e2, float e3, float o[16]) {
    float rd = e2 + e3;
    const float md = (e1 + rd) / 3.0f;
    rd = rd / 2.0f;
    const float num = (e1 - md) * (e1 - md) + (e2 - md) * (e2 - md) + (e3 - md) * (e3 - md);
    const float den = e1 * e1 + e2 * e2 + e3 * e3;
    o[13] = rd; o[14] = md; o[15] = sqrtf(num / den * 1.5f);
}
__device__ __forceinline__ void dti_finish_inl(const float d[7], float o[16]) {
    float w[3], ev[3][3];
    o[0] = expf(d[6]);
    sym3_eigen(d[0], d[1], d[2], d[3], d[4], d[5], w, ev);
    const float e1 = w[2], e2 = w[1], e3 = w[0];
    o[1] = e1; o[2] = e2; o[3] = e3;
#pragma unroll
    for (int c = 0; c < 3; c++) { o[4 + c] = ev[2][c]; o[7 + c] = ev[1][c]; o[10 + c] = ev[0][c]; }
    dti_maps(e1, e2, e3, o);
}
