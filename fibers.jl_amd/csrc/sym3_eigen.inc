// sym3_eigen.inc — the 3x3 symmetric eigen-solver shared by the tensor fit (dti.hip) and the structure tensor (structens.hip).
// Included inside an anonymous namespace, after `#pragma clang fp contract(off)`: the includer owns both, so every copy
// compiles to the same arithmetic (fibd_st_eigen and the fused st_recon eigen-solve agree bit for bit).

__device__ __forceinline__ void cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// StaticArrays `_eig(::Size{(3,3)}, ::RealHermSymComplexHerm)`: trigonometric eigenvalues, eigenvectors
// from the best-conditioned cross product, 2x2 sub-problem for the second one.  Ascending eigenvalues
// w[0..2], eigenvectors ev[k][:].
__device__ __forceinline__ void sym3_eigen(float a11, float a12, float a13, float a22, float a23, float a33,
                           float w[3], float ev[3][3]) {
    const float p1 = a12 * a12 + a13 * a13 + a23 * a23;
    if (p1 == 0.0f) {  // diagonal matrix: sorted diagonal, unit axes
        int o0, o1, o2;
        if (a11 < a22) {
            if (a22 < a33)      { o0 = 0; o1 = 1; o2 = 2; }
            else if (a33 < a11) { o0 = 2; o1 = 0; o2 = 1; }
            else                { o0 = 0; o1 = 2; o2 = 1; }
        } else {
            if (a11 < a33)      { o0 = 1; o1 = 0; o2 = 2; }
            else if (a33 < a22) { o0 = 2; o1 = 1; o2 = 0; }
            else                { o0 = 1; o1 = 2; o2 = 0; }
        }
#define FIB_DIAG_ROW(k, o)                                   \
        w[k] = (o) == 0 ? a11 : ((o) == 1 ? a22 : a33);      \
        ev[k][0] = (o) == 0 ? 1.0f : 0.0f;                   \
        ev[k][1] = (o) == 1 ? 1.0f : 0.0f;                   \
        ev[k][2] = (o) == 2 ? 1.0f : 0.0f;
        FIB_DIAG_ROW(0, o0)
        FIB_DIAG_ROW(1, o1)
        FIB_DIAG_ROW(2, o2)
#undef FIB_DIAG_ROW
        return;
    }
    const float q = (a11 + a22 + a33) / 3.0f;
    const float p2 = (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + (a33 - q) * (a33 - q) + 2.0f * p1;
    const float p = sqrtf(p2 / 6.0f);
    const float invp = 1.0f / p;
    const float b11 = (a11 - q) * invp, b22 = (a22 - q) * invp, b33 = (a33 - q) * invp;
    const float b12 = a12 * invp, b13 = a13 * invp, b23 = a23 * invp;
    const float detB = b11 * (b22 * b33 - b23 * b23) - b12 * (b12 * b33 - b23 * b13) + b13 * (b12 * b23 - b22 * b13);
    const float r = detB / 2.0f;
    const float PI_F = 3.14159274101257324f;
    float phi;
    if (r <= -1.0f)     phi = PI_F / 3.0f;
    else if (r >= 1.0f) phi = 0.0f;
    else                phi = acosf(r) / 3.0f;
    float eig3 = q + 2.0f * p * cosf(phi);
    float eig1 = q + 2.0f * p * cosf(phi + (2.0f * PI_F / 3.0f));
    const float eig2 = 3.0f * q - eig1 - eig3;
    if (r > 0.0f) { const float t = eig1; eig1 = eig3; eig3 = t; }

    const float r1[3] = {a11 - eig1, a12, a13};
    const float r2[3] = {a12, a22 - eig1, a23};
    const float r3[3] = {a13, a23, a33 - eig1};
    const float n1 = r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2];
    const float n2 = r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2];
    const float n3 = r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2];
    float r12[3], r23[3], r31[3];
    cross3(r1, r2, r12); cross3(r2, r3, r23); cross3(r3, r1, r31);
    const float n12 = r12[0] * r12[0] + r12[1] * r12[1] + r12[2] * r12[2];
    const float n23 = r23[0] * r23[0] + r23[1] * r23[1] + r23[2] * r23[2];
    const float n31 = r31[0] * r31[0] + r31[1] * r31[1] + r31[2] * r31[2];
    int sel;  // 0: r12, 1: r23, 2: r31
    if (n12 * n3 > n23 * n1) sel = (n12 * n3 > n31 * n2) ? 0 : 2;
    else                     sel = (n23 * n1 > n31 * n2) ? 1 : 2;
    float v1[3];
    {
        const float nb = sel == 0 ? n12 : (sel == 1 ? n23 : n31);
        const float s = sqrtf(nb);
#pragma unroll
        for (int c = 0; c < 3; c++) v1[c] = (sel == 0 ? r12[c] : (sel == 1 ? r23[c] : r31[c])) / s;
    }
    float o1[3], o2[3];
    if (fabsf(v1[0]) < fabsf(v1[1])) {
        const float s = sqrtf(v1[0] * v1[0] + v1[2] * v1[2]);
        o1[0] = -v1[2] / s; o1[1] = 0.0f / s; o1[2] = v1[0] / s;
    } else {
        const float s = sqrtf(v1[1] * v1[1] + v1[2] * v1[2]);
        o1[0] = 0.0f / s; o1[1] = v1[2] / s; o1[2] = -v1[1] / s;
    }
    cross3(v1, o1, o2);
    const float ao1[3] = {a11 * o1[0] + a12 * o1[1] + a13 * o1[2],
                          a12 * o1[0] + a22 * o1[1] + a23 * o1[2],
                          a13 * o1[0] + a23 * o1[1] + a33 * o1[2]};
    const float ao2[3] = {a11 * o2[0] + a12 * o2[1] + a13 * o2[2],
                          a12 * o2[0] + a22 * o2[1] + a23 * o2[2],
                          a13 * o2[0] + a23 * o2[1] + a33 * o2[2]};
    const float c11 = o1[0] * ao1[0] + o1[1] * ao1[1] + o1[2] * ao1[2] - eig2;
    const float c12 = o1[0] * ao2[0] + o1[1] * ao2[1] + o1[2] * ao2[2];
    const float c22 = o2[0] * ao2[0] + o2[1] * ao2[1] + o2[2] * ao2[2] - eig2;
    const float c11s = c11 * c11, c12s = c12 * c12, c22s = c22 * c22;
    float q1 = 1.0f, q2 = 0.0f;   // eigvec2 = q1*o1 - q2*o2 (defaults: orthogonal1)
    if (c11s >= c22s) {
        if (c11s > 0.0f || c12s > 0.0f) {
            if (c11s >= c12s) { const float t = c12 / c11; q2 = 1.0f / sqrtf(1.0f + t * t); q1 = t * q2; }
            else              { const float t = c11 / c12; q1 = 1.0f / sqrtf(1.0f + t * t); q2 = t * q1; }
        }
    } else {
        if (c22s >= c12s) { const float t = c12 / c22; q1 = 1.0f / sqrtf(1.0f + t * t); q2 = t * q1; }
        else              { const float t = c22 / c12; q2 = 1.0f / sqrtf(1.0f + t * t); q1 = t * q2; }
    }
    float v2[3], v3[3];
    const bool degenerate = (c11s >= c22s) && !(c11s > 0.0f || c12s > 0.0f);
#pragma unroll
    for (int c = 0; c < 3; c++) v2[c] = degenerate ? o1[c] : q1 * o1[c] - q2 * o2[c];
    cross3(v1, v2, v3);
    if (r > 0.0f) {
        const float t = eig1; eig1 = eig3; eig3 = t;
#pragma unroll
        for (int c = 0; c < 3; c++) { const float u = v1[c]; v1[c] = v3[c]; v3[c] = u; }
    }
    w[0] = eig1; w[1] = eig2; w[2] = eig3;
#pragma unroll
    for (int c = 0; c < 3; c++) { ev[0][c] = v1[c]; ev[1][c] = v2[c]; ev[2][c] = v3[c]; }
}
