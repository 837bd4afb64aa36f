// dki.hip — per-voxel diffusion kurtosis fit and the MK / AK / RK maps on gfx950 (not in the reference: DESIGN.md §5 is the definition).
//
//   ln S = ln S0 - b g'Dg + (b^2 / 6) sum g_i g_j g_k g_l V_ijkl,   V = MD^2 W,   d[22] = (D 6, V 15, ln S0) = pA log(max(s, min_signal))
//
// Design (1080 B in at 270 frames, 136 B out per voxel; ~6 k FMAs for the fit and ~12 k VALU operations for the maps at 321 directions):
//   - one thread per voxel, planar coalesced frame reads, as dti.hip's fit_kernel;
//   - the pseudo-inverse columns ([nvol][24]: the 22 float32 values widened to double, and padding) are read at wave-uniform
//     addresses, i.e. through the scalar cache into SGPRs; 22 float64 accumulators per lane and float64 logarithms, rounded to
//     float32 once, at d: a scheme that barely determines the 22 unknowns (22 frames: sigma_min / sigma_max = 1.2e-4) turns the last
//     place of a float32 logarithm into 1e-4 of mk, and which way is luck;
//   - the direction table ([ndir][21]: the 6 quadratic and 15 multiplicity-weighted quartic monomials of every vertex of the half
//     sphere) takes the same scalar path: D(n) and V(n) are 21 FMAs with one SGPR operand each, no LDS and no VGPRs for the table;
//   - fit and maps are one kernel: the 22 fitted values never leave the registers.
#include <cmath>

#include "common.h"

// as dti.hip: the eigen-solver's cancellation-prone cross products stay uncontracted, FMAs are written explicitly
#pragma clang fp contract(off)

namespace {

struct DkiOutPtrs {
    float *s0, *l1, *l2, *l3, *e1, *e2, *e3, *rd, *md, *fa, *mk, *ak, *rk, *kt;
};
// the kernel's constants: fib_dki_params, whether the clip applies, and the radial quadrature's cos / sin (m pi / 16)
struct DkiConst {
    float min_signal, min_diffusivity, min_kurtosis, max_kurtosis;
    int clip;
    float cs[16], sn[16];
};

#include "sym3_eigen.inc"
#include "dti_finish.inc"

// K = clip(V(n) / max(D(n), min_diffusivity)^2): comparisons, so that NaN passes through
__device__ __forceinline__ float dki_ratio(float dn, float vn, const DkiConst &P) {
    const float den = dn < P.min_diffusivity ? P.min_diffusivity : dn;
    float k = vn / (den * den);
    if (P.clip) {
        if (k < P.min_kurtosis) k = P.min_kurtosis;
        if (k > P.max_kurtosis) k = P.max_kurtosis;
    }
    return k;
}

// K(n) from a row of the direction table (wave-uniform: SGPR operands)
__device__ __forceinline__ float dki_k_row(const float *__restrict__ q, const float d[22], const DkiConst &P) {
    float dn = q[0] * d[0];
#pragma unroll
    for (int k = 1; k < 6; k++) dn = __builtin_fmaf(q[k], d[k], dn);
    float vn = q[6] * d[6];
#pragma unroll
    for (int k = 7; k < 21; k++) vn = __builtin_fmaf(q[k], d[k], vn);
    return dki_ratio(dn, vn, P);
}

// K(n) of a direction that differs from lane to lane (an eigenvector): the same 21 monomials, in registers
__device__ __forceinline__ float dki_k_dir(float x, float y, float z, const float d[22], const DkiConst &P) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
    float q[21];
    q[0] = xx; q[1] = 2.0f * xy; q[2] = 2.0f * xz; q[3] = yy; q[4] = 2.0f * yz; q[5] = zz;
    q[6] = xx * xx; q[7] = yy * yy; q[8] = zz * zz;
    q[9] = 4.0f * (xx * xy); q[10] = 4.0f * (xx * xz); q[11] = 4.0f * (xy * yy); q[12] = 4.0f * (yy * yz);
    q[13] = 4.0f * (xz * zz); q[14] = 4.0f * (yz * zz);
    q[15] = 6.0f * (xx * yy); q[16] = 6.0f * (xx * zz); q[17] = 6.0f * (yy * zz);
    q[18] = 12.0f * (xx * yz); q[19] = 12.0f * (yy * xz); q[20] = 12.0f * (zz * xy);
    return dki_k_row(q, d, P);
}

// coef: [nvol][24] = pA[:, i] (22 values) and padding; dirs: [ndir][21]
template <int UNR>
__global__ __launch_bounds__(256) void dki_kernel(const float *__restrict__ dwi, const uint8_t *__restrict__ mask,
                                                  const double *__restrict__ coef, const float *__restrict__ dirs, int ndir,
                                                  int nvol, int64_t nvox, DkiOutPtrs out, const DkiConst P) {
    const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= nvox) return;
    const bool inside = mask[vox] != 0;
    // a wave whose voxels are all outside the mask reads no frame at all
    const int nframes = __any(inside) ? nvol : 0;
    double acc[22];
#pragma unroll
    for (int j = 0; j < 22; j++) acc[j] = 0.0;
    float smax = -INFINITY;
    bool anynan = false;
    const float *src = dwi + vox;
#pragma unroll UNR
    for (int i = 0; i < nframes; i++) {
        const float s = __builtin_nontemporal_load(src + (int64_t)i * nvox);
        const double *c = coef + 24 * i;                                           // wave-uniform: scalar loads
        smax = fmaxf(smax, s);
        anynan |= s != s;
        const double l = log((double)(s < P.min_signal ? P.min_signal : s));       // the clamp is the rule for non-positive samples
#pragma unroll
        for (int j = 0; j < 22; j++) acc[j] = __builtin_fma(c[j], l, acc[j]);
    }
    float d[22];
#pragma unroll
    for (int j = 0; j < 22; j++) d[j] = (float)acc[j];
    const bool solved = inside && smax > 0.0f && !anynan;

    float o[16];
#pragma unroll
    for (int k = 0; k < 16; k++) o[k] = 0.0f;
    if (solved) {
        const float d7[7] = {d[0], d[1], d[2], d[3], d[4], d[5], d[21]};
        dti_finish_inl(d7, o);
    }
    __builtin_nontemporal_store(o[0], out.s0 + vox);
    __builtin_nontemporal_store(o[1], out.l1 + vox);
    __builtin_nontemporal_store(o[2], out.l2 + vox);
    __builtin_nontemporal_store(o[3], out.l3 + vox);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        __builtin_nontemporal_store(o[4 + c], out.e1 + c * nvox + vox);
        __builtin_nontemporal_store(o[7 + c], out.e2 + c * nvox + vox);
        __builtin_nontemporal_store(o[10 + c], out.e3 + c * nvox + vox);
    }
    __builtin_nontemporal_store(o[13], out.rd + vox);
    __builtin_nontemporal_store(o[14], out.md + vox);
    __builtin_nontemporal_store(o[15], out.fa + vox);

    float mk = 0.0f, ak = 0.0f, rk = 0.0f;
#ifndef FIB_DKI_NO_MAPS
    if (solved) {
        // mean kurtosis: a sequential sum over the half sphere in vertex order
        float sum = 0.0f;
#pragma unroll 2
        for (int v = 0; v < ndir; v++) sum += dki_k_row(dirs + 21 * v, d, P);
        mk = sum / (float)ndir;
        ak = dki_k_dir(o[4], o[5], o[6], d, P);
        // radial kurtosis: 16 equally spaced directions of the half circle spanned by eigvec2 and eigvec3
        float rsum = 0.0f;
#pragma unroll 1
        for (int m = 0; m < 16; m++) {
            const float c = P.cs[m], s = P.sn[m];
            rsum += dki_k_dir(c * o[7] + s * o[10], c * o[8] + s * o[11], c * o[9] + s * o[12], d, P);
        }
        rk = rsum / 16.0f;
    }
#endif
    __builtin_nontemporal_store(mk, out.mk + vox);
    __builtin_nontemporal_store(ak, out.ak + vox);
    __builtin_nontemporal_store(rk, out.rk + vox);
    if (out.kt) {
        const float md2 = o[14] * o[14];
#pragma unroll
        for (int k = 0; k < 15; k++) __builtin_nontemporal_store(solved ? d[6 + k] / md2 : 0.0f, out.kt + (int64_t)k * nvox + vox);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------
struct fib_dki_plan {
    int device = 0;
    int nvol = 0;
    int ndir = 0;
    std::vector<float> A, pA, dirs;     // host copies: [nvol x 22], [22 x nvol] column-major; [ndir][21]
    fib::DevBuf<double> coef;           // [nvol][24]
    fib::DevBuf<float> dirtab;          // [ndir][21]
    DkiConst P;
};

extern "C" int fib_dki_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                                   const fib_dki_params *params, fib_dki_plan **plan) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan output pointer is NULL");
    *plan = nullptr;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    FIB_CHECK(verts != nullptr && nverts >= 2, FIB_ERR_INVALID, "the ODF tessellation needs at least two vertices");
    fib_dki_params pr{1e-4f, 1e-6f, -3.0f / 7.0f, 10.0f};
    if (params) pr = *params;
    FIB_CHECK(pr.min_signal > 0.0f && pr.min_diffusivity > 0.0f, FIB_ERR_INVALID, "min_signal and min_diffusivity must be positive");
    FIB_CHECK(pr.min_kurtosis == pr.min_kurtosis && pr.max_kurtosis == pr.max_kurtosis, FIB_ERR_INVALID, "the kurtosis limits must not be NaN");
    fib::DeviceGuard guard;
    FIB_RC(fib::use_device(device));
    std::unique_ptr<fib_dki_plan> p(new fib_dki_plan());
    p->device = device;
    p->nvol = nvol;
    p->ndir = nverts / 2;
    p->A.resize((size_t)nvol * 22);
    p->pA.resize((size_t)nvol * 22);
    FIB_RC(fib_dki_design(bval, bvec, nvol, p->A.data(), p->pA.data(), nullptr));
    p->dirs.resize((size_t)p->ndir * 21);
    for (int v = 0; v < p->ndir; v++) {
        double row[21];
        fib::host_dki_dir_row(verts[v], verts[v + nverts], verts[v + 2 * (size_t)nverts], row);
        for (int k = 0; k < 21; k++) p->dirs[(size_t)21 * v + k] = (float)row[k];
    }
    p->P.min_signal = pr.min_signal; p->P.min_diffusivity = pr.min_diffusivity;
    p->P.min_kurtosis = pr.min_kurtosis; p->P.max_kurtosis = pr.max_kurtosis;
    p->P.clip = pr.min_kurtosis < pr.max_kurtosis ? 1 : 0;
    for (int m = 0; m < 16; m++) {
        p->P.cs[m] = (float)std::cos(m * M_PI / 16.0);
        p->P.sn[m] = (float)std::sin(m * M_PI / 16.0);
    }
    std::vector<double> coef((size_t)nvol * 24, 0.0);
    for (int i = 0; i < nvol; i++)
        for (int j = 0; j < 22; j++) coef[(size_t)24 * i + j] = p->pA[j + (size_t)22 * i];
    FIB_RC(fib::upload(p->coef, coef));
    FIB_RC(fib::upload(p->dirtab, p->dirs));
    *plan = p.release();
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fib_dki_plan_destroy(fib_dki_plan *plan) try { fib::plan_destroy(plan); } FIB_API_CATCH_VOID

extern "C" int fib_dki_plan_tables(const fib_dki_plan *plan, float *A, float *pA, float *dirs) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan is NULL");
    if (A) memcpy(A, plan->A.data(), plan->A.size() * sizeof(float));
    if (pA) memcpy(pA, plan->pA.data(), plan->pA.size() * sizeof(float));
    if (dirs) memcpy(dirs, plan->dirs.data(), plan->dirs.size() * sizeof(float));
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dki_fit(const fib_dki_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox,
                            const fib_dki_out *out, void *stream) try {
    FIB_CHECK(plan && dwi && mask && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(out->s0 && out->eigval1 && out->eigval2 && out->eigval3 && out->eigvec1 && out->eigvec2 && out->eigvec3 &&
              out->rd && out->md && out->fa && out->mk && out->ak && out->rk, FIB_ERR_INVALID, "NULL output volume");
    FIB_CHECK(nvox > 0, FIB_ERR_INVALID, "nvox must be positive");
    FIB_CHECK(nvox < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(plan->device));
    const DkiOutPtrs o{out->s0, out->eigval1, out->eigval2, out->eigval3, out->eigvec1, out->eigvec2, out->eigvec3,
                       out->rd, out->md, out->fa, out->mk, out->ak, out->rk, out->kt};
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("dki_fit", st);
    const int block = 256;
    const unsigned grid = (unsigned)fib::cdiv(nvox, block);
    hipLaunchKernelGGL((dki_kernel<4>), dim3(grid), dim3(block), 0, st, dwi, mask, plan->coef.p, plan->dirtab.p, plan->ndir,
                       plan->nvol, nvox, o, plan->P);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
