// csd.hip — constrained spherical deconvolution (fODF) per voxel on gfx950 (not in the reference: include/fibers_hip.h and
// DESIGN.md §5 are the definition).
//
//   f0 = argmin |X0 f - s|  (the columns of l <= 4),   thr = tau B[0,0] f0[0]
//   repeat:  a = B f;  set = {i : a_i < thr};  stop when the set repeats;  (X'X + sum_{i in set} b_i b_i') f = X's
//
// Design (one wave per voxel; n = 45 unknowns, nreg = 362 directions, 84 shell frames at the headline shape):
//   - the loop is wave-uniform: the set is nreg ballot bits in SGPRs, the stopping test compares six scalar words, the rows of
//     the set are walked by s_ff1 on those words -- no lane diverges on membership;
//   - P = X'X + sum b b' is accumulated IN REGISTERS: lane (a, b) of the 8 x 8 lane grid owns the entries (a + 8p, b + 8q), p >= q,
//     of the lower triangle (21 float64 accumulators at n = 45), so a row of the set costs 2 NB LDS reads and conversions and
//     NB (NB + 1) / 2 FMAs per lane instead of two reads per entry.  When the set is the larger side, the complement's rows are
//     subtracted from X'X + B'B (both bases come from the cache, 18 KB each, once per iteration);
//   - the factor lives in the wave's LDS as a column-packed lower triangle (1035 float64): a right-looking Cholesky whose trailing
//     update is one contiguous range of the packing, spread over the 64 lanes through a table entry -> (row, column);
//   - the two triangular solves keep the right-hand side in registers (lane r holds element r) and broadcast with readlane;
//   - B ([nreg][n | 1] float32, 65 KB) sits in LDS for the whole workgroup at lmax 8 (eight waves, 142 KB, one workgroup per CU); at
//     lmax <= 6 it is read through the cache and two workgroups share a CU (profiles/csd/ has both sides of both);
//   - every sum after the float32 loads is float64 (the set is discontinuous in f: the header says why); outputs are rounded once.
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "common.h"

namespace {

constexpr int CSD_NW = 8;                 // waves (= voxels in flight) per workgroup
constexpr int CSD_MAXW = 6;               // ballot words of the set: nreg <= 384
constexpr int CSD_MAXSHELL = 256;         // shell frames a wave keeps in LDS
constexpr int CSD_LDS_LIMIT = 160 * 1024;

struct CsdArgs {
    const float *dwi;
    const uint8_t *mask;
    int64_t nvox;
    const int32_t *frames;                // [nshell] frame of every shell sample
    const float *X;                       // [nshell][n] row-major
    const float *Brow;                    // [nreg][NS] row-major, NS = n | 1
    const float *Yt;                      // [n][NRP] direction-major rows of the unscaled basis, NRP = nreg rounded up to 64
    const double *G0, *G1;                // [NP][NP]: X'X and X'X + B'B, zero-padded to NP = 8 NB
    const double *M0;                     // [n0][n0]: inverse of the leading block of X'X
    double thrc;                          // tau * B[0,0]
    int nshell, nreg, nrp, n0, niter, complement;
    float *sh, *odf, *niter_out;
};

#include "csd_shared.inc"                 // wave helpers, the peak gather, the basis, the response quadrature, the host Cholesky

// NB: 8 x 8 blocks of P's rows / columns (n <= 8 NB); BLDS: B in LDS
template <int N, bool BLDS>
__global__ __launch_bounds__(CSD_NW * 64) void csd_kernel(const CsdArgs A) {
    constexpr int NB = (N + 7) / 8, NS = N | 1, NP = 8 * NB, NT = N * (N + 1) / 2;
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int spad = (A.nshell + 63) & ~63;
    double *Pw = reinterpret_cast<double *>(smem) + (size_t)wave * (NT + 64);                 // the wave's triangle ..
    double *fw = Pw + NT;                                                                      // .. and its coefficients [64]
    float *sw = reinterpret_cast<float *>(reinterpret_cast<double *>(smem) + (size_t)CSD_NW * (NT + 64)) + (size_t)wave * spad;
    float *Bs = reinterpret_cast<float *>(reinterpret_cast<double *>(smem) + (size_t)CSD_NW * (NT + 64)) + (size_t)CSD_NW * spad;
    uint16_t *rc = reinterpret_cast<uint16_t *>(Bs + (BLDS ? (size_t)A.nreg * NS : 0));       // entry of the packing -> row | column << 8

    // once per workgroup: the entry table and B
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
        const int off = c * N - c * (c - 1) / 2;
        for (int r = c; r < N; r++) rc[off + r - c] = (uint16_t)(r | (c << 8));
    }
    if (BLDS) for (int i = threadIdx.x; i < A.nreg * NS; i += blockDim.x) Bs[i] = A.Brow[i];
    __syncthreads();
    const float *Bm = BLDS ? Bs : A.Brow;

    // the lane's rows and columns of P: (la + 8p, lb + 8q); a row or column past n reads element n - 1 and counts as 0
    const int la = lane & 7, lb = lane >> 3;
    const int npass = (A.nreg + 63) >> 6;

    for (int64_t vox = (int64_t)blockIdx.x * CSD_NW + wave; vox < A.nvox; vox += (int64_t)gridDim.x * CSD_NW) {
        // ---- samples of the shell; a voxel outside the mask or without a positive sample is all zeros ----
        bool pos = false;
        const bool inside = A.mask[vox] != 0;                                                  // wave-uniform
        if (inside)
            for (int i = lane; i < A.nshell; i += 64) {
                const float s = __builtin_nontemporal_load(A.dwi + (int64_t)A.frames[i] * A.nvox + vox);
                sw[i] = s;
                pos |= s > 0.0f;
            }
        const bool solve = __any(pos);
        double f = 0.0;                                                                        // lane k: coefficient k
        int nsolve = 0;
        if (solve) {
            wave_sync();
            // z = X's, lane j: element j
            double z = 0.0;
            if (lane < N)
                for (int i = 0; i < A.nshell; i++) z = __builtin_fma((double)A.X[i * N + lane], (double)sw[i], z);
            // f0 = M0 z[0 : n0]
            for (int c = 0; c < A.n0; c++) {
                const double zc = lane_bcast(z, c);
                if (lane < A.n0) f = __builtin_fma(A.M0[lane * A.n0 + c], zc, f);
            }
            const double thr = A.thrc * lane_bcast(f, 0);
            unsigned long long prev[CSD_MAXW];
#pragma unroll
            for (int c = 0; c < CSD_MAXW; c++) prev[c] = 0;
            for (int it = 0; it < A.niter; it++) {
                fw[lane] = f;
                wave_sync();
                // ---- a = B f and the set ----
                unsigned long long cur[CSD_MAXW];
                int count = 0;
#pragma unroll
                for (int c = 0; c < CSD_MAXW; c++) {
                    cur[c] = 0;
                    if (c < npass) {
                        const int i = c * 64 + lane;
                        const float *bi = Bm + (size_t)(i < A.nreg ? i : A.nreg - 1) * NS;
                        double a = 0.0;
#pragma unroll 5
                        for (int k = 0; k < N; k++) a = __builtin_fma((double)bi[k], fw[k], a);
                        cur[c] = __ballot(i < A.nreg && a < thr);
                        count += __popcll(cur[c]);
                    }
                }
                bool same = it > 0;
#pragma unroll
                for (int c = 0; c < CSD_MAXW; c++) same = same && cur[c] == prev[c];
                if (same) break;
#pragma unroll
                for (int c = 0; c < CSD_MAXW; c++) prev[c] = cur[c];

                // ---- P = X'X + sum over the set, or X'X + B'B - sum over the complement, in registers ----
                const bool neg = A.complement && 2 * count > A.nreg;
                const double *G = neg ? A.G1 : A.G0;
                double acc[NB][NB];
#pragma unroll
                for (int p = 0; p < NB; p++)
#pragma unroll
                    for (int q = 0; q <= p; q++) acc[p][q] = G[(la + 8 * p) * NP + lb + 8 * q];
#pragma unroll
                for (int c = 0; c < CSD_MAXW; c++) {
                    if (c >= npass) continue;
                    unsigned long long w = cur[c];
                    if (neg) {
                        const int left = A.nreg - 64 * c;
                        w = ~w & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
                    }
                    while (w) {
                        const int i = c * 64 + __builtin_ctzll(w);
                        w &= w - 1;
                        const float *bi = Bm + (size_t)i * NS;
                        double br[NB], bc[NB];
#pragma unroll
                        for (int p = 0; p < NB; p++) {
                            const int r = la + 8 * p, cc = lb + 8 * p;
                            const double vr = (double)bi[r < N ? r : N - 1], vc = (double)bi[cc < N ? cc : N - 1];
                            br[p] = r < N ? (neg ? -vr : vr) : 0.0;
                            bc[p] = cc < N ? vc : 0.0;
                        }
#pragma unroll
                        for (int p = 0; p < NB; p++)
#pragma unroll
                            for (int q = 0; q <= p; q++) acc[p][q] = __builtin_fma(br[p], bc[q], acc[p][q]);
                    }
                }
#pragma unroll
                for (int p = 0; p < NB; p++)
#pragma unroll
                    for (int q = 0; q <= p; q++) {
                        const int r = la + 8 * p, c = lb + 8 * q;
                        if (r < N && r >= c) Pw[c * N - c * (c - 1) / 2 + r - c] = acc[p][q];
                    }
                wave_sync();

                // ---- right-looking Cholesky on the column-packed triangle ----
                for (int j = 0; j < N; j++) {
                    const int oj = j * N - j * (j - 1) / 2;
                    const double piv = sqrt(Pw[oj]);
                    wave_sync();                                                               // every lane has read the diagonal
                    const int r = j + lane;
                    if (r < N) Pw[oj + lane] = lane == 0 ? piv : Pw[oj + lane] / piv;
                    wave_sync();
                    for (int e = oj + (N - j) + lane; e < NT; e += 64) {
                        const int ik = rc[e], i = ik & 255, k = ik >> 8;
                        Pw[e] = __builtin_fma(-Pw[oj + i - j], Pw[oj + k - j], Pw[e]);
                    }
                    wave_sync();
                }
                // ---- L y = z (columns), L' f = y (rows of L as columns of L') ----
                double y = z;
                for (int j = 0; j < N; j++) {
                    const int oj = j * N - j * (j - 1) / 2;
                    if (lane == j) y = y / Pw[oj];
                    const double yj = lane_bcast(y, j);
                    if (lane > j && lane < N) y = __builtin_fma(-Pw[oj + lane - j], yj, y);
                }
                for (int r = N - 1; r >= 0; r--) {
                    if (lane == r) y = y / Pw[r * N - r * (r - 1) / 2];
                    const double fr = lane_bcast(y, r);
                    if (lane < r) y = __builtin_fma(-Pw[lane * N - lane * (lane - 1) / 2 + r - lane], fr, y);
                }
                f = lane < N ? y : 0.0;
                nsolve++;
                wave_sync();                                                                   // the factor is read before the next build
            }
            fw[lane] = f;
            wave_sync();
        }
        // ---- outputs: rounded once ----
        if (lane < N) __builtin_nontemporal_store((float)f, A.sh + (int64_t)lane * A.nvox + vox);
        if (lane == 0) __builtin_nontemporal_store((float)nsolve, A.niter_out + vox);
        for (int i = lane; i < A.nreg; i += 64) {
            double v = 0.0;
            if (solve)
                for (int k = 0; k < N; k++) v = __builtin_fma((double)A.Yt[(size_t)k * A.nrp + i], fw[k], v);
            __builtin_nontemporal_store(v > 0.0 ? (float)v : 0.0f, A.odf + (int64_t)i * A.nvox + vox);
        }
        wave_sync();                                                                           // fw and sw are rewritten by the next voxel
    }
}

struct CsdDesign {
    int lmax = 0, n = 0, nshell = 0, nreg = 0, rank = 0;
    double bbar = 0.0;
    std::vector<int32_t> frames;
    double R[5] = {0, 0, 0, 0, 0};
    std::vector<double> X, B, Y;          // column-major [nshell x n], [nreg x n], [nreg x n], float64
};

int csd_design(const float *bval, const float *bvec, int nvol, const float *verts, int nverts, const fib_csd_params &pr, CsdDesign &d) {
    FIB_CHECK(pr.lmax == 2 || pr.lmax == 4 || pr.lmax == 6 || pr.lmax == 8, FIB_ERR_INVALID, "lmax must be 2, 4, 6 or 8, not %d", pr.lmax);
    FIB_CHECK(pr.lambda_para > 0.0f && pr.lambda_perp >= 0.0f && pr.lambda_para >= pr.lambda_perp && pr.s0 > 0.0f, FIB_ERR_INVALID,
              "the response needs lambda_para >= lambda_perp >= 0, lambda_para > 0 and s0 > 0");
    FIB_CHECK(pr.b0_thresh >= 0.0f && pr.b_tol >= 0.0f && pr.lambda >= 0.0f && pr.tau == pr.tau && pr.niter >= 1, FIB_ERR_INVALID,
              "b0_thresh, b_tol and lambda must not be negative, tau not NaN and niter at least 1");
    d.lmax = pr.lmax;
    d.n = (pr.lmax + 1) * (pr.lmax + 2) / 2;
    d.nreg = nverts / 2;
    float shell = pr.shell;
    if (!(shell > 0.0f)) { shell = bval[0]; for (int i = 1; i < nvol; i++) shell = std::max(shell, bval[i]); }
    d.frames.clear();
    double bsum = 0.0;
    for (int i = 0; i < nvol; i++)
        if (bval[i] > pr.b0_thresh && std::fabs(bval[i] - shell) <= pr.b_tol * shell) { d.frames.push_back(i); bsum += bval[i]; }
    d.nshell = (int)d.frames.size();
    FIB_CHECK(d.nshell >= d.n, FIB_ERR_INVALID, "CSD at lmax %d needs at least %d frames on the shell b = %g, the scheme has %d", pr.lmax, d.n,
              (double)shell, d.nshell);
    d.bbar = bsum / d.nshell;
    response_R(d.bbar, pr.lambda_para, pr.lambda_perp, pr.s0, pr.lmax, d.R);
    const int n = d.n;
    d.X.assign((size_t)d.nshell * n, 0.0);
    std::vector<double> row(n);
    for (int i = 0; i < d.nshell; i++) {
        const int fr = d.frames[i];
        sh_row(bvec[fr], bvec[fr + nvol], bvec[fr + 2 * (size_t)nvol], pr.lmax, row.data());
        for (int l = 0; l <= pr.lmax; l += 2)
            for (int m = -l; m <= l; m++) { const int c = l * (l + 1) / 2 + m; d.X[i + (size_t)d.nshell * c] = row[c] * d.R[l / 2]; }
    }
    d.B.assign((size_t)d.nreg * n, 0.0);
    d.Y.assign((size_t)d.nreg * n, 0.0);
    const double scale = (double)pr.lambda * d.R[0] * d.nshell / d.nreg;
    for (int v = 0; v < d.nreg; v++) {
        sh_row(verts[v], verts[v + nverts], verts[v + 2 * (size_t)nverts], pr.lmax, row.data());
        for (int c = 0; c < n; c++) { d.Y[v + (size_t)d.nreg * c] = row[c]; d.B[v + (size_t)d.nreg * c] = row[c] * scale; }
    }
    std::vector<double> pX((size_t)d.nshell * n);
    d.rank = fib::host_pinv(d.X.data(), d.nshell, n, pX.data());
    return FIB_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// design, plan
// ------------------------------------------------------------------------------------------
extern "C" int fib_csd_design(const float *bval, const float *bvec, int nvol, const float *verts, int nverts, const fib_csd_params *params,
                              int32_t *frames, int *nshell, float *R, float *X, float *B, float *Y, int *rank) try {
    if (rank) *rank = 0;
    if (nshell) *nshell = 0;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    FIB_CHECK(verts != nullptr && nverts >= 2 && nverts % 2 == 0, FIB_ERR_INVALID, "the ODF tessellation needs an even number of vertices");
    FIB_CHECK(params != nullptr, FIB_ERR_INVALID, "CSD needs its parameters (the response has no default)");
    CsdDesign d;
    // the frame list is reported before the count is judged: a caller that is refused can see what was selected
    const int rc = csd_design(bval, bvec, nvol, verts, nverts, *params, d);
    if (nshell) *nshell = d.nshell;
    if (frames) for (int i = 0; i < d.nshell; i++) frames[i] = d.frames[i];
    if (rc != FIB_OK) return rc;
    if (rank) *rank = d.rank;
    if (R) for (int l = 0; l <= d.lmax; l += 2) R[l / 2] = (float)d.R[l / 2];
    if (X) for (size_t i = 0; i < d.X.size(); i++) X[i] = (float)d.X[i];
    if (B) for (size_t i = 0; i < d.B.size(); i++) B[i] = (float)d.B[i];
    if (Y) for (size_t i = 0; i < d.Y.size(); i++) Y[i] = (float)d.Y[i];
    FIB_CHECK(d.rank == d.n, FIB_ERR_INVALID, "the shell's directions do not determine the %d harmonics of lmax %d (the kernel matrix has rank %d on %d frames)",
              d.n, d.lmax, d.rank, d.nshell);
    return FIB_OK;
} FIB_API_CATCH

struct fib_csd_plan {
    int device = 0;
    int lmax = 0, n = 0, nshell = 0, nreg = 0, nverts = 0, nrp = 0, n0 = 0, niter = 0, rank = 0;
    double thrc = 0.0;
    bool b_lds = true, complement = true;
    size_t smem = 0;
    std::vector<int32_t> frames_h;
    std::vector<float> R, X, B, Y;        // host copies, column-major, rounded
    fib::DevBuf<int32_t> frames;
    fib::DevBuf<float> Xd, Brow, Yt, verts;
    fib::DevBuf<double> G0, G1, M0;
    fib_odf_plan *peaks = nullptr;        // the folded neighbour table of the tessellation (fib::peaks_plan_create)
    mutable fib::DevBuf<int32_t> top, nvalid;   // the peak finder's results of the call in flight (grow-only)
    ~fib_csd_plan() { if (peaks) fib_odf_plan_destroy(peaks); }
};

namespace {
size_t csd_smem(int n, int nshell, int nreg, bool b_lds) {
    const size_t nt = (size_t)n * (n + 1) / 2, spad = (size_t)((nshell + 63) & ~63);
    return CSD_NW * (nt + 64) * sizeof(double) + CSD_NW * spad * sizeof(float) + (b_lds ? (size_t)nreg * (n | 1) * sizeof(float) : 0) +
           ((nt + 7) & ~(size_t)7) * sizeof(uint16_t);
}

template <int N>
int csd_launch(const fib_csd_plan *p, const CsdArgs &a, unsigned grid, hipStream_t st) {
    if (p->b_lds) {
        FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(csd_kernel<N, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->smem));
        hipLaunchKernelGGL((csd_kernel<N, true>), dim3(grid), dim3(CSD_NW * 64), p->smem, st, a);
    } else {
        FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(csd_kernel<N, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->smem));
        hipLaunchKernelGGL((csd_kernel<N, false>), dim3(grid), dim3(CSD_NW * 64), p->smem, st, a);
    }
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}
}  // namespace

extern "C" int fib_csd_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                                   const int32_t *faces, int nfaces, const fib_csd_params *params, fib_csd_plan **plan) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan output pointer is NULL");
    *plan = nullptr;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    FIB_CHECK(verts != nullptr && faces != nullptr && nverts >= 2 && nverts % 2 == 0 && nfaces > 0, FIB_ERR_INVALID, "invalid ODF tessellation");
    FIB_CHECK(params != nullptr, FIB_ERR_INVALID, "CSD needs its parameters (the response has no default)");
    CsdDesign d;
    FIB_RC(csd_design(bval, bvec, nvol, verts, nverts, *params, d));
    FIB_CHECK(d.rank == d.n, FIB_ERR_INVALID, "the shell's directions do not determine the %d harmonics of lmax %d (the kernel matrix has rank %d on %d frames)",
              d.n, d.lmax, d.rank, d.nshell);
    FIB_CHECK(d.nshell <= CSD_MAXSHELL, FIB_ERR_UNSUPPORTED, "a shell of %d frames exceeds the supported %d", d.nshell, CSD_MAXSHELL);
    FIB_CHECK(d.nreg <= 64 * CSD_MAXW, FIB_ERR_UNSUPPORTED, "a tessellation of %d directions exceeds the supported %d", d.nreg, 64 * CSD_MAXW);
    fib::DeviceGuard guard;
    FIB_RC(fib::use_device(device));
    std::unique_ptr<fib_csd_plan> p(new fib_csd_plan());
    const int n = d.n, ns = n | 1, np = (n + 7) / 8 * 8;
    p->device = device; p->lmax = d.lmax; p->n = n; p->nshell = d.nshell; p->nreg = d.nreg; p->nverts = nverts; p->rank = d.rank;
    p->nrp = (d.nreg + 63) & ~63;
    p->n0 = std::min(n, 15);
    p->niter = params->niter;
    p->frames_h = d.frames;
    p->R.resize(d.lmax / 2 + 1);
    for (size_t i = 0; i < p->R.size(); i++) p->R[i] = (float)d.R[i];
    p->X.resize(d.X.size()); p->B.resize(d.B.size()); p->Y.resize(d.Y.size());
    for (size_t i = 0; i < d.X.size(); i++) p->X[i] = (float)d.X[i];
    for (size_t i = 0; i < d.B.size(); i++) { p->B[i] = (float)d.B[i]; p->Y[i] = (float)d.Y[i]; }
    p->thrc = (double)params->tau * (double)p->B[0];
    // the device images: from the ROUNDED tables, in float64 where the kernel sums in float64
    std::vector<float> Xr((size_t)d.nshell * n), Br((size_t)d.nreg * ns, 0.0f), Yt((size_t)n * p->nrp, 0.0f);
    for (int i = 0; i < d.nshell; i++) for (int c = 0; c < n; c++) Xr[(size_t)i * n + c] = p->X[i + (size_t)d.nshell * c];
    for (int v = 0; v < d.nreg; v++)
        for (int c = 0; c < n; c++) { Br[(size_t)v * ns + c] = p->B[v + (size_t)d.nreg * c]; Yt[(size_t)c * p->nrp + v] = p->Y[v + (size_t)d.nreg * c]; }
    std::vector<double> G0((size_t)np * np, 0.0), G1((size_t)np * np, 0.0), M0((size_t)p->n0 * p->n0);
    for (int r = 0; r < n; r++)
        for (int c = 0; c <= r; c++) {
            double xx = 0.0, bb = 0.0;
            for (int i = 0; i < d.nshell; i++) xx += (double)Xr[(size_t)i * n + r] * (double)Xr[(size_t)i * n + c];
            for (int v = 0; v < d.nreg; v++) bb += (double)Br[(size_t)v * ns + r] * (double)Br[(size_t)v * ns + c];
            G0[(size_t)r * np + c] = G0[(size_t)c * np + r] = xx;
            G1[(size_t)r * np + c] = G1[(size_t)c * np + r] = xx + bb;
        }
    for (int r = 0; r < p->n0; r++) for (int c = 0; c < p->n0; c++) M0[r + (size_t)p->n0 * c] = G0[(size_t)r * np + c];
    FIB_CHECK(host_spd_inverse(M0, p->n0), FIB_ERR_INVALID, "the kernel matrix of the low orders is not positive definite");
    // where B lives (profiles/csd/): in LDS at lmax 8 when the workgroup's budget holds it, 6 % faster than through the cache there; through
    // the cache below, 14 % faster at lmax 6, where two workgroups then share a CU (the A/B partner is built with -DFIB_CSD_B_GLOBAL)
    p->b_lds = n == 45 && csd_smem(n, d.nshell, d.nreg, true) <= (size_t)CSD_LDS_LIMIT;
#ifdef FIB_CSD_B_GLOBAL
    p->b_lds = false;
#endif
#ifdef FIB_CSD_ADD_ONLY
    p->complement = false;
#endif
    p->smem = csd_smem(n, d.nshell, d.nreg, p->b_lds);
    FIB_CHECK(p->smem <= (size_t)CSD_LDS_LIMIT, FIB_ERR_UNSUPPORTED, "the CSD workgroup does not fit the LDS");
    FIB_RC(fib::peaks_plan_create(device, verts, nverts, faces, nfaces, &p->peaks));
    FIB_RC(fib::upload(p->frames, d.frames));
    FIB_RC(fib::upload(p->Xd, Xr));
    FIB_RC(fib::upload(p->Brow, Br));
    FIB_RC(fib::upload(p->Yt, Yt));
    FIB_RC(fib::upload(p->verts, verts, (size_t)3 * nverts));
    FIB_RC(fib::upload(p->G0, G0));
    FIB_RC(fib::upload(p->G1, G1));
    FIB_RC(fib::upload(p->M0, M0));
    *plan = p.release();
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fib_csd_plan_destroy(fib_csd_plan *plan) try { fib::plan_destroy(plan); } FIB_API_CATCH_VOID

extern "C" int fib_csd_plan_tables(const fib_csd_plan *plan, int32_t *frames, int *nshell, float *R, float *X, float *B, float *Y) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan is NULL");
    if (nshell) *nshell = plan->nshell;
    if (frames) memcpy(frames, plan->frames_h.data(), plan->frames_h.size() * sizeof(int32_t));
    if (R) memcpy(R, plan->R.data(), plan->R.size() * sizeof(float));
    if (X) memcpy(X, plan->X.data(), plan->X.size() * sizeof(float));
    if (B) memcpy(B, plan->B.data(), plan->B.size() * sizeof(float));
    if (Y) memcpy(Y, plan->Y.data(), plan->Y.size() * sizeof(float));
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_csd_rec(const fib_csd_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox, const fib_csd_out *out, void *stream) try {
    FIB_CHECK(plan && dwi && mask && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(out->sh && out->odf && out->niter && out->peak[0] && out->peak[1] && out->peak[2] && out->f[0] && out->f[1] && out->f[2],
              FIB_ERR_INVALID, "NULL output volume");
    FIB_CHECK(nvox > 0, FIB_ERR_INVALID, "nvox must be positive");
    FIB_CHECK(nvox < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(plan->device));
    int rc = plan->top.ensure((size_t)3 * nvox);
    if (rc == FIB_OK) rc = plan->nvalid.ensure((size_t)nvox);
    if (rc != FIB_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    CsdArgs a{};
    a.dwi = dwi; a.mask = mask; a.nvox = nvox; a.frames = plan->frames.p; a.X = plan->Xd.p; a.Brow = plan->Brow.p; a.Yt = plan->Yt.p;
    a.G0 = plan->G0.p; a.G1 = plan->G1.p; a.M0 = plan->M0.p; a.thrc = plan->thrc;
    a.nshell = plan->nshell; a.nreg = plan->nreg; a.nrp = plan->nrp; a.n0 = plan->n0; a.niter = plan->niter; a.complement = plan->complement ? 1 : 0;
    a.sh = out->sh; a.odf = out->odf; a.niter_out = out->niter;
    {
        fib::ProfScope prof("csd_rec", st);
        int ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, plan->device);
        // one workgroup per CU with B in LDS (its fill is paid once), two without
        const unsigned grid = (unsigned)std::min<int64_t>(fib::cdiv(nvox, CSD_NW), (int64_t)ncu * (plan->b_lds ? 1 : 2));
        switch (plan->n) {
            case 6:  rc = csd_launch<6>(plan, a, grid, st); break;
            case 15: rc = csd_launch<15>(plan, a, grid, st); break;
            case 28: rc = csd_launch<28>(plan, a, grid, st); break;
            default: rc = csd_launch<45>(plan, a, grid, st); break;
        }
        if (rc != FIB_OK) return rc;
    }
    rc = fibd_find_peaks(plan->peaks, out->odf, nvox, plan->top.p, plan->nvalid.p, stream);
    if (rc != FIB_OK) return rc;
    hipLaunchKernelGGL(csd_peaks_kernel, dim3((unsigned)fib::cdiv(nvox, 256)), dim3(256), 0, st, out->odf, plan->top.p, plan->nvalid.p,
                       plan->verts.p, plan->nverts, plan->nreg, nvox, out->peak[0], out->peak[1], out->peak[2], out->f[0], out->f[1], out->f[2]);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
