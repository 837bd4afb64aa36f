// msmt.hip — multi-shell multi-tissue constrained spherical deconvolution per voxel on gfx950 (not in the reference:
// include/fibers_hip.h "Multi-shell multi-tissue deconvolution" and DESIGN.md §5 are the definition).
//
//   unknowns: n_wm harmonics of the white-matter fODF, then niso isotropic fractions (GM, CSF); samples: EVERY frame of the series
//   f0 = argmin |X0 f - s|  (the WM columns of l <= 4 and the isotropic columns),   thr = tau B[0,0] f0[0] (WM rows), 0 (isotropic rows)
//   repeat:  a = B f;  set = {i : a_i < thr_i};  stop when the set repeats;  (X'X + sum_{i in set} b_i b_i') f = X's
//
// Design: csd_kernel's (csd.hip), one wave per voxel, on a different problem shape:
//   - n = n_wm + niso is a RUN-TIME count inside NB = ceil(n / 8) compile-time blocks (n = 45, 46, 47 share NB = 6, whose last block
//     holds 5 to 7 live rows): five instantiations serve the twelve (lmax, niso) pairs;
//   - the WM constraint rows are csd_kernel's: nreg ballot bits in six scalar words, rows of the set added to (or, where the set is the
//     larger side, the complement's subtracted from) the register-held lower triangle.  They touch the leading n_wm x n_wm block only;
//   - an isotropic constraint row is a unit vector: one bit of a seventh scalar and one addition to one diagonal entry when the
//     triangle is written to LDS.  It is never stored as a dense row;
//   - up to 512 sample rows per voxel sit in the wave's LDS; z = X's runs over all of them on n of 64 lanes as one chain of FMAs
//     (four independent chains were measured and gain nothing);
//   - the factor, the solves and the float64 arithmetic are csd_kernel's.
#include <algorithm>
#include <cmath>
#include <memory>
#include <numeric>
#include <string>

#include "common.h"

namespace {

constexpr int MS_NW = 8;                  // waves (= voxels in flight) per workgroup
constexpr int MS_MAXW = 6;                // ballot words of the WM rows of the set: nreg <= 384
constexpr int MS_MAXVOL = 512;            // frames a wave keeps in LDS
constexpr int MS_MAXSHELLS = 8;           // shells above b0_thresh
constexpr int MS_LDS_LIMIT = 160 * 1024;

struct MsmtArgs {
    const float *dwi;
    const uint8_t *mask;
    int64_t nvox;
    const float *X;                       // [nvol][n] row-major
    const float *Brow;                    // [nreg][ns] row-major, the WM columns of the WM rows, ns = n_wm | 1
    const float *Yt;                      // [n_wm][nrp] direction-major rows of the unscaled basis, nrp = nreg rounded up to 64
    const double *G0, *G1;                // [NP][NP]: X'X and X'X + B_wm'B_wm, zero-padded to NP = 8 NB
    const double *M0;                     // [n0][n0]: inverse of X'X on the columns of the initial fit
    double thrc;                          // tau * B[0,0]
    double biso0, biso1;                  // the one entry of each isotropic constraint row
    int nvol, nreg, nrp, n, nwm, niso, n0w, niter;
    float *sh, *iso0, *iso1, *odf, *niter_out;
};

#include "csd_shared.inc"                 // wave helpers, the peak gather, the basis, the response quadrature, the host Cholesky

// NB: 8 x 8 blocks of P's rows / columns (n <= 8 NB); BLDS: the WM rows of B in LDS
template <int NB, bool BLDS>
__global__ __launch_bounds__(MS_NW * 64) void msmt_kernel(const MsmtArgs A) {
    constexpr int NP = 8 * NB;
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = A.n, nwm = A.nwm, ns = nwm | 1, nt = n * (n + 1) / 2;
    const int spad = (A.nvol + 63) & ~63;
    double *Pw = reinterpret_cast<double *>(smem) + (size_t)wave * (nt + 64);                  // the wave's triangle ..
    double *fw = Pw + nt;                                                                      // .. and its coefficients [64]
    float *sw = reinterpret_cast<float *>(reinterpret_cast<double *>(smem) + (size_t)MS_NW * (nt + 64)) + (size_t)wave * spad;
    float *Bs = reinterpret_cast<float *>(reinterpret_cast<double *>(smem) + (size_t)MS_NW * (nt + 64)) + (size_t)MS_NW * spad;
    uint16_t *rc = reinterpret_cast<uint16_t *>(Bs + (BLDS ? (size_t)A.nreg * ns : 0));        // entry of the packing -> row | column << 8

    // once per workgroup: the entry table and B
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        const int off = c * n - c * (c - 1) / 2;
        for (int r = c; r < n; r++) rc[off + r - c] = (uint16_t)(r | (c << 8));
    }
    if (BLDS) for (int i = threadIdx.x; i < A.nreg * ns; i += blockDim.x) Bs[i] = A.Brow[i];
    __syncthreads();
    const float *Bm = BLDS ? Bs : A.Brow;

    // the lane's rows and columns of P: (la + 8p, lb + 8q); a WM row or column past n_wm reads element n_wm - 1 and counts as 0
    const int la = lane & 7, lb = lane >> 3;
    const int npass = (A.nreg + 63) >> 6;
    // the lane's row of the initial fit: the WM columns of l <= 4, then the isotropic columns
    const int n0 = A.n0w + A.niso;
    const int r0 = lane < A.n0w ? lane : (lane >= nwm && lane < n ? A.n0w + lane - nwm : -1);
    const double bq0 = A.biso0 * A.biso0, bq1 = A.biso1 * A.biso1;

    for (int64_t vox = (int64_t)blockIdx.x * MS_NW + wave; vox < A.nvox; vox += (int64_t)gridDim.x * MS_NW) {
        // ---- every sample of the series; a voxel outside the mask or without a positive sample is all zeros ----
        bool pos = false;
        const bool inside = A.mask[vox] != 0;                                                  // wave-uniform
        if (inside)
            for (int i = lane; i < A.nvol; i += 64) {
                const float s = __builtin_nontemporal_load(A.dwi + (int64_t)i * A.nvox + vox);
                sw[i] = s;
                pos |= s > 0.0f;
            }
        const bool solve = __any(pos);
        double f = 0.0;                                                                        // lane k: coefficient k
        int nsolve = 0;
        if (solve) {
            wave_sync();
            // z = X's, lane j: element j.  One chain of nvol dependent FMAs: four independent chains (the A/B partner,
            // -DFIB_MSMT_FOUR_CHAINS) measured no faster (profiles/msmt/): presumably the workgroup's other waves hide the latency
            double z = 0.0;
            if (lane < n) {
                const float *x = A.X + lane;
#ifdef FIB_MSMT_FOUR_CHAINS
                double z1 = 0.0, z2 = 0.0, z3 = 0.0;
                int i = 0;
                for (; i + 4 <= A.nvol; i += 4) {
                    z = __builtin_fma((double)x[(size_t)i * n], (double)sw[i], z);
                    z1 = __builtin_fma((double)x[(size_t)(i + 1) * n], (double)sw[i + 1], z1);
                    z2 = __builtin_fma((double)x[(size_t)(i + 2) * n], (double)sw[i + 2], z2);
                    z3 = __builtin_fma((double)x[(size_t)(i + 3) * n], (double)sw[i + 3], z3);
                }
                for (; i < A.nvol; i++) z = __builtin_fma((double)x[(size_t)i * n], (double)sw[i], z);
                z = (z + z1) + (z2 + z3);
#else
                for (int i = 0; i < A.nvol; i++) z = __builtin_fma((double)x[(size_t)i * n], (double)sw[i], z);
#endif
            }
            // f0 = M0 z[columns of the initial fit]
            for (int c = 0; c < n0; c++) {
                const int col = c < A.n0w ? c : nwm + c - A.n0w;
                const double zc = lane_bcast(z, col);
                if (r0 >= 0) f = __builtin_fma(A.M0[r0 * n0 + c], zc, f);
            }
            const double thr = A.thrc * lane_bcast(f, 0);
            unsigned long long prev[MS_MAXW];
            unsigned previso = 0;
#pragma unroll
            for (int c = 0; c < MS_MAXW; c++) prev[c] = 0;
            for (int it = 0; it < A.niter; it++) {
                fw[lane] = f;
                wave_sync();
                // ---- a = B f and the set: the WM rows, then the isotropic rows (a = b f_t against 0) ----
                unsigned long long cur[MS_MAXW];
                int count = 0;
#pragma unroll
                for (int c = 0; c < MS_MAXW; c++) {
                    cur[c] = 0;
                    if (c < npass) {
                        const int i = c * 64 + lane;
                        const float *bi = Bm + (size_t)(i < A.nreg ? i : A.nreg - 1) * ns;
                        double a = 0.0;
#pragma unroll 5
                        for (int k = 0; k < nwm; k++) a = __builtin_fma((double)bi[k], fw[k], a);
                        cur[c] = __ballot(i < A.nreg && a < thr);
                        count += __popcll(cur[c]);
                    }
                }
                unsigned curiso = 0;
                if (A.niso > 0 && A.biso0 * lane_bcast(f, nwm) < 0.0) curiso |= 1u;
                if (A.niso > 1 && A.biso1 * lane_bcast(f, nwm + 1) < 0.0) curiso |= 2u;
                bool same = it > 0 && curiso == previso;
#pragma unroll
                for (int c = 0; c < MS_MAXW; c++) same = same && cur[c] == prev[c];
                if (same) break;
#pragma unroll
                for (int c = 0; c < MS_MAXW; c++) prev[c] = cur[c];
                previso = curiso;

                // ---- P = X'X + sum over the set, or X'X + B_wm'B_wm - sum over the complement, in registers ----
                const bool neg = 2 * count > A.nreg;
                const double *G = neg ? A.G1 : A.G0;
                double acc[NB][NB];
#pragma unroll
                for (int p = 0; p < NB; p++)
#pragma unroll
                    for (int q = 0; q <= p; q++) acc[p][q] = G[(la + 8 * p) * NP + lb + 8 * q];
#pragma unroll
                for (int c = 0; c < MS_MAXW; c++) {
                    if (c >= npass) continue;
                    unsigned long long w = cur[c];
                    if (neg) {
                        const int left = A.nreg - 64 * c;
                        w = ~w & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
                    }
                    while (w) {
                        const int i = c * 64 + __builtin_ctzll(w);
                        w &= w - 1;
                        const float *bi = Bm + (size_t)i * ns;
                        double br[NB], bc[NB];
#pragma unroll
                        for (int p = 0; p < NB; p++) {
                            const int r = la + 8 * p, cc = lb + 8 * p;
                            const double vr = (double)bi[r < nwm ? r : nwm - 1], vc = (double)bi[cc < nwm ? cc : nwm - 1];
                            br[p] = r < nwm ? (neg ? -vr : vr) : 0.0;
                            bc[p] = cc < nwm ? vc : 0.0;
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
                        if (r < n && r >= c) {
                            double v = acc[p][q];
                            // an isotropic row of the set: b^2 on its own diagonal entry
                            if (r == c && r >= nwm && ((curiso >> (r - nwm)) & 1u)) v += r == nwm ? bq0 : bq1;
                            Pw[c * n - c * (c - 1) / 2 + r - c] = v;
                        }
                    }
                wave_sync();

                // ---- right-looking Cholesky on the column-packed triangle ----
                for (int j = 0; j < n; j++) {
                    const int oj = j * n - j * (j - 1) / 2;
                    const double piv = sqrt(Pw[oj]);
                    wave_sync();                                                               // every lane has read the diagonal
                    const int r = j + lane;
                    if (r < n) Pw[oj + lane] = lane == 0 ? piv : Pw[oj + lane] / piv;
                    wave_sync();
                    for (int e = oj + (n - j) + lane; e < nt; e += 64) {
                        const int ik = rc[e], i = ik & 255, k = ik >> 8;
                        Pw[e] = __builtin_fma(-Pw[oj + i - j], Pw[oj + k - j], Pw[e]);
                    }
                    wave_sync();
                }
                // ---- L y = z (columns), L' f = y (rows of L as columns of L') ----
                double y = z;
                for (int j = 0; j < n; j++) {
                    const int oj = j * n - j * (j - 1) / 2;
                    if (lane == j) y = y / Pw[oj];
                    const double yj = lane_bcast(y, j);
                    if (lane > j && lane < n) y = __builtin_fma(-Pw[oj + lane - j], yj, y);
                }
                for (int r = n - 1; r >= 0; r--) {
                    if (lane == r) y = y / Pw[r * n - r * (r - 1) / 2];
                    const double fr = lane_bcast(y, r);
                    if (lane < r) y = __builtin_fma(-Pw[lane * n - lane * (lane - 1) / 2 + r - lane], fr, y);
                }
                f = lane < n ? y : 0.0;
                nsolve++;
                wave_sync();                                                                   // the factor is read before the next build
            }
            fw[lane] = f;
            wave_sync();
        }
        // ---- outputs: rounded once ----
        if (lane < nwm) __builtin_nontemporal_store((float)f, A.sh + (int64_t)lane * A.nvox + vox);
        if (lane == nwm && A.niso > 0) __builtin_nontemporal_store((float)f, A.iso0 + vox);
        if (lane == nwm + 1 && A.niso > 1) __builtin_nontemporal_store((float)f, A.iso1 + vox);
        if (lane == 0) __builtin_nontemporal_store((float)nsolve, A.niter_out + vox);
        for (int i = lane; i < A.nreg; i += 64) {
            double v = 0.0;
            if (solve)
                for (int k = 0; k < nwm; k++) v = __builtin_fma((double)A.Yt[(size_t)k * A.nrp + i], fw[k], v);
            __builtin_nontemporal_store(v > 0.0 ? (float)v : 0.0f, A.odf + (int64_t)i * A.nvox + vox);
        }
        wave_sync();                                                                           // fw and sw are rewritten by the next voxel
    }
}

// ------------------------------------------------------------------------------------------
// host: the shells and the tables
// ------------------------------------------------------------------------------------------
struct MsmtDesign {
    int lmax = 0, nwm = 0, niso = 0, n = 0, nvol = 0, nreg = 0, nshells = 0, rank = 0;
    std::vector<int32_t> shell;           // [nvol]
    std::vector<double> bbar;             // [nshells]
    std::vector<double> X, B, Y;          // column-major [nvol x n], [(nreg + niso) x n], [nreg x n], float64
};

int msmt_check_params(const fib_msmt_params &pr) {
    FIB_CHECK(pr.lmax == 2 || pr.lmax == 4 || pr.lmax == 6 || pr.lmax == 8, FIB_ERR_INVALID, "lmax must be 2, 4, 6 or 8, not %d", pr.lmax);
    FIB_CHECK(pr.niso >= 0 && pr.niso <= 2, FIB_ERR_INVALID, "niso must be 0, 1 or 2, not %d", pr.niso);
    FIB_CHECK(pr.b0_thresh >= 0.0f && pr.b_tol >= 0.0f && pr.lambda >= 0.0f && pr.lambda_iso >= 0.0f && pr.tau == pr.tau && pr.niter >= 1,
              FIB_ERR_INVALID, "b0_thresh, b_tol, lambda and lambda_iso must not be negative, tau not NaN and niter at least 1");
    return FIB_OK;
}

// the shell of every frame, the shells' mean b; the refusals of the series itself
int msmt_shells(const float *bval, const float *bvec, int nvol, const fib_msmt_params &pr, MsmtDesign &d) {
    d.nvol = nvol;
    d.shell.assign(nvol, 0);
    std::vector<int> order;
    for (int i = 0; i < nvol; i++) if (bval[i] > pr.b0_thresh) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bval[a] < bval[b]; });
    int cur = 0;
    double first = 0.0;
    for (int i : order) {
        const double b = (double)bval[i];
        if (cur == 0 || !(b <= (1.0 + 2.0 * (double)pr.b_tol) * first)) { cur++; first = b; }
        d.shell[i] = cur;
    }
    d.nshells = cur + 1;
    d.bbar.assign(d.nshells, 0.0);
    std::vector<int> cnt(d.nshells, 0);
    for (int i = 0; i < nvol; i++) { d.bbar[d.shell[i]] += (double)bval[i]; cnt[d.shell[i]]++; }
    for (int s = 0; s < d.nshells; s++) if (cnt[s]) d.bbar[s] /= cnt[s];
    FIB_CHECK(cur <= MS_MAXSHELLS, FIB_ERR_UNSUPPORTED, "a series of %d shells above b = %g exceeds the supported %d", cur, (double)pr.b0_thresh, MS_MAXSHELLS);
    FIB_CHECK(nvol <= MS_MAXVOL, FIB_ERR_UNSUPPORTED, "a series of %d frames exceeds the supported %d", nvol, MS_MAXVOL);
    for (int i = 0; i < nvol; i++)
        FIB_CHECK(d.shell[i] == 0 || bvec[i] != 0.0f || bvec[i + nvol] != 0.0f || bvec[i + 2 * (size_t)nvol] != 0.0f, FIB_ERR_INVALID,
                  "frame %d (b = %g, shell %d) has a zero gradient direction", i, (double)bval[i], d.shell[i]);
    return FIB_OK;
}

int msmt_design(const float *bvec, const float *verts, int nverts, const fib_msmt_params &pr, const float *wm_R, const float *iso_r,
                int nshells_in, MsmtDesign &d) {
    const int nvol = d.nvol, nl = pr.lmax / 2 + 1;
    FIB_CHECK(nshells_in == d.nshells, FIB_ERR_INVALID, "the responses are given for %d shells, the series has %d (shell 0, b <= %g, included)",
              nshells_in, d.nshells, (double)pr.b0_thresh);
    FIB_CHECK(pr.niso == 0 || iso_r != nullptr, FIB_ERR_INVALID, "%d isotropic tissues need their response table", pr.niso);
    d.lmax = pr.lmax; d.niso = pr.niso;
    d.nwm = (pr.lmax + 1) * (pr.lmax + 2) / 2;
    d.n = d.nwm + d.niso;
    d.nreg = nverts / 2;
    const int n = d.n, nwm = d.nwm, nreg = d.nreg, nb = nreg + d.niso;
    FIB_CHECK(nvol >= n, FIB_ERR_INVALID, "lmax %d with %d isotropic tissues needs at least %d frames, the series has %d", pr.lmax, d.niso, n, nvol);
    d.X.assign((size_t)nvol * n, 0.0);
    std::vector<double> row(nwm);
    double sum_r0 = 0.0, sum_iso[2] = {0.0, 0.0};
    for (int i = 0; i < nvol; i++) {
        const int s = d.shell[i];
        const float *R = wm_R + (size_t)s * nl;
        if (s == 0) {                                                          // Y_00 R_0(0), whatever the bvec says
            sh_row(0.0, 0.0, 1.0, 0, row.data());
            d.X[i] = row[0] * (double)R[0];
        } else {
            sh_row(bvec[i], bvec[i + nvol], bvec[i + 2 * (size_t)nvol], pr.lmax, row.data());
            for (int l = 0; l <= pr.lmax; l += 2)
                for (int m = -l; m <= l; m++) { const int c = l * (l + 1) / 2 + m; d.X[i + (size_t)nvol * c] = row[c] * (double)R[l / 2]; }
        }
        sum_r0 += (double)R[0];
        for (int t = 0; t < d.niso; t++) {
            const double v = (double)iso_r[(size_t)t * d.nshells + s];
            d.X[i + (size_t)nvol * (nwm + t)] = v;
            sum_iso[t] += v;
        }
    }
    d.B.assign((size_t)nb * n, 0.0);
    d.Y.assign((size_t)nreg * n, 0.0);
    const double scale = (double)pr.lambda * sum_r0 / nreg;
    for (int v = 0; v < nreg; v++) {
        sh_row(verts[v], verts[v + nverts], verts[v + 2 * (size_t)nverts], pr.lmax, row.data());
        for (int c = 0; c < nwm; c++) { d.Y[v + (size_t)nreg * c] = row[c]; d.B[v + (size_t)nb * c] = row[c] * scale; }
    }
    for (int t = 0; t < d.niso; t++) d.B[nreg + t + (size_t)nb * (nwm + t)] = (double)pr.lambda_iso * sum_iso[t];
    std::vector<double> pX((size_t)nvol * n);
    d.rank = fib::host_pinv(d.X.data(), nvol, n, pX.data());
    return FIB_OK;
}

const char *const MS_RANK_MSG = "the series does not determine the %d unknowns of lmax %d with %d isotropic tissues (the kernel matrix has rank %d on %d frames "
                                "in %d shells; two isotropic tissues need three distinct shells, shell 0 counted)";

size_t msmt_smem(int n, int nwm, int nvol, int nreg, bool b_lds) {
    const size_t nt = (size_t)n * (n + 1) / 2, spad = (size_t)((nvol + 63) & ~63);
    return MS_NW * (nt + 64) * sizeof(double) + MS_NW * spad * sizeof(float) + (b_lds ? (size_t)nreg * (nwm | 1) * sizeof(float) : 0) +
           ((nt + 7) & ~(size_t)7) * sizeof(uint16_t);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// response, design, plan
// ------------------------------------------------------------------------------------------
extern "C" int fib_msmt_wm_response(float lambda_para, float lambda_perp, float s0, const double *bbar, int nshells, int lmax, float *R) try {
    FIB_CHECK(bbar != nullptr && R != nullptr && nshells >= 1, FIB_ERR_INVALID, "NULL argument or no shell");
    FIB_CHECK(lmax == 2 || lmax == 4 || lmax == 6 || lmax == 8, FIB_ERR_INVALID, "lmax must be 2, 4, 6 or 8, not %d", lmax);
    FIB_CHECK(lambda_para > 0.0f && lambda_perp >= 0.0f && lambda_para >= lambda_perp && s0 > 0.0f, FIB_ERR_INVALID,
              "the response needs lambda_para >= lambda_perp >= 0, lambda_para > 0 and s0 > 0");
    const int nl = lmax / 2 + 1;
    for (int s = 0; s < nshells; s++) {
        double Rd[5];
        response_R(bbar[s], lambda_para, lambda_perp, s0, lmax, Rd);
        for (int k = 0; k < nl; k++) R[(size_t)s * nl + k] = (float)Rd[k];
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_msmt_design(const float *bval, const float *bvec, int nvol, const float *verts, int nverts, const fib_msmt_params *params,
                               const float *wm_R, const float *iso_r, int nshells_in, int32_t *shell, int *nshells, double *bbar,
                               float *X, float *B, float *Y, int *rank) try {
    if (rank) *rank = 0;
    if (nshells) *nshells = 0;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    FIB_CHECK(params != nullptr, FIB_ERR_INVALID, "the deconvolution needs its parameters");
    FIB_RC(msmt_check_params(*params));
    MsmtDesign d;
    // the shells are reported before they are judged: a caller that is refused can see the walk
    int rc = msmt_shells(bval, bvec, nvol, *params, d);
    if (nshells) *nshells = d.nshells;
    if (shell) for (int i = 0; i < nvol; i++) shell[i] = d.shell[i];
    if (bbar) for (int s = 0; s < std::min(d.nshells, MS_MAXSHELLS + 1); s++) bbar[s] = d.bbar[s];
    if (rc != FIB_OK) return rc;
    if (wm_R == nullptr) return FIB_OK;                                        // the shell walk alone
    FIB_CHECK(verts != nullptr && nverts >= 2 && nverts % 2 == 0, FIB_ERR_INVALID, "the ODF tessellation needs an even number of vertices");
    FIB_RC(msmt_design(bvec, verts, nverts, *params, wm_R, iso_r, nshells_in, d));
    if (rank) *rank = d.rank;
    if (X) for (size_t i = 0; i < d.X.size(); i++) X[i] = (float)d.X[i];
    if (B) for (size_t i = 0; i < d.B.size(); i++) B[i] = (float)d.B[i];
    if (Y) for (size_t i = 0; i < d.Y.size(); i++) Y[i] = (float)d.Y[i];
    FIB_CHECK(d.rank == d.n, FIB_ERR_INVALID, MS_RANK_MSG, d.n, d.lmax, d.niso, d.rank, nvol, d.nshells);
    return FIB_OK;
} FIB_API_CATCH

struct fib_msmt_plan {
    int device = 0;
    int lmax = 0, n = 0, nwm = 0, niso = 0, nvol = 0, nreg = 0, nverts = 0, nrp = 0, n0w = 0, niter = 0, rank = 0, nshells = 0;
    double thrc = 0.0, biso[2] = {0.0, 0.0};
    bool b_lds = true;
    size_t smem = 0;
    std::vector<int32_t> shell_h;
    std::vector<double> bbar_h;
    std::vector<float> X, B, Y;           // host copies, column-major, rounded
    fib::DevBuf<float> Xd, Brow, Yt, verts;
    fib::DevBuf<double> G0, G1, M0;
    fib_odf_plan *peaks = nullptr;        // the folded neighbour table of the tessellation (fib::peaks_plan_create)
    mutable fib::DevBuf<int32_t> top, nvalid;   // the peak finder's results of the call in flight (grow-only)
    ~fib_msmt_plan() { if (peaks) fib_odf_plan_destroy(peaks); }
};

namespace {
template <int NB>
int msmt_launch(const fib_msmt_plan *p, const MsmtArgs &a, unsigned grid, hipStream_t st) {
    if (p->b_lds) {
        FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(msmt_kernel<NB, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->smem));
        hipLaunchKernelGGL((msmt_kernel<NB, true>), dim3(grid), dim3(MS_NW * 64), p->smem, st, a);
    } else {
        FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(msmt_kernel<NB, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->smem));
        hipLaunchKernelGGL((msmt_kernel<NB, false>), dim3(grid), dim3(MS_NW * 64), p->smem, st, a);
    }
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}
}  // namespace

extern "C" int fib_msmt_plan_create(int device, const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                                    const int32_t *faces, int nfaces, const fib_msmt_params *params, const float *wm_R, const float *iso_r,
                                    int nshells_in, fib_msmt_plan **plan) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan output pointer is NULL");
    *plan = nullptr;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    FIB_CHECK(verts != nullptr && faces != nullptr && nverts >= 2 && nverts % 2 == 0 && nfaces > 0, FIB_ERR_INVALID, "invalid ODF tessellation");
    FIB_CHECK(params != nullptr && wm_R != nullptr, FIB_ERR_INVALID, "the deconvolution needs its parameters and the white-matter response table");
    FIB_RC(msmt_check_params(*params));
    MsmtDesign d;
    FIB_RC(msmt_shells(bval, bvec, nvol, *params, d));
    FIB_RC(msmt_design(bvec, verts, nverts, *params, wm_R, iso_r, nshells_in, d));
    FIB_CHECK(d.rank == d.n, FIB_ERR_INVALID, MS_RANK_MSG, d.n, d.lmax, d.niso, d.rank, nvol, d.nshells);
    FIB_CHECK(d.nreg <= 64 * MS_MAXW, FIB_ERR_UNSUPPORTED, "a tessellation of %d directions exceeds the supported %d", d.nreg, 64 * MS_MAXW);
    fib::DeviceGuard guard;
    FIB_RC(fib::use_device(device));
    std::unique_ptr<fib_msmt_plan> p(new fib_msmt_plan());
    const int n = d.n, nwm = d.nwm, ns = nwm | 1, np = (n + 7) / 8 * 8, nreg = d.nreg, nb = nreg + d.niso;
    p->device = device; p->lmax = d.lmax; p->n = n; p->nwm = nwm; p->niso = d.niso; p->nvol = nvol; p->nreg = nreg; p->nverts = nverts;
    p->rank = d.rank; p->nshells = d.nshells;
    p->nrp = (nreg + 63) & ~63;
    p->n0w = std::min(nwm, 15);
    p->niter = params->niter;
    p->shell_h = d.shell;
    p->bbar_h = d.bbar;
    p->X.resize(d.X.size()); p->B.resize(d.B.size()); p->Y.resize(d.Y.size());
    for (size_t i = 0; i < d.X.size(); i++) p->X[i] = (float)d.X[i];
    for (size_t i = 0; i < d.B.size(); i++) p->B[i] = (float)d.B[i];
    for (size_t i = 0; i < d.Y.size(); i++) p->Y[i] = (float)d.Y[i];
    p->thrc = (double)params->tau * (double)p->B[0];
    for (int t = 0; t < d.niso; t++) p->biso[t] = (double)p->B[nreg + t + (size_t)nb * (nwm + t)];
    // the device images: from the ROUNDED tables, in float64 where the kernel sums in float64
    std::vector<float> Xr((size_t)nvol * n), Br((size_t)nreg * ns, 0.0f), Yt((size_t)nwm * p->nrp, 0.0f);
    for (int i = 0; i < nvol; i++) for (int c = 0; c < n; c++) Xr[(size_t)i * n + c] = p->X[i + (size_t)nvol * c];
    for (int v = 0; v < nreg; v++)
        for (int c = 0; c < nwm; c++) { Br[(size_t)v * ns + c] = p->B[v + (size_t)nb * c]; Yt[(size_t)c * p->nrp + v] = p->Y[v + (size_t)nreg * c]; }
    const int n0 = p->n0w + d.niso;
    std::vector<double> G0((size_t)np * np, 0.0), G1((size_t)np * np, 0.0), M0((size_t)n0 * n0);
    for (int r = 0; r < n; r++)
        for (int c = 0; c <= r; c++) {
            double xx = 0.0, bb = 0.0;
            for (int i = 0; i < nvol; i++) xx += (double)Xr[(size_t)i * n + r] * (double)Xr[(size_t)i * n + c];
            if (r < nwm) for (int v = 0; v < nreg; v++) bb += (double)Br[(size_t)v * ns + r] * (double)Br[(size_t)v * ns + c];
            G0[(size_t)r * np + c] = G0[(size_t)c * np + r] = xx;
            G1[(size_t)r * np + c] = G1[(size_t)c * np + r] = xx + bb;
        }
    auto col0 = [&](int k) { return k < p->n0w ? k : nwm + k - p->n0w; };     // column k of the initial fit
    for (int r = 0; r < n0; r++) for (int c = 0; c < n0; c++) M0[r + (size_t)n0 * c] = G0[(size_t)col0(r) * np + col0(c)];
    FIB_CHECK(host_spd_inverse(M0, n0), FIB_ERR_INVALID, "the kernel matrix of the initial fit is not positive definite");
    // where the WM rows of B live (profiles/msmt/): in LDS at lmax 8, 25 % faster than through the cache on the headline volume (1082
    // against 1440 ms; the A/B partner is built with -DFIB_MSMT_B_GLOBAL), at every frame count: the largest workgroup (n = 47, 512
    // frames, 364 directions) is 160 448 B.  Below lmax 8 csd_kernel's measured rule is kept (profiles/csd/): through the cache.
    p->b_lds = nwm == 45 && msmt_smem(n, nwm, nvol, nreg, true) <= (size_t)MS_LDS_LIMIT;
#ifdef FIB_MSMT_B_GLOBAL
    p->b_lds = false;
#endif
    p->smem = msmt_smem(n, nwm, nvol, nreg, p->b_lds);
    FIB_CHECK(p->smem <= (size_t)MS_LDS_LIMIT, FIB_ERR_UNSUPPORTED, "the workgroup does not fit the LDS");
    FIB_RC(fib::peaks_plan_create(device, verts, nverts, faces, nfaces, &p->peaks));
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

extern "C" void fib_msmt_plan_destroy(fib_msmt_plan *plan) try { fib::plan_destroy(plan); } FIB_API_CATCH_VOID

extern "C" int fib_msmt_plan_tables(const fib_msmt_plan *plan, int32_t *shell, int *nshells, double *bbar, float *X, float *B, float *Y) try {
    FIB_CHECK(plan != nullptr, FIB_ERR_INVALID, "plan is NULL");
    if (nshells) *nshells = plan->nshells;
    if (shell) memcpy(shell, plan->shell_h.data(), plan->shell_h.size() * sizeof(int32_t));
    if (bbar) memcpy(bbar, plan->bbar_h.data(), plan->bbar_h.size() * sizeof(double));
    if (X) memcpy(X, plan->X.data(), plan->X.size() * sizeof(float));
    if (B) memcpy(B, plan->B.data(), plan->B.size() * sizeof(float));
    if (Y) memcpy(Y, plan->Y.data(), plan->Y.size() * sizeof(float));
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_msmt_rec(const fib_msmt_plan *plan, const float *dwi, const uint8_t *mask, int64_t nvox, const fib_msmt_out *out, void *stream) try {
    FIB_CHECK(plan && dwi && mask && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(out->sh && out->odf && out->niter && out->peak[0] && out->peak[1] && out->peak[2] && out->f[0] && out->f[1] && out->f[2],
              FIB_ERR_INVALID, "NULL output volume");
    for (int t = 0; t < plan->niso; t++) FIB_CHECK(out->iso[t] != nullptr, FIB_ERR_INVALID, "NULL output volume of isotropic tissue %d", t);
    FIB_CHECK(nvox > 0, FIB_ERR_INVALID, "nvox must be positive");
    FIB_CHECK(nvox < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(plan->device));
    int rc = plan->top.ensure((size_t)3 * nvox);
    if (rc == FIB_OK) rc = plan->nvalid.ensure((size_t)nvox);
    if (rc != FIB_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    MsmtArgs a{};
    a.dwi = dwi; a.mask = mask; a.nvox = nvox; a.X = plan->Xd.p; a.Brow = plan->Brow.p; a.Yt = plan->Yt.p;
    a.G0 = plan->G0.p; a.G1 = plan->G1.p; a.M0 = plan->M0.p; a.thrc = plan->thrc; a.biso0 = plan->biso[0]; a.biso1 = plan->biso[1];
    a.nvol = plan->nvol; a.nreg = plan->nreg; a.nrp = plan->nrp; a.n = plan->n; a.nwm = plan->nwm; a.niso = plan->niso; a.n0w = plan->n0w;
    a.niter = plan->niter;
    a.sh = out->sh; a.iso0 = out->iso[0]; a.iso1 = out->iso[1]; a.odf = out->odf; a.niter_out = out->niter;
    {
        fib::ProfScope prof("msmt_rec", st);
        int ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, plan->device);
        // one workgroup per CU with B in LDS (its fill is paid once), two without; the voxels are walked with the grid's stride
        const unsigned grid = (unsigned)std::min<int64_t>(fib::cdiv(nvox, MS_NW), (int64_t)ncu * (plan->b_lds ? 1 : 2));
        switch ((plan->n + 7) / 8) {
            case 1:  rc = msmt_launch<1>(plan, a, grid, st); break;
            case 2:  rc = msmt_launch<2>(plan, a, grid, st); break;
            case 3:  rc = msmt_launch<3>(plan, a, grid, st); break;
            case 4:  rc = msmt_launch<4>(plan, a, grid, st); break;
            default: rc = msmt_launch<6>(plan, a, grid, st); break;
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
