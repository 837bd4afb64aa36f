// denoise.hip — dwi_denoise: Marchenko-Pastur PCA denoising of a DWI series on gfx950 (not in the reference; the definition is
// include/fibers_hip.h "Marchenko-Pastur PCA denoising" and DESIGN.md §5).
//
// One workgroup per voxel, float64 throughout.  The Gram matrix G (r x r, r = min(P^3, N) <= 128) lives in LDS in packed symmetric
// form and is diagonalised by parallel cyclic Jacobi: an odd r gets one phantom index (zero row, never rotated) so that the n = r or
// r + 1 indices always form m = n / 2 disjoint pairs per step, in round-robin order, n - 1 steps a sweep.  A step is two phases:
//   A  thread k < m takes pair k's rotation from the three entries of its diagonal block, records tan(theta) in the workgroup's
//      scratch, and carries y = V' e_c (or V' x_c) through it;
//   B  every 2 x 2 block (rows of pair k) x (columns of pair l), k <= l, belongs to one thread, which applies both rotations to it in
//      registers: each stored entry is read and written once a step, and no barrier separates row from column rotations.
// The eigenvectors are never formed (a float64 V beside G does not fit LDS at r = 125, the 5^3 patch of a long series).  Only V V_kept'
// applied to one vector is wanted: after convergence the rule runs on the diagonal, the entries of y under the `cutoff` smallest
// eigenvalues are zeroed, and the recorded rotations are replayed backwards over y, a sweep at a time through the LDS that held G.
// Workgroups are persistent and take voxels by ticket, so the scratch is DN_MAXWG records of DN_SWEEPS sweeps whatever the volume.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int DN_RMAX = 128;         // largest Gram matrix
constexpr int DN_SWEEPS = 24;        // cap on sweeps; a voxel that reaches it is handed back unchanged with sigma = NaN, rank = -1
constexpr int DN_MAXWG = 512;        // persistent workgroups (two to a CU at r = 128)
constexpr int DN_TC = 16;            // contraction steps staged in LDS per pass of the Gram accumulation
constexpr int DN_THREADS = 512;      // largest workgroup
constexpr int DN_NB = 5;             // blocks a thread owns at most: ceil(64 * 65 / 2 / 512)
constexpr size_t DN_HEAD = 256;      // bytes in front of the rotation records: the ticket counter

struct DnArgs {
    const float *dwi;                // [N][nx * ny * nzin], planes [zin0, zin0 + nzin)
    const uint8_t *mask;             // [nx * ny * (z1 - z0)]
    float *out, *sigma, *rank;       // [N][nout], [nout], [nout]
    unsigned *ticket;
    double *rec;                     // [grid][DN_SWEEPS][n - 1][m] tan(theta)
    int nx, ny, nz, zin0, nzin, z0, z1, N, P, exp2;
    int M, r, n, m, q;               // P^3, min(M, N), r rounded up to even, n / 2, max(M, N)
};

__device__ __forceinline__ int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// packed index e -> (row i, column j <= i)
__device__ __forceinline__ void untri(int e, int &i, int &j) {
    i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > e) i--;
    while ((i + 1) * (i + 2) / 2 <= e) i++;
    j = e - i * (i + 1) / 2;
}

// pair k of step s of a sweep over n indices (n even): the circle method, index n - 1 stays put
__device__ __forceinline__ void pair_of(int s, int k, int n, int &p, int &q) {
    if (k == 0) { p = s; q = n - 1; return; }
    p = s + k;
    if (p >= n - 1) p -= n - 1;
    q = s - k;
    if (q < 0) q += n - 1;
}

__device__ __forceinline__ void cs_of(double t, double &c, double &s) {
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

__global__ void __launch_bounds__(DN_THREADS) dwi_denoise_kernel(const DnArgs a) {
    extern __shared__ __align__(16) double G[];            // packed lower triangle of n x n; later one sweep of rotation records
    __shared__ double y[DN_RMAX], lam[DN_RMAX], rt[DN_RMAX / 2];
    __shared__ double2 rcs[DN_RMAX / 2];                    // (cos, sin) of the step's rotations
    __shared__ float stage[DN_TC * DN_RMAX];
    __shared__ int step_rot[2];
    __shared__ int s_vox, s_cut;
    __shared__ double s_sig2;

    const int tid = threadIdx.x, nt = blockDim.x;
    const int nx = a.nx, ny = a.ny, P = a.P, N = a.N, M = a.M, r = a.r, n = a.n, m = a.m;
    const int64_t plane = (int64_t)nx * ny, nin = plane * a.nzin, nout = plane * (a.z1 - a.z0);
    const int ne = n * (n + 1) / 2, nblk = m * (m + 1) / 2;
    const bool wide = M <= N;                               // G = X X' over the patch's voxels; else X' X over the frames
    double *rec = a.rec + (size_t)blockIdx.x * DN_SWEEPS * (n - 1) * m;

    int kl[DN_NB];                                          // the thread's blocks: l << 8 | k, k <= l (fixed over the steps)
#pragma unroll
    for (int b = 0; b < DN_NB; b++) {
        const int e = tid + b * nt;
        int l = 0, k = 0;
        if (e < nblk) untri(e, l, k);
        kl[b] = l << 8 | k;
    }

    for (;;) {
        __syncthreads();                                    // (the last voxel's reads of the shared scalars are over)
        if (tid == 0) s_vox = (int)atomicAdd(a.ticket, 1u);
        __syncthreads();
        const int64_t vo = s_vox;
        if (vo >= nout) break;
        if (a.mask[vo] == 0) {
            for (int f = tid; f < N; f += nt) a.out[(int64_t)f * nout + vo] = 0.0f;
            if (tid == 0) { a.sigma[vo] = 0.0f; a.rank[vo] = 0.0f; }
            continue;
        }
        const int x = (int)(vo % nx), yy = (int)((vo / nx) % ny), z = (int)(vo / plane) + a.z0;
        const int h = P / 2;
        const int x0 = min(max(x - h, 0), nx - P), y0 = min(max(yy - h, 0), ny - P), z0p = min(max(z - h, 0), a.nz - P);
        const int crow = ((z - z0p) * P + (yy - y0)) * P + (x - x0);
        const float *base = a.dwi + ((int64_t)(z0p - a.zin0) * ny + y0) * nx + x0;     // the patch's first voxel, frame 0
        auto voxoff = [&](int i) -> int64_t { const int dx = i % P, dy = (i / P) % P, dz = i / (P * P); return ((int64_t)dz * ny + dy) * nx + dx; };

        // ---- G: float64 sums of float64 products, DN_TC contraction steps at a time through LDS ----
        for (int e = tid; e < ne; e += nt) G[e] = 0.0;
        const int T = wide ? N : M, nr = r * (r + 1) / 2;
        for (int t0 = 0; t0 < T; t0 += DN_TC) {
            const int tc = min(DN_TC, T - t0);
            __syncthreads();
            for (int id = tid; id < tc * r; id += nt) {
                const int c = id / r, u = id - c * r;
                const int vox = wide ? u : t0 + c, fr = wide ? t0 + c : u;
                stage[c * DN_RMAX + u] = base[(int64_t)fr * nin + voxoff(vox)];
            }
            __syncthreads();
            for (int e = tid; e < nr; e += nt) {
                int i, j;
                untri(e, i, j);
                double acc = 0.0;
                for (int c = 0; c < tc; c++) acc += (double)stage[c * DN_RMAX + i] * (double)stage[c * DN_RMAX + j];
                G[e] += acc;
            }
        }
        // y = V' e_c (wide) or V' x_c, V = the identity for now
        for (int i = tid; i < n; i += nt) y[i] = wide ? (i == crow ? 1.0 : 0.0) : (i < r ? (double)base[(int64_t)i * nin + voxoff(crow)] : 0.0);
        if (tid < 2) step_rot[tid] = 0;
        __syncthreads();

        // ---- parallel cyclic Jacobi ----
        int sweeps = -1;                                     // sweeps that rotated, once one has passed without a rotation
        for (int sw = 0; sw < DN_SWEEPS && sweeps < 0; sw++) {
            int rotated = 0;
            for (int s = 0; s < n - 1; s++) {
                const int par = (sw * (n - 1) + s) & 1;      // (n - 1 is odd: the flags alternate across sweeps too)
                if (tid < m) {                               // phase A
                    int p, q;
                    pair_of(s, tid, n, p, q);
                    const double app = G[tri(p, p)], aqq = G[tri(q, q)], apq = G[tri(p, q)];
                    double t = 0.0, c = 1.0, sn = 0.0;
                    if (fabs(apq) > 0x1p-52 * sqrt(fabs(app * aqq))) {
                        const double th = (aqq - app) / (2.0 * apq);
                        t = 1.0 / (fabs(th) + sqrt(th * th + 1.0));
                        if (th < 0.0) t = -t;
                        cs_of(t, c, sn);
                        step_rot[par] = 1;
                        const double yp = y[p], yq = y[q];
                        y[p] = c * yp - sn * yq;
                        y[q] = sn * yp + c * yq;
                    }
                    rcs[tid] = make_double2(c, sn);
                    rt[tid] = t;
                    rec[((size_t)sw * (n - 1) + s) * m + tid] = t;
                }
                if (tid == 0) step_rot[par ^ 1] = 0;
                __syncthreads();
                const int any = step_rot[par];
                rotated |= any;
                if (any) {                                   // phase B
#pragma unroll
                    for (int b = 0; b < DN_NB; b++) {
                        if (tid + b * nt < nblk) {
                            const int l = kl[b] >> 8, k = kl[b] & 255;
                            int pk, qk;
                            pair_of(s, k, n, pk, qk);
                            if (k == l) {
                                const int ipp = tri(pk, pk), iqq = tri(qk, qk), ipq = tri(pk, qk);
                                const double d = rt[k] * G[ipq];
                                G[ipp] -= d;
                                G[iqq] += d;
                                if (rt[k] != 0.0) G[ipq] = 0.0;
                            } else {
                                int pl, ql;
                                pair_of(s, l, n, pl, ql);
                                const int i00 = tri(pk, pl), i01 = tri(pk, ql), i10 = tri(qk, pl), i11 = tri(qk, ql);
                                const double2 rk = rcs[k], rl = rcs[l];
                                const double ck = rk.x, sk = rk.y, cl = rl.x, sl = rl.y;
                                const double b00 = G[i00], b01 = G[i01], b10 = G[i10], b11 = G[i11];
                                const double c00 = cl * b00 - sl * b01, c01 = sl * b00 + cl * b01;      // columns: B R_l
                                const double c10 = cl * b10 - sl * b11, c11 = sl * b10 + cl * b11;
                                G[i00] = ck * c00 - sk * c10; G[i01] = ck * c01 - sk * c11;              // rows: R_k' (B R_l)
                                G[i10] = sk * c00 + ck * c10; G[i11] = sk * c01 + ck * c11;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            if (!rotated) sweeps = sw;
        }

        const int64_t self = (int64_t)(z - a.zin0) * plane + (int64_t)yy * nx + x;
        if (sweeps < 0) {                                    // no convergence under the cap: the input row, marked
            for (int f = tid; f < N; f += nt) a.out[(int64_t)f * nout + vo] = a.dwi[(int64_t)f * nin + self];
            if (tid == 0) { a.sigma[vo] = nanf(""); a.rank[vo] = -1.0f; }
            continue;
        }

        // ---- eigenvalues in ascending order (ties: the lower index first), the rule, the projector ----
        int myrank = -1;
        if (tid < r) {
            const double d = G[tri(tid, tid)];
            myrank = 0;
            for (int j = 0; j < r; j++) {
                const double dj = G[tri(j, j)];
                myrank += (dj < d || (dj == d && j < tid)) ? 1 : 0;
            }
        }
        __syncthreads();                                     // G is free from here on
        if (tid < r) lam[myrank] = fmax(G[tri(tid, tid)], 0.0) / (double)a.q;
        __syncthreads();
        if (tid == 0) {
            double clam = 0.0, sig2 = 0.0;
            int cut = 0;
            for (int p = 0; p < r; p++) {
                clam += lam[p];
                const double gam = a.exp2 ? (double)(p + 1) / (double)(a.q - (r - p - 1)) : (double)(p + 1) / (double)a.q;
                const double s1 = clam / (double)(p + 1), s2 = (lam[p] - lam[0]) / (4.0 * sqrt(gam));
                if (s2 < s1) { sig2 = s1; cut = p + 1; }
            }
            s_cut = cut;
            s_sig2 = sig2;
        }
        __syncthreads();
        const int cut = s_cut;
        if (tid < r && myrank < cut) y[tid] = 0.0;
        // replay: y <- J_1 (J_2 ( ... J_last y)), a sweep's records at a time through the LDS that held G ((n - 1) m <= n (n + 1) / 2)
        for (int sw = sweeps - 1; sw >= 0 && cut > 0 && cut < r; sw--) {
            __syncthreads();
            for (int e = tid; e < (n - 1) * m; e += nt) G[e] = rec[(size_t)sw * (n - 1) * m + e];
            __syncthreads();
            for (int s = n - 2; s >= 0; s--) {
                if (tid < m) {
                    const double t = G[s * m + tid];
                    if (t != 0.0) {
                        int p, q;
                        pair_of(s, tid, n, p, q);
                        double c, sn;
                        cs_of(t, c, sn);
                        const double yp = y[p], yq = y[q];
                        y[p] = c * yp + sn * yq;
                        y[q] = c * yq - sn * yp;
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();
        // ---- the denoised row ----
        if (cut == 0) {
            for (int f = tid; f < N; f += nt) a.out[(int64_t)f * nout + vo] = a.dwi[(int64_t)f * nin + self];
        } else if (cut == r) {
            for (int f = tid; f < N; f += nt) a.out[(int64_t)f * nout + vo] = 0.0f;
        } else if (wide) {                                   // X' (E E' e_c): r-long dot products over the patch
            for (int f = tid; f < N; f += nt) {
                const float *col = base + (int64_t)f * nin;
                double acc = 0.0;
                int i = 0;
                for (int dz = 0; dz < P; dz++)
                    for (int dy = 0; dy < P; dy++) {
                        const float *row = col + ((int64_t)dz * ny + dy) * nx;
                        for (int dx = 0; dx < P; dx++, i++) acc += y[i] * (double)row[dx];
                    }
                a.out[(int64_t)f * nout + vo] = (float)acc;
            }
        } else {
            for (int f = tid; f < N; f += nt) a.out[(int64_t)f * nout + vo] = (float)y[f];
        }
        if (tid == 0) { a.sigma[vo] = (float)sqrt(s_sig2); a.rank[vo] = (float)(r - cut); }
    }
}

// the sizes that follow from (nvol, patch), after the refusals every entry shares
int dn_shape(int nx, int ny, int nz, int nvol, int patch, int *M, int *r, int *n) {
    FIB_CHECK(patch == 3 || patch == 5 || patch == 7, FIB_ERR_INVALID, "dwi_denoise: the patch edge must be 3, 5 or 7, not %d", patch);
    FIB_CHECK(nvol >= 2, FIB_ERR_INVALID, "dwi_denoise: at least 2 frames are needed, not %d", nvol);
    FIB_CHECK(nx >= patch && ny >= patch && nz >= patch, FIB_ERR_INVALID,
              "dwi_denoise: every dimension of the volume (%d x %d x %d) must be at least the patch edge %d", nx, ny, nz, patch);
    *M = patch * patch * patch;
    *r = std::min(*M, nvol);
    FIB_CHECK(*r <= DN_RMAX, FIB_ERR_UNSUPPORTED,
              "dwi_denoise: P = %d with N = %d frames needs a Gram matrix of %d rows; the limit is %d (P = 5 serves any N, P = 7 up to %d frames)",
              patch, nvol, *r, DN_RMAX, DN_RMAX);
    *n = (*r + 1) & ~1;
    return FIB_OK;
}

int dn_grid(int64_t nout) { return (int)std::min<int64_t>(nout, DN_MAXWG); }
size_t dn_work(int64_t nout, int n) { return DN_HEAD + (size_t)dn_grid(nout) * DN_SWEEPS * (n - 1) * (n / 2) * sizeof(double); }

}  // namespace

extern "C" int fib_dwi_denoise_check(int nx, int ny, int nz, int nvol, int patch, int estimator) try {
    int M, r, n;
    FIB_RC(dn_shape(nx, ny, nz, nvol, patch, &M, &r, &n));
    FIB_CHECK(estimator == FIB_DENOISE_EXP1 || estimator == FIB_DENOISE_EXP2, FIB_ERR_INVALID, "dwi_denoise: unknown estimator %d", estimator);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dwi_denoise_work_size(int nx, int ny, int nz, int nvol, int patch, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    FIB_CHECK(patch == 3 || patch == 5 || patch == 7, FIB_ERR_INVALID, "dwi_denoise: the patch edge must be 3, 5 or 7, not %d", patch);
    FIB_CHECK(nvol >= 2, FIB_ERR_INVALID, "dwi_denoise: at least 2 frames are needed, not %d", nvol);
    const int r = std::min(patch * patch * patch, nvol);
    FIB_CHECK(r <= DN_RMAX, FIB_ERR_UNSUPPORTED, "dwi_denoise: P = %d with N = %d frames needs a Gram matrix of %d rows; the limit is %d",
              patch, nvol, r, DN_RMAX);
    *bytes = dn_work((int64_t)nx * ny * nz, (r + 1) & ~1);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dwi_denoise(const float *dwi, int nx, int ny, int nz, int zin0, int nzin, int z0, int z1, int nvol, int patch,
                                int estimator, const uint8_t *mask, float *out, float *sigma, float *rank, void *work, size_t work_bytes,
                                void *stream) try {
    FIB_CHECK(dwi && mask && out && sigma && rank && work, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    FIB_RC(fib_dwi_denoise_check(nx, ny, nz, nvol, patch, estimator));
    FIB_CHECK(0 <= z0 && z0 < z1 && z1 <= nz, FIB_ERR_INVALID, "output planes [%d, %d) outside [0, %d)", z0, z1, nz);
    FIB_CHECK(0 <= zin0 && nzin > 0 && zin0 + nzin <= nz, FIB_ERR_INVALID, "input planes [%d, %d) outside [0, %d)", zin0, zin0 + nzin, nz);
    int M, r, n;
    FIB_RC(dn_shape(nx, ny, nz, nvol, patch, &M, &r, &n));
    // the clamp is taken against the whole volume: the patches of planes z0 and z1 - 1 bound what the slab must hold
    const int h = patch / 2, need0 = std::min(std::max(z0 - h, 0), nz - patch), need1 = std::min(std::max(z1 - 1 - h, 0), nz - patch) + patch;
    FIB_CHECK(need0 >= zin0 && need1 <= zin0 + nzin, FIB_ERR_INVALID,
              "dwi holds planes [%d, %d); outputs [%d, %d) need [%d, %d)", zin0, zin0 + nzin, z0, z1, need0, need1);
    const int64_t nout = (int64_t)nx * ny * (z1 - z0);
    FIB_CHECK(nout < ((int64_t)1 << 31) - DN_MAXWG, FIB_ERR_UNSUPPORTED, "dwi_denoise: %lld output voxels in one call; split the volume into z-slabs", (long long)nout);
    const size_t need = dn_work(nout, n);
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "workspace of %zu bytes, %zu needed (fibd_dwi_denoise_work_size)", work_bytes, need);
    FIB_CHECK(reinterpret_cast<uintptr_t>(work) % 8 == 0, FIB_ERR_INVALID, "the workspace must be 8-byte aligned");

    const hipStream_t st = (hipStream_t)stream;
    DnArgs a{dwi, mask, out, sigma, rank, (unsigned *)work, (double *)((char *)work + DN_HEAD),
             nx, ny, nz, zin0, nzin, z0, z1, nvol, patch, estimator == FIB_DENOISE_EXP2 ? 1 : 0,
             M, r, n, n / 2, std::max(M, nvol)};
    const int nblk = a.m * (a.m + 1) / 2;
    int threads = 64;                                      // no thread owns more than DN_NB blocks
    while (threads * DN_NB < nblk) threads *= 2;
    const size_t lds = sizeof(double) * n * (n + 1) / 2;
    FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dwi_denoise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FIB_HIP(hipMemsetAsync(work, 0, DN_HEAD, st));
    {
        fib::ProfScope prof("dwi_denoise", st);
        hipLaunchKernelGGL(dwi_denoise_kernel, dim3(dn_grid(nout)), dim3(threads), lds, st, a);
        FIB_HIP(hipGetLastError());
    }
    return FIB_OK;
} FIB_API_CATCH
