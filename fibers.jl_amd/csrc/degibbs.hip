// degibbs.hip — Gibbs-ringing removal by local subvoxel shifts (include/fibers_hip.h "Gibbs-ringing removal").
//
// Two stages per batch of slices, everything float64, all intermediates in the caller's workspace:
//   (a) the filter: a[u][v] -> au (rings along u only) and av (rings along v only).  Four launches of one direct-DFT kernel, each a
//       product with a twiddle table along one axis: v forward (half spectrum: a is real), u forward with the weighting Gu, u inverse,
//       v inverse.  Lanes always run along the axis that is NOT transformed and that axis is contiguous in the stage's input, so every
//       load is coalesced; the transposition a stage needs happens in its (once per output) store.  av = a - au - the corner bin's term:
//       Gu + Gv = 1 in every bin but the one where 2p == nu and 2q == nv, where both are 0.
//   (b) the search: one kernel for both axes.  au lies as rows along u, av (stored transposed) as rows along v, so a workgroup reads
//       whole contiguous rows into LDS; a thread owns DG_TL consecutive samples of one row.  Per candidate j the circulant row D_j is
//       staged in LDS (doubled, so that no index wraps, and padded by one double per 8, so that lanes 8 samples apart hit different
//       banks), the shifted row is a register-blocked circulant product (8 new LDS reads of D and 8 of r per 64 FMAs), it goes to LDS
//       once for the differences of the neighbours, and only the running minimum, the pick and the three samples the output needs stay
//       in registers.  No J x n array goes to memory.  The pass along u writes its float64 result over its input rows; the pass along v
//       adds it, rounds once and scatters float32 (and j*) to the volume.
// Work is dealt by index: no workgroup waits for another.
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

#include "common.h"

namespace {

constexpr int DG_NMAX = FIB_DEGIBBS_MAX_SIZE;
constexpr int DG_TL = 8;                                   // consecutive samples of a row per thread (the search)
constexpr int DG_THREADS = 256;
constexpr int DG_KB = 4;                                   // outputs per thread along the transformed axis (the filter)
constexpr size_t DG_BATCH_BYTES = (size_t)64 << 20;        // the float64 planes of a batch of slices stay near this

// the slices of a call: in-plane sizes, slices per frame, element strides of u, v and the slice axis, voxels per frame
struct DgGeom {
    int nu, nv, ns;
    int64_t su, sv, ss, nvox;
    __host__ __device__ int64_t base(int64_t g) const { return (g / ns) * nvox + (g % ns) * ss; }     // slice g of the series
};

// ---- (a) the filter -----------------------------------------------------------------------------------------------------------------
struct DftArgs {
    const float *a;                                        // the series
    DgGeom g;
    int64_t slice0;                                        // the batch's first slice
    const double *tw, *cu, *cv;                            // (cos, sin) pairs of the stage's length; the weights
    const double *in_re, *in_im;                           // the stage's complex input [slice][t][x]
    double *out_re, *out_im;                               // its output (stage 4: xu, xv)
    double *corner;                                        // [slice]: A[nu/2][nv/2] where both sizes are even
};

// Stage S of the filter.  t: the summed index, x: the lane index, k: the output index along the transformed axis; nvh = nv / 2 + 1.
//   1: t = v, x = u, k = q < nvh   Bt[u][q] = sum_v a[u][v] W_nv^{qv}
//   2: t = u, x = q, k = p         C[p][q]  = Gu[p][q] sum_u Bt[u][q] W_nu^{pu}
//   3: t = p, x = q, k = u'        Ft[q][u'] = sum_p C[p][q] W_nu^{-pu'}
//   4: t = q, x = u', k = v'       au[u'][v'] = (1 / (nu nv)) sum_q w_q Re(Ft[q][u'] W_nv^{-qv'}), w = 1 at q = 0 and at the Nyquist bin, else 2
template <int S>
__global__ __launch_bounds__(DG_THREADS) void dg_dft_kernel(DftArgs A) {
    __shared__ __attribute__((aligned(16))) double tw_s[2 * DG_NMAX];
    const int nu = A.g.nu, nv = A.g.nv, nvh = nv / 2 + 1;
    const int n = (S == 1 || S == 4) ? nv : nu;            // the transformed length
    const int nt = S == 1 ? nv : (S == 4 ? nvh : nu);
    const int X = (S == 1 || S == 4) ? nu : nvh;
    const int nk = S == 1 ? nvh : (S == 4 ? nv : nu);
    for (int i = threadIdx.x; i < 2 * n; i += DG_THREADS) tw_s[i] = A.tw[i];
    __syncthreads();
    const int nkg = (nk + DG_KB - 1) / DG_KB;
    const int id = blockIdx.x * DG_THREADS + threadIdx.x;
    if (id >= X * nkg) return;
    const int x = id % X, k0 = (id / X) * DG_KB;
    const int sb = blockIdx.y;
    const int64_t plane = (int64_t)nu * nvh;               // complex elements of a slice between the stages
    int kk[DG_KB], idx[DG_KB];
    double re[DG_KB], im[DG_KB];
#pragma unroll
    for (int i = 0; i < DG_KB; i++) { kk[i] = k0 + i < nk ? k0 + i : 0; idx[i] = 0; re[i] = 0.0; im[i] = 0.0; }

    const float *af = nullptr;
    const double *pr = nullptr, *pi = nullptr;
    int64_t tstride;
    if (S == 1) { af = A.a + A.g.base(A.slice0 + sb) + x * A.g.su; tstride = A.g.sv; }
    else if (S == 2) { pr = A.in_re + sb * plane + x; pi = A.in_im + sb * plane + x; tstride = nvh; }
    else if (S == 3) { pr = A.in_re + sb * plane + x; pi = A.in_im + sb * plane + x; tstride = nvh; }
    else { pr = A.in_re + sb * plane + x; pi = A.in_im + sb * plane + x; tstride = nu; }

    for (int t = 0; t < nt; t++) {
        double vr, vi = 0.0;
        if (S == 1) vr = (double)af[t * tstride];
        else { vr = pr[t * tstride]; vi = pi[t * tstride]; }
        double w = 1.0;
        if (S == 4) { w = (t == 0 || 2 * t == nv) ? 1.0 : 2.0; vr *= w; vi *= w; }
#pragma unroll
        for (int i = 0; i < DG_KB; i++) {
            const double c = tw_s[2 * idx[i]], s = tw_s[2 * idx[i] + 1];
            if (S == 1) { re[i] += vr * c; im[i] -= vr * s; }
            else if (S == 2) { re[i] += vr * c + vi * s; im[i] += vi * c - vr * s; }
            else if (S == 3) { re[i] += vr * c - vi * s; im[i] += vi * c + vr * s; }
            else re[i] += vr * c - vi * s;
            idx[i] += kk[i];
            if (idx[i] >= n) idx[i] -= n;
        }
    }
#pragma unroll
    for (int i = 0; i < DG_KB; i++) {
        const int k = k0 + i;
        if (k >= nk) break;
        if (S == 1) {
            A.out_re[sb * plane + (int64_t)x * nvh + k] = re[i];
            A.out_im[sb * plane + (int64_t)x * nvh + k] = im[i];
        } else if (S == 2) {                               // k = p, x = q
            double gu;
            if (2 * k == nu && 2 * x == nv) { gu = 0.0; A.corner[sb] = re[i]; }
            else gu = A.cv[x] / (A.cu[k] + A.cv[x]);
            A.out_re[sb * plane + (int64_t)k * nvh + x] = re[i] * gu;
            A.out_im[sb * plane + (int64_t)k * nvh + x] = im[i] * gu;
        } else if (S == 3) {                               // k = u', x = q
            A.out_re[sb * plane + (int64_t)x * nu + k] = re[i];
            A.out_im[sb * plane + (int64_t)x * nu + k] = im[i];
        } else {                                           // k = v', x = u'
            const double scale = (double)nu * (double)nv, au = re[i] / scale;
            double av = (double)A.a[A.g.base(A.slice0 + sb) + x * A.g.su + k * A.g.sv] - au;
            if (nu % 2 == 0 && nv % 2 == 0) { const double ct = A.corner[sb] / scale; av -= ((x + k) & 1) ? -ct : ct; }
            const int64_t pl = (int64_t)nu * nv;
            A.out_re[sb * pl + (int64_t)k * nu + x] = au;  // xu[v'][u']: rows along u
            A.out_im[sb * pl + (int64_t)x * nv + k] = av;  // xv[u'][v']: rows along v
        }
    }
}

// ---- (b) the search -----------------------------------------------------------------------------------------------------------------
struct SearchArgs {
    double *rows;                                          // [nb * nrows][n]: the float64 rows (xu or xv)
    const double *D;                                       // [2K][n]
    int n, nrows, nb, K, minW, maxW;
    int items, rw;                                         // threads per row = ceil(n / DG_TL); rows per workgroup
    const double *add;                                     // NULL: the result goes back to `rows`; else [nb][n][nrows], what the other pass left
    float *out;                                            // with add: the volume
    int8_t *shift;                                         // j* or NULL
    DgGeom g;
    int64_t slice0, row_stride, l_stride;                  // where sample l of row `row` of a slice lies in the volume
};

// The total variation of a candidate row around the thread's DG_TL samples, against the running minimum.  CW = 3: the windows are the
// default 1 .. 3, known to the compiler (16 samples, 6 additions a sample); CW = 0: minW .. maxW as given, every w up to 6 predicated.
template <int CW>
__device__ __forceinline__ void dg_pick(const double *row, int n, int l0, int minW, int maxW, int j, double (&bt)[DG_TL], int (&bj)[DG_TL],
                                        double (&sm)[DG_TL][3]) {
    constexpr int MW = CW ? CW : 6, NE = DG_TL + 2 * (MW + 1);      // samples l0 - MW - 1 .. l0 + DG_TL + MW
    double e[NE];
    int idx = (l0 - MW - 1) % n;                           // (n may be as short as 5)
    if (idx < 0) idx += n;
#pragma unroll
    for (int k = 0; k < NE; k++) { e[k] = row[idx]; idx = idx + 1 == n ? 0 : idx + 1; }
    double d[NE - 1];
#pragma unroll
    for (int k = 0; k < NE - 1; k++) d[k] = fabs(e[k + 1] - e[k]);      // d[k] = d_j[l0 - MW - 1 + k]
#pragma unroll
    for (int i = 0; i < DG_TL; i++) {
        double L = 0.0, R = 0.0;
#pragma unroll
        for (int w = 1; w <= MW; w++)
            if (CW || (w >= minW && w <= maxW)) { L += d[i + MW - w]; R += d[i + MW + 1 + w]; }
        const double t = L < R ? L : R;
        if (j == 0 || t < bt[i]) { bt[i] = t; bj[i] = j; sm[i][0] = e[MW + i]; sm[i][1] = e[MW + 1 + i]; sm[i][2] = e[MW + 2 + i]; }
    }
}

// LDS_TABLE: D_j staged in LDS per candidate (the library); false: read through the cache from the table in memory, the A/B partner
// of the diagnostic build (FIBERS_DEGIBBS_TABLE=cache): the same sums in the same order, the same bits.
template <bool LDS_TABLE, int CW>
__global__ __launch_bounds__(DG_THREADS) void dg_search_kernel(SearchArgs A) {
    extern __shared__ __attribute__((aligned(16))) double dg_lds[];
    const int n = A.n, items = A.items, npad = items * DG_TL, rs = npad + 1;      // (an odd row stride: rows start in different banks)
    double *rbuf = dg_lds, *cbuf = rbuf + (size_t)A.rw * rs, *d2 = cbuf + (size_t)A.rw * rs;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * A.rw, total = (int64_t)A.nb * A.nrows;

    // the rows, zero-padded to whole items (a row past the end is zeros)
    for (int i = tid; i < A.rw * rs; i += DG_THREADS) {
        const int r = i / rs, m = i - r * rs;
        rbuf[i] = (row0 + r < total && m < n) ? A.rows[(row0 + r) * n + m] : 0.0;
    }
    const int rloc = tid / items, item = tid - rloc * items, l0 = item * DG_TL;
    const bool active = rloc < A.rw && row0 + rloc < total;
    const double *rb = rbuf + (size_t)(active ? rloc : 0) * rs;
    double *cb = cbuf + (size_t)(active ? rloc : 0) * rs;
    double bt[DG_TL], sm[DG_TL][3];
    int bj[DG_TL];
    __syncthreads();
    if (active) dg_pick<CW>(rb, n, l0, A.minW, A.maxW, 0, bt, bj, sm);

    for (int j = 1; j <= 2 * A.K; j++) {
        // D_j doubled: d2[pad(x)] = D_j[(x - npad) mod n], x in [0, 2 npad), pad(x) = x + x / 8
        const double *Dj = A.D + (size_t)(j - 1) * n;
        if (LDS_TABLE)
            for (int x = tid; x < 2 * npad; x += DG_THREADS) {
                int t = (x - npad) % n;
                if (t < 0) t += n;
                d2[x + (x >> 3)] = Dj[t];
            }
        __syncthreads();                                   // (also: every thread is through with cbuf of candidate j - 1)
        if (active) {
            double acc[DG_TL], v[2 * DG_TL - 1];           // v[k + 7] = D_j(l0 - m0 + k), k = -7 .. 7
#pragma unroll
            for (int i = 0; i < DG_TL; i++) acc[i] = 0.0;
            for (int mb = 0; mb < items; mb++) {
                const int q = item - mb + items;           // l0 - m0 + npad = 8 q, 1 <= q <= 2 items - 1
                if (mb > 0) {
#pragma unroll
                    for (int k = DG_TL - 2; k >= 0; k--) v[k + 8] = v[k];
                }
                if (LDS_TABLE) {
                    if (mb == 0) {
#pragma unroll
                        for (int k = 1; k < DG_TL; k++) v[k + 7] = d2[9 * q + k];
                    }
                    v[7] = d2[9 * q];
#pragma unroll
                    for (int k = -7; k < 0; k++) v[k + 7] = d2[9 * (q - 1) + k + 8];
                } else {
                    int idx = (l0 - mb * DG_TL - 7) % n;   // k = -7
                    if (idx < 0) idx += n;
                    const int kend = mb == 0 ? 2 * DG_TL - 1 : DG_TL;
#pragma unroll
                    for (int kk = 0; kk < 2 * DG_TL - 1; kk++)
                        if (kk < kend) { v[kk] = Dj[idx]; idx = idx + 1 == n ? 0 : idx + 1; }
                }
                double r8[DG_TL];
#pragma unroll
                for (int mm = 0; mm < DG_TL; mm++) r8[mm] = rb[mb * DG_TL + mm];
#pragma unroll
                for (int mm = 0; mm < DG_TL; mm++)
#pragma unroll
                    for (int i = 0; i < DG_TL; i++) acc[i] += r8[mm] * v[i - mm + 7];
            }
#pragma unroll
            for (int i = 0; i < DG_TL; i++) if (l0 + i < n) cb[l0 + i] = acc[i];
        }
        __syncthreads();
        if (active) dg_pick<CW>(cb, n, l0, A.minW, A.maxW, j, bt, bj, sm);
    }
    if (!active) return;

    const int64_t row = row0 + rloc;
    const int sb = (int)(row / A.nrows), rr = (int)(row - (int64_t)sb * A.nrows);
    const int64_t vbase = A.g.base(A.slice0 + sb) + rr * A.row_stride;
    const double J = (double)(2 * A.K + 1);
#pragma unroll
    for (int i = 0; i < DG_TL; i++) {
        const int l = l0 + i;
        if (l >= n) break;
        const double s = bj[i] <= A.K ? (double)bj[i] / J : -(double)(bj[i] - A.K) / J;
        const double val = s > 0.0 ? sm[i][1] * (1.0 - s) + sm[i][0] * s : sm[i][1] * (1.0 + s) - sm[i][2] * s;
        if (A.add) A.out[vbase + l * A.l_stride] = (float)(A.add[((int64_t)sb * n + l) * A.nrows + rr] + val);
        else A.rows[row * n + l] = val;
        if (A.shift) A.shift[vbase + l * A.l_stride] = (int8_t)bj[i];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
const fib_degibbs_params DG_DEFAULT = FIB_DEGIBBS_PARAMS_DEFAULT;

// the refusals every entry shares, and the geometry that follows
int dg_shape(int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, fib_degibbs_params *p, DgGeom *g) {
    *p = params ? *params : DG_DEFAULT;
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && nvol > 0, FIB_ERR_INVALID, "dwi_degibbs: nx, ny, nz and the number of frames must be positive");
    FIB_CHECK(p->slice_axis >= 0 && p->slice_axis <= 2, FIB_ERR_INVALID, "dwi_degibbs: slice_axis must be 0, 1 or 2, not %d", p->slice_axis);
    FIB_CHECK(p->nshifts >= 1 && p->nshifts <= 32, FIB_ERR_INVALID, "dwi_degibbs: nshifts must lie in 1 .. 32, not %d", p->nshifts);
    FIB_CHECK(1 <= p->minW && p->minW <= p->maxW && p->maxW <= 6, FIB_ERR_INVALID, "dwi_degibbs: the windows must satisfy 1 <= minW <= maxW <= 6, not %d, %d",
              p->minW, p->maxW);
    const int64_t sx = 1, sy = nx, sz = (int64_t)nx * ny;
    if (p->slice_axis == 2) *g = DgGeom{nx, ny, nz, sx, sy, sz, 0};
    else if (p->slice_axis == 1) *g = DgGeom{nx, nz, ny, sx, sz, sy, 0};
    else *g = DgGeom{ny, nz, nx, sy, sz, sx, 0};
    g->nvox = (int64_t)nx * ny * nz;
    const int need = 2 * p->maxW + 3;
    FIB_CHECK(g->nu >= need && g->nv >= need, FIB_ERR_INVALID, "dwi_degibbs: the in-plane sizes (%d x %d) must be at least 2 maxW + 3 = %d", g->nu, g->nv, need);
    FIB_CHECK(g->nu <= DG_NMAX && g->nv <= DG_NMAX, FIB_ERR_UNSUPPORTED, "dwi_degibbs: the in-plane sizes (%d x %d) exceed the limit of %d", g->nu, g->nv, DG_NMAX);
    return FIB_OK;
}

// the workspace: the tables, then the planes of a batch of nb slices (byte offsets; everything is float64)
struct DgLayout {
    int nb;
    size_t tw_u, tw_v, cu, cv, du, dv, corner, b_re, b_im, c_re, c_im, xu, xv, total;
};
DgLayout dg_layout(const DgGeom &g, int K, int nvol) {
    DgLayout L;
    const size_t nu = g.nu, nv = g.nv, nvh = nv / 2 + 1, cplx = nu * nvh, pl = nu * nv;
    const size_t per_slice = 8 * (4 * cplx + 2 * pl + 1);
    const int64_t slices = (int64_t)nvol * g.ns;
    L.nb = (int)std::max<int64_t>(1, std::min<int64_t>({slices, (int64_t)(DG_BATCH_BYTES / per_slice), (int64_t)32768}));   // (a grid dimension)
    size_t o = 0;
    auto take = [&](size_t doubles) { const size_t at = o; o += 8 * doubles; return at; };
    L.tw_u = take(2 * nu); L.tw_v = take(2 * nv); L.cu = take(nu); L.cv = take(nv);
    L.du = take(2 * K * nu); L.dv = take(2 * K * nv);
    L.corner = take(L.nb);
    L.b_re = take(L.nb * cplx); L.b_im = take(L.nb * cplx); L.c_re = take(L.nb * cplx); L.c_im = take(L.nb * cplx);
    L.xu = take(L.nb * pl); L.xv = take(L.nb * pl);
    L.total = o;
    return L;
}

// The host tables of a row length and a number of shifts, built once per process (setup.cpp builds them).  Entries are never freed:
// a pointer handed to an asynchronous copy stays valid, and a process meets few (n, K) pairs.
struct DgTables { std::vector<double> tw, c, D; };
const DgTables &dg_tables(int n, int K) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::unique_ptr<DgTables>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto &slot = cache[std::make_pair(n, K)];
    if (!slot) {
        std::unique_ptr<DgTables> t(new DgTables());
        t->tw.resize(2 * (size_t)n); t->c.resize(n); t->D.resize(2 * (size_t)K * n);
        fib::host_degibbs_twiddles(n, t->tw.data(), t->c.data());
        fib::host_degibbs_table(n, K, t->D.data());
        slot = std::move(t);
    }
    return *slot;
}

int dg_upload(char *work, size_t off, const std::vector<double> &v, hipStream_t st) {
    FIB_HIP(hipMemcpyAsync(work + off, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return FIB_OK;
}

template <int S>
int dg_dft(const DftArgs &a, int nb, hipStream_t st) {
    const DgGeom &g = a.g;
    const int nvh = g.nv / 2 + 1;
    const int X = (S == 1 || S == 4) ? g.nu : nvh, nk = S == 1 ? nvh : (S == 4 ? g.nv : g.nu);
    const int work = X * ((nk + DG_KB - 1) / DG_KB);
    hipLaunchKernelGGL(dg_dft_kernel<S>, dim3((work + DG_THREADS - 1) / DG_THREADS, nb), dim3(DG_THREADS), 0, st, a);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

int dg_search(SearchArgs a, hipStream_t st) {
    a.items = (a.n + DG_TL - 1) / DG_TL;
    a.rw = std::max(1, DG_THREADS / a.items);
    const int npad = a.items * DG_TL;
    const size_t lds = sizeof(double) * ((size_t)2 * a.rw * (npad + 1) + (size_t)2 * npad + 2 * a.items + 2);
    const int64_t total = (int64_t)a.nb * a.nrows;
    const char *e = fib::ab_env("FIBERS_DEGIBBS_TABLE");
    const bool cache = e && !strcmp(e, "cache"), w13 = a.minW == 1 && a.maxW == 3;
    auto kernel = cache ? (w13 ? dg_search_kernel<false, 3> : dg_search_kernel<false, 0>) : (w13 ? dg_search_kernel<true, 3> : dg_search_kernel<true, 0>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)fib::cdiv(total, a.rw)), dim3(DG_THREADS), lds, st, a);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

}  // namespace

extern "C" int fib_dwi_degibbs_check(int nx, int ny, int nz, int nvol, const fib_degibbs_params *params) try {
    fib_degibbs_params p;
    DgGeom g;
    return dg_shape(nx, ny, nz, nvol, params, &p, &g);
} FIB_API_CATCH

extern "C" int fibd_dwi_degibbs_work_size(int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    fib_degibbs_params p;
    DgGeom g;
    FIB_RC(dg_shape(nx, ny, nz, nvol, params, &p, &g));
    *bytes = dg_layout(g, p.nshifts, nvol).total;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_dwi_degibbs(const float *dwi, int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, float *out, int8_t *shift_u,
                                int8_t *shift_v, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(dwi && out && work, FIB_ERR_INVALID, "NULL argument");
    fib_degibbs_params p;
    DgGeom g;
    FIB_RC(dg_shape(nx, ny, nz, nvol, params, &p, &g));
    const size_t nbytes = sizeof(float) * (size_t)g.nvox * nvol;
    const uintptr_t ai = reinterpret_cast<uintptr_t>(dwi), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK(ai + nbytes <= ao || ao + nbytes <= ai, FIB_ERR_INVALID, "dwi_degibbs: dwi and out must not overlap (there is no in-place form)");
    const DgLayout L = dg_layout(g, p.nshifts, nvol);
    FIB_CHECK(work_bytes >= L.total, FIB_ERR_INVALID, "workspace of %zu bytes, %zu needed (fibd_dwi_degibbs_work_size)", work_bytes, L.total);
    FIB_CHECK(reinterpret_cast<uintptr_t>(work) % 8 == 0, FIB_ERR_INVALID, "the workspace must be 8-byte aligned");

    const hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(work);
    const DgTables &tu = dg_tables(g.nu, p.nshifts), &tv = dg_tables(g.nv, p.nshifts);
    FIB_RC(dg_upload(w, L.tw_u, tu.tw, st)); FIB_RC(dg_upload(w, L.cu, tu.c, st)); FIB_RC(dg_upload(w, L.du, tu.D, st));
    FIB_RC(dg_upload(w, L.tw_v, tv.tw, st)); FIB_RC(dg_upload(w, L.cv, tv.c, st)); FIB_RC(dg_upload(w, L.dv, tv.D, st));
    auto at = [&](size_t off) { return reinterpret_cast<double *>(w + off); };

    const int64_t slices = (int64_t)nvol * g.ns;
    for (int64_t s0 = 0; s0 < slices; s0 += L.nb) {
        const int nb = (int)std::min<int64_t>(L.nb, slices - s0);
        {
            fib::ProfScope prof("dwi_degibbs_filter", st);
            DftArgs a{dwi, g, s0, at(L.tw_v), at(L.cu), at(L.cv), nullptr, nullptr, at(L.b_re), at(L.b_im), at(L.corner)};
            FIB_RC(dg_dft<1>(a, nb, st));
            a.tw = at(L.tw_u); a.in_re = at(L.b_re); a.in_im = at(L.b_im); a.out_re = at(L.c_re); a.out_im = at(L.c_im);
            FIB_RC(dg_dft<2>(a, nb, st));
            a.in_re = at(L.c_re); a.in_im = at(L.c_im); a.out_re = at(L.b_re); a.out_im = at(L.b_im);
            FIB_RC(dg_dft<3>(a, nb, st));
            a.tw = at(L.tw_v); a.in_re = at(L.b_re); a.in_im = at(L.b_im); a.out_re = at(L.xu); a.out_im = at(L.xv);
            FIB_RC(dg_dft<4>(a, nb, st));
        }
        {
            fib::ProfScope prof("dwi_degibbs_search", st);
            SearchArgs a{at(L.xu), at(L.du), g.nu, g.nv, nb, p.nshifts, p.minW, p.maxW, 0, 0, nullptr, nullptr, shift_u, g, s0, g.sv, g.su};
            FIB_RC(dg_search(a, st));                       // along u: rows of xu, one per v
            SearchArgs b{at(L.xv), at(L.dv), g.nv, g.nu, nb, p.nshifts, p.minW, p.maxW, 0, 0, at(L.xu), out, shift_v, g, s0, g.su, g.sv};
            FIB_RC(dg_search(b, st));                       // along v: rows of xv, one per u; adds the first pass and rounds
        }
    }
    return FIB_OK;
} FIB_API_CATCH
