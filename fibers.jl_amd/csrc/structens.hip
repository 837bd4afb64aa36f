// structens.hip — st_recon (structens.jl:40-88): structure-tensor reconstruction of a scalar volume on gfx950.
//
//   image = G_sigma * vol                 (skipped when sigma <= 0)
//   g     = Scharr(image)                 ([-1 0 1]/2 along the derivative's axis, [3 10 3]/16 along the two others)
//   S     = G_rho * (g g^T)               (six products; the smoothing is skipped when rho <= 0)
//   eigen(Symmetric(S, :L)) per voxel     (sym3_eigen.inc, the solver st_eigen and the tensor fit use)
//
// Every filter is ImageFiltering's imfilter(..., "reflect"): correlation, the input mirrored about its edge voxel.
//
// Two launches per z-range of outputs:
//   K1 st_grad_kernel:   vol -> (gx, gy, gz) into the caller's workspace (12 B / voxel).  G_sigma of a mirrored volume is itself
//                        mirror-symmetric, so the Scharr stencil may read the smoothed image past a face by smoothing the mirrored
//                        volume there: K1 reads vol at reflected indices and never materialises the image.
//   K2 st_tensor_kernel: (gx, gy, gz) -> six products -> G_rho -> eigen -> eigvec / eigval (+ S when asked).  The products are formed
//                        from gradients read at reflected IN-RANGE indices: a gradient computed past a face has the opposite sign
//                        across it, so K2 cannot be fused with K1 the way K1 fuses the smoothing (the off-diagonal products would
//                        come out wrong within rho's radius of every face).
// Both kernels give a workgroup one x-y tile and march it along z: per input plane the x and y passes run in LDS, the z pass is a
// ring of 2R+1 accumulators in registers (the radius R is a template parameter, so the ring shifts by register renaming).  Each
// output's z sum starts from zero at its first contributing plane, so an output does not depend on where the march started:
// slabs of any thickness give bit-identical results.
#include "common.h"

#include <cmath>

// the eigen-solve must compile exactly as in dti.hip (fibd_st_eigen): no contraction of a*b+c anywhere in this file
#pragma clang fp contract(off)

namespace {

#include "sym3_eigen.inc"

constexpr int ST_RMAX = 16;                 // sigma, rho <= 8
constexpr int TX = 32, TY = 8;              // 256 threads: K1's region of smoothed columns (30 x 6 gradients), K2's output tile
constexpr int NT = TX * TY;

struct Taps { float w[ST_RMAX + 1]; };      // w[|d|], d in [-R, R]

// numpy.pad(mode="reflect"): mirror about the edge voxel, repeated while the index is still out of range; an axis of length 1 gives 0
__device__ __host__ __forceinline__ int refl(int i, int n) {
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

struct GradArgs {
    const float *vol; int nx, ny, nz, zin0;   // vol: planes [zin0, ...) of the nx*ny*nz volume
    float *g; int gz0, ngz;                   // gradients [3][ngz][ny][nx] of planes [gz0, gz0 + ngz)
    Taps t;
};

template <int R>
__global__ __launch_bounds__(NT) void st_grad_kernel(const GradArgs a) {
    constexpr int LW = TX + 2 * R, LH = TY + 2 * R;
    __shared__ float L[LH][LW];               // one plane of vol around the region
    __shared__ float X[LH][TX];               // after the x pass
    __shared__ float I[3][TY][TX];            // the last three smoothed planes (the Scharr stencil's z extent)
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int rx0 = blockIdx.x * (TX - 2) - 1, ry0 = blockIdx.y * (TY - 2) - 1;   // region origin: gradient tile minus 1
    const size_t plane = (size_t)a.nx * a.ny;
    float acc[2 * R + 1];
#pragma unroll
    for (int k = 0; k <= 2 * R; k++) acc[k] = 0.0f;

    const int pfirst = a.gz0 - 1 - R, plast = a.gz0 + a.ngz + R;
    for (int p = pfirst; p <= plast; p++) {
        const float *src = a.vol + (size_t)(refl(p, a.nz) - a.zin0) * plane;
        for (int e = tid; e < LH * LW; e += NT) {
            const int j = e / LW, i = e - j * LW;
            L[j][i] = src[(size_t)refl(ry0 - R + j, a.ny) * a.nx + refl(rx0 - R + i, a.nx)];
        }
        __syncthreads();
        for (int e = tid; e < LH * TX; e += NT) {
            const int j = e / TX, i = e - j * TX;
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k <= 2 * R; k++) s = fmaf(a.t.w[k < R ? R - k : k - R], L[j][i + k], s);
            X[j][i] = s;
        }
        __syncthreads();
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) v = fmaf(a.t.w[k < R ? R - k : k - R], X[ty + k][tx], v);
        // plane p contributes to smoothed planes p-R .. p+R (acc[0] .. acc[2R]); acc[0] is then complete
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) acc[k] = fmaf(a.t.w[k < R ? R - k : k - R], v, acc[k]);
        const int q = p - R;
        I[((q % 3) + 3) % 3][ty][tx] = acc[0];
#pragma unroll
        for (int k = 0; k < 2 * R; k++) acc[k] = acc[k + 1];
        acc[2 * R] = 0.0f;
        __syncthreads();
        const int c = q - 1;                  // the gradient plane whose three smoothed planes are now in I
        const int x = rx0 + tx, y = ry0 + ty;
        if (c >= a.gz0 && tx >= 1 && tx < TX - 1 && ty >= 1 && ty < TY - 1 && x < a.nx && y < a.ny) {
            float n[3][3][3];                 // n[dz][dy][dx]
#pragma unroll
            for (int dz = 0; dz < 3; dz++) {
                const int s = (((c - 1 + dz) % 3) + 3) % 3;
#pragma unroll
                for (int dy = 0; dy < 3; dy++)
#pragma unroll
                    for (int dx = 0; dx < 3; dx++) n[dz][dy][dx] = I[s][ty - 1 + dy][tx - 1 + dx];
            }
            const float sw[3] = {0.1875f, 0.625f, 0.1875f};   // [3 10 3] / 16
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
            for (int u = 0; u < 3; u++) {
                float hx = 0.0f, hy = 0.0f, hz = 0.0f;
#pragma unroll
                for (int w = 0; w < 3; w++) {
                    hx = fmaf(sw[w], n[u][w][2] - n[u][w][0], hx);    // u = dz, w = dy
                    hy = fmaf(sw[w], n[u][2][w] - n[u][0][w], hy);    // u = dz, w = dx
                    hz = fmaf(sw[w], n[2][u][w] - n[0][u][w], hz);    // u = dy, w = dx
                }
                gx = fmaf(sw[u], hx, gx);
                gy = fmaf(sw[u], hy, gy);
                gz = fmaf(sw[u], hz, gz);
            }
            const size_t o = (size_t)(c - a.gz0) * plane + (size_t)y * a.nx + x, gs = (size_t)a.ngz * plane;
            a.g[o] = 0.5f * gx;
            a.g[o + gs] = 0.5f * gy;
            a.g[o + 2 * gs] = 0.5f * gz;
        }
    }
}

struct TensorArgs {
    const float *g; int nx, ny, nz, gz0, ngz;  // gradients as GradArgs wrote them
    float *eigvec, *eigval; int z0, z1;        // output planes [z0, z1): eigvec [9][nout], eigval [3][nout]
    float *S[6];                               // NULL or the smoothed tensor [6][nout]
    Taps t;
};

template <int R>
__global__ __launch_bounds__(NT) void st_tensor_kernel(const TensorArgs a) {
    constexpr int LW = TX + 2 * R, LH = TY + 2 * R;
    // R <= 8: the six products are formed once per loaded element and the x pass reads them (46 KB of LDS at R = 8); above, the
    // plane of products would not fit beside X, so the three gradients are kept and the x pass forms the products at every tap.
    // Either way each product is the same f32 multiply, so the results do not depend on the choice.
    constexpr bool PRE = R <= 8;
    __shared__ float G[PRE ? 6 : 3][LH][LW];  // one plane of products (PRE) or gradients around the tile
    __shared__ float X[6][LH][TX];            // products after the x pass
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int bx0 = blockIdx.x * TX, by0 = blockIdx.y * TY;
    const int x = bx0 + tx, y = by0 + ty;
    const size_t plane = (size_t)a.nx * a.ny, gs = (size_t)a.ngz * plane, nout = (size_t)(a.z1 - a.z0) * plane;
    float acc[2 * R + 1][6];
#pragma unroll
    for (int k = 0; k <= 2 * R; k++)
#pragma unroll
        for (int c = 0; c < 6; c++) acc[k][c] = 0.0f;

    for (int p = a.z0 - R; p < a.z1 + R; p++) {
        const float *src = a.g + (size_t)(refl(p, a.nz) - a.gz0) * plane;
        for (int e = tid; e < LH * LW; e += NT) {
            const int j = e / LW, i = e - j * LW;
            const size_t off = (size_t)refl(by0 - R + j, a.ny) * a.nx + refl(bx0 - R + i, a.nx);
            const float gx = src[off], gy = src[off + gs], gz = src[off + 2 * gs];
            if constexpr (PRE) {
                G[0][j][i] = gx * gx; G[1][j][i] = gx * gy; G[2][j][i] = gx * gz;
                G[3][j][i] = gy * gy; G[4][j][i] = gy * gz; G[5][j][i] = gz * gz;
            } else {
                G[0][j][i] = gx; G[1][j][i] = gy; G[2][j][i] = gz;
            }
        }
        __syncthreads();
        for (int e = tid; e < LH * TX; e += NT) {
            const int j = e / TX, i = e - j * TX;
            float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k <= 2 * R; k++) {
                const float w = a.t.w[k < R ? R - k : k - R];
                if constexpr (PRE) {
#pragma unroll
                    for (int c = 0; c < 6; c++) s[c] = fmaf(w, G[c][j][i + k], s[c]);
                } else {
                    const float gx = G[0][j][i + k], gy = G[1][j][i + k], gz = G[2][j][i + k];
                    s[0] = fmaf(w, gx * gx, s[0]);
                    s[1] = fmaf(w, gx * gy, s[1]);
                    s[2] = fmaf(w, gx * gz, s[2]);
                    s[3] = fmaf(w, gy * gy, s[3]);
                    s[4] = fmaf(w, gy * gz, s[4]);
                    s[5] = fmaf(w, gz * gz, s[5]);
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c++) X[c][j][i] = s[c];
        }
        __syncthreads();
        float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const float w = a.t.w[k < R ? R - k : k - R];
#pragma unroll
            for (int c = 0; c < 6; c++) v[c] = fmaf(w, X[c][ty + k][tx], v[c]);
        }
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const float w = a.t.w[k < R ? R - k : k - R];
#pragma unroll
            for (int c = 0; c < 6; c++) acc[k][c] = fmaf(w, v[c], acc[k][c]);
        }
        const int o = p - R;                  // acc[0] now holds output plane o
        if (o >= a.z0 && x < a.nx && y < a.ny) {
            const size_t vo = (size_t)(o - a.z0) * plane + (size_t)y * a.nx + x;
            if (a.S[0]) {
#pragma unroll
                for (int c = 0; c < 6; c++) a.S[c][vo] = acc[0][c];
            }
            float w3[3], ev[3][3];
            sym3_eigen(acc[0][0], acc[0][1], acc[0][2], acc[0][3], acc[0][4], acc[0][5], w3, ev);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                a.eigval[(size_t)j * nout + vo] = w3[j];
#pragma unroll
                for (int c = 0; c < 3; c++) a.eigvec[(size_t)(c + 3 * j) * nout + vo] = ev[j][c];
            }
        }
#pragma unroll
        for (int k = 0; k < 2 * R; k++)
#pragma unroll
            for (int c = 0; c < 6; c++) acc[k][c] = acc[k + 1][c];
#pragma unroll
        for (int c = 0; c < 6; c++) acc[2 * R][c] = 0.0f;
    }
}

// KernelFactors.gaussian(s): 4 ceil(s) + 1 taps exp(-x^2 / (2 s^2)), normalised to sum 1 (double on the host, then float)
int radius(float s) { return s > 0.0f ? 2 * (int)std::ceil((double)s) : 0; }
Taps taps(float s, int R) {
    Taps t{};
    if (R == 0) { t.w[0] = 1.0f; return t; }
    double w[ST_RMAX + 1], sum = 0.0;
    for (int k = 0; k <= R; k++) { w[k] = std::exp(-(double)k * k / (2.0 * (double)s * s)); sum += k ? 2.0 * w[k] : w[k]; }
    for (int k = 0; k <= R; k++) t.w[k] = (float)(w[k] / sum);
    return t;
}

int check_params(float sigma, float rho, int *rs, int *rr) {
    FIB_CHECK(!std::isnan(sigma) && !std::isnan(rho) && !std::isinf(sigma) && !std::isinf(rho), FIB_ERR_INVALID,
              "sigma and rho must be finite");
    *rs = radius(sigma);
    *rr = radius(rho);
    FIB_CHECK(*rs <= ST_RMAX && *rr <= ST_RMAX, FIB_ERR_UNSUPPORTED,
              "st_recon: Gaussian radius 2*ceil(sigma) = %d, 2*ceil(rho) = %d; at most %d is supported (sigma, rho <= 8)", *rs, *rr, ST_RMAX);
    return FIB_OK;
}

// [lo, hi) of the reflected images of the indices [a, b) on an axis of length n
void refl_range(int a, int b, int n, int *lo, int *hi) {
    *lo = n; *hi = 0;
    for (int i = a; i < b; i++) { const int r = refl(i, n); if (r < *lo) *lo = r; if (r + 1 > *hi) *hi = r + 1; }
}

template <int R> void launch_grad(const GradArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(st_grad_kernel<R>, dim3((unsigned)fib::cdiv(a.nx, TX - 2), (unsigned)fib::cdiv(a.ny, TY - 2)), dim3(NT), 0, st, a);
}
template <int R> void launch_tensor(const TensorArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(st_tensor_kernel<R>, dim3((unsigned)fib::cdiv(a.nx, TX), (unsigned)fib::cdiv(a.ny, TY)), dim3(NT), 0, st, a);
}
template <int... Rs> struct Radii {
    static void grad(int R, const GradArgs &a, hipStream_t st) { (void)((R == Rs ? (launch_grad<Rs>(a, st), true) : false) || ...); }
    static void tensor(int R, const TensorArgs &a, hipStream_t st) { (void)((R == Rs ? (launch_tensor<Rs>(a, st), true) : false) || ...); }
};
using AllRadii = Radii<0, 2, 4, 6, 8, 10, 12, 14, 16>;   // 2 ceil(s) is even

}  // namespace

extern "C" int fib_st_recon_halo(float sigma, float rho, int *halo) try {
    FIB_CHECK(halo, FIB_ERR_INVALID, "NULL argument");
    int rs, rr;
    const int rc = check_params(sigma, rho, &rs, &rr);
    if (rc != FIB_OK) return rc;
    *halo = rs + 1 + rr;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_st_recon_work_size(int nx, int ny, int nz_out, float sigma, float rho, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz_out > 0, FIB_ERR_INVALID, "nx, ny, nz_out must be positive");
    int rs, rr;
    const int rc = check_params(sigma, rho, &rs, &rr);
    if (rc != FIB_OK) return rc;
    *bytes = (size_t)3 * sizeof(float) * nx * ny * (size_t)(nz_out + 2 * rr);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_st_recon(const float *vol, int nx, int ny, int nz, int zin0, int nzin, int z0, int z1, float sigma, float rho,
                             float *eigvec, float *eigval, float *const *S_out, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(vol && eigvec && eigval && work, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    FIB_CHECK(0 <= z0 && z0 < z1 && z1 <= nz, FIB_ERR_INVALID, "output planes [%d, %d) outside [0, %d)", z0, z1, nz);
    FIB_CHECK(0 <= zin0 && nzin > 0 && zin0 + nzin <= nz, FIB_ERR_INVALID, "input planes [%d, %d) outside [0, %d)", zin0, zin0 + nzin, nz);
    if (S_out) for (int c = 0; c < 6; c++) FIB_CHECK(S_out[c] != nullptr, FIB_ERR_INVALID, "NULL S_out volume %d", c);
    int rs, rr;
    const int rc = check_params(sigma, rho, &rs, &rr);
    if (rc != FIB_OK) return rc;
    int gz0, gz1, vz0, vz1;
    refl_range(z0 - rr, z1 + rr, nz, &gz0, &gz1);             // gradient planes K2 reads
    refl_range(gz0 - 1 - rs, gz1 + 1 + rs, nz, &vz0, &vz1);    // vol planes K1 reads
    FIB_CHECK(vz0 >= zin0 && vz1 <= zin0 + nzin, FIB_ERR_INVALID,
              "vol holds planes [%d, %d); outputs [%d, %d) need [%d, %d)", zin0, zin0 + nzin, z0, z1, vz0, vz1);
    const size_t need = (size_t)3 * sizeof(float) * nx * ny * (size_t)(gz1 - gz0);
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "workspace of %zu bytes, %zu needed (fibd_st_recon_work_size)", work_bytes, need);

    const hipStream_t st = (hipStream_t)stream;
    GradArgs ga{vol, nx, ny, nz, zin0, (float *)work, gz0, gz1 - gz0, taps(sigma, rs)};
    {
        fib::ProfScope prof("st_grad", st);
        AllRadii::grad(rs, ga, st);
        FIB_HIP(hipGetLastError());
    }
    TensorArgs ta{(const float *)work, nx, ny, nz, gz0, gz1 - gz0, eigvec, eigval, z0, z1, {}, taps(rho, rr)};
    if (S_out) for (int c = 0; c < 6; c++) ta.S[c] = S_out[c];
    {
        fib::ProfScope prof("st_tensor", st);
        AllRadii::tensor(rr, ta, st);
        FIB_HIP(hipGetLastError());
    }
    return FIB_OK;
} FIB_API_CATCH
