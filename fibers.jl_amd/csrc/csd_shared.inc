// csd_shared.inc — what csd.hip and msmt.hip have in common, included inside each file's anonymous namespace: the wave helpers, the
// peak gather, the even-harmonic basis, the response quadrature and the host Cholesky (include/fibers_hip.h "Constrained spherical
// deconvolution" defines the basis and R_l; "Multi-shell multi-tissue deconvolution" refers to it unchanged).

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// peak[k] = vertex isort_top[k], f[k] = odf there, for k < nvalid; zeros beyond
__global__ __launch_bounds__(256) void csd_peaks_kernel(const float *__restrict__ odf, const int32_t *__restrict__ top, const int32_t *__restrict__ nvalid,
                                                        const float *__restrict__ verts, int nverts, int nreg, int64_t nvox,
                                                        float *p0, float *p1, float *p2, float *f0, float *f1, float *f2) {
    const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= nvox) return;
    const int nv = nvalid[vox];
    float *const pk[3] = {p0, p1, p2};
    float *const fk[3] = {f0, f1, f2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int idx = top[(int64_t)k * nvox + vox];
        const bool ok = k < nv && idx >= 0 && idx < nreg;
#pragma unroll
        for (int c = 0; c < 3; c++) pk[k][(int64_t)c * nvox + vox] = ok ? verts[idx + (size_t)c * nverts] : 0.0f;
        fk[k][vox] = ok ? odf[(int64_t)idx * nvox + vox] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------
// host: the basis, the response, the Cholesky
// ------------------------------------------------------------------------------------------
// real even spherical harmonics of a direction, column l (l + 1) / 2 + m; P with the Condon-Shortley phase
void sh_row(double x, double y, double z, int lmax, double *row) {
    const double r = std::sqrt(x * x + y * y + z * z);
    const double ct = r > 0.0 ? std::min(1.0, std::max(-1.0, z / r)) : 1.0, st = std::sqrt(std::max(0.0, 1.0 - ct * ct));
    const double phi = std::atan2(y, x);
    for (int m = 0; m <= lmax; m++) {
        double pmm = 1.0;                                                 // P_m^m = (-1)^m (2m - 1)!! sin^m
        for (int k = 1; k <= m; k++) pmm *= -(2.0 * k - 1.0) * st;
        double pl2 = 0.0, pl1 = pmm;                                       // P_{l-2}^m, P_{l-1}^m
        for (int l = m; l <= lmax; l++) {
            double plm;
            if (l == m) plm = pmm;
            else if (l == m + 1) plm = ct * (2.0 * m + 1.0) * pmm;
            else plm = ((2.0 * l - 1.0) * ct * pl1 - (l + m - 1.0) * pl2) / (double)(l - m);
            if (l > m) { pl2 = pl1; pl1 = plm; }
            if (l % 2) continue;
            double fr = 1.0;                                               // (l - m)! / (l + m)!
            for (int k = l - m + 1; k <= l + m; k++) fr /= (double)k;
            const double nlm = std::sqrt((2.0 * l + 1.0) / (4.0 * M_PI) * fr);
            const int c = l * (l + 1) / 2;
            if (m == 0) row[c] = nlm * plm;
            else {
                row[c + m] = M_SQRT2 * nlm * plm * std::cos(m * phi);
                row[c - m] = M_SQRT2 * nlm * plm * std::sin(m * phi);
            }
        }
    }
}

// Gauss-Legendre nodes and weights on [-1, 1] (Newton on P_n)
void gauss_legendre(int n, std::vector<double> &x, std::vector<double> &w) {
    x.resize(n); w.resize(n);
    for (int i = 0; i < n; i++) {
        double t = std::cos(M_PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
        for (int itr = 0; itr < 100; itr++) {
            double p0 = 1.0, p1 = t;
            for (int k = 2; k <= n; k++) { const double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
            dp = n * (t * p1 - p0) / (t * t - 1.0);
            const double dt = p1 / dp;
            t -= dt;
            if (std::fabs(dt) < 1e-16) break;
        }
        double p0 = 1.0, p1 = t;
        for (int k = 2; k <= n; k++) { const double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
        dp = n * (t * p1 - p0) / (t * t - 1.0);
        x[i] = t;
        w[i] = 2.0 / ((1.0 - t * t) * dp * dp);
    }
}

// R_l = 2 pi S0 int exp(-b (lperp + (lpara - lperp) t^2)) P_l(t) dt, l = 0, 2, .. lmax -> R[l / 2], by 64-point Gauss-Legendre
void response_R(double bbar, float lambda_para, float lambda_perp, float s0, int lmax, double *R) {
    std::vector<double> gx, gw;
    gauss_legendre(64, gx, gw);
    for (int l = 0; l <= lmax; l += 2) {
        double acc = 0.0;
        for (size_t k = 0; k < gx.size(); k++) {
            const double t = gx[k];
            double p0 = 1.0, p1 = t;
            for (int j = 2; j <= l; j++) { const double p2 = ((2.0 * j - 1.0) * t * p1 - (j - 1.0) * p0) / j; p0 = p1; p1 = p2; }
            const double pl = l == 0 ? 1.0 : p1;
            acc += gw[k] * std::exp(-bbar * ((double)lambda_perp + ((double)lambda_para - (double)lambda_perp) * t * t)) * pl;
        }
        R[l / 2] = 2.0 * M_PI * (double)s0 * acc;
    }
}

// in-place Cholesky of a dense symmetric [n x n] float64 matrix and its inverse; false: a pivot is not positive
bool host_spd_inverse(std::vector<double> &Mx, int n) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; j++) {
        double dg = Mx[j + (size_t)n * j];
        for (int k = 0; k < j; k++) dg -= L[j + (size_t)n * k] * L[j + (size_t)n * k];
        if (!(dg > 0.0)) return false;
        L[j + (size_t)n * j] = std::sqrt(dg);
        for (int i = j + 1; i < n; i++) {
            double v = Mx[i + (size_t)n * j];
            for (int k = 0; k < j; k++) v -= L[i + (size_t)n * k] * L[j + (size_t)n * k];
            L[i + (size_t)n * j] = v / L[j + (size_t)n * j];
        }
    }
    for (int c = 0; c < n; c++) {                                             // column c of the inverse: L L' x = e_c
        std::vector<double> y(n, 0.0);
        for (int i = 0; i < n; i++) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) v -= L[i + (size_t)n * k] * y[k];
            y[i] = v / L[i + (size_t)n * i];
        }
        for (int i = n - 1; i >= 0; i--) {
            double v = y[i];
            for (int k = i + 1; k < n; k++) v -= L[k + (size_t)n * i] * y[k];
            y[i] = v / L[i + (size_t)n * i];
        }
        for (int i = 0; i < n; i++) Mx[i + (size_t)n * c] = y[i];
    }
    return true;
}
