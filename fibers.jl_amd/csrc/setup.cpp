// setup.cpp — host-side construction of the reference's work structs (run once per plan).
//   DTIwork/ADCwork  dti.jl:39-84,101-155   -> host_dti_design + host_pinv
//   GQIwork          gqi.jl:32-82           -> host_gqi_matrix + host_neighbours
//   DSIwork          dsi.jl:41-143          -> host_dsi_matrix (+ the linear per-voxel chain dsi.jl:204-242)
//   Registration (not in the reference; include/fibers_hip.h): fib_reg_matrix, fib_reg_nmi and the pattern search fib_reg_search_*
// Nothing here runs per voxel; tables are built in float64 where the reference uses LAPACK/FFTW
// float32 routines and rounded once to float32.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>

#include "common.h"

namespace fib {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// the library's only reader of the process environment (common.h lists the names)
const char *env(const char *name) { return std::getenv(name); }

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

const char *last_error() { return g_err; }

int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(FIB_ERR_NO_DEVICE, "no HIP device available (%s); libfibers_hip has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n) return fail(FIB_ERR_NO_DEVICE, "device %d out of range [0,%d)", device, n);
    FIB_HIP(hipSetDevice(device));
    return FIB_OK;
}

// ------------------------------------------------------------------------------------------
// pinv: one-sided (Hestenes) Jacobi SVD in float64
// ------------------------------------------------------------------------------------------
int host_pinv(const double *A, int m, int n, double *pA) {
    std::vector<double> U((size_t)m * n), V((size_t)n * n, 0.0), sig(n);
    for (size_t i = 0; i < (size_t)m * n; i++) U[i] = A[i];
    for (int j = 0; j < n; j++) V[j + (size_t)n * j] = 1.0;
    for (int sweep = 0; sweep < 80; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double *up = &U[(size_t)m * p], *uq = &U[(size_t)m * q];
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < m; i++) { alpha += up[i] * up[i]; beta += uq[i] * uq[i]; gamma += up[i] * uq[i]; }
                if (gamma == 0.0 || std::fabs(gamma) <= 1e-15 * std::sqrt(alpha * beta)) continue;
                rotated = true;
                double zeta = (beta - alpha) / (2.0 * gamma);
                double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < m; i++) { double a = up[i], b = uq[i]; up[i] = c * a - s * b; uq[i] = s * a + c * b; }
                double *vp = &V[(size_t)n * p], *vq = &V[(size_t)n * q];
                for (int i = 0; i < n; i++) { double a = vp[i], b = vq[i]; vp[i] = c * a - s * b; vq[i] = s * a + c * b; }
            }
        if (!rotated) break;
    }
    double smax = 0;
    for (int j = 0; j < n; j++) {
        double s = 0;
        for (int i = 0; i < m; i++) s += U[i + (size_t)m * j] * U[i + (size_t)m * j];
        sig[j] = std::sqrt(s);
        smax = std::max(smax, sig[j]);
    }
    // LinearAlgebra.pinv: rtol = eps(Float32) * min(m, n); keep S .> rtol * maximum(S)
    const double tol = (double)1.1920929e-07f * std::min(m, n) * smax;
    for (int r = 0; r < n; r++)
        for (int i = 0; i < m; i++) {
            double acc = 0;
            for (int j = 0; j < n; j++)
                if (sig[j] > tol) acc += V[r + (size_t)n * j] * U[i + (size_t)m * j] / (sig[j] * sig[j]);
            pA[r + (size_t)n * i] = acc;          // U columns are unnormalised: u = U/sig
        }
    int rank = 0;
    for (int j = 0; j < n; j++) rank += sig[j] > tol;
    return rank;
}

// the float form: the same arithmetic on the widened matrix, rounded once
void host_pinv(const float *A, int m, int n, float *pA) {
    std::vector<double> Ad((size_t)m * n), pd((size_t)m * n);
    for (size_t i = 0; i < (size_t)m * n; i++) Ad[i] = A[i];
    (void)host_pinv(Ad.data(), m, n, pd.data());
    for (size_t i = 0; i < (size_t)m * n; i++) pA[i] = (float)pd[i];
}

// ------------------------------------------------------------------------------------------
// DTI / ADC design matrix (float32 like the reference)
// ------------------------------------------------------------------------------------------
void host_dti_design(const float *bval, const float *bvec, int nvol, int np, float *A) {
    for (int i = 0; i < nvol; i++) {
        const float nb = -bval[i];
        if (np == 2) {                          // ADCwork, dti.jl:68-69
            A[i] = nb;
            A[i + nvol] = 1.0f;
            continue;
        }
        const float gx = bvec[i], gy = bvec[i + nvol], gz = bvec[i + 2 * nvol];
        A[i + 0 * nvol] = (gx * gx) * nb;       // dti.jl:131-138
        A[i + 1 * nvol] = ((2.0f * gx) * gy) * nb;
        A[i + 2 * nvol] = ((2.0f * gx) * gz) * nb;
        A[i + 3 * nvol] = (gy * gy) * nb;
        A[i + 4 * nvol] = ((2.0f * gy) * gz) * nb;
        A[i + 5 * nvol] = (gz * gz) * nb;
        A[i + 6 * nvol] = 1.0f;                 // dti.jl:140
    }
}

// ------------------------------------------------------------------------------------------
// DKI design matrix and pseudo-inverse (float64, b in ms/um^2)
// ------------------------------------------------------------------------------------------
// the 15 quartic monomials x^a y^b z^c of the kurtosis tensor in the order of d[6..20], and how often each occurs in
// sum_ijkl n_i n_j n_k n_l V_ijkl
const int dki_pow[15][3] = {{4, 0, 0}, {0, 4, 0}, {0, 0, 4}, {3, 1, 0}, {3, 0, 1}, {1, 3, 0}, {0, 3, 1}, {1, 0, 3}, {0, 1, 3},
                            {2, 2, 0}, {2, 0, 2}, {0, 2, 2}, {2, 1, 1}, {1, 2, 1}, {1, 1, 2}};
const double dki_mult[15] = {1, 1, 1, 4, 4, 4, 4, 4, 4, 6, 6, 6, 12, 12, 12};

void host_dki_dir_row(double x, double y, double z, double row[21]) {
    row[0] = x * x; row[1] = 2.0 * x * y; row[2] = 2.0 * x * z; row[3] = y * y; row[4] = 2.0 * y * z; row[5] = z * z;
    const double px[5] = {1.0, x, x * x, x * x * x, (x * x) * (x * x)};
    const double py[5] = {1.0, y, y * y, y * y * y, (y * y) * (y * y)};
    const double pz[5] = {1.0, z, z * z, z * z * z, (z * z) * (z * z)};
    for (int k = 0; k < 15; k++) row[6 + k] = dki_mult[k] * (px[dki_pow[k][0]] * py[dki_pow[k][1]] * pz[dki_pow[k][2]]);
}

int host_dki_design(const float *bval, const float *bvec, int nvol, double *A, double *pA) {
    const int np = 22;
    for (int i = 0; i < nvol; i++) {
        const double b = (double)bval[i] / 1000.0;                    // ms/um^2: the columns -b, b^2/6 and 1 within 1e2 of each other
        double row[21];
        host_dki_dir_row(bvec[i], bvec[i + nvol], bvec[i + 2 * nvol], row);
        for (int k = 0; k < 6; k++) A[i + (size_t)nvol * k] = -b * row[k];
        for (int k = 6; k < 21; k++) A[i + (size_t)nvol * k] = (b * b / 6.0) * row[k];
        A[i + (size_t)nvol * 21] = 1.0;
    }
    const int rank = host_pinv(A, nvol, np, pA);
    for (int i = 0; i < nvol; i++) {                                  // back to s/mm^2: D in mm^2/s, V in mm^4/s^2
        for (int k = 0; k < 6; k++) pA[k + (size_t)np * i] *= 1e-3;
        for (int k = 6; k < 21; k++) pA[k + (size_t)np * i] *= 1e-6;
    }
    return rank;
}

// ------------------------------------------------------------------------------------------
// GQI system matrix
// ------------------------------------------------------------------------------------------
void host_gqi_matrix(const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                     float sigma, float *A) {
    const int nvert = nverts / 2;
    const float pif = 3.14159274101257324f;
    const float sop = sigma / pif;              // T(sigma / pi), gqi.jl:68
    for (int j = 0; j < nvol; j++) {
        const float sc = std::sqrt(bval[j] * 0.01506f) * sop;
        const float bq[3] = {bvec[j] * sc, bvec[j + nvol] * sc, bvec[j + 2 * nvol] * sc};
        for (int v = 0; v < nvert; v++) {
            const int r = nvert + v;            // second half of the sphere, gqi.jl:69
            float x = verts[r] * bq[0];
            x += verts[r + nverts] * bq[1];
            x += verts[r + 2 * nverts] * bq[2];
            const double xd = x;
            const double y = (xd == 0.0) ? 1.0 : std::sin(M_PI * xd) / (M_PI * xd);   // Base.sinc
            A[v + (size_t)nvert * j] = (float)y;
        }
    }
}

// ------------------------------------------------------------------------------------------
// DSI as two dense maps
// ------------------------------------------------------------------------------------------
int host_dsi_matrix(const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                    int hann_width, float *A, int *scale_frame, float *scale_coef, std::vector<int> *iq_out) {
    const int nvert = nverts / 2;
    float bmin = bval[0];
    for (int j = 1; j < nvol; j++) bmin = std::min(bmin, bval[j]);
    float b1 = INFINITY;
    for (int j = 0; j < nvol; j++) if (bval[j] > bmin) b1 = std::min(b1, bval[j]);
    if (!(b1 < INFINITY)) return fail(FIB_ERR_UNSUPPORTED, "DSI needs at least two distinct b-values");
    const float dq = std::sqrt(b1);                                   // dsi.jl:66
    std::vector<int> iq((size_t)3 * nvol);
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int j = 0; j < nvol; j++) {
        const float sb = std::sqrt(bval[j]);
        for (int c = 0; c < 3; c++) {
            const float q = bvec[j + c * nvol] * sb;                  // dsi.jl:62
            const int v = (int)std::nearbyint(q / dq);               // dsi.jl:67 (ties to even)
            iq[3 * j + c] = v;
            lo = std::min(lo, v); hi = std::max(hi, v);
        }
    }
    if (iq_out) *iq_out = iq;
    int nfft = 1;
    while (nfft < hi - lo + 1) nfft *= 2;                             // dsi.jl:70-71
    const int shift = nfft / 2 + 1;                                   // dsi.jl:73 (1-based)
    if (lo + shift < 1 || hi + shift > nfft)
        return fail(FIB_ERR_UNSUPPORTED, "q-space lattice [%d,%d] does not fit the %d^3 FFT grid (BoundsError in the reference)", lo, hi, nfft);
    if (nfft < 4) return fail(FIB_ERR_UNSUPPORTED, "q-space grid too small (nfft=%d)", nfft);

    // effective frame per lattice point: later frames overwrite earlier ones (dsi.jl:205)
    std::vector<int64_t> lin(nvol);
    std::vector<char> eff(nvol, 1);
    for (int j = 0; j < nvol; j++)
        lin[j] = (iq[3 * j] + shift - 1) + (int64_t)nfft * ((iq[3 * j + 1] + shift - 1) + (int64_t)nfft * (iq[3 * j + 2] + shift - 1));
    for (int j = 0; j < nvol; j++)
        for (int k = j + 1; k < nvol; k++) if (lin[k] == lin[j]) { eff[j] = 0; break; }
    std::vector<float> H(nvol);
    for (int j = 0; j < nvol; j++) {
        if (hann_width == 0) { H[j] = 1.0f; continue; }
        const double r = std::sqrt((double)(iq[3 * j] * iq[3 * j] + iq[3 * j + 1] * iq[3 * j + 1] + iq[3 * j + 2] * iq[3 * j + 2]));
        H[j] = (float)((1.0 + std::cos(r * (2.0 * M_PI / hann_width))) * 0.5);   // dsi.jl:84
    }
    std::vector<double> ctab(nfft);
    for (int k = 0; k <= nfft / 2; k++) ctab[k] = std::cos(2.0 * M_PI * k / nfft);
    for (int k = nfft / 2 + 1; k < nfft; k++) ctab[k] = ctab[nfft - k];   // exactly even: columns of q and -q are bit-identical
    auto cosk = [&](int64_t k) { int64_t r = k % nfft; if (r < 0) r += nfft; return ctab[r]; };

    *scale_frame = -1; *scale_coef = 0.0f;
    const int nrows = nvol + nvert;
    // pdf rows: p[iq_i] for a unit sample at frame j = H_j cos(2 pi iq_i.iq_j / nfft)  (dsi.jl:212-227)
    for (int j = 0; j < nvol; j++) {
        float *col = A + (size_t)nrows * j;
        if (!eff[j]) { for (int i = 0; i < nrows; i++) col[i] = 0.0f; continue; }
        if (iq[3 * j] == 0 && iq[3 * j + 1] == 0 && iq[3 * j + 2] == 0) {
            *scale_frame = j;                                          // sum(p) = nfft^3 * H(0) * s_j
            *scale_coef = (float)((double)nfft * nfft * nfft * H[j]);
        }
        for (int i = 0; i < nvol; i++) {
            const int64_t d = (int64_t)iq[3 * i] * iq[3 * j] + (int64_t)iq[3 * i + 1] * iq[3 * j + 1] + (int64_t)iq[3 * i + 2] * iq[3 * j + 2];
            col[i] = (float)((double)H[j] * cosk(d));
        }
    }
    // odf rows: dqr * sum_r qr2[r] * trilinear(p; v*qr[r] + shift)   (dsi.jl:104-109, 230-242)
    const int nrad = 21;
    float qr[nrad], qr2[nrad];
    for (int r = 0; r < nrad; r++) {
        const double t = 0.3 + 0.03 * r;                               // .3:.03:.9
        qr[r] = (float)(nfft / 2 - 1) * (float)t;
        qr2[r] = qr[r] * qr[r];
    }
    const float dqr = qr[1] - qr[0];
    struct Tap { int g[3]; double w; };
    std::vector<Tap> taps((size_t)8 * nrad);
    for (int v = 0; v < nvert; v++) {
        const int rv = nvert + v;                                      // second-half vertex, dsi.jl:108
        for (int r = 0; r < nrad; r++) {
            int i0[3]; double f[3];
            for (int c = 0; c < 3; c++) {
                const float x = verts[rv + c * nverts] * qr[r] + (float)shift;    // 1-based coordinate, float32
                int ix = (int)std::floor(x);
                ix = std::min(std::max(ix, 1), nfft - 1);
                i0[c] = ix - 1 - nfft / 2;                              // centred 0-based grid offset (r - nfft/2)
                f[c] = (double)(x - (float)ix);
            }
            for (int t = 0; t < 8; t++) {
                Tap &tp = taps[(size_t)8 * r + t];
                double w = (double)qr2[r];
                for (int c = 0; c < 3; c++) {
                    const int b = (t >> c) & 1;
                    tp.g[c] = i0[c] + b;
                    w *= b ? f[c] : 1.0 - f[c];
                }
                tp.w = w;
            }
        }
        for (int j = 0; j < nvol; j++) {
            float *col = A + (size_t)nrows * j;
            if (!eff[j]) { col[nvol + v] = 0.0f; continue; }
            double acc = 0;
            for (size_t t = 0; t < taps.size(); t++) {
                const Tap &tp = taps[t];
                const int64_t d = (int64_t)tp.g[0] * iq[3 * j] + (int64_t)tp.g[1] * iq[3 * j + 1] + (int64_t)tp.g[2] * iq[3 * j + 2];
                acc += tp.w * cosk(d);
            }
            col[nvol + v] = (float)(acc * (double)H[j] * (double)dqr);
        }
    }
    return FIB_OK;
}

// ------------------------------------------------------------------------------------------
// neighbour table of the folded half-sphere
// ------------------------------------------------------------------------------------------
int host_neighbours(const int32_t *faces, int nfaces, int nverts, std::vector<int32_t> &nbr, int *maxdeg) {
    const int nvert = nverts / 2;
    std::vector<std::vector<int32_t>> adj(nvert);
    for (int f = 0; f < nfaces; f++) {
        int32_t v[3];
        for (int c = 0; c < 3; c++) {
            int32_t x = faces[f + (size_t)nfaces * c];
            if (x < 1 || x > nverts) return fail(FIB_ERR_INVALID, "face %d references vertex %d outside 1..%d", f, x, nverts);
            if (x > nvert) x -= nvert;                                 // gqi.jl:64
            v[c] = x - 1;
        }
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                if (a == b) continue;
                // a vertex that meets ITSELF in a folded face is always zeroed (o[a] >= o[a]); keep the self edge
                auto &l = adj[v[a]];
                if (std::find(l.begin(), l.end(), v[b]) == l.end()) l.push_back(v[b]);
            }
    }
    int md = 0;
    for (auto &l : adj) md = std::max(md, (int)l.size());
    if (md > 16) return fail(FIB_ERR_UNSUPPORTED, "ODF vertex degree %d exceeds the supported maximum of 16", md);
    *maxdeg = md;
    nbr.assign((size_t)nvert * (md > 0 ? md : 1), -1);
    for (int v = 0; v < nvert; v++)
        for (size_t k = 0; k < adj[v].size(); k++) nbr[(size_t)v * md + k] = adj[v][k];
    return FIB_OK;
}

// ------------------------------------------------------------------------------------------
// per-kernel event timing
// ------------------------------------------------------------------------------------------
struct ProfPair { hipEvent_t first, second; int dev; };
struct ProfEntry { std::string name; std::vector<ProfPair> pending; double ms = 0; int64_t count = 0; };
static std::mutex g_prof_mu;
static std::vector<ProfEntry> g_prof;
static bool g_prof_on = false;
static std::vector<std::string> g_prof_filter;          // empty: every kernel
static std::vector<std::pair<int, hipEvent_t>> g_prof_pool;   // (device, event) between uses: an event is recorded on streams of the device it was created on

bool profiling_on() { return g_prof_on; }

bool profile_wants(const char *name) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_filter.empty()) return true;
    for (auto &f : g_prof_filter) if (f == name) return true;
    return false;
}

bool profile_events(hipEvent_t *a, hipEvent_t *b) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        int got = 0;
        for (size_t i = g_prof_pool.size(); i-- > 0 && got < 2;)
            if (g_prof_pool[i].first == dev) { ev[got++] = g_prof_pool[i].second; g_prof_pool.erase(g_prof_pool.begin() + (long)i); }
    }
    for (int i = 0; i < 2; i++)
        if (!ev[i] && hipEventCreate(&ev[i]) != hipSuccess) {
            std::lock_guard<std::mutex> lk(g_prof_mu);
            for (int j = 0; j < 2; j++) if (ev[j]) g_prof_pool.emplace_back(dev, ev[j]);
            return false;
        }
    *a = ev[0]; *b = ev[1];
    return true;
}
static void profile_recycle(const ProfPair &pr) {         // (g_prof_mu held) back to the pool of the device the pair belongs to
    g_prof_pool.emplace_back(pr.dev, pr.first);
    g_prof_pool.emplace_back(pr.dev, pr.second);
}

void profile_push(const char *name, hipEvent_t a, hipEvent_t b) {
    int dev = 0;
    (void)hipGetDevice(&dev);                                // (the scope that recorded the pair runs under the device it launches on)
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &e : g_prof) if (e.name == name) { e.pending.push_back(ProfPair{a, b, dev}); return; }
    g_prof.emplace_back();
    g_prof.back().name = name;
    g_prof.back().pending.push_back(ProfPair{a, b, dev});
}

// a host-side stage's duration (the host tier's gather / scatter stages), into the same table
void profile_add_ms(const char *name, double ms) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &e : g_prof) if (e.name == name) { e.ms += ms; e.count++; return; }
    g_prof.emplace_back();
    g_prof.back().name = name;
    g_prof.back().ms = ms; g_prof.back().count = 1;
}

}  // namespace fib

extern "C" int fib_profile_enable(int on) { fib::g_prof_on = on != 0; return FIB_OK; }

// only the kernels named in the comma-separated list are bracketed (NULL or "": every kernel).  An event pair is two packets in the queue:
// bench.py brackets the one kernel its roofline is about during the timed steps
extern "C" int fib_profile_filter(const char *names) try {
    std::lock_guard<std::mutex> lk(fib::g_prof_mu);
    fib::g_prof_filter.clear();
    if (!names) return FIB_OK;
    std::string cur;
    for (const char *c = names;; c++) {
        if (*c == ',' || *c == '\0') { if (!cur.empty()) fib::g_prof_filter.push_back(cur); cur.clear(); if (*c == '\0') break; }
        else if (*c != ' ') cur.push_back(*c);
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_profile_reset(void) try {
    std::lock_guard<std::mutex> lk(fib::g_prof_mu);
    for (auto &e : fib::g_prof) {
        for (auto &pr : e.pending) { (void)hipEventSynchronize(pr.second); fib::profile_recycle(pr); }
    }
    fib::g_prof.clear();
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_profile_get(const char *kernel, double *total_ms, int64_t *count) try {
    FIB_CHECK(kernel && total_ms && count, FIB_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(fib::g_prof_mu);
    *total_ms = 0; *count = 0;
    for (auto &e : fib::g_prof) {
        if (e.name != kernel) continue;
        for (auto &pr : e.pending) {
            float ms = 0;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { e.ms += ms; e.count++; }
            fib::profile_recycle(pr);
        }
        e.pending.clear();
        *total_ms = e.ms; *count = e.count;
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" const char *fib_last_error(void) { return fib::last_error(); }
extern "C" const char *fib_version(void) { return "fibers-hip 0.1 (gfx950)"; }
extern "C" int fib_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} FIB_API_CATCH

extern "C" int fib_dki_design(const float *bval, const float *bvec, int nvol, float *A, float *pA, int *rank) try {
    if (rank) *rank = 0;
    FIB_RC(fib::check_tables(bval, bvec, nvol));
    std::vector<double> Ad((size_t)nvol * 22), pd((size_t)nvol * 22);
    const int r = fib::host_dki_design(bval, bvec, nvol, Ad.data(), pd.data());
    if (rank) *rank = r;
    if (A) for (size_t i = 0; i < Ad.size(); i++) A[i] = (float)Ad[i];
    if (pA) for (size_t i = 0; i < pd.size(); i++) pA[i] = (float)pd[i];
    FIB_CHECK(r == 22, FIB_ERR_INVALID, "DKI needs a b ~ 0 frame and at least two non-zero shells with 15 or more distinct directions "
              "(the design has rank %d of 22 on %d frames)", r, nvol);
    return FIB_OK;
} FIB_API_CATCH

// ---- Gibbs-ringing removal (include/fibers_hip.h): the tables of a row length n ---------------------------------------------------
namespace fib {
// D[(j - 1) * n + t] = D(t + s_j), j = 1 .. 2K, t = 0 .. n - 1, with D(t) = (1 + 2 sum_{k=1..h} cos(2 pi k t / n)) / n, h = (n - 1) / 2,
// s_j = j / (2K + 1) for j <= K and -(j - K) / (2K + 1) after.  The argument k (t J + i) mod (n J) is reduced in integers, so every
// cosine is taken of an angle in [0, 2 pi); the sum runs in long double and is rounded to float64 once.
void host_degibbs_table(int n, int K, double *D) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int64_t J = 2 * (int64_t)K + 1, period = (int64_t)n * J;
    const int h = (n - 1) / 2;
    std::vector<long double> c((size_t)period);                    // cos(2 pi a / (n J)): every angle the sums meet
    for (int64_t a = 0; a < period; a++) c[(size_t)a] = cosl(two_pi * (long double)a / (long double)period);
    for (int j = 1; j <= 2 * K; j++) {
        const int64_t i = j <= K ? j : -(int64_t)(j - K);          // the shift in units of 1 / J
        for (int t = 0; t < n; t++) {
            const int64_t a = (((int64_t)t * J + i) % period + period) % period;
            long double s = 0.0L;
            for (int k = h; k >= 1; k--) s += c[(size_t)((a * k) % period)];
            D[(size_t)(j - 1) * n + t] = (double)((1.0L + 2.0L * s) / (long double)n);
        }
    }
}
// cos and sin of 2 pi k / n, k = 0 .. n - 1, as (cos, sin) pairs, and the weights c[p] = 1 + cos(2 pi p / n), exactly 0 where 2 p == n
void host_degibbs_twiddles(int n, double *cs, double *c) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < n; k++) {
        const long double a = two_pi * (long double)k / (long double)n;
        cs[2 * k] = (double)cosl(a);
        cs[2 * k + 1] = (double)sinl(a);
        c[k] = 2 * k == n ? 0.0 : 1.0 + cs[2 * k];
    }
}
}  // namespace fib

extern "C" int fib_degibbs_table(int n, int nshifts, double *table) try {
    FIB_CHECK(table, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(n >= 1 && n <= FIB_DEGIBBS_MAX_SIZE, FIB_ERR_INVALID, "degibbs_table: the row length must lie in 1 .. %d, not %d", FIB_DEGIBBS_MAX_SIZE, n);
    FIB_CHECK(nshifts >= 1 && nshifts <= 32, FIB_ERR_INVALID, "dwi_degibbs: nshifts must lie in 1 .. 32, not %d", nshifts);
    fib::host_degibbs_table(n, nshifts, table);
    return FIB_OK;
} FIB_API_CATCH

// ---- Registration (include/fibers_hip.h): the matrices, the cost and the pattern search, in float64 on the host ---------------------
namespace {

using M4 = double[16];

void m4_mul(const double *a, const double *b, double *c) {
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = s;
        }
    memcpy(c, r, sizeof r);
}

bool m4_inv(const double *a, double *out) {                    // Gauss-Jordan with partial pivoting
    double w[4][8];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) { w[i][j] = a[4 * i + j]; w[i][4 + j] = i == j; }
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int r = c + 1; r < 4; r++) if (std::fabs(w[r][c]) > std::fabs(w[p][c])) p = r;
        if (!(std::fabs(w[p][c]) > 0) || !std::isfinite(w[p][c])) return false;
        if (p != c) for (int j = 0; j < 8; j++) std::swap(w[p][j], w[c][j]);
        const double d = w[c][c];
        for (int j = 0; j < 8; j++) w[c][j] /= d;
        for (int r = 0; r < 4; r++) {
            if (r == c) continue;
            const double f = w[r][c];
            if (f != 0) for (int j = 0; j < 8; j++) w[r][j] -= f * w[c][j];
        }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = w[i][4 + j];
    return true;
}

void m3_mul(const double a[9], const double b[9], double c[9]) {
    double r[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
    memcpy(c, r, sizeof r);
}

// G(theta) = C A C^-1 with A = [Rz Ry Rx Sh S | t] and c = V_fix (n - 1) / 2: fixed RAS -> moving RAS
void reg_G(const double *theta, int dof, const float *Vf, const int32_t *size, double *G) {
    double th[12] = {0};
    for (int i = 0; i < dof; i++) th[i] = theta[i];
    const double d2r = M_PI / 180.0, rx = th[3] * d2r, ry = th[4] * d2r, rz = th[5] * d2r;
    const double Rx[9] = {1, 0, 0, 0, std::cos(rx), -std::sin(rx), 0, std::sin(rx), std::cos(rx)};
    const double Ry[9] = {std::cos(ry), 0, std::sin(ry), 0, 1, 0, -std::sin(ry), 0, std::cos(ry)};
    const double Rz[9] = {std::cos(rz), -std::sin(rz), 0, std::sin(rz), std::cos(rz), 0, 0, 0, 1};
    const double Sh[9] = {1, th[9], th[10], 0, 1, th[11], 0, 0, 1};
    const double S[9] = {std::exp(th[6]), 0, 0, 0, std::exp(th[7]), 0, 0, 0, std::exp(th[8])};
    double L[9];
    m3_mul(Rz, Ry, L); m3_mul(L, Rx, L); m3_mul(L, Sh, L); m3_mul(L, S, L);
    double c[3];
    for (int i = 0; i < 3; i++) {
        c[i] = (double)Vf[4 * i + 3];
        for (int j = 0; j < 3; j++) c[i] += (double)Vf[4 * i + j] * (((double)size[j] - 1.0) / 2.0);
    }
    for (int i = 0; i < 16; i++) G[i] = (i % 5 == 0);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) G[4 * i + j] = L[3 * i + j];
        G[4 * i + 3] = c[i] + th[i] - (L[3 * i] * c[0] + L[3 * i + 1] * c[1] + L[3 * i + 2] * c[2]);
    }
}

// out2in of a level: float32(inv(V_mov D_l) G (V_fix D_l)); D_l = [2^l I | (2^l - 1) / 2]
bool reg_out2in(const double *G, const float *Vf, const float *Vm, int level, float *out) {
    double D[16], A[16], B[16], Ai[16], vf[16], vm[16];
    for (int i = 0; i < 16; i++) { D[i] = 0; vf[i] = Vf[i]; vm[i] = Vm[i]; }
    const double s = std::ldexp(1.0, level);
    D[0] = D[5] = D[10] = s; D[15] = 1;
    D[3] = D[7] = D[11] = (s - 1.0) / 2.0;
    m4_mul(vm, D, A);
    m4_mul(vf, D, B);
    if (!m4_inv(A, Ai)) return false;
    m4_mul(Ai, G, A);
    m4_mul(A, B, A);
    for (int i = 0; i < 16; i++) out[i] = (float)A[i];
    return true;
}

double reg_entropy(const uint64_t *c, int n, double N) {      // ln N - (sum c ln c) / N over the non-zero cells, in their order
    double s = 0;
    for (int i = 0; i < n; i++) if (c[i]) s += (double)c[i] * std::log((double)c[i]);
    return std::log(N) - s / N;
}

double reg_nmi(const uint32_t *h, int nb, int64_t nfinite, double min_overlap) {
    const double ninf = -HUGE_VAL;
    std::vector<uint64_t> rows((size_t)nb, 0), cols((size_t)nb, 0), cells((size_t)nb * nb);
    uint64_t N = 0;
    for (int a = 0; a < nb; a++)
        for (int b = 0; b < nb; b++) { const uint64_t c = h[(size_t)a * nb + b]; cells[(size_t)a * nb + b] = c; rows[a] += c; cols[b] += c; N += c; }
    if (N == 0 || (double)N < min_overlap * (double)nfinite) return ninf;
    const double hj = reg_entropy(cells.data(), nb * nb, (double)N);
    if (hj == 0) return ninf;
    return (reg_entropy(rows.data(), nb, (double)N) + reg_entropy(cols.data(), nb, (double)N)) / hj;
}

int reg_levels(const int32_t *a, const int32_t *b) {
    int n = 1, sa[3] = {a[0], a[1], a[2]}, sb[3] = {b[0], b[1], b[2]};
    for (int l = 1; l <= 3; l++) {
        int lo = 1 << 30;
        for (int c = 0; c < 3; c++) { sa[c] = (sa[c] + 1) / 2; sb[c] = (sb[c] + 1) / 2; lo = std::min({lo, sa[c], sb[c]}); }
        if (lo >= 8) n = l + 1;
    }
    return n;
}

}  // namespace

// The pattern search as a state machine: fib_reg_search_jobs hands out the matrices to evaluate, fib_reg_search_feed takes their
// histograms and decides.  A stage is (level, parameters searched); a stage starts with one job, the cost of the current theta there.
struct fib_reg_search {
    int dof, halvings, maxit;
    double min_overlap;
    int32_t fsize[3];
    float fres[3], Vf[16], Vm[16];
    double theta[12], step[12], cur, cand[24][12];
    int nstages, stage, stage_level[5], stage_nd[5], phase, fails, it;
    bool done;
    std::vector<double> trace;

    int level() const { return stage_level[stage]; }
    int nd() const { return stage_nd[stage]; }
    void start_stage() {
        phase = 0; fails = it = 0;
        const int l = level();
        const double h = std::ldexp(1.0, l) * (double)std::min({fres[0], fres[1], fres[2]});
        double s = 0;
        for (int c = 0; c < 3; c++) { const double e = (double)fsize[c] * (double)fres[c]; s = s + e * e; }
        const double R = 0.5 * std::sqrt(s) / std::sqrt(3.0);
        for (int i = 0; i < 12; i++) step[i] = i < 3 ? h : i < 6 ? (h / R) * (180.0 / M_PI) : h / R;
    }
    void end_iteration() {
        if (fails < halvings + 1 && it < maxit) return;
        if (++stage >= nstages) { done = true; stage = nstages - 1; return; }
        start_stage();
    }
};

extern "C" int fib_reg_levels(const int32_t fixed_size[3], const int32_t moving_size[3], int *levels) try {
    FIB_CHECK(fixed_size && moving_size && levels, FIB_ERR_INVALID, "NULL argument");
    for (int c = 0; c < 3; c++) FIB_CHECK(fixed_size[c] > 0 && moving_size[c] > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    *levels = reg_levels(fixed_size, moving_size);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_reg_matrix(const double *theta, int dof, const float fixed_vox2ras[16], const int32_t fixed_size[3], const float moving_vox2ras[16],
                              int level, float out2in[16], double *G) try {
    FIB_CHECK(theta && fixed_vox2ras && fixed_size && moving_vox2ras && (out2in || G), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(dof == 6 || dof == 12, FIB_ERR_INVALID, "dof must be 6 or 12, not %d", dof);
    FIB_CHECK(level >= 0 && level <= 3, FIB_ERR_INVALID, "level %d outside 0..3", level);
    double g[16];
    reg_G(theta, dof, fixed_vox2ras, fixed_size, g);
    if (G) memcpy(G, g, sizeof g);
    if (out2in) FIB_CHECK(reg_out2in(g, fixed_vox2ras, moving_vox2ras, level, out2in), FIB_ERR_INVALID, "the moving volume's vox2ras is singular");
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_reg_nmi(const uint32_t *hist, int nbins, int64_t nfinite_fixed, double min_overlap, double *cost) try {
    FIB_CHECK(hist && cost, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nbins >= FIB_REG_MIN_BINS && nbins <= FIB_REG_MAX_BINS, FIB_ERR_INVALID, "nbins %d outside %d..%d", nbins, FIB_REG_MIN_BINS, FIB_REG_MAX_BINS);
    FIB_CHECK(nfinite_fixed >= 0 && min_overlap >= 0, FIB_ERR_INVALID, "nfinite_fixed and min_overlap must not be negative");
    *cost = reg_nmi(hist, nbins, nfinite_fixed, min_overlap);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_reg_search_create(int dof, const int32_t fixed_size[3], const float fixed_res[3], const float fixed_vox2ras[16],
                                     const int32_t moving_size[3], const float moving_vox2ras[16], int levels, int halvings, int maxit,
                                     double min_overlap, const double *theta0, fib_reg_search **out) try {
    FIB_CHECK(fixed_size && fixed_res && fixed_vox2ras && moving_size && moving_vox2ras && out, FIB_ERR_INVALID, "NULL argument");
    *out = nullptr;
    FIB_CHECK(dof == 6 || dof == 12, FIB_ERR_INVALID, "dof must be 6 or 12, not %d", dof);
    for (int c = 0; c < 3; c++)
        FIB_CHECK(fixed_size[c] > 0 && moving_size[c] > 0 && fixed_res[c] > 0 && std::isfinite(fixed_res[c]), FIB_ERR_INVALID, "sizes and voxel sizes must be positive");
    FIB_CHECK(levels >= 0 && levels <= 4, FIB_ERR_INVALID, "levels must lie in 1 .. 4 (0: the default), not %d", levels);
    FIB_CHECK(halvings >= 0 && maxit >= 0 && min_overlap >= 0, FIB_ERR_INVALID, "halvings, maxit and min_overlap must not be negative");
    float probe[16];
    double g[16];
    const double zero[12] = {0};
    reg_G(zero, 6, fixed_vox2ras, fixed_size, g);
    FIB_CHECK(reg_out2in(g, fixed_vox2ras, moving_vox2ras, 0, probe), FIB_ERR_INVALID, "the moving volume's vox2ras is singular");
    std::unique_ptr<fib_reg_search> s(new fib_reg_search());
    s->dof = dof; s->halvings = halvings; s->maxit = maxit; s->min_overlap = min_overlap;
    for (int c = 0; c < 3; c++) { s->fsize[c] = fixed_size[c]; s->fres[c] = fixed_res[c]; }
    memcpy(s->Vf, fixed_vox2ras, sizeof s->Vf);
    memcpy(s->Vm, moving_vox2ras, sizeof s->Vm);
    for (int i = 0; i < 12; i++) s->theta[i] = theta0 && i < dof ? theta0[i] : 0.0;
    const int nl = levels ? levels : reg_levels(fixed_size, moving_size);
    s->nstages = 0;
    for (int l = nl - 1; l >= 0; l--) { s->stage_level[s->nstages] = l; s->stage_nd[s->nstages++] = 6; }
    if (dof == 12) { s->stage_level[s->nstages] = 0; s->stage_nd[s->nstages++] = 12; }
    s->stage = 0; s->done = false; s->cur = -HUGE_VAL;
    s->start_stage();
    *out = s.release();
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fib_reg_search_destroy(fib_reg_search *s) try { delete s; } FIB_API_CATCH_VOID

extern "C" int fib_reg_search_jobs(fib_reg_search *s, int *level, int *njobs, float *out2in) try {
    FIB_CHECK(s && level && njobs && out2in, FIB_ERR_INVALID, "NULL argument");
    *level = s->level();
    *njobs = 0;
    if (s->done) return FIB_OK;
    double g[16];
    if (s->phase == 0) {
        reg_G(s->theta, 12, s->Vf, s->fsize, g);
        reg_out2in(g, s->Vf, s->Vm, s->level(), out2in);
        *njobs = 1;
        return FIB_OK;
    }
    const int nd = s->nd();
    for (int i = 0; i < nd; i++)
        for (int sg = 0; sg < 2; sg++) {
            double *c = s->cand[2 * i + sg];
            memcpy(c, s->theta, sizeof s->theta);
            c[i] = c[i] + (sg ? -1.0 : 1.0) * s->step[i];
            reg_G(c, 12, s->Vf, s->fsize, g);
            reg_out2in(g, s->Vf, s->Vm, s->level(), out2in + 16 * (2 * i + sg));
        }
    *njobs = 2 * nd;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_reg_search_feed(fib_reg_search *s, const uint32_t *hist, int nbins, int64_t nfinite_fixed) try {
    FIB_CHECK(s && hist, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(!s->done, FIB_ERR_INVALID, "the search has finished: it handed out no jobs");
    FIB_CHECK(nbins >= FIB_REG_MIN_BINS && nbins <= FIB_REG_MAX_BINS, FIB_ERR_INVALID, "nbins %d outside %d..%d", nbins, FIB_REG_MIN_BINS, FIB_REG_MAX_BINS);
    const size_t nb2 = (size_t)nbins * nbins;
    if (s->phase == 0) {
        s->cur = reg_nmi(hist, nbins, nfinite_fixed, s->min_overlap);
        s->phase = 1;
        s->end_iteration();                                     // (maxit == 0: the stage is over)
        return FIB_OK;
    }
    const int nd = s->nd();
    double row[FIB_REG_TRACE_ROW];
    for (int i = 0; i < FIB_REG_TRACE_ROW; i++) row[i] = std::nan("");
    int best = 0;
    for (int j = 0; j < 2 * nd; j++) {
        row[5 + j] = reg_nmi(hist + nb2 * j, nbins, nfinite_fixed, s->min_overlap);
        if (row[5 + j] > row[5 + best]) best = j;               // the first maximum
    }
    row[0] = s->level(); row[1] = nd; row[2] = best; row[4] = s->cur;
    if (row[5 + best] > s->cur) {
        memcpy(s->theta, s->cand[best], sizeof s->theta);
        s->cur = row[5 + best];
        row[3] = 1;
    } else {
        for (int i = 0; i < 12; i++) s->step[i] = s->step[i] / 2.0;
        s->fails++;
        row[3] = 0;
    }
    s->trace.insert(s->trace.end(), row, row + FIB_REG_TRACE_ROW);
    s->it++;
    s->end_iteration();
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_reg_search_result(const fib_reg_search *s, double *theta, double *cost, int *niter, double *trace, int trace_rows) try {
    FIB_CHECK(s, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(trace_rows >= 0 && (trace || trace_rows == 0), FIB_ERR_INVALID, "trace_rows rows need a trace buffer");
    const int n = (int)(s->trace.size() / FIB_REG_TRACE_ROW);
    if (theta) memcpy(theta, s->theta, sizeof s->theta);
    if (cost) *cost = s->cur;
    if (niter) *niter = n;
    if (trace) memcpy(trace, s->trace.data(), sizeof(double) * FIB_REG_TRACE_ROW * (size_t)std::min(n, trace_rows));
    return FIB_OK;
} FIB_API_CATCH

// ---- Non-linear registration (include/fibers_hip.h): the matrices of a level and the Gaussian taps, in float64 on the host ----------
extern "C" int fib_nlreg_level(const float fixed_vox2ras[16], const float moving_vox2ras[16], const float *post, int level, float step,
                               float to_ras[16], float from_ras[16], float T[9], float *kappa) try {
    FIB_CHECK(fixed_vox2ras && moving_vox2ras && to_ras && from_ras && T && kappa, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(level >= 0 && level <= 3, FIB_ERR_INVALID, "level %d outside 0..3", level);
    FIB_CHECK(step > 0.f && std::isfinite(step), FIB_ERR_INVALID, "step must be positive and finite, not %g", (double)step);
    double D[16], A[16], B[16], Ai[16], Bi[16], vf[16], vm[16], P[16];
    for (int i = 0; i < 16; i++) { D[i] = 0; vf[i] = fixed_vox2ras[i]; vm[i] = moving_vox2ras[i]; P[i] = post ? (double)post[i] : (double)(i % 5 == 0); }
    const double s = std::ldexp(1.0, level);
    D[0] = D[5] = D[10] = s; D[15] = 1;
    D[3] = D[7] = D[11] = (s - 1.0) / 2.0;
    m4_mul(vf, D, B);                                           // V_fix D_l
    m4_mul(vm, D, A);                                           // V_mov D_l
    FIB_CHECK(m4_inv(A, Ai), FIB_ERR_INVALID, "the moving volume's vox2ras is singular");
    double L[16];                                               // the linear part of V_fix D_l, alone
    for (int i = 0; i < 16; i++) L[i] = (i % 4 < 3 && i / 4 < 3) ? B[i] : (double)(i % 5 == 0);
    FIB_CHECK(m4_inv(L, Bi), FIB_ERR_INVALID, "the fixed volume's vox2ras is singular");
    m4_mul(Ai, P, A);                                           // inv(V_mov D_l) post
    for (int i = 0; i < 16; i++) { to_ras[i] = (float)B[i]; from_ras[i] = (float)A[i]; }
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) T[3 * c + k] = (float)Bi[4 * k + c];                // inv(L) transposed
    const double ell = s * (double)step;
    *kappa = (float)(1.0 / (ell * ell));
    for (int i = 0; i < 16; i++) FIB_CHECK(std::isfinite(to_ras[i]) && std::isfinite(from_ras[i]), FIB_ERR_INVALID, "a matrix of level %d is not finite", level);
    return FIB_OK;
} FIB_API_CATCH

namespace fib {

int host_gauss_taps(float sigma, int max_radius, int *radius, float *w) {
    FIB_CHECK(sigma >= 0.f && sigma <= 4.f, FIB_ERR_INVALID, "sigma %g outside [0, 4]", (double)sigma);
    const double sg = (double)sigma;
    const int r = (int)std::ceil(3.0 * sg);
    FIB_CHECK(r <= max_radius, FIB_ERR_INVALID, "sigma %g needs a radius of %d, above %d", sg, r, max_radius);
    *radius = r;
    if (r == 0) { w[0] = 1.f; return FIB_OK; }
    double e[64], sum = 0;
    for (int t = -r; t <= r; t++) { e[t + r] = std::exp(-((double)t * (double)t) / (2.0 * sg * sg)); sum += e[t + r]; }
    for (int t = 0; t <= 2 * r; t++) w[t] = (float)(e[t] / sum);
    return FIB_OK;
}

}  // namespace fib
