// common.h — internal helpers shared by the translation units of libfibers_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <vector>

#include "../../include/fibers_hip.h"

namespace fib {

// thread-local last-error message (fib_last_error)
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define FIB_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess)                                                                \
            return fib::fail(FIB_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                            \
    } while (0)

#define FIB_CHECK(cond, code, ...)                          \
    do {                                                    \
        if (!(cond)) return fib::fail((code), __VA_ARGS__); \
    } while (0)

// pass a callee's error code (and its message) on
#define FIB_RC(x) do { int _rc = (x); if (_rc != FIB_OK) return _rc; } while (0)

// No C++ exception crosses the C ABI (include/fibers_hip.h): every extern "C" body is a function-try-block that ends in one of these.
#define FIB_API_CATCH                                                                                                  \
    catch (const std::bad_alloc &) { return fib::fail(FIB_ERR_NOMEM, "out of host memory"); }                           \
    catch (const std::exception &e_) { return fib::fail(FIB_ERR_INVALID, "internal error: %s", e_.what()); }            \
    catch (...) { return fib::fail(FIB_ERR_INVALID, "internal error (unknown exception)"); }
#define FIB_API_CATCH_VOID catch (...) { }

// selects `device` after validating it; FIB_ERR_NO_DEVICE when there is none (no CPU fallback)
int use_device(int device);

struct DeviceGuard {  // restores the caller's current device on scope exit
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <typename T>
struct DevBuf {  // RAII device allocation
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    int alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return fail(FIB_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e)); }
        n = count;
        return FIB_OK;
    }
    int ensure(size_t count) { return (count <= n && p) ? FIB_OK : alloc(count); }
};

// ---- what every plan constructor is made of (host only) -----------------------------------
// alloc + copy of `count` elements; a count of zero allocates as DevBuf::alloc(0) does and copies nothing
template <typename T>
int upload(DevBuf<T> &buf, const T *host, size_t count) {
    FIB_RC(buf.alloc(count));
    if (count) FIB_HIP(hipMemcpy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return FIB_OK;
}
template <typename T>
int upload(DevBuf<T> &buf, const std::vector<T> &host) { return upload(buf, host.data(), host.size()); }

template <typename T>
int zeroed(DevBuf<T> &buf, size_t count) {  // alloc + clear
    FIB_RC(buf.alloc(count));
    FIB_HIP(hipMemset(buf.p, 0, buf.n * sizeof(T)));
    return FIB_OK;
}

// the body of every fib_*_plan_destroy: the plan's buffers are freed on the device that holds them
template <typename Plan>
void plan_destroy(Plan *plan) {
    if (!plan) return;
    DeviceGuard guard;
    (void)hipSetDevice(plan->device);
    delete plan;
}

// "destroy this when the scope ends": Scoped<fib_odf_plan, fib_odf_plan_destroy> plan(raw);
template <typename T, void (*Destroy)(T *)>
struct DestroyWith { void operator()(T *p) const { Destroy(p); } };
template <typename T, void (*Destroy)(T *)>
using Scoped = std::unique_ptr<T, DestroyWith<T, Destroy>>;

// the b-table refusals, in the reference's words
static inline int check_tables(const float *bval, const float *bvec, int nvol, bool need_bvec = true) {
    FIB_CHECK(bval != nullptr && nvol > 0, FIB_ERR_MISSING_BVAL, "Missing b-value table from input DWI structure");
    FIB_CHECK(!need_bvec || bvec != nullptr, FIB_ERR_MISSING_BVEC, "Missing gradient table from input DWI structure");
    return FIB_OK;
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Environment variables.  The product library reads these names, none of which selects a kernel variant: FIBERS_ODF_FORMAT (what
// FIB_ODF_FORMAT_DEFAULT means: fp16x2 | bf16x3 | f32 -- the format itself is a plan-creation parameter; its former spellings
// FIBERS_ODF_GEMM=f32 / FIBERS_ODF_EXACT=1 are still honoured) and the host tier's pipeline shape (FIBERS_HOST_CHUNK, FIBERS_HOST_PACK,
// FIBERS_COPY_THREADS, FIBERS_HOST_NT) and fib_st_recon's and fib_dwi_denoise's slab thickness (FIBERS_ST_RECON_SLAB, FIBERS_DENOISE_SLAB) and the frames per chunk of fib_vol_xform, fib_dwi_mask and fib_vol_median (FIBERS_VOL_XFORM_FRAMES, FIBERS_MASK_FRAMES, FIBERS_MEDIAN_FRAMES) and the chunks of fib_warp_points / fib_warp_volume (FIBERS_WARP_POINTS, FIBERS_WARP_FRAMES) and the slices per chunk of fib_dwi_degibbs (FIBERS_DEGIBBS_SLICES) and the points per chunk of fib_str_weights (FIBERS_FIXEL_POINTS), through env() below.  The A/B partners of the shipped kernels
// and the knobs of the measurement tools (schedule variants, the split of an XCD's workgroups, the list unit, the phase stamps) exist
// in the DIAGNOSTIC build only (`make stamp`: -DFIB_CLOCK_STAMP -DFIB_AB_VARIANTS -> libfibers_hip_stamp.so, which tools/ load
// through FIBERS_HIP_LIB): ab_env() is a constant nullptr in the product.
const char *env(const char *name);
#ifdef FIB_AB_VARIANTS
static inline const char *ab_env(const char *name) { return env(name); }
#else
static inline const char *ab_env(const char *) { return nullptr; }
#endif

// hipEvent bracket around a kernel launch when fib_profile_enable(1) is active (no-op otherwise)
bool profiling_on();
bool profile_wants(const char *name);                 // fib_profile_filter: only the named kernels are bracketed (every event is a packet in the queue)
bool profile_events(hipEvent_t *a, hipEvent_t *b);   // a pair from the pool (events are reused: creating one costs more than recording it)
void profile_push(const char *name, hipEvent_t a, hipEvent_t b);
void profile_add_ms(const char *name, double ms);
struct ProfScope {
    const char *name; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(const char *n, hipStream_t s) : name(n), st(s) {
        if (!profiling_on() || !profile_wants(n)) return;
        if (!profile_events(&a, &b)) { a = b = nullptr; return; }
        (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        profile_push(name, a, b);
    }
};

// ---- host-side work-struct mathematics (setup.cpp) ----------------------------------------
// pinv of a column-major float32 [m x n] matrix (n <= 8 for DTI / ADC, 22 for DKI): float64 one-sided Jacobi SVD,
// Julia's LinearAlgebra.pinv cut-off (singular values <= eps(Float32)*min(m,n)*smax dropped).
void host_pinv(const float *A, int m, int n, float *pA /* [n x m] column-major */);
// the same on a float64 matrix, not rounded; returns the rank under that cut-off
int host_pinv(const double *A, int m, int n, double *pA /* [n x m] column-major */);
// DKI: the design A [nvol x 22] column-major with b in ms/um^2 and pA = pinv(A) [22 x nvol] with rows 0-5 scaled by 1e-3
// and rows 6-20 by 1e-6 (the fit's unknowns in mm^2/s and mm^4/s^2), both float64; returns the rank of A under host_pinv's cut-off.
// host_dki_dir_row: the 6 quadratic (off-diagonals doubled) and 15 multiplicity-weighted quartic monomials of a direction
int host_dki_design(const float *bval, const float *bvec, int nvol, double *A, double *pA);
void host_dki_dir_row(double x, double y, double z, double row[21]);
// DTIwork / ADCwork design matrix (dti.jl:129-140, 66-69); A column-major [nvol x np]
void host_dti_design(const float *bval, const float *bvec, int nvol, int np, float *A);
// GQIwork system matrix (gqi.jl:67-69): A column-major [nvert x nvol]
void host_gqi_matrix(const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                     float sigma, float *A);
// DSIwork as dense maps (dsi.jl:59-143 + 204-242): A column-major [(nvol+nvert) x nvol];
// returns FIB_OK or FIB_ERR_UNSUPPORTED.  scale_frame/scale_coef: sum(p) = scale_coef*max(s[scale_frame],0).
int host_dsi_matrix(const float *bval, const float *bvec, int nvol, const float *verts, int nverts,
                    int hann_width, float *A, int *scale_frame, float *scale_coef, std::vector<int> *iq_out = nullptr);
// folded-face neighbour table (gqi.jl:63-64 + 185-196): nbr [nvert x maxdeg] row-major, -1 padded
int host_neighbours(const int32_t *faces, int nfaces, int nverts, std::vector<int32_t> &nbr, int *maxdeg);

// O[M x n] = A[M x K] * max(S[K x n], 0) on the contraction kernels of odf.hip (row N4, RUMBA-SD): A column-major
// [nrows x ncols]; S, out planar (row stride n); `ones` = n bytes of 1 on the device; recompact = (re)build the column
// list (needed once per n)
int matrix_plan_create(int device, const float *A, int nrows, int ncols, fib_odf_plan **plan);
// the plan fib_find_peaks* and CSD hand to the peak finder: fib_gqi_plan_create on one dummy frame, with its refusals
int peaks_plan_create(int device, const float *verts, int nverts, const int32_t *faces, int nfaces, fib_odf_plan **plan);
int matrix_plan_run(const fib_odf_plan *plan, const float *S, const uint8_t *ones, int64_t n, float *out, bool recompact, void *stream);

// The probabilistic tracer in its two phases (probtrack.hip), for fibd_prob_run and fib_prob_stream: all pointers of a run on the device.
struct ProbRun {
    const fib_prob_plan *plan;
    int nx, ny, nz, len_min, len_max, nsub;
    float step;
    const uint16_t *table;
    const int64_t *seeds;
    int64_t nseed;
    const float *sublist;
    uint64_t rng_seed;
};
size_t prob_work_bytes(int64_t nlines);                  // the work area of a run of nlines = nseed * nsub lines (fibd_prob_work_size)
// the run's refusals, pass 1, len_min, the offsets; waits for the stream and returns the totals
int prob_count(const ProbRun &run, void *work, size_t work_bytes, hipStream_t stream, int64_t *nlines, int64_t *npoints);
// pass 2: the kept lines replayed into npts / seed_index / xyz (which hold at least the totals prob_count returned); asynchronous
int prob_emit(const ProbRun &run, void *work, int32_t *npts, int64_t *seed_index, float *xyz, hipStream_t stream);

// The mean of dwi_mask as fib_dwi_mask takes it (volmask.hip): nf frames [nf][nvox] on the device added, in their order, to the float64
// sums that lie in a workspace of fibd_dwi_mask_work_size bytes (first: the sums start from zero); then the sums divided by `count`
// and everything fibd_dwi_mask does after its mean.  b0 may be NULL; info is device memory.
int vm_mean_add(void *work, const float *frames, int64_t nvox, int nf, bool first, hipStream_t stream);
int vm_mask_finish(void *work, int count, int nx, int ny, int nz, const fib_mask_params *params, uint8_t *mask, float *b0, fib_mask_info *info,
                   hipStream_t stream);

// Gibbs-ringing removal (include/fibers_hip.h; setup.cpp): the circulant table of a row length n, D[(j - 1) * n + t] = D(t + s_j) for the
// 2K shifted candidates j = 1 .. 2K; the (cos, sin) pairs of 2 pi k / n and the weights c[p] = 1 + cos(2 pi p / n) (0 where 2 p == n)
void host_degibbs_table(int n, int K, double *D);
void host_degibbs_twiddles(int n, double *cs, double *c);

// Non-linear registration (include/fibers_hip.h; setup.cpp): the taps of the regularisation, radius r = ceil(3 sigma) <= max_radius and
// w[t + r] = float32(exp(-t^2 / (2 sigma^2)) / sum) for t = -r .. r, made in float64; sigma == 0 gives r = 0 and the one tap 1
int host_gauss_taps(float sigma, int max_radius, int *radius, float *w);

}  // namespace fib
