// register.hip — the device side of intensity-based registration on gfx950 ("Registration", include/fibers_hip.h): the pyramid
// (fibd_vol_halve), the range of a volume's finite values (fibd_vol_range) and the hot kernel, the joint histograms of one fixed volume
// against the frames of a moving series under many candidate matrices at once (fibd_reg_hist).  Not in the reference.  The driver that
// turns histograms into costs and decisions is host code (setup.cpp); tests/register_ref.py restates all of it and the kernels are held
// to that bit for bit: the pull-back and the sampler are those of volxform.hip (xfm_apply.inc, vol_sample.inc), the counts are integers.
//
// rg_hist_kernel: blockIdx.z is the job (a moving frame and a fixed voxel -> moving voxel matrix), so one launch carries every candidate
// of every live frame.  A workgroup is vx_kernel's tile, four neighbouring x-row segments with a wave each, walked through RG_ZC planes;
// each fixed voxel is pulled back, tested, sampled and counted into an LDS histogram, and the non-zero bins go to global memory with
// integer atomics once per workgroup.  Two LDS schemes were built and measured (profiles/register/README.md): <0> one histogram per
// workgroup, <1> a private copy per wave, summed at the flush.  On 140^3 with 12 jobs <1> is level with <0> at 8 and 32 bins (0.8 to 2.5 %
// faster in paired runs, less than two builds of one scheme differ) and, its four copies being 64 KB of LDS, 2.1 times slower at 64: the product takes <1> up to RG_WAVE_COPIES_MAX_BINS and <0> above; the diagnostic
// build forces either (FIBERS_REG_HIST_SCHEME=a|b, tools/register_time.py).  Sums are integer sums: the result does not depend on the
// scheme or the launch.
#include "common.h"

#include <algorithm>

// the pull-back, the interpolation and the binning are sequences of separately rounded float32 operations: nothing here may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "xfm_apply.inc"

#include "vol_sample.inc"

constexpr int RG_MAX_DIM = 1 << 24;                            // every size is exact in float32 (the inside test compares floats)
constexpr int RG_T = 256, RG_BX = 64, RG_BY = 4, RG_ZC = 8;    // a workgroup: 64 x 4 voxels of a plane, RG_ZC planes
constexpr int RG_WAVE_COPIES_MAX_BINS = 32;                     // the shipped LDS scheme: a copy per wave up to here (four copies in 16 KB), one above

// the ordered-uint key of volmask.hip (vm_key): key order is value order for every bit pattern, so extremes do not depend on the order
__device__ inline unsigned rg_key(unsigned b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ inline unsigned rg_unkey(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }
__device__ inline bool rg_finite(unsigned b) { return (b & 0x7f800000u) != 0x7f800000u; }

// what fibd_vol_range leaves per frame (16 bytes); while the reduction runs the words hold max(~key), max(key), -, count
struct RegRange { float lo, hi, scale; uint32_t nfinite; };
struct RegJob { float m[16]; int32_t frame; int32_t pad[3]; };  // a job as the kernel reads it (the head of the workspace)

// ---- pyramid ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_T) void rg_halve_kernel(const float *__restrict__ in, int nx, int ny, int nz, float *__restrict__ out, int ox, int oy,
                                                        int oz) {
    const int64_t nvo = (int64_t)ox * oy * oz, o = (int64_t)blockIdx.x * RG_T + threadIdx.x;
    if (o >= nvo) return;
    const int i = (int)(o % ox), j = (int)((o / ox) % oy), k = (int)(o / ((int64_t)ox * oy));
    const float *src = in + (int64_t)blockIdx.y * nx * ny * nz;
    float s = 0.f;
    int c = 0;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const int x = 2 * i + dx, y = 2 * j + dy, z = 2 * k + dz;
                if (x < nx && y < ny && z < nz) { s = s + src[(int64_t)x + (int64_t)nx * ((int64_t)y + (int64_t)ny * z)]; c++; }
            }
    out[(int64_t)blockIdx.y * nvo + o] = s / (float)c;
}

// ---- range --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_T) void rg_minmax_kernel(const float *__restrict__ v, int64_t nvox, unsigned *acc) {
    __shared__ unsigned sm[3];
    if (threadIdx.x < 3) sm[threadIdx.x] = 0;
    __syncthreads();
    const float *f = v + (int64_t)blockIdx.y * nvox;
    unsigned a = 0, b = 0, c = 0;
    for (int64_t i = (int64_t)blockIdx.x * RG_T + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * RG_T) {
        const unsigned u = __float_as_uint(f[i]);
        if (rg_finite(u)) { const unsigned k = rg_key(u); a = max(a, ~k); b = max(b, k); c++; }
    }
    if (c) { atomicMax(&sm[0], a); atomicMax(&sm[1], b); atomicAdd(&sm[2], c); }
    __syncthreads();
    if (threadIdx.x == 0 && sm[2]) {
        unsigned *g = acc + 4 * blockIdx.y;
        atomicMax(&g[0], sm[0]); atomicMax(&g[1], sm[1]); atomicAdd(&g[3], sm[2]);
    }
}

__global__ void rg_range_kernel(unsigned *acc, int nframes, float nbins) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const unsigned nk = acc[4 * f], kmax = acc[4 * f + 1], n = acc[4 * f + 3];
    RegRange r;
    r.lo = n ? __uint_as_float(rg_unkey(~nk)) : 0.f;
    r.hi = n ? __uint_as_float(rg_unkey(kmax)) : 0.f;
    r.scale = n ? nbins / (r.hi - r.lo) : __uint_as_float(0x7fc00000u);
    r.nfinite = n;
    reinterpret_cast<RegRange *>(acc)[f] = r;
}

// ---- joint histograms ---------------------------------------------------------------------------------------------------------------
// t = (v - lo) * scale, two roundings; no bin when t is NaN (a NaN v; Inf * 0); else clamp(floor(t), 0, nbins - 1), clamped as a float
__device__ __forceinline__ int rg_bin(float v, float lo, float scale, float top) {
    const float t = (v - lo) * scale;
    if (t != t) return -1;
    const float b = floorf(t);
    return (int)(b < 0.f ? 0.f : (b > top ? top : b));
}

template <int SCHEME>
__global__ __launch_bounds__(RG_T) void rg_hist_kernel(const float *__restrict__ fixed, int nxf, int nyf, int nzf, const RegRange *__restrict__ rf,
                                                       const float *__restrict__ moving, int nxm, int nym, int nzm,
                                                       const RegRange *__restrict__ rm, const RegJob *__restrict__ jobs, int nbins,
                                                       unsigned *__restrict__ hist, unsigned nsx, unsigned nsy) {
    extern __shared__ unsigned rg_lds[];
    const int nb2 = nbins * nbins, copies = SCHEME ? RG_BY : 1;
    for (int t = threadIdx.x; t < copies * nb2; t += RG_T) rg_lds[t] = 0;
    __syncthreads();
    const RegJob &J = jobs[blockIdx.z];
    XfmMat M;
#pragma unroll
    for (int e = 0; e < 16; e++) M.m[e] = J.m[e];
    const RegRange ra = rf[0], rv = rm[J.frame];
    const float *__restrict__ mov = moving + (int64_t)J.frame * nxm * nym * nzm;
    const float top = (float)(nbins - 1);
    const unsigned b = blockIdx.x, bx = b % nsx, r = b / nsx, by = r % nsy, kc = r / nsy;
    const int i = (int)(bx * RG_BX) + (int)(threadIdx.x % RG_BX), j = (int)(by * RG_BY) + (int)(threadIdx.x / RG_BX);
    unsigned *h = rg_lds + (SCHEME ? (int)(threadIdx.x / RG_BX) * nb2 : 0);      // (a row of the tile is one wave)
    if (i < nxf && j < nyf) {
        const int k1 = min(nzf, (int)(kc + 1) * RG_ZC);
        for (int k = (int)kc * RG_ZC; k < k1; k++) {
            const float a = fixed[(int64_t)i + (int64_t)nxf * ((int64_t)j + (int64_t)nyf * k)];
            if (!rg_finite(__float_as_uint(a))) continue;
            const float3 p = xfm_point(M, (float)i, (float)j, (float)k);
            if (!vx_inside(p, nxm, nym, nzm)) continue;
            const int bv = rg_bin(vx_cell_value(vx_cell(p, nxm, nym, nzm), mov), rv.lo, rv.scale, top);
            const int ba = rg_bin(a, ra.lo, ra.scale, top);
            if (bv < 0 || ba < 0) continue;
            atomicAdd(&h[ba * nbins + bv], 1u);
        }
    }
    __syncthreads();
    unsigned *g = hist + (int64_t)blockIdx.z * nb2;
    for (int t = threadIdx.x; t < nb2; t += RG_T) {
        unsigned c = rg_lds[t];
        if (SCHEME) c += rg_lds[t + nb2] + rg_lds[t + 2 * nb2] + rg_lds[t + 3 * nb2];
        if (c) atomicAdd(&g[t], c);
    }
}
static_assert(RG_BY == 4 && RG_BX * RG_BY == RG_T, "the flush of scheme <1> adds four copies");

bool rg_apart(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x + na <= y || y + nb <= x;
}

}  // namespace

extern "C" int fibd_vol_halve(const float *in, int nx, int ny, int nz, int nframes, float *out, void *stream) try {
    FIB_CHECK(in && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(std::max({nx, ny, nz}) <= RG_MAX_DIM && nframes <= 65535, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24 or more than 65535 frames");
    const int ox = (nx + 1) / 2, oy = (ny + 1) / 2, oz = (nz + 1) / 2;
    const uint64_t nvi = (uint64_t)nx * ny * nz, nvo = (uint64_t)ox * oy * oz;
    FIB_CHECK(fib::cdiv((int64_t)nvo, RG_T) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the output volume needs 2^31 workgroups or more");
    FIB_CHECK(rg_apart(in, 4 * nvi * nframes, out, 4 * nvo * nframes), FIB_ERR_INVALID, "in and out must not overlap");
    fib::ProfScope prof("vol_halve", (hipStream_t)stream);
    hipLaunchKernelGGL(rg_halve_kernel, dim3((unsigned)fib::cdiv((int64_t)nvo, RG_T), (unsigned)nframes), dim3(RG_T), 0, (hipStream_t)stream, in, nx, ny,
                       nz, out, ox, oy, oz);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_vol_range(const float *vol, int64_t nvox, int nframes, int nbins, void *range, void *stream) try {
    FIB_CHECK(vol && range, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nvox > 0 && nframes > 0, FIB_ERR_INVALID, "nvox and nframes must be positive");
    FIB_CHECK(nbins >= FIB_REG_MIN_BINS && nbins <= FIB_REG_MAX_BINS, FIB_ERR_INVALID, "nbins %d outside %d..%d", nbins, FIB_REG_MIN_BINS, FIB_REG_MAX_BINS);
    FIB_CHECK(nvox < ((int64_t)1 << 32) && nframes <= 65535, FIB_ERR_UNSUPPORTED, "2^32 voxels or more in a frame, or more than 65535 frames");
    FIB_CHECK((reinterpret_cast<uintptr_t>(range) & 15) == 0, FIB_ERR_INVALID, "range must be 16-byte aligned");
    FIB_CHECK(rg_apart(vol, 4ull * (uint64_t)nvox * nframes, range, 16ull * nframes), FIB_ERR_INVALID, "vol and range must not overlap");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("vol_range", st);
    FIB_HIP(hipMemsetAsync(range, 0, 16ull * nframes, st));
    const unsigned nblk = (unsigned)std::min<int64_t>(fib::cdiv(nvox, RG_T * 8), 1024);
    hipLaunchKernelGGL(rg_minmax_kernel, dim3(nblk, (unsigned)nframes), dim3(RG_T), 0, st, vol, nvox, static_cast<unsigned *>(range));
    hipLaunchKernelGGL(rg_range_kernel, dim3((unsigned)fib::cdiv(nframes, 64)), dim3(64), 0, st, static_cast<unsigned *>(range), nframes, (float)nbins);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_reg_hist_work_size(int njobs, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(njobs > 0 && njobs <= FIB_REG_MAX_JOBS, FIB_ERR_INVALID, "njobs %d outside 1..%d", njobs, FIB_REG_MAX_JOBS);
    *bytes = sizeof(RegJob) * (size_t)njobs;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_reg_hist(const float *fixed, int nxf, int nyf, int nzf, const void *fixed_range, const float *moving, int nxm, int nym, int nzm,
                             int nframes, const void *moving_range, const int32_t *job_frame, const float *job_out2in, int njobs, int nbins,
                             uint32_t *hist, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(fixed && fixed_range && moving && moving_range && job_frame && job_out2in && hist && work, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nxf > 0 && nyf > 0 && nzf > 0 && nxm > 0 && nym > 0 && nzm > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(nbins >= FIB_REG_MIN_BINS && nbins <= FIB_REG_MAX_BINS, FIB_ERR_INVALID, "nbins %d outside %d..%d", nbins, FIB_REG_MIN_BINS, FIB_REG_MAX_BINS);
    size_t need = 0;
    FIB_RC(fibd_reg_hist_work_size(njobs, &need));
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "workspace of %zu bytes, fibd_reg_hist_work_size asks for %zu", work_bytes, need);
    FIB_CHECK(std::max({nxf, nyf, nzf, nxm, nym, nzm}) <= RG_MAX_DIM, FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    for (int j = 0; j < njobs; j++)
        FIB_CHECK(job_frame[j] >= 0 && job_frame[j] < nframes, FIB_ERR_INVALID, "job %d names frame %d of %d", j, (int)job_frame[j], nframes);
    const uintptr_t af = reinterpret_cast<uintptr_t>(fixed), am = reinterpret_cast<uintptr_t>(moving), ah = reinterpret_cast<uintptr_t>(hist);
    FIB_CHECK((af & 3) == 0 && (am & 3) == 0 && (ah & 3) == 0, FIB_ERR_INVALID, "volumes and hist must be 4-byte aligned");
    FIB_CHECK(((reinterpret_cast<uintptr_t>(fixed_range) | reinterpret_cast<uintptr_t>(moving_range)) & 15) == 0 &&
              (reinterpret_cast<uintptr_t>(work) & 7) == 0, FIB_ERR_INVALID, "ranges must be 16-byte and work 8-byte aligned");
    const uint64_t bf = 4ull * (uint64_t)nxf * nyf * nzf, bm = 4ull * (uint64_t)nxm * nym * nzm * nframes, bh = 4ull * (uint64_t)njobs * nbins * nbins;
    // everything the kernel reads while other workgroups add to hist
    FIB_CHECK(rg_apart(hist, bh, fixed, bf) && rg_apart(hist, bh, moving, bm) && rg_apart(hist, bh, work, need) && rg_apart(hist, bh, fixed_range, 16) &&
              rg_apart(hist, bh, moving_range, 16ull * nframes) && rg_apart(work, need, fixed, bf) && rg_apart(work, need, moving, bm) &&
              rg_apart(work, need, fixed_range, 16) && rg_apart(work, need, moving_range, 16ull * nframes),
              FIB_ERR_INVALID, "hist and work must not overlap the volumes, the ranges or each other");
    const unsigned nsx = (unsigned)fib::cdiv(nxf, RG_BX), nsy = (unsigned)fib::cdiv(nyf, RG_BY), nsz = (unsigned)fib::cdiv(nzf, RG_ZC);
    FIB_CHECK((int64_t)nsx * nsy * nsz < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the fixed volume needs 2^31 workgroups or more");
    int scheme = nbins <= RG_WAVE_COPIES_MAX_BINS ? 1 : 0;
    if (const char *e = fib::ab_env("FIBERS_REG_HIST_SCHEME")) scheme = (e[0] == 'b' || e[0] == '1') ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    std::vector<RegJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; j++) {
        memset(&jobs[j], 0, sizeof(RegJob));
        memcpy(jobs[j].m, job_out2in + 16 * (size_t)j, sizeof jobs[j].m);
        jobs[j].frame = job_frame[j];
    }
    fib::ProfScope prof("reg_hist", st);
    FIB_HIP(hipMemcpyAsync(work, jobs.data(), need, hipMemcpyHostToDevice, st));
    FIB_HIP(hipMemsetAsync(hist, 0, bh, st));
    const dim3 grid(nsx * nsy * nsz, 1, (unsigned)njobs), block(RG_T);
    const size_t lds = 4 * (size_t)nbins * nbins * (scheme ? RG_BY : 1);
    const RegRange *rf = static_cast<const RegRange *>(fixed_range), *rm = static_cast<const RegRange *>(moving_range);
    const RegJob *dj = static_cast<const RegJob *>(work);
    if (scheme) hipLaunchKernelGGL(rg_hist_kernel<1>, grid, block, lds, st, fixed, nxf, nyf, nzf, rf, moving, nxm, nym, nzm, rm, dj, nbins, hist, nsx, nsy);
    else hipLaunchKernelGGL(rg_hist_kernel<0>, grid, block, lds, st, fixed, nxf, nyf, nzf, rf, moving, nxm, nym, nzm, rm, dj, nbins, hist, nsx, nsy);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

// ---- the searches run to their end on device-resident volumes -------------------------------------------------------------------------
namespace {

// the workspace of fibd_reg_run: pyramid levels 1 .. levels - 1 of the fixed volume and of the moving series, a range table per level,
// the histograms and the job table of the largest launch (24 jobs a search)
struct RegLayout {
    int fs[4][3], ms[4][3];
    size_t fixed[4], moving[4], rf[4], rm[4], hist, jobs, total;
    RegLayout(const int32_t *fsize, const int32_t *msize, int nframes, int nsearch, int levels, int nbins) {
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
        for (int l = 0; l < levels; l++) {
            for (int c = 0; c < 3; c++) { fs[l][c] = l ? (fs[l - 1][c] + 1) / 2 : fsize[c]; ms[l][c] = l ? (ms[l - 1][c] + 1) / 2 : msize[c]; }
            fixed[l] = l ? take(4 * fvox(l)) : 0;
            moving[l] = l ? take(4 * mvox(l) * nframes) : 0;
            rf[l] = take(16);
            rm[l] = take(16 * (size_t)nframes);
        }
        hist = take(4 * (size_t)24 * nsearch * nbins * nbins);
        jobs = take(sizeof(RegJob) * (size_t)24 * nsearch);
        total = at;
    }
    size_t fvox(int l) const { return (size_t)fs[l][0] * fs[l][1] * fs[l][2]; }
    size_t mvox(int l) const { return (size_t)ms[l][0] * ms[l][1] * ms[l][2]; }
};

int rg_run_checks(const int32_t *fsize, const int32_t *msize, int nframes, int nsearch, int levels, int nbins) {
    FIB_CHECK(fsize && msize, FIB_ERR_INVALID, "NULL argument");
    for (int c = 0; c < 3; c++) FIB_CHECK(fsize[c] > 0 && msize[c] > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nframes > 0 && nframes <= 65535, FIB_ERR_INVALID, "nframes %d outside 1..65535", nframes);
    FIB_CHECK(nsearch > 0 && 24 * (int64_t)nsearch <= FIB_REG_MAX_JOBS, FIB_ERR_INVALID, "%d searches: one launch carries at most %d", nsearch, FIB_REG_MAX_JOBS / 24);
    FIB_CHECK(levels >= 1 && levels <= 4, FIB_ERR_INVALID, "levels must lie in 1 .. 4, not %d", levels);
    FIB_CHECK(nbins >= FIB_REG_MIN_BINS && nbins <= FIB_REG_MAX_BINS, FIB_ERR_INVALID, "nbins %d outside %d..%d", nbins, FIB_REG_MIN_BINS, FIB_REG_MAX_BINS);
    return FIB_OK;
}

}  // namespace

extern "C" int fibd_reg_run_work_size(const int32_t fixed_size[3], const int32_t moving_size[3], int nframes, int nsearch, int levels, int nbins,
                                      size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(rg_run_checks(fixed_size, moving_size, nframes, nsearch, levels, nbins));
    *bytes = RegLayout(fixed_size, moving_size, nframes, nsearch, levels, nbins).total;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_reg_run(fib_reg_search *const *searches, const int32_t *frames, int nsearch, const float *fixed, const int32_t fixed_size[3],
                            const float *moving, const int32_t moving_size[3], int nframes, int levels, int nbins, void *work, size_t work_bytes,
                            void *stream) try {
    FIB_CHECK(searches && frames && fixed && moving && work, FIB_ERR_INVALID, "NULL argument");
    FIB_RC(rg_run_checks(fixed_size, moving_size, nframes, nsearch, levels, nbins));
    for (int s = 0; s < nsearch; s++)
        FIB_CHECK(searches[s] && frames[s] >= 0 && frames[s] < nframes, FIB_ERR_INVALID, "search %d: a NULL handle, or frame %d of %d", s, (int)frames[s], nframes);
    const RegLayout lay(fixed_size, moving_size, nframes, nsearch, levels, nbins);
    FIB_CHECK(work_bytes >= lay.total && (reinterpret_cast<uintptr_t>(work) & 15) == 0, FIB_ERR_INVALID,
              "a 16-byte aligned workspace of fibd_reg_run_work_size = %zu bytes is needed, not %zu", lay.total, work_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(work);
    auto fx = [&](int l) { return l ? reinterpret_cast<const float *>(w + lay.fixed[l]) : fixed; };
    auto mv = [&](int l) { return l ? reinterpret_cast<const float *>(w + lay.moving[l]) : moving; };
    // the pyramids and the ranges; the ranges come back once: a volume without two distinct finite values is refused
    for (int l = 0; l < levels; l++) {
        if (l) {
            FIB_RC(fibd_vol_halve(fx(l - 1), lay.fs[l - 1][0], lay.fs[l - 1][1], lay.fs[l - 1][2], 1, reinterpret_cast<float *>(w + lay.fixed[l]), st));
            FIB_RC(fibd_vol_halve(mv(l - 1), lay.ms[l - 1][0], lay.ms[l - 1][1], lay.ms[l - 1][2], nframes, reinterpret_cast<float *>(w + lay.moving[l]), st));
        }
        FIB_RC(fibd_vol_range(fx(l), (int64_t)lay.fvox(l), 1, nbins, w + lay.rf[l], st));
        FIB_RC(fibd_vol_range(mv(l), (int64_t)lay.mvox(l), nframes, nbins, w + lay.rm[l], st));
    }
    int64_t nfinite[4];
    std::vector<RegRange> rng((size_t)nframes + 1);
    for (int l = 0; l < levels; l++) {
        FIB_HIP(hipMemcpyAsync(rng.data(), w + lay.rf[l], 16, hipMemcpyDeviceToHost, st));
        FIB_HIP(hipMemcpyAsync(rng.data() + 1, w + lay.rm[l], 16 * (size_t)nframes, hipMemcpyDeviceToHost, st));
        FIB_HIP(hipStreamSynchronize(st));
        for (int f = 0; f <= nframes; f++)
            FIB_CHECK(rng[f].scale == rng[f].scale && rng[f].hi != rng[f].lo, FIB_ERR_INVALID, "constant volume: %s at level %d has no two distinct finite values",
                      f ? "a moving frame" : "the fixed volume", l);
        nfinite[l] = rng[0].nfinite;
    }
    // every round: the searches that wait at the coarsest pending level put their jobs into one launch
    const size_t nb2 = (size_t)nbins * nbins;
    std::vector<float> mats((size_t)24 * 16 * nsearch), asked((size_t)24 * 16 * nsearch);
    std::vector<int32_t> jframe((size_t)24 * nsearch), owner((size_t)nsearch), count((size_t)nsearch), level((size_t)nsearch), nj((size_t)nsearch);
    std::vector<uint32_t> hist;
    std::vector<char> stale((size_t)nsearch, 1);             // a search's jobs stand until it is fed: only a fed search is asked again
    for (;;) {
        int top = -1;
        for (int s = 0; s < nsearch; s++) {
            if (stale[s]) {
                FIB_RC(fib_reg_search_jobs(searches[s], &level[s], &nj[s], asked.data() + (size_t)24 * 16 * s));
                if (nj[s]) FIB_CHECK(level[s] < levels, FIB_ERR_INVALID, "search %d asks for level %d of a pyramid of %d", s, (int)level[s], levels);
                stale[s] = 0;
            }
            if (nj[s] && level[s] > top) top = level[s];
        }
        if (top < 0) return FIB_OK;
        int njobs = 0, nown = 0;
        for (int s = 0; s < nsearch; s++) {
            if (!nj[s] || level[s] != top) continue;
            memcpy(mats.data() + 16 * (size_t)njobs, asked.data() + (size_t)24 * 16 * s, sizeof(float) * 16 * nj[s]);
            for (int j = 0; j < nj[s]; j++) jframe[njobs + j] = frames[s];
            owner[nown] = s; count[nown++] = nj[s];
            njobs += nj[s];
        }
        uint32_t *d_hist = reinterpret_cast<uint32_t *>(w + lay.hist);
        FIB_RC(fibd_reg_hist(fx(top), lay.fs[top][0], lay.fs[top][1], lay.fs[top][2], w + lay.rf[top], mv(top), lay.ms[top][0], lay.ms[top][1],
                             lay.ms[top][2], nframes, w + lay.rm[top], jframe.data(), mats.data(), njobs, nbins, d_hist, w + lay.jobs,
                             sizeof(RegJob) * (size_t)24 * nsearch, st));
        hist.resize(nb2 * njobs);
        FIB_HIP(hipMemcpyAsync(hist.data(), d_hist, 4 * nb2 * njobs, hipMemcpyDeviceToHost, st));
        FIB_HIP(hipStreamSynchronize(st));
        size_t at = 0;
        for (int o = 0; o < nown; o++) {
            FIB_RC(fib_reg_search_feed(searches[owner[o]], hist.data() + at, nbins, nfinite[top]));
            stale[owner[o]] = 1;
            at += nb2 * count[o];
        }
    }
} FIB_API_CATCH
