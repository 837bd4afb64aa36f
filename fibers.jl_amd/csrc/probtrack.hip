// probtrack.hip — probabilistic tractography from the ODF on gfx950: the quantised weight table of an ODF volume (fibd_prob_table),
// the cone plan of a direction set (fib_prob_plan_create) and the tracer (fibd_prob_run), with the host form fib_prob_stream.  Not in
// the reference: the definitions are the "Probabilistic tracking" section of include/fibers_hip.h.  Every sum of the definition is an
// integer sum and every float operation is rounded on its own, so that the output equals the NumPy restatement bit for bit.
//
// Kernels
//   pb_table<TV>      TV voxels per workgroup.  The planar ODF is read along the voxels (TV consecutive floats per vertex row) into an
//                     LDS tile [nvert][TV + 1]; per voxel the minimum, the clipped differences (written back into the tile) and their
//                     maximum; then the workgroup's TV rows, which are one contiguous span of the table, go out as 16-byte stores in
//                     thread order.  TV = 32 while the tile fits 64 KB of LDS (nvert <= PB_TV32_NVERT), else 16.
//   pb_trace<G, EMIT> G lanes per line (16 shipped; 64 = a wave per line, the A/B partner of the diagnostic build).  A row is cut into
//                     16-byte pieces of 8 weights; lane g holds pieces [g * cpl, (g + 1) * cpl), cpl = ceil(pitch / 8 / G) <= 4.  A step:
//                     the row of the voxel of nxt (kept in registers while the line stays in the voxel), AND with row j of the cone's
//                     bit table (LDS), the lanes' sums scanned over the group by shuffles, one 64-bit multiply for the draw, the lane
//                     that owns the draw finds the vertex, a ballot hands it to the group.  No arithmetic on directions: a direction
//                     is +-U[j] (LDS).  The loop runs until every line of the wave has ended; lines that have ended ride along masked.
//                     EMIT = false counts (nfwd, nbwd per line), EMIT = true replays a kept line and stores its points at their final
//                     place: the generator is counter-based, so the replay is exact and no scratch rows exist.
//   ls_block / ls_totals / ls_apply <PbItem>   (line_scan.inc) len_min and the exclusive scan of (kept lines, their points) between the passes
#include "common.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

// the definition rounds every product and sum on its own (include/fibers_hip.h): nothing in this file, host or device, may fuse a*b+c
#pragma clang fp contract(off)

struct fib_prob_plan {
    int device = 0, nvert = 0, nchunk = 0;                     // nchunk = pitch / 8: the 16-byte pieces (and cone bytes) of a row
    float cosang = 0.0f;
    fib::DevBuf<uint8_t> bits;                                 // allow [nvert][nchunk] bytes, then same [nvert][nchunk]; bit e of byte c: vertex 8c + e
    fib::DevBuf<float> U;                                      // [nvert][3]
};

namespace {

#include "line_scan.inc"                                       // LsVec, ls_scan, ls_check_work

constexpr int PB_BLOCK = 256;
constexpr int PB_NVERT_MAX = 512;
constexpr int PB_TV32_NVERT = 480;                            // 33 floats per vertex + the partials stay under 64 KB
constexpr int PB_LEN_MAX = 1 << 24;
constexpr size_t PB_HEAD_BYTES = 16;                           // {lines, points} as int64

__host__ __device__ __forceinline__ unsigned long long pb_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the generator of fibd_stream_trace_lcm, top 32 bits
__host__ __device__ __forceinline__ unsigned long long pb_u32(unsigned long long seed, unsigned long long line, unsigned k) {
    return pb_splitmix64(seed ^ pb_splitmix64(line * 0xD1342543DE82EF95ull + (unsigned long long)k)) >> 32;
}

// ---- table -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pb_quant(float w, float wmax, float thresh) {
    const float t = w / wmax;                                   // (IEEE division)
    if (t < thresh) return 0u;
    return (unsigned)floorf(t * 65535.0f);
}

template <int TV>
__global__ __launch_bounds__(PB_BLOCK) void pb_table(const float *__restrict__ odf, const uint8_t *__restrict__ mask, int64_t nvox, int nvert, int nchunk,
                                                     int subtract_min, float thresh, uint4 *__restrict__ table) {
    extern __shared__ float s_o[];                             // [nvert][TV + 1]
    __shared__ float s_part[PB_BLOCK];
    __shared__ float s_wmax[TV];
    constexpr int P = PB_BLOCK / TV, LD = TV + 1;
    const int t = threadIdx.x;
    const int64_t v0 = (int64_t)blockIdx.x * TV;
    for (int idx = t; idx < nvert * TV; idx += PB_BLOCK) {
        const int i = idx / TV, v = idx - i * TV;
        s_o[i * LD + v] = v0 + v < nvox ? odf[(int64_t)i * nvox + v0 + v] : 0.0f;
    }
    __syncthreads();
    const int v = t % TV, p = t / TV;
    float m = INFINITY;                                         // the minimum of the values that are not NaN (fminf drops a NaN)
    for (int i = p; i < nvert; i += P) m = fminf(m, s_o[i * LD + v]);
    s_part[t] = m;
    __syncthreads();
    for (int q = 0; q < P; q++) m = fminf(m, s_part[q * TV + v]);
    if (!subtract_min) m = 0.0f;
    __syncthreads();                                            // (s_part is written again)
    float wmax = 0.0f;
    for (int i = p; i < nvert; i += P) {
        float w = s_o[i * LD + v] - m;
        w = w > 0.0f ? w : 0.0f;                                // (a NaN fails the test)
        s_o[i * LD + v] = w;
        wmax = fmaxf(wmax, w);
    }
    s_part[t] = wmax;
    __syncthreads();
    if (p == 0) {
        for (int q = 1; q < P; q++) wmax = fmaxf(wmax, s_part[q * TV + v]);
        const bool live = wmax > 0.0f && wmax < INFINITY && v0 + v < nvox && (!mask || mask[v0 + v]);
        s_wmax[v] = live ? wmax : 0.0f;
    }
    __syncthreads();
    const int64_t c0 = v0 * nchunk, cend = (v0 + TV < nvox ? v0 + TV : nvox) * nchunk;     // the workgroup's rows are one span of the table
    for (int idx = t; c0 + idx < cend; idx += PB_BLOCK) {
        const int vv = idx / nchunk, c = idx - vv * nchunk;
        const float wm = s_wmax[vv];
        unsigned q[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int i = 8 * c + e;
            q[e] = (wm > 0.0f && i < nvert) ? pb_quant(s_o[i * LD + vv], wm, thresh) : 0u;
        }
        table[c0 + idx] = make_uint4(q[0] | q[1] << 16, q[2] | q[3] << 16, q[4] | q[5] << 16, q[6] | q[7] << 16);
    }
}

// ---- tracer ----------------------------------------------------------------------------------------------------------------------
struct PbArgs {
    int nx, ny, nz, nvert, nchunk, len_max, nsub;
    float step;
    unsigned long long rng_seed;
    int64_t nlines, nvox;
    const uint4 *table;
    const uint8_t *bits;                                       // allow, then same
    const float *U;
    const int64_t *seeds;
    const float *sublist;
    int32_t *counts;                                           // [nlines][2]: nfwd, nbwd
    const int64_t *lineoff, *ptoff;                            // EMIT: the place of a kept line (lineoff < 0: dropped)
    int32_t *npts;
    int64_t *seed_index;
    float *xyz;
};

__device__ __forceinline__ unsigned pb_w(const uint4 &r, int e) {
    const unsigned x = e < 2 ? r.x : e < 4 ? r.y : e < 6 ? r.z : r.w;
    return (e & 1) ? x >> 16 : x & 0xFFFFu;
}

// the masked weights of a lane, pieces in order: their sum
template <int CPL>
__device__ __forceinline__ unsigned pb_lane_sum(const uint4 (&raw)[CPL], const unsigned (&msk)[CPL]) {
    unsigned sum = 0;
#pragma unroll
    for (int c = 0; c < CPL; c++)
#pragma unroll
        for (int e = 0; e < 8; e++) sum += (msk[c] >> e & 1u) ? pb_w(raw[c], e) : 0u;
    return sum;
}
// the first vertex of the lane whose running sum, started at `run`, exceeds r (the lane that owns r has one); -1 otherwise
template <int CPL>
__device__ __forceinline__ int pb_lane_pick(const uint4 (&raw)[CPL], const unsigned (&msk)[CPL], unsigned run, unsigned r, int first_chunk) {
    int pick = -1;
#pragma unroll
    for (int c = 0; c < CPL; c++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            run += (msk[c] >> e & 1u) ? pb_w(raw[c], e) : 0u;
            if (pick < 0 && run > r) pick = 8 * (first_chunk + c) + e;
        }
    return pick;
}

// One draw by the group: the lanes' sums scanned over the group, Q, and -- when Q > 0 and `want` -- the pick for the uniform u.
// Every lane of the wave comes through here together (shuffles and a ballot).
template <int G, int CPL>
__device__ __forceinline__ void pb_draw(const uint4 (&raw)[CPL], const unsigned (&msk)[CPL], int g, int first_chunk, unsigned long long u, unsigned &Q, int &pick) {
    const unsigned mine = pb_lane_sum<CPL>(raw, msk);
    unsigned inc = mine;
#pragma unroll
    for (int d = 1; d < G; d <<= 1) { const unsigned o = __shfl_up(inc, d, G); if (g >= d) inc += o; }
    Q = __shfl(inc, G - 1, G);
    const unsigned r = (unsigned)((u * (unsigned long long)Q) >> 32);      // < Q
    const unsigned exc = inc - mine;
    const bool owner = Q > 0 && exc <= r && r < inc;
    const int cand = pb_lane_pick<CPL>(raw, msk, exc, r, first_chunk);
    const unsigned long long b = __ballot(owner);
    const int lane = threadIdx.x & 63, base = lane & ~(G - 1);
    const unsigned long long mine_b = G == 64 ? b : (b >> base) & ((1ull << (G & 63)) - 1ull);
    const int src = mine_b ? __builtin_ctzll(mine_b) : 0;
    pick = __shfl(cand, src, G);
}

template <int G, int CPL, bool EMIT>
__global__ __launch_bounds__(PB_BLOCK) void pb_trace(const PbArgs a) {
    extern __shared__ unsigned char s_raw[];
    float *s_U = reinterpret_cast<float *>(s_raw);             // [nvert][3]
    uint8_t *s_allow = s_raw + sizeof(float) * 3 * a.nvert;    // [nvert][nchunk]
    for (int w = threadIdx.x; w < 3 * a.nvert; w += PB_BLOCK) s_U[w] = a.U[w];
    for (int w = threadIdx.x; w < a.nvert * a.nchunk / 4; w += PB_BLOCK)       // (nchunk is a multiple of 8)
        reinterpret_cast<uint32_t *>(s_allow)[w] = reinterpret_cast<const uint32_t *>(a.bits)[w];
    __syncthreads();
    const uint8_t *same_bits = a.bits + (size_t)a.nvert * a.nchunk;

    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * PB_BLOCK + threadIdx.x) / G;
    const int first_chunk = g * CPL;
    bool live = line < a.nlines;
    int64_t out0 = 0;
    int nfwd_total = 0;
    if (EMIT && live) {
        const int64_t lo = a.lineoff[line];
        live = lo >= 0;
        if (live) {
            out0 = a.ptoff[line];
            nfwd_total = a.counts[2 * line];
            if (g == 0) { a.npts[lo] = nfwd_total + a.counts[2 * line + 1]; a.seed_index[lo] = line; }
        }
    }
    int64_t seed = 0;
    int sub = 0;
    if (live) {
        seed = a.seeds[line / a.nsub];
        sub = (int)(line % a.nsub);
        live = seed >= 0 && seed < a.nvox;                      // (a seed outside the volume has no points)
    }
    float p0x = 0.0f, p0y = 0.0f, p0z = 0.0f;
    if (live) {
        const int64_t sx = seed % a.nx, sy = (seed / a.nx) % a.ny, sz = seed / ((int64_t)a.nx * a.ny);
        p0x = (float)(sx + 1) + a.sublist[3 * sub];
        p0y = (float)(sy + 1) + a.sublist[3 * sub + 1];
        p0z = (float)(sz + 1) + a.sublist[3 * sub + 2];
    }
    uint4 raw[CPL];
    unsigned msk[CPL];
    int64_t curvox = live ? seed : -1;
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        const bool have = live && first_chunk + c < a.nchunk;
        raw[c] = have ? a.table[curvox * a.nchunk + first_chunk + c] : make_uint4(0, 0, 0, 0);
        msk[c] = have ? 0xFFu : 0u;
    }
    unsigned k = 0, Q;
    int j0;
    pb_draw<G, CPL>(raw, msk, g, first_chunk, pb_u32(a.rng_seed, (unsigned long long)line, 0), Q, j0);
    live = live && Q > 0;                                       // (a seed on a zero row has no points)
    k = 1;
    int phase = live ? 0 : 2;                                   // 0 forward, 1 backward, 2 ended
    float px = p0x, py = p0y, pz = p0z, s = 1.0f;
    int j = live ? j0 : 0, npts = 0, nf = 0, nb = 0;
    while (__any(phase < 2)) {
        const bool act = phase < 2;
        const float nxtx = px + (s * s_U[3 * j]) * a.step, nxty = py + (s * s_U[3 * j + 1]) * a.step, nxtz = pz + (s * s_U[3 * j + 2]) * a.step;
        const float vx = rintf(nxtx), vy = rintf(nxty), vz = rintf(nxtz);
        const bool ok = act && vx >= 1.0f && vx <= (float)a.nx && vy >= 1.0f && vy <= (float)a.ny && vz >= 1.0f && vz <= (float)a.nz;
        if (ok) {
            const int64_t vox = (int64_t)((int)vx - 1) + (int64_t)a.nx * (((int)vy - 1) + (int64_t)a.ny * ((int)vz - 1));
            if (vox != curvox) {
                curvox = vox;
#pragma unroll
                for (int c = 0; c < CPL; c++)
                    if (first_chunk + c < a.nchunk) raw[c] = a.table[vox * a.nchunk + first_chunk + c];
            }
        }
#pragma unroll
        for (int c = 0; c < CPL; c++) msk[c] = (ok && first_chunk + c < a.nchunk) ? s_allow[j * a.nchunk + first_chunk + c] : 0u;
        int pick;
        pb_draw<G, CPL>(raw, msk, g, first_chunk, pb_u32(a.rng_seed, (unsigned long long)line, k), Q, pick);
        bool end = act;
        if (ok && Q > 0) {                                      // (no draw is consumed otherwise)
            k++;
            if (!(same_bits[j * a.nchunk + (pick >> 3)] >> (pick & 7) & 1)) s = -s;
            j = pick;
            npts++;
            int64_t at;
            if (phase == 0) { nf++; at = out0 + nfwd_total - nf; } else { nb++; at = out0 + nfwd_total + nb - 1; }
            if (EMIT && g == 0) { a.xyz[3 * at] = px; a.xyz[3 * at + 1] = py; a.xyz[3 * at + 2] = pz; }
            end = npts > a.len_max;
            px = nxtx; py = nxty; pz = nxtz;
        }
        if (end) {
            phase++;
            px = p0x; py = p0y; pz = p0z; s = -1.0f; j = j0;
        }
    }
    if (!EMIT && g == 0 && line < a.nlines) { a.counts[2 * line] = nf; a.counts[2 * line + 1] = nb; }
}

// ---- len_min and the offsets -----------------------------------------------------------------------------------------------------
// the scan of (kept lines, their points): a line is kept when it has at least len_min points.  lineoff is -1 for a dropped line; ptoff
// is written for every line.  Nothing is refused; head = {lines, points}.
struct PbItem {
    static constexpr int N = 2;
    const int32_t *counts;
    int len_min;
    int64_t *lineoff, *ptoff, *head;
    __device__ LsVec<2> load(int64_t l, bool &) const {
        const int n = counts[2 * l] + counts[2 * l + 1];
        const bool kept = n >= len_min;
        return {kept ? 1 : 0, kept ? n : 0};
    }
    __device__ void store(int64_t l, const LsVec<2> &run, const LsVec<2> &mine) const {
        lineoff[l] = mine.v[0] ? run.v[0] : -1;
        ptoff[l] = run.v[1];
    }
    __device__ void verdict(const LsVec<2> &grand, bool) const { head[0] = grand.v[0]; head[1] = grand.v[1]; }
    __device__ bool go() const { return true; }
};

// the work area: counts int32 [nlines][2] | lineoff int64 [nlines] | ptoff int64 [nlines] | head int64 [2] | block totals int64 [nblocks][2]
struct PbWork {
    int32_t *counts;
    int64_t *lineoff, *ptoff, *head;
    LsVec<2> *totals;
};
size_t pb_work_bytes(int64_t nlines) {
    const size_t n = (size_t)std::max<int64_t>(nlines, 1);
    return 8 * n + 8 * n + 8 * n + PB_HEAD_BYTES + sizeof(LsVec<2>) * (size_t)ls_total_slots(nlines);
}
PbWork pb_work(void *work, int64_t nlines) {
    const size_t n = (size_t)std::max<int64_t>(nlines, 1);
    PbWork w;
    char *p = reinterpret_cast<char *>(work);
    w.counts = reinterpret_cast<int32_t *>(p);
    w.lineoff = reinterpret_cast<int64_t *>(p + 8 * n);
    w.ptoff = w.lineoff + n;
    w.head = w.ptoff + n;
    w.totals = reinterpret_cast<LsVec<2> *>(w.head + 2);
    return w;
}

// lanes per line: 16; the diagnostic build's A/B switch FIBERS_PROB_LANES=64 selects a wave per line
int pb_lanes() {
    const char *e = fib::ab_env("FIBERS_PROB_LANES");
    return e && atoi(e) == 64 ? 64 : 16;
}

template <int G, int CPL>
void pb_launch(bool emit, const PbArgs &a, hipStream_t st) {
    const unsigned grid = (unsigned)fib::cdiv(a.nlines * G, PB_BLOCK);
    const size_t lds = sizeof(float) * 3 * a.nvert + (size_t)a.nvert * a.nchunk;
    if (emit) hipLaunchKernelGGL((pb_trace<G, CPL, true>), dim3(grid), dim3(PB_BLOCK), lds, st, a);
    else hipLaunchKernelGGL((pb_trace<G, CPL, false>), dim3(grid), dim3(PB_BLOCK), lds, st, a);
}
void pb_trace_launch(bool emit, const PbArgs &a, hipStream_t st) {
    if (pb_lanes() == 64) return pb_launch<64, 1>(emit, a, st);
    switch ((int)fib::cdiv(a.nchunk, 16)) {
        case 1: return pb_launch<16, 1>(emit, a, st);
        case 2: return pb_launch<16, 2>(emit, a, st);
        case 3: return pb_launch<16, 3>(emit, a, st);
        default: return pb_launch<16, 4>(emit, a, st);
    }
}

int pb_check(const fib::ProbRun &r, void *work, size_t work_bytes) {
    FIB_CHECK(r.plan && r.table && r.sublist, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(r.nx > 0 && r.ny > 0 && r.nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(r.nx <= (1 << 24) && r.ny <= (1 << 24) && r.nz <= (1 << 24), FIB_ERR_UNSUPPORTED, "a volume dimension above 2^24");
    FIB_CHECK(r.nseed >= 0 && (r.nseed == 0 || r.seeds), FIB_ERR_INVALID, "NULL seeds or a negative nseed");
    FIB_CHECK(r.nsub >= 1, FIB_ERR_INVALID, "sublist must hold at least one offset");
    FIB_CHECK(r.len_min >= 0 && r.len_max >= 0 && r.len_max <= PB_LEN_MAX, FIB_ERR_INVALID, "len_min >= 0 and 0 <= len_max <= 2^24 are required");
    FIB_CHECK(r.step == r.step, FIB_ERR_INVALID, "step_size is NaN");
    FIB_CHECK((reinterpret_cast<uintptr_t>(r.table) & 15) == 0, FIB_ERR_INVALID, "table must be 16-byte aligned");
    FIB_CHECK(r.nseed < ((int64_t)1 << 40) / r.nsub, FIB_ERR_UNSUPPORTED, "too many lines");
    const int64_t nlines = r.nseed * r.nsub;
    FIB_CHECK(fib::cdiv(nlines * 64, PB_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    return ls_check_work(work, work_bytes, pb_work_bytes(nlines), "fibd_prob_work_size");
}

PbArgs pb_args(const fib::ProbRun &r, const PbWork &w) {
    PbArgs a{};
    a.nx = r.nx; a.ny = r.ny; a.nz = r.nz; a.nvert = r.plan->nvert; a.nchunk = r.plan->nchunk; a.len_max = r.len_max; a.nsub = r.nsub;
    a.step = r.step; a.rng_seed = r.rng_seed; a.nlines = r.nseed * r.nsub; a.nvox = (int64_t)r.nx * r.ny * r.nz;
    a.table = reinterpret_cast<const uint4 *>(r.table); a.bits = r.plan->bits.p; a.U = r.plan->U.p; a.seeds = r.seeds; a.sublist = r.sublist;
    a.counts = w.counts; a.lineoff = w.lineoff; a.ptoff = w.ptoff;
    return a;
}

}  // namespace

size_t fib::prob_work_bytes(int64_t nlines) { return pb_work_bytes(nlines); }

int fib::prob_count(const ProbRun &r, void *work, size_t work_bytes, hipStream_t st, int64_t *nlines_out, int64_t *npoints_out) {
    FIB_RC(pb_check(r, work, work_bytes));
    const int64_t nlines = r.nseed * r.nsub;
    const PbWork w = pb_work(work, nlines);
    if (nlines > 0) {
        fib::ProfScope prof("prob_trace_count", st);
        pb_trace_launch(false, pb_args(r, w), st);
    }
    ls_scan(PbItem{w.counts, r.len_min, w.lineoff, w.ptoff, w.head}, nlines, w.totals, st);
    FIB_HIP(hipGetLastError());
    int64_t head[2] = {0, 0};
    FIB_HIP(hipMemcpyAsync(head, w.head, sizeof head, hipMemcpyDeviceToHost, st));
    FIB_HIP(hipStreamSynchronize(st));
    *nlines_out = head[0]; *npoints_out = head[1];
    return FIB_OK;
}

int fib::prob_emit(const ProbRun &r, void *work, int32_t *npts, int64_t *seed_index, float *xyz, hipStream_t st) {
    if (r.nseed * r.nsub == 0) return FIB_OK;
    PbArgs a = pb_args(r, pb_work(work, r.nseed * r.nsub));
    a.npts = npts; a.seed_index = seed_index; a.xyz = xyz;
    fib::ProfScope prof("prob_trace_emit", st);
    pb_trace_launch(true, a, st);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

extern "C" int fib_prob_row_pitch(int nvert) {
    return nvert >= 1 && nvert <= PB_NVERT_MAX ? 64 * ((nvert + 63) / 64) : 0;
}

extern "C" int fibd_prob_table(const float *odf, const uint8_t *mask, int64_t nvox, int nvert, int subtract_min, float pmf_thresh, uint16_t *table,
                               void *stream) try {
    FIB_CHECK(nvert >= 1 && nvert <= PB_NVERT_MAX, FIB_ERR_UNSUPPORTED, "1 to %d directions, not %d", PB_NVERT_MAX, nvert);
    FIB_CHECK(nvox >= 0, FIB_ERR_INVALID, "nvox must not be negative");
    FIB_CHECK(nvox == 0 || (odf && table), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK((reinterpret_cast<uintptr_t>(odf) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0, FIB_ERR_INVALID,
              "odf must be 4-byte and table 16-byte aligned");
    FIB_CHECK(nvox < ((int64_t)1 << 34), FIB_ERR_UNSUPPORTED, "too many voxels");
    if (nvox == 0) return FIB_OK;
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("prob_table", st);
    const int nchunk = fib_prob_row_pitch(nvert) / 8;
    if (nvert <= PB_TV32_NVERT)
        hipLaunchKernelGGL(pb_table<32>, dim3((unsigned)fib::cdiv(nvox, 32)), dim3(PB_BLOCK), sizeof(float) * 33 * nvert, st, odf, mask, nvox, nvert, nchunk,
                           subtract_min, pmf_thresh, reinterpret_cast<uint4 *>(table));
    else
        hipLaunchKernelGGL(pb_table<16>, dim3((unsigned)fib::cdiv(nvox, 16)), dim3(PB_BLOCK), sizeof(float) * 17 * nvert, st, odf, mask, nvox, nvert, nchunk,
                           subtract_min, pmf_thresh, reinterpret_cast<uint4 *>(table));
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_prob_plan_create(int device, const float *vertices, int nvert, float cosang_thresh, fib_prob_plan **plan) try {
    FIB_CHECK(plan && vertices, FIB_ERR_INVALID, "NULL argument");
    *plan = nullptr;
    FIB_CHECK(nvert >= 1 && nvert <= PB_NVERT_MAX, FIB_ERR_UNSUPPORTED, "1 to %d directions, not %d", PB_NVERT_MAX, nvert);
    FIB_CHECK(cosang_thresh > 0.0f, FIB_ERR_INVALID, "cosang_thresh must be > 0 (an angle below 90 degrees): the cone is the only bend limit");
    fib::DeviceGuard guard;
    FIB_RC(fib::use_device(device));
    std::unique_ptr<fib_prob_plan> p(new fib_prob_plan());
    p->device = device; p->nvert = nvert; p->nchunk = fib_prob_row_pitch(nvert) / 8; p->cosang = cosang_thresh;
    const size_t half = (size_t)nvert * p->nchunk;
    std::vector<uint8_t> bits(2 * half, 0);
    for (int j = 0; j < nvert; j++)
        for (int i = 0; i < nvert; i++) {
            const float *a = vertices + 3 * j, *b = vertices + 3 * i;
            const float c = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
            if (fabsf(c) >= cosang_thresh) bits[(size_t)j * p->nchunk + (i >> 3)] |= (uint8_t)(1u << (i & 7));
            if (c > 0.0f) bits[half + (size_t)j * p->nchunk + (i >> 3)] |= (uint8_t)(1u << (i & 7));
        }
    FIB_RC(fib::upload(p->bits, bits));
    FIB_RC(fib::upload(p->U, vertices, (size_t)3 * nvert));
    *plan = p.release();
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fib_prob_plan_destroy(fib_prob_plan *plan) try { fib::plan_destroy(plan); } FIB_API_CATCH_VOID

extern "C" int fibd_prob_work_size(int64_t nlines, size_t *bytes) try {
    FIB_CHECK(bytes && nlines >= 0, FIB_ERR_INVALID, "NULL bytes or negative nlines");
    *bytes = fib::prob_work_bytes(nlines);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_prob_run(const fib_prob_plan *plan, int nx, int ny, int nz, int32_t len_min, int32_t len_max, float step_size, const uint16_t *table,
                             const int64_t *seeds, int64_t nseed, const float *sublist, int32_t nsub, uint64_t rng_seed, int32_t *npts,
                             int64_t *seed_index, int64_t lines_cap, float *xyz, int64_t points_cap, int64_t *nlines, int64_t *npoints, void *work,
                             size_t work_bytes, void *stream) try {
    FIB_CHECK(nlines && npoints, FIB_ERR_INVALID, "NULL nlines / npoints");
    *nlines = 0; *npoints = 0;
    const fib::ProbRun r{plan, nx, ny, nz, len_min, len_max, nsub, step_size, table, seeds, nseed, sublist, rng_seed};
    hipStream_t st = (hipStream_t)stream;
    FIB_RC(fib::prob_count(r, work, work_bytes, st, nlines, npoints));
    FIB_CHECK(lines_cap >= 0 && points_cap >= 0, FIB_ERR_INVALID, "negative capacity");
    FIB_CHECK((lines_cap == 0 || (npts && seed_index)) && (points_cap == 0 || xyz), FIB_ERR_INVALID, "NULL output buffer");
    FIB_CHECK((reinterpret_cast<uintptr_t>(xyz) & 3) == 0, FIB_ERR_INVALID, "xyz must be 4-byte aligned");
    if (*nlines > lines_cap || *npoints > points_cap)
        return fib::fail(FIB_ERR_CAPACITY, "fibd_prob_run needs room for %lld lines and %lld points (capacities: %lld, %lld); nothing was written",
                         (long long)*nlines, (long long)*npoints, (long long)lines_cap, (long long)points_cap);
    FIB_RC(fib::prob_emit(r, work, npts, seed_index, xyz, st));
    FIB_HIP(hipStreamSynchronize(st));
    return FIB_OK;
} FIB_API_CATCH
