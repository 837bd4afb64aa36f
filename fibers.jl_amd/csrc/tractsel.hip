// tractsel.hip — choosing lines of a tractogram and counting what they connect, on gfx950: the ROI bit volume (fibd_str_roi_pack),
// per-line ROI predicates and the keep rule (fibd_str_select), stable compaction of the kept lines (fibd_str_gather) and the
// node-by-node matrix of line counts and summed lengths from a label volume (fibd_str_connectome).  Not in the reference: the
// definitions are the "Tract selection and connectomes" section of include/fibers_hip.h.  Inputs are packed lines as for the tract
// maps (tractmap.hip): xyz float32 [npoints][3] (any 4-byte boundary), npts int32 [nlines]; the voxel of a point and the offset scan
// with its verdict on npts are the ones of tm_lines.inc.
//
// Kernels
//   ts_roi_pack       a lane per voxel: bit r of the word = (ROI r is non-zero there)
//   ts_select<G>      a workgroup takes 256 consecutive lines.  G rounds: G lanes per line, each lane strides over the line's points and
//                     gathers the 4-byte ROI word of the point's voxel; an OR butterfly over the group gives {visit, end0, end1}, kept
//                     in LDS.  Then a lane per line evaluates the rule and writes keep / hits as consecutive elements; kept lines and
//                     points are summed over the workgroup, then one 64-bit atomic each
//   ls_block / ls_totals / ls_apply <TsItem>   (line_scan.inc) ONE exclusive scan of three int64 sums per line (points so far, kept
//                     lines so far, points of kept lines so far); the totals kernel judges npts AND the capacities and publishes
//                     totals, status and the go-ahead in device memory.  <TmItem> (tm_lines.inc): the offset scan of select and connectome
//   ts_gather_copy<G> G lanes per line; a kept line's points (and scalar rows) are copied as 32-bit words to their output offset
//   ts_connectome<G>  256 consecutive lines per workgroup and at the end a lane per line: two point loads, two label gathers, the remap
//                     gathers, the atomics.  G = 1 (no W): that is all, and lanes of a wave that add to the same cell are merged into
//                     one add.  G = 16 (W asked for): before it, 16 rounds in which 16 lanes per line sum the line's length in float64
//                     exactly as tm_stats does, into LDS; the lane of the line adds it with atomicAdd on double
#include "common.h"

#include <algorithm>

// a line's length is defined as float64 operations rounded one by one (include/fibers_hip.h): nothing in this file may fuse a*b+c
#pragma clang fp contract(off)

namespace {

#include "tm_lines.inc"                                        // TM_BLOCK, TmHead, tm_voxel, the offset scan (tm_offsets), tm_check_lines; line_scan.inc

constexpr int TS_SELECT_G = 16;                                // lanes per line of ts_select (profiles/tract_select/README.md)
constexpr int TS_GATHER_G = 64;                                // lanes per line of ts_gather_copy: 256 B per round
constexpr int TS_LENGTH_G = 16;                                // lanes per line of ts_connectome when W is asked for (tm_stats' mapping)

// ---- ROI bits --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_BLOCK) void ts_roi_pack(const uint8_t *rois, int nroi, int64_t nvox, uint32_t *roibits) {
    const int64_t v = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (v >= nvox) return;
    uint32_t bits = 0;
    for (int r = 0; r < nroi; r++) bits |= (rois[(int64_t)r * nvox + v] != 0 ? 1u : 0u) << r;
    roibits[v] = bits;
}

// sum over the workgroup of a per-lane (lines, points) pair; the result is valid in thread 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ void ts_block_sum(int &lines, int64_t &points) {
    __shared__ int s_l[TM_BLOCK / 64];
    __shared__ int64_t s_p[TM_BLOCK / 64];
    for (int d = 32; d >= 1; d >>= 1) { lines += __shfl_xor(lines, d); points += __shfl_xor(points, d); }
    if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = lines; s_p[threadIdx.x >> 6] = points; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lines = 0; points = 0;
        for (int w = 0; w < TM_BLOCK / 64; w++) { lines += s_l[w]; points += s_p[w]; }
    }
}

__device__ __forceinline__ void ts_add64(int64_t *p, int64_t n) {
    if (n) atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)n);
}

// ---- select ----------------------------------------------------------------------------------------------------------------------
struct TsRule {
    uint32_t visit_all, visit_none, end_any, end_both;
    int32_t min_npts, max_npts;
};

// A workgroup takes TM_BLOCK consecutive lines.  Phase 1, G rounds: in round r the group of G lanes q takes line r * (TM_BLOCK / G) + q,
// strides over its points and ORs the predicates over the group; they go to LDS.  Phase 2: a lane per line evaluates the rule and
// writes keep / hits (consecutive lanes, consecutive lines); one pair of 64-bit atomics per workgroup.
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void ts_select(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines, int nx, int ny, int nz,
                                                      const uint32_t *roibits, TsRule rule, const TmHead *head, uint8_t *keep, uint32_t *hits,
                                                      int64_t *counts) {
    __shared__ uint32_t s_hits[3][TM_BLOCK];
    constexpr int PER_ROUND = TM_BLOCK / G;
    const bool ok = head->ok != 0;                              // (uniform over the grid)
    const int g = threadIdx.x % G, grp = threadIdx.x / G;
    const int64_t line0 = (int64_t)blockIdx.x * TM_BLOCK;
    for (int r = 0; r < G; r++) {
        const int slot = r * PER_ROUND + grp;
        int n = 0;
        int64_t first = 0;
        if (ok && roibits && line0 + slot < nlines) { n = npts[line0 + slot]; first = off[line0 + slot]; }
        uint32_t visit = 0, end0 = 0, end1 = 0;
        for (int k = g; k < n; k += G) {
            const int64_t v = tm_voxel_at(xyz, first + k, nx, ny, nz);
            const uint32_t b = v >= 0 ? roibits[v] : 0u;
            visit |= b;
            if (k == 0) end0 = b;
            if (k == n - 1) end1 = b;
        }
        for (int d = G / 2; d >= 1; d >>= 1) {
            visit |= __shfl_xor(visit, d, G);
            end0 |= __shfl_xor(end0, d, G);
            end1 |= __shfl_xor(end1, d, G);
        }
        if (g == 0) { s_hits[0][slot] = visit; s_hits[1][slot] = end0; s_hits[2][slot] = end1; }
    }
    __syncthreads();
    const int64_t line = line0 + threadIdx.x;
    int kept_lines = 0;
    int64_t kept_points = 0;
    if (line < nlines) {
        bool k = false;
        if (ok) {
            const int n = npts[line];
            const uint32_t visit = s_hits[0][threadIdx.x], end0 = s_hits[1][threadIdx.x], end1 = s_hits[2][threadIdx.x];
            k = (visit & rule.visit_all) == rule.visit_all && (visit & rule.visit_none) == 0 && ((end0 | end1) & rule.end_any) == rule.end_any &&
                (end0 & end1 & rule.end_both) == rule.end_both && rule.min_npts <= n && (rule.max_npts == 0 || n <= rule.max_npts);
            if (hits) { hits[3 * line] = visit; hits[3 * line + 1] = end0; hits[3 * line + 2] = end1; }
            if (k) { kept_lines = 1; kept_points = n; }
        }
        keep[line] = k ? 1 : 0;                                 // (a refused input: zero-filled)
    }
    ts_block_sum(kept_lines, kept_points);
    if (threadIdx.x == 0) {
        if (ok) { ts_add64(counts, kept_lines); ts_add64(counts + 1, kept_points); }
        else if (blockIdx.x == 0) counts[0] = counts[1] = -1;
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------
// per line: the points of the lines before it, the kept lines before it, the points of the kept lines before it
struct Ts3 {
    int64_t in, ln, pt;
};
static_assert(sizeof(Ts3) == sizeof(LsVec<3>), "off3 and the block totals share the work area's element size");

// the scan of (points, kept lines, kept points).  Refused: a negative count, a sum that is not npoints, or more than a capacity holds;
// counts = {kept lines, kept points, status}, and head->ok is the go-ahead of the copy: valid AND within both capacities.
struct TsItem {
    static constexpr int N = 3;
    const int32_t *npts;
    const uint8_t *keep;
    int64_t npoints, cap_lines, cap_points;
    TmHead *head;
    Ts3 *off3;
    int64_t *counts;
    __device__ LsVec<3> load(int64_t l, bool &bad) const {
        const int32_t c = npts[l];
        const bool k = keep[l] != 0;
        bad |= c < 0;
        return {c, k ? 1 : 0, k ? c : 0};
    }
    __device__ void store(int64_t l, const LsVec<3> &run, const LsVec<3> &) const { off3[l] = Ts3{run.v[0], run.v[1], run.v[2]}; }
    __device__ void verdict(const LsVec<3> &grand, bool bad) const {
        const bool valid = !bad && grand.v[0] == npoints;
        const bool fits = grand.v[1] <= cap_lines && grand.v[2] <= cap_points;
        head->ok = valid && fits ? 1 : 0;
        counts[0] = valid ? grand.v[1] : -1;
        counts[1] = valid ? grand.v[2] : -1;
        counts[2] = valid && !fits ? -1 : 0;
    }
    __device__ bool go() const { return head->ok != 0; }
};

// G lanes per line.  Everything is copied as 32-bit words: NaN payloads and -0.0 arrive as they left.
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void ts_gather_copy(const uint32_t *xyz, const int32_t *npts, const uint8_t *keep, const Ts3 *off3, int64_t nlines,
                                                           const uint32_t *scalars, int ns, const TmHead *head, uint32_t *xyz_out, int32_t *npts_out,
                                                           int64_t *index_out, uint32_t *scalars_out) {
    if (!head->ok) return;
    const int g = threadIdx.x % G;
    const int64_t line = ((int64_t)blockIdx.x * TM_BLOCK + threadIdx.x) / G;
    if (line >= nlines || !keep[line]) return;                  // (whole groups leave together)
    const Ts3 o = off3[line];
    const int n = npts[line];
    if (g == 0) {
        npts_out[o.ln] = n;
        if (index_out) index_out[o.ln] = line;
    }
    const uint32_t *src = xyz + 3 * o.in;
    uint32_t *dst = xyz_out + 3 * o.pt;
    const int64_t nw = (int64_t)3 * n;
    for (int64_t w = g; w < nw; w += G) dst[w] = src[w];
    if (scalars_out) {
        const uint32_t *ssrc = scalars + (int64_t)ns * o.in;
        uint32_t *sdst = scalars_out + (int64_t)ns * o.pt;
        const int64_t nsw = (int64_t)ns * n;
        for (int64_t w = g; w < nsw; w += G) sdst[w] = ssrc[w];
    }
}

// ---- connectome ------------------------------------------------------------------------------------------------------------------
// node of a line end: 0 outside the volume; else labels[v], through remap if there is one, and 0 unless 1 <= y <= L
__device__ __forceinline__ int ts_node(const float *xyz, int64_t p, int nx, int ny, int nz, const int32_t *labels, const int32_t *remap, int64_t nremap,
                                       int L) {
    const int64_t v = tm_voxel_at(xyz, p, nx, ny, nz);
    if (v < 0) return 0;
    int y = labels[v];
    if (remap) y = y >= 0 && y < nremap ? remap[y] : 0;
    return y >= 1 && y <= L ? y : 0;
}

// A workgroup takes TM_BLOCK consecutive lines.  With W (G > 1), phase 1 as in ts_select: G rounds, a group of G lanes per line sums the
// line's length (the terms of tm_stats' column 0, kept in float64) into LDS.  Then a lane per line: the nodes of its two ends and the
// atomics.  Without W, lanes of a wave that add to the same cell of C are merged into one add (neighbouring lines mostly join the
// same two nodes, and adds to one address queue up behind each other).
template <int G>
__global__ __launch_bounds__(TM_BLOCK) void ts_connectome(const float *xyz, const int32_t *npts, const int64_t *off, int64_t nlines, int nx, int ny, int nz,
                                                          float rx, float ry, float rz, const int32_t *labels, const int32_t *remap, int64_t nremap, int L,
                                                          const TmHead *head, uint32_t *C, double *W, int32_t *assign, int64_t *n_lines) {
    __shared__ double s_len[G > 1 ? TM_BLOCK : 1];
    if (!head->ok) return;                                      // (uniform over the grid: nothing is added for a refused input)
    const int64_t line0 = (int64_t)blockIdx.x * TM_BLOCK;
    if (G > 1) {
        constexpr int PER_ROUND = TM_BLOCK / G;
        const int g = threadIdx.x % G, grp = threadIdx.x / G;
        const double dx = (double)rx, dy = (double)ry, dz = (double)rz;
        for (int r = 0; r < G; r++) {
            const int slot = r * PER_ROUND + grp;
            int n = 0;
            int64_t first = 0;
            if (line0 + slot < nlines) { n = npts[line0 + slot]; first = off[line0 + slot]; }
            double len = 0.0;
            for (int k = g; k + 1 < n; k += G) {
                const float *a = xyz + 3 * (first + k);
                const double ux = ((double)a[3] - (double)a[0]) * dx, uy = ((double)a[4] - (double)a[1]) * dy, uz = ((double)a[5] - (double)a[2]) * dz;
                len += sqrt(ux * ux + uy * uy + uz * uz);
            }
            for (int d = G / 2; d >= 1; d >>= 1) len += __shfl_xor(len, d, G);
            if (g == 0) s_len[slot] = len;
        }
        __syncthreads();
    }
    const int64_t line = line0 + threadIdx.x;
    int counted = 0;
    int64_t ij = -1, ji = -1;
    if (line < nlines) {
        const int n = npts[line];
        int a = 0, b = 0;
        if (n >= 1) {
            const int64_t first = off[line];
            a = ts_node(xyz, first, nx, ny, nz, labels, remap, nremap, L);
            b = ts_node(xyz, first + n - 1, nx, ny, nz, labels, remap, nremap, L);
            const int64_t i = a < b ? a : b, j = a < b ? b : a;
            ij = i * (L + 1) + j;
            if (i != j) ji = j * (L + 1) + i;
            counted = 1;
        }
        if (assign) { assign[2 * line] = a; assign[2 * line + 1] = b; }
    }
    if (G > 1) {
        if (ij >= 0) {
            const double len = s_len[threadIdx.x];
            atomicAdd(C + ij, 1u);
            atomicAdd(W + ij, len);
            if (ji >= 0) { atomicAdd(C + ji, 1u); atomicAdd(W + ji, len); }
        }
    } else {
        const int lane = threadIdx.x & 63;
        uint64_t todo = __ballot(ij >= 0);
        while (todo) {                                          // (uniform over the wave: one round per distinct cell)
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int64_t cell = __shfl(ij, leader);
            const uint64_t same = __ballot(ij == cell);
            if (lane == leader) {
                atomicAdd(C + cell, (unsigned)__popcll(same));
                if (ji >= 0) atomicAdd(C + ji, (unsigned)__popcll(same));
            }
            todo &= ~same;
        }
    }
    int64_t unused = 0;
    ts_block_sum(counted, unused);
    if (threadIdx.x == 0) ts_add64(n_lines, counted);
}

// the work area: head | off3 [nlines + 1] | block totals
struct TsWork {
    TmHead *head;
    Ts3 *off3;
    LsVec<3> *totals;
};
size_t ts_work_bytes(int64_t nlines) { return TM_HEAD_BYTES + sizeof(Ts3) * (size_t)(nlines + 1) + sizeof(Ts3) * (size_t)ls_total_slots(nlines); }
TsWork ts_work(void *work, int64_t nlines) {
    TsWork w;
    w.head = reinterpret_cast<TmHead *>(work);
    w.off3 = reinterpret_cast<Ts3 *>(reinterpret_cast<char *>(work) + TM_HEAD_BYTES);
    w.totals = reinterpret_cast<LsVec<3> *>(w.off3 + nlines + 1);
    return w;
}
int ts_check_work(void *work, size_t work_bytes, int64_t nlines) {
    return ls_check_work(work, work_bytes, ts_work_bytes(nlines), "fibd_str_select_work_size");
}

template <int G>
void ts_launch_select(const float *xyz, const int32_t *npts, const TmWork &w, int64_t nlines, int nx, int ny, int nz, const uint32_t *roibits,
                      const TsRule &rule, uint8_t *keep, uint32_t *hits, int64_t *counts, hipStream_t st) {
    hipLaunchKernelGGL(ts_select<G>, dim3((unsigned)std::max<int64_t>(1, fib::cdiv(nlines, TM_BLOCK))), dim3(TM_BLOCK), 0, st, xyz, npts, w.off, nlines,
                       nx, ny, nz, roibits, rule, w.head, keep, hits, counts);
}

template <int G>
void ts_launch_connectome(const float *xyz, const int32_t *npts, const TmWork &w, int64_t nlines, int nx, int ny, int nz, const float *res,
                          const int32_t *labels, const int32_t *remap, int64_t nremap, int L, uint32_t *C, double *W, int32_t *assign, int64_t *n_lines,
                          hipStream_t st) {
    hipLaunchKernelGGL(ts_connectome<G>, dim3((unsigned)fib::cdiv(nlines, TM_BLOCK)), dim3(TM_BLOCK), 0, st, xyz, npts, w.off, nlines, nx, ny, nz,
                       res[0], res[1], res[2], labels, remap, nremap, L, w.head, C, W, assign, n_lines);
}

}  // namespace

extern "C" int fibd_str_roi_pack(const uint8_t *rois, int nroi, int64_t nvox, uint32_t *roibits, void *stream) try {
    FIB_CHECK(nroi >= 0 && nroi <= 32, FIB_ERR_INVALID, "an ROI bit volume holds 0 to 32 ROIs, not %d", nroi);
    FIB_CHECK(nvox >= 0, FIB_ERR_INVALID, "nvox must not be negative");
    if (nvox == 0) return FIB_OK;
    FIB_CHECK(roibits && (nroi == 0 || rois), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(fib::cdiv(nvox, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many voxels");
    fib::ProfScope prof("str_roi_pack", (hipStream_t)stream);
    hipLaunchKernelGGL(ts_roi_pack, dim3((unsigned)fib::cdiv(nvox, TM_BLOCK)), dim3(TM_BLOCK), 0, (hipStream_t)stream, rois, nroi, nvox, roibits);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_select_work_size(int64_t nlines, size_t *bytes) try {
    FIB_CHECK(bytes, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    *bytes = ts_work_bytes(nlines);
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_select(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, const uint32_t *roibits,
                               uint64_t visit_all, uint64_t visit_none, uint64_t end_any, uint64_t end_both, int32_t min_npts, int32_t max_npts,
                               uint8_t *keep, uint32_t *hits, int64_t *counts, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(((visit_all | visit_none | end_any | end_both) >> 32) == 0, FIB_ERR_INVALID, "a mask has bits above bit 31: there are 32 ROIs at most");
    FIB_CHECK(roibits || !(visit_all | visit_none | end_any | end_both), FIB_ERR_INVALID, "a mask is set but roibits is NULL");
    FIB_CHECK(min_npts >= 0 && max_npts >= 0, FIB_ERR_INVALID, "min_npts and max_npts must not be negative");
    FIB_CHECK(counts && (nlines == 0 || keep), FIB_ERR_INVALID, "NULL argument");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_RC(ts_check_work(work, work_bytes, nlines));
    FIB_CHECK(fib::cdiv(nlines, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_select", st);
    FIB_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, nullptr, st, w));
    const TsRule rule{(uint32_t)visit_all, (uint32_t)visit_none, (uint32_t)end_any, (uint32_t)end_both, min_npts, max_npts};
    int g = TS_SELECT_G;
#ifdef FIB_AB_VARIANTS                                          // the lane mapping's A/B partners (tools/tract_select_time.py, diagnostic build only)
    if (const char *e = fib::ab_env("FIBERS_TS_SELECT_G")) g = atoi(e);
    if (g == 8) ts_launch_select<8>(xyz, npts, w, nlines, nx, ny, nz, roibits, rule, keep, hits, counts, st);
    else if (g == 32) ts_launch_select<32>(xyz, npts, w, nlines, nx, ny, nz, roibits, rule, keep, hits, counts, st);
    else if (g == 64) ts_launch_select<64>(xyz, npts, w, nlines, nx, ny, nz, roibits, rule, keep, hits, counts, st);
    else
#endif
    { (void)g; ts_launch_select<TS_SELECT_G>(xyz, npts, w, nlines, nx, ny, nz, roibits, rule, keep, hits, counts, st); }
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_gather(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const uint8_t *keep, const float *scalars,
                               int nscalars, int64_t cap_lines, int64_t cap_points, float *xyz_out, int32_t *npts_out, int64_t *index_out,
                               float *scalars_out, int64_t *counts, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK(nscalars >= 0 && cap_lines >= 0 && cap_points >= 0, FIB_ERR_INVALID, "nscalars and the capacities must not be negative");
    FIB_CHECK(counts && (nlines == 0 || keep), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK((cap_lines == 0 || npts_out) && (cap_points == 0 || xyz_out), FIB_ERR_INVALID, "NULL output with a capacity above 0");
    FIB_CHECK(!scalars_out || (nscalars > 0 && (npoints == 0 || scalars)), FIB_ERR_INVALID, "scalars_out needs scalars and nscalars > 0");
    FIB_CHECK(((reinterpret_cast<uintptr_t>(xyz_out) | reinterpret_cast<uintptr_t>(scalars) | reinterpret_cast<uintptr_t>(scalars_out)) & 3) == 0,
              FIB_ERR_INVALID, "points and scalars must be 4-byte aligned");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_RC(ts_check_work(work, work_bytes, nlines));
    FIB_CHECK(fib::cdiv(nlines * TS_GATHER_G, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof("str_gather", st);
    const TsWork w = ts_work(work, nlines);
    ls_scan(TsItem{npts, keep, npoints, cap_lines, cap_points, w.head, w.off3, counts}, nlines, w.totals, st);
    if (nlines > 0)
        hipLaunchKernelGGL(ts_gather_copy<TS_GATHER_G>, dim3((unsigned)fib::cdiv(nlines * TS_GATHER_G, TM_BLOCK)), dim3(TM_BLOCK), 0, st,
                           reinterpret_cast<const uint32_t *>(xyz), npts, keep, w.off3, nlines, reinterpret_cast<const uint32_t *>(scalars), nscalars, w.head,
                           reinterpret_cast<uint32_t *>(xyz_out), npts_out, index_out, reinterpret_cast<uint32_t *>(scalars_out));
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_str_connectome(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz, const float volres[3],
                                   const int32_t *labels, const int32_t *remap, int64_t nremap, int nnodes, int flags, uint32_t *cmat, double *wmat,
                                   int32_t *assign, int64_t *n_lines_dev, void *work, size_t work_bytes, void *stream) try {
    FIB_CHECK((flags & ~FIB_CONNECTOME_ACCUMULATE) == 0, FIB_ERR_INVALID, "unknown connectome flags 0x%x", flags);
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nnodes >= 1 && nnodes < (1 << 24), FIB_ERR_INVALID, "the number of nodes must be between 1 and 2^24 - 1");
    FIB_CHECK(labels && cmat && n_lines_dev, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(!wmat || volres, FIB_ERR_INVALID, "the lengths of W need volres");
    FIB_CHECK(nremap >= 0 && (nremap == 0 || remap), FIB_ERR_INVALID, "nremap entries need a remap array");
    FIB_RC(tm_check_lines(xyz, npts, nlines, npoints));
    FIB_RC(ts_check_work(work, work_bytes, nlines));
    FIB_CHECK(fib::cdiv(nlines, TM_BLOCK) < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "too many lines");
    hipStream_t st = (hipStream_t)stream;
    fib::ProfScope prof(wmat ? "str_connectome_w" : "str_connectome", st);
    const size_t cells = (size_t)(nnodes + 1) * (size_t)(nnodes + 1);
    if (!(flags & FIB_CONNECTOME_ACCUMULATE)) {
        FIB_HIP(hipMemsetAsync(cmat, 0, sizeof(uint32_t) * cells, st));
        if (wmat) FIB_HIP(hipMemsetAsync(wmat, 0, sizeof(double) * cells, st));
    }
    TmWork w;
    FIB_RC(tm_offsets(npts, nlines, npoints, work, work_bytes, n_lines_dev, st, w));      // (*n_lines_dev = 0, or -1 for a refused input)
    if (nlines == 0) return FIB_OK;
    const float none[3] = {1.0f, 1.0f, 1.0f};
    const float *res = wmat ? volres : none;
    if (wmat) ts_launch_connectome<TS_LENGTH_G>(xyz, npts, w, nlines, nx, ny, nz, res, labels, remap, nremap, nnodes, cmat, wmat, assign, n_lines_dev, st);
    else ts_launch_connectome<1>(xyz, npts, w, nlines, nx, ny, nz, res, labels, remap, nremap, nnodes, cmat, wmat, assign, n_lines_dev, st);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
