// stream.hip — K6/K7: deterministic streamline tractography (nearest-voxel lookup + fixed-step Euler).
//
// Replaces StreamWork's mask/vector repack (stream.jl:95-145), stream_new_line (stream.jl:625-690),
// stream_new_point! (stream.jl:501-541), stream_pick_by_angle! (stream.jl:340-374) and the seed loop /
// len_min filter / concatenation of `stream` (stream.jl:761-787), for the non-LCM macro-scale path.
//
// Layout.  The orientation field is repacked to float4 [nvox][nvec] (xyz0): one aligned 16-byte gather
// per candidate vector per step; vectors of masked-out voxels are zero, which makes the reference's
// separate mask lookup (stream.jl:520) redundant (an all-zero voxel fails stream_pick_by_angle! the same
// way).  One lane integrates one (seed, sub-voxel offset) line, forward then backward.  Points go to a
// slot-major scratch [2*(len_max+2) slots][nlines][3]: forward step i -> slot i, backward step j -> slot
// L+j, so that at every step the 64 lanes of a wave (consecutive lines, same step) store one contiguous
// 768-byte run.  (Line-major rows cost 2.6x: 12-byte stores to 64 different cache lines per step, partial
// lines evicted to HBM.)  Worst-case rows are affordable with 288 GB: 1 M lines x 284 slots x 12 B = 3.4 GB.
// A scan over the per-line counts gives every kept line its offset; the pack kernel transposes 16-slot x
// 64-line blocks through LDS and emits the reference's point order [fwd_N .. fwd_1, bwd_1 .. bwd_M]
// (prepend!/append!, stream.jl:652) in 48-byte pieces.  The pack side -- the pack kernels and the fused trace kernel's pack tail --
// is stream_pack.inc, included below behind the scan kernels.
//
// Arithmetic.  No a*b+c contraction anywhere in this file: positions are compared after round-to-nearest-
// even (stream.jl:514) so one ulp moves a line to another voxel; with contraction off every operation is
// an IEEE single/double operation in the reference's order and the CPU restatement is matched bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <mutex>

#include "common.h"

#pragma clang fp contract(off)

namespace {

struct FieldArgs {
    const float *ovec[8];
    const float *f[8];
    const float *fa;
    const uint8_t *mask;
    float4 *field;
    uint8_t *mask_out;
    int64_t nvox;
    int nvec;
    int has_f;
    float f_thresh, fa_thresh;
};

__global__ __launch_bounds__(256) void stream_field_kernel(const FieldArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nvox) return;
    float v[8][3];
    bool any = false;
    for (int k = 0; k < a.nvec; k++)
        for (int c = 0; c < 3; c++) {
            v[k][c] = a.ovec[k][(int64_t)c * a.nvox + i];
            any |= v[k][c] != 0.0f;                               // any(x -> x != 0, ...), stream.jl:99
        }
    bool m = a.mask ? a.mask[i] != 0 : any;                       // stream.jl:95-103 (mask already '> 0'-tested)
    if (a.fa) m = m && (a.fa[i] >= a.fa_thresh);                  // stream.jl:116
    for (int k = 0; k < a.nvec; k++) {
        bool om = m;
        if (a.has_f) om = m && (a.f[k][i] >= a.f_thresh);         // stream.jl:138
        // w = the voxel mask itself (the microscopy regime tests W.mask apart from the vectors, stream.jl:596)
        const float w = m ? 1.0f : 0.0f;
        a.field[i * a.nvec + k] = om ? make_float4(v[k][0], v[k][1], v[k][2], w) : make_float4(0.0f, 0.0f, 0.0f, w);
    }
    if (a.mask_out) a.mask_out[i] = m ? 1 : 0;
}

struct Pair { int64_t pts, lines; };
constexpr int SCR_TILE = 16;         // lines per pack tile: the unit whose output range a pack workgroup assembles in LDS
constexpr int FUSED_TILE = 16;       // .. in the fused trace + pack kernel
constexpr int FUSED_BLOCK = 512;     // its workgroup: 8 waves, so that 4 workgroups of 35 KB of LDS keep the CU's 32 wave slots full
// Lines that share a ROW of the point scratch (a row = one slot of SCR_ROW lines, SCR_ROW x 12 bytes).  [r5] The tracer is bound by these
// stores (tools/stream_bound_probe.py: without them the trace takes 0.43 of 0.50 ms, without the field gathers nothing less), and
// non-temporal stores that end in the middle of a 128-byte line are slow: 192-byte rows (16 lines) reach 4.1 TB/s alone, 384-byte rows
// (32 lines = three whole lines) 5.1 (tools/probes/write_probe.hip), and the trace kernel went 0.54 -> 0.49 ms with them.  But then the
// pack side pays the same back: 16-line tiles that read 192 of every 384 bytes 0.54 -> 0.63 ms, 32-line tiles (55 KB of LDS, two
// workgroups per CU) 0.60 (1 024 threads) / 0.64 (512), the fused kernel 10.6 -> 11.7 ms (half rows) / 13.3 (32-line tiles, 1 024
// threads): profiles/r05/negative_results.txt.  So the row stays the pack tile, and the trace kernel gets its whole lines another way:
// it parks four trips' points in LDS and stores the four rows together (see there).  (8-line rows, 96 B: the trace 3 x slower.)
constexpr int SCR_ROW = 16;
static_assert(SCR_ROW % SCR_TILE == 0 && SCR_ROW % FUSED_TILE == 0, "pack tiles are whole fractions of a scratch row");
constexpr int SCR_SLOT_FLOATS = SCR_ROW * 3;                       // from one slot of a line to its next
// first float of line li's slot 0:  [row = li / SCR_ROW][slot][li % SCR_ROW][3]
__host__ __device__ __forceinline__ int64_t scratch_line_base(int64_t li, int nslots) {
    return (li / SCR_ROW) * ((int64_t)nslots * SCR_SLOT_FLOATS) + (li % SCR_ROW) * 3;
}
constexpr int TRACE_SCAN_B = 2048;   // = SCAN_B (lines per block of the scan)
struct TraceArgs {
    const float4 *field;        // [nvox][nvec]
    const int64_t *seeds;       // [nseed] 0-based linear voxel index
    const float *sublist;       // [nsub][3]
    float *scratch;             // [nlines/16 rows][nslots][16 lines][3]: the point a line emits at loop trip t -> slot t: forward point i in slot i,
                                // backward point j in slot nf + gap + j (a row's slots are one contiguous run that the pack kernel streams; the
                                // trace kernel stores four trips' rows of a tile together, as whole 128-byte lines)
    int32_t *npts, *nfwd;       // [nlines]; nfwd = forward points | gap << 30 (gap = 1: the forward pass ended on a trip that emitted nothing)
    int64_t line0, nlines;      // this batch covers global lines [line0, line0+nlines)
    int nx, ny, nz, nvec, nsub, len_max, stride, nslots;
    int scratch_plain;          // diagnostic build only (FIBERS_STREAM_SCRATCH_PLAIN): the point scratch with the default cache policy instead of non-temporal
    int norm_generic;           // diagnostic build only (FIBERS_STREAM_NORM_GENERIC): normalise3's generic expansion for every vector
    int lcm_plain;              // LCM runs: lcm_thresh >= 2^-40 (every entry of the thresholded matrices is 0 or at least that)
    int dbg;                    // diagnostic build only (FIBERS_STREAM_DBG bit mask; WRONG RESULTS, timing experiments): 1 = no gather after the seed's, 2 = no point stores
    // FUSED (fibd_stream_run): the block that traced 512 lines also packs them -- a decoupled look-back over the blocks' kept-line / point
    // totals gives it its place in the output
    unsigned long long *fstate; // [blocks] granules: status << 62 | kept lines << 36 | points (zeroed before the launch)
    int32_t *out_npts;
    int64_t *out_seed;
    float *out_xyz;
    Pair *ftotal;               // the last block's inclusive prefix = the call's totals
    int64_t *fcounts;           // .. and, fibd_stream_run_enqueue, {lines, points} for the caller
    int64_t lines_cap, points_cap;
    int len_min;
    float cosang, step, smooth;
    // microscopy regime (stream.jl:252-287, 547-619)
    // LCM-guided tracking (stream.jl:200-236, 380-495)
    const float *lcm;           // [nvox][10] thresholded local connection matrices (lcm_prepare_kernel)
    int sd0, sd1;               // in-plane dimensions (0-based)
    unsigned long long rng_seed;
    const float4 *search;       // half of the search cube's cells with rho < 1, column-major order: {unit vector, bits of (kx | ky<<8 | kz<<16)} (0-based cell)
    int nsearch, search_dist;
    int sdx, sdy, sdz;          // .. per axis: search_dist, or 0 along the through-plane axis of 2-D angle inputs (stream.jl:153-155)
    float search_cosang;
    const int32_t *cell_start;  // [G^3 + 1]: the table is sorted by direction cell (x fastest); entries of cell i = [cell_start[i], cell_start[i+1])
    int G;                      // direction grid: cell (floor((v + 1) / h)) per axis, h = 2 / G
};

// iszero(v) on a 3-view (stream.jl:353): all three components == 0, -0.0 included.  One OR of the three bit patterns and one class
// test (a pattern with no magnitude bit set is +-0) instead of three compares.
__device__ __forceinline__ bool is_zero3(float x, float y, float z) {
    const unsigned u = __float_as_uint(x) | __float_as_uint(y) | __float_as_uint(z);
    return __builtin_amdgcn_classf(__uint_as_float(u), 0x60);     // (v_cmp_class: -0 | +0)
}
// v_cvt_i32_f32 itself (NaN -> 0, out of range -> INT_MIN / INT_MAX): what the bounds test below wants, and not what C++ promises
__device__ __forceinline__ int cvt_i32_sat(float x) {
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return ax * bx + ay * by + az * bz;                           // (x+y)+z, no fma
}
// A point on its way out: written once, read back by the pack kernel (or by nobody on the device).  NON-TEMPORAL -- [r4] with the
// default policy the 1.6 GB of scratch points of a million lines go through the XCDs' L2 and push the orientation field out of it:
// the trace kernel took 0.69 ms, 0.55 with this store (and 0.50 with no store at all); the pack kernel gains 4 % too.
typedef float f32x3_t __attribute__((ext_vector_type(3)));
__device__ __forceinline__ void store_point(float *d, float x, float y, float z) {   // (the microscopy tracer: one lane per line stores)
    const f32x3_t v = {x, y, z};
    __builtin_nontemporal_store(v, reinterpret_cast<f32x3_t *>(d));
}
#ifdef FIB_AB_VARIANTS
typedef float fib_f4_t __attribute__((ext_vector_type(4)));
// (diagnostic build, FIBERS_STREAM_SCRATCH_PLAIN = 1..6: the scratch stores with another cache policy, as inline assembly -- written as a second
// C++ store hipcc once merged the two branches into ONE store without the non-temporal hint; tests/test_kernel_schedule.py asserts the hint)
__device__ __forceinline__ void store_x4_variant(fib_f4_t *d, fib_f4_t v, int flavour) {
    if (flavour == 1) asm volatile("global_store_dwordx4 %0, %1, off" :: "v"(d), "v"(v) : "memory");
    else if (flavour == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(d), "v"(v) : "memory");
    else if (flavour == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(d), "v"(v) : "memory");
    else if (flavour == 4) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" :: "v"(d), "v"(v) : "memory");
    else if (flavour == 5) asm volatile("global_store_dwordx4 %0, %1, off sc0 nt" :: "v"(d), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc0" :: "v"(d), "v"(v) : "memory");
}
#endif

// w ./= norm(w)  (stream.jl:680).  LinearAlgebra.norm on a 3-vector is generic_norm2: the largest magnitude first (zero / Inf / NaN return
// it), then the squares in Float32, their sum and the square root in Float64, the result converted to Float32; then three IEEE divisions.
// [r5] Written out as `(float)sqrt(acc)` and `w / n` this is ~60 of the tracer's ~125 vector instructions per step (which bound the
// three-vector tracer and, once its stores leave as whole lines, the one-vector tracer too): hipcc expands the f64 square root with a range-scaling prologue / special-value epilogue and each division with two
// v_div_scale, a reciprocal, its refinement, v_div_fmas and v_div_fixup.  Where every component is 0 or within 2^-40 .. 2^40 -- any
// orientation field -- none of the scaling or fix-up can trigger, and the SAME instruction sequences without them give the same bits:
// the Goldschmidt square root of llvm's f64 lowering, ONE refined reciprocal for the three divisions, two residual corrections per
// quotient.  Anything outside that range takes the generic expansion.  tests/test_gpu_stream.py compares the two over random and edge inputs.
__device__ __forceinline__ void normalise3(float &wx, float &wy, float &wz, bool generic = false) {
    const float m = fmaxf(fabsf(wx), fmaxf(fabsf(wy), fabsf(wz)));
    const float lo = fminf(fabsf(wx), fminf(fabsf(wy), fabsf(wz)));
    bool plain = lo >= 0x1p-40f && m <= 0x1p40f;                   // (NaN fails)
#ifdef FIB_AB_VARIANTS
    if (generic) plain = false;                                    // diagnostic build, FIBERS_STREAM_NORM_GENERIC: hipcc's expansions throughout
    else
#endif
    if (!plain && m <= 0x1p40f && m >= 0x1p-40f)                   // components that are exactly zero (2-D sections) are fine too
        plain = (wx == 0.0f || fabsf(wx) >= 0x1p-40f) && (wy == 0.0f || fabsf(wy) >= 0x1p-40f) && (wz == 0.0f || fabsf(wz) >= 0x1p-40f);
    if (plain) {
        double acc = (double)(wx * wx);
        acc += (double)(wy * wy);
        acc += (double)(wz * wz);
        const double y = __builtin_amdgcn_rsq(acc);
        double g = acc * y, h = y * 0.5;
        const double r = fma(-h, g, 0.5);
        g = fma(g, r, g);
        double d = fma(-g, g, acc);
        h = fma(h, r, h);
        g = fma(d, h, g);
        d = fma(-g, g, acc);
        g = fma(d, h, g);
        const float n = (float)g;
        float rc = __builtin_amdgcn_rcpf(n);
        rc = fmaf(fmaf(-n, rc, 1.0f), rc, rc);
        auto quot = [&](float x) {
            float q = x * rc;
            q = fmaf(fmaf(-n, q, x), rc, q);
            q = fmaf(fmaf(-n, q, x), rc, q);
            return __builtin_copysignf(q, x);                     // (-0 / n = -0; the residual steps give +0)
        };
        wx = quot(wx); wy = quot(wy); wz = quot(wz);
        return;
    }
    float n;
    if (m == 0.0f || !(m < INFINITY)) n = m;
    else {
        double acc = (double)(wx * wx);
        acc += (double)(wy * wy);
        acc += (double)(wz * wz);
        n = (float)sqrt(acc);
    }
    wx = wx / n; wy = wy / n; wz = wz / n;
}

// The random-number contract of LCM-guided tracking (include/fibers_hip.h): the k-th uniform of streamline `line` is
// splitmix64 of (seed, line, k), top 24 bits -> [0,1).  Same function in the oracle (orc_uniform).
__host__ __device__ __forceinline__ unsigned long long fib_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ float fib_uniform(unsigned long long seed, unsigned long long line, unsigned k) {
    const unsigned long long h = fib_splitmix64(seed ^ fib_splitmix64(line * 0xD1342543DE82EF95ull + (unsigned long long)k));
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}

// lcm_array = permutedims(lcms.vol, (4,1,2,3)) .* (. >= lcm_thresh)  (stream.jl:207,217): [nvox][10] from planar [10][nvox]
__global__ __launch_bounds__(256) void lcm_prepare_kernel(const float *__restrict__ lcms, float thresh, int64_t nvox, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    for (int j = 0; j < 10; j++) {
        const float x = lcms[(int64_t)j * nvox + i];
        out[i * 10 + j] = x >= thresh ? x : 0.0f;                  // `x * false` is a strong zero in Julia (NaN -> 0)
    }
}

// coordinate increments for exiting through edge j = 1..4 (stream.jl:224-226) along dimension c
__device__ __forceinline__ int lcm_dxyz(int j, int c, int sd0, int sd1) {
    const int a4 = (j == 1) ? -1 : (j == 3 ? 1 : 0), b4 = (j == 2) ? -1 : (j == 4 ? 1 : 0);
    return c == sd0 ? a4 : (c == sd1 ? b4 : 0);
}
__device__ __forceinline__ int lcm_match_edge(int dx, int dy, int dz, int sd0, int sd1) {
    for (int j = 1; j <= 4; j++)
        if (lcm_dxyz(j, 0, sd0, sd1) == dx && lcm_dxyz(j, 1, sd0, sd1) == dy && lcm_dxyz(j, 2, sd0, sd1) == dz) return j;
    return 0;
}

// The points go into the slot-major scratch and the per-line counts beside them; the scan + pack kernels below give every kept
// line its place.  ([r5] the two-pass form -- count, scan, trace again straight into the output -- was as slow as the copy it
// saved (a trace without stores takes 0.50 of the 0.53 ms) and has been removed: profiles/r04/negative_results.txt.)
// TRI (params.interp = 1, 2, 3, not in the reference): the direction followed is the trilinear blend of the eight voxels around the
// tentative position instead of the nearest voxel's vector -- see `blend` below for the exact definition.  TRI is also the
// integrator that finds the tentative position: 1 = forward Euler, 2 = midpoint (RK2, one more blend per step), 3 = classical RK4
// (three more) -- include/fibers_hip.h, fib_stream_params.interp.
// WIDE: 64-bit voxel indices and gather offsets, for orientation fields of 2^28 vectors (4 GiB) or more -- the microscopy
// regime's whole-slide sections (stream.jl:83,147-172); chosen at launch, bit-identical to the 32-bit form on small fields.
template <int NVEC> __device__ void fused_pack_block(const TraceArgs &a, int64_t b, int64_t li, bool live, int npts, int nf, int gap);   // (stream_pack.inc)

// [rk] The stages of RK2 / RK4 probe the SAME register cell cache as the final evaluation (NVEC == 1): the positions a line visits --
// pos + h/2, pos + h/2, pos + h, nxt, then the next step's -- advance along the line, so the stages reload the cell where the Euler
// form would and otherwise hit it.  0: the stages gather their eight corners directly (the alternative that was measured:
// profiles/stream_rk/README.md).
#ifndef FIB_RK_STAGE_CACHE
#define FIB_RK_STAGE_CACHE 1
#endif
template <int NVEC, bool LCM = false, int TRI = 0, bool WIDE = false, bool FUSED = false>   // NVEC > 0: compile-time vector count; 0: runtime
__global__ __launch_bounds__(FUSED ? FUSED_BLOCK : 256) void stream_trace_kernel(const TraceArgs a) {
    // FUSED: the workgroup's place in the line order is a TICKET, not blockIdx: whatever order workgroups are dispatched in, everything a
    // workgroup later waits for in the look-back (tickets below its own) was drawn by a workgroup that is already running
    int64_t wg = blockIdx.x;
    if constexpr (FUSED) {
        __shared__ unsigned s_ticket;
        if (threadIdx.x == 0) s_ticket = atomicAdd(reinterpret_cast<unsigned *>(a.fstate + gridDim.x), 1u);
        __syncthreads();
        wg = s_ticket;
    }
    const int64_t li = wg * blockDim.x + threadIdx.x;
    const bool live_line = li < a.nlines;              // (every thread takes part in the scratch stores and, FUSED, in the pack)
    typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type vox_t;
    const int nvec = NVEC > 0 ? NVEC : a.nvec;
    const int64_t line = a.line0 + (!live_line ? a.nlines - 1 : li);   // (a thread past the end borrows the last line's seed and traces nothing)
    const int64_t iseed = line / a.nsub;
    const int isub = (int)(line - iseed * a.nsub);
    const int64_t lin = a.seeds[iseed];
    const int sx = (int)(lin % a.nx), sy = (int)((lin / a.nx) % a.ny), sz = (int)(lin / ((int64_t)a.nx * a.ny));
    const float p0x = (float)(sx + 1) + a.sublist[3 * isub];      // pos_now .= seed_vox .+ sub_vox, stream.jl:649
    const float p0y = (float)(sy + 1) + a.sublist[3 * isub + 1];
    const float p0z = (float)(sz + 1) + a.sublist[3 * isub + 2];
    // [r5] The points leave in GROUPS OF FOUR TRIPS as whole 128-byte lines.  A trip's points of a tile are a 192-byte row, and a
    // non-temporal store instruction that ends in the middle of a line is slow (such stores alone: 4.1 TB/s; whole lines: 5.1 --
    // tools/probes/write_probe.hip), and these stores bound the kernel (tools/stream_bound_probe.py).  So a lane parks its point in LDS
    // (768 B per tile: 4 slots x 16 lines x 12 B) and after every fourth trip the tile's 16 lanes store the 48 float4 of those four rows --
    // 3 instructions per wave, each 4 runs of 256 contiguous bytes -- instead of 4 instructions of 4 x 192 B.  Same scratch layout, same
    // bytes; lanes whose line has ended stay in the loop (switched off) to do their share of the stores.
    static_assert(SCR_ROW == 16, "the grouped scratch stores map a tile's 16 lanes to its 48 float4 per four slots");
    float *stage;                                                 // this lane's tile: [4 slots][16 lines][3]
    if constexpr (FUSED) {
        extern __shared__ __attribute__((aligned(16))) float f_obuf[];   // (the pack phase's tile buffer: free until the trace loop is over)
        stage = f_obuf + (threadIdx.x >> 4) * (4 * SCR_SLOT_FLOATS);
    } else {
        __shared__ __attribute__((aligned(16))) float s_stage[256 / 16][4 * SCR_SLOT_FLOATS];
        stage = s_stage[threadIdx.x >> 4];
    }
    const int tj = threadIdx.x & 15;                              // this line's place in its tile
    float *const tile0 = a.scratch + scratch_line_base(li - tj, a.nslots);   // the tile's slot 0
    const bool tile_ok = li - tj < a.nlines;                      // (a tile wholly past the end has no scratch)
    int trip = 0;                                                 // wave-uniform: the slot the current trip writes
    const char *fbase = reinterpret_cast<const char *>(a.field);   // wave-uniform base; per-lane offsets are 32-bit
    const float fnx = (float)a.nx, fny = (float)a.ny, fnz = (float)a.nz;
    const float omc = 1.0f - a.smooth;
    int ivec = 0, npts = 0, nf = 0, pass = 0, gap = 0;
    unsigned ndraw = 0;                                           // uniforms consumed by this line (LCM)
    // [r4] The voxel's vectors stay in registers while the line stays in the voxel (a step is half a voxel: 35-50 % of the steps do): a
    // lane that does not need the gather is switched off for it.  Same data, same arithmetic.  Three vectors per voxel (C5): trace
    // 6.4 -> 6.0 ms; one vector (C4): nothing (tools/stream_c5_times.py, stream_kernel_times.py).
    constexpr int NCV = NVEC > 0 ? NVEC : 1;
    constexpr int NTRI = (TRI && NVEC == 1) ? 8 : 1;             // the trilinear option's cell of corner vectors (one vector per voxel)
    float tri_x[NTRI], tri_y[NTRI], tri_z[NTRI];
    float tri_gx = __builtin_nanf(""), tri_gy = 0.0f, tri_gz = 0.0f;   // (NaN: no cell yet)
    float4 cvec[NCV];
    vox_t cvox = ~(vox_t)0;
    float px = p0x, py = p0y, pz = p0z;
    float vx, vy, vz;
    {
        const float4 s = a.field[lin * nvec];                     // view(W.ovecs, :, ivec_next, seed...), stream.jl:650 (ivec_next = 1)
        vx = s.x * 1.0f; vy = s.y * 1.0f; vz = s.z * 1.0f;
    }
    // One trip of the loop = one step of whichever pass the lane is in.  true: the pass ended at this trip (stream.jl:657, :670, :674).
    // D(q, r): the trilinear option's direction at position q against the reference direction r,
    //   w = normalise( sum over the 8 corners c of floor(q) + {0,1}^3 inside the volume of  t_c * s_c * u_c ),
    // t_c = (ax * ay) * az with a = frac or 1 - frac per axis, u_c = the corner's vector picked by the angle rule against r (corners
    // without a vector contribute nothing), s_c = sign of its cosine; products and sums in Float32 in corner order x fastest, the norm
    // as LinearAlgebra.norm does it (normalise3).  false: no direction (a zero or non-finite blend; a q that is not finite has no corner
    // inside the volume).  The 8 x nvec float4 loads of a blend hit L2 / the vector cache (the stencil moves by half a voxel per step); an
    // LDS copy per lane (128 B x nvec x 256 lanes) was not worth its LDS traffic.  [r5] CACHED (one vector per voxel): the cell's eight
    // vectors are kept in REGISTERS between the blends that stay in it (trace 2.39 -> 1.82 ms).
    auto blend = [&](auto cached, float qx, float qy, float qz, float rx, float ry, float rz, float &wx, float &wy, float &wz) -> bool {
        const float gx0 = floorf(qx), gy0 = floorf(qy), gz0 = floorf(qz);
        const float tx = qx - gx0, ty = qy - gy0, tz = qz - gz0;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        // per-axis validity of the low / high corner and the linear index of the low corner: no per-corner bounds test
        const bool xl = gx0 >= 1.0f && gx0 <= fnx, xh = gx0 + 1.0f >= 1.0f && gx0 + 1.0f <= fnx;
        const bool yl = gy0 >= 1.0f && gy0 <= fny, yh = gy0 + 1.0f >= 1.0f && gy0 + 1.0f <= fny;
        const bool zl = gz0 >= 1.0f && gz0 <= fnz, zh = gz0 + 1.0f >= 1.0f && gz0 + 1.0f <= fnz;
        const int64_t cbase = ((int64_t)gx0 - 1) + (int64_t)a.nx * (((int64_t)gy0 - 1) + (int64_t)a.ny * ((int64_t)gz0 - 1));
        const float ax0 = 1.0f - tx, ay0 = 1.0f - ty, az0 = 1.0f - tz;
        if constexpr (NVEC == 1 && decltype(cached)::value) {
            // [r5] one vector per voxel: the eight corner vectors stay in registers while the position stays in the cell (a step is
            // half a voxel: ~40 % of the steps do) -- the lanes that changed cell reload, corners outside the volume count as
            // "no vector".  Same data, same arithmetic.
            if (gx0 != tri_gx || gy0 != tri_gy || gz0 != tri_gz) {
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
                    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if ((cx ? xh : xl) && (cy ? yh : yl) && (cz ? zh : zl)) {
                        if constexpr (WIDE) w = *reinterpret_cast<const float4 *>(fbase + (uint64_t)(cbase + cx + (int64_t)a.nx * (cy + a.ny * cz)) * (uint64_t)16);
                        else w = *reinterpret_cast<const float4 *>(fbase + (size_t)((uint32_t)((int)cbase + cx + a.nx * (cy + a.ny * cz)) * 16u));
                    }
                    tri_x[c] = w.x; tri_y[c] = w.y; tri_z[c] = w.z;
                }
                tri_gx = gx0; tri_gy = gy0; tri_gz = gz0;
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
                const float ux = tri_x[c], uy = tri_y[c], uz = tri_z[c];
                if (is_zero3(ux, uy, uz)) continue;           // (no vector there, or a corner outside the volume)
                const float tc = ((cx ? tx : ax0) * (cy ? ty : ay0)) * (cz ? tz : az0);
                const float uc = dot3(rx, ry, rz, ux, uy, uz);
                if (!(fabsf(uc) < INFINITY)) continue;
                const float sg = uc > 0.0f ? tc : -tc;
                sx = sx + sg * ux; sy = sy + sg * uy; sz = sz + sg * uz;
            }
        } else
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
            if (!((cx ? xh : xl) && (cy ? yh : yl) && (cz ? zh : zl))) continue;
            const float tc = ((cx ? tx : ax0) * (cy ? ty : ay0)) * (cz ? tz : az0);
            const float4 *cc;
            if constexpr (WIDE) cc = reinterpret_cast<const float4 *>(fbase + (uint64_t)(cbase + cx + (int64_t)a.nx * (cy + a.ny * cz)) * (uint64_t)(nvec * 16));
            else {
                const uint32_t cv = (uint32_t)((int)cbase + cx + a.nx * (cy + a.ny * cz));
                cc = reinterpret_cast<const float4 *>(fbase + (size_t)(cv * (uint32_t)(nvec * 16)));
            }
            float ux = 0.0f, uy = 0.0f, uz = 0.0f, uc = 0.0f, ua = 0.0f;
#pragma unroll
            for (int k = 0; k < nvec; k++) {
                const float4 w = cc[k];
                float cs, ca;
                if (is_zero3(w.x, w.y, w.z)) { cs = -INFINITY; ca = -INFINITY; }
                else { cs = dot3(rx, ry, rz, w.x, w.y, w.z); ca = fabsf(cs); }
                if (k == 0 || __float_as_int(ca) > __float_as_int(ua)) { ua = ca; uc = cs; ux = w.x; uy = w.y; uz = w.z; }
            }
            if (!(fabsf(uc) < INFINITY)) continue;
            const float sg = uc > 0.0f ? tc : -tc;
            sx = sx + sg * ux; sy = sy + sg * uy; sz = sz + sg * uz;
        }
        const float m = fmaxf(fabsf(sx), fmaxf(fabsf(sy), fabsf(sz)));
        if (m == 0.0f || !(m < INFINITY)) return false;
        wx = sx; wy = sy; wz = sz;
        normalise3(wx, wy, wz, a.norm_generic != 0);
        return true;
    };
    constexpr std::integral_constant<bool, NVEC == 1> cell_cached{};                                   // the evaluation at the tentative position
    constexpr std::integral_constant<bool, NVEC == 1 && FIB_RK_STAGE_CACHE != 0> stage_cached{};      // the stages of RK2 / RK4
    const float h_half = a.step * 0.5f, h_sixth = a.step / 6.0f;  // (TRI >= 2; one IEEE division)
    bool emitted = false;
    auto step = [&]() -> bool {
        emitted = false;
        {
            // the tentative position: stream.jl:512 (forward Euler), or -- TRI = 2, 3 -- the midpoint rule / classical Runge-Kutta on the
            // blended field (include/fibers_hip.h).  k1 is the carried direction; every product and sum is rounded on its own, in the
            // header's order; a stage without a direction ends the pass like an invalid position does (stream.jl:657): nothing is emitted.
            float nxp, nyp, nzp;
            if constexpr (TRI >= 2) {
                float k2x, k2y, k2z;
                if (!blend(stage_cached, px + vx * h_half, py + vy * h_half, pz + vz * h_half, vx, vy, vz, k2x, k2y, k2z)) return true;
                if constexpr (TRI == 2) {
                    nxp = px + k2x * a.step; nyp = py + k2y * a.step; nzp = pz + k2z * a.step;
                } else {
                    float k3x, k3y, k3z, k4x, k4y, k4z;
                    if (!blend(stage_cached, px + k2x * h_half, py + k2y * h_half, pz + k2z * h_half, k2x, k2y, k2z, k3x, k3y, k3z)) return true;
                    if (!blend(stage_cached, px + k3x * a.step, py + k3y * a.step, pz + k3z * a.step, k3x, k3y, k3z, k4x, k4y, k4z)) return true;
                    const float smx = ((vx + 2.0f * k2x) + 2.0f * k3x) + k4x;
                    const float smy = ((vy + 2.0f * k2y) + 2.0f * k3y) + k4y;
                    const float smz = ((vz + 2.0f * k2z) + 2.0f * k3z) + k4z;
                    nxp = px + smx * h_sixth; nyp = py + smy * h_sixth; nzp = pz + smz * h_sixth;
                }
            } else {
                nxp = px + vx * a.step; nyp = py + vy * a.step; nzp = pz + vz * a.step;              // stream.jl:512
            }
            const float rx = rintf(nxp), ry = rintf(nyp), rz = rintf(nzp);                        // stream.jl:514
            // x in axes(mask, 1) ... (:517) on the 0-based integers: one unsigned compare per axis (NaN -> 0 - 1, +-huge -> saturated: outside)
            const unsigned ux = (unsigned)cvt_i32_sat(rx) - 1u, uy = (unsigned)cvt_i32_sat(ry) - 1u, uz = (unsigned)cvt_i32_sat(rz) - 1u;   // (unsigned: no overflow to reason about)
            if (!((ux < (unsigned)a.nx) & (uy < (unsigned)a.ny) & (uz < (unsigned)a.nz))) return true;
            const int ix = (int)ux, iy = (int)uy, iz = (int)uz;
            vox_t vox;
            const float4 *cand;
            if constexpr (WIDE) {
                vox = (uint64_t)((int64_t)ix + (int64_t)a.nx * ((int64_t)iy + (int64_t)a.ny * (int64_t)iz));
                cand = reinterpret_cast<const float4 *>(fbase + vox * (uint64_t)(nvec * 16));
            } else {
                vox = (uint32_t)(ix + a.nx * (iy + a.ny * iz));   // nvox < 2^28 / nvec: the byte offset fits 32 bits
                cand = reinterpret_cast<const float4 *>(fbase + (size_t)(vox * (uint32_t)(nvec * 16)));
            }
            float bx = 0.0f, by = 0.0f, bz = 0.0f, bestc = 0.0f, besta = 0.0f;
            int best = 0;
            if constexpr (NVEC > 0) {
#ifdef FIB_AB_VARIANTS
                if (a.dbg & 1) { if (cvox == ~(vox_t)0) { for (int k = 0; k < NVEC; k++) cvec[k] = cand[k]; } cvox = vox; }
#endif
                if (vox != cvox) {
#pragma unroll
                    for (int k = 0; k < NVEC; k++) cvec[k] = cand[k];
                    cvox = vox;
                }
            }
#pragma unroll
            for (int k = 0; k < nvec; k++) {                      // stream_pick_by_angle!, stream.jl:350-361
                const float4 w = NVEC > 0 ? cvec[k < NCV ? k : 0] : cand[k];
                float c, ca;
                if (is_zero3(w.x, w.y, w.z)) { c = -INFINITY; ca = -INFINITY; }
                else { c = dot3(vx, vy, vz, w.x, w.y, w.z); ca = fabsf(c); }
                // argmax: first maximum, NaN wins over everything -- as ONE signed compare of the bit patterns: ca is -Inf, >= +0 or a NaN
                // with its sign cleared, and as integers -Inf < +0 <= .. <= +Inf < every such NaN.  (A later NaN with a larger payload
                // replaces an earlier one where the reference keeps the first: both end the line, below, before `best` is used.)
                if (k == 0 || __float_as_int(ca) > __float_as_int(besta)) {
                    best = k; besta = ca; bestc = c; bx = w.x; by = w.y; bz = w.z;
                }
            }
            if (!(fabsf(bestc) < INFINITY)) return true;          // !isfinite -> false, stream.jl:363
            float wx, wy, wz;
            if (bestc > 0.0f) { wx = bx; wy = by; wz = bz; } else { wx = -bx; wy = -by; wz = -bz; }   // :365-369
            ivec = best;                                          // stream.jl:371
            if constexpr (TRI != 0) {
                // Trilinear option.  Everything above still decides whether the line goes on (bounds, the nearest voxel's pick must
                // exist) and which vector index the backward pass starts from; the direction becomes the blend at the tentative
                // position against the current direction (`blend` above).  A zero or non-finite blend ends the line.
                if (!blend(cell_cached, nxp, nyp, nzp, vx, vy, vz, wx, wy, wz)) return true;
            }
            bool isdiff = false;
            if (LCM) {
                // stream_pick_by_lcm! (stream.jl:380-495), after the angle pick above set W.ivec_next (stream.jl:530-531)
                const int ivec_ang = ivec;
                int dvx = (int)rintf(px) - (ix + 1), dvy = (int)rintf(py) - (iy + 1), dvz = (int)rintf(pz) - (iz + 1);   // :394-398
                if (dvx == 0 && dvy == 0 && dvz == 0) {           // not entering a new voxel, :400-413
                    float4 w;                                     // (the voxel's vectors are in registers when their count is a template constant)
                    if constexpr (NVEC > 0) { w = cvec[0]; for (int k = 1; k < NVEC; k++) if (ivec == k) w = cvec[k]; }
                    else w = cand[ivec];
                    if (dot3(vx, vy, vz, w.x, w.y, w.z) > 0.0f) { wx = w.x; wy = w.y; wz = w.z; } else { wx = -w.x; wy = -w.y; wz = -w.z; }
                } else {
                    int entry = lcm_match_edge(dvx, dvy, dvz, a.sd0, a.sd1);                         // :416-422
                    if (entry == 0) {                             // diagonal jump: keep the dimension that changes faster, :424-438
                        const float p1 = a.sd0 == 0 ? px : (a.sd0 == 1 ? py : pz), q1 = a.sd0 == 0 ? nxp : (a.sd0 == 1 ? nyp : nzp);
                        const float p2 = a.sd1 == 0 ? px : (a.sd1 == 1 ? py : pz), q2 = a.sd1 == 0 ? nxp : (a.sd1 == 1 ? nyp : nzp);
                        const int zap = fabsf(p1 - q1) < fabsf(p2 - q2) ? a.sd1 : a.sd0;
                        if (zap == 0) dvx = 0; else if (zap == 1) dvy = 0; else dvz = 0;
                        entry = lcm_match_edge(dvx, dvy, dvz, a.sd0, a.sd1);
                    }
                    const float *lp = a.lcm + (size_t)vox * 10;
                    float lcm[10];
                    bool any = false;
#pragma unroll
                    for (int j = 0; j < 10; j++) {                // :441-446
                        const int e0 = j < 4 ? 1 : (j < 7 ? 2 : (j < 9 ? 3 : 4));
                        const int e1 = j < 4 ? j + 1 : (j < 7 ? j - 2 : (j < 9 ? j - 4 : 4));
                        lcm[j] = (e0 == entry || e1 == entry) ? lp[j] : 0.0f;
                        any |= lcm[j] != 0.0f;
                    }
                    if (!any) return true;                        // :448, :492
                    float sum = lcm[0];
#pragma unroll
                    for (int j = 1; j < 10; j++) sum += lcm[j];
                    // lcm ./ sum (:450): ten IEEE divisions by one divisor.  Every entry is 0 or >= lcm_thresh (lcm_prepare_kernel), so with a threshold
                    // >= 2^-40 and a sum <= 2^40 neither operand nor quotient comes near the ends of the exponent range and the
                    // division's expansion without scaling and fix-up gives the same bits (as normalise3): ONE refined reciprocal, two
                    // residual corrections per quotient -- 5 instructions each instead of 11.
                    if (a.lcm_plain && sum <= 0x1p40f) {
                        float rc = __builtin_amdgcn_rcpf(sum);
                        rc = fmaf(fmaf(-sum, rc, 1.0f), rc, rc);
#pragma unroll
                        for (int j = 0; j < 10; j++) {
                            float q = lcm[j] * rc;
                            q = fmaf(fmaf(-sum, q, lcm[j]), rc, q);
                            lcm[j] = fmaf(fmaf(-sum, q, lcm[j]), rc, q);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 10; j++) lcm[j] = lcm[j] / sum;
                    }
                    const float u = fib_uniform(a.rng_seed, (unsigned long long)line, ndraw++);
                    int il = 0;                                   // rand(Categorical(lcm)): first index whose running sum exceeds u
                    float cp = lcm[0];
#pragma unroll
                    for (int j = 1; j < 10; j++) { const bool go = cp <= u && il == j - 1; if (go) { cp += lcm[j]; il = j; } }
                    const int e0 = il < 4 ? 1 : (il < 7 ? 2 : (il < 9 ? 3 : 4));
                    const int e1 = il < 4 ? il + 1 : (il < 7 ? il - 2 : (il < 9 ? il - 4 : 4));
                    const int exitedge = e0 == entry ? e1 : e0;  // :454-456
                    const float ex = (float)lcm_dxyz(exitedge, 0, a.sd0, a.sd1), ey = (float)lcm_dxyz(exitedge, 1, a.sd0, a.sd1),
                                ez = (float)lcm_dxyz(exitedge, 2, a.sd0, a.sd1);
                    float lx = 0.0f, ly = 0.0f, lz = 0.0f, lc = 0.0f, la = 0.0f;
                    int lb = 0;
#pragma unroll
                    for (int k = 0; k < nvec; k++) {              // :462-472
                        const float4 w = NVEC > 0 ? cvec[k < NCV ? k : 0] : cand[k];
                        float c, ca;
                        if (is_zero3(w.x, w.y, w.z)) { c = -INFINITY; ca = -INFINITY; }
                        else { c = dot3(ex, ey, ez, w.x, w.y, w.z); ca = fabsf(c); }
                        if (k == 0 || __float_as_int(ca) > __float_as_int(la)) { lb = k; la = ca; lc = c; lx = w.x; ly = w.y; lz = w.z; }
                    }
                    if (!(fabsf(lc) < INFINITY)) return true;     // :476
                    if (lc > 0.0f) { wx = lx; wy = ly; wz = lz; } else { wx = -lx; wy = -ly; wz = -lz; }   // :480-484
                    ivec = lb;                                    // :486
                }
                isdiff = ivec != ivec_ang;                        // :538
            }
            // push!/prepend! of pos_now (stream.jl:660): the slot of this trip
            // LCM runs: the method-difference flag of the point (stream.jl:666) rides in the sign bit of x (x > 0)
            {
                float *sp = stage + (trip & 3) * SCR_SLOT_FLOATS + tj * 3;
                sp[0] = (LCM && isdiff) ? -px : px; sp[1] = py; sp[2] = pz;
            }
            emitted = true;
            npts++;                                               // (nf = the count when the forward pass ends: below)
            if (!LCM && dot3(vx, vy, vz, wx, wy, wz) < a.cosang) return true;   // stream.jl:670 (not used with LCMs, :668)
            if (npts > a.len_max) return true;                    // stream.jl:674
            if (a.smooth != 0.0f) {                               // stream.jl:677-681
                wx = a.smooth * vx + omc * wx;
                wy = a.smooth * vy + omc * wy;
                wz = a.smooth * vz + omc * wz;
                normalise3(wx, wy, wz, a.norm_generic != 0);
            }
            px = nxp; py = nyp; pz = nzp;                         // stream.jl:684-685
            vx = wx; vy = wy; vz = wz;
        }
        return false;
    };
    // [r4] ONE loop for both passes: a lane whose forward pass ends turns round on the spot (back to the seed, opposite direction,
    // stream.jl:649-650 with dir = -1) while its neighbours go on, so a wave runs max(forward + backward trips) over its lanes --
    // with one loop per pass it ran max(forward) + max(backward): 1.5 x the trips on the benchmark field, whose lines all use up
    // len_max but split it differently between the two directions.  The trip counter is wave-uniform, and so is the scratch slot
    // a trip writes (the 64 lanes' points of a trip are 4 x 192-byte rows): forward point i sits in slot i, backward
    // point j in slot nf + gap + j, gap = 1 if the forward pass ended on a trip that emitted nothing (a failed step).
    auto flush = [&](int t0) {                                   // slots t0 .. t0 + 3 of the wave's four tiles: whole lines
        typedef float nt4_t __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_wave_barrier();                          // (LDS is in order within a wave: the lanes' points are there)
#ifdef FIB_AB_VARIANTS
        if (!(a.dbg & 2))
#endif
        if (tile_ok) {
            nt4_t *g = reinterpret_cast<nt4_t *>(tile0 + (int64_t)t0 * SCR_SLOT_FLOATS);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const nt4_t q = reinterpret_cast<const nt4_t *>(stage)[tj + 16 * k];
#ifdef FIB_AB_VARIANTS
                if (a.scratch_plain) { store_x4_variant(g + tj + 16 * k, q, a.scratch_plain); continue; }
#endif
                __builtin_nontemporal_store(q, g + tj + 16 * k);
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    bool dead = !live_line;
    for (;;) {
        if (!dead) {
            const bool ended = step();
            if (ended) {
                if (pass == 1) dead = true;
                else {
                    pass = 1;
                    nf = npts;                                    // the forward pass's points
                    gap = emitted ? 0 : 1;
                    px = p0x; py = p0y; pz = p0z;
                    const float4 s = a.field[lin * nvec + ivec];  // view(W.ovecs, :, ivec_next, seed...), stream.jl:650
                    vx = s.x * -1.0f; vy = s.y * -1.0f; vz = s.z * -1.0f;
                }
            }
        }
        if ((trip & 3) == 3) flush(trip - 3);
        trip++;
        if (__ballot(!dead) == 0ull) break;                       // (wave-uniform)
    }
    if (trip & 3) flush(trip & ~3);                               // (the last, partial group: its unused slots carry stale points nobody reads)
    if (live_line) { a.npts[li] = npts; a.nfwd[li] = nf | (gap << 30); }
    if constexpr (FUSED) fused_pack_block<NVEC>(a, wg, li, live_line, npts, nf, gap);
}

// Divergent termination (lines of a wave end at different steps: 30-53 % of the lane-steps idle on a phantom with a broad length
// distribution, 8 % on the benchmark field).  Four remedies were built, each bit-identical to this kernel, and each measured slower
// on every workload (tools/trace_divergence.py; profiles/r03/trace_compaction.log): a per-lane state machine over one
// flat step loop that refills finished lanes from a queue (round 2, two forms); rounds of launches with the surviving lines
// compacted into a dense list in between (one returning atomic per hand-over on one word: ~88 / us); persistent waves that stash
// their surviving lines in LDS and refill from their own share of the lines, with the two passes as two launches of a flat loop
// (static shares: tail imbalance; a chunked global queue: the atomic rate again).  One lane per line is final; the source of the
// others is in the repository's history.
// ---- microscopy regime: stream_micro_new_point! (stream.jl:547-619) -------------------------------------------
// The next point is the voxel, among those within search_dist voxels of the tentative position and inside a cone of
// search_ang around the current direction, whose first orientation vector is best aligned with the current direction
// (first maximum of |cos| in the column-major order of the (2d+1)^3 search cube; the position snaps to that voxel).
// One wave per line: the 64 lanes share out the cells of the search ball each step.  The unit vectors of the cells
// (search_area, stream.jl:255-277) sit in LDS, one entry per antipodal pair (v(-cell) = -v(cell) exactly, and so is
// its dot product).  The centre cell's vector is 0/0 = NaN, which passes `iszero` and the `<=` cone test in the
// reference: the tentative voxel itself is always a candidate (lane 0 adds it).
__device__ __forceinline__ unsigned long long micro_key(float c, unsigned lin) {
    const float ca = fabsf(c);
    unsigned hi = __float_as_uint(ca);                            // |c| >= 0: the bit pattern is order preserving
    if (ca != ca) hi = 0xffffffffu;                               // NaN wins (Base.argmax)
    return ((unsigned long long)hi << 32) | (unsigned)(~lin);     // ties: the smaller linear index
}

__global__ __launch_bounds__(1024) void stream_trace_micro_kernel(const TraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 stab[];  // [nsearch] entries, then [G^3 + 1] cell offsets
    int32_t *cst = reinterpret_cast<int32_t *>(stab + a.nsearch);
    for (int i = threadIdx.x; i < a.nsearch; i += blockDim.x) stab[i] = a.search[i];
    for (int i = threadIdx.x; i <= a.G * a.G * a.G; i += blockDim.x) cst[i] = a.cell_start[i];
    __syncthreads();
    const float gh = 2.0f / (float)a.G;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int dx = a.sdx, dy = a.sdy, dz = a.sdz, Sx = 2 * dx + 1, Sy = 2 * dy + 1, Sz = 2 * dz + 1;
    const unsigned lin_centre = (unsigned)(dx + Sx * (dy + Sy * dz)), lin_last = (unsigned)(Sx * Sy * Sz - 1);
    constexpr int64_t slot_floats = SCR_SLOT_FLOATS;
    const float fnx = (float)a.nx, fny = (float)a.ny, fnz = (float)a.nz;
    const float omc = 1.0f - a.smooth;
    for (int64_t li = wave0; li < a.nlines; li += nwaves) {
        const int64_t line = a.line0 + li;
        const int64_t iseed = line / a.nsub;
        const int isub = (int)(line - iseed * a.nsub);
        const int64_t lin = a.seeds[iseed];
        const int sx = (int)(lin % a.nx), sy = (int)((lin / a.nx) % a.ny), sz = (int)(lin / ((int64_t)a.nx * a.ny));
        const float p0x = (float)(sx + 1) + a.sublist[3 * isub];
        const float p0y = (float)(sy + 1) + a.sublist[3 * isub + 1];
        const float p0z = (float)(sz + 1) + a.sublist[3 * isub + 2];
        float *dcur = a.scratch + scratch_line_base(li, a.nslots);   // next slot: the line's points one after the other (gap 0)
        int npts = 0, nf = 0;
        for (int pass = 0; pass < 2; pass++) {
            const float fwd = pass == 0 ? 1.0f : -1.0f;
            float px = p0x, py = p0y, pz = p0z;
            const float4 s = a.field[lin * a.nvec];               // the first vector of the seed voxel (W.ivec_next stays 1)
            float vx = s.x * fwd, vy = s.y * fwd, vz = s.z * fwd;
            for (;;) {
                const float nxp = px + vx * a.step, nyp = py + vy * a.step, nzp = pz + vz * a.step;   // stream.jl:561
                const float rx = rintf(nxp), ry = rintf(nyp), rz = rintf(nzp);                        // :563
                if (!(rx >= 1.0f && rx <= fnx && ry >= 1.0f && ry <= fny && rz >= 1.0f && rz <= fnz)) break;   // :566
                const int cx = (int)rx - 1, cy = (int)ry - 1, cz = (int)rz - 1;                       // 0-based
                const float4 fc = a.field[((int64_t)cx + a.nx * ((int64_t)cy + (int64_t)a.ny * cz)) * a.nvec];
                if (fc.w == 0.0f) break;                                                              // :569
                unsigned long long best = 0ull;                  // 0 = nothing found (every real key has |c| bits or ~lin != 0)
                if (lane == 0) best = micro_key(dot3(vx, vy, vz, fc.x, fc.y, fc.z), lin_centre);     // the centre cell
                // Entries that can pass dot(u, v) > c lie within |v - u/|u|| < sqrt(2 - 2c/|u|) of the (normalised) direction:
                // only the direction cells that box touches are visited (the test itself stays exact); sg = 1 visits the
                // antipodes (dot(u, -v) > c  <=>  v near -u).  A degenerate direction falls back to the whole table.
                const float un = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
                const float r2 = 2.0f - 2.0f * a.search_cosang / un;
                const bool boxed = un > 0.0f && r2 < 1.0f;           // NaN / zero / very short vectors: everything
                const float rr = boxed ? sqrtf(r2 > 0.0f ? r2 : 0.0f) + 2e-3f : 3.0f;
                auto test_entry = [&](int e, int sg) {
                    const float4 t = stab[e];
                    const float sdot = dot3(vx, vy, vz, t.x, t.y, t.z);
                    const float dv = sg ? -sdot : sdot;
                    if (dv <= a.search_cosang) return;                                                // :597-598
                    const unsigned cell = __float_as_uint(t.w);
                    const int kx = (int)(cell & 255u), ky = (int)((cell >> 8) & 255u), kz = (int)(cell >> 16);
                    const int ox = sg ? dx - kx : kx - dx, oy = sg ? dy - ky : ky - dy, oz = sg ? dz - kz : kz - dz;
                    const int ix = cx + ox, iy = cy + oy, iz = cz + oz;
                    if (ix < 0 || ix >= a.nx || iy < 0 || iy >= a.ny || iz < 0 || iz >= a.nz) return;   // :586-588
                    const float4 f = a.field[((int64_t)ix + a.nx * ((int64_t)iy + (int64_t)a.ny * iz)) * a.nvec];
                    if (f.w == 0.0f) return;                                                          // :596
                    const unsigned l0 = (unsigned)(kx + Sx * (ky + Sy * kz));
                    const unsigned long long k = micro_key(dot3(vx, vy, vz, f.x, f.y, f.z), sg ? lin_last - l0 : l0);   // :600-601
                    best = k > best ? k : best;
                };
                if (!boxed) {
                    for (int e = lane; e < a.nsearch; e += 64) { test_entry(e, 0); test_entry(e, 1); }
                } else {
#pragma unroll 1
                    for (int sg = 0; sg < 2; sg++) {
                        const float qx = (sg ? -vx : vx) / un, qy = (sg ? -vy : vy) / un, qz = (sg ? -vz : vz) / un;
                        auto cl = [&](float x) { int c = (int)floorf((x + 1.0f) / gh); return c < 0 ? 0 : (c >= a.G ? a.G - 1 : c); };
                        const int x0 = cl(qx - rr), x1 = cl(qx + rr), y0 = cl(qy - rr), y1 = cl(qy + rr), z0 = cl(qz - rr), z1 = cl(qz + rr);
                        for (int gz = z0; gz <= z1; gz++)
                            for (int gy = y0; gy <= y1; gy++) {
                                const int rowc = a.G * (gy + a.G * gz);
                                const int e0 = cst[rowc + x0], e1 = cst[rowc + x1 + 1];   // cells x0..x1 of this row are contiguous
                                for (int e = e0 + lane; e < e1; e += 64) test_entry(e, sg);
                            }
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const unsigned long long o = ((unsigned long long)(unsigned)__shfl_xor((int)(best >> 32), off) << 32) |
                                                 (unsigned)__shfl_xor((int)(unsigned)best, off);
                    best = o > best ? o : best;
                }
                if (best == 0ull) break;                          // (cannot happen: the centre is always a candidate)
                const unsigned bl = ~(unsigned)best;              // argmax cell, column-major in the cube
                const int bx = cx + (int)(bl % (unsigned)Sx) - dx, by = cy + (int)((bl / (unsigned)Sx) % (unsigned)Sy) - dy,
                          bz = cz + (int)(bl / (unsigned)(Sx * Sy)) - dz;
                const float4 fb = a.field[((int64_t)bx + a.nx * ((int64_t)by + (int64_t)a.ny * bz)) * a.nvec];
                const float bc = dot3(vx, vy, vz, fb.x, fb.y, fb.z);
                if (!(fabsf(bc) < INFINITY)) break;               // !isfinite, :609
                float wx, wy, wz;
                if (bc > 0.0f) { wx = fb.x; wy = fb.y; wz = fb.z; } else { wx = -fb.x; wy = -fb.y; wz = -fb.z; }   // :616-620
                if (lane == 0) store_point(dcur, px, py, pz);                    // addpt!(strline, pos_now), stream.jl:660
                dcur += slot_floats;
                npts++;
                if (pass == 0) nf++;
                if (dot3(vx, vy, vz, wx, wy, wz) < a.cosang) break;   // :670
                if (npts > a.len_max) break;                          // :674
                if (a.smooth != 0.0f) {                               // :677-681
                    wx = a.smooth * vx + omc * wx;
                    wy = a.smooth * vy + omc * wy;
                    wz = a.smooth * vz + omc * wz;
                    normalise3(wx, wy, wz, a.norm_generic != 0);
                }
                px = (float)(bx + 1); py = (float)(by + 1); pz = (float)(bz + 1);   // the position snaps to the voxel found, :612-614
                vx = wx; vy = wy; vz = wz;
            }
        }
        if (lane == 0) { a.npts[li] = npts; a.nfwd[li] = nf; }
    }
}

// ---- exclusive scan of (kept ? npts : 0, kept ? 1 : 0) over the lines, int64 pairs --------------------
constexpr int SCAN_T = 256, SCAN_E = 8, SCAN_B = SCAN_T * SCAN_E;
static_assert(SCAN_B == TRACE_SCAN_B, "scan block size");

__global__ __launch_bounds__(SCAN_T) void scan_block_kernel(const int32_t *npts, int64_t n, int len_min,
                                                            Pair *excl, Pair *block_tot) {
    __shared__ Pair sh[SCAN_T];
    const int64_t base = (int64_t)blockIdx.x * SCAN_B + (int64_t)threadIdx.x * SCAN_E;
    Pair loc[SCAN_E], run{0, 0};
#pragma unroll
    for (int e = 0; e < SCAN_E; e++) {
        const int64_t i = base + e;
        const int np = i < n ? npts[i] : 0;
        const bool keep = i < n && np >= len_min;                 // size(strline, 2) < W.len_min && continue, stream.jl:769
        loc[e] = run;
        run.pts += keep ? np : 0;
        run.lines += keep ? 1 : 0;
    }
    sh[threadIdx.x] = run;
    __syncthreads();
    for (int off = 1; off < SCAN_T; off <<= 1) {
        Pair t{0, 0};
        if ((int)threadIdx.x >= off) t = sh[threadIdx.x - off];
        __syncthreads();
        sh[threadIdx.x].pts += t.pts; sh[threadIdx.x].lines += t.lines;
        __syncthreads();
    }
    const Pair before = threadIdx.x ? sh[threadIdx.x - 1] : Pair{0, 0};
#pragma unroll
    for (int e = 0; e < SCAN_E; e++) {
        const int64_t i = base + e;
        if (i < n) excl[i] = Pair{loc[e].pts + before.pts, loc[e].lines + before.lines};
    }
    if (threadIdx.x == SCAN_T - 1) block_tot[blockIdx.x] = sh[SCAN_T - 1];
}

// exclusive scan of the per-block totals in place (single workgroup, chunks of SCAN_T with a running carry)
// base (optional): the totals of everything before this batch of lines -- the offsets start there and *total continues from it
__global__ __launch_bounds__(SCAN_T) void scan_totals_kernel(Pair *block_tot, int nblocks, Pair *total, const Pair *base = nullptr, int64_t *counts = nullptr) {
    __shared__ Pair sh[SCAN_T];
    Pair carry = base ? *base : Pair{0, 0};
    for (int base = 0; base < nblocks; base += SCAN_T) {
        const int i = base + (int)threadIdx.x;
        const Pair mine = i < nblocks ? block_tot[i] : Pair{0, 0};
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < SCAN_T; off <<= 1) {
            Pair t{0, 0};
            if ((int)threadIdx.x >= off) t = sh[threadIdx.x - off];
            __syncthreads();
            sh[threadIdx.x].pts += t.pts; sh[threadIdx.x].lines += t.lines;
            __syncthreads();
        }
        const Pair incl = sh[threadIdx.x], last = sh[SCAN_T - 1];
        if (i < nblocks) block_tot[i] = Pair{carry.pts + incl.pts - mine.pts, carry.lines + incl.lines - mine.lines};
        carry.pts += last.pts; carry.lines += last.lines;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (counts) { counts[0] = carry.lines; counts[1] = carry.pts; }   // (fibd_stream_run_enqueue: {lines, points} for the caller)
    }
}

#include "xfm_apply.inc"
#include "stream_pack.inc"   // PackArgs, the tile packer, stream_pack_kernel / stream_pack_tile_kernel, fused_pack_block

__global__ __launch_bounds__(256) void copy_i32_kernel(const int32_t *src, int32_t *dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

}  // namespace

// Caller-owned, grow-only scratch arena of the tracer (fib_stream_params::ws): avoids a multi-GB hipMalloc/hipFree per job.
// A job holds it through a ScratchLease (below), which is the only code that takes, grows and gives back the arena.
struct fib_stream_ws {
    int device = 0;
    std::mutex mu;
    void *p = nullptr;
    size_t bytes = 0;
    bool busy = false, pending = false;
    hipEvent_t done = nullptr;
};

extern "C" int fibd_stream_ws_create(int device, fib_stream_ws **ws) try {
    FIB_CHECK(ws != nullptr, FIB_ERR_INVALID, "NULL argument");
    *ws = nullptr;
    fib::DeviceGuard guard;
    int rc = fib::use_device(device);
    if (rc != FIB_OK) return rc;
    fib_stream_ws *w = new fib_stream_ws();
    w->device = device;
    if (hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess) { delete w; return fib::fail(FIB_ERR_HIP, "hipEventCreate failed"); }
    *ws = w;
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fibd_stream_ws_destroy(fib_stream_ws *ws) try {
    if (!ws) return;
    fib::DeviceGuard guard;
    (void)hipSetDevice(ws->device);
    if (ws->pending) (void)hipEventSynchronize(ws->done);
    if (ws->p) (void)hipFree(ws->p);
    if (ws->done) (void)hipEventDestroy(ws->done);
    delete ws;
} FIB_API_CATCH_VOID

namespace {
// The scratch of nlines lines of up to len_max points: ONE block of device memory, each region rounded up to 256 bytes -- the point
// rows (TraceArgs::scratch), npts and nfwd [nlines] int32, the scan's exclusive prefixes [nlines] Pair (the fused kernel's look-back
// granules instead), the scan blocks' totals [nblocks] Pair and the call's totals (one Pair).
struct ScratchLayout {
    struct Regions { float *points; int32_t *npts, *nfwd; Pair *excl, *block_tot, *total; };
    int64_t nlines = 0;
    int stride = 0, nslots = 0, nblocks = 0;
    size_t off_npts = 0, off_nfwd = 0, off_excl = 0, off_btot = 0, off_total = 0, bytes = 0;   // byte offsets (the points at 0); the size
    ScratchLayout() = default;
    ScratchLayout(int64_t nl, int len_max)
        : nlines(nl), stride(len_max + 2),
          nslots((len_max + 4 + 3) & ~3),   // trips of a line's loop: <= len_max + 1 points + two failed steps; whole groups of four (the tracer stores four slots together)
          nblocks((int)fib::cdiv(nl, SCAN_B)) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        off_npts = up((size_t)fib::cdiv(nl, SCR_ROW) * SCR_ROW * nslots * 3 * sizeof(float));
        off_nfwd = off_npts + up((size_t)nl * sizeof(int32_t));
        off_excl = off_nfwd + up((size_t)nl * sizeof(int32_t));
        off_btot = off_excl + up((size_t)nl * sizeof(Pair));
        off_total = off_btot + up((size_t)nblocks * sizeof(Pair));
        bytes = off_total + up(sizeof(Pair));
    }
    Regions at(void *base) const {
        char *b = static_cast<char *>(base);
        return {reinterpret_cast<float *>(b), reinterpret_cast<int32_t *>(b + off_npts), reinterpret_cast<int32_t *>(b + off_nfwd),
                reinterpret_cast<Pair *>(b + off_excl), reinterpret_cast<Pair *>(b + off_btot), reinterpret_cast<Pair *>(b + off_total)};
    }
};

// The scratch a job holds (include/fibers_hip.h): the caller's arena when it is free and on the job's device, else device memory of
// the job's own.  The arena changes hands in stream order, so a pack kernel still reading it is never overtaken: release() -- also
// when the lease ends -- records an event on `last`, the stream of the holder's latest launch, and acquire() makes the next holder's
// stream wait for it (the host waits instead when that wait cannot be enqueued, and before the arena grows).  The job's own memory is
// freed once `last` is done.
struct ScratchLease {
    fib_stream_ws *ws = nullptr;    // the arena held, or NULL: p is the job's own
    void *p = nullptr;
    hipStream_t last = nullptr;
    ScratchLease() = default;
    ScratchLease(const ScratchLease &) = delete;
    ScratchLease &operator=(const ScratchLease &) = delete;
    ~ScratchLease() { release(); }

    int acquire(fib_stream_ws *arena, int device, size_t bytes, hipStream_t st) {
        last = st;
        auto alloc = [bytes](void **q) -> int {
            const hipError_t e = hipMalloc(q, bytes);
            if (e == hipSuccess) return FIB_OK;
            *q = nullptr;
            return fib::fail(FIB_ERR_NOMEM, "cannot allocate %zu bytes of streamline scratch: %s", bytes, hipGetErrorString(e));
        };
        if (arena) {
            std::lock_guard<std::mutex> lk(arena->mu);
            if (!arena->busy && arena->device == device) {
                if (arena->bytes < bytes) {
                    if (arena->pending) { (void)hipEventSynchronize(arena->done); arena->pending = false; }
                    if (arena->p) (void)hipFree(arena->p);
                    arena->bytes = 0;
                    const int rc = alloc(&arena->p);
                    if (rc != FIB_OK) return rc;
                    arena->bytes = bytes;
                }
                if (arena->pending) {
                    if (hipStreamWaitEvent(st, arena->done, 0) != hipSuccess) (void)hipEventSynchronize(arena->done);
                    arena->pending = false;
                }
                arena->busy = true;
                ws = arena; p = arena->p;
                return FIB_OK;
            }
        }
        return alloc(&p);
    }
    void release() {
        if (ws) {
            std::lock_guard<std::mutex> lk(ws->mu);
            ws->pending = hipEventRecord(ws->done, last) == hipSuccess;
            if (!ws->pending) (void)hipStreamSynchronize(last);
            ws->busy = false;
        } else if (p) {
            (void)hipStreamSynchronize(last);
            (void)hipFree(p);
        }
        ws = nullptr; p = nullptr;
    }
};
}  // namespace

struct fib_stream_job {
    int device = 0;
    int len_min = 0;
    ScratchLayout lay;
    ScratchLease scratch;           // (scratch.last: the stream of the job's latest launch -- trace or pack)
    int64_t kept_lines = 0, kept_pts = 0;
    bool lcm = false;               // LCM run: the method-difference flag rides in the sign bit of x until unpacked
};

extern "C" void fib_stream_job_destroy(fib_stream_job *job) try {
    if (!job) return;
    fib::DeviceGuard guard;
    (void)hipSetDevice(job->device);
    delete job;                     // (gives the scratch back)
} FIB_API_CATCH_VOID

extern "C" int fibd_stream_field(int32_t nvec, int64_t nvox, const float *const *ovec, const float *const *f,
                                 float f_thresh, const float *fa, float fa_thresh, const uint8_t *mask,
                                 float *field4, uint8_t *mask_out, void *stream) try {
    FIB_CHECK(ovec && field4 && nvox > 0, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nvec >= 1 && nvec <= 8, FIB_ERR_UNSUPPORTED, "1..8 orientation vectors per voxel are supported (got %d)", nvec);
    FieldArgs a{};
    for (int k = 0; k < nvec; k++) {
        FIB_CHECK(ovec[k] != nullptr, FIB_ERR_INVALID, "NULL orientation volume %d", k);
        a.ovec[k] = ovec[k];
        if (f) { FIB_CHECK(f[k] != nullptr, FIB_ERR_INVALID, "NULL amplitude volume %d", k); a.f[k] = f[k]; }
    }
    a.fa = fa; a.mask = mask; a.field = reinterpret_cast<float4 *>(field4); a.mask_out = mask_out;
    a.nvox = nvox; a.nvec = nvec; a.has_f = f ? 1 : 0; a.f_thresh = f_thresh; a.fa_thresh = fa_thresh;
    hipLaunchKernelGGL(stream_field_kernel, dim3((unsigned)fib::cdiv(nvox, 256)), dim3(256), 0, (hipStream_t)stream, a);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

namespace {
// 2^28 vectors of 16 bytes = 4 GiB: from there on the gather offsets need 64 bits (stream_trace_kernel<.., WIDE>)
// (diagnostic build: FIBERS_STREAM_WIDE=1 takes the wide form on any field -- tools/stream_wide_check.py compares it with the 32-bit form)
bool field_is_wide(const fib_stream_params *prm) {
    return (int64_t)prm->nx * prm->ny * prm->nz * prm->nvec >= ((int64_t)1 << 28) || fib::ab_env("FIBERS_STREAM_WIDE") != nullptr;
}

// the checks fibd_stream_trace and fibd_stream_run share (after their NULL checks); each entry point adds those of its own modes
int check_args(const fib_stream_params *prm, const int64_t *seeds, int64_t nseed, const float *sublist, int32_t nsub) {
    FIB_CHECK(nseed >= 0 && (nseed == 0 || seeds), FIB_ERR_INVALID, "invalid seed list");
    FIB_CHECK(nsub >= 1 && sublist, FIB_ERR_INVALID, "sublist must hold at least one offset (use [0,0,0] for nsub=0, stream.jl:180)");
    FIB_CHECK(prm->nx > 0 && prm->ny > 0 && prm->nz > 0 && prm->nvec >= 1 && prm->nvec <= 8, FIB_ERR_INVALID, "invalid volume / nvec");
    FIB_CHECK(prm->len_max >= 0 && prm->len_max < (1 << 24), FIB_ERR_INVALID, "invalid len_max");
    FIB_CHECK(prm->interp >= FIB_STREAM_NEAREST && prm->interp <= FIB_STREAM_TRILINEAR_RK4, FIB_ERR_INVALID,
              "interp must be 0 (nearest voxel, the reference), 1 (trilinear), 2 (trilinear, RK2) or 3 (trilinear, RK4)");
    FIB_CHECK((int64_t)prm->nx * prm->ny * prm->nz < ((int64_t)1 << 40), FIB_ERR_UNSUPPORTED, "volumes of 2^40 voxels or more are not supported");
    return FIB_OK;
}

// TraceArgs of a trace of every line into the regions buf (the fields of the microscopy, LCM and fused forms are their callers')
TraceArgs trace_args(const fib_stream_params *prm, const float *field4, const int64_t *seeds, const float *sublist, int32_t nsub,
                     const ScratchLayout &lay, const ScratchLayout::Regions &buf) {
    TraceArgs ta{};
    ta.field = reinterpret_cast<const float4 *>(field4); ta.seeds = seeds; ta.sublist = sublist;
    ta.scratch = buf.points; ta.npts = buf.npts; ta.nfwd = buf.nfwd;
    ta.line0 = 0; ta.nlines = lay.nlines;
    ta.nx = prm->nx; ta.ny = prm->ny; ta.nz = prm->nz; ta.nvec = prm->nvec; ta.nsub = nsub;
    ta.len_max = prm->len_max; ta.stride = lay.stride; ta.nslots = lay.nslots;
    ta.cosang = prm->cosang_thresh; ta.step = prm->step_size; ta.smooth = prm->smooth_coeff;
    { const char *e = fib::ab_env("FIBERS_STREAM_SCRATCH_PLAIN"); ta.scratch_plain = e ? std::atoi(e) : 0; }
    ta.norm_generic = fib::ab_env("FIBERS_STREAM_NORM_GENERIC") != nullptr;
    { const char *e = fib::ab_env("FIBERS_STREAM_DBG"); ta.dbg = e ? std::atoi(e) : 0; }
    return ta;
}

// PackArgs of a pack of every kept line of the regions buf into npts / seed_index / xyz (the .trk, LCM and capacity fields are the callers')
PackArgs pack_args(const ScratchLayout &lay, const ScratchLayout::Regions &buf, int len_min, int32_t *npts, int64_t *seed_index, float *xyz) {
    PackArgs pa{};
    pa.scratch = buf.points; pa.npts = buf.npts; pa.nfwd = buf.nfwd;
    pa.excl = buf.excl; pa.block_off = buf.block_tot;
    pa.out_npts = npts; pa.out_seed = seed_index; pa.out_xyz = xyz;
    pa.nlines = lay.nlines; pa.line0 = 0; pa.out_line0 = 0; pa.out_pt0 = 0;
    pa.stride = lay.stride; pa.nslots = lay.nslots; pa.len_min = len_min;
    pa.scratch_plain = fib::ab_env("FIBERS_STREAM_PACK_PLAIN") != nullptr;
    return pa;
}

// the one-lane-per-line tracer for (LCM, TRI); the vector count is a compile-time constant for 1, 2 and 3 vectors per voxel, wide
// fields take the run-time count (one instantiation per mode)
template <bool LCM, int TRI>
void launch_trace(const TraceArgs &ta, int nvec, bool wide, hipStream_t st) {
    const unsigned grid = (unsigned)fib::cdiv(ta.nlines, 256);
    if (wide)           hipLaunchKernelGGL((stream_trace_kernel<0, LCM, TRI, true>), dim3(grid), dim3(256), 0, st, ta);
    else if (nvec == 1) hipLaunchKernelGGL((stream_trace_kernel<1, LCM, TRI>), dim3(grid), dim3(256), 0, st, ta);
    else if (nvec == 2) hipLaunchKernelGGL((stream_trace_kernel<2, LCM, TRI>), dim3(grid), dim3(256), 0, st, ta);
    else if (nvec == 3) hipLaunchKernelGGL((stream_trace_kernel<3, LCM, TRI>), dim3(grid), dim3(256), 0, st, ta);
    else                hipLaunchKernelGGL((stream_trace_kernel<0, LCM, TRI>), dim3(grid), dim3(256), 0, st, ta);
}

// the scan of the traced lines: offsets of the kept lines and the totals (counts_dev != NULL: {lines, points} there too)
void scan_lines(const ScratchLayout &lay, const ScratchLayout::Regions &buf, int len_min, int64_t *counts_dev, hipStream_t st) {
    fib::ProfScope prof("stream_scan", st);
    hipLaunchKernelGGL(scan_block_kernel, dim3(lay.nblocks), dim3(SCAN_T), 0, st, buf.npts, lay.nlines, len_min, buf.excl, buf.block_tot);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(SCAN_T), 0, st, buf.block_tot, lay.nblocks, buf.total, (const Pair *)nullptr, counts_dev);
}

// macro-scale angle-picked tracking (nearest voxel or the trilinear option), then the scan
void trace_and_scan(const TraceArgs &ta, const fib_stream_params *prm, bool wide, const ScratchLayout &lay, const ScratchLayout::Regions &buf,
                    int64_t *counts_dev, hipStream_t st) {
    {
        fib::ProfScope prof("stream_trace", st);
        switch (prm->interp) {                                    // (check_args: 0 .. 3)
        case FIB_STREAM_NEAREST:       launch_trace<false, 0>(ta, prm->nvec, wide, st); break;
        case FIB_STREAM_TRILINEAR:     launch_trace<false, 1>(ta, prm->nvec, wide, st); break;
        case FIB_STREAM_TRILINEAR_RK2: launch_trace<false, 2>(ta, prm->nvec, wide, st); break;
        default:                       launch_trace<false, 3>(ta, prm->nvec, wide, st); break;
        }
    }
    scan_lines(lay, buf, prm->len_min, counts_dev, st);
}

struct LcmIn { const float *lcms = nullptr; float thresh = 0.0f; int sd0 = 0, sd1 = 1; unsigned long long seed = 0; };
int stream_trace_impl(const fib_stream_params *prm, const float *field4, const LcmIn &lin, const int64_t *seeds, int64_t nseed,
                      const float *sublist, int32_t nsub, void *stream,
                      fib_stream_job **job_out, int64_t *nlines_out, int64_t *npoints_out) {
    FIB_CHECK(prm && field4 && job_out && nlines_out && npoints_out, FIB_ERR_INVALID, "NULL argument");
    *job_out = nullptr;
    int rc = check_args(prm, seeds, nseed, sublist, nsub);
    if (rc != FIB_OK) return rc;
    FIB_CHECK(prm->search_dist <= 60, FIB_ERR_UNSUPPORTED, "search_dist up to 60 voxels is supported (got %d)", prm->search_dist);
    FIB_CHECK(prm->search_flat_axis >= 0 && prm->search_flat_axis <= 3, FIB_ERR_INVALID, "search_flat_axis must be 0 (none) or 1..3 (x, y, z)");
    FIB_CHECK(prm->interp == 0 || (prm->search_dist == 0 && !lin.lcms), FIB_ERR_UNSUPPORTED,
              "trilinear interpolation is an option of macro-scale angle-picked tracking only");
    const bool wide = field_is_wide(prm);
    int device = 0;
    FIB_HIP(hipGetDevice(&device));
    hipStream_t st = (hipStream_t)stream;
    std::unique_ptr<fib_stream_job> job(new (std::nothrow) fib_stream_job());
    FIB_CHECK(job != nullptr, FIB_ERR_NOMEM, "out of host memory");
    job->device = device; job->len_min = prm->len_min;
    job->lay = ScratchLayout(nseed * nsub, prm->len_max);
    const int64_t nl = job->lay.nlines;
    *nlines_out = 0; *npoints_out = 0;
    if (nl == 0) { *job_out = job.release(); return FIB_OK; }
    if ((rc = job->scratch.acquire(prm->ws, device, job->lay.bytes, st)) != FIB_OK) return rc;
    const ScratchLayout::Regions buf = job->lay.at(job->scratch.p);
    TraceArgs ta = trace_args(prm, field4, seeds, sublist, nsub, job->lay, buf);
    fib::DevBuf<float4> d_search;
    fib::DevBuf<int32_t> d_cell;
    fib::DevBuf<float> d_lcm;
    if (prm->search_dist > 0) {
        // search_area (stream.jl:255-277), Float32 arithmetic like the reference's T; one entry per antipodal pair
        const int d = prm->search_dist;
        int d3[3] = {d, d, d};
        if (prm->search_flat_axis >= 1 && prm->search_flat_axis <= 3) d3[prm->search_flat_axis - 1] = 0;   // micro_search_dist[thrudim] = 0, stream.jl:153-155
        const int Sx = 2 * d3[0] + 1, Sy = 2 * d3[1] + 1, Sz = 2 * d3[2] + 1;
        std::vector<float4> tab;
        const int64_t ncell = (int64_t)Sx * Sy * Sz;
        for (int64_t l = 0; l < ncell / 2; l++) {                 // the first half in column-major order; the centre is cell ncell/2
            const int kx = (int)(l % Sx), ky = (int)((l / Sx) % Sy), kz = (int)(l / ((int64_t)Sx * Sy));
            const float rx = (float)(kx - d3[0]) / ((float)d3[0] + 0.5f), ry = (float)(ky - d3[1]) / ((float)d3[1] + 0.5f),
                        rz = (float)(kz - d3[2]) / ((float)d3[2] + 0.5f);
            float q = rx * rx; q = q + ry * ry; q = q + rz * rz;
            const float r = sqrtf(q);
            if (!(r < 1.0f)) continue;
            const uint32_t cell = (uint32_t)kx | ((uint32_t)ky << 8) | ((uint32_t)kz << 16);
            float w; memcpy(&w, &cell, 4);
            tab.push_back(make_float4(rx / r, ry / r, rz / r, w));
        }
        // direction grid: cell size a little above the chord of the search cone, so a query box spans <= 3 cells per axis
        const float chord = std::sqrt(std::max(0.0f, 2.0f - 2.0f * prm->search_cosang));
        int G = (int)std::floor(2.0f / std::max(chord * 1.05f + 4e-3f, 0.1f));
        G = std::max(1, std::min(G, 24));
        const float gh = 2.0f / (float)G;
        auto cell_of = [&](const float4 &t) {
            auto cl = [&](float x) { int c = (int)std::floor((x + 1.0f) / gh); return c < 0 ? 0 : (c >= G ? G - 1 : c); };
            return cl(t.x) + G * (cl(t.y) + G * cl(t.z));
        };
        std::stable_sort(tab.begin(), tab.end(), [&](const float4 &p, const float4 &q) { return cell_of(p) < cell_of(q); });
        std::vector<int32_t> cstart((size_t)G * G * G + 1, 0);
        for (const float4 &t : tab) cstart[(size_t)cell_of(t) + 1]++;
        for (size_t i = 1; i < cstart.size(); i++) cstart[i] += cstart[i - 1];
        const size_t smem = tab.size() * sizeof(float4) + cstart.size() * sizeof(int32_t);
        if (smem > 150 * 1024) return fib::fail(FIB_ERR_UNSUPPORTED, "search_dist %d needs %zu bytes of LDS for the search table (max 150 KiB)", d, smem);
        if ((rc = d_search.alloc(tab.size())) != FIB_OK) return rc;
        if ((rc = d_cell.alloc(cstart.size())) != FIB_OK) return rc;
        hipError_t ec = hipMemcpyAsync(d_search.p, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice, st);
        if (ec == hipSuccess) ec = hipMemcpyAsync(d_cell.p, cstart.data(), cstart.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (ec == hipSuccess) ec = hipStreamSynchronize(st);     // (the tables are locals: they must outlive the copies)
        if (ec != hipSuccess) return fib::fail(FIB_ERR_HIP, "search table upload failed: %s", hipGetErrorString(ec));
        ta.search = d_search.p; ta.nsearch = (int)tab.size(); ta.search_dist = d; ta.search_cosang = prm->search_cosang;
        ta.sdx = d3[0]; ta.sdy = d3[1]; ta.sdz = d3[2];
        ta.cell_start = d_cell.p; ta.G = G;
        int ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        const unsigned mg = (unsigned)std::min<int64_t>(ncu, fib::cdiv(nl, 16));
        ec = hipFuncSetAttribute(reinterpret_cast<const void *>(stream_trace_micro_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (ec != hipSuccess) return fib::fail(FIB_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(ec));
        {
            fib::ProfScope prof("stream_trace_micro", st);
            hipLaunchKernelGGL(stream_trace_micro_kernel, dim3(mg), dim3(1024), smem, st, ta);
        }
        scan_lines(job->lay, buf, prm->len_min, nullptr, st);
    } else if (lin.lcms) {
        const int64_t nvox = (int64_t)prm->nx * prm->ny * prm->nz;
        if ((rc = d_lcm.alloc((size_t)nvox * 10)) != FIB_OK) return rc;
        hipLaunchKernelGGL(lcm_prepare_kernel, dim3((unsigned)fib::cdiv(nvox, 256)), dim3(256), 0, st, lin.lcms, lin.thresh, nvox, d_lcm.p);
        ta.lcm = d_lcm.p; ta.sd0 = lin.sd0; ta.sd1 = lin.sd1; ta.rng_seed = lin.seed;
        ta.lcm_plain = lin.thresh >= 0x1p-40f && !ta.norm_generic;
        job->lcm = true;
        {
            fib::ProfScope prof("stream_trace_lcm", st);
            launch_trace<true, 0>(ta, prm->nvec, wide, st);
        }
        scan_lines(job->lay, buf, prm->len_min, nullptr, st);
    } else {
        trace_and_scan(ta, prm, wide, job->lay, buf, nullptr, st);
    }
    hipError_t e = hipGetLastError();
    Pair tot{0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&tot, buf.total, sizeof(Pair), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fib::fail(FIB_ERR_HIP, "streamline trace failed: %s", hipGetErrorString(e));
    job->kept_lines = tot.lines; job->kept_pts = tot.pts;
    *nlines_out = tot.lines; *npoints_out = tot.pts;
    *job_out = job.release();
    return FIB_OK;
}
}  // namespace

extern "C" int fibd_stream_trace(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                                 const float *sublist, int32_t nsub, void *stream,
                                 fib_stream_job **job_out, int64_t *nlines_out, int64_t *npoints_out) try {
    return stream_trace_impl(prm, field4, LcmIn{}, seeds, nseed, sublist, nsub, stream, job_out, nlines_out, npoints_out);
} FIB_API_CATCH

extern "C" int fibd_stream_trace_lcm(const fib_stream_params *prm, const float *field4, const float *lcms, float lcm_thresh,
                                     int32_t strdim0, int32_t strdim1, uint64_t rng_seed,
                                     const int64_t *seeds, int64_t nseed, const float *sublist, int32_t nsub, void *stream,
                                     fib_stream_job **job_out, int64_t *nlines_out, int64_t *npoints_out) try {
    FIB_CHECK(lcms != nullptr, FIB_ERR_INVALID, "NULL lcms volume");
    FIB_CHECK(strdim0 >= 0 && strdim0 < 3 && strdim1 >= 0 && strdim1 < 3 && strdim0 != strdim1, FIB_ERR_INVALID, "invalid in-plane dimensions");
    FIB_CHECK(prm && prm->search_dist == 0, FIB_ERR_UNSUPPORTED, "LCM-guided tracking is a macro-scale mode (search_dist must be 0)");
    LcmIn lin;
    lin.lcms = lcms; lin.thresh = lcm_thresh; lin.sd0 = strdim0; lin.sd1 = strdim1; lin.seed = rng_seed;
    return stream_trace_impl(prm, field4, lin, seeds, nseed, sublist, nsub, stream, job_out, nlines_out, npoints_out);
} FIB_API_CATCH

// flags[i] = sign bit of x of point i, then the sign is cleared (LCM runs; see stream_trace_kernel)
__global__ __launch_bounds__(256) void stream_unpack_flags_kernel(float *xyz, uint8_t *flags, int64_t npts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const float x = xyz[3 * i];
    if (flags) flags[i] = (__float_as_uint(x) >> 31) ? 1 : 0;
    xyz[3 * i] = fabsf(x);
}

// whole-tile kernel while 16 (len_max + 2) points (+ the .trk headers and the alignment slack) fit in LDS
template <bool XF = false>
static int launch_pack_n(const PackArgs &pa_in, hipStream_t st, bool *flags_done = nullptr) {
    PackArgs pa = pa_in;
    const size_t smem = ((size_t)PK_LINES * pa.stride * 3 + PK_LINES + 8) * sizeof(float) + (pa.lcm ? (((size_t)PK_LINES * pa.stride + 15) & ~(size_t)15) : 0);
    if (flags_done) *flags_done = smem <= 120 * 1024;          // (the wave-per-tile kernel below leaves the flag bit in x: the caller strips it)
    if (smem > 120 * 1024) { pa.lcm = 0; pa.out_flags = nullptr; }
    if (smem <= 120 * 1024) {
        if (smem > 48 * 1024)
            FIB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(stream_pack_tile_kernel<PK_LINES, 16, XF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL((stream_pack_tile_kernel<PK_LINES, 16, XF>), dim3((unsigned)fib::cdiv(pa.nlines, PK_LINES)), dim3(16 * PK_LINES), smem, st, pa);
    } else
        hipLaunchKernelGGL(stream_pack_kernel<XF>, dim3((unsigned)fib::cdiv(pa.nlines, PK_LINES * PK_WAVES)), dim3(PK_WAVES * 64), 0, st, pa);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

static int pack_plain(fib_stream_job *job, int32_t *npts, int64_t *seed_index, float *xyz, uint8_t *flags, bool *flags_done, void *stream) {
    FIB_CHECK(job != nullptr, FIB_ERR_INVALID, "job is NULL");
    if (job->kept_lines == 0) return FIB_OK;
    FIB_CHECK(npts && seed_index && xyz, FIB_ERR_INVALID, "NULL output buffer");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(job->device));
    PackArgs pa = pack_args(job->lay, job->lay.at(job->scratch.p), job->len_min, npts, seed_index, xyz);
    pa.lcm = job->lcm ? 1 : 0; pa.out_flags = job->lcm ? flags : nullptr;
    fib::ProfScope prof("stream_pack", (hipStream_t)stream);
    job->scratch.last = (hipStream_t)stream;
    return launch_pack_n(pa, (hipStream_t)stream, flags_done);   // (LCM jobs whose lines do not fit the tile kernel: x still carries the flag bit; the caller strips it)
}

extern "C" int fibd_stream_pack_flags(fib_stream_job *job, int32_t *npts, int64_t *seed_index, float *xyz, uint8_t *flags, void *stream) try {
    bool done = false;
    int rc = pack_plain(job, npts, seed_index, xyz, flags, &done, stream);
    if (rc != FIB_OK || job->kept_pts == 0) return rc;
    if (job->lcm && done) return FIB_OK;                        // (the pack kernel stripped the flag bits and wrote the flags)
    if (job->lcm)
        hipLaunchKernelGGL(stream_unpack_flags_kernel, dim3((unsigned)fib::cdiv(job->kept_pts, 256)), dim3(256), 0, (hipStream_t)stream, xyz, flags, job->kept_pts);
    else if (flags) FIB_HIP(hipMemsetAsync(flags, 0, (size_t)job->kept_pts, (hipStream_t)stream));
    else return FIB_OK;
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fibd_stream_pack(fib_stream_job *job, int32_t *npts, int64_t *seed_index, float *xyz, void *stream) try {
    return fibd_stream_pack_flags(job, npts, seed_index, xyz, nullptr, stream);   // (strips the flag bit of LCM runs)
} FIB_API_CATCH

// fibd_stream_pack_trk and fibd_stream_pack_trk_xfm (vox2vox != NULL: the XF variant of the pack kernels)
static int pack_trk(fib_stream_job *job, const float *vox2vox, const float voxel_size[3], void *body, void *stream) {
    FIB_CHECK(job != nullptr && voxel_size != nullptr, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(!job->lcm, FIB_ERR_UNSUPPORTED, "the .trk body serialiser does not carry the per-point scalars of an LCM run");
    if (job->kept_lines == 0) return FIB_OK;
    FIB_CHECK(body != nullptr, FIB_ERR_INVALID, "NULL output buffer");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(job->device));
    PackArgs pa = pack_args(job->lay, job->lay.at(job->scratch.p), job->len_min, nullptr, nullptr, reinterpret_cast<float *>(body));
    pa.trk = 1; pa.vs[0] = voxel_size[0]; pa.vs[1] = voxel_size[1]; pa.vs[2] = voxel_size[2];
    if (vox2vox) memcpy(pa.xf.m, vox2vox, sizeof pa.xf.m);
    fib::ProfScope prof(vox2vox ? "stream_pack_trk_xfm" : "stream_pack_trk", (hipStream_t)stream);
    job->scratch.last = (hipStream_t)stream;
    return vox2vox ? launch_pack_n<true>(pa, (hipStream_t)stream) : launch_pack_n(pa, (hipStream_t)stream);
}

extern "C" int fibd_stream_pack_trk(fib_stream_job *job, const float voxel_size[3], void *body, void *stream) try {
    return pack_trk(job, nullptr, voxel_size, body, stream);
} FIB_API_CATCH

extern "C" int fibd_stream_pack_trk_xfm(fib_stream_job *job, const float vox2vox[16], const float voxel_size[3], void *body, void *stream) try {
    FIB_CHECK(vox2vox != nullptr, FIB_ERR_INVALID, "NULL argument");
    return pack_trk(job, vox2vox, voxel_size, body, stream);
} FIB_API_CATCH

// the fused trace + look-back + pack kernel for NVEC vectors per voxel (fibd_stream_run)
template <int NVEC>
static int launch_fused(const TraceArgs &ta, unsigned grid, size_t smem, hipStream_t st) {
    if (smem > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(stream_trace_kernel<NVEC, false, 0, false, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return fib::fail(FIB_ERR_HIP, "hipFuncSetAttribute failed");
    fib::ProfScope prof("stream_trace", st);
    hipLaunchKernelGGL((stream_trace_kernel<NVEC, false, 0, false, true>), dim3(grid), dim3(FUSED_BLOCK), smem, st, ta);
    return FIB_OK;
}

// stream (stream.jl:730-790) in ONE call, straight into the caller's buffers (no second call, no allocation by the library):
// trace, scan and pack one after the other on the caller's stream.  ([r5] the batched form -- a batch packed on a second stream
// while the next one is traced -- was measured slower for every batch count, 1.33 ... 1.55 ms against 1.30: both kernels are bound
// by the same HBM traffic, profiles/r04/negative_results.txt; it and its side stream / events have been removed.)
// Macro-scale angle picking only (nearest voxel or trilinear); the microscopy regime and LCM runs use fibd_stream_trace / _pack.
// counts_dev != NULL (fibd_stream_run_enqueue): the call returns once everything is enqueued; the stream writes {lines, points} there.
static int stream_run_impl(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                           const float *sublist, int32_t nsub, int32_t *npts, int64_t *seed_index, int64_t lines_cap,
                           float *xyz, int64_t points_cap, int64_t *nlines_out, int64_t *npoints_out, int64_t *counts_dev, void *stream) {
    FIB_CHECK(prm && field4 && (counts_dev || (nlines_out && npoints_out)), FIB_ERR_INVALID, "NULL argument");
    if (nlines_out) *nlines_out = 0;
    if (npoints_out) *npoints_out = 0;
    int rc = check_args(prm, seeds, nseed, sublist, nsub);
    if (rc != FIB_OK) return rc;
    FIB_CHECK(prm->search_dist == 0, FIB_ERR_UNSUPPORTED, "fibd_stream_run covers macro-scale tracking (search_dist 0); use fibd_stream_trace for the microscopy regime");
    FIB_CHECK(lines_cap >= 0 && points_cap >= 0 && (lines_cap == 0 || (npts && seed_index)) && (points_cap == 0 || xyz), FIB_ERR_INVALID, "invalid output buffers");
    const int64_t nl = nseed * nsub;
    hipStream_t st = (hipStream_t)stream;
    if (nl == 0) {
        if (counts_dev) FIB_HIP(hipMemsetAsync(counts_dev, 0, 2 * sizeof(int64_t), st));
        return FIB_OK;
    }
    const bool wide = field_is_wide(prm);
    int device = 0;
    FIB_HIP(hipGetDevice(&device));
    const ScratchLayout lay(nl, prm->len_max);
    ScratchLease scratch;                                          // (given back when the call returns)
    if ((rc = scratch.acquire(prm->ws, device, lay.bytes, st)) != FIB_OK) return rc;
    const ScratchLayout::Regions buf = lay.at(scratch.p);
    TraceArgs ta = trace_args(prm, field4, seeds, sublist, nsub, lay, buf);
    // [r5] FUSED (fused_pack_block): trace + look-back + pack in ONE launch, for nearest-voxel tracking with 1, 2 or 3 vectors per voxel on fields
    // below 2^28 vectors whose lines fit a 16-line LDS tile (len_max <= ~200) -- from 2^21 lines on: the fused kernel wins by overlapping
    // workgroups that pack with workgroups that still trace, which needs several rounds of workgroups per CU (measured, tools/stream_fused_ab.py:
    // 9.96 M lines x 3 vectors 9.7-10.6 ms against 11.5-11.8; 1 M lines 1.05-1.17 ms against 1.09-1.13: two rounds, no steady state).
    // Everything else takes the three launches below.  (Diagnostic build: FIBERS_STREAM_UNFUSED=1 / FIBERS_STREAM_FUSED=1 force either.)
    const size_t fsmem = std::max(((size_t)FUSED_TILE * lay.stride * 3 + FUSED_TILE + 8) * sizeof(float), (size_t)(FUSED_BLOCK / 16) * 4 * SCR_SLOT_FLOATS * sizeof(float));   // the pack's tile buffer; the trace loop parks four trips of points there
    const bool fused_ok = !wide && !prm->interp && prm->nvec >= 1 && prm->nvec <= 3 && fsmem <= 40 * 1024 &&
                          nl < ((int64_t)1 << 26) && nl * (int64_t)(prm->len_max + 2) < ((int64_t)1 << 36) &&
                          lay.off_btot - lay.off_excl >= ((size_t)fib::cdiv(nl, FUSED_BLOCK) + 1) * sizeof(unsigned long long);   // (the look-back state lives in excl)
    const bool fused = fused_ok && fib::ab_env("FIBERS_STREAM_UNFUSED") == nullptr && (nl >= ((int64_t)1 << 21) || fib::ab_env("FIBERS_STREAM_FUSED") != nullptr);
    if (fused) {
        const unsigned fgrid = (unsigned)fib::cdiv(nl, FUSED_BLOCK);
        ta.fstate = reinterpret_cast<unsigned long long *>(buf.excl);   // (the scan's array is free: no scan)
        ta.out_npts = npts; ta.out_seed = seed_index; ta.out_xyz = xyz; ta.ftotal = buf.total; ta.fcounts = counts_dev;
        ta.lines_cap = lines_cap; ta.points_cap = points_cap; ta.len_min = prm->len_min;
        if (hipMemsetAsync(ta.fstate, 0, ((size_t)fgrid + 1) * sizeof(unsigned long long), st) != hipSuccess)      // (+ the ticket counter behind the granules)
            return fib::fail(FIB_ERR_HIP, "hipMemsetAsync failed");
        // [r6] one code path per vector count 1..3 (DTI e1 | e1 + e2 or two peaks | three peaks)
        rc = prm->nvec == 1 ? launch_fused<1>(ta, fgrid, fsmem, st) : prm->nvec == 2 ? launch_fused<2>(ta, fgrid, fsmem, st) : launch_fused<3>(ta, fgrid, fsmem, st);
        if (rc != FIB_OK) return rc;
    } else {
        trace_and_scan(ta, prm, wide, lay, buf, counts_dev, st);
        if (hipGetLastError() != hipSuccess) return fib::fail(FIB_ERR_HIP, "streamline trace launch failed");
        PackArgs pa = pack_args(lay, buf, prm->len_min, npts, seed_index, xyz);
        pa.lines_cap = lines_cap; pa.points_cap = points_cap; pa.capped = 1;   // a line whose place lies beyond the buffers is dropped, the totals say what was needed
        fib::ProfScope prof("stream_pack", st);
        if ((rc = launch_pack_n(pa, st)) != FIB_OK) return rc;
    }
    if (hipGetLastError() != hipSuccess) return fib::fail(FIB_ERR_HIP, "streamline launch failed");
    if (counts_dev) return FIB_OK;                                 // ({lines, points} were written by the scan / the last workgroup: no host round trip)
    Pair tot{0, 0};
    hipError_t e = hipMemcpyAsync(&tot, buf.total, sizeof(Pair), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fib::fail(FIB_ERR_HIP, "streamline run failed: %s", hipGetErrorString(e));
    *nlines_out = tot.lines; *npoints_out = tot.pts;
    if (tot.lines > lines_cap || tot.pts > points_cap)
        return fib::fail(FIB_ERR_CAPACITY, "output buffers too small: %lld lines / %lld points needed, %lld / %lld given",
                         (long long)tot.lines, (long long)tot.pts, (long long)lines_cap, (long long)points_cap);
    return FIB_OK;
}

extern "C" int fibd_stream_run(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                               const float *sublist, int32_t nsub, int32_t *npts, int64_t *seed_index, int64_t lines_cap,
                               float *xyz, int64_t points_cap, int64_t *nlines_out, int64_t *npoints_out, void *stream) try {
    FIB_CHECK(nlines_out && npoints_out, FIB_ERR_INVALID, "NULL argument");
    return stream_run_impl(prm, field4, seeds, nseed, sublist, nsub, npts, seed_index, lines_cap, xyz, points_cap, nlines_out, npoints_out, nullptr, stream);
} FIB_API_CATCH

// [r5] fibd_stream_run without its host round trip: a step of a stream of volumes ends with a 16-byte download and a synchronisation
// during which the GPU idles (~45 us of C4's 1.03 ms between back-to-back calls); here the counts stay on the device.
extern "C" int fibd_stream_run_enqueue(const fib_stream_params *prm, const float *field4, const int64_t *seeds, int64_t nseed,
                                       const float *sublist, int32_t nsub, int32_t *npts, int64_t *seed_index, int64_t lines_cap,
                                       float *xyz, int64_t points_cap, int64_t *counts_dev, void *stream) try {
    FIB_CHECK(counts_dev != nullptr, FIB_ERR_INVALID, "NULL argument");
    return stream_run_impl(prm, field4, seeds, nseed, sublist, nsub, npts, seed_index, lines_cap, xyz, points_cap, nullptr, nullptr, counts_dev, stream);
} FIB_API_CATCH

extern "C" int fibd_stream_all_npts(fib_stream_job *job, int32_t *all_npts, void *stream) try {
    FIB_CHECK(job != nullptr, FIB_ERR_INVALID, "job is NULL");
    if (job->lay.nlines == 0) return FIB_OK;
    FIB_CHECK(all_npts != nullptr, FIB_ERR_INVALID, "NULL output buffer");
    fib::DeviceGuard guard;
    FIB_HIP(hipSetDevice(job->device));
    job->scratch.last = (hipStream_t)stream;
    hipLaunchKernelGGL(copy_i32_kernel, dim3((unsigned)fib::cdiv(job->lay.nlines, 256)), dim3(256), 0, (hipStream_t)stream,
                       job->lay.at(job->scratch.p).npts, all_npts, job->lay.nlines);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
} FIB_API_CATCH
