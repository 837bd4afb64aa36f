// stream_pack.inc -- the pack side of the tracer: scratch tiles -> the reference's packed lines (or a .trk body).  Textually included
// by stream.hip inside its anonymous namespace, behind the scan kernels and xfm_apply.inc (it needs Pair, TraceArgs, the SCR_* layout,
// SCAN_B and XfmMat).  Its parts:
//   pk_slot_pos, pk_line_head, pk_trk_point        the point order of a line, the place of a kept line, the .trk epilogue: every kernel here
//   pk_tile_summary, pk_gather, pk_stream_out      THE TILE PACKER: the kept lines of a 16-line scratch tile occupy ONE contiguous range of
//                                                  the output, so a workgroup assembles that range in LDS and streams it out aligned
//   stream_pack_kernel                             one wave per tile, no LDS range: lines longer than the LDS holds (its own algorithm)
//   stream_pack_tile_kernel                        the default pack: one workgroup per tile, two barriers
//   fused_pack_block                               the tail of the fused trace kernel: look-back, then its 32 tiles, three barriers per tile

struct PackArgs {
    const float *scratch;
    const int32_t *npts, *nfwd;
    const Pair *excl, *block_off;
    int32_t *out_npts;
    int64_t *out_seed;
    float *out_xyz;
    int64_t nlines, line0, out_line0, out_pt0;
    int stride, nslots, len_min, scratch_plain;
    int64_t lines_cap, points_cap;   // capped: a line whose place lies beyond the caller's buffers is dropped (fibd_stream_run reports the need)
    int capped;
    int trk;                    // 1: out_xyz is a .trk body: [Int32 npts, npts x 3 Float32 ((xyz+.5)*voxel_size)] per line
    float vs[3];
    // LCM runs (the tile kernel; not with trk): the method-difference flag of a point rides in the sign bit of its x (stream.jl:666) -- the pack
    // strips it and, if flags != NULL, writes it out as one byte per point ([r5] a second pass over the packed points did this: 3.0 of
    // the 17 ms of the 2048^2 benchmark section)
    int lcm;
    uint8_t *out_flags;
    XfmMat xf;                  // the pack kernels' XF variant (fibd_stream_pack_trk_xfm): vox2vox applied before the .trk epilogue
};

struct P3 { float x, y, z; };
typedef float nt4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    return ((unsigned long long)(unsigned)__shfl((int)(v >> 32), src) << 32) | (unsigned)__shfl((int)(unsigned)v, src);
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off) {
    return ((unsigned long long)(unsigned)__shfl_up((int)(v >> 32), off) << 32) | (unsigned)__shfl_up((int)(unsigned)v, off);
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    return ((unsigned long long)(unsigned)__shfl_xor((int)(v >> 32), off) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, off);
}

// The point that scratch slot t (= the loop trip that emitted it) holds, counted from the line's first packed point: forward points
// reversed, backward points behind them (prepend! / append!, stream.jl:652).  nf forward points in slots [0, nf), nb backward points
// from slot bs on.  -1: the slot holds no point of the line (a dropped line has nf = nb = 0).
__device__ __forceinline__ int pk_slot_pos(int t, int nf, int bs, int nb) {
    if (t < nf) return nf - 1 - t;
    if (t >= bs && t - bs < nb) return nf + (t - bs);
    return -1;
}

// A line of a traced job on its way out.  n = 0: not kept (shorter than len_min, stream.jl:769, or no room for it in capped buffers).
struct PkLine {
    int n = 0, nf = 0, nb = 0, bs = 0;
    int64_t p0 = 0;             // first float of its points in out_xyz (a .trk body: its Int32 point count sits at p0 - 1, trk.jl:472)
};
// .. from the trace's counts and the scan's offsets; a kept line's entry in out_npts / out_seed is written here (a .trk body has none)
__device__ __forceinline__ PkLine pk_line_head(const PackArgs &a, int64_t li) {
    PkLine h;
    const int n = a.npts[li];
    if (n < a.len_min) return h;
    const int nfr = a.nfwd[li];
    const Pair e = a.excl[li], bo = a.block_off[li / SCAN_B];
    const int64_t pt = a.out_pt0 + e.pts + bo.pts, l0 = a.out_line0 + e.lines + bo.lines;
    if (a.capped && (l0 >= a.lines_cap || pt + n > a.points_cap)) return h;
    h.n = n; h.nf = nfr & 0x3fffffff; h.nb = n - h.nf; h.bs = h.nf + (nfr >> 30);
    if (a.trk) h.p0 = pt * 3 + l0 + 1;
    else { a.out_npts[l0] = n; a.out_seed[l0] = a.line0 + li; h.p0 = pt * 3; }
    return h;
}

// The .trk epilogue T.((xyz .+ .5) .* voxel_size) in Float64 arithmetic (trk.jl:475-476); XF: str_xform's xfm_apply (trk.jl:345,
// util.jl:401-420) on the point first (fibd_stream_pack_trk_xfm)
template <bool XF>
__device__ __forceinline__ P3 pk_trk_point(const PackArgs &a, P3 v) {
    if (XF) { const float3 r = xfm_point(a.xf, v.x, v.y, v.z); v = P3{r.x, r.y, r.z}; }
    return P3{(float)(((double)v.x + 0.5) * (double)a.vs[0]), (float)(((double)v.y + 0.5) * (double)a.vs[1]), (float)(((double)v.z + 0.5) * (double)a.vs[2])};
}

// One wave per scratch tile (16 lines), four independent waves per workgroup: no workgroup barriers.  A chunk = 16 slots of
// the tile = 3 KiB of contiguous scratch: three 16-byte loads per lane, parked in a wave-private LDS tile (rows padded
// to 52 dwords), then written out line by line: 16 lanes per line, one point each -> a wave instruction emits 4 runs
// of 192 contiguous bytes.  The next chunk's loads fly during the write-out.
constexpr int PK_LINES = SCR_TILE, PK_SLOTS = 16, PK_ROW = 52, PK_WAVES = 4;
static_assert(PK_LINES == 16, "the pack kernel maps 16 lanes to the 16 lines of a tile");
// XF (always with a.trk): pk_trk_point's; XF = false is the kernel fibd_stream_pack / fibd_stream_pack_trk have always run
template <bool XF = false>
__global__ __launch_bounds__(PK_WAVES * 64) void stream_pack_kernel(const PackArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[PK_WAVES][2][PK_SLOTS * PK_ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tix = (int64_t)blockIdx.x * PK_WAVES + wave;   // scratch tile of this wave
    const int64_t line0 = tix * PK_LINES;
    if (line0 >= a.nlines) return;
    PkLine h;                                                   // lanes 0..15: the tile's lines
    if (lane < PK_LINES && line0 + lane < a.nlines) {
        h = pk_line_head(a, line0 + lane);
        if (a.trk && h.n > 0) reinterpret_cast<int32_t *>(a.out_xyz)[h.p0 - 1] = h.n;
    }
    int cnt = h.nb > 0 ? h.bs + h.nb : h.nf;                    // slots of the tile that hold points of kept lines
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) cnt = max(cnt, __shfl_xor(cnt, o));
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    const int nch = (cnt + PK_SLOTS - 1) / PK_SLOTS;
    // write-out mapping: lane = (line group lg, point pt); line tl = lg + 4 j
    const int lg = lane >> 4, pt = lane & 15;
    int wnf[4], wnb[4], wbs[4];
    int64_t wp0[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        wnf[j] = __shfl(h.nf, lg + 4 * j); wnb[j] = __shfl(h.nb, lg + 4 * j); wbs[j] = __shfl(h.bs, lg + 4 * j);
        wp0[j] = (int64_t)shfl_u64((unsigned long long)h.p0, lg + 4 * j);
    }
    const float4 *tbase = reinterpret_cast<const float4 *>(a.scratch + scratch_line_base(line0, a.nslots));
    float4 v[3];
    auto fetch = [&](int c) {                                   // 16 slots of the tile
        const int s0 = c * PK_SLOTS;
        const int live = cnt - s0;                              // live slots of the chunk
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int f = lane + 64 * i;                        // float4 index within the chunk: slot f / 12 (rows of 16 lines: one contiguous 3-KiB run)
            v[i] = (f < live * 12) ? tbase[(int64_t)(s0 + f / 12) * (SCR_SLOT_FLOATS / 4) + f % 12] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if (nch > 0) fetch(0);
    for (int c = 0; c < nch; c++) {
        float *T = tile[wave][c & 1];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int f = lane + 64 * i;
            *reinterpret_cast<float4 *>(T + (f / 12) * PK_ROW + (f % 12) * 4) = v[i];
        }
        __builtin_amdgcn_wave_barrier();
        if (c + 1 < nch) fetch(c + 1);                          // next chunk's loads fly during the write-out
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = pk_slot_pos(c * PK_SLOTS + pt, wnf[j], wbs[j], wnb[j]);
            if (p < 0) continue;
            const float *t = T + pt * PK_ROW + (lg + 4 * j) * 3;
            const P3 q = {t[0], t[1], t[2]};
            *reinterpret_cast<P3 *>(a.out_xyz + wp0[j] + (int64_t)p * 3) = (XF || a.trk) ? pk_trk_point<XF>(a, q) : q;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- the tile packer ----------------------------------------------------------------------------------------------------------------
// The kept lines of a scratch tile occupy ONE contiguous range of the packed output (or of the .trk body), so a workgroup assembles
// that whole range in LDS -- thread = (slot, line) reads its 12-byte point from the contiguous tile (coalesced) and drops it at its
// final position -- and then streams the range out with 16-byte stores aligned to the output address (fill-like: 12-byte stores in
// 192-byte runs reached 2.7 TB/s, aligned 16-byte stores of whole lines reach twice that).  obuf = TL (len_max + 2) points + TL .trk
// count words + 8 floats of alignment slack (launch_pack_n, stream_run_impl).  Three steps with a workgroup barrier between them;
// what surrounds them -- where the lines come from, how many barriers a tile costs -- is the caller's.
template <int TL>
struct PkTile {
    int nf[TL], nb[TL], bs[TL], o[TL];   // per line: forward / backward counts (0 if dropped), first backward slot, offset of its points in obuf
    int cnt, len;                        // slots in use; the range's length in floats (0: no kept line)
    int64_t g0;                          // first float of the range in out_xyz
};
// .. and how many floats out_xyz[g0] lies behind a 16-byte boundary (0..3): the range sits that far into obuf
__device__ __forceinline__ int pk_mis(const float *out_xyz, int64_t g0) { return (int)((reinterpret_cast<uintptr_t>(out_xyz + g0) >> 2) & 3); }

// Step 1, the first wave: lanes < TL bring a line each (lanes >= TL an empty one); a kept line owns out_xyz from hdr floats in front of
// its first point on (1: a .trk count word).  Returns the offset of the line's points in obuf.
template <int TL>
__device__ __forceinline__ int pk_tile_summary(PkTile<TL> &s, const float *out_xyz, int lane, const PkLine &h, int hdr) {
    const int n = h.n, nf = h.nf, nb = h.nb, bs = h.bs;
    const int64_t p0 = h.p0;
    int mf = nb > 0 ? bs + nb : nf;                             // slots of the tile that hold points of kept lines
    int64_t g0 = n > 0 ? p0 - hdr : INT64_MAX, g1 = n > 0 ? p0 + (int64_t)n * 3 : -1;
#pragma unroll
    for (int o = 1; o < TL; o <<= 1) {
        mf = max(mf, __shfl_xor(mf, o));
        const int64_t og0 = (int64_t)shfl_xor_u64((unsigned long long)g0, o), og1 = (int64_t)shfl_xor_u64((unsigned long long)g1, o);
        g0 = og0 < g0 ? og0 : g0; g1 = og1 > g1 ? og1 : g1;
    }
    const int o = n > 0 ? (int)(p0 - g0) + pk_mis(out_xyz, g0) : 0;
    if (lane < TL) { s.nf[lane] = nf; s.nb[lane] = nb; s.bs[lane] = bs; s.o[lane] = o; }
    if (lane == 0) { s.cnt = mf; s.len = g1 >= 0 ? (int)(g1 - g0) : 0; s.g0 = g0; }
    return o;
}

// How point pos of a line whose points start at obuf[o] goes there: emit(obuf, o, pos, v)
__device__ __forceinline__ void pk_put(float *d, P3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
struct PkEmitPlain {
    __device__ __forceinline__ void operator()(float *obuf, int o, int pos, P3 v) const { pk_put(obuf + o + pos * 3, v); }
};
// .. of the stand-alone kernel, by PackArgs: .trk (XF: after xfm_apply) | LCM: |x|, and the flag byte its sign bit carried to fbuf | plain
template <bool XF>
struct PkEmitArgs {
    const PackArgs &a;
    int mis;                    // the range starts at obuf[mis]
    uint8_t *fbuf;              // [points of the range] (a range without count words)
    __device__ __forceinline__ void operator()(float *obuf, int o, int pos, P3 v) const {
        float *d = obuf + o + pos * 3;                          // (a store in every arm: one merged store behind them costs the plain arm moves and hops)
        if (XF || a.trk) pk_put(d, pk_trk_point<XF>(a, v));
        else if (a.lcm) { pk_put(d, P3{fabsf(v.x), v.y, v.z}); fbuf[(o - mis) / 3 + pos] = (uint8_t)(__float_as_uint(v.x) >> 31); }
        else pk_put(d, v);
    }
};

// Step 2, TL x SPC threads: thread = (line, slot within a pass of SPC slots), a pass reads TL x SPC x 12 contiguous bytes of the tile
// (first float: tile); four passes in flight.  plain_loads: diagnostic build only (FIBERS_STREAM_SCRATCH_PLAIN, the stand-alone kernel).
template <int TL, int SPC, class Emit>
__device__ __forceinline__ void pk_gather(const PkTile<TL> &s, const float *tile, float *obuf, int tid, const Emit &emit, bool plain_loads = false) {
    const int nch = (s.cnt + SPC - 1) / SPC;
    const int l = tid % TL, sl = tid / TL;
    const int nf = s.nf[l], nb = s.nb[l], bs = s.bs[l], o = s.o[l];
    const P3 *tbase = reinterpret_cast<const P3 *>(tile) + l + sl * SCR_ROW;
    for (int c0 = 0; c0 < nch; c0 += 4) {
        P3 v[4];
        int pos[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = c0 + i;
            pos[i] = c < nch ? pk_slot_pos(c * SPC + sl, nf, bs, nb) : -1;
            if (pos[i] >= 0) {                                  // read once: non-temporal (the orientation field should keep the Infinity Cache)
                const float *src = reinterpret_cast<const float *>(tbase + (int64_t)c * (SPC * SCR_ROW));
#ifdef FIB_AB_VARIANTS
                if (plain_loads) { f32x3_t q; asm volatile("global_load_dwordx3 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(q) : "v"(src) : "memory"); v[i] = P3{q[0], q[1], q[2]}; }
                else
#endif
                v[i] = P3{__builtin_nontemporal_load(src), __builtin_nontemporal_load(src + 1), __builtin_nontemporal_load(src + 2)};
            } else v[i] = P3{0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (pos[i] >= 0) emit(obuf, o, pos[i], v[i]);
    }
}

// Step 3, NT threads: obuf[mis .. mis + len) -> out_xyz[g0 .. g0 + len): obuf[4k .. 4k+3] lands on a 16-byte aligned address.  Whole
// quads go out non-temporal (written once, read by nobody on the device), the ragged head and tail float by float.
template <int NT>
__device__ __forceinline__ void pk_stream_out(const float *obuf, float *out_xyz, int64_t g0, int len, int tid) {
    const int mis = pk_mis(out_xyz, g0);
    float *gbase = out_xyz + g0 - mis;
    const int nq = (mis + len + 3) >> 2;
    for (int k = tid; k < nq; k += NT) {
        const float4 q = reinterpret_cast<const float4 *>(obuf)[k];
        if (4 * k >= mis && 4 * k + 4 <= mis + len) {
            const nt4_t qn = {q.x, q.y, q.z, q.w};
            __builtin_nontemporal_store(qn, reinterpret_cast<nt4_t *>(gbase + 4 * k));
        } else {
            const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; j++) if (4 * k + j >= mis && 4 * k + j < mis + len) gbase[4 * k + j] = e[j];
        }
    }
}

// Default pack kernel: one workgroup per scratch tile; longer lines than the LDS holds go through stream_pack_kernel above.
template <int TL, int SPC, bool XF = false>   // TL lines per tile (a whole fraction of a scratch row); SPC slots per pass of the workgroup's
                                              // SPC x TL threads; XF: as stream_pack_kernel's
__global__ __launch_bounds__(SPC * TL) void stream_pack_tile_kernel(const PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float obuf[];
    __shared__ PkTile<TL> s;
    const int tid = threadIdx.x;
    const int64_t line0 = (int64_t)blockIdx.x * TL;
    if (tid < 64) {
        PkLine h;
        if (tid < TL && line0 + tid < a.nlines) h = pk_line_head(a, line0 + tid);
        const int o = pk_tile_summary(s, a.out_xyz, tid, h, a.trk);
        if (a.trk && h.n > 0) obuf[o - 1] = __int_as_float(h.n);
    }
    __syncthreads();
    if (s.len == 0) return;
    uint8_t *fbuf = reinterpret_cast<uint8_t *>(obuf + ((size_t)TL * a.stride * 3 + TL + 8));   // [TL * stride] flags of the range's points (LCM runs)
    pk_gather<TL, SPC>(s, a.scratch + scratch_line_base(line0, a.nslots), obuf, tid, PkEmitArgs<XF>{a, pk_mis(a.out_xyz, s.g0), fbuf}, a.scratch_plain != 0);
    __syncthreads();
    if (a.lcm && a.out_flags) {                                 // the range's flags: one byte per point, in the order of the points
        uint8_t *fg = a.out_flags + s.g0 / 3;
        for (int k = tid; k < s.len / 3; k += SPC * TL) fg[k] = fbuf[k];
    }
    pk_stream_out<SPC * TL>(obuf, a.out_xyz, s.g0, s.len, tid);
}

// ---- [r5] FUSED: the block that traced 512 lines packs them (fibd_stream_run; VERDICT r4 item 4) --------------------------------------
// After its trace loop a block knows its kept lines and points; a decoupled look-back over the blocks' totals (one 64-bit granule per
// block: status | kept lines | points -- the data is the flag, agent-scope atomics, no fence; blocks are dispatched in order, so every
// block a block waits for is running or done) gives it its place in the packed output, and it then packs its own 32 scratch tiles
// with the tile packer above.  No scan kernels, no pack launch; the scratch is still written and read back (512 lines x 144
// slots x 12 B = 885 KB per block: it does not stay on chip), but blocks that pack overlap with blocks that still trace.
constexpr unsigned long long FG_PTS_MASK = (1ull << 36) - 1ull, FG_VAL_MASK = (1ull << 62) - 1ull;
typedef __attribute__((address_space(1))) unsigned long long fib_gu64s;
template <int NVEC>
__device__ void fused_pack_block(const TraceArgs &a, int64_t b, int64_t li, bool live, int npts, int nf, int gap) {
    extern __shared__ __attribute__((aligned(16))) float f_obuf[];              // [FT * stride * 3 + slack]: a tile's output range
    __shared__ uint16_t f_nf[FUSED_BLOCK], f_nb[FUSED_BLOCK], f_bs[FUSED_BLOCK];                        // (16 bits: a tile of such lines fits the LDS, so len_max < 2^15)
    __shared__ int64_t f_p0[FUSED_BLOCK];
    constexpr int FB = FUSED_BLOCK, FW = FB / 64;
    __shared__ unsigned long long f_wsum[FW], f_base;
    constexpr int FT = FUSED_TILE, FSL = FB / FT;                               // lines per tile; slots a pass of the 512 threads covers
    __shared__ PkTile<FT> f_tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __builtin_amdgcn_s_setprio(3);                                               // the pack's few memory instructions go ahead of the neighbours' trace loops
    const bool keep = live && npts >= a.len_min;                                 // stream.jl:769
    const unsigned long long v = keep ? ((1ull << 36) | (unsigned long long)npts) : 0ull;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = shfl_up_u64(inc, off); if (lane >= off) inc += o; }
    if (lane == 63) f_wsum[wave] = inc;
    __syncthreads();
    unsigned long long wbase = 0ull;
    for (int w = 0; w < wave; w++) wbase += f_wsum[w];
    unsigned long long agg = 0ull;
    for (int w = 0; w < FW; w++) agg += f_wsum[w];
    if (wave == 0) {
        if (lane == 0)
            __hip_atomic_store((fib_gu64s *)(a.fstate + b), ((b == 0 ? 2ull : 1ull) << 62) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long excl = 0ull;
        int64_t j0 = b - 1;                                                     // lane l looks at block j0 - l
        while (j0 >= 0) {
            const int64_t j = j0 - lane;
            unsigned long long g = 2ull << 62;                                   // (before block 0: an inclusive prefix of nothing)
            if (j >= 0) {
                for (;;) {
                    g = __hip_atomic_load((fib_gu64s *)(a.fstate + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((g >> 62) != 0ull) break;
                    __builtin_amdgcn_s_sleep(4);                                 // (a predecessor still tracing: do not take its issue slots)
                }
            }
            const unsigned long long pre = __ballot((g >> 62) == 2ull);          // nearest predecessor that knows its inclusive prefix
            const int first = pre ? __builtin_ctzll(pre) : 63;
            unsigned long long c = lane <= first ? (g & FG_VAL_MASK) : 0ull;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += shfl_xor_u64(c, off);
            excl += c;
            if (pre) break;
            j0 -= 64;
        }
        if (lane == 0) {
            if (b > 0) __hip_atomic_store((fib_gu64s *)(a.fstate + b), (2ull << 62) | (excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            f_base = excl;
            if (b == (int64_t)gridDim.x - 1) {
                const unsigned long long tot = excl + agg;
                a.ftotal->pts = (int64_t)(tot & FG_PTS_MASK); a.ftotal->lines = (int64_t)(tot >> 36);
                if (a.fcounts) { a.fcounts[0] = (int64_t)(tot >> 36); a.fcounts[1] = (int64_t)(tot & FG_PTS_MASK); }
            }
        }
    }
    __syncthreads();
    {
        const unsigned long long ex = f_base + wbase + inc - v;                  // kept lines / points before this line
        const int64_t l0 = (int64_t)(ex >> 36), pt = (int64_t)(ex & FG_PTS_MASK);
        int mnf = 0, mnb = 0, mbs = 0;
        int64_t p0 = 0;
        if (keep && !(l0 >= a.lines_cap || pt + npts > a.points_cap)) {          // (no room: dropped; the totals say what was needed)
            a.out_npts[l0] = npts; a.out_seed[l0] = a.line0 + li;
            mnf = nf; mnb = npts - nf; mbs = nf + gap; p0 = pt * 3;
        }
        f_nf[tid] = (uint16_t)mnf; f_nb[tid] = (uint16_t)mnb; f_bs[tid] = (uint16_t)mbs; f_p0[tid] = p0;
    }
    __syncthreads();
    // per tile: [one wave: the tile's summary] barrier [gather the tile's points into its output range in LDS] barrier [stream the range out]
    // barrier.  (Preparing the next tile's summary beside the stream-out -- two barriers per tile -- measured SLOWER: C4 1.18 against 1.05 ms.)
    for (int t = 0; t < FB / FT; t++) {
        if (tid < 64) {
            PkLine h;
            if (tid < FT) { h.nf = f_nf[t * FT + tid]; h.nb = f_nb[t * FT + tid]; h.bs = f_bs[t * FT + tid]; h.n = h.nf + h.nb; h.p0 = f_p0[t * FT + tid]; }
            pk_tile_summary(f_tile, a.out_xyz, tid, h, 0);
        }
        __syncthreads();
        const int len = f_tile.len;
        if (len > 0)
            pk_gather<FT, FSL>(f_tile, a.scratch + scratch_line_base((b * (FB / FT) + t) * FT, a.nslots), f_obuf, tid, PkEmitPlain{});
        __syncthreads();
        if (len > 0) pk_stream_out<FB>(f_obuf, a.out_xyz, f_tile.g0, len, tid);
        __syncthreads();
    }
}
