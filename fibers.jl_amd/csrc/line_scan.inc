// line_scan.inc -- the exclusive scan of N int64 sums per line, with a verdict on the input, that every kernel file working on packed
// lines needs (tm_lines.inc for tractmap.hip / tractsel.hip / bundle.hip, probtrack.hip; textually included inside their anonymous
// namespace).  Three launches: ls_block (the sums of LS_TILE lines), ls_totals (ONE workgroup: the exclusive scan of the block totals
// in place, and the verdict), ls_apply (the exclusive value of every line).  What is summed and where it goes is the Item, a small
// trivially copyable struct passed by value:
//   static constexpr int N                                              the number of components
//   LsVec<N> load(int64_t line, bool &bad) const                        a line's contribution; bad |= ... marks an input the scan refuses
//   void store(int64_t line, const LsVec<N> &run, const LsVec<N> &mine) const   the exclusive value of a line (mine: its contribution)
//   void verdict(const LsVec<N> &grand, bool bad) const                 lane 0 of ls_totals: the grand totals and whether anything was refused
//   bool go() const                                                     false: ls_apply returns at once
// A refusal travels as a NEGATIVE COMPONENT 0 (contributions are not negative): of a wave's partial sum, of a block's total in memory,
// of a lane's partial sum in ls_totals.  The offsets of a refused input are never read, so ls_totals leaves the totals unscanned.

constexpr int LS_BLOCK = 256;
constexpr int LS_ITEMS = 4;                                    // lines per lane
constexpr int LS_TILE = LS_BLOCK * LS_ITEMS;

template <int N>
struct LsVec {
    int64_t v[N];
};
template <int N>
__device__ __forceinline__ LsVec<N> ls_add(LsVec<N> a, const LsVec<N> &b) { for (int i = 0; i < N; i++) a.v[i] += b.v[i]; return a; }
template <int N>
__device__ __forceinline__ LsVec<N> ls_sub(LsVec<N> a, const LsVec<N> &b) { for (int i = 0; i < N; i++) a.v[i] -= b.v[i]; return a; }
template <int N>
__device__ __forceinline__ LsVec<N> ls_xor(LsVec<N> a, int d) { for (int i = 0; i < N; i++) a.v[i] = __shfl_xor(a.v[i], d); return a; }
template <int N>
__device__ __forceinline__ LsVec<N> ls_up(LsVec<N> a, int d) { for (int i = 0; i < N; i++) a.v[i] = __shfl_up(a.v[i], d); return a; }

// block b: the sums of its LS_TILE lines
template <class Item>
__global__ __launch_bounds__(LS_BLOCK) void ls_block(const Item it, int64_t nlines, LsVec<Item::N> *totals) {
    using V = LsVec<Item::N>;
    __shared__ V s_sum[LS_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * LS_TILE + (int64_t)threadIdx.x * LS_ITEMS;
    V sum{};
    bool bad = false;
    for (int j = 0; j < LS_ITEMS; j++)
        if (base + j < nlines) sum = ls_add(sum, it.load(base + j, bad));
    for (int d = 32; d >= 1; d >>= 1) sum = ls_add(sum, ls_xor(sum, d));
    if (__any(bad)) sum.v[0] = -1;
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        V t{};
        bad = false;
        for (int w = 0; w < LS_BLOCK / 64; w++) { bad |= s_sum[w].v[0] < 0; t = ls_add(t, s_sum[w]); }
        if (bad) t.v[0] = -1;
        totals[blockIdx.x] = t;
    }
}

// one workgroup: lane t takes the blocks [t * per, (t + 1) * per); totals -> their exclusive scan (in place), and the verdict
template <class Item>
__global__ __launch_bounds__(LS_BLOCK) void ls_totals(const Item it, LsVec<Item::N> *totals, int64_t nblocks) {
    using V = LsVec<Item::N>;
    __shared__ V s_part[LS_BLOCK];
    const int64_t per = (nblocks + LS_BLOCK - 1) / LS_BLOCK, b0 = threadIdx.x * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    V sum{};
    bool bad = false;
    for (int64_t b = b0; b < b1; b++) { const V t = totals[b]; bad |= t.v[0] < 0; sum = ls_add(sum, t); }
    if (bad) sum.v[0] = -1;
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        constexpr int UNROLL = Item::N == 1 ? 16 : 8;           // a chain of LDS round trips: at least eight 16-byte loads in flight per trip
        V run{};
        bad = false;
#pragma unroll UNROLL
        for (int t = 0; t < LS_BLOCK; t++) { const V v = s_part[t]; bad |= v.v[0] < 0; s_part[t] = run; run = ls_add(run, v); }
        it.verdict(run, bad);
        if (bad) s_part[0].v[0] = -1;                           // (lane 0 starts at 0: its slot tells the other lanes)
    }
    __syncthreads();
    if (s_part[0].v[0] < 0) return;
    V run = s_part[threadIdx.x];
    for (int64_t b = b0; b < b1; b++) { const V t = totals[b]; totals[b] = run; run = ls_add(run, t); }
}

template <class Item>
__global__ __launch_bounds__(LS_BLOCK) void ls_apply(const Item it, int64_t nlines, const LsVec<Item::N> *totals) {
    using V = LsVec<Item::N>;
    __shared__ V s_sum[LS_BLOCK / 64];
    if (!it.go()) return;
    const int64_t base = (int64_t)blockIdx.x * LS_TILE + (int64_t)threadIdx.x * LS_ITEMS;
    V c[LS_ITEMS];
    V mine{};
    bool bad = false;                                           // (judged by ls_block)
    for (int j = 0; j < LS_ITEMS; j++) { c[j] = base + j < nlines ? it.load(base + j, bad) : V{}; mine = ls_add(mine, c[j]); }
    V inc = mine;                                               // inclusive scan over the wave
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const V o = ls_up(inc, d); if (lane >= d) inc = ls_add(inc, o); }
    if (lane == 63) s_sum[threadIdx.x >> 6] = inc;
    __syncthreads();
    V run = totals[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) run = ls_add(run, s_sum[w]);
    run = ls_add(run, ls_sub(inc, mine));
    for (int j = 0; j < LS_ITEMS; j++) if (base + j < nlines) { it.store(base + j, run, c[j]); run = ls_add(run, c[j]); }
}

// the block totals a scan of nlines lines needs room for (at least one, so that the area is never empty)
int64_t ls_total_slots(int64_t nlines) { return std::max<int64_t>(1, fib::cdiv(nlines, LS_TILE)); }

// the three launches, enqueued on st; the caller asks hipGetLastError
template <class Item>
void ls_scan(const Item &it, int64_t nlines, LsVec<Item::N> *totals, hipStream_t st) {
    const int64_t nblocks = fib::cdiv(nlines, LS_TILE);
    if (nblocks > 0) hipLaunchKernelGGL(ls_block<Item>, dim3((unsigned)nblocks), dim3(LS_BLOCK), 0, st, it, nlines, totals);
    hipLaunchKernelGGL(ls_totals<Item>, dim3(1), dim3(LS_BLOCK), 0, st, it, totals, nblocks);
    if (nblocks > 0) hipLaunchKernelGGL(ls_apply<Item>, dim3((unsigned)nblocks), dim3(LS_BLOCK), 0, st, it, nlines, totals);
}

// a work area of `need` bytes; size_entry names the *_work_size entry that says so
int ls_check_work(const void *work, size_t work_bytes, size_t need, const char *size_entry) {
    FIB_CHECK(work && (reinterpret_cast<uintptr_t>(work) & 7) == 0, FIB_ERR_INVALID, "work must be an 8-byte aligned device buffer");
    FIB_CHECK(work_bytes >= need, FIB_ERR_INVALID, "work holds %zu bytes, %s asks for %zu", work_bytes, size_entry, need);
    return FIB_OK;
}
