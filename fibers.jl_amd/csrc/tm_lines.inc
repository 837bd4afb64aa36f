// tm_lines.inc -- what every kernel file that reads PACKED LINES shares (tractmap.hip, tractsel.hip; textually included inside
// their anonymous namespace): the voxel of a point, the exclusive int64 scan of npts with its verdict on the input, the work area.
// The definitions are the "Tract maps" section of include/fibers_hip.h.

constexpr int TM_BLOCK = 256;
constexpr int TM_SCAN_ITEMS = 4;                               // counts per lane of the scan
constexpr int TM_SCAN_TILE = TM_BLOCK * TM_SCAN_ITEMS;

// header of the work area (then the int64 offsets [nlines + 1], then the scan's block totals)
struct TmHead {
    int32_t ok;                                                // 1: npts is valid and sums to npoints
    int32_t pad;
};
constexpr size_t TM_HEAD_BYTES = 16;

// rint (ties to even, v_rndne_f32), the test on the float value: NaN fails every comparison, +-Inf and +-1e30 the range
__device__ __forceinline__ int64_t tm_voxel(float x, float y, float z, int nx, int ny, int nz) {
    const float vx = rintf(x), vy = rintf(y), vz = rintf(z);
    const bool in = vx >= 1.0f && vx <= (float)nx && vy >= 1.0f && vy <= (float)ny && vz >= 1.0f && vz <= (float)nz;
    if (!in) return -1;
    return (int64_t)((int)vx - 1) + (int64_t)nx * (((int)vy - 1) + (int64_t)ny * ((int)vz - 1));
}
__device__ __forceinline__ int64_t tm_voxel_at(const float *xyz, int64_t p, int nx, int ny, int nz) {
    return tm_voxel(xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], nx, ny, nz);
}

// ---- offsets ---------------------------------------------------------------------------------------------------------------------
// block b: the sum of its TM_SCAN_TILE counts (a negative count makes the total -1 - what the totals kernel refuses)
__global__ __launch_bounds__(TM_BLOCK) void tm_scan_block(const int32_t *npts, int64_t nlines, int64_t *totals) {
    __shared__ int64_t s_sum[TM_BLOCK / 64];
    __shared__ int s_neg;
    if (threadIdx.x == 0) s_neg = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * TM_SCAN_TILE + (int64_t)threadIdx.x * TM_SCAN_ITEMS;
    int64_t sum = 0;
    bool neg = false;
    for (int j = 0; j < TM_SCAN_ITEMS; j++)
        if (base + j < nlines) { const int32_t c = npts[base + j]; neg |= c < 0; sum += c; }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    if (neg) s_neg = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int w = 0; w < TM_BLOCK / 64; w++) t += s_sum[w];
        totals[blockIdx.x] = s_neg ? -1 : t;
    }
}

// one workgroup: totals -> their exclusive scan (in place), the verdict, off[nlines] and the start value of n_outside
__global__ __launch_bounds__(TM_BLOCK) void tm_scan_totals(int64_t *totals, int64_t nblocks, int64_t nlines, int64_t npoints, TmHead *head,
                                                           int64_t *off, int64_t *n_outside) {
    __shared__ int64_t s_part[TM_BLOCK];
    __shared__ int s_neg;
    if (threadIdx.x == 0) s_neg = 0;
    __syncthreads();
    const int64_t per = (nblocks + TM_BLOCK - 1) / TM_BLOCK, b0 = threadIdx.x * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    int64_t sum = 0;
    bool neg = false;
    for (int64_t b = b0; b < b1; b++) { const int64_t t = totals[b]; neg |= t < 0; sum += t; }
    s_part[threadIdx.x] = sum;
    if (neg) s_neg = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < TM_BLOCK; t++) { const int64_t v = s_part[t]; s_part[t] = run; run += v; }
        const bool ok = !s_neg && run == npoints;
        head->ok = ok ? 1 : 0;
        off[nlines] = ok ? run : 0;
        if (n_outside) *n_outside = ok ? 0 : -1;
    }
    __syncthreads();
    if (s_neg) return;                                          // (the offsets of a refused input are never read)
    int64_t run = s_part[threadIdx.x];
    for (int64_t b = b0; b < b1; b++) { const int64_t t = totals[b]; totals[b] = run; run += t; }
}

__global__ __launch_bounds__(TM_BLOCK) void tm_scan_apply(const int32_t *npts, int64_t nlines, const int64_t *totals, const TmHead *head,
                                                          int64_t *off) {
    __shared__ int64_t s_sum[TM_BLOCK / 64];
    if (!head->ok) return;
    const int64_t base = (int64_t)blockIdx.x * TM_SCAN_TILE + (int64_t)threadIdx.x * TM_SCAN_ITEMS;
    int32_t c[TM_SCAN_ITEMS];
    int64_t mine = 0;
    for (int j = 0; j < TM_SCAN_ITEMS; j++) { c[j] = base + j < nlines ? npts[base + j] : 0; mine += c[j]; }
    int64_t inc = mine;                                         // inclusive scan over the wave
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const int64_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    if (lane == 63) s_sum[threadIdx.x >> 6] = inc;
    __syncthreads();
    int64_t run = totals[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) run += s_sum[w];
    run += inc - mine;
    for (int j = 0; j < TM_SCAN_ITEMS; j++) if (base + j < nlines) { off[base + j] = run; run += c[j]; }
}

struct TmWork {
    TmHead *head;
    int64_t *off, *totals;
    int64_t nblocks;
};

size_t tm_work_bytes(int64_t nlines) {
    return TM_HEAD_BYTES + sizeof(int64_t) * (size_t)(nlines + 1) + sizeof(int64_t) * (size_t)std::max<int64_t>(1, fib::cdiv(nlines, TM_SCAN_TILE));
}

// the offset scan and the verdict, enqueued on st
int tm_offsets(const int32_t *npts, int64_t nlines, int64_t npoints, void *work, size_t work_bytes, int64_t *n_outside, hipStream_t st, TmWork &w) {
    FIB_CHECK(work && (reinterpret_cast<uintptr_t>(work) & 7) == 0, FIB_ERR_INVALID, "work must be an 8-byte aligned device buffer");
    FIB_CHECK(work_bytes >= tm_work_bytes(nlines), FIB_ERR_INVALID, "work holds %zu bytes, fibd_str_work_size asks for %zu", work_bytes, tm_work_bytes(nlines));
    w.head = reinterpret_cast<TmHead *>(work);
    w.off = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(work) + TM_HEAD_BYTES);
    w.totals = w.off + nlines + 1;
    w.nblocks = fib::cdiv(nlines, TM_SCAN_TILE);
    if (w.nblocks > 0) hipLaunchKernelGGL(tm_scan_block, dim3((unsigned)w.nblocks), dim3(TM_BLOCK), 0, st, npts, nlines, w.totals);
    hipLaunchKernelGGL(tm_scan_totals, dim3(1), dim3(TM_BLOCK), 0, st, w.totals, w.nblocks, nlines, npoints, w.head, w.off, n_outside);
    if (w.nblocks > 0) hipLaunchKernelGGL(tm_scan_apply, dim3((unsigned)w.nblocks), dim3(TM_BLOCK), 0, st, npts, nlines, w.totals, w.head, w.off);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

int tm_check_lines(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints) {
    FIB_CHECK(nlines >= 0 && npoints >= 0, FIB_ERR_INVALID, "nlines and npoints must not be negative");
    FIB_CHECK(nlines < ((int64_t)1 << 31) * (TM_SCAN_TILE / 2), FIB_ERR_UNSUPPORTED, "too many lines");
    FIB_CHECK(nlines == 0 || npts, FIB_ERR_INVALID, "NULL npts");
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    FIB_CHECK((reinterpret_cast<uintptr_t>(xyz) & 3) == 0, FIB_ERR_INVALID, "points must be 4-byte aligned");
    return FIB_OK;
}
