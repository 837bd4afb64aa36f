// tm_lines.inc -- what every kernel file that reads PACKED LINES shares (tractmap.hip, tractsel.hip, bundle.hip; textually included
// inside their anonymous namespace): the voxel of a point, the exclusive int64 scan of npts with its verdict on the input (an Item of
// line_scan.inc), the work area.  The definitions are the "Tract maps" section of include/fibers_hip.h.

#include "line_scan.inc"                                       // LS_BLOCK, LS_TILE, LsVec, ls_scan, ls_check_work

constexpr int TM_BLOCK = LS_BLOCK;

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
// the scan of npts: off[l] = the first point of line l.  Refused: a negative count, or a sum that is not npoints; the verdict goes to
// head->ok, off[nlines] and the start value of n_outside (0, or -1 for a refused input), and nothing is written to off[0 .. nlines).
struct TmItem {
    static constexpr int N = 1;
    const int32_t *npts;
    int64_t nlines, npoints;
    TmHead *head;
    int64_t *off, *n_outside;
    __device__ LsVec<1> load(int64_t l, bool &bad) const { const int32_t c = npts[l]; bad |= c < 0; return {c}; }
    __device__ void store(int64_t l, const LsVec<1> &run, const LsVec<1> &) const { off[l] = run.v[0]; }
    __device__ void verdict(const LsVec<1> &grand, bool bad) const {
        const bool ok = !bad && grand.v[0] == npoints;
        head->ok = ok ? 1 : 0;
        off[nlines] = ok ? grand.v[0] : 0;
        if (n_outside) *n_outside = ok ? 0 : -1;
    }
    __device__ bool go() const { return head->ok != 0; }
};

struct TmWork {
    TmHead *head;
    int64_t *off;
};

size_t tm_work_bytes(int64_t nlines) { return TM_HEAD_BYTES + sizeof(int64_t) * (size_t)(nlines + 1) + sizeof(int64_t) * (size_t)ls_total_slots(nlines); }

// the offset scan and the verdict, enqueued on st
int tm_offsets(const int32_t *npts, int64_t nlines, int64_t npoints, void *work, size_t work_bytes, int64_t *n_outside, hipStream_t st, TmWork &w) {
    FIB_RC(ls_check_work(work, work_bytes, tm_work_bytes(nlines), "fibd_str_work_size"));
    w.head = reinterpret_cast<TmHead *>(work);
    w.off = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(work) + TM_HEAD_BYTES);
    ls_scan(TmItem{npts, nlines, npoints, w.head, w.off, n_outside}, nlines, reinterpret_cast<LsVec<1> *>(w.off + nlines + 1), st);
    FIB_HIP(hipGetLastError());
    return FIB_OK;
}

int tm_check_lines(const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints) {
    FIB_CHECK(nlines >= 0 && npoints >= 0, FIB_ERR_INVALID, "nlines and npoints must not be negative");
    FIB_CHECK(nlines < ((int64_t)1 << 31) * (LS_TILE / 2), FIB_ERR_UNSUPPORTED, "too many lines");
    FIB_CHECK(nlines == 0 || npts, FIB_ERR_INVALID, "NULL npts");
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    FIB_CHECK((reinterpret_cast<uintptr_t>(xyz) & 3) == 0, FIB_ERR_INVALID, "points must be 4-byte aligned");
    return FIB_OK;
}
