// api.hip — host-buffer ("drop-in") entry points: the functions the Julia wrapper ccalls in place of the bodies of
// dti_fit / adc_fit / gqi_rec / dsi_rec / stream.  Caller-owned host arrays in, caller-owned host arrays out.
//
// The reference threads its volume loops over z-slices (dti.jl:258, gqi.jl:132, dsi.jl:197) and its seed list over
// contiguous chunks (stream.jl:757-761).  Here the same decomposition feeds GPUs:
//   * a device set (fib_init; default: device 0) — the voxel range is cut into contiguous slabs, one per device, each
//     driven by its own host thread; seeds shard round-robin;
//   * per device a three-stage pipeline over voxel chunks: gather rows of the planar host arrays into a pinned ring
//     (threaded memcpy) -> H2D on one stream || the device-resident path (fibd_*) on a second || D2H on a third ->
//     scatter rows back.  PCIe runs in both directions at once; the kernels hide completely behind the link;
//   * the only exchange step of the fits, odfmax = maximum(mean(odf, dims=4)) (gqi.jl:164, dsi.jl:263), is one float per
//     chunk: reduced on the host, then qa ./= odfmax runs on every device before the qa volumes are copied out;
//   * plans (the reference's work structs) are cached per device, keyed by the tables they were built from.
// The voxel fits share their argument handling (fit_call) and their per-worker body (fit_run); what a form keeps is its own checks, its
// rows, its plan and the layout of a chunk on the device.
// Every other host form but fib_xfm_apply runs on one device with blocking copies, under a DevLease (the worker, its lock, the device).
// The tractogram forms (fib_str_*) take a TmLease, which adds the worker's buffer set; the five that take lines of any length walk them with
// tm_walk_lines, in the chunks that fibh::next_line_chunk cuts (host_tier.h), and keep a body per chunk.
// fib_str_weights cuts the same chunks with a size of its own (FIBERS_FIXEL_POINTS) and keeps the fixel ids of every chunk resident.
// The volume, warp, structure-tensor, RUMBA and peak-finder forms keep nothing between calls: their buffers are local.  The two frame
// resamplers share frame_checks / frame_chunks, the peak finders find_peaks_host; the sizes taken from the free memory are host_tier.h's.
// The tracking forms (fib_stream, fib_stream_lcm, fib_prob_stream) return through one owner, fibh::TractArrays, and one download path,
// d2h_pipelined on the worker's output ring; their seed list, the seed share of a device set and the merge of its shards are host_tier.h's.
#include <sched.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "common.h"
#include "host_tier.h"

namespace {

using fibh::bind_this_thread; using fibh::chunk_count; using fibh::CopyPool; using fibh::dtype_size; using fibh::LiveMap; using fibh::NBUF; using fibh::Rows;
using fibh::slab;

#define RC(x) FIB_RC(x)

// (mask element types, the copy pool, live maps, the chunk schedule and the chunk pipeline itself: host_tier.h -- pure host code, also built
// under the sanitizers by tests/test_host_sanitizers.py)
int mask_convert_range(const void *m, int dtype, int64_t i0, int64_t n, bool positive, uint8_t *out) {
    if (!fibh::mask_convert_range(m, dtype, i0, n, positive, out)) return fib::fail(FIB_ERR_INVALID, "unknown mask dtype %d", dtype);
    return FIB_OK;
}
int mask_convert(const void *m, int dtype, int64_t n, bool positive, std::vector<uint8_t> &out) {
    out.resize((size_t)n);
    return mask_convert_range(m, dtype, 0, n, positive, out.data());
}

int h2d(void *dst, const void *src, size_t bytes) {
    FIB_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return FIB_OK;
}
int d2h(void *dst, const void *src, size_t bytes) {
    FIB_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return FIB_OK;
}

// ---- NUMA: the host CPUs next to a device ---------------------------------------------------------------------------------------
// [r5] The pinned ring a device's DMA engines read and write, and the threads that fill and drain it, belong on the NUMA node the device
// hangs off (a two-socket box: the driver's run of fib_gqi_rec took 122 ms where a run whose pages happened to sit on the device's
// node took 90).  The node's CPUs come from sysfs (local_cpulist of the device's PCI function), intersected with the CPUs this process
// may use; an empty list (no sysfs, one node, a container without the file) leaves everything where the scheduler puts it.
std::vector<int> device_local_cpus(int device) {
    std::vector<int> cpus;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return cpus;
    for (char *c = bdf; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/local_cpulist";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return cpus;
    char line[4096] = {0};
    const bool ok = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!ok) return cpus;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return cpus;
    for (const char *q = line; *q;) {                        // "0-63,128-191"
        char *e = nullptr;
        const long a = strtol(q, &e, 10);
        if (e == q) break;
        long b = a;
        q = e;
        if (*q == '-') { b = strtol(q + 1, &e, 10); q = e; }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) if (CPU_ISSET((int)c, &allowed)) cpus.push_back((int)c);
        if (*q == ',') q++; else break;
    }
    return cpus;
}
// a host-side phase, into the profile table while fib_profile_enable(1) is active
struct HostTimer {
    const char *name; std::chrono::steady_clock::time_point t0;
    explicit HostTimer(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() { if (fib::profiling_on()) fib::profile_add_ms(name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};

// ---- per-device state of the host tier -----------------------------------------------------------------------------------
struct PinBuf {                                          // grow-only pinned host buffer
    char *p = nullptr; size_t n = 0;
    // cpus: the allocation (and the first touch of its pages) happens on a thread bound to these CPUs -- the device's NUMA node
    int ensure(size_t bytes, int device, const std::vector<int> &cpus) {
        if (bytes <= n && p) return FIB_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipSuccess;
        auto body = [&] {
            bind_this_thread(cpus);
            (void)hipSetDevice(device);
            e = hipHostMalloc((void **)&p, bytes ? bytes : 1, hipHostMallocDefault);
            if (e == hipSuccess) for (size_t o = 0; o < bytes; o += 4096) p[o] = 0;    // (first touch, should the driver have left any page untouched)
        };
        if (cpus.empty()) body(); else { std::thread t(body); t.join(); }
        if (e != hipSuccess) { p = nullptr; return fib::fail(FIB_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); }
        n = bytes;
        return FIB_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    ~PinBuf() { release(); }
};

// a cached plan of any type: `destroy` releases it and tells the plan types apart (plan cache, below)
struct CachedPlan { std::string key; void *plan = nullptr; void (*destroy)(void *) = nullptr; uint64_t stamp = 0; };

struct DevState {
    int device = 0;
    std::mutex mu;                                       // one host-tier call at a time per entry of the device set
    bool ready = false;
    hipStream_t s_in = nullptr, s_cmp = nullptr, s_out = nullptr;
    hipEvent_t e_in[NBUF] = {}, e_cmp[NBUF] = {}, e_out[NBUF] = {};
    PinBuf pin_in[NBUF], pin_out[NBUF];
    fib::DevBuf<char> dev_in[NBUF], dev_out[NBUF];
    std::vector<int> cpus;                               // the host CPUs on the device's NUMA node (empty: unknown / not bound)
    std::unique_ptr<CopyPool> pool, pool_out;            // row copies into the ring (gather) | out of it (scatter): the two stages run side by side
    std::vector<CachedPlan> plans;
    uint64_t clock = 0;
    fib_stream_ws *ws = nullptr;
    // device buffers of fib_stream, kept between calls (grow-only, like the ring and the tracer's workspace): a hipMalloc / hipFree pair
    // per 1.5-GB result costs more than the tracking itself
    struct StreamBufs {
        fib::DevBuf<float> vec, f, fa, field, sub, lcms, xyz;
        fib::DevBuf<uint8_t> mask, mout, flags;
        fib::DevBuf<int64_t> seeds, sidx;
        fib::DevBuf<int32_t> npts;
    };
    // device buffers of fib_str_density / fib_str_sample / fib_str_stats (grow-only): one chunk of points and what belongs to it, the
    // resident volume (density map or sampled volume), the offset scratch
    struct TractMapBufs {
        fib::DevBuf<float> xyz, vol, scal, props;
        fib::DevBuf<int32_t> npts;
        fib::DevBuf<uint32_t> dens;
        fib::DevBuf<char> work;
        fib::DevBuf<int64_t> nout;
        // fib_str_select / fib_str_connectome: the ROIs and their bit volume, keep and hits of a chunk; labels, remap, C, W, assign
        fib::DevBuf<uint8_t> rois, keep;
        fib::DevBuf<uint32_t> roibits, hits, cmat;
        fib::DevBuf<int32_t> labels, remap, assign;
        fib::DevBuf<double> wmat;
        // fib_str_resample / fib_str_assign / fib_str_centroids: the equal-length lines of a chunk, the models, label / dist / flip of a
        // chunk, all distances, sums and counts
        fib::DevBuf<float> lines, models, dist, dall;
        fib::DevBuf<int32_t> label;
        fib::DevBuf<uint8_t> flip;
        fib::DevBuf<double> sums;
        fib::DevBuf<uint32_t> bcnt;
        // fib_str_weights: the peak field, every line's count, and what stays resident for the iterations: ids, Aq, TDq, N_s, q
        fib::DevBuf<float> fx_vec, fx_f, fx_w, fx_td;
        fib::DevBuf<uint8_t> fx_mask;
        fib::DevBuf<int32_t> fx_npts, fx_ids;
        fib::DevBuf<uint64_t> fx_aq, fx_tdq, fx_nline;
        fib::DevBuf<uint32_t> fx_q;
        fib::DevBuf<double> fx_cost;
        fib::DevBuf<int64_t> fx_state;
    };
    // each set is created by its first user (stream_worker, TmLease) and released as a whole by trim()
    std::unique_ptr<StreamBufs> sb;
    std::unique_ptr<TractMapBufs> tm;

    int init(int nthreads) {
        if (ready) return FIB_OK;
        FIB_HIP(hipSetDevice(device));
        FIB_HIP(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        FIB_HIP(hipStreamCreateWithFlags(&s_cmp, hipStreamNonBlocking));
        FIB_HIP(hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        for (int b = 0; b < NBUF; b++) {
            FIB_HIP(hipEventCreateWithFlags(&e_in[b], hipEventDisableTiming));
            FIB_HIP(hipEventCreateWithFlags(&e_cmp[b], hipEventDisableTiming));
            FIB_HIP(hipEventCreateWithFlags(&e_out[b], hipEventDisableTiming));
        }
        { const char *e = fib::ab_env("FIBERS_HOST_NUMA"); if (!(e && e[0] == '0')) cpus = device_local_cpus(device); }
        pool.reset(new CopyPool(nthreads, cpus));
        pool_out.reset(new CopyPool(nthreads, cpus));
        ready = true;
        return FIB_OK;
    }
    // fib_trim: everything this worker keeps BETWEEN calls to make the next call cheap -- the pinned ring and its device mirror, fib_stream's
    // device buffers (C4: 1.5 GB of points), the tracer's workspace -- goes back to the driver; plans stay (they are small and costly to
    // rebuild).  The caller holds `mu`: no call is in flight on this worker.
    void trim() {
        if (!ready) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(s_in); (void)hipStreamSynchronize(s_cmp); (void)hipStreamSynchronize(s_out);
        for (int b = 0; b < NBUF; b++) { pin_in[b].release(); pin_out[b].release(); dev_in[b].release(); dev_out[b].release(); }
        sb.reset();
        tm.reset();
        if (ws) { fibd_stream_ws_destroy(ws); ws = nullptr; }
    }
    void drop_plans() {
        for (auto &c : plans) c.destroy(c.plan);
        plans.clear();
    }
    ~DevState() {
        if (!ready) return;
        (void)hipSetDevice(device);
        drop_plans();
        if (ws) fibd_stream_ws_destroy(ws);
        for (int b = 0; b < NBUF; b++) { (void)hipEventDestroy(e_in[b]); (void)hipEventDestroy(e_cmp[b]); (void)hipEventDestroy(e_out[b]); }
        (void)hipStreamDestroy(s_in); (void)hipStreamDestroy(s_cmp); (void)hipStreamDestroy(s_out);
    }
};

// The device set of the host tier (fib_init).  Entry i is an independent worker: the same device may appear twice (two
// concurrent pipelines on one GPU; used by the tests on a 1-GPU box).
// Workers are handed out as shared pointers: a call that fib_init / fib_shutdown overtakes keeps its workers alive until it returns.
using Worker = std::shared_ptr<DevState>;
struct HostCtx {
    std::mutex mu;
    std::vector<Worker> devs;                            // the set for device == FIB_DEVICE_ALL
    std::vector<Worker> single;                          // workers for calls that name one device
};
// Never destroyed: at process exit the HIP runtime's own exit handlers may already have run, and destroying streams, events and
// device buffers then crashes or hangs.  Only fib_shutdown releases resources.
HostCtx &ctx() { static HostCtx *c = new HostCtx(); return *c; }

int copy_threads(int nworkers) {
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 8;
    if (const char *e = fib::env("FIBERS_COPY_THREADS")) { const int t = atoi(e); if (t >= 1) return t; }
    int t = (int)hw / (2 * (nworkers > 0 ? nworkers : 1));
    // 8-16 threads reach the host's copy bandwidth on whole rows (tools/probes/host_probe.hip); the runs of a masked volume are a few hundred
    // bytes each; [r6] 32 or 64 threads per stage were measured and are WORSE, dense and masked (profiles/r06/host_tier_threads.txt)
    return t < 2 ? 2 : (t > 16 ? 16 : t);
}

// workers of a call: the fib_init set for FIB_DEVICE_ALL, else the (lazily created) worker of that device
int workers_for(int device, std::vector<Worker> &out) {
    HostCtx &c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    if (device == FIB_DEVICE_ALL) {
        if (c.devs.empty()) {                            // no fib_init: every visible device
            const int n = fib_device_count();
            if (n <= 0) return fib::fail(FIB_ERR_NO_DEVICE, "no HIP device is available and this back end has no CPU fallback");
            for (int d = 0; d < n; d++) { c.devs.emplace_back(new DevState()); c.devs.back()->device = d; }
        }
        for (auto &d : c.devs) out.push_back(d);
        return FIB_OK;
    }
    RC(fib::use_device(device));
    for (auto &d : c.single) if (d->device == device) { out.push_back(d); return FIB_OK; }
    c.single.emplace_back(new DevState());
    c.single.back()->device = device;
    out.push_back(c.single.back());
    return FIB_OK;
}

// ---- plan cache ----------------------------------------------------------------------------------------------------------------
void key_add(std::string &k, const void *p, size_t bytes) { k.append((const char *)&bytes, sizeof bytes); if (p) k.append((const char *)p, bytes); }

template <typename Plan, void (*Destroy)(Plan *)>
void destroy_plan(void *p) { Destroy(static_cast<Plan *>(p)); }

// the worker's plan of type Plan for `key`, made by make(Plan **) where the cache has none.  An entry matches on its key and its
// destroy function: plans of different types never stand for each other, whatever their keys.
template <typename Plan, void (*Destroy)(Plan *), typename MakeFn>
int cached_plan(DevState &d, const std::string &key, MakeFn make, Plan **plan) {
    void (*const destroy)(void *) = &destroy_plan<Plan, Destroy>;
    for (auto &c : d.plans) if (c.destroy == destroy && c.key == key) { c.stamp = ++d.clock; *plan = static_cast<Plan *>(c.plan); return FIB_OK; }
    Plan *p = nullptr;
    RC(make(&p));
    if (d.plans.size() >= 4) {                           // evict the least recently used
        size_t lru = 0;
        for (size_t i = 1; i < d.plans.size(); i++) if (d.plans[i].stamp < d.plans[lru].stamp) lru = i;
        d.plans[lru].destroy(d.plans[lru].plan);
        d.plans.erase(d.plans.begin() + lru);
    }
    d.plans.push_back(CachedPlan{key, p, destroy, ++d.clock});
    *plan = p;
    return FIB_OK;
}

// ---- the chunk pipeline (host_tier.h: fibh::run_chunks) on HIP streams ------------------------------------------------------------
// what a fit does with one chunk, all pointers on the device: din = the input rows back to back (row stride n), dmask = n
// bytes, dout = the output rows back to back (row stride n)
using ChunkFn = std::function<int(int chunk, int64_t rel, int64_t n, const float *din, const uint8_t *dmask, float *dout, hipStream_t st)>;

// the slab's LiveMap where packing pays (*use = &lm), NULL where the mask keeps (nearly) everything.  FIBERS_HOST_PACK=0: never.
int live_map_for(DevState &d, const void *mask, int mask_dtype, int64_t v0, int64_t v1, LiveMap &lm, const LiveMap **use) {
    *use = nullptr;
    const char *e = fib::env("FIBERS_HOST_PACK");
    if ((e && e[0] == '0') || v1 <= v0) return FIB_OK;
    if (!fibh::build_live_map(*d.pool, mask, mask_dtype, v0, v1, lm)) return fib::fail(FIB_ERR_INVALID, "unknown mask dtype %d", mask_dtype);
    if (fibh::live_pack_pays(lm, v0, v1)) *use = &lm;
    return FIB_OK;
}
int64_t pick_chunk(int64_t nrange, int rows_in, int rows_out) { return fibh::pick_chunk(nrange, rows_in, rows_out, fib::env("FIBERS_HOST_CHUNK")); }

// the device back end of fibh::run_chunks: the worker's pinned ring, its three streams (upload | kernels | download) and one event per
// ring slot and stage
struct HipDev {
    DevState &d;
    const ChunkFn &fn;
    hipStream_t st(fibh::Stream s) const { return s == fibh::S_IN ? d.s_in : (s == fibh::S_CMP ? d.s_cmp : d.s_out); }
    hipEvent_t ev(fibh::Event e, int b) const { return e == fibh::E_IN ? d.e_in[b] : (e == fibh::E_CMP ? d.e_cmp[b] : d.e_out[b]); }
    int ensure(size_t in_bytes, size_t out_bytes) {
        for (int b = 0; b < NBUF; b++) {
            RC(d.pin_in[b].ensure(in_bytes, d.device, d.cpus));
            RC(d.pin_out[b].ensure(out_bytes, d.device, d.cpus));
            RC(d.dev_in[b].ensure(in_bytes));
            RC(d.dev_out[b].ensure(out_bytes));
        }
        return FIB_OK;
    }
    char *pin_in(int b) { return d.pin_in[b].p; }
    char *pin_out(int b) { return d.pin_out[b].p; }
    int upload(int b, size_t bytes) {
        fib::ProfScope prof("host_h2d", d.s_in);
        FIB_HIP(hipMemcpyAsync(d.dev_in[b].p, d.pin_in[b].p, bytes, hipMemcpyHostToDevice, d.s_in));
        return FIB_OK;
    }
    int compute(int k, int b, int64_t rel, int64_t nd, int rin) {
        return fn(k, rel, nd, reinterpret_cast<const float *>(d.dev_in[b].p), reinterpret_cast<const uint8_t *>(d.dev_in[b].p) + (size_t)rin * nd * 4,
                  reinterpret_cast<float *>(d.dev_out[b].p), d.s_cmp);
    }
    int download(int b, size_t bytes) {
        fib::ProfScope prof("host_d2h", d.s_out);
        FIB_HIP(hipMemcpyAsync(d.pin_out[b].p, d.dev_out[b].p, bytes, hipMemcpyDeviceToHost, d.s_out));
        return FIB_OK;
    }
    int record(fibh::Event e, int b) { FIB_HIP(hipEventRecord(ev(e, b), st((fibh::Stream)e))); return FIB_OK; }      // (event kinds and streams are numbered alike)
    int stream_wait(fibh::Stream s, fibh::Event e, int b) { FIB_HIP(hipStreamWaitEvent(st(s), ev(e, b), 0)); return FIB_OK; }
    int host_wait(fibh::Event e, int b) { (void)hipSetDevice(d.device); return hipEventSynchronize(ev(e, b)) == hipSuccess ? FIB_OK : FIB_ERR_HIP; }
    void drain() { (void)hipStreamSynchronize(d.s_in); (void)hipStreamSynchronize(d.s_cmp); (void)hipStreamSynchronize(d.s_out); }
    void prof(const char *name, double ms) { if (fib::profiling_on()) fib::profile_add_ms(name, ms); }
    int fail(int code, const char *msg) { return fib::fail(code, "%s", msg); }
    std::string last_error() { return fib_last_error(); }
    void set_error(const std::string &m) { fib::set_error("%s", m.c_str()); }
};

// voxels [vbeg, vend) of a volume of nvox voxels through device d.  Blocking.  The caller holds d.mu.  (lm, outputs_zeroed: fibh::run_chunks)
int run_chunks(DevState &d, int64_t vbeg, int64_t vend, int64_t nvox, const std::vector<Rows> &ins, const void *mask, int mask_dtype,
               const std::vector<Rows> &outs, int64_t chunk, const ChunkFn &fn, const LiveMap *lm = nullptr, bool outputs_zeroed = false) {
    if (vend <= vbeg) return FIB_OK;
    FIB_HIP(hipSetDevice(d.device));
    HipDev dev{d, fn};
    const char *ent = fib::env("FIBERS_HOST_NT");        // streaming stores in the row copies: on unless FIBERS_HOST_NT=0
    const bool nt = !(ent && ent[0] == '0');
    return fibh::run_chunks(dev, *d.pool, *d.pool_out, vbeg, vend, nvox, ins, mask, mask_dtype, outs, chunk, lm, outputs_zeroed, nt);
}

// runs job(worker index, worker) on every worker of the set, one host thread each; the first error wins
int for_each_worker(const std::vector<Worker> &ws, const std::function<int(int, DevState &)> &job) {
    std::vector<int> rcs(ws.size(), FIB_OK);
    std::vector<std::string> msgs(ws.size());
    auto body = [&](int i) {
        try {
            std::lock_guard<std::mutex> lk(ws[i]->mu);
            fib::DeviceGuard guard;
            int rc = ws[i]->init(copy_threads((int)ws.size()));
            if (rc == FIB_OK) rc = job(i, *ws[i]);
            rcs[i] = rc;
            if (rc != FIB_OK) msgs[i] = fib_last_error();       // (thread-local message of the worker thread)
        } catch (const std::bad_alloc &) { rcs[i] = FIB_ERR_NOMEM; msgs[i] = "out of host memory"; }
        catch (...) { rcs[i] = FIB_ERR_INVALID; msgs[i] = "internal error in a device worker"; }
    };
    if (ws.size() == 1) body(0);
    else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < ws.size(); i++) th.emplace_back(body, (int)i);
        for (auto &t : th) t.join();
    }
    for (size_t i = 0; i < ws.size(); i++) if (rcs[i] != FIB_OK) return fib::fail(rcs[i], "%s", msgs[i].c_str());
    return FIB_OK;
}

// One call of a single-device, blocking-copy host form on its worker.  take() finds the worker of `device` (workers_for checks the index
// and makes the device current) and waits for its lock; the caller's device comes back when the lease goes.  FIB_DEVICE_ALL names no
// worker: refused under the form's sentence all_msg, or (NULL) answered as the index -1 that it is.  What is declared after the lease
// (buffers, plans) goes while it holds the lock.
struct DevLease {
    fib::DeviceGuard guard;
    Worker wk;
    std::unique_lock<std::mutex> lk;
    int take(int device, const char *all_msg) {
        if (device == FIB_DEVICE_ALL) return all_msg ? fib::fail(FIB_ERR_UNSUPPORTED, "%s", all_msg) : fib::use_device(device);
        std::vector<Worker> ws;
        RC(workers_for(device, ws));
        wk = ws[0];
        lk = std::unique_lock<std::mutex>(wk->mu);
        return FIB_OK;
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// device set
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_init(int ndev, const int *devs) try {
    FIB_CHECK(ndev >= 0 && (ndev == 0 || devs), FIB_ERR_INVALID, "invalid device list");
    const int have = fib_device_count();
    FIB_CHECK(have > 0, FIB_ERR_NO_DEVICE, "no HIP device is available and this back end has no CPU fallback");
    for (int i = 0; i < ndev; i++) FIB_CHECK(devs[i] >= 0 && devs[i] < have, FIB_ERR_NO_DEVICE, "device %d is not available (%d devices)", devs[i], have);
    HostCtx &c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    fib::DeviceGuard guard;
    for (auto &d : c.devs) { std::lock_guard<std::mutex> lk2(d->mu); }   // wait for calls in flight
    c.devs.clear();
    const int n = ndev > 0 ? ndev : have;
    for (int i = 0; i < n; i++) { c.devs.emplace_back(new DevState()); c.devs.back()->device = ndev > 0 ? devs[i] : i; }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_trim(void) try {
    HostCtx &c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    fib::DeviceGuard guard;
    for (auto *set : {&c.devs, &c.single})
        for (auto &d : *set) { std::lock_guard<std::mutex> lk2(d->mu); d->trim(); }     // (waits for a call in flight on that worker)
    return FIB_OK;
} FIB_API_CATCH

extern "C" void fib_shutdown(void) try {
    HostCtx &c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    fib::DeviceGuard guard;
    for (auto &d : c.devs) { std::lock_guard<std::mutex> lk2(d->mu); }     // wait for calls in flight (a call that has its workers but
    for (auto &d : c.single) { std::lock_guard<std::mutex> lk2(d->mu); }   // not yet their locks keeps them alive through its shared pointers)
    c.devs.clear();
    c.single.clear();
} FIB_API_CATCH_VOID

// ------------------------------------------------------------------------------------------------------------------------------
// dti_fit / adc_fit
// ------------------------------------------------------------------------------------------------------------------------------
namespace {
// What the voxel fits (fib_dti_fit, fib_adc_fit, fib_dki_fit, the ODF forms) share of a call's arguments, in the order every form checks
// them: the tables, the tessellation where there is one (tess_ok), the form's pointer arguments (ptrs_ok), the dimensions (with
// dims_more_ok: what else the form counts among them, under its own dims_msg), the FIB_MASK_OUTPUTS_ZEROED bit, the mask type, the
// form's output volumes (outs_ok, outs_msg), the workers.
struct FitCall {
    int mask_dtype = 0;                                  // without the FIB_MASK_OUTPUTS_ZEROED bit
    bool zeroed = false;
    int64_t nvox = 0;
    std::vector<Worker> ws;
};
int fit_call(FitCall &c, int device, const float *bval, int nvol, bool bvec_ok, bool ptrs_ok, int nx, int ny, int nz, int mask_dtype, bool outs_ok,
             const char *outs_msg = "NULL output volume", bool tess_ok = true, bool dims_more_ok = true,
             const char *dims_msg = "volume dimensions must be positive") {
    FIB_RC(fib::check_tables(bval, nullptr, nvol, false));
    FIB_CHECK(bvec_ok, FIB_ERR_MISSING_BVEC, "Missing gradient table from input DWI structure");
    FIB_CHECK(tess_ok, FIB_ERR_INVALID, "invalid ODF tessellation");
    FIB_CHECK(ptrs_ok, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && dims_more_ok, FIB_ERR_INVALID, "%s", dims_msg);
    c.zeroed = (mask_dtype & FIB_MASK_OUTPUTS_ZEROED) != 0;
    c.mask_dtype = mask_dtype & ~FIB_MASK_OUTPUTS_ZEROED;
    FIB_CHECK(dtype_size(c.mask_dtype) > 0, FIB_ERR_INVALID, "unknown mask dtype %d", c.mask_dtype);
    FIB_CHECK(outs_ok, FIB_ERR_INVALID, "%s", outs_msg);
    c.nvox = (int64_t)nx * ny * nz;
    return workers_for(device, c.ws);
}

// A fit on every worker of the call: its slab of the volume, its plan (plan_for(d, &plan)), the slab's live map where packing pays, the
// chunks.  fit(plan, din, dmask, n, dout, stream) is the form's fibd_* call on one chunk: n voxels, the rows of `outs` back to back in dout.
template <typename Plan, typename PlanFor, typename Fit>
int fit_run(const FitCall &c, const std::vector<Rows> &ins, const void *mask, const std::vector<Rows> &outs, PlanFor plan_for, Fit fit) {
    int rows_in = 0, rows_out = 0;
    for (auto &r : ins) rows_in += r.nrows;
    for (auto &r : outs) rows_out += r.nrows;
    return for_each_worker(c.ws, [&](int i, DevState &d) -> int {
        int64_t v0, v1;
        slab(c.nvox, (int)c.ws.size(), i, v0, v1);
        Plan *plan = nullptr;
        RC(plan_for(d, &plan));
        LiveMap lm;
        const LiveMap *use = nullptr;
        RC(live_map_for(d, mask, c.mask_dtype, v0, v1, lm, &use));
        return run_chunks(d, v0, v1, c.nvox, ins, mask, c.mask_dtype, outs, pick_chunk(use ? use->nlive : v1 - v0, rows_in, rows_out),
                          [&](int, int64_t, int64_t n, const float *din, const uint8_t *dm, float *b, hipStream_t st) -> int {
                              return fit(plan, din, dm, n, b, st);
                          }, use, c.zeroed);
    });
}

int dti_plan_for(DevState &d, const float *bval, const float *bvec, int nvol, fib_dti_plan **plan) {
    std::string key;
    key_add(key, bval, sizeof(float) * nvol);
    key_add(key, bvec, bvec ? sizeof(float) * 3 * nvol : 0);
    return cached_plan<fib_dti_plan, fib_dti_plan_destroy>(d, key, [&](fib_dti_plan **p) { return fib_dti_plan_create(d.device, bval, bvec, nvol, p); }, plan);
}
}  // namespace

extern "C" int fib_dti_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, const float *bvec,
                           const fib_dti_out *out) try {
    FitCall c;
    RC(fit_call(c, device, bval, nvol, bvec != nullptr, dwi && mask && out, nx, ny, nz, mask_dtype,
                out && out->s0 && out->eigval1 && out->eigval2 && out->eigval3 && out->eigvec1 && out->eigvec2 && out->eigvec3 && out->rd && out->md && out->fa));
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    const std::vector<Rows> outs = {{nullptr, out->s0, 1}, {nullptr, out->eigval1, 1}, {nullptr, out->eigval2, 1}, {nullptr, out->eigval3, 1},
                                    {nullptr, out->eigvec1, 3}, {nullptr, out->eigvec2, 3}, {nullptr, out->eigvec3, 3},
                                    {nullptr, out->rd, 1}, {nullptr, out->md, 1}, {nullptr, out->fa, 1}};
    return fit_run<fib_dti_plan>(c, ins, mask, outs, [&](DevState &d, fib_dti_plan **p) { return dti_plan_for(d, bval, bvec, nvol, p); },
                                 [](const fib_dti_plan *plan, const float *din, const uint8_t *dm, int64_t n, float *b, hipStream_t st) -> int {
                                     fib_dti_out dev{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 7 * n, b + 10 * n, b + 13 * n, b + 14 * n, b + 15 * n};
                                     return fibd_dti_fit(plan, din, dm, n, &dev, st);
                                 });
} FIB_API_CATCH

extern "C" int fib_adc_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, float *adc, float *s0) try {
    FitCall c;
    RC(fit_call(c, device, bval, nvol, true, dwi && mask && adc && s0, nx, ny, nz, mask_dtype, true));
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    const std::vector<Rows> outs = {{nullptr, adc, 1}, {nullptr, s0, 1}};
    return fit_run<fib_dti_plan>(c, ins, mask, outs, [&](DevState &d, fib_dti_plan **p) { return dti_plan_for(d, bval, nullptr, nvol, p); },
                                 [](const fib_dti_plan *plan, const float *din, const uint8_t *dm, int64_t n, float *b, hipStream_t st) -> int {
                                     return fibd_adc_fit(plan, din, dm, n, b, b + n, st);
                                 });
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// dki_fit
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_dki_fit(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, const float *bvec,
                           const float *verts, int nverts, const fib_dki_params *params, const fib_dki_out *out) try {
    FitCall c;
    RC(fit_call(c, device, bval, nvol, bvec != nullptr, dwi && mask && out && verts, nx, ny, nz, mask_dtype,
                out && out->s0 && out->eigval1 && out->eigval2 && out->eigval3 && out->eigvec1 && out->eigvec2 && out->eigvec3 && out->rd && out->md && out->fa &&
                    out->mk && out->ak && out->rk,
                "NULL output volume", true, nverts >= 2, "volume dimensions and the vertex count must be positive"));
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    std::vector<Rows> outs = {{nullptr, out->s0, 1}, {nullptr, out->eigval1, 1}, {nullptr, out->eigval2, 1}, {nullptr, out->eigval3, 1},
                              {nullptr, out->eigvec1, 3}, {nullptr, out->eigvec2, 3}, {nullptr, out->eigvec3, 3},
                              {nullptr, out->rd, 1}, {nullptr, out->md, 1}, {nullptr, out->fa, 1},
                              {nullptr, out->mk, 1}, {nullptr, out->ak, 1}, {nullptr, out->rk, 1}};
    const bool want_kt = out->kt != nullptr;
    if (want_kt) outs.push_back({nullptr, out->kt, 15});
    std::string key;
    key_add(key, bval, sizeof(float) * nvol);
    key_add(key, bvec, sizeof(float) * 3 * nvol);
    key_add(key, verts, sizeof(float) * 3 * nverts);
    key_add(key, params, params ? sizeof *params : 0);
    return fit_run<fib_dki_plan>(c, ins, mask, outs,
                                 [&](DevState &d, fib_dki_plan **p) {
                                     return cached_plan<fib_dki_plan, fib_dki_plan_destroy>(d, key, [&](fib_dki_plan **q) {
                                         return fib_dki_plan_create(d.device, bval, bvec, nvol, verts, nverts, params, q); }, p);
                                 },
                                 [&](const fib_dki_plan *plan, const float *din, const uint8_t *dm, int64_t n, float *b, hipStream_t st) -> int {
                                     fib_dki_out dev{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 7 * n, b + 10 * n, b + 13 * n, b + 14 * n, b + 15 * n,
                                                     b + 16 * n, b + 17 * n, b + 18 * n, want_kt ? b + 19 * n : nullptr};
                                     return fibd_dki_fit(plan, din, dm, n, &dev, st);
                                 });
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// csd_rec
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_csd_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, const float *bvec,
                           const float *verts, int nverts, const int32_t *faces, int nfaces, const fib_csd_params *params, const fib_csd_out *out) try {
    FitCall c;
    RC(fit_call(c, device, bval, nvol, bvec != nullptr, dwi && mask && out && params, nx, ny, nz, mask_dtype,
                out && out->sh && out->odf && out->niter && out->peak[0] && out->peak[1] && out->peak[2] && out->f[0] && out->f[1] && out->f[2],
                "NULL output volume", verts && faces && nverts >= 2 && nverts % 2 == 0 && nfaces > 0));
    // the refusals of the design come before any device is touched, and give the output rows their counts
    int nshell = 0, rank = 0;
    RC(fib_csd_design(bval, bvec, nvol, verts, nverts, params, nullptr, &nshell, nullptr, nullptr, nullptr, nullptr, &rank));
    const int n = (params->lmax + 1) * (params->lmax + 2) / 2, nreg = nverts / 2;
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    const std::vector<Rows> outs = {{nullptr, out->sh, n}, {nullptr, out->odf, nreg}, {nullptr, out->niter, 1},
                                    {nullptr, out->peak[0], 3}, {nullptr, out->peak[1], 3}, {nullptr, out->peak[2], 3},
                                    {nullptr, out->f[0], 1}, {nullptr, out->f[1], 1}, {nullptr, out->f[2], 1}};
    std::string key;
    key_add(key, "csd", 3);
    key_add(key, bval, sizeof(float) * nvol);
    key_add(key, bvec, sizeof(float) * 3 * nvol);
    key_add(key, verts, sizeof(float) * 3 * nverts);
    key_add(key, faces, sizeof(int32_t) * 3 * nfaces);
    key_add(key, params, sizeof *params);
    return fit_run<fib_csd_plan>(c, ins, mask, outs,
                                 [&](DevState &d, fib_csd_plan **p) {
                                     return cached_plan<fib_csd_plan, fib_csd_plan_destroy>(d, key, [&](fib_csd_plan **q) {
                                         return fib_csd_plan_create(d.device, bval, bvec, nvol, verts, nverts, faces, nfaces, params, q); }, p);
                                 },
                                 [&](const fib_csd_plan *plan, const float *din, const uint8_t *dm, int64_t nv, float *b, hipStream_t st) -> int {
                                     float *pk = b + (int64_t)(n + nreg + 1) * nv;
                                     fib_csd_out dev{b, b + (int64_t)n * nv, b + (int64_t)(n + nreg) * nv, {pk, pk + 3 * nv, pk + 6 * nv},
                                                     {pk + 9 * nv, pk + 10 * nv, pk + 11 * nv}};
                                     return fibd_csd_rec(plan, din, dm, nv, &dev, st);
                                 });
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// msmt_rec
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_msmt_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                            const void *mask, int mask_dtype, const float *bval, const float *bvec,
                            const float *verts, int nverts, const int32_t *faces, int nfaces, const fib_msmt_params *params,
                            const float *wm_R, const float *iso_r, int nshells, const fib_msmt_out *out) try {
    FitCall c;
    const int niso = params ? std::min(std::max(params->niso, 0), 2) : 0;
    RC(fit_call(c, device, bval, nvol, bvec != nullptr, dwi && mask && out && params && wm_R, nx, ny, nz, mask_dtype,
                out && out->sh && out->odf && out->niter && out->peak[0] && out->peak[1] && out->peak[2] && out->f[0] && out->f[1] && out->f[2] &&
                    (niso < 1 || out->iso[0]) && (niso < 2 || out->iso[1]),
                "NULL output volume", verts && faces && nverts >= 2 && nverts % 2 == 0 && nfaces > 0));
    // the refusals of the design come before any device is touched, and give the output rows their counts
    int rank = 0;
    RC(fib_msmt_design(bval, bvec, nvol, verts, nverts, params, wm_R, iso_r, nshells, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rank));
    const int nwm = (params->lmax + 1) * (params->lmax + 2) / 2, nreg = nverts / 2, nl = params->lmax / 2 + 1;
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    std::vector<Rows> outs = {{nullptr, out->sh, nwm}};
    for (int t = 0; t < niso; t++) outs.push_back({nullptr, out->iso[t], 1});
    for (const Rows &r : std::vector<Rows>{{nullptr, out->odf, nreg}, {nullptr, out->niter, 1},
                                           {nullptr, out->peak[0], 3}, {nullptr, out->peak[1], 3}, {nullptr, out->peak[2], 3},
                                           {nullptr, out->f[0], 1}, {nullptr, out->f[1], 1}, {nullptr, out->f[2], 1}}) outs.push_back(r);
    std::string key;
    key_add(key, "msmt", 4);
    key_add(key, bval, sizeof(float) * nvol);
    key_add(key, bvec, sizeof(float) * 3 * nvol);
    key_add(key, verts, sizeof(float) * 3 * nverts);
    key_add(key, faces, sizeof(int32_t) * 3 * nfaces);
    key_add(key, params, sizeof *params);
    key_add(key, wm_R, sizeof(float) * nshells * nl);
    key_add(key, iso_r, niso ? sizeof(float) * niso * nshells : 0);
    return fit_run<fib_msmt_plan>(c, ins, mask, outs,
                                  [&](DevState &d, fib_msmt_plan **p) {
                                      return cached_plan<fib_msmt_plan, fib_msmt_plan_destroy>(d, key, [&](fib_msmt_plan **q) {
                                          return fib_msmt_plan_create(d.device, bval, bvec, nvol, verts, nverts, faces, nfaces, params, wm_R, iso_r,
                                                                      nshells, q); }, p);
                                  },
                                  [&](const fib_msmt_plan *plan, const float *din, const uint8_t *dm, int64_t nv, float *b, hipStream_t st) -> int {
                                      float *is = b + (int64_t)nwm * nv, *od = is + (int64_t)niso * nv, *pk = od + (int64_t)(nreg + 1) * nv;
                                      fib_msmt_out dev{b, {niso > 0 ? is : nullptr, niso > 1 ? is + nv : nullptr}, od, od + (int64_t)nreg * nv,
                                                       {pk, pk + 3 * nv, pk + 6 * nv}, {pk + 9 * nv, pk + 10 * nv, pk + 11 * nv}};
                                      return fibd_msmt_rec(plan, din, dm, nv, &dev, st);
                                  });
} FIB_API_CATCH

extern "C" int fib_st_eigen(int device, const float *const S[6], int64_t nvox, float *eigvec, float *eigval) try {
    FIB_CHECK(S && eigvec && eigval, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nvox > 0, FIB_ERR_INVALID, "nvox must be positive");
    for (int k = 0; k < 6; k++) FIB_CHECK(S[k] != nullptr, FIB_ERR_INVALID, "NULL structure tensor volume %d", k);
    DevLease lease;
    RC(lease.take(device, nullptr));
    fib::DevBuf<float> d_in, d_out;
    RC(d_in.alloc((size_t)nvox * 6));
    RC(d_out.alloc((size_t)nvox * 12));
    const float *dS[6];
    for (int k = 0; k < 6; k++) { dS[k] = d_in.p + (size_t)k * nvox; RC(h2d(d_in.p + (size_t)k * nvox, S[k], sizeof(float) * nvox)); }
    RC(fibd_st_eigen(dS, nvox, d_out.p, d_out.p + (size_t)9 * nvox, nullptr));
    FIB_HIP(hipDeviceSynchronize());
    RC(d2h(eigvec, d_out.p, sizeof(float) * nvox * 9));
    RC(d2h(eigval, d_out.p + (size_t)9 * nvox, sizeof(float) * nvox * 3));
    return FIB_OK;
} FIB_API_CATCH

// xfm_apply host form: the 3 npoints floats are one planar row of 3 npoints "voxels" for the chunk pipeline (no mask).  Chunks and
// worker slabs start at multiples of 3 floats: the chunk is 3 * 2^17 floats, so its 1/8, 1/4, 1/2 lead-in pieces (host_tier.h:
// chunk_schedule) are multiples of 96, and the slabs are cut at whole points.
extern "C" int fib_xfm_apply(int device, const float vox2vox[16], const float *in, float *out, int64_t npoints) try {
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    if (npoints == 0) return FIB_OK;
    FIB_CHECK(vox2vox && in && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(in == out || in + 3 * npoints <= out || out + 3 * npoints <= in, FIB_ERR_INVALID, "in and out must be the same array or not overlap");
    const int64_t nf = 3 * npoints;
    std::vector<Worker> ws;
    RC(workers_for(device, ws));
    const std::vector<Rows> ins = {{in, nullptr, 1}};
    const std::vector<Rows> outs = {{nullptr, out, 1}};
    constexpr int64_t chunk = (int64_t)3 << 17;
    return for_each_worker(ws, [&](int i, DevState &d) -> int {
        const int64_t n = (int64_t)ws.size();
        const int64_t v0 = 3 * (npoints * i / n), v1 = 3 * (npoints * (i + 1) / n);
        return run_chunks(d, v0, v1, nf, ins, nullptr, 0, outs, chunk,
                          [&](int, int64_t, int64_t nd, const float *din, const uint8_t *, float *dout, hipStream_t st) -> int {
                              return fibd_xfm_apply(vox2vox, din, dout, nd / 3, st);
                          });
    });
} FIB_API_CATCH

// st_recon host form: z-slabs of the volume, each uploaded with its halo; a slab's outputs scatter into the [nx,ny,nz,...] arrays
extern "C" int fib_st_recon(int device, const float *vol, int nx, int ny, int nz, float sigma, float rho, float *eigvec, float *eigval) try {
    FIB_CHECK(vol && eigvec && eigval, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    FIB_CHECK(device != FIB_DEVICE_ALL, FIB_ERR_UNSUPPORTED, "st_recon runs on one device (FIB_DEVICE_ALL is not supported)");
    int halo = 0;
    RC(fib_st_recon_halo(sigma, rho, &halo));
    DevLease lease;
    RC(lease.take(device, nullptr));                       // (FIB_DEVICE_ALL: refused above, before the radii)
    const size_t plane = (size_t)nx * ny;
    int nzs = 0;
    if (const char *e = fib::env("FIBERS_ST_RECON_SLAB")) nzs = std::min(atoi(e), nz);
    if (nzs <= 0) {
        size_t fr = 0, tot = 0;
        FIB_HIP(hipMemGetInfo(&fr, &tot));
        nzs = fibh::planes_per_slab(fr, plane, halo, nz);
        FIB_CHECK(nzs >= 1, FIB_ERR_NOMEM, "st_recon: one %d x %d plane with its halo does not fit in device memory", nx, ny);
    }
    size_t work_bytes = 0;
    RC(fibd_st_recon_work_size(nx, ny, nzs, sigma, rho, &work_bytes));
    const int nzin_max = std::min(nz, nzs + 2 * halo);
    fib::DevBuf<float> d_vol, d_out;
    fib::DevBuf<char> d_work;
    RC(d_vol.alloc(plane * nzin_max));
    RC(d_out.alloc(plane * nzs * 12));
    RC(d_work.alloc(work_bytes));
    const size_t nvox = plane * nz;
    for (int z0 = 0; z0 < nz; z0 += nzs) {
        const int z1 = std::min(nz, z0 + nzs), zin0 = std::max(0, z0 - halo), zin1 = std::min(nz, z1 + halo);
        const size_t nout = plane * (z1 - z0);
        RC(h2d(d_vol.p, vol + plane * zin0, sizeof(float) * plane * (zin1 - zin0)));
        RC(fibd_st_recon(d_vol.p, nx, ny, nz, zin0, zin1 - zin0, z0, z1, sigma, rho, d_out.p, d_out.p + 9 * nout, nullptr,
                         d_work.p, work_bytes, nullptr));
        FIB_HIP(hipDeviceSynchronize());
        for (int k = 0; k < 9; k++) RC(d2h(eigvec + k * nvox + plane * z0, d_out.p + k * nout, sizeof(float) * nout));
        for (int k = 0; k < 3; k++) RC(d2h(eigval + k * nvox + plane * z0, d_out.p + (9 + k) * nout, sizeof(float) * nout));
    }
    return FIB_OK;
} FIB_API_CATCH

// dwi_denoise host form: z-slabs of every frame, each uploaded with the planes its clamped patches reach (P - 1 beyond the slab, all to
// one side at a face); a slab's rows scatter into the [nx,ny,nz,nvol] array
extern "C" int fib_dwi_denoise(int device, const float *dwi, int nx, int ny, int nz, int nvol, const uint8_t *mask, int patch, int estimator,
                               float *out, float *sigma, float *rank) try {
    FIB_CHECK(dwi && mask && out && sigma && rank, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "nx, ny, nz must be positive");
    FIB_CHECK(device != FIB_DEVICE_ALL, FIB_ERR_UNSUPPORTED, "dwi_denoise runs on one device (FIB_DEVICE_ALL is not supported)");
    RC(fib_dwi_denoise_check(nx, ny, nz, nvol, patch, estimator));
    DevLease lease;
    RC(lease.take(device, nullptr));                       // (FIB_DEVICE_ALL: refused above, before the shape)
    const size_t plane = (size_t)nx * ny;
    size_t work_bytes = 0;
    RC(fibd_dwi_denoise_work_size(nx, ny, nz, nvol, patch, &work_bytes));   // (the whole volume's: no slab needs more)
    int nzs = 0;
    if (const char *e = fib::env("FIBERS_DENOISE_SLAB")) nzs = std::min(atoi(e), nz);
    if (nzs <= 0) {
        size_t fr = 0, tot = 0;
        FIB_HIP(hipMemGetInfo(&fr, &tot));
        // planes_per_slab counts 64 bytes a voxel of an output plane and 16 a voxel of each of 2 * halo further planes.  Here an output
        // plane costs 8 nvol + 9 (frames in and out, sigma, rank, mask) and each of the P - 1 further planes 4 nvol: with planes of
        // ceil((8 nvol + 9) / 64) voxels' worth and halo = P - 1 both are covered.  It plans with half of what it is given, so the
        // workspace comes off twice
        const size_t scale = ((size_t)8 * nvol + 9 + 63) / 64;
        nzs = fibh::planes_per_slab(fr > 2 * work_bytes ? fr - 2 * work_bytes : 0, plane * scale, patch - 1, nz);
        FIB_CHECK(nzs >= 1, FIB_ERR_NOMEM, "dwi_denoise: one %d x %d plane of %d frames with its halo does not fit in device memory", nx, ny, nvol);
    }
    const int nzin_max = std::min(nz, nzs + patch - 1), h = patch / 2;
    fib::DevBuf<float> d_in, d_out;
    fib::DevBuf<uint8_t> d_mask;
    fib::DevBuf<char> d_work;
    RC(d_in.alloc(plane * nzin_max * nvol));
    RC(d_out.alloc(plane * nzs * ((size_t)nvol + 2)));
    RC(d_mask.alloc(plane * nzs));
    RC(d_work.alloc(work_bytes));
    const size_t nvox = plane * nz;
    for (int z0 = 0; z0 < nz; z0 += nzs) {
        const int z1 = std::min(nz, z0 + nzs);
        const int zin0 = std::min(std::max(z0 - h, 0), nz - patch), zin1 = std::min(std::max(z1 - 1 - h, 0), nz - patch) + patch;
        const size_t nin = plane * (zin1 - zin0), nout = plane * (z1 - z0);
        for (int f = 0; f < nvol; f++) RC(h2d(d_in.p + f * nin, dwi + f * nvox + plane * zin0, sizeof(float) * nin));
        RC(h2d(d_mask.p, mask + plane * z0, nout));
        float *d_sigma = d_out.p + (size_t)nvol * nout, *d_rank = d_sigma + nout;
        RC(fibd_dwi_denoise(d_in.p, nx, ny, nz, zin0, zin1 - zin0, z0, z1, nvol, patch, estimator, d_mask.p, d_out.p, d_sigma, d_rank,
                            d_work.p, work_bytes, nullptr));
        FIB_HIP(hipDeviceSynchronize());
        for (int f = 0; f < nvol; f++) RC(d2h(out + f * nvox + plane * z0, d_out.p + f * nout, sizeof(float) * nout));
        RC(d2h(sigma + plane * z0, d_sigma, sizeof(float) * nout));
        RC(d2h(rank + plane * z0, d_rank, sizeof(float) * nout));
    }
    return FIB_OK;
} FIB_API_CATCH

// The frame resampler of fib_vol_xform and fib_warp_volume, in the two pieces a form puts around its lease: frame_checks after its own
// checks; frame_chunks once what stays resident is on the device.  Frames are independent: chunks of whole frames, per chunk upload,
// launch(d_in, d_out, nf) = the form's fibd_* call, download.  Copies block on the NULL stream: the read-back comes behind the kernel.
namespace {
int frame_checks(const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, const void *out, int nxo, int nyo, int nzo) {
    FIB_CHECK(nxi > 0 && nyi > 0 && nzi > 0 && nxo > 0 && nyo > 0 && nzo > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(interp == FIB_VOL_NEAREST || interp == FIB_VOL_TRILINEAR, FIB_ERR_INVALID, "unknown interpolation %d", interp);
    const size_t nvi = (size_t)nxi * nyi * nzi, nvo = (size_t)nxo * nyo * nzo;
    const uintptr_t ai = reinterpret_cast<uintptr_t>(vol), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK(ai + 4 * nvi * nframes <= ao || ao + 4 * nvo * nframes <= ai, FIB_ERR_INVALID, "vol and out must not overlap");
    return FIB_OK;
}
// frames of nvi voxels in, nvo out; a chunk holds env_name's count of them, else what fits in half the memory free now (or nomem_msg)
template <typename Launch>
int frame_chunks(const void *vol, size_t nvi, void *out, size_t nvo, int nframes, const char *env_name, const char *nomem_msg, Launch launch) {
    int nfc = 0;
    if (const char *e = fib::env(env_name)) nfc = std::min(atoi(e), nframes);
    if (nfc <= 0) {
        size_t fr = 0, tot = 0;
        FIB_HIP(hipMemGetInfo(&fr, &tot));
        nfc = fibh::frames_per_chunk(fr, nvi, nvo, nframes);
        FIB_CHECK(nfc >= 1, FIB_ERR_NOMEM, "%s", nomem_msg);
    }
    fib::DevBuf<uint32_t> d_in, d_out;
    RC(d_in.alloc(nvi * nfc));
    RC(d_out.alloc(nvo * nfc));
    for (int f0 = 0; f0 < nframes; f0 += nfc) {
        const int nf = std::min(nfc, nframes - f0);
        RC(h2d(d_in.p, static_cast<const uint32_t *>(vol) + nvi * f0, sizeof(uint32_t) * nvi * nf));
        RC(launch(d_in.p, d_out.p, nf));
        RC(d2h(static_cast<uint32_t *>(out) + nvo * f0, d_out.p, sizeof(uint32_t) * nvo * nf));
    }
    return FIB_OK;
}
}  // namespace

extern "C" int fib_vol_xform(int device, const float out2in[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp,
                             int32_t outside_bits, void *out, int nxo, int nyo, int nzo) try {
    FIB_CHECK(out2in && vol && out, FIB_ERR_INVALID, "NULL argument");
    RC(frame_checks(vol, nxi, nyi, nzi, nframes, interp, out, nxo, nyo, nzo));
    DevLease lease;
    RC(lease.take(device, "vol_xform runs on one device (FIB_DEVICE_ALL is not supported)"));
    return frame_chunks(vol, (size_t)nxi * nyi * nzi, out, (size_t)nxo * nyo * nzo, nframes, "FIBERS_VOL_XFORM_FRAMES",
                        "vol_xform: one input and one output frame do not fit in device memory", [&](const uint32_t *d_in, uint32_t *d_out, int nf) {
                            return fibd_vol_xform(out2in, d_in, nxi, nyi, nzi, nf, interp, outside_bits, d_out, nxo, nyo, nzo, nullptr);
                        });
} FIB_API_CATCH

// ---- the brain mask's host forms (volmask.hip).  What stays resident is allocated first, so that the chunk is sized by what is left.
// dwi_mask: only the listed frames travel, a chunk at a time in the list's order, into the float64 sums of the workspace
extern "C" int fib_dwi_mask(int device, const float *dwi, int nx, int ny, int nz, int nvol, const int32_t *frames, int nframes,
                            const fib_mask_params *params, uint8_t *mask, float *b0, fib_mask_info *info) try {
    FIB_CHECK(dwi && mask && info, FIB_ERR_INVALID, "NULL argument");
    RC(fib_dwi_mask_check(nx, ny, nz, nvol, frames, nframes, params));
    DevLease lease;
    RC(lease.take(device, "dwi_mask runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvox = (size_t)nx * ny * nz;
    size_t work_bytes = 0;
    RC(fibd_dwi_mask_work_size(nx, ny, nz, &work_bytes));
    fib::DevBuf<char> d_work;
    fib::DevBuf<uint8_t> d_mask;
    fib::DevBuf<float> d_b0, d_frames;
    fib::DevBuf<fib_mask_info> d_info;
    RC(d_work.alloc(work_bytes));
    RC(d_mask.alloc(nvox));
    if (b0) RC(d_b0.alloc(nvox));
    RC(d_info.alloc(1));
    int nfc = 0;
    if (const char *e = fib::env("FIBERS_MASK_FRAMES")) nfc = std::min(atoi(e), nframes);
    if (nfc <= 0) {
        size_t fr = 0, tot = 0;
        FIB_HIP(hipMemGetInfo(&fr, &tot));
        nfc = fibh::frames_per_chunk(fr, nvox, 0, nframes);
        FIB_CHECK(nfc >= 1, FIB_ERR_NOMEM, "dwi_mask: one frame does not fit in device memory beside the workspace");
    }
    RC(d_frames.alloc(nvox * nfc));
    for (int f0 = 0; f0 < nframes; f0 += nfc) {
        const int nf = std::min(nfc, nframes - f0);
        for (int j = 0; j < nf; j++) RC(h2d(d_frames.p + nvox * j, dwi + nvox * frames[f0 + j], sizeof(float) * nvox));
        RC(fib::vm_mean_add(d_work.p, d_frames.p, (int64_t)nvox, nf, f0 == 0, nullptr));
        FIB_HIP(hipStreamSynchronize(nullptr));             // (the chunk's buffer is written again next round)
    }
    RC(fib::vm_mask_finish(d_work.p, nframes, nx, ny, nz, params, d_mask.p, b0 ? d_b0.p : nullptr, d_info.p, nullptr));
    RC(d2h(mask, d_mask.p, nvox));
    if (b0) RC(d2h(b0, d_b0.p, sizeof(float) * nvox));
    RC(d2h(info, d_info.p, sizeof(fib_mask_info)));
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_vol_median(int device, const float *in, int nx, int ny, int nz, int nframes, int radius, int numpass, float *out) try {
    FIB_CHECK(in && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nframes > 0, FIB_ERR_INVALID, "nframes must be positive");
    size_t work_bytes = 0;
    RC(fibd_vol_median_work_size(nx, ny, nz, numpass, &work_bytes));
    FIB_CHECK(radius >= 1 && radius <= 3, FIB_ERR_INVALID, "the median's radius must be 1, 2 or 3, not %d", radius);
    const size_t nvox = (size_t)nx * ny * nz;
    const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK(ai + 4 * nvox * nframes <= ao || ao + 4 * nvox * nframes <= ai, FIB_ERR_INVALID, "in and out must not overlap");
    DevLease lease;
    RC(lease.take(device, "vol_median runs on one device (FIB_DEVICE_ALL is not supported)"));
    fib::DevBuf<char> d_work;
    RC(d_work.alloc(work_bytes));
    return frame_chunks(in, nvox, out, nvox, nframes, "FIBERS_MEDIAN_FRAMES", "vol_median: one input and one output frame do not fit in device memory",
                        [&](const uint32_t *d_in, uint32_t *d_out, int nf) {
                            for (int f = 0; f < nf; f++)
                                RC(fibd_vol_median(reinterpret_cast<const float *>(d_in) + nvox * f, nx, ny, nz, radius, numpass,
                                                   reinterpret_cast<float *>(d_out) + nvox * f, d_work.p, work_bytes, nullptr));
                            return (int)FIB_OK;
                        });
} FIB_API_CATCH

extern "C" int fib_mask_components(int device, const uint8_t *mask, int nx, int ny, int nz, int flags, int32_t *labels, uint8_t *out_mask,
                                   fib_mask_info *info) try {
    FIB_CHECK(mask && info, FIB_ERR_INVALID, "NULL argument");
    size_t work_bytes = 0;
    RC(fibd_mask_components_work_size(nx, ny, nz, &work_bytes));
    FIB_CHECK((flags & ~(FIB_MASK_KEEP_LARGEST | FIB_MASK_FILL_HOLES)) == 0, FIB_ERR_INVALID, "mask_components: unknown flags 0x%x", flags);
    DevLease lease;
    RC(lease.take(device, "mask_components runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvox = (size_t)nx * ny * nz;
    fib::DevBuf<char> d_work;
    fib::DevBuf<uint8_t> d_mask, d_out;
    fib::DevBuf<int32_t> d_labels;
    fib::DevBuf<fib_mask_info> d_info;
    RC(d_work.alloc(work_bytes));
    RC(fib::upload(d_mask, mask, nvox));
    if (out_mask) RC(d_out.alloc(nvox));
    if (labels) RC(d_labels.alloc(nvox));
    RC(d_info.alloc(1));
    RC(fibd_mask_components(d_mask.p, nx, ny, nz, flags, labels ? d_labels.p : nullptr, out_mask ? d_out.p : nullptr, d_info.p, d_work.p,
                            work_bytes, nullptr));
    if (out_mask) RC(d2h(out_mask, d_out.p, nvox));
    if (labels) RC(d2h(labels, d_labels.p, sizeof(int32_t) * nvox));
    RC(d2h(info, d_info.p, sizeof(fib_mask_info)));
    return FIB_OK;
} FIB_API_CATCH

// ---- Gibbs-ringing removal (degibbs.hip).  Slices are independent: a chunk is whole frames, or slices [a0, a1) of one frame, and the
// device entry takes it as a volume of its own whose slice axis is that short.  A slab of slices is a run of `height` pieces of `width`
// elements, `pitch` apart in the host volume and back to back on the device (slice axis 2: one piece).
namespace {
struct SliceSlab { size_t off, width, height, pitch; };
SliceSlab slice_slab(int axis, int nx, int ny, int nz, int a0, int a1) {
    const size_t s = (size_t)(a1 - a0), plane = (size_t)nx * ny;
    if (axis == 2) return SliceSlab{plane * a0, plane * s, 1, plane * s};
    if (axis == 1) return SliceSlab{(size_t)nx * a0, (size_t)nx * s, (size_t)nz, plane};
    return SliceSlab{(size_t)a0, s, (size_t)ny * nz, (size_t)nx};
}
int slab_copy(void *dev, void *host, const SliceSlab &b, size_t es, bool to_device) {
    char *h = static_cast<char *>(host) + b.off * es;
    if (b.height == 1) return to_device ? h2d(dev, h, b.width * es) : d2h(h, dev, b.width * es);
    if (to_device) FIB_HIP(hipMemcpy2D(dev, b.width * es, h, b.pitch * es, b.width * es, b.height, hipMemcpyHostToDevice));
    else FIB_HIP(hipMemcpy2D(h, b.pitch * es, dev, b.width * es, b.width * es, b.height, hipMemcpyDeviceToHost));
    return FIB_OK;
}
}  // namespace

extern "C" int fib_dwi_degibbs(int device, const float *dwi, int nx, int ny, int nz, int nvol, const fib_degibbs_params *params, float *out,
                               int8_t *shift_u, int8_t *shift_v) try {
    FIB_CHECK(dwi && out, FIB_ERR_INVALID, "NULL argument");
    RC(fib_dwi_degibbs_check(nx, ny, nz, nvol, params));
    const fib_degibbs_params dflt = FIB_DEGIBBS_PARAMS_DEFAULT, prm = params ? *params : dflt;
    const size_t nvox = (size_t)nx * ny * nz;
    const uintptr_t ai = reinterpret_cast<uintptr_t>(dwi), ao = reinterpret_cast<uintptr_t>(out);
    FIB_CHECK(ai + 4 * nvox * nvol <= ao || ao + 4 * nvox * nvol <= ai, FIB_ERR_INVALID, "dwi_degibbs: dwi and out must not overlap (there is no in-place form)");
    DevLease lease;
    RC(lease.take(device, "dwi_degibbs runs on one device (FIB_DEVICE_ALL is not supported)"));
    const int axis = prm.slice_axis, dims[3] = {nx, ny, nz}, ns = dims[axis];
    const size_t slice = nvox / ns;                        // voxels of a slice
    int64_t per = 0;                                       // slices per chunk
    if (const char *e = fib::env("FIBERS_DEGIBBS_SLICES")) per = atoll(e);
    if (per <= 0) {
        size_t fr = 0, tot = 0, wb = 0;
        FIB_HIP(hipMemGetInfo(&fr, &tot));
        RC(fibd_dwi_degibbs_work_size(nx, ny, nz, nvol, &prm, &wb));        // (the whole series': no chunk needs more)
        // a slice costs its float32 input and output and two int8 planes; the workspace comes off first, twice, as the plan is for half
        per = (int64_t)((fr > 2 * wb ? fr - 2 * wb : 0) / 2 / (10 * slice));
        FIB_CHECK(per >= 1, FIB_ERR_NOMEM, "dwi_degibbs: one slice does not fit in device memory beside the workspace");
    }
    const int nfc = per >= ns ? (int)std::min<int64_t>(per / ns, nvol) : 1, nsc = per >= ns ? ns : (int)per;      // frames and slices of a chunk
    int cd[3] = {nx, ny, nz};
    cd[axis] = nsc;
    size_t work_bytes = 0;
    RC(fibd_dwi_degibbs_work_size(cd[0], cd[1], cd[2], nfc, &prm, &work_bytes));
    const size_t cvox = slice * nsc;
    fib::DevBuf<float> d_in, d_out;
    fib::DevBuf<int8_t> d_su, d_sv;
    fib::DevBuf<char> d_work;
    RC(d_in.alloc(cvox * nfc));
    RC(d_out.alloc(cvox * nfc));
    if (shift_u) RC(d_su.alloc(cvox * nfc));
    if (shift_v) RC(d_sv.alloc(cvox * nfc));
    RC(d_work.alloc(work_bytes));
    for (int f0 = 0; f0 < nvol; f0 += nfc)
        for (int a0 = 0; a0 < ns; a0 += nsc) {
            const int nf = std::min(nfc, nvol - f0), a1 = std::min(ns, a0 + nsc);
            const SliceSlab b = slice_slab(axis, nx, ny, nz, a0, a1);
            const size_t n = slice * (a1 - a0);
            cd[axis] = a1 - a0;
            for (int f = 0; f < nf; f++) RC(slab_copy(d_in.p + n * f, const_cast<float *>(dwi) + nvox * (f0 + f), b, 4, true));
            RC(fibd_dwi_degibbs(d_in.p, cd[0], cd[1], cd[2], nf, &prm, d_out.p, shift_u ? d_su.p : nullptr, shift_v ? d_sv.p : nullptr, d_work.p,
                                work_bytes, nullptr));
            for (int f = 0; f < nf; f++) {                 // (blocking copies on the NULL stream: behind the kernels)
                RC(slab_copy(d_out.p + n * f, out + nvox * (f0 + f), b, 4, false));
                if (shift_u) RC(slab_copy(d_su.p + n * f, shift_u + nvox * (f0 + f), b, 1, false));
                if (shift_v) RC(slab_copy(d_sv.p + n * f, shift_v + nvox * (f0 + f), b, 1, false));
            }
        }
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// non-linear warps: host forms. One device; the planar field is uploaded and packed once and stays resident for the call, the points
// or the frames travel in chunks.  Copies block on the NULL stream, so a read-back comes behind its kernel.  The buffers are local.
// ------------------------------------------------------------------------------------------------------------------------------
namespace {
// the field of a host call (checked by the form) on the current device: upload, pack, and the planar copy goes back to the driver
int warp_field_upload(const float *disp, int nx, int ny, int nz, fib::DevBuf<float> &packed) {
    const size_t nvox = (size_t)nx * ny * nz;
    fib::DevBuf<float> planar;
    RC(planar.alloc(3 * nvox));
    RC(packed.alloc(4 * nvox));
    RC(h2d(planar.p, disp, sizeof(float) * 3 * nvox));
    RC(fibd_warp_pack(planar.p, nx, ny, nz, packed.p, nullptr));
    FIB_HIP(hipDeviceSynchronize());
    return FIB_OK;
}
}  // namespace

extern "C" int fib_warp_points(int device, const float *disp, int nx, int ny, int nz, const float to_ras[16], const float to_field[16],
                               const float from_ras[16], const float *xyz, float *out, int64_t npoints) try {
    FIB_CHECK(disp && to_ras && to_field && from_ras, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    FIB_CHECK(npoints == 0 || (xyz && out), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(xyz == out || xyz + 3 * npoints <= out || out + 3 * npoints <= xyz, FIB_ERR_INVALID, "xyz and out must be the same array or not overlap");
    DevLease lease;
    RC(lease.take(device, "warp_points runs on one device (FIB_DEVICE_ALL is not supported)"));
    if (npoints == 0) return FIB_OK;
    int64_t chunk = (int64_t)1 << 22;                       // 48 MB of points per chunk
    if (const char *e = fib::env("FIBERS_WARP_POINTS")) { const long long v = atoll(e); if (v > 0) chunk = v; }
    fib::DevBuf<float> d_field, d_xyz;
    RC(warp_field_upload(disp, nx, ny, nz, d_field));
    RC(d_xyz.alloc((size_t)3 * std::min(chunk, npoints)));
    for (int64_t p0 = 0; p0 < npoints; p0 += chunk) {
        const int64_t np = std::min(chunk, npoints - p0);
        RC(h2d(d_xyz.p, xyz + 3 * p0, sizeof(float) * 3 * (size_t)np));
        RC(fibd_warp_points(d_field.p, nx, ny, nz, to_ras, to_field, from_ras, d_xyz.p, d_xyz.p, np, nullptr));
        RC(d2h(out + 3 * p0, d_xyz.p, sizeof(float) * 3 * (size_t)np));
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_warp_volume(int device, const float *disp, int nx, int ny, int nz, const float to_ras[16], const float to_field[16],
                               const float from_ras[16], const void *vol, int nxi, int nyi, int nzi, int nframes, int interp, int32_t outside_bits,
                               void *out, int nxo, int nyo, int nzo) try {
    FIB_CHECK(disp && to_ras && to_field && from_ras && vol && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    RC(frame_checks(vol, nxi, nyi, nzi, nframes, interp, out, nxo, nyo, nzo));
    DevLease lease;
    RC(lease.take(device, "warp_volume runs on one device (FIB_DEVICE_ALL is not supported)"));
    fib::DevBuf<float> d_field;
    RC(warp_field_upload(disp, nx, ny, nz, d_field));       // (resident before frame_chunks looks at the free memory)
    char nomem[128];
    snprintf(nomem, sizeof nomem, "warp_volume: the field (%zu voxels), one input and one output frame do not fit in device memory", (size_t)nx * ny * nz);
    return frame_chunks(vol, (size_t)nxi * nyi * nzi, out, (size_t)nxo * nyo * nzo, nframes, "FIBERS_WARP_FRAMES", nomem,
                        [&](const uint32_t *d_in, uint32_t *d_out, int nf) {
                            return fibd_warp_volume(d_field.p, nx, ny, nz, to_ras, to_field, from_ras, d_in, nxi, nyi, nzi, nf, interp, outside_bits,
                                                    d_out, nxo, nyo, nzo, nullptr);
                        });
} FIB_API_CATCH

extern "C" int fib_warp_invert(int device, const float *disp, int nx, int ny, int nz, const float out_to_ras[16], const float ras_to_field[16],
                               int niter, float *inv, float *err, int nxo, int nyo, int nzo) try {
    FIB_CHECK(disp && out_to_ras && ras_to_field && inv, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && nxo > 0 && nyo > 0 && nzo > 0, FIB_ERR_INVALID, "the field's and the output's dimensions must be positive");
    FIB_CHECK(niter >= 0, FIB_ERR_INVALID, "niter must not be negative");
    DevLease lease;
    RC(lease.take(device, "warp_invert runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvo = (size_t)nxo * nyo * nzo;
    fib::DevBuf<float> d_field, d_out;
    RC(warp_field_upload(disp, nx, ny, nz, d_field));
    RC(d_out.alloc(4 * nvo));
    RC(fibd_warp_invert(d_field.p, nx, ny, nz, out_to_ras, ras_to_field, niter, d_out.p, err ? d_out.p + 3 * nvo : nullptr, nxo, nyo, nzo, nullptr));
    RC(d2h(inv, d_out.p, sizeof(float) * 3 * nvo));
    if (err) RC(d2h(err, d_out.p + 3 * nvo, sizeof(float) * nvo));
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// registration: the host form.  One device; both volumes, the pyramids and (for dwi_moco) the resampled series stay on the device, the
// searches are the host state machines of setup.cpp and fibd_reg_run moves histograms between the two.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_mri_register(int device, const float *moving, const int32_t moving_size[3], const float moving_vox2ras[16], int nframes,
                                const float *fixed, const int32_t fixed_size[3], const float fixed_res[3], const float fixed_vox2ras[16], int dof,
                                int nbins, int levels, int halvings, int maxit, double min_overlap, double *theta, double *cost, int *niter,
                                double *trace, int trace_rows, float *resampled) try {
    FIB_CHECK(moving && moving_size && moving_vox2ras && fixed && fixed_size && fixed_res && fixed_vox2ras && theta, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nframes > 0, FIB_ERR_INVALID, "nframes must be positive");
    FIB_CHECK(trace_rows >= 0 && (trace || trace_rows == 0), FIB_ERR_INVALID, "trace_rows rows need a trace buffer");
    struct Searches {                                       // (the refusals of fib_reg_search_create come before the device is touched)
        std::vector<fib_reg_search *> h;
        ~Searches() { for (auto *s : h) fib_reg_search_destroy(s); }
    } searches;
    for (int f = 0; f < nframes; f++) {
        fib_reg_search *s = nullptr;
        RC(fib_reg_search_create(dof, fixed_size, fixed_res, fixed_vox2ras, moving_size, moving_vox2ras, levels, halvings, maxit, min_overlap, nullptr, &s));
        searches.h.push_back(s);
    }
    if (levels == 0) RC(fib_reg_levels(fixed_size, moving_size, &levels));
    size_t work_bytes = 0;
    RC(fibd_reg_run_work_size(fixed_size, moving_size, nframes, nframes, levels, nbins, &work_bytes));
    DevLease lease;
    RC(lease.take(device, "mri_register runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvf = (size_t)fixed_size[0] * fixed_size[1] * fixed_size[2], nvm = (size_t)moving_size[0] * moving_size[1] * moving_size[2];
    fib::DevBuf<float> d_fixed, d_moving, d_out;
    fib::DevBuf<char> d_work;
    RC(fib::upload(d_fixed, fixed, nvf));
    RC(fib::upload(d_moving, moving, nvm * nframes));
    RC(d_work.alloc(work_bytes));
    std::vector<int32_t> frames((size_t)nframes);
    for (int f = 0; f < nframes; f++) frames[f] = f;
    RC(fibd_reg_run(searches.h.data(), frames.data(), nframes, d_fixed.p, fixed_size, d_moving.p, moving_size, nframes, levels, nbins, d_work.p,
                    work_bytes, nullptr));
    for (int f = 0; f < nframes; f++)
        RC(fib_reg_search_result(searches.h[f], theta + 12 * (size_t)f, cost ? cost + f : nullptr, niter ? niter + f : nullptr,
                                 trace ? trace + (size_t)FIB_REG_TRACE_ROW * trace_rows * f : nullptr, trace_rows));
    if (!resampled) return FIB_OK;
    // every frame through its own final level-0 matrix onto the fixed grid: trilinear, 0 outside
    RC(d_out.alloc(nvf * nframes));
    for (int f = 0; f < nframes; f++) {
        float M[16];
        RC(fib_reg_matrix(theta + 12 * (size_t)f, 12, fixed_vox2ras, fixed_size, moving_vox2ras, 0, M, nullptr));
        RC(fibd_vol_xform(M, d_moving.p + nvm * f, moving_size[0], moving_size[1], moving_size[2], 1, FIB_VOL_TRILINEAR, 0, d_out.p + nvf * f,
                          fixed_size[0], fixed_size[1], fixed_size[2], nullptr));
    }
    RC(d2h(resampled, d_out.p, sizeof(float) * nvf * nframes));
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// non-linear registration: the host forms.  One device; both volumes, the workspace of fibd_nlreg_run and the field stay on the device
// for the call, the planar field and the warped volume come back at its end.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_mri_nlreg(int device, const float *moving, const int32_t moving_size[3], const float moving_vox2ras[16], const float *fixed,
                             const int32_t fixed_size[3], const float fixed_vox2ras[16], const float *post, int levels, const int32_t *niter,
                             float sigma, float step, float *disp, double *cost, int64_t *count, const float *warp_mats, float *warped) try {
    FIB_CHECK(moving && moving_size && moving_vox2ras && fixed && fixed_size && fixed_vox2ras && niter && disp, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(!warped || warp_mats, FIB_ERR_INVALID, "the warped volume needs its three matrices");
    size_t work_bytes = 0;
    RC(fibd_nlreg_work_size(fixed_size, moving_size, levels, niter, &work_bytes));     // (sizes, levels and niter are refused here)
    FIB_CHECK(sigma >= 0.f && sigma <= 4.f, FIB_ERR_INVALID, "sigma %g outside [0, 4]", (double)sigma);
    float m[16 + 16 + 9 + 1];
    for (int l = 0; l < levels; l++) RC(fib_nlreg_level(fixed_vox2ras, moving_vox2ras, post, l, step, m, m + 16, m + 32, m + 41));
    DevLease lease;
    RC(lease.take(device, "mri_nlreg runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvf = (size_t)fixed_size[0] * fixed_size[1] * fixed_size[2], nvm = (size_t)moving_size[0] * moving_size[1] * moving_size[2];
    fib::DevBuf<float> d_fixed, d_moving, d_field, d_out;
    fib::DevBuf<char> d_work;
    RC(fib::upload(d_fixed, fixed, nvf));
    RC(fib::upload(d_moving, moving, nvm));
    RC(d_field.alloc(4 * nvf));
    RC(d_out.alloc(3 * nvf));
    RC(d_work.alloc(work_bytes));
    RC(fibd_nlreg_run(d_fixed.p, fixed_size, fixed_vox2ras, d_moving.p, moving_size, moving_vox2ras, post, levels, niter, sigma, step, d_field.p, cost,
                      count, d_work.p, work_bytes, nullptr));
    RC(fibd_warp_unpack(d_field.p, fixed_size[0], fixed_size[1], fixed_size[2], d_out.p, nullptr));
    RC(d2h(disp, d_out.p, sizeof(float) * 3 * nvf));
    if (!warped) return FIB_OK;
    RC(fibd_warp_volume(d_field.p, fixed_size[0], fixed_size[1], fixed_size[2], warp_mats, warp_mats + 16, warp_mats + 32, d_moving.p, moving_size[0],
                        moving_size[1], moving_size[2], 1, FIB_VOL_TRILINEAR, 0, d_out.p, fixed_size[0], fixed_size[1], fixed_size[2], nullptr));
    RC(d2h(warped, d_out.p, sizeof(float) * nvf));
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_warp_jacobian(int device, const float *disp, int nx, int ny, int nz, const float linv[9], float *out) try {
    FIB_CHECK(disp && linv && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "the field's dimensions must be positive");
    DevLease lease;
    RC(lease.take(device, "warp_jacobian runs on one device (FIB_DEVICE_ALL is not supported)"));
    const size_t nvox = (size_t)nx * ny * nz;
    fib::DevBuf<float> d_field, d_out;
    RC(warp_field_upload(disp, nx, ny, nz, d_field));
    RC(d_out.alloc(nvox));
    RC(fibd_warp_jacobian(d_field.p, nx, ny, nz, linv, d_out.p, nullptr));
    RC(d2h(out, d_out.p, sizeof(float) * nvox));
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// tract maps: host forms.  One device; the points travel in chunks cut at line boundaries, the volume stays on the device.
// ------------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t TM_CHUNK_POINTS = (int64_t)1 << 22;      // 48 MB of points per chunk (a longer line is a chunk of its own)

// npts >= 0 and sum(npts) == npoints, before anything is written
int tm_host_check(const int32_t *npts, int64_t nlines, int64_t npoints) {
    FIB_CHECK(nlines >= 0 && npoints >= 0, FIB_ERR_INVALID, "nlines and npoints must not be negative");
    FIB_CHECK(nlines == 0 || npts, FIB_ERR_INVALID, "NULL npts");
    int64_t sum = 0;
    for (int64_t l = 0; l < nlines; l++) {
        FIB_CHECK(npts[l] >= 0, FIB_ERR_INVALID, "line %lld has a negative point count", (long long)l);
        sum += npts[l];
    }
    FIB_CHECK(sum == npoints, FIB_ERR_INVALID, "the point counts sum to %lld, not to npoints = %lld", (long long)sum, (long long)npoints);
    return FIB_OK;
}

// One call of a tractogram host form on its worker: a DevLease, and the worker's buffer set, b.  (init: the forms use nothing it makes,
// but DevState::trim releases the set only on a worker that is ready.)
struct TmLease : DevLease {
    DevState::TractMapBufs *b = nullptr;
    int take(int device) {
        RC(DevLease::take(device, "the tract maps, the selection and the connectome run on one device (FIB_DEVICE_ALL is not supported)"));
        RC(wk->init(copy_threads(1)));
        if (!wk->tm) wk->tm.reset(new DevState::TractMapBufs());
        b = wk->tm.get();
        return FIB_OK;
    }
};

// The lines of a call in chunks (fibh::next_line_chunk: at most TM_CHUNK_POINTS points and max_lines lines each).  Per chunk: the work
// area work_size asks for, npts and xyz of the chunk on the device (b.work, b.npts, b.xyz), then body(l0, nl, p0, np, work bytes) for
// lines [l0, l0 + nl) = points [p0, p0 + np).  Copies block on the NULL stream, so a body's read-back comes behind its kernels.
template <typename Body>
int tm_walk_lines(DevState::TractMapBufs &b, const float *xyz, const int32_t *npts, int64_t nlines, int (*work_size)(int64_t, size_t *),
                  int64_t max_lines, Body body) {
    int64_t p0 = 0;
    for (int64_t l0 = 0; l0 < nlines;) {
        const fibh::LineChunk c = fibh::next_line_chunk(npts, nlines, l0, TM_CHUNK_POINTS, max_lines);
        const int64_t nl = c.l1 - l0, np = c.np;
        size_t wb = 0;
        RC(work_size(nl, &wb));
        RC(b.work.ensure(wb));
        RC(b.npts.ensure((size_t)nl));
        RC(b.xyz.ensure((size_t)3 * np));
        RC(h2d(b.npts.p, npts + l0, sizeof(int32_t) * (size_t)nl));
        if (np) RC(h2d(b.xyz.p, xyz + 3 * p0, sizeof(float) * 3 * (size_t)np));
        RC(body(l0, nl, p0, np, wb));
        p0 += np; l0 = c.l1;
    }
    return FIB_OK;
}
}  // namespace

extern "C" int fib_str_density(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                               int mode, uint32_t *density, int64_t *n_outside) try {
    FIB_CHECK(density && n_outside, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    const int what = mode & ~FIB_DENSITY_ACCUMULATE;
    FIB_CHECK(what >= FIB_DENSITY_POINTS && what <= FIB_DENSITY_ENDPOINTS, FIB_ERR_INVALID, "unknown density mode %d", mode);
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const size_t nvox = (size_t)nx * ny * nz;
    RC(b.dens.ensure(nvox));
    RC(b.nout.ensure(1));
    if (mode & FIB_DENSITY_ACCUMULATE) RC(h2d(b.dens.p, density, sizeof(uint32_t) * nvox));
    else FIB_HIP(hipMemset(b.dens.p, 0, sizeof(uint32_t) * nvox));
    int64_t total_out = 0;
    RC(tm_walk_lines(b, xyz, npts, nlines, fibd_str_work_size, fibh::LINES_UNBOUNDED, [&](int64_t, int64_t nl, int64_t, int64_t np, size_t wb) -> int {
        RC(fibd_str_density(b.xyz.p, b.npts.p, nl, np, nx, ny, nz, what | FIB_DENSITY_ACCUMULATE, b.dens.p, b.nout.p, b.work.p, wb, nullptr));
        int64_t out = 0;
        RC(d2h(&out, b.nout.p, sizeof out));
        FIB_CHECK(out >= 0, FIB_ERR_INVALID, "internal error: the device refused a chunk the host accepted");
        total_out += out;
        return FIB_OK;
    }));
    RC(d2h(density, b.dens.p, sizeof(uint32_t) * nvox));
    *n_outside = total_out;
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_str_sample(int device, const float *xyz, int64_t npoints, const float *vol, int nx, int ny, int nz, int nframes, float outside,
                              float *scalars) try {
    FIB_CHECK(npoints >= 0, FIB_ERR_INVALID, "npoints must not be negative");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0 && nframes > 0, FIB_ERR_INVALID, "volume dimensions and nframes must be positive");
    FIB_CHECK(npoints == 0 || (xyz && vol && scalars), FIB_ERR_INVALID, "NULL argument");
    TmLease lease;
    RC(lease.take(device));                                // (no points: FIB_DEVICE_ALL and an unknown device are refused all the same)
    if (npoints == 0) return FIB_OK;
    auto &b = *lease.b;
    const size_t nvox = (size_t)nx * ny * nz;
    RC(b.vol.ensure(nvox * nframes));
    RC(h2d(b.vol.p, vol, sizeof(float) * nvox * nframes));
    const int64_t chunk = std::max<int64_t>(1, TM_CHUNK_POINTS / std::max(1, nframes / 3));
    RC(b.xyz.ensure((size_t)3 * std::min(chunk, npoints)));
    RC(b.scal.ensure((size_t)nframes * std::min(chunk, npoints)));
    for (int64_t p0 = 0; p0 < npoints; p0 += chunk) {
        const int64_t np = std::min(chunk, npoints - p0);
        RC(h2d(b.xyz.p, xyz + 3 * p0, sizeof(float) * 3 * (size_t)np));
        RC(fibd_str_sample(b.xyz.p, np, b.vol.p, nx, ny, nz, nframes, outside, b.scal.p, nullptr));
        RC(d2h(scalars + p0 * nframes, b.scal.p, sizeof(float) * (size_t)nframes * np));
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_str_stats(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3],
                             const float *scalars, int nscalars, float *props) try {
    FIB_CHECK(volres, FIB_ERR_INVALID, "NULL volres");
    FIB_CHECK(nscalars >= 0, FIB_ERR_INVALID, "nscalars must not be negative");
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || (xyz && (nscalars == 0 || scalars)), FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nlines == 0 || props, FIB_ERR_INVALID, "NULL props");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const int ncol = 1 + nscalars;
    return tm_walk_lines(b, xyz, npts, nlines, fibd_str_work_size, fibh::LINES_UNBOUNDED, [&](int64_t l0, int64_t nl, int64_t p0, int64_t np, size_t wb) -> int {
        RC(b.scal.ensure((size_t)nscalars * np));
        RC(b.props.ensure((size_t)ncol * nl));
        if (np && nscalars) RC(h2d(b.scal.p, scalars + p0 * nscalars, sizeof(float) * (size_t)nscalars * np));
        RC(fibd_str_stats(b.xyz.p, b.npts.p, nl, np, volres, b.scal.p, nscalars, b.props.p, b.work.p, wb, nullptr));
        return d2h(props + l0 * ncol, b.props.p, sizeof(float) * (size_t)ncol * nl);
    });
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// tract selection and connectome: host forms.  One device; the points travel in chunks cut at line boundaries, the ROI bit volume /
// the label volume and C, W stay on the device.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_str_select(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                              const uint8_t *const *rois, int nroi, uint64_t visit_all, uint64_t visit_none, uint64_t end_any, uint64_t end_both,
                              int32_t min_npts, int32_t max_npts, uint8_t *keep, uint32_t *hits, int64_t *counts) try {
    FIB_CHECK(nroi >= 0 && nroi <= 32, FIB_ERR_INVALID, "fib_str_select takes 0 to 32 ROIs (one bit each of a 32-bit word), not %d", nroi);
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(counts && (nlines <= 0 || keep) && (nroi == 0 || rois), FIB_ERR_INVALID, "NULL argument");
    for (int r = 0; r < nroi; r++) FIB_CHECK(rois[r], FIB_ERR_INVALID, "ROI %d is NULL", r);
    const uint64_t used = visit_all | visit_none | end_any | end_both;
    FIB_CHECK((used >> 32) == 0 && (nroi == 32 || (used >> nroi) == 0), FIB_ERR_INVALID, "a mask names an ROI beyond the %d given", nroi);
    FIB_CHECK(min_npts >= 0 && max_npts >= 0, FIB_ERR_INVALID, "min_npts and max_npts must not be negative");
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const size_t nvox = (size_t)nx * ny * nz;
    RC(b.nout.ensure(3));
    if (nroi) {
        RC(b.rois.ensure(nvox * nroi));
        RC(b.roibits.ensure(nvox));
        for (int r = 0; r < nroi; r++) RC(h2d(b.rois.p + nvox * r, rois[r], nvox));
        RC(fibd_str_roi_pack(b.rois.p, nroi, (int64_t)nvox, b.roibits.p, nullptr));
    }
    int64_t total[2] = {0, 0};
    RC(tm_walk_lines(b, xyz, npts, nlines, fibd_str_select_work_size, fibh::LINES_UNBOUNDED, [&](int64_t l0, int64_t nl, int64_t, int64_t np, size_t wb) -> int {
        RC(b.keep.ensure((size_t)nl));
        if (hits) RC(b.hits.ensure((size_t)3 * nl));
        RC(fibd_str_select(b.xyz.p, b.npts.p, nl, np, nx, ny, nz, nroi ? b.roibits.p : nullptr, visit_all, visit_none, end_any, end_both, min_npts,
                           max_npts, b.keep.p, hits ? b.hits.p : nullptr, b.nout.p, b.work.p, wb, nullptr));
        int64_t got[2] = {0, 0};
        RC(d2h(got, b.nout.p, sizeof got));
        FIB_CHECK(got[0] >= 0, FIB_ERR_INVALID, "internal error: the device refused a chunk the host accepted");
        RC(d2h(keep + l0, b.keep.p, (size_t)nl));
        if (hits) RC(d2h(hits + 3 * l0, b.hits.p, sizeof(uint32_t) * 3 * (size_t)nl));
        total[0] += got[0]; total[1] += got[1];
        return FIB_OK;
    }));
    counts[0] = total[0]; counts[1] = total[1];
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_str_connectome(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                                  const float volres[3], const int32_t *labels, const int32_t *remap, int64_t nremap, int nnodes, int flags,
                                  uint32_t *cmat, double *wmat, int32_t *assign, int64_t *n_lines) try {
    FIB_CHECK((flags & ~FIB_CONNECTOME_ACCUMULATE) == 0, FIB_ERR_INVALID, "unknown connectome flags 0x%x", flags);
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nnodes >= 1 && nnodes < (1 << 24), FIB_ERR_INVALID, "the number of nodes must be between 1 and 2^24 - 1");
    FIB_CHECK(labels && cmat && n_lines, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(!wmat || volres, FIB_ERR_INVALID, "the lengths of W need volres");
    FIB_CHECK(nremap >= 0 && (nremap == 0 || remap), FIB_ERR_INVALID, "nremap entries need a remap array");
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const size_t nvox = (size_t)nx * ny * nz, cells = (size_t)(nnodes + 1) * (size_t)(nnodes + 1);
    RC(b.nout.ensure(3));
    RC(b.labels.ensure(nvox));
    RC(h2d(b.labels.p, labels, sizeof(int32_t) * nvox));
    if (nremap) { RC(b.remap.ensure((size_t)nremap)); RC(h2d(b.remap.p, remap, sizeof(int32_t) * (size_t)nremap)); }
    RC(b.cmat.ensure(cells));
    if (wmat) RC(b.wmat.ensure(cells));
    if (flags & FIB_CONNECTOME_ACCUMULATE) {
        RC(h2d(b.cmat.p, cmat, sizeof(uint32_t) * cells));
        if (wmat) RC(h2d(b.wmat.p, wmat, sizeof(double) * cells));
    } else {
        FIB_HIP(hipMemset(b.cmat.p, 0, sizeof(uint32_t) * cells));
        if (wmat) FIB_HIP(hipMemset(b.wmat.p, 0, sizeof(double) * cells));
    }
    int64_t total = 0;
    RC(tm_walk_lines(b, xyz, npts, nlines, fibd_str_select_work_size, fibh::LINES_UNBOUNDED, [&](int64_t l0, int64_t nl, int64_t, int64_t np, size_t wb) -> int {
        if (assign) RC(b.assign.ensure((size_t)2 * nl));
        RC(fibd_str_connectome(b.xyz.p, b.npts.p, nl, np, nx, ny, nz, volres, b.labels.p, nremap ? b.remap.p : nullptr, nremap, nnodes,
                               FIB_CONNECTOME_ACCUMULATE, b.cmat.p, wmat ? b.wmat.p : nullptr, assign ? b.assign.p : nullptr, b.nout.p, b.work.p, wb,
                               nullptr));
        int64_t got = 0;
        RC(d2h(&got, b.nout.p, sizeof got));
        FIB_CHECK(got >= 0, FIB_ERR_INVALID, "internal error: the device refused a chunk the host accepted");
        if (assign) RC(d2h(assign + 2 * l0, b.assign.p, sizeof(int32_t) * 2 * (size_t)nl));
        total += got;
        return FIB_OK;
    }));
    RC(d2h(cmat, b.cmat.p, sizeof(uint32_t) * cells));
    if (wmat) RC(d2h(wmat, b.wmat.p, sizeof(double) * cells));
    *n_lines = total;
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// tractogram weights: host form.  One device; the points go up once, in chunks cut at line boundaries, only to make the fixel ids; the
// ids, q, TDq and the field stay resident for the iterations.  FIBERS_FIXEL_POINTS=<n> overrides the points per chunk.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_str_weights(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, int nx, int ny, int nz,
                               int32_t nvec, const float *const *ovec, const float *const *f, const uint8_t *mask, float f_thresh, float cos2,
                               int niter, const uint32_t *q0, uint32_t *q, float *weights, float *td, double *mu, double *cost, int64_t *counts) try {
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nvec >= 1 && nvec <= 3, FIB_ERR_INVALID, "nvec must be 1, 2 or 3, not %d", nvec);
    FIB_CHECK(niter >= 0, FIB_ERR_INVALID, "niter must not be negative");
    FIB_CHECK(f_thresh >= 0.0f, FIB_ERR_INVALID, "f_thresh must not be negative (amplitudes are positive)");
    FIB_CHECK(ovec && f && td && mu && cost && counts && (nlines <= 0 || (q && weights)), FIB_ERR_INVALID, "NULL argument");
    for (int k = 0; k < nvec; k++) FIB_CHECK(ovec[k] && f[k], FIB_ERR_INVALID, "peak %d is NULL", k);
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    const size_t nvox = (size_t)nx * ny * nz, nfix = nvox * nvec;
    FIB_CHECK(nfix < ((size_t)1 << 31) && npoints < ((int64_t)1 << 31), FIB_ERR_UNSUPPORTED, "the weights take fewer than 2^31 fixels and points");
    int64_t chunk = TM_CHUNK_POINTS;
    if (const char *e = fib::env("FIBERS_FIXEL_POINTS")) { const long long v = atoll(e); if (v > 0) chunk = v; }
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    RC(b.fx_vec.ensure(3 * nfix)); RC(b.fx_f.ensure(nfix)); RC(b.fx_aq.ensure(nfix)); RC(b.fx_tdq.ensure(nfix)); RC(b.fx_td.ensure(nfix));
    RC(b.fx_npts.ensure((size_t)nlines)); RC(b.fx_nline.ensure((size_t)nlines)); RC(b.fx_q.ensure((size_t)nlines)); RC(b.fx_w.ensure((size_t)nlines));
    RC(b.fx_ids.ensure((size_t)npoints)); RC(b.fx_cost.ensure((size_t)niter + 1)); RC(b.fx_state.ensure(FIB_FIXEL_STATE_SLOTS));
    const float *d_ovec[3] = {nullptr, nullptr, nullptr}, *d_f[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < nvec; k++) {
        d_ovec[k] = b.fx_vec.p + 3 * nvox * k; d_f[k] = b.fx_f.p + nvox * k;
        RC(h2d(b.fx_vec.p + 3 * nvox * k, ovec[k], sizeof(float) * 3 * nvox));
        RC(h2d(b.fx_f.p + nvox * k, f[k], sizeof(float) * nvox));
    }
    if (mask) { RC(b.fx_mask.ensure(nvox)); RC(h2d(b.fx_mask.p, mask, nvox)); }
    const uint8_t *d_mask = mask ? b.fx_mask.p : nullptr;
    RC(fibd_fixel_quantise(nvec, (int64_t)nvox, d_ovec, d_f, d_mask, f_thresh, b.fx_aq.p, b.fx_state.p, nullptr));
    int64_t total[2] = {0, 0}, p0 = 0;
    for (int64_t l0 = 0; l0 < nlines;) {
        const fibh::LineChunk c = fibh::next_line_chunk(npts, nlines, l0, chunk, fibh::LINES_UNBOUNDED);
        const int64_t nl = c.l1 - l0, np = c.np;
        size_t wb = 0;
        RC(fibd_str_work_size(nl, &wb));
        RC(b.work.ensure(wb)); RC(b.npts.ensure((size_t)nl)); RC(b.xyz.ensure((size_t)3 * np)); RC(b.nout.ensure(3));
        RC(h2d(b.npts.p, npts + l0, sizeof(int32_t) * (size_t)nl));
        if (np) RC(h2d(b.xyz.p, xyz + 3 * p0, sizeof(float) * 3 * (size_t)np));
        RC(fibd_fixel_assign(b.xyz.p, b.npts.p, nl, np, nx, ny, nz, nvec, d_ovec, d_f, d_mask, f_thresh, cos2, b.fx_ids.p + p0, b.nout.p, b.work.p, wb,
                             nullptr));
        int64_t got[2] = {0, 0};
        RC(d2h(got, b.nout.p, sizeof got));
        FIB_CHECK(got[0] >= 0, FIB_ERR_INVALID, "internal error: the device refused a chunk the host accepted");
        total[0] += got[0]; total[1] += got[1];
        p0 += np; l0 = c.l1;
    }
    RC(h2d(b.fx_state.p + 5, total, sizeof total));
    std::vector<uint32_t> start(q0 ? q0 : nullptr, q0 ? q0 + nlines : nullptr);
    if (!q0) start.assign((size_t)nlines, 1u << 20);
    if (nlines) { RC(h2d(b.fx_q.p, start.data(), sizeof(uint32_t) * (size_t)nlines)); RC(h2d(b.fx_npts.p, npts, sizeof(int32_t) * (size_t)nlines)); }
    size_t wb = 0;
    RC(fibd_fixel_fit_work_size(nlines, &wb));
    RC(b.work.ensure(wb));
    RC(fibd_fixel_fit(b.fx_ids.p, b.fx_npts.p, nlines, npoints, b.fx_aq.p, (int64_t)nfix, niter, b.fx_q.p, b.fx_w.p, b.fx_td.p, b.fx_cost.p, b.fx_state.p,
                      b.fx_tdq.p, b.fx_nline.p, b.work.p, wb, nullptr));
    int64_t state[FIB_FIXEL_STATE_SLOTS];
    RC(d2h(state, b.fx_state.p, sizeof state));
    if (nlines) { RC(d2h(q, b.fx_q.p, sizeof(uint32_t) * (size_t)nlines)); RC(d2h(weights, b.fx_w.p, sizeof(float) * (size_t)nlines)); }
    RC(d2h(td, b.fx_td.p, sizeof(float) * nfix));
    RC(d2h(cost, b.fx_cost.p, sizeof(double) * ((size_t)niter + 1)));
    memcpy(mu, &state[1], sizeof(double));
    for (int i = 0; i < 5; i++) counts[i] = state[5 + i];
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// bundle tools: host forms.  One device; the lines travel in chunks, the models and sums / counts stay on the device.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_str_resample(int device, const float *xyz, const int32_t *npts, int64_t nlines, int64_t npoints, const float volres[3], int K,
                                const uint8_t *flip, float *out) try {
    FIB_CHECK(K >= 2 && K <= 256, FIB_ERR_UNSUPPORTED, "fib_str_resample gives 2 to 256 points per line, not %d", K);
    FIB_CHECK(volres, FIB_ERR_INVALID, "NULL volres");
    RC(tm_host_check(npts, nlines, npoints));
    FIB_CHECK(npoints == 0 || xyz, FIB_ERR_INVALID, "NULL xyz");
    FIB_CHECK(nlines == 0 || out, FIB_ERR_INVALID, "NULL out");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    RC(b.nout.ensure(3));
    const int64_t max_lines = std::max<int64_t>(1, TM_CHUNK_POINTS / K);       // the output of a chunk is no larger than its largest input
    return tm_walk_lines(b, xyz, npts, nlines, fibd_str_work_size, max_lines, [&](int64_t l0, int64_t nl, int64_t, int64_t np, size_t wb) -> int {
        RC(b.lines.ensure((size_t)3 * K * nl));
        if (flip) { RC(b.flip.ensure((size_t)nl)); RC(h2d(b.flip.p, flip + l0, (size_t)nl)); }
        RC(fibd_str_resample(b.xyz.p, b.npts.p, nl, np, volres, K, flip ? b.flip.p : nullptr, b.lines.p, b.nout.p, b.work.p, wb, nullptr));
        int64_t got = 0;
        RC(d2h(&got, b.nout.p, sizeof got));
        FIB_CHECK(got == nl, FIB_ERR_INVALID, "internal error: the device refused a chunk the host accepted");
        return d2h(out + (size_t)3 * K * l0, b.lines.p, sizeof(float) * 3 * K * (size_t)nl);
    });
} FIB_API_CATCH

extern "C" int fib_str_assign(int device, const float *lines, int64_t nlines, int K, const float *models, int nmodels, const float volres[3],
                              float thresh_mm, int32_t *label, float *dist, uint8_t *flip, float *dist_all) try {
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    FIB_CHECK(K >= 1 && K <= 256, FIB_ERR_UNSUPPORTED, "lines of 1 to 256 points each, not %d", K);
    FIB_CHECK(nmodels >= 1 && nmodels < (1 << 24), FIB_ERR_INVALID, "the number of models must be between 1 and 2^24 - 1");
    FIB_CHECK(models && volres && (nlines == 0 || (lines && label && dist && flip)), FIB_ERR_INVALID, "NULL argument");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const size_t row = (size_t)3 * K;
    RC(b.models.ensure(row * nmodels));
    RC(h2d(b.models.p, models, sizeof(float) * row * nmodels));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(TM_CHUNK_POINTS / K, dist_all ? ((int64_t)1 << 26) / nmodels : nlines));
    for (int64_t l0 = 0; l0 < nlines; l0 += chunk) {
        const size_t nl = (size_t)std::min(chunk, nlines - l0);
        RC(b.lines.ensure(row * nl));
        RC(b.label.ensure(nl));
        RC(b.dist.ensure(nl));
        RC(b.flip.ensure(nl));
        if (dist_all) RC(b.dall.ensure(nl * nmodels));
        RC(h2d(b.lines.p, lines + row * l0, sizeof(float) * row * nl));
        RC(fibd_str_assign(b.lines.p, (int64_t)nl, K, b.models.p, nmodels, volres, thresh_mm, b.label.p, b.dist.p, b.flip.p, dist_all ? b.dall.p : nullptr,
                           nullptr));
        RC(d2h(label + l0, b.label.p, sizeof(int32_t) * nl));
        RC(d2h(dist + l0, b.dist.p, sizeof(float) * nl));
        RC(d2h(flip + l0, b.flip.p, nl));
        if (dist_all) RC(d2h(dist_all + (size_t)l0 * nmodels, b.dall.p, sizeof(float) * nl * nmodels));
    }
    return FIB_OK;
} FIB_API_CATCH

extern "C" int fib_str_centroids(int device, const float *lines, int64_t nlines, int K, const int32_t *label, const uint8_t *flip, int nmodels,
                                 int flags, double *sums, uint32_t *counts) try {
    FIB_CHECK((flags & ~FIB_CENTROIDS_ACCUMULATE) == 0, FIB_ERR_INVALID, "unknown centroid flags 0x%x", flags);
    FIB_CHECK(nlines >= 0, FIB_ERR_INVALID, "nlines must not be negative");
    FIB_CHECK(K >= 1 && K <= 256, FIB_ERR_UNSUPPORTED, "lines of 1 to 256 points each, not %d", K);
    FIB_CHECK(nmodels >= 1 && nmodels < (1 << 24), FIB_ERR_INVALID, "the number of models must be between 1 and 2^24 - 1");
    FIB_CHECK(sums && counts && (nlines == 0 || (lines && label)), FIB_ERR_INVALID, "NULL argument");
    TmLease lease;
    RC(lease.take(device));
    auto &b = *lease.b;
    const size_t row = (size_t)3 * K, cells = row * nmodels;
    RC(b.sums.ensure(cells));
    RC(b.bcnt.ensure((size_t)nmodels));
    if (flags & FIB_CENTROIDS_ACCUMULATE) {
        RC(h2d(b.sums.p, sums, sizeof(double) * cells));
        RC(h2d(b.bcnt.p, counts, sizeof(uint32_t) * (size_t)nmodels));
    } else {
        FIB_HIP(hipMemset(b.sums.p, 0, sizeof(double) * cells));
        FIB_HIP(hipMemset(b.bcnt.p, 0, sizeof(uint32_t) * (size_t)nmodels));
    }
    const int64_t chunk = std::max<int64_t>(1, TM_CHUNK_POINTS / K);
    for (int64_t l0 = 0; l0 < nlines; l0 += chunk) {
        const size_t nl = (size_t)std::min(chunk, nlines - l0);
        RC(b.lines.ensure(row * nl));
        RC(b.label.ensure(nl));
        if (flip) RC(b.flip.ensure(nl));
        RC(h2d(b.lines.p, lines + row * l0, sizeof(float) * row * nl));
        RC(h2d(b.label.p, label + l0, sizeof(int32_t) * nl));
        if (flip) RC(h2d(b.flip.p, flip + l0, nl));
        RC(fibd_str_centroids(b.lines.p, (int64_t)nl, K, b.label.p, flip ? b.flip.p : nullptr, nmodels, FIB_CENTROIDS_ACCUMULATE, b.sums.p, b.bcnt.p,
                              nullptr));
        FIB_HIP(hipStreamSynchronize(nullptr));                // (the chunk's buffers are written again)
    }
    RC(d2h(sums, b.sums.p, sizeof(double) * cells));
    RC(d2h(counts, b.bcnt.p, sizeof(uint32_t) * (size_t)nmodels));
    return FIB_OK;
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// gqi_rec / dsi_rec
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

struct OdfSpec {                                        // what identifies a GQIwork / DSIwork
    bool dsi; const float *bval, *bvec; int nvol; const float *verts; int nverts; const int32_t *faces; int nfaces; float sigma; int hann_width;
};
int odf_plan_for(DevState &d, const OdfSpec &s, fib_odf_plan **plan) {
    std::string key;
    key.push_back(s.dsi ? 'D' : 'G');
    key_add(key, s.bval, sizeof(float) * s.nvol);
    key_add(key, s.bvec, sizeof(float) * 3 * s.nvol);
    key_add(key, s.verts, sizeof(float) * 3 * s.nverts);
    key_add(key, s.faces, sizeof(int32_t) * 3 * s.nfaces);
    key_add(key, s.dsi ? (const void *)&s.hann_width : (const void *)&s.sigma, 4);
    const int fmt = fib_odf_default_format();            // the operand format is part of a plan's identity (it may change with the environment)
    key_add(key, &fmt, sizeof(fmt));
    return cached_plan<fib_odf_plan, fib_odf_plan_destroy>(d, key, [&](fib_odf_plan **q) {
        return s.dsi ? fib_dsi_plan_create_fmt(d.device, s.bval, s.bvec, s.nvol, s.verts, s.nverts, s.faces, s.nfaces, s.hann_width, fmt, q)
                     : fib_gqi_plan_create_fmt(d.device, s.bval, s.bvec, s.nvol, s.verts, s.nverts, s.faces, s.nfaces, s.sigma, fmt, q);
    }, plan);
}

int odf_rec_host(int device, const OdfSpec &spec, const float *dwi, int nx, int ny, int nz, const void *mask, int mask_dtype,
                 float *pdf, float *odf, float *const peak[3], float *const qa[3]) {
    FitCall c;
    RC(fit_call(c, device, spec.bval, spec.nvol, spec.bvec != nullptr, dwi && mask && odf && peak && qa, nx, ny, nz, mask_dtype,
                peak && qa && peak[0] && qa[0] && peak[1] && qa[1] && peak[2] && qa[2], "NULL peak/qa output volume",
                spec.verts && spec.faces && spec.nverts >= 2 && spec.nverts % 2 == 0 && spec.nfaces > 0));
    mask_dtype = c.mask_dtype;
    const bool zeroed = c.zeroed;                        // (the qa planes below are written in full either way: their outside value can be NaN)
    const int64_t nvox = c.nvox;
    const int nvol = spec.nvol, nvert = spec.nverts / 2;
    const std::vector<Worker> &ws = c.ws;
    const int nw = (int)ws.size();
    const std::vector<Rows> ins = {{dwi, nullptr, nvol}};
    std::vector<Rows> outs;
    if (pdf) outs.push_back({nullptr, pdf, nvol});
    outs.push_back({nullptr, odf, nvert});
    for (int k = 0; k < 3; k++) outs.push_back({nullptr, peak[k], 3});
    const int rows_out = (pdf ? nvol : 0) + nvert + 9;
    // per worker: qa of its slab stays on the device until the global odfmax is known; one {max, NaN flag} pair per chunk
    // (the buffer belongs to the CALL, not to the worker: the worker's lock is released between the two passes below, and another
    // thread's call on the same worker must not find -- or reallocate -- this call's qa)
    struct Slab { int64_t v0 = 0, v1 = 0, nq = 0; float *qa = nullptr; std::vector<float> maxes; fib::DevBuf<float> keep; LiveMap lm; const LiveMap *use = nullptr; };
    std::vector<Slab> slabs((size_t)nw);
    RC(for_each_worker(ws, [&](int i, DevState &d) -> int {
        Slab &sl = slabs[i];
        slab(nvox, nw, i, sl.v0, sl.v1);
        const int64_t nr = sl.v1 - sl.v0;
        if (nr <= 0) return FIB_OK;
        fib_odf_plan *plan = nullptr;
        RC(odf_plan_for(d, spec, &plan));
        RC(live_map_for(d, mask, mask_dtype, sl.v0, sl.v1, sl.lm, &sl.use));
        const int64_t ntr = sl.use ? sl.use->nlive : nr;        // voxels that travel
        const int64_t chunk = pick_chunk(ntr, nvol, rows_out);
        const int nchunks = chunk_count(ntr, chunk);
        sl.nq = (ntr + 31) / 32 * 32 + 32;                      // a plane of the qa kept on the device (a packed chunk is padded to 32 voxels)
        FIB_HIP(hipSetDevice(d.device));
        RC(sl.keep.alloc((size_t)3 * sl.nq + (size_t)2 * std::max(nchunks, 1)));
        sl.qa = sl.keep.p;
        float *dmax = sl.qa + 3 * sl.nq;
        const int64_t nq = sl.nq;
        RC(run_chunks(d, sl.v0, sl.v1, nvox, ins, mask, mask_dtype, outs, chunk,
                      [&](int k, int64_t rel, int64_t n, const float *din, const uint8_t *dm, float *b, hipStream_t st) -> int {
                          float *dpdf = pdf ? b : nullptr, *dodf = b + (size_t)(pdf ? nvol : 0) * n, *dpk = dodf + (size_t)nvert * n;
                          float *pk[3] = {dpk, dpk + 3 * n, dpk + 6 * n};
                          float *q[3] = {sl.qa + rel, sl.qa + nq + rel, sl.qa + 2 * nq + rel};
                          // (one volume in pieces: the same peak-finder form for every piece, whatever the cut -- see FIB_ODF_SEPARATE_PEAKS)
                          return fibd_odf_rec(plan, din, dm, n, dpdf, dodf, pk, q, dmax + 2 * k, nvox % 4 != 0 ? FIB_ODF_SEPARATE_PEAKS : 0, st);
                      }, sl.use, zeroed));
        sl.maxes.resize((size_t)2 * nchunks);
        if (nchunks > 0) RC(d2h(sl.maxes.data(), dmax, sl.maxes.size() * sizeof(float)));
        return FIB_OK;
    }));
    // odfmax = maximum(mean(odf, dims=4)) over the whole volume (gqi.jl:164, dsi.jl:263); maximum() propagates NaN
    float odfmax = -INFINITY;
    bool anynan = false;
    for (auto &sl : slabs)
        for (size_t c = 0; c + 1 < sl.maxes.size(); c += 2) {
            if (sl.maxes[c + 1] != 0.0f || sl.maxes[c] != sl.maxes[c]) anynan = true;
            else if (sl.maxes[c] > odfmax) odfmax = sl.maxes[c];
        }
    // (a packed slab leaves voxels out: their ODF is 0 and so is their mean -- the unpacked pipeline's kernels count it the same way)
    for (auto &sl : slabs) if (sl.use && sl.use->nlive < sl.v1 - sl.v0 && 0.0f > odfmax) odfmax = 0.0f;
    if (anynan) odfmax = __builtin_nanf("");
    const float qa_outside = 0.0f / odfmax;              // qa of a voxel outside the mask after `qa ./= odfmax`: 0, or NaN when odfmax is 0 / NaN
    // qa[k] ./= odfmax (gqi.jl:166-168) on every device, then out
    return for_each_worker(ws, [&](int i, DevState &d) -> int {
        Slab &sl = slabs[i];
        const int64_t nr = sl.v1 - sl.v0;
        if (nr <= 0) return FIB_OK;
        FIB_HIP(hipSetDevice(d.device));
        float *q[3] = {sl.qa, sl.qa + sl.nq, sl.qa + 2 * sl.nq};
        const int64_t ntr = sl.use ? sl.use->nlive : nr;
        if (ntr > 0) RC(fibd_qa_normalize(q, ntr, odfmax, d.s_cmp));
        if (!sl.use) {
            for (int k = 0; k < 3; k++) FIB_HIP(hipMemcpyAsync(qa[k] + sl.v0, q[k], (size_t)nr * sizeof(float), hipMemcpyDeviceToHost, d.s_cmp));
            FIB_HIP(hipStreamSynchronize(d.s_cmp));
            return FIB_OK;
        }
        // packed: the three planes come back dense and go to their runs; the gaps read 0
        std::vector<float> hq((size_t)3 * std::max<int64_t>(ntr, 1));
        for (int k = 0; k < 3 && ntr > 0; k++) FIB_HIP(hipMemcpyAsync(hq.data() + (size_t)k * ntr, q[k], (size_t)ntr * sizeof(float), hipMemcpyDeviceToHost, d.s_cmp));
        FIB_HIP(hipStreamSynchronize(d.s_cmp));
        const LiveMap &lm = *sl.use;
        d.pool->run(3, [&](int k) {
            float *row = qa[k];
            const float *src = hq.data() + (size_t)k * ntr;
            int64_t g0 = lm.vbeg;
            for (size_t r = 0; r < lm.start.size(); r++) {
                std::fill(row + g0, row + lm.start[r], qa_outside);
                memcpy(row + lm.start[r], src + lm.off[r], (size_t)lm.len[r] * 4);
                g0 = lm.start[r] + lm.len[r];
            }
            std::fill(row + g0, row + lm.vend, qa_outside);
        });
        return FIB_OK;
    });
}

}  // namespace

extern "C" int fib_gqi_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, const float *bvec,
                           const float *verts, int nverts, const int32_t *faces, int nfaces, float sigma,
                           float *odf, float *const peak[3], float *const qa[3]) try {
    const OdfSpec spec{false, bval, bvec, nvol, verts, nverts, faces, nfaces, sigma, 0};
    return odf_rec_host(device, spec, dwi, nx, ny, nz, mask, mask_dtype, nullptr, odf, peak, qa);
} FIB_API_CATCH

extern "C" int fib_dsi_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol,
                           const void *mask, int mask_dtype, const float *bval, const float *bvec,
                           const float *verts, int nverts, const int32_t *faces, int nfaces, int hann_width,
                           float *pdf, float *odf, float *const peak[3], float *const qa[3]) try {
    FIB_CHECK(pdf != nullptr, FIB_ERR_INVALID, "NULL pdf output volume");
    const OdfSpec spec{true, bval, bvec, nvol, verts, nverts, faces, nfaces, 0.0f, hann_width};
    return odf_rec_host(device, spec, dwi, nx, ny, nz, mask, mask_dtype, pdf, odf, peak, qa);
} FIB_API_CATCH

// rumba_rec (rusd.jl:419-636), host buffers.  A whole-volume fixed-point iteration: not chunked.
extern "C" int fib_rumba_rec(int device, const float *dwi, int nx, int ny, int nz, int nvol, const void *mask, int mask_dtype,
                             const float *bval, const float *bvec, const float *verts, int nverts, int niter,
                             float lam_para, float lam_perp, float lam_csf, float lam_gm, int ncoils, int sos_grappa, int ipat_factor,
                             int use_tv, const fib_rumba_out *out, float *snr_mean, float *snr_std) try {
    FIB_CHECK(dwi && mask && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    DevLease lease;
    fib_rumba_plan *p = nullptr;                             // the constructor's refusals come first, the device index among them (FIB_DEVICE_ALL too)
    RC(fib_rumba_plan_create(device, bval, bvec, nvol, verts, nverts, lam_para, lam_perp, lam_csf, lam_gm, &p));
    fib::Scoped<fib_rumba_plan, fib_rumba_plan_destroy> del(p);
    RC(lease.take(device, nullptr));
    const int64_t nvox = (int64_t)nx * ny * nz;
    const int nvert = nverts / 2;
    std::vector<uint8_t> m8;
    RC(mask_convert(mask, mask_dtype, nvox, true, m8));            // mask.vol .> 0, rusd.jl:446
    fib::DevBuf<float> d_dwi, d_fodf, d_sc, d_pk;
    fib::DevBuf<uint8_t> d_mask;
    RC(d_dwi.alloc((size_t)nvox * nvol));
    RC(d_mask.alloc((size_t)nvox));
    RC(d_fodf.alloc((size_t)nvox * nvert));
    RC(d_sc.alloc((size_t)nvox * 4));
    RC(d_pk.alloc((size_t)nvox * 15));
    RC(h2d(d_dwi.p, dwi, sizeof(float) * nvox * nvol));
    RC(h2d(d_mask.p, m8.data(), (size_t)nvox));
    fib_rumba_out dev{};
    dev.fodf = d_fodf.p; dev.fgm = d_sc.p; dev.fcsf = d_sc.p + nvox; dev.gfa = d_sc.p + 2 * nvox; dev.var = d_sc.p + 3 * nvox;
    for (int i = 0; i < 5; i++) dev.peak[i] = d_pk.p + (size_t)i * 3 * nvox;
    RC(fibd_rumba_rec(p, d_dwi.p, d_mask.p, nx, ny, nz, niter, ncoils, sos_grappa, ipat_factor, use_tv, &dev, snr_mean, snr_std, nullptr));
    RC(d2h(out->fodf, dev.fodf, sizeof(float) * nvox * nvert));
    RC(d2h(out->fgm, dev.fgm, sizeof(float) * nvox));
    RC(d2h(out->fcsf, dev.fcsf, sizeof(float) * nvox));
    RC(d2h(out->gfa, dev.gfa, sizeof(float) * nvox));
    RC(d2h(out->var, dev.var, sizeof(float) * nvox));
    for (int i = 0; i < 5; i++) RC(d2h(out->peak[i], dev.peak[i], sizeof(float) * nvox * 3));
    return FIB_OK;
} FIB_API_CATCH

// find_peaks!(W) (gqi.jl:180-201) for nvox ODFs held in host memory: odf [nvox x nvert] planar (vertex-major rows of
// nvox values, like MRI.vol[:,:,:,v]); isort_top [3 x nvox] planar, 0-based first-half vertex rows, -1 where the
// tessellation has fewer vertices; nvalid [nvox] = count(odf_peak .> 0) (gqi.jl:200).
namespace {
// fib_find_peaks / fib_find_peaks_work: the checks, the plan (its constructor refuses what is left, the device index among them), the lease,
// the ODFs up, call(plan, d_odf, d_a, d_b, d_nv) = the form's fibd_* call, the outputs back.  a and, for a form that has_b, b are the
// form's own outputs, of wa and wb elements per voxel.
template <typename A, typename B, typename Call>
int find_peaks_host(int device, const float *odf, int64_t nvox, const float *verts, int nverts, const int32_t *faces, int nfaces, A *a, int wa,
                    bool has_b, B *b, int wb, int32_t *nvalid, Call call) {
    FIB_CHECK(odf && verts && faces && a && (b || !has_b) && nvalid, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nvox > 0 && nverts >= 2 && nverts % 2 == 0 && nfaces > 0, FIB_ERR_INVALID, "invalid sizes");
    DevLease lease;
    fib_odf_plan *plan = nullptr;
    RC(fib::peaks_plan_create(device, verts, nverts, faces, nfaces, &plan));
    fib::Scoped<fib_odf_plan, fib_odf_plan_destroy> del(plan);
    RC(lease.take(device, nullptr));
    const size_t nv = (size_t)nvox, n = nv * (nverts / 2);
    fib::DevBuf<float> d_odf;
    fib::DevBuf<A> d_a;
    fib::DevBuf<B> d_b;
    fib::DevBuf<int32_t> d_nv;
    RC(d_odf.alloc(n)); RC(d_a.alloc(nv * wa)); RC(d_nv.alloc(nv));
    if (has_b) RC(d_b.alloc(nv * wb));
    RC(h2d(d_odf.p, odf, n * sizeof(float)));
    RC(call(plan, d_odf.p, d_a.p, d_b.p, d_nv.p));
    FIB_HIP(hipDeviceSynchronize());
    RC(d2h(a, d_a.p, nv * wa * sizeof(A)));
    if (has_b) RC(d2h(b, d_b.p, nv * wb * sizeof(B)));
    return d2h(nvalid, d_nv.p, nv * sizeof(int32_t));
}
}  // namespace

extern "C" int fib_find_peaks(int device, const float *odf, int64_t nvox, const float *verts, int nverts,
                              const int32_t *faces, int nfaces, int32_t *isort_top, int32_t *nvalid) try {
    return find_peaks_host(device, odf, nvox, verts, nverts, faces, nfaces, isort_top, 3, false, (int32_t *)nullptr, 0, nvalid,
                           [&](const fib_odf_plan *plan, const float *d_odf, int32_t *d_top, int32_t *, int32_t *d_nv) {
                               return fibd_find_peaks(plan, d_odf, nvox, d_top, d_nv, nullptr); });
} FIB_API_CATCH

extern "C" int fib_find_peaks_work(int device, const float *odf, int64_t nvox, const float *verts, int nverts,
                                   const int32_t *faces, int nfaces, float *odf_peak, int32_t *isort, int32_t *nvalid) try {
    return find_peaks_host(device, odf, nvox, verts, nverts, faces, nfaces, odf_peak, nverts / 2, true, isort, nverts / 2, nvalid,
                           [&](const fib_odf_plan *plan, const float *d_odf, float *d_pk, int32_t *d_is, int32_t *d_nv) {
                               return fibd_find_peaks_work(plan, d_odf, nvox, d_pk, d_is, d_nv, nullptr); });
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// stream
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" void fib_tract_free(fib_tract_out *out) try {
    if (!out) return;
    free(out->npts); free(out->seed_index); free(out->xyz); free(out->flags);
    out->npts = nullptr; out->seed_index = nullptr; out->xyz = nullptr; out->flags = nullptr;
    out->nlines = 0; out->npoints = 0;
} FIB_API_CATCH_VOID

namespace {

struct StreamIn {
    const fib_stream_params *prm; const float *const *ovec; const float *const *f; float f_thresh; const float *fa; float fa_thresh;
    const float *sublist; int32_t nsub; const float *lcms; float lcm_thresh; uint64_t rng_seed; int strd0, strd1;
};
// what a tracking form returns, or one worker of a device set traced (host_tier.h); with one worker its arrays ARE the result
using fibh::TractArrays;
int tract_alloc(TractArrays &t, int64_t nl, int64_t np, bool with_flags) {
    return t.alloc(nl, np, with_flags) ? FIB_OK : fib::fail(FIB_ERR_NOMEM, "out of host memory");
}

// device -> pageable host memory, pipelined: pieces of up to 64 MB come down into two slots of the worker's pinned output ring while the
// scatter pool copies the previous piece to its destination (a plain hipMemcpy into pageable memory stages through a small driver buffer
// at a third of the link's rate, and the first touch of a freshly malloc'ed destination falls on one thread)
int d2h_pipelined(DevState &d, void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return FIB_OK;
    const size_t piece = std::min<size_t>(bytes, (size_t)64 << 20);
    for (int b = 0; b < 2; b++) RC(d.pin_out[b].ensure(piece, d.device, d.cpus));
    const size_t np = (bytes + piece - 1) / piece;
    const int nt = 16;
    auto drain = [&](size_t i) -> int {                  // piece i: ring -> destination
        const int b = (int)(i & 1);
        FIB_HIP(hipEventSynchronize(d.e_out[b]));
        const size_t o = i * piece, n = std::min(piece, bytes - o);
        const size_t part = ((n + nt - 1) / nt + 63) & ~(size_t)63;
        d.pool_out->run(nt, [&](int t) {
            const size_t a = (size_t)t * part;
            if (a < n) memcpy((char *)dst + o + a, d.pin_out[b].p + a, std::min(part, n - a));
        });
        return FIB_OK;
    };
    for (size_t i = 0; i < np; i++) {
        const int b = (int)(i & 1);
        const size_t o = i * piece, n = std::min(piece, bytes - o);
        {
            fib::ProfScope prof("host_d2h", st);
            FIB_HIP(hipMemcpyAsync(d.pin_out[b].p, (const char *)src + o, n, hipMemcpyDeviceToHost, st));
        }
        FIB_HIP(hipEventRecord(d.e_out[b], st));
        if (i > 0) RC(drain(i - 1));
    }
    return drain(np - 1);
}

// worker w of nw on its share of the seeds (fibh::seed_share)
int stream_worker(DevState &d, int w, int nw, const StreamIn &in, const std::vector<uint8_t> *m8, const std::vector<int64_t> &seeds,
                  std::vector<uint8_t> *seed_mask_out, TractArrays &sh) {
    const fib_stream_params &prm0 = *in.prm;
    const int nvec = prm0.nvec;
    const int64_t nvox = (int64_t)prm0.nx * prm0.ny * prm0.nz;
    FIB_HIP(hipSetDevice(d.device));
    if (!d.ws) RC(fibd_stream_ws_create(d.device, &d.ws));
    hipStream_t st = d.s_cmp;
    std::unique_ptr<HostTimer> tm(new HostTimer("stream_host_upload_field"));
    if (!d.sb) d.sb.reset(new DevState::StreamBufs());
    auto &sb = *d.sb;
    auto &d_vec = sb.vec; auto &d_f = sb.f; auto &d_fa = sb.fa; auto &d_field = sb.field; auto &d_sub = sb.sub; auto &d_lcms = sb.lcms;
    auto &d_mask = sb.mask; auto &d_mout = sb.mout;
    RC(d_vec.ensure((size_t)nvox * 3 * nvec));
    RC(d_field.ensure((size_t)nvox * 4 * nvec));
    RC(d_mout.ensure((size_t)nvox));
    const float *dv[8] = {}, *df[8] = {};
    for (int k = 0; k < nvec; k++) {
        RC(h2d(d_vec.p + (size_t)k * nvox * 3, in.ovec[k], sizeof(float) * nvox * 3));
        dv[k] = d_vec.p + (size_t)k * nvox * 3;
    }
    if (in.f) {
        RC(d_f.ensure((size_t)nvox * nvec));
        for (int k = 0; k < nvec; k++) { RC(h2d(d_f.p + (size_t)k * nvox, in.f[k], sizeof(float) * nvox)); df[k] = d_f.p + (size_t)k * nvox; }
    }
    if (in.fa) { RC(d_fa.ensure((size_t)nvox)); RC(h2d(d_fa.p, in.fa, sizeof(float) * nvox)); }
    if (m8) { RC(d_mask.ensure((size_t)nvox)); RC(h2d(d_mask.p, m8->data(), (size_t)nvox)); }
    RC(fibd_stream_field(nvec, nvox, dv, in.f ? df : nullptr, in.f_thresh, in.fa ? d_fa.p : nullptr, in.fa_thresh,
                         m8 ? d_mask.p : nullptr, d_field.p, d_mout.p, st));
    if (seed_mask_out) {                                 // first pass (no seed volume): the tracking mask back to the host
        seed_mask_out->resize((size_t)nvox);
        FIB_HIP(hipStreamSynchronize(st));
        RC(d2h(seed_mask_out->data(), d_mout.p, (size_t)nvox));
        return FIB_OK;
    }
    tm.reset(new HostTimer("stream_host_seeds_trace"));
    std::vector<int64_t> mine;
    fibh::seed_share(seeds, w, nw, mine);
    auto &d_seeds = sb.seeds;
    RC(d_seeds.ensure(mine.size()));
    if (!mine.empty()) RC(h2d(d_seeds.p, mine.data(), sizeof(int64_t) * mine.size()));
    RC(d_sub.ensure((size_t)in.nsub * 3));
    RC(h2d(d_sub.p, in.sublist, sizeof(float) * 3 * in.nsub));
    fib_stream_params prm = prm0;
    prm.ws = d.ws;
    fib_stream_job *job = nullptr;
    int64_t nl = 0, np = 0;
    if (in.lcms) {
        // the uniforms of a line are a function of its index in the WHOLE list (the header's random-number contract), which a
        // shard of a round-robin split cannot express -> LCM runs use one worker (stream_host)
        RC(d_lcms.ensure((size_t)nvox * 10));
        RC(h2d(d_lcms.p, in.lcms, sizeof(float) * nvox * 10));
        RC(fibd_stream_trace_lcm(&prm, d_field.p, d_lcms.p, in.lcm_thresh, in.strd0, in.strd1, in.rng_seed, d_seeds.p, (int64_t)mine.size(),
                                 d_sub.p, in.nsub, st, &job, &nl, &np));
    } else {
        RC(fibd_stream_trace(&prm, d_field.p, d_seeds.p, (int64_t)mine.size(), d_sub.p, in.nsub, st, &job, &nl, &np));
    }
    fib::Scoped<fib_stream_job, fib_stream_job_destroy> jg(job);
    tm.reset(new HostTimer("stream_host_results"));
    RC(tract_alloc(sh, nl, np, in.lcms != nullptr));
    if (nl > 0) {
        auto &d_npts = sb.npts; auto &d_sidx = sb.sidx; auto &d_xyz = sb.xyz; auto &d_flags = sb.flags;
        RC(d_npts.ensure((size_t)nl));
        RC(d_sidx.ensure((size_t)nl));
        RC(d_xyz.ensure((size_t)np * 3));
        if (in.lcms) RC(d_flags.ensure((size_t)np));
        RC(fibd_stream_pack_flags(job, d_npts.p, d_sidx.p, d_xyz.p, in.lcms ? d_flags.p : nullptr, st));
        RC(d2h_pipelined(d, sh.xyz, d_xyz.p, sizeof(float) * 3 * (size_t)np, st));     // (stream order: behind the pack kernels)
        RC(d2h_pipelined(d, sh.npts, d_npts.p, sizeof(int32_t) * (size_t)nl, st));
        RC(d2h_pipelined(d, sh.sidx, d_sidx.p, sizeof(int64_t) * (size_t)nl, st));
        if (in.lcms) RC(d2h_pipelined(d, sh.flags, d_flags.p, (size_t)np, st));
        if (nw > 1) for (int64_t i = 0; i < nl; i++) sh.sidx[i] = fibh::global_seed_index(sh.sidx[i], w, nw, in.nsub);
    }
    return FIB_OK;
}

int stream_host(int device, const fib_stream_params *prm, const float *const *ovec, const float *const *f,
                float f_thresh, const float *fa, float fa_thresh, const void *mask, int mask_dtype,
                const void *seed, int seed_dtype, const float *sublist, int32_t nsub,
                const float *lcms, float lcm_thresh, uint64_t rng_seed, fib_tract_out *out) {
    FIB_CHECK(prm && ovec && sublist && out, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(prm->nx > 0 && prm->ny > 0 && prm->nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(prm->nvec >= 1 && prm->nvec <= 8, FIB_ERR_UNSUPPORTED, "1..8 orientation vectors per voxel are supported");
    FIB_CHECK(nsub >= 1, FIB_ERR_INVALID, "sublist must hold at least one offset");
    memset(out, 0, sizeof *out);
    const int nvec = prm->nvec;
    const int64_t nvox = (int64_t)prm->nx * prm->ny * prm->nz;
    for (int k = 0; k < nvec; k++) {
        FIB_CHECK(ovec[k] != nullptr, FIB_ERR_INVALID, "NULL orientation volume %d", k);
        if (f) FIB_CHECK(f[k] != nullptr, FIB_ERR_INVALID, "NULL amplitude volume %d", k);
    }
    std::vector<Worker> ws;
    RC(workers_for(device, ws));
    if (lcms && ws.size() > 1) ws.resize(1);             // (see stream_worker)
    StreamIn in{prm, ovec, f, f_thresh, fa, fa_thresh, sublist, nsub, lcms, lcm_thresh, rng_seed, 0, 1};
    if (lcms) {
        // through-plane dimension = the one in which the first orientation volume is zero everywhere (stream.jl:221-223)
        bool allzero[3] = {true, true, true};
        for (int c = 0; c < 3; c++)
            for (int64_t i = 0; i < nvox && allzero[c]; i++) if (ovec[0][(size_t)c * nvox + i] != 0.0f) allzero[c] = false;
        int strd[3], ns = 0;
        for (int c = 0; c < 3; c++) if (!allzero[c]) strd[ns++] = c;
        FIB_CHECK(ns >= 2, FIB_ERR_INVALID, "LCM-guided tracking needs two in-plane dimensions with non-zero orientation components");
        in.strd0 = strd[0]; in.strd1 = strd[1];
    }
    std::unique_ptr<HostTimer> tm(new HostTimer("stream_host_masks_first_pass"));
    std::vector<uint8_t> m8, s8;
    if (mask) RC(mask_convert(mask, mask_dtype, nvox, true, m8));   // mask.vol .> 0, stream.jl:102
    // seed voxels: findall(W.mask) (stream.jl:744) or findall(seed.vol .> 0) (stream.jl:751), column-major order
    if (seed) RC(mask_convert(seed, seed_dtype, nvox, true, s8));
    else {
        TractArrays none;
        std::vector<int64_t> noseeds;
        RC(for_each_worker({ws[0]}, [&](int, DevState &d) { return stream_worker(d, 0, 1, in, mask ? &m8 : nullptr, noseeds, &s8, none); }));
    }
    tm.reset(new HostTimer("stream_host_seed_list"));
    std::vector<int64_t> seeds;
    fibh::seed_voxels(s8.data(), nvox, seeds);
    tm.reset();
    const int nw = (int)ws.size();
    std::vector<TractArrays> shards((size_t)nw);
    RC(for_each_worker(ws, [&](int w, DevState &d) { return stream_worker(d, w, nw, in, mask ? &m8 : nullptr, seeds, nullptr, shards[w]); }));
    if (nw == 1) { shards[0].give(out); return FIB_OK; }   // one worker: its arrays are the result
    int64_t nl = 0, np = 0;
    for (auto &s : shards) { nl += s.nl; np += s.np; }
    TractArrays merged;
    RC(tract_alloc(merged, nl, np, false));              // (no flags: an LCM run has one worker)
    fibh::merge_lines(shards.data(), nw, merged);
    merged.give(out);
    return FIB_OK;
}

}  // namespace

extern "C" int fib_stream(int device, const fib_stream_params *prm, const float *const *ovec, const float *const *f,
                          float f_thresh, const float *fa, float fa_thresh, const void *mask, int mask_dtype,
                          const void *seed, int seed_dtype, const float *sublist, int32_t nsub, fib_tract_out *out) try {
    return stream_host(device, prm, ovec, f, f_thresh, fa, fa_thresh, mask, mask_dtype, seed, seed_dtype, sublist, nsub,
                       nullptr, 0.0f, 0, out);
} FIB_API_CATCH

extern "C" int fib_stream_lcm(int device, const fib_stream_params *prm, const float *const *ovec, const float *const *f,
                              float f_thresh, const float *fa, float fa_thresh, const void *mask, int mask_dtype,
                              const void *seed, int seed_dtype, const float *sublist, int32_t nsub,
                              const float *lcms, float lcm_thresh, uint64_t rng_seed, fib_tract_out *out) try {
    FIB_CHECK(lcms != nullptr, FIB_ERR_INVALID, "NULL lcms volume");
    return stream_host(device, prm, ovec, f, f_thresh, fa, fa_thresh, mask, mask_dtype, seed, seed_dtype, sublist, nsub,
                       lcms, lcm_thresh, rng_seed, out);
} FIB_API_CATCH

// ------------------------------------------------------------------------------------------------------------------------------
// prob_stream: probabilistic ODF tracking (probtrack.hip), host buffers.  One device.
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int fib_prob_stream(int device, int nx, int ny, int nz, const float *odf, int nvert, const float *vertices, const uint8_t *mask,
                               const uint8_t *seed, const float *sublist, int32_t nsub, int32_t len_min, int32_t len_max, float cosang_thresh,
                               float step_size, float pmf_thresh, int32_t subtract_min, uint64_t rng_seed, fib_tract_out *out) try {
    FIB_CHECK(out, FIB_ERR_INVALID, "NULL out");
    memset(out, 0, sizeof *out);
    FIB_CHECK(device != FIB_DEVICE_ALL, FIB_ERR_UNSUPPORTED, "prob_stream runs on one device (FIB_DEVICE_ALL is not supported)");
    FIB_CHECK(odf && vertices && sublist, FIB_ERR_INVALID, "NULL argument");
    FIB_CHECK(nx > 0 && ny > 0 && nz > 0, FIB_ERR_INVALID, "volume dimensions must be positive");
    FIB_CHECK(nsub >= 1, FIB_ERR_INVALID, "sublist must hold at least one offset");
    DevLease lease;
    RC(lease.take(device, nullptr));
    DevState &d = *lease.wk;
    RC(d.init(copy_threads(1)));                         // (the download below runs on the worker's output ring)
    fib_prob_plan *plan_raw = nullptr;
    RC(fib_prob_plan_create(device, vertices, nvert, cosang_thresh, &plan_raw));
    fib::Scoped<fib_prob_plan, fib_prob_plan_destroy> plan(plan_raw);
    const int64_t nvox = (int64_t)nx * ny * nz;
    const int pitch = fib_prob_row_pitch(nvert);
    // the table, from voxel chunks of the host ODF: the float ODF is never whole on the device
    fib::DevBuf<uint16_t> d_table;
    fib::DevBuf<float> d_odf;
    fib::DevBuf<uint8_t> d_mask;
    const int64_t chunk = std::min<int64_t>(nvox, (int64_t)1 << 18);
    RC(d_table.alloc((size_t)nvox * pitch));
    RC(d_odf.alloc((size_t)chunk * nvert));
    if (mask) RC(d_mask.alloc((size_t)chunk));
    for (int64_t v0 = 0; v0 < nvox; v0 += chunk) {
        const int64_t n = std::min(chunk, nvox - v0);
        FIB_HIP(hipMemcpy2D(d_odf.p, sizeof(float) * (size_t)n, odf + v0, sizeof(float) * (size_t)nvox, sizeof(float) * (size_t)n, (size_t)nvert,
                            hipMemcpyHostToDevice));
        if (mask) RC(h2d(d_mask.p, mask + v0, (size_t)n));
        RC(fibd_prob_table(d_odf.p, mask ? d_mask.p : nullptr, n, nvert, subtract_min, pmf_thresh, d_table.p + (size_t)v0 * pitch, nullptr));
        FIB_HIP(hipStreamSynchronize(nullptr));                // (the chunk buffers are written again)
    }
    d_odf.release(); d_mask.release();
    // seeds: the seed volume, else the mask, else every voxel
    std::vector<int64_t> seeds;
    fibh::seed_voxels(seed ? seed : mask, nvox, seeds);
    const int64_t nseed = (int64_t)seeds.size();
    fib::DevBuf<int64_t> d_seeds, d_sidx, d_work;
    fib::DevBuf<float> d_sub, d_xyz;
    fib::DevBuf<int32_t> d_npts;
    RC(fib::upload(d_seeds, seeds));
    RC(fib::upload(d_sub, sublist, (size_t)3 * nsub));
    const size_t wb = fib::prob_work_bytes(nseed * nsub);
    RC(d_work.alloc(wb / 8));
    const fib::ProbRun r{plan_raw, nx, ny, nz, len_min, len_max, nsub, step_size, d_table.p, d_seeds.p, nseed, d_sub.p, rng_seed};
    hipStream_t st = d.s_cmp;                            // (the table is complete: every chunk waited for the NULL stream)
    int64_t nl = 0, np = 0;
    RC(fib::prob_count(r, d_work.p, wb, st, &nl, &np));
    RC(d_npts.alloc((size_t)nl));
    RC(d_sidx.alloc((size_t)nl));
    RC(d_xyz.alloc((size_t)3 * np));
    RC(fib::prob_emit(r, d_work.p, d_npts.p, d_sidx.p, d_xyz.p, st));
    TractArrays res;
    RC(tract_alloc(res, nl, np, false));
    RC(d2h_pipelined(d, res.xyz, d_xyz.p, sizeof(float) * 3 * (size_t)np, st));     // (stream order: behind the emit kernel)
    RC(d2h_pipelined(d, res.npts, d_npts.p, sizeof(int32_t) * (size_t)nl, st));
    RC(d2h_pipelined(d, res.sidx, d_sidx.p, sizeof(int64_t) * (size_t)nl, st));
    res.give(out);
    return FIB_OK;
} FIB_API_CATCH
