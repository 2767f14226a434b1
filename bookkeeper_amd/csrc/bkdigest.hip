// libbkdigest.so — C-ABI over the CDNA4 CRC kernels (include/bkdigest.h).
//
// Runtime glue: per-device operator-table images, launch geometry, per-stream bounds flags,
// the host-memory staging paths and the DigestManager batch framing sequences. The only CPU
// arithmetic is the per-call route for host buffers (host_crc.cpp, bkd_resume*); every batch
// entry point runs on the GPU and returns BKD_ERR_NO_DEVICE without one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <shared_mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bkdigest.h"
#include "crc_kernels.hpp"
#include "plan_kernels.hpp"
#include "crc_tables.hpp"
#include "host_batch.hpp"
#include "host_crc.hpp"
#include "host_mac.hpp"
#include "host_scrub.hpp"
#include "mac_kernels.hpp"
#include "scrub_kernels.hpp"
#include "scrub_report_kernels.hpp"

namespace {

thread_local std::string t_err;

int fail(int code, const std::string& msg) {
    t_err = msg;
    return code;
}

#define BKD_HIP(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(BKD_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

constexpr int kLaneChoices[6] = {1, 4, 8, 16, 32, 64};
constexpr int kNumLaneChoices = 6;
constexpr int kMaxDevices = 64;

int lane_index(int lanes) {
    for (int k = 0; k < kNumLaneChoices; ++k)
        if (kLaneChoices[k] == lanes) return k;
    return -1;
}

// Scratch kept per (device, stream) between calls. A call's kernels use it in stream order, so
// consecutive calls on one stream can share it; the launch sequence is enqueued under `mu` so that
// host threads sharing a stream do not interleave their sequences. It only grows: the old buffer is
// freed after a sync of its stream (growth is rare; per-call allocation left the GPU idle ~40 us
// between calls, profiles/r01_diag_ragged.log). Plain hipMalloc, not the stream-ordered pool:
// reused hipMallocAsync blocks fed stale data to the kernels on the host one-copy route (round 3,
// DESIGN.md §5a), so the library keeps no device memory of its own in that pool.
struct StreamScratch {
    std::recursive_mutex mu;
    static constexpr int kSlots = 5;
    // slot 0: plan scratch (launch_plan), 1: verify pipeline, 2: segment CRCs, 3: package_v2's frames,
    // 4: the ledger scrub's (its CRC classes nest the verify pipeline, which nests the plan)
    uint8_t* buf[kSlots] = {};
    size_t cap[kSlots] = {};
    // Sticky bounds-violation flag of the indexed batches enqueued on this stream (one per
    // stream, so a caller's out-of-range entry is reported to that caller's bkd_stream_sync
    // only); read and cleared in stream order. h_err: pinned landing word for the read.
    uint32_t* err = nullptr;
    uint32_t* h_err = nullptr;
    // PlanRun word of the plans enqueued on this stream and the epoch of the latest one
    uint32_t* run = nullptr;
    uint32_t* uni = nullptr;  // PlanRun uniform-lengths word (the epoch of the call it holds for)
    uint32_t epoch = 0;
    // verify gate word (verify_gate_kernel) and the epoch of the latest verify on this stream
    uint32_t* vflag = nullptr;
    uint32_t vepoch = 0;
    // One of the lazily made, zero-initialised device words above (err, run, uni, vflag).
    hipError_t word(uint32_t*& w, hipStream_t st) {
        if (w) return hipSuccess;
        hipError_t e = hipMalloc((void**)&w, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemsetAsync(w, 0, sizeof(uint32_t), st);
        if (e != hipSuccess) w = nullptr;
        return e;
    }
    hipError_t flag(hipStream_t st) {  // err, with its pinned landing word
        if (err) return hipSuccess;
        hipError_t e = word(err, st);
        if (e == hipSuccess && !h_err) e = hipHostMalloc((void**)&h_err, sizeof(uint32_t), hipHostMallocDefault);
        if (e != hipSuccess) err = nullptr;
        return e;
    }
    // Returns slot `which` with at least `bytes` bytes, stream-ordered on `st`.
    hipError_t get(int which, size_t bytes, hipStream_t st, uint8_t** out) {
        if (cap[which] < bytes) {
            if (buf[which]) {  // work already enqueued on this stream may still use the old buffer
                const hipError_t e = hipStreamSynchronize(st);
                if (e != hipSuccess) return e;
                (void)hipFree(buf[which]);
            }
            buf[which] = nullptr;
            cap[which] = 0;
            const size_t want = bytes + bytes / 4 + 4096;
            hipError_t e = hipMalloc((void**)&buf[which], want);
            if (e != hipSuccess) return e;
            cap[which] = want;
        }
        *out = buf[which];
        return hipSuccess;
    }
};

// Lays out 256-byte-aligned sub-buffers of one scratch allocation: take() returns offsets
// during the sizing pass; at(base, off) turns them into pointers.
struct Carver {
    size_t used = 0;
    size_t take(size_t bytes) {
        const size_t at = used;
        used += (bytes + 255) & ~(size_t)255;
        return at;
    }
    template <class T>
    static T* at(uint8_t* base, size_t off) {
        return reinterpret_cast<T*>(base + off);
    }
};

// Per device: tables uploaded once (under g_mu, published by `ready`), then read-only; the two maps
// below grow on first use of an (algo, chunk size) or a stream and are read under a shared lock, so
// concurrent callers on their own streams never serialise on a process-wide lock.
struct DeviceState {
    std::atomic<bool> ready{false};
    int cus = 0;
    uint32_t* tables[2][kNumLaneChoices] = {};  // [algo][lane choice] compact operator images
    uint32_t* xinv[2] = {};       // [algo] x^(-8k), k = 0..127: removes the plan's zero padding
    uint32_t* xp8[2] = {};        // [algo] word 256 k + b = x^(8 b 256^k), k = 0..3 (reframe_frame_kernel)
    std::shared_mutex maps_mu;    // guards xtab and scratch
    std::map<uint64_t, uint32_t*> xtab;  // (algo, CH) -> x^(8*CH) operator for the plan's combine
    std::map<hipStream_t, std::unique_ptr<StreamScratch>> scratch;
};

std::mutex g_mu;  // device initialisation only
DeviceState g_dev[kMaxDevices];
std::atomic<int> g_forced_lanes{0};
std::atomic<int> g_plan_mode{0};  // 0 auto, 1 direct (one entry per group), 2 chunked plan

// Chunked plan geometry (bkd_set_plan_geometry): lanes per group, steps per full chunk
// (CH = 16 * lanes * jc bytes) and the head-merge threshold in bytes.
std::atomic<int> g_plan_lanes{8};
std::atomic<int> g_plan_jc{32};
std::atomic<int> g_plan_merge{16};
std::atomic<int> g_fold_sched{0};  // bkd_set_fold_schedule: 0 by the measured clock, 1 fixed, 2 low-clock
std::atomic<int> g_plan_pf{2};  // loads in flight per lane in the chunk kernel (2, 4 or 8)
// Short-entry class of indexed batches: entries of <= this many bytes skip the plan and run in
// their own launch (4-lane groups, next entry loaded during the current one). 0 = none.
constexpr int kSmallLanes = 4;
constexpr uint32_t kSmallBytes4 = 16u * kSmallLanes * 3u;  // one register set per entry (4 lanes, PF = 2): 192 B
constexpr int kSmallLanesWide = 8;                         // bounds above 192 B: 8 lanes, PF = 3
constexpr uint32_t kSmallMaxBytes = 16u * kSmallLanesWide * 4u;
std::atomic<uint32_t> g_plan_small{kSmallBytes4};
// Entries shorter than this skip the chunks: plan_combine computes them, one thread each. Longer
// bounds cost more than they save on config 3's Zipf mix: 128 B took 36 us off the chunk kernel
// and added 54 us to combine (random slice-by-16 lookups from 64 lanes conflict in LDS banks).
constexpr uint32_t kPlanSerial = 16;
std::atomic<uint32_t> g_plan_serial{kPlanSerial};
constexpr uint64_t kShortMeanMax = 1024;
std::atomic<uint64_t> g_short_mean_max{kShortMeanMax};  // bytes of base buffer per entry (bkd_set_short_class_mean)
// Indexed batches whose base buffer is at most this size skip the plan (latency over balance).
constexpr uint64_t kDirectMaxBytes = 256u << 10;

// Visible HIP devices, probed once per process (0 when the runtime finds none).
int visible_devices() {
    static std::once_flag once;
    static int count = 0;
    std::call_once(once, [] {
        if (hipGetDeviceCount(&count) != hipSuccess) {
            (void)hipGetLastError();
            count = 0;
        }
    });
    return count;
}

// The device a call runs on: a created stream's own device (hipStreamGetDevice), else the
// calling thread's current device (null, legacy and per-thread default streams).
int stream_device(hipStream_t st, int* dev) {
    if (visible_devices() <= 0) return fail(BKD_ERR_NO_DEVICE, "no HIP device");
    if (st == nullptr || st == hipStreamLegacy || st == hipStreamPerThread) {
        BKD_HIP(hipGetDevice(dev));
    } else {
        hipDevice_t d = 0;
        BKD_HIP(hipStreamGetDevice(st, &d));
        *dev = (int)d;
    }
    if (*dev < 0 || *dev >= kMaxDevices) return fail(BKD_ERR_NO_DEVICE, "device index out of range");
    return BKD_OK;
}

// Makes the stream's device current for the duration of a call and restores the caller's.
struct DeviceScope {
    int prev = -1;
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int init_device_locked(int dev) {
    DeviceState& ds = g_dev[dev];
    if (ds.ready.load(std::memory_order_acquire)) return BKD_OK;
    int prev = 0;
    BKD_HIP(hipGetDevice(&prev));
    BKD_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    BKD_HIP(hipGetDeviceProperties(&prop, dev));
    ds.cus = prop.multiProcessorCount;
    std::vector<uint32_t> img;
    for (int algo = 0; algo < 2; ++algo) {
        for (int k = 0; k < kNumLaneChoices; ++k) {
            const int lanes = kLaneChoices[k];
            img.assign((size_t)bkd::gf2::compact_words(lanes), 0u);
            bkd::gf2::build_compact(algo, lanes, img.data());
            BKD_HIP(hipMalloc(&ds.tables[algo][k], img.size() * sizeof(uint32_t)));
            BKD_HIP(hipMemcpy(ds.tables[algo][k], img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    for (int algo = 0; algo < 2; ++algo) {
        uint32_t inv[128];
        for (uint32_t k = 0; k < 128; ++k) inv[k] = bkd::gf2::xpow_neg8(algo, k);
        BKD_HIP(hipMalloc(&ds.xinv[algo], sizeof(inv)));
        BKD_HIP(hipMemcpy(ds.xinv[algo], inv, sizeof(inv), hipMemcpyHostToDevice));
        std::vector<uint32_t> xp(1024);
        for (uint32_t k = 0; k < 4u; ++k)
            for (uint64_t b = 0; b < 256u; ++b) xp[256u * k + b] = bkd::gf2::xpow(algo, (8ull * b) << (8u * k));
        BKD_HIP(hipMalloc(&ds.xp8[algo], xp.size() * sizeof(uint32_t)));
        BKD_HIP(hipMemcpy(ds.xp8[algo], xp.data(), xp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    BKD_HIP(hipSetDevice(prev));
    ds.ready.store(true, std::memory_order_release);
    return BKD_OK;
}

// The plan combine's operators, built once per (algo, ch) and device (bkd::kXtab* layout):
// tables of X = x^(8*ch), X^64 and X^1024, then X^L (L = 0..63) and X^(64 w) (w = 0..15).
int xtab_for(DeviceState& ds, int algo, uint32_t ch, const uint32_t** out) {
    const uint64_t key = ((uint64_t)algo << 32) | ch;
    {
        std::shared_lock<std::shared_mutex> rd(ds.maps_mu);
        auto it = ds.xtab.find(key);
        if (it != ds.xtab.end()) {
            *out = it->second;
            return BKD_OK;
        }
    }
    std::unique_lock<std::shared_mutex> wr(ds.maps_mu);
    auto it = ds.xtab.find(key);
    if (it == ds.xtab.end()) {
        std::vector<uint32_t> xt(bkd::kXtabWords);
        bkd::gf2::operator_tables(algo, bkd::gf2::xpow(algo, 8ull * ch), xt.data() + bkd::kXtabX);
        bkd::gf2::operator_tables(algo, bkd::gf2::xpow(algo, 8ull * ch * 64u), xt.data() + bkd::kXtabX64);
        bkd::gf2::operator_tables(algo, bkd::gf2::xpow(algo, 8ull * ch * 1024u), xt.data() + bkd::kXtabX1024);
        for (uint32_t k = 0; k < 64u; ++k) xt[bkd::kXtabLane + k] = bkd::gf2::xpow(algo, 8ull * ch * k);
        for (uint32_t k = 0; k < 16u; ++k) xt[bkd::kXtabWave + k] = bkd::gf2::xpow(algo, 8ull * ch * 64u * k);
        uint32_t* d = nullptr;
        BKD_HIP(hipMalloc(&d, xt.size() * sizeof(uint32_t)));
        BKD_HIP(hipMemcpy(d, xt.data(), xt.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        it = ds.xtab.emplace(key, d).first;
    }
    *out = it->second;
    return BKD_OK;
}

int enter(hipStream_t st, DeviceScope& scope, DeviceState** out) {
    int dev = 0;
    int rc = stream_device(st, &dev);
    if (rc) return rc;
    int cur = 0;
    BKD_HIP(hipGetDevice(&cur));
    if (cur != dev) {
        BKD_HIP(hipSetDevice(dev));
        scope.prev = cur;
    }
    if (!g_dev[dev].ready.load(std::memory_order_acquire)) {  // first call on the device only
        std::lock_guard<std::mutex> lk(g_mu);
        rc = init_device_locked(dev);
    }
    if (rc) return rc;
    *out = &g_dev[dev];
    return BKD_OK;
}

// A C-ABI call on `stream`: the stream's device made current until the call returns, that device's
// state, and what enter() answered.
struct Call {
    DeviceScope scope;
    DeviceState* ds = nullptr;
    const hipStream_t st;
    int rc;
    explicit Call(void* stream) : st((hipStream_t)stream), rc(enter(st, scope, &ds)) {}
};

// The stream's scratch, or nullptr when nothing was ever enqueued on it (no entry is created).
StreamScratch* scratch_find(DeviceState& ds, hipStream_t st) {
    std::shared_lock<std::shared_mutex> rd(ds.maps_mu);
    auto it = ds.scratch.find(st);
    return it == ds.scratch.end() ? nullptr : it->second.get();
}

StreamScratch& scratch_for(DeviceState& ds, hipStream_t st) {
    if (StreamScratch* sc = scratch_find(ds, st)) return *sc;  // hits take the shared lock only
    std::unique_lock<std::shared_mutex> wr(ds.maps_mu);
    auto& slot = ds.scratch[st];
    if (!slot) slot.reset(new StreamScratch());
    return *slot;
}

// *err = the stream's bounds flag (StreamScratch::err), made on first use.
int bounds_flag(DeviceState& ds, hipStream_t st, uint32_t** err) {
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);
    const hipError_t e = sc.flag(st);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("bounds flag: ") + hipGetErrorString(e));
    *err = sc.err;
    return BKD_OK;
}

// What bkd_stream_sync and bkd_stream_release report for a raised bounds flag.
constexpr const char* kBoundsMsg = "an indexed entry exceeded its base buffer (entries skipped, out = 0)";

// Lanes per entry group for the direct kernel, from the size sweep (profiles/r01_size_sweep.log):
// 4 lanes below 512 B, 8 up to 32 KiB, 32 above; then more lanes while the batch would not give
// every lane slot of the chip (CUs x 1024) one group lane, so a few huge entries still fill it.
int auto_lanes(uint64_t mean_len, uint64_t n = UINT64_MAX, int cus = 256) {
    const int forced = g_forced_lanes.load();
    if (forced) return forced;
    int g = mean_len < 512 ? 4 : (mean_len < 32768 ? 8 : 32);
    while (g < 64 && n < UINT64_MAX / 64 && n * (uint64_t)g < (uint64_t)cus * 1024u) g *= 2;
    return g;
}

// Loads in flight per lane (register double buffer depth) and load cache policy: the two build-time
// knobs, so that tools/tune.py can time its variants in one process.
#ifndef BKD_PF
#define BKD_PF 2
#endif
#ifndef BKD_NT
#define BKD_NT 1
#endif
constexpr int kPF = BKD_PF;
constexpr bool kNT = BKD_NT != 0;

// Turns a runtime lane count into a template argument: f(std::integral_constant<int, G>{}) for G in
// {1 (only if MinG <= 1), 4, 8, 16, 32, 64}. The one-entry-per-group kernel exists from G = 1; the
// plan, fused-verify and fused-package kernels from 4.
template <int MinG, class F>
int with_lanes(int lanes, F&& f) {
    switch (lanes) {
        case 1:
            if constexpr (MinG <= 1) return f(std::integral_constant<int, 1>{});
            break;
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
    }
    return fail(BKD_ERR_INVALID_ARG, "lanes must be 1, 4, 8, 16, 32 or 64");
}

// Grid of the one-entry-per-group kernels: a block per kBlock / G entries, at most one per CU.
unsigned group_blocks(const DeviceState& ds, uint64_t n, int G) {
    const uint64_t per_block = bkd::kBlock / G;
    return (unsigned)std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)ds.cus);
}

// host_count: an upper bound of src.count() used only to size the grid.
template <class Src>
int dispatch_lanes(DeviceState& ds, int lanes, int algo, const uint8_t* base, const Src& src, uint64_t host_count,
                   hipStream_t stream, uint32_t* err = nullptr) {
    return with_lanes<1>(lanes, [&](auto g) -> int {
        constexpr int G = decltype(g)::value;
        if (host_count == 0) return BKD_OK;
        hipLaunchKernelGGL((bkd::crc_groups_kernel<G, kPF, kNT, Src>), dim3(group_blocks(ds, host_count, G)),
                           dim3(bkd::kBlock), 0, stream, base, src, ds.tables[algo][lane_index(G)], err,
                           g_fold_sched.load());
        BKD_HIP(hipGetLastError());
        return BKD_OK;
    });
}

// Indexed batch through the chunked plan (plan_kernels.hpp): five stream-ordered kernels, no
// host sync, scratch from the stream's arena.
int launch_plan(DeviceState& ds, int algo, const uint8_t* base, uint64_t size, const uint64_t* offsets,
                const uint32_t* lengths, uint64_t n, const uint32_t* seeds, uint32_t seed_all, uint32_t* out,
                hipStream_t st, bool short_class = true, bool direct_gate = true, const uint32_t* ext_flag = nullptr,
                uint32_t ext_epoch = 0) {
    // ext_flag: the plan runs only if *ext_flag == ext_epoch when its kernels start (a gate decided on
    // the device before this call, verify_framed's); no short class and no uniformity gate then
    if (n == 0) return BKD_OK;
    if (ext_flag) short_class = direct_gate = false;
    if (n >= 0xFFFFFFF0ull) return fail(BKD_ERR_INVALID_ARG, "indexed batches hold fewer than 2^32 - 16 entries");
    const int G = g_plan_lanes.load();
    bkd::PlanGeo pg;
    pg.step = 16u * (uint32_t)G;
    pg.jc = (uint32_t)g_plan_jc.load();
    pg.ch = pg.step * pg.jc;
    pg.mis = (uint32_t)((uintptr_t)base & 127u);
    pg.merge = (uint32_t)g_plan_merge.load();
    pg.serial = g_plan_serial.load();
    // chunks of <= kShortPF + 1 steps: the chunk kernel's short tail, three chunks in flight per
    // group (short_chunks_loop)
    const int pf = g_plan_pf.load();
    pg.jshort = (uint32_t)bkd::kShortPF + 1u;
    // 8-byte descriptors when the batch has one seed for every entry (its head register is then a
    // kernel argument) and the default loads in flight (PlanDesc8, crc_kernels.hpp)
    pg.d8 = (seeds == nullptr && size < bkd::kPlanMaxSize8 && pf == 2) ? 1u : 0u;
    pg.nbins = (pg.ch + pg.merge - 1u + pg.step - 1u) / pg.step + 1u;
    pg.step_sh = (uint32_t)__builtin_ctz(pg.step);
    pg.ch_sh = (pg.ch & (pg.ch - 1u)) == 0u ? (uint32_t)__builtin_ctz(pg.ch) : 0xFFu;
    // The short-entry launch walks every entry's index in rounds of one entry per 4-lane group, a
    // memory round trip each: it pays where short entries dominate (64 M x 64 B: 7.2 -> 1.9 ms) and
    // costs more than it saves where they are a minority of a large-entry batch (config 3's Zipf:
    // +54 us launch, -43 us chunk kernel). So it runs when the mean entry is at most 1 KiB.
    const uint64_t mean_max = g_short_mean_max.load();
    // size <= mean_max * n, without forming the product (it could overflow for large bounds)
    const bool short_gate = mean_max == UINT64_MAX || size / n < mean_max || (size / n == mean_max && size % n == 0u);
    pg.small = (short_class && short_gate) ? g_plan_small.load() : 0u;
    const uint32_t* xtab = nullptr;
    int rc = xtab_for(ds, algo, pg.ch, &xtab);
    if (rc) return rc;
    // non-overlapping entries need at most sum(ceil((len + 127) / CH)) <= n + (size + 127 n) / CH chunks
    const uint64_t capacity = std::min<uint64_t>(n + (size + 128u * n) / pg.ch + 16, 0xFFFFFFF0ull);
    const uint32_t nb = (uint32_t)((n + bkd::kPlanBlock - 1) / bkd::kPlanBlock);
    const uint32_t ncols = bkd::plan_ncols(pg);
    Carver cv;
    const size_t o_blk = cv.take((size_t)nb * ncols * 4), o_live = cv.take((size_t)nb * 4),
                 o_bok = cv.take((size_t)nb * 4),
                 o_blkoff = cv.take((size_t)nb * ncols * 4), o_hdr = cv.take(bkd::kHdrWords * 4),
                 o_ps = cv.take((size_t)n * 4), o_hs = cv.take((size_t)n * 4), o_part = cv.take((size_t)capacity * 4),
                 o_desc = cv.take((size_t)capacity * sizeof(bkd::PlanDesc));
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);
    uint8_t* sb = nullptr;
    // without a short class (mean entry > 1 KiB), lengths all within 1/16 + 64 B of the first
    // entry's skip the chunks: the chunk kernel computes them whole, as the direct kernel would (PlanRun::uniform,
    // decided on the device: plan_count's per-block ballots, reduced by plan_scan). Only where the
    // direct kernel would use the plan's lane count.
    const bool gate = pg.small == 0u && direct_gate && auto_lanes(size / n, n, ds.cus) == G;
    hipError_t e = sc.get(0, cv.used, st, &sb);
    if (e == hipSuccess) e = sc.flag(st);
    if (e == hipSuccess && pg.small) e = sc.word(sc.run, st);
    if (e == hipSuccess && gate) e = sc.word(sc.uni, st);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("plan scratch: ") + hipGetErrorString(e));
    uint32_t *err = sc.err, *run_word = pg.small ? sc.run : nullptr, *uni = gate ? sc.uni : nullptr;
    if (++sc.epoch == 0u) ++sc.epoch;  // 0 is the words' initial value
    const bkd::PlanRun run = ext_flag ? bkd::PlanRun{ext_flag, nullptr, ext_epoch} : bkd::PlanRun{run_word, uni, sc.epoch};
    uint32_t *blk = Carver::at<uint32_t>(sb, o_blk), *blive = Carver::at<uint32_t>(sb, o_live),
             *bok = gate ? Carver::at<uint32_t>(sb, o_bok) : nullptr,
             *blkoff = Carver::at<uint32_t>(sb, o_blkoff), *hdr = Carver::at<uint32_t>(sb, o_hdr),
             *pslot = Carver::at<uint32_t>(sb, o_ps), *hslot = Carver::at<uint32_t>(sb, o_hs),
             *partials = Carver::at<uint32_t>(sb, o_part);
    bkd::PlanDesc* descs = Carver::at<bkd::PlanDesc>(sb, o_desc);
    if (pg.small) {  // the short-entry class, in its own launch (any order against the plan kernels)
        const bkd::SmallIndexedSrc ss{n, offsets, lengths, seeds, seed_all, size, out, pg.small, run_word, run.epoch};
        // bounds above 192 B: kSmallLanesWide-lane groups (8: up to 512 B), an entry's PF + 1 steps in one register set
        with_lanes<4>(pg.small <= kSmallBytes4 ? kSmallLanes : kSmallLanesWide, [&](auto g) -> int {
            constexpr int SG = decltype(g)::value;
            if constexpr (SG == kSmallLanes || SG == kSmallLanesWide)  // the class has these two widths only
                hipLaunchKernelGGL((bkd::crc_groups_kernel<SG, SG == kSmallLanes ? 2 : 3, kNT, bkd::SmallIndexedSrc>),
                                   dim3(group_blocks(ds, n, SG)), dim3(bkd::kBlock), 0, st, base, ss,
                                   ds.tables[algo][lane_index(SG)], err, 1);
            return BKD_OK;
        });
    }
    // count / emit / combine walk their 1024-entry blocks in grid stride (kPlanGrid blocks per CU)
    constexpr uint32_t kPlanGrid = 2;
    const uint32_t pgrid = kPlanGrid * (uint32_t)ds.cus;
    const uint32_t cgrid = std::min((nb + bkd::kCountBlocks - 1u) / bkd::kCountBlocks, pgrid);
    hipLaunchKernelGGL(bkd::plan_count_kernel, dim3(cgrid), dim3(bkd::kPlanBlock), 0, st, offsets,
                       lengths, size, n, pg, blk, blive, nb, run, bok);
    hipLaunchKernelGGL(bkd::plan_scan_kernel, dim3(ncols + (gate ? 1u : 0u)), dim3(bkd::kPlanBlock), 0, st, blk, nb,
                       blkoff, hdr, run, ncols, bok);
    // few entry blocks (large entries): replicate emit and combine blocks so ~2 blocks per CU work
    const uint32_t reps = nb >= 2u * (uint32_t)ds.cus ? 1u : std::min<uint32_t>(64u, (2u * (uint32_t)ds.cus + nb - 1u) / nb);
    hipLaunchKernelGGL(bkd::plan_emit_kernel, dim3(std::min(nb * reps, pgrid)), dim3(bkd::kPlanBlock), 0, st, offsets,
                       lengths, seeds, seed_all, size, n, pg, capacity, blkoff, pslot, hslot, hdr, descs, reps, blive, nb, run);
    const uint32_t* tab = ds.tables[algo][lane_index(G)];
    const bkd::PlanDirectSrc ov{n, offsets, lengths, seeds, seed_all, size, out, pslot, hdr, capacity, false};
    rc = with_lanes<4>(G, [&](auto g) -> int {
        auto launch = [&](auto depth, const auto* d) {
            using Desc = std::remove_cv_t<std::remove_pointer_t<decltype(d)>>;
            hipLaunchKernelGGL((bkd::crc_plan_chunks_kernel<decltype(g)::value, decltype(depth)::value, kNT,
                                                            bkd::PlanDirectSrc, Desc>),
                               dim3((unsigned)ds.cus), dim3(bkd::kBlock), 0, st, base, d, ~seed_all,
                               hdr + bkd::kHdrWork, tab, out, partials, ov, run, err);
        };
        // pf: read once above (one value per call); d8 (PlanDesc8) only with the default pf
        if (pf == 8) launch(std::integral_constant<int, 8>{}, descs);
        else if (pf == 4) launch(std::integral_constant<int, 4>{}, descs);
        else if (pg.d8) launch(std::integral_constant<int, 2>{}, reinterpret_cast<const bkd::PlanDesc8*>(descs));
        else launch(std::integral_constant<int, 2>{}, descs);
        return BKD_OK;
    });
    if (rc) return rc;
    const uint32_t* btab = tab + bkd::gf2::byte_table_offset(G);
    hipLaunchKernelGGL(bkd::plan_combine_kernel, dim3(std::min(nb * reps, pgrid)), dim3(1024), 0, st, base, offsets, lengths, seeds,
                       seed_all, size, n, pg, xtab, btab, ds.xinv[algo],
                       bkd::gf2::poly(algo), pslot, hslot, partials, out, err, reps, blive, nb, run);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(BKD_ERR_HIP, std::string("plan kernels: ") + hipGetErrorString(e));
    return BKD_OK;
}

// The route indexed_batch takes: the direct kernel (one entry per group) or the chunked plan.
bool indexed_direct(uint64_t size) {
    const int mode = g_plan_mode.load();
    // plan descriptors hold a biased 41-bit window start (PlanDesc): buffers >= 1 TiB take the direct kernel
    return mode == 1 || (mode == 0 && size <= kDirectMaxBytes) || size >= bkd::kPlanMaxSize;
}

// route: -1 decided here from the plan mode and the buffer size, else the caller's decision
// (0 direct, 1 plan) so that a route chosen once per call cannot change under bkd_set_plan_mode.
int indexed_batch(DeviceState& ds, int algo, const uint8_t* base, uint64_t size, const uint64_t* offsets,
                  const uint32_t* lengths, uint64_t n, const uint32_t* seeds, uint32_t seed_all, uint32_t* out,
                  hipStream_t st, const uint32_t* ext_flag = nullptr, uint32_t ext_epoch = 0, int route = -1) {
    if (route < 0) route = indexed_direct(size) ? 0 : 1;
    if (route == 1)
        return launch_plan(ds, algo, base, size, offsets, lengths, n, seeds, seed_all, out, st, true, true, ext_flag,
                           ext_epoch);
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    bkd::IndexedSrc src{n, offsets, lengths, seeds, seed_all, size, out};
    return dispatch_lanes(ds, auto_lanes(n ? size / n : 0, n, ds.cus), algo, base, src, n, st, err);
}

bool valid_algo(int algo) { return algo == BKD_CRC32C || algo == BKD_CRC32; }

using bkd::host::mac_len;

// The runtime's memory type of p (hipMemoryTypeUnregistered for plain pageable memory, which it does
// not know); *dev (if given) = the device a device pointer lives on.
hipMemoryType pointer_type(const void* p, int* dev = nullptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return hipMemoryTypeUnregistered;
    }
    if (dev) *dev = attr.device;
    return attr.type;
}

// ---- host-memory batches: pinned, double-buffered H2D -> kernel -> D2H -------------------
// Entries sorted by offset are cut into segments of at most kSeg payload bytes / kSegEntries
// entries; segment k uses staging slot k % 2 (its own stream), so the H2D copy of one segment
// overlaps the kernel and D2H of the other. A pinned (page-locked / registered) source is DMA'd
// in place; a pageable one is first copied into the slot's pinned buffer by the host.
struct HostStage {
    static constexpr size_t kSeg = 64u << 20;
    static constexpr size_t kSegEntries = 1u << 20;
    // d_buf holds kSeg staged bytes and this much more: the indexed kernels load whole 16-byte blocks (an
    // entry shorter than 16 bytes, an empty one included, the block at offset & ~15), which for an entry
    // at the very end of a full segment must still lie inside the allocation
    static constexpr size_t kSegSlack = 256;
    bool ready = false;
    uint8_t *h_pin[2] = {}, *d_buf[2] = {};
    uint64_t *h_off[2] = {}, *d_off[2] = {};
    uint32_t *h_len[2] = {}, *d_len[2] = {};
    uint32_t *h_seed[2] = {}, *d_seed[2] = {};
    uint32_t *h_res[2] = {}, *d_res[2] = {};
    hipStream_t st[2] = {};
    hipEvent_t done[2] = {};
    // framed-entry batches (bkd_digest_*_batch_host), allocated on first use and sized per path
    // (ADVICE r2): package needs per-entry ids, LACs and length fields in (24 B per entry) and the
    // frame headers out; verify only its first_bad word
    static constexpr size_t kAux = 64u << 20;
    bool pkg_ready = false, fb_ready = false;
    uint8_t *h_aux[2] = {}, *d_aux[2] = {};
    uint8_t *h_frm[2] = {}, *d_frm[2] = {};
    uint64_t *h_fb[2] = {}, *d_fb[2] = {};
    // reframe: the new LACs in (8 B per entry); its digests come back through d_seed / h_seed
    bool lac_ready = false;
    int64_t *h_lac[2] = {}, *d_lac[2] = {};
    // verify requests: per-entry expectations in (8 + 8 + 4 B per entry), then one zero u64 (the
    // segment's request 0 starts at its entry 0)
    static constexpr size_t kRqBytes = kSegEntries * 20 + 8;
    bool rq_ready = false;
    uint8_t *h_rq[2] = {}, *d_rq[2] = {};
    // Every buffer is made by pin() (pinned host) or dev() (device), which record it for the
    // destructor. Each allocation is made once: a call after a failed init*() completes the set,
    // nothing leaks.
    std::vector<void*> pinned, device;
    template <class T>
    int pin(T*& p, size_t bytes) {
        if (p) return BKD_OK;
        BKD_HIP(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
        pinned.push_back(p);
        return BKD_OK;
    }
    template <class T>
    int dev(T*& p, size_t bytes) {
        if (p) return BKD_OK;
        BKD_HIP(hipMalloc((void**)&p, bytes));
        device.push_back(p);
        return BKD_OK;
    }
    int init() {
        if (ready) return BKD_OK;
        for (int s = 0, rc; s < 2; ++s) {
            if ((rc = pin(h_pin[s], kSeg)) || (rc = dev(d_buf[s], kSeg + kSegSlack)) ||
                (rc = pin(h_off[s], kSegEntries * 8)) || (rc = dev(d_off[s], kSegEntries * 8)) ||
                (rc = pin(h_len[s], kSegEntries * 4)) || (rc = dev(d_len[s], kSegEntries * 4)) ||
                (rc = pin(h_seed[s], kSegEntries * 4)) || (rc = dev(d_seed[s], kSegEntries * 4)) ||
                (rc = pin(h_res[s], kSegEntries * 4)) || (rc = dev(d_res[s], kSegEntries * 4)))
                return rc;
            if (!st[s]) BKD_HIP(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
            if (!done[s]) BKD_HIP(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
        }
        ready = true;
        return BKD_OK;
    }
    int init_package() {
        if (pkg_ready) return BKD_OK;
        for (int s = 0, rc; s < 2; ++s)
            if ((rc = pin(h_aux[s], kAux)) || (rc = dev(d_aux[s], kAux)) || (rc = pin(h_frm[s], kAux)) ||
                (rc = dev(d_frm[s], kAux)))
                return rc;
        pkg_ready = true;
        return BKD_OK;
    }
    int init_verify() {
        if (fb_ready) return BKD_OK;
        for (int s = 0, rc; s < 2; ++s)
            if ((rc = pin(h_fb[s], sizeof(uint64_t))) || (rc = dev(d_fb[s], sizeof(uint64_t)))) return rc;
        fb_ready = true;
        return BKD_OK;
    }
    int init_requests() {
        if (rq_ready) return BKD_OK;
        for (int s = 0, rc; s < 2; ++s)
            if ((rc = pin(h_rq[s], kRqBytes)) || (rc = dev(d_rq[s], kRqBytes))) return rc;
        rq_ready = true;
        return BKD_OK;
    }
    int init_reframe() {
        if (lac_ready) return BKD_OK;
        for (int s = 0, rc; s < 2; ++s)
            if ((rc = pin(h_lac[s], kSegEntries * 8)) || (rc = dev(d_lac[s], kSegEntries * 8))) return rc;
        lac_ready = true;
        return BKD_OK;
    }
    ~HostStage() {  // (bkd_host_release: idle sets only, so no work of theirs is queued)
        for (void* h : pinned) (void)hipHostFree(h);
        for (void* d : device) (void)hipFree(d);
        for (int s = 0; s < 2; ++s) {
            if (st[s]) (void)hipStreamDestroy(st[s]);
            if (done[s]) (void)hipEventDestroy(done[s]);
        }
    }
};

// Host-resident batches from concurrent callers each take a staging set of their own (created on
// demand, at most BKD_HOST_STAGES per device, default 4; a caller beyond that waits for one), so
// one caller's gather and PCIe copies do not hold up another's (no global lock on the
// hot path). A set with the framed-entry buffers is ~0.4 GiB of pinned memory.
struct StagePool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::unique_ptr<HostStage>> all;
    std::vector<HostStage*> idle;
};
// Deliberately never destroyed: static destructors run after HIP's own teardown, where
// hipHostFree / hipStreamDestroy can crash or hang at exit; bkd_host_release frees idle sets instead.
StagePool* const g_stages = new StagePool[kMaxDevices];

size_t max_stages() {
    static const size_t m = [] {
        const char* v = getenv("BKD_HOST_STAGES");
        const int k = v ? atoi(v) : 4;
        return (size_t)std::max(1, std::min(64, k));
    }();
    return m;
}

// A staging set for the duration of one host-resident call.
class StageLease {
  public:
    explicit StageLease(int dev) : pool_(g_stages[dev]) {
        std::unique_lock<std::mutex> lk(pool_.mu);
        pool_.cv.wait(lk, [&] { return !pool_.idle.empty() || pool_.all.size() < max_stages(); });
        if (!pool_.idle.empty()) {
            hs_ = pool_.idle.back();
            pool_.idle.pop_back();
        } else {
            pool_.all.emplace_back(new HostStage());
            hs_ = pool_.all.back().get();
        }
    }
    ~StageLease() {
        {
            std::lock_guard<std::mutex> lk(pool_.mu);
            pool_.idle.push_back(hs_);
        }
        pool_.cv.notify_one();
    }
    HostStage& operator*() const { return *hs_; }

  private:
    StagePool& pool_;
    HostStage* hs_ = nullptr;
};

// A host-resident call on the GPU route: entered on the null stream, with a staging set leased for
// the call and its init() and the named init_*() groups run. rc: the first failure of any of these.
struct StagedCall : Call {
    std::optional<StageLease> lease;
    template <class... Init>
    explicit StagedCall(Init... more) : Call(nullptr) {
        if (rc) return;
        lease.emplace((int)(ds - g_dev));
        rc = (**lease).init();
        ((rc = rc ? rc : ((**lease).*more)()), ...);
    }
};

// Host copies into pinned staging (a pageable source, or a list of separate entry buffers such as a
// ByteBufList) run on the library's host pool (host_batch.hpp): one core copies ~10-20 GB/s, below
// PCIe Gen5's ~55. At most BKD_COPY_THREADS parts (default 8: 12 measured no better on the 16-core
// share of the GPU box, host verify of 1M separate 4 KiB frames 42.5 vs 43.4 GiB/s mean).
int copy_threads() {
    static const int t = [] {
        const char* v = getenv("BKD_COPY_THREADS");
        return v ? std::max(1, std::min(64, atoi(v))) : 8;
    }();
    return std::min(t, bkd::host::Pool::get().active());
}

// Bytes per copy-pool part (BKD_COPY_PART_KIB overrides the default).
size_t copy_part_bytes() {
    static const size_t b = [] {
        const char* v = getenv("BKD_COPY_PART_KIB");
        const long k = v ? atol(v) : 4096;
        return (size_t)std::max(64L, std::min(1L << 20, k)) << 10;
    }();
    return b;
}

// memcpy of one range on the copy pool (parts of >= copy_part_bytes()).
void parallel_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    bkd::host::Pool& pool = bkd::host::Pool::get();
    const int parts = (int)std::min<size_t>((size_t)copy_threads(), std::max<size_t>(1, n / copy_part_bytes()));
    const size_t per = (n + parts - 1) / parts;
    pool.run(parts, [&](int p) {
        const size_t a = std::min(n, per * (size_t)p), b = std::min(n, a + per);
        if (b > a) memcpy(dst + a, src + a, b - a);
    });
}

// Packs entries src[i] (len[i] bytes) back to back into dst; off[i] = where entry i landed.
// Split over the copy pool by bytes.
void gather_entries(const void* const* src, const uint32_t* len, uint64_t cnt, uint8_t* dst, uint64_t* off) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < cnt; ++i) {
        off[i] = at;
        at += len[i];
    }
    bkd::host::Pool& pool = bkd::host::Pool::get();
    const int parts = (int)std::min<uint64_t>((uint64_t)copy_threads(), std::max<uint64_t>(1, at / copy_part_bytes()));
    const uint64_t per = (at + parts - 1) / parts;
    pool.run(parts, [&](int p) {
        // entries whose first byte lies in [p*per, (p+1)*per)
        const uint64_t lo = per * (uint64_t)p, hi = lo + per;
        uint64_t i = (uint64_t)(std::lower_bound(off, off + cnt, lo) - off);
        for (; i < cnt && off[i] < hi; ++i)
            if (len[i]) memcpy(dst + off[i], src[i], len[i]);
    });
}

// Unsorted index: one device copy of the spanned bytes. The buffers are allocated with hipMalloc
// and released with hipFree: reusing stream-ordered (hipMallocAsync) allocations of this size for
// the copy gave wrong digests from the second call on (128-512 MiB spans, both pinned and pageable
// sources, with or without a sync after the copy; tools/diag_host_big.py, profiles/r03l_*), and
// hipMalloc'd buffers did not.
int host_batch_oneshot(DeviceState& ds, HostStage& hs, int algo, const uint8_t* h_base, uint64_t base_size,
                       const uint64_t* h_offsets, const uint32_t* h_lengths, uint64_t n, const uint32_t* h_seeds,
                       uint32_t seed_all, uint32_t* h_out) {
    hipStream_t st = hs.st[0];
    uint8_t* d_base = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t *d_len = nullptr, *d_seeds = nullptr, *d_out = nullptr;
    hipError_t e = hipSuccess;
    if (base_size) e = hipMalloc((void**)&d_base, base_size);
    if (e == hipSuccess) e = hipMalloc((void**)&d_off, n * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&d_len, n * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 4);
    if (e == hipSuccess && h_seeds) e = hipMalloc((void**)&d_seeds, n * 4);
    int rc = BKD_OK;
    if (e != hipSuccess) rc = fail(BKD_ERR_NOMEM, std::string("host batch staging: ") + hipGetErrorString(e));
    if (rc == BKD_OK && base_size) e = hipMemcpyAsync(d_base, h_base, base_size, hipMemcpyHostToDevice, st);
    if (rc == BKD_OK && e == hipSuccess) e = hipMemcpyAsync(d_off, h_offsets, n * 8, hipMemcpyHostToDevice, st);
    if (rc == BKD_OK && e == hipSuccess) e = hipMemcpyAsync(d_len, h_lengths, n * 4, hipMemcpyHostToDevice, st);
    if (rc == BKD_OK && e == hipSuccess && h_seeds) e = hipMemcpyAsync(d_seeds, h_seeds, n * 4, hipMemcpyHostToDevice, st);
    if (rc == BKD_OK && e != hipSuccess) rc = fail(BKD_ERR_HIP, std::string("host batch staging: ") + hipGetErrorString(e));
    if (rc == BKD_OK) rc = indexed_batch(ds, algo, d_base, base_size, d_off, d_len, n, d_seeds, seed_all, d_out, st);
    if (rc == BKD_OK) {
        e = hipMemcpyAsync(h_out, d_out, n * 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(BKD_ERR_HIP, std::string("host batch: ") + hipGetErrorString(e));
    }
    e = hipStreamSynchronize(st);
    if (rc == BKD_OK && e != hipSuccess) rc = fail(BKD_ERR_HIP, std::string("host batch: ") + hipGetErrorString(e));
    for (void* p : {(void*)d_base, (void*)d_off, (void*)d_len, (void*)d_seeds, (void*)d_out})
        if (p) (void)hipFree(p);
    return rc;
}

// The two-slot loop of every staged route. cut(i0, &bytes) returns the end of the segment that
// starts at entry i0 and its staged bytes; seg(s, i0, cnt, bytes) enqueues it on slot s = k % 2
// (copies in, the device sequence, copies out) and drain_slot(s, i0, cnt) hands a finished slot's
// results back, so one segment's gather and H2D overlap the other's kernels and D2H.
template <class Cut, class Seg, class Drain>
int staged_pipeline(HostStage& hs, uint64_t n, Cut&& cut, Seg&& seg, Drain&& drain_slot) {
    uint64_t pend_i0[2] = {0, 0}, pend_cnt[2] = {0, 0};
    bool busy[2] = {false, false};
    auto drain = [&](int s) -> int {  // wait for slot s and hand its results back
        if (!busy[s]) return BKD_OK;
        BKD_HIP(hipEventSynchronize(hs.done[s]));
        busy[s] = false;
        return drain_slot(s, pend_i0[s], pend_cnt[s]);
    };
    int rc = BKD_OK;
    uint64_t i0 = 0;
    for (int k = 0; i0 < n && rc == BKD_OK; ++k) {
        const int s = k & 1;
        uint64_t bytes = 0;
        const uint64_t i1 = cut(i0, &bytes);
        if ((rc = drain(s))) break;
        if ((rc = seg(s, i0, i1 - i0, bytes))) {
            (void)hipStreamSynchronize(hs.st[s]);  // copies of the failed segment may be queued
            break;
        }
        // every exit below goes through the final drains: no staging set returns to the pool with
        // copies or kernels of this call still queued on its streams
        const hipError_t e = hipEventRecord(hs.done[s], hs.st[s]);
        if (e != hipSuccess) {
            rc = fail(BKD_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
            (void)hipStreamSynchronize(hs.st[s]);
            break;
        }
        busy[s] = true;
        pend_i0[s] = i0;
        pend_cnt[s] = i1 - i0;
        i0 = i1;
    }
    const int r0 = drain(0), r1 = drain(1);
    return rc ? rc : (r0 ? r0 : r1);
}

// The contiguous route: segments cut by the span of the sorted offsets.
int host_batch_pipelined(DeviceState& ds, HostStage& hs, int algo, const uint8_t* h_base, const uint64_t* h_offsets,
                         const uint32_t* h_lengths, uint64_t n, const uint32_t* h_seeds, uint32_t seed_all,
                         uint32_t* h_out) {
    const bool pinned = pointer_type(h_base) == hipMemoryTypeHost;
    auto cut = [&](uint64_t i0, uint64_t* span) {
        const uint64_t b0 = h_offsets[i0];
        uint64_t i1 = i0, b1 = b0;
        while (i1 < n && i1 - i0 < HostStage::kSegEntries) {
            const uint64_t e1 = std::max<uint64_t>(b1, h_offsets[i1] + h_lengths[i1]);
            if (e1 - b0 > HostStage::kSeg && i1 > i0) break;
            b1 = e1;
            ++i1;
        }
        *span = b1 - b0;  // <= kSeg: longer entries arrive in pieces
        return i1;
    };
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t span) -> int {
        const uint64_t b0 = h_offsets[i0];
        for (uint64_t j = 0; j < cnt; ++j) {
            hs.h_off[s][j] = h_offsets[i0 + j] - b0;
            hs.h_len[s][j] = h_lengths[i0 + j];
        }
        if (h_seeds) memcpy(hs.h_seed[s], h_seeds + i0, cnt * 4);
        const uint8_t* src = h_base + b0;
        if (!pinned) {
            parallel_copy(hs.h_pin[s], src, span);
            src = hs.h_pin[s];
        }
        hipStream_t st = hs.st[s];
        hipError_t e = hipMemcpyAsync(hs.d_buf[s], src, span, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hs.d_off[s], hs.h_off[s], cnt * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hs.d_len[s], hs.h_len[s], cnt * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && h_seeds) e = hipMemcpyAsync(hs.d_seed[s], hs.h_seed[s], cnt * 4, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(BKD_ERR_HIP, std::string("host batch H2D: ") + hipGetErrorString(e));
        const int rc = indexed_batch(ds, algo, hs.d_buf[s], span, hs.d_off[s], hs.d_len[s], cnt,
                                     h_seeds ? hs.d_seed[s] : nullptr, seed_all, hs.d_res[s], st);
        if (rc) return rc;
        e = hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return fail(BKD_ERR_HIP, std::string("host batch D2H: ") + hipGetErrorString(e));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {  // hand the slot's digests back
        memcpy(h_out + i0, hs.h_res[s], cnt * 4);
        return BKD_OK;
    };
    return staged_pipeline(hs, n, cut, seg, drain);
}

// ---- DigestManager batch framing: the device sequences shared by the device- and host-resident
// entry points -------------------------------------------------------------------------------

// Package: header kernel (32 B BE header, header CRC as the payload's seed) -> payload CRCs through
// the direct kernel -> digest kernel (BE digest after the header, in a pass of its own: the payload
// groups storing it themselves measured 3 % slower on 1M x 4 KiB, profiles/r03m_ab_order*.log) — or
// the fused route, which folds the header inside the payload kernel. Out-of-range payload
// entries raise the stream's bounds flag.
// Fused route (4..64-lane groups, frames apart from the payload): each lane group builds its
// entry's header from the index arrays and folds header + payload in one pass, storing the digest
// (crc_package_fused_kernel); package_frame_kernel then writes every frame's header and digest.
// d_ledger_ids (bkd_digest_package_batch_ledgers): one ledger id per entry instead of ledger_id; the
// same routes and the same kernels, instantiated for the other id source.
// d_frames == nullptr (package_v2, which writes whole requests itself): only d_digests is wanted, and the
// fused route ends after its first kernel. The header-first route needs frames to write its headers to.

// Turns the ledger-id arguments into the package kernels' id source: f(bkd::LedgerPerEntry) when
// d_ledger_ids is given, f(bkd::OneLedger) otherwise.
template <class F>
int with_ledger_ids(int64_t ledger_id, const int64_t* d_ledger_ids, F&& f) {
    return d_ledger_ids ? f(bkd::LedgerPerEntry{d_ledger_ids}) : f(bkd::OneLedger{ledger_id});
}

int package_framed(DeviceState& ds, hipStream_t st, int algo, int64_t ledger_id, const int64_t* d_entry_ids,
                   const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                   uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                   void* d_frames, uint64_t frame_stride, uint32_t* d_digests,
                   const int64_t* d_ledger_ids = nullptr) {
    const uint32_t mac = mac_len(algo);
    const int lanes = auto_lanes(payload_size / n, n, ds.cus);
    const uint32_t* tab = ds.tables[algo][lane_index(lanes)];
    uint32_t* err = nullptr;
    int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    // The fused route when the frames are their own buffer (DigestManager's ByteBufList(header, data),
    // bench.py --config verify4k: 0.674 -> 0.659 ms per 1M 4 KiB entries); frames written in place in
    // front of their payloads keep the header-first route (0.821 vs 0.832 ms fused, profiles/r06r_*).
    const uint64_t fr0 = (uint64_t)(uintptr_t)d_frames, fr1 = fr0 + (n - 1u) * frame_stride + 32u + mac;
    const uint64_t pl0 = (uint64_t)(uintptr_t)d_payload, pl1 = pl0 + payload_size;
    const bool frames_apart = !d_frames || fr1 <= pl0 || pl1 <= fr0;
    return with_ledger_ids(ledger_id, d_ledger_ids, [&](auto lid) -> int {
        using Lid = decltype(lid);
        if (lanes >= 4 && frames_apart) {
            rc = with_lanes<4>(lanes, [&](auto g) -> int {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL((bkd::crc_package_fused_kernel<G, kPF, kNT, Lid>), dim3(group_blocks(ds, n, G)),
                                   dim3(bkd::kBlock), 0, st, (const uint8_t*)d_payload, payload_size, d_offsets, d_lengths,
                                   n, lid, d_entry_ids, d_lacs, d_length_fields, ds.tables[algo][lane_index(G)],
                                   d_digests, err, g_fold_sched.load());
                BKD_HIP(hipGetLastError());
                return BKD_OK;
            });
            if (rc || !d_frames) return rc;
            hipLaunchKernelGGL(bkd::package_frame_kernel<Lid>, dim3(blocks), dim3(256), 0, st, lid, d_entry_ids, d_lacs,
                               d_length_fields, d_digests, n, (uint8_t*)d_frames, frame_stride, mac);
            BKD_HIP(hipGetLastError());
            return BKD_OK;
        }
        if (!d_frames) return fail(BKD_ERR_INVALID_ARG, "the header-first package route needs a frame buffer");
        const unsigned hblocks = (unsigned)std::min<uint64_t>((n + 1023) / 1024, 2u * (uint64_t)ds.cus);
        hipLaunchKernelGGL(bkd::package_header_kernel<Lid>, dim3(hblocks), dim3(1024), 0, st, tab + 1024, lid,
                           d_entry_ids, d_lacs, d_length_fields, n, (uint8_t*)d_frames, frame_stride, d_digests);
        BKD_HIP(hipGetLastError());
        bkd::IndexedSrc src{n, d_offsets, d_lengths, d_digests, 0u, payload_size, d_digests};
        rc = dispatch_lanes(ds, lanes, algo, (const uint8_t*)d_payload, src, n, st, err);
        if (rc) return rc;
        hipLaunchKernelGGL(bkd::package_digest_kernel, dim3(blocks), dim3(256), 0, st, d_digests, n,
                           (uint8_t*)d_frames, frame_stride, mac);
        BKD_HIP(hipGetLastError());
        return BKD_OK;
    });
}

// V2 add requests (bkd_digest_package_batch_v2; DigestManager.java:126-167): the digests exactly as
// package_framed gets them (no frames wanted on its fused route; on the header-first route, which a
// forced one-lane geometry takes, its frames go to the stream's scratch), then package_v2_head_kernel
// (prefix, key, header and digest of every request) and package_v2_copy_kernel (the payloads under the
// threshold, one lane group per entry). Two passes over the small payloads; no host sync. (A kernel
// that copied each entry as its lane group folded it measured 14 % slower: DESIGN.md §3.)

// Lanes per entry of package_v2_copy_kernel: about eight 16-byte blocks per lane (two turns of its loop
// with four loads in flight), from 4 to 32 lanes. Measured at 4 KiB entries only: 32 lanes 2.47 ms per 1M
// against 2.51 at 8 and 2.62 at 4, flat from 16 up. A forced lane width
// (bkd_set_group_lanes) is the copy's too, its narrowest group for a one-lane geometry.
int v2_copy_lanes(uint64_t mean_len) {
    const int forced = g_forced_lanes.load();
    if (forced) return std::max(forced, 4);
    int g = 4;
    while (g < 32 && (uint64_t)g * 2u * 128u <= mean_len) g *= 2;
    return g;
}

int package_v2(DeviceState& ds, hipStream_t st, int algo, int64_t ledger_id, const int64_t* d_ledger_ids,
               const int64_t* d_entry_ids, const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
               uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
               const uint8_t* d_keys, uint64_t key_stride, uint32_t packet_header, uint32_t small_threshold,
               void* d_requests, uint64_t requests_size, const uint64_t* d_request_offsets, uint32_t* d_digests) {
    const uint32_t mac = mac_len(algo);
    const int lanes = auto_lanes(payload_size / n, n, ds.cus);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // the digests and the request kernels as one sequence
    uint32_t* err = nullptr;
    int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    const bkd::V2Requests rq{(uint8_t*)d_requests, requests_size, d_request_offsets, mac, small_threshold};
    uint8_t* frames = nullptr;
    if (lanes < 4) {
        const hipError_t e = sc.get(3, (size_t)n * (32u + mac), st, &frames);
        if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("package_v2 scratch: ") + hipGetErrorString(e));
    }
    rc = package_framed(ds, st, algo, ledger_id, d_entry_ids, d_lacs, d_length_fields, d_payload, payload_size,
                        d_offsets, d_lengths, n, frames, 32u + mac, d_digests, d_ledger_ids);
    if (rc) return rc;
    const unsigned hblocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 8u * (uint64_t)ds.cus);
    return with_ledger_ids(ledger_id, d_ledger_ids, [&](auto lid) -> int {
        using Lid = decltype(lid);
        hipLaunchKernelGGL(bkd::package_v2_head_kernel<Lid>, dim3(hblocks), dim3(256), 0, st, lid, d_entry_ids, d_lacs,
                           d_length_fields, d_lengths, d_digests, n, d_keys, key_stride, packet_header, rq, err);
        BKD_HIP(hipGetLastError());
        if (small_threshold == 0u) return BKD_OK;
        return with_lanes<4>(v2_copy_lanes(payload_size / n), [&](auto g) -> int {
            constexpr int G = decltype(g)::value;
            const uint64_t per_block = 256 / G;
            const unsigned cblocks = (unsigned)std::min<uint64_t>((n + per_block - 1) / per_block, 8u * (uint64_t)ds.cus);
            hipLaunchKernelGGL(bkd::package_v2_copy_kernel<G>, dim3(cblocks), dim3(256), 0, st, (const uint8_t*)d_payload,
                               payload_size, d_offsets, d_lengths, n, rq);
            BKD_HIP(hipGetLastError());
            return BKD_OK;
        });
    });
}

// Package with composite payloads (bkd_digest_package_batch_segments): every segment's zero-initialised
// register through the indexed path (seed ~0, as bkd_crc_batch_segments; direct kernel or chunked plan,
// out-of-range segments skipped and flagged there) -> package_segments_join_kernel (header fold, then
// the entry's segments joined with the byte-power table; the CSR clamped and checked) -> the frame
// writer of the fused package route. Each payload byte is read once and none is copied; no host sync.
// On the plan route one launch goes in front (segments_for_plan_kernel): the plan's short-entry launch
// loads whole 16-byte blocks for entries under 16 bytes, so those segments are handed to it as (0, 0)
// from the stream's scratch and the join kernel folds their bytes itself. No segment, wherever it lies
// in the payload, then makes the call read a byte outside [d_payload, d_payload + payload_size) but the
// plan's aligned lines around segments of 16 bytes and more, as for every indexed batch.
int package_segments(DeviceState& ds, hipStream_t st, int algo, int64_t ledger_id, const int64_t* d_ledger_ids,
                     const int64_t* d_entry_ids, const int64_t* d_lacs, const int64_t* d_length_fields,
                     const void* d_payload, uint64_t payload_size, const uint64_t* d_seg_offsets,
                     const uint32_t* d_seg_lengths, uint64_t nseg, const uint64_t* d_seg_first, uint64_t n,
                     void* d_frames, uint64_t frame_stride, uint32_t* d_digests) {
    const uint32_t mac = mac_len(algo);
    // the segments' route, decided once for the call; a payload under 16 bytes holds only segments the
    // join folds itself and never takes the plan (whose (0, 0) entries load base[0, 16))
    const int route = (payload_size < 16u || indexed_direct(payload_size)) ? 0 : 1;
    Carver cv;
    const size_t o_crc = cv.take((size_t)std::max<uint64_t>(nseg, 1) * 4),
                 o_off = cv.take(route == 1 ? (size_t)nseg * 8 : 0), o_len = cv.take(route == 1 ? (size_t)nseg * 4 : 0);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // held across the nested plan (slot 0)
    uint8_t* seg = nullptr;
    hipError_t e = sc.get(2, cv.used, st, &seg);
    if (e == hipSuccess) e = sc.flag(st);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("segment scratch: ") + hipGetErrorString(e));
    uint32_t* segcrc = Carver::at<uint32_t>(seg, o_crc);
    if (nseg) {
        const uint64_t* offs = d_seg_offsets;
        const uint32_t* lens = d_seg_lengths;
        if (route == 1) {
            uint64_t* poff = Carver::at<uint64_t>(seg, o_off);
            uint32_t* plen = Carver::at<uint32_t>(seg, o_len);
            const unsigned pblocks = (unsigned)std::min<uint64_t>((nseg + 255) / 256, 8u * (uint64_t)ds.cus);
            hipLaunchKernelGGL(bkd::segments_for_plan_kernel, dim3(pblocks), dim3(256), 0, st, d_seg_offsets, d_seg_lengths,
                               nseg, payload_size, poff, plen);
            BKD_HIP(hipGetLastError());
            offs = poff;
            lens = plen;
        }
        const int rc = indexed_batch(ds, algo, (const uint8_t*)d_payload, payload_size, offs, lens, nseg, nullptr,
                                     0xFFFFFFFFu, segcrc, st, nullptr, 0, route);
        if (rc) return rc;
    }
    const uint32_t* x32tab = ds.tables[algo][lane_index(4)] + 1024;  // x^32 operator, 4 x 256
    const uint64_t ntiles = (n + bkd::kSegJoinBlock - 1) / bkd::kSegJoinBlock;
    const unsigned jblocks = (unsigned)std::min<uint64_t>(ntiles, 8u * (uint64_t)ds.cus);
    hipLaunchKernelGGL(bkd::package_segments_join_kernel, dim3(jblocks), dim3(bkd::kSegJoinBlock), 0, st, x32tab,
                       ds.xp8[algo], bkd::gf2::poly(algo), ledger_id, d_ledger_ids, d_entry_ids, d_lacs, d_length_fields,
                       (const uint8_t*)d_payload, payload_size, d_seg_offsets, d_seg_lengths, segcrc, d_seg_first, n, nseg,
                       d_digests, sc.err);
    BKD_HIP(hipGetLastError());
    const unsigned blocks = (unsigned)((n + 255) / 256);
    return with_ledger_ids(ledger_id, d_ledger_ids, [&](auto lid) -> int {
        hipLaunchKernelGGL(bkd::package_frame_kernel<decltype(lid)>, dim3(blocks), dim3(256), 0, st, lid, d_entry_ids,
                           d_lacs, d_length_fields, d_digests, n, (uint8_t*)d_frames, frame_stride, mac);
        BKD_HIP(hipGetLastError());
        return BKD_OK;
    });
}

// Verify (bkd_digest_verify_batch and bkd_entrylog_verify): header CRCs -> payload CRCs seeded
// with them through the indexed path (chunked plan for large ragged batches) -> compare. Batches
// that take the plan route first run a gate over the frame lengths: when every frame is within
// PlanRun::in_band of the first, the fused kernel verifies each frame whole (header, payload and
// compare in one pass over it) and the header / plan / finish kernels return at once; otherwise
// the fused kernel returns and they run. Both give the same statuses; the device decides, no sync.
// The read requests of bkd_digest_verify_requests (device arrays; include/bkdigest.h).
// expanded (the host-resident form's staged segments): exp_lid / exp_eid / req_of hold the per-entry
// expectations already, no expansion runs, and `first` / `first_bad` are what req_of's request
// indices refer to (one request 0 per segment: the host computes the prefixes from the statuses).
struct Requests {
    uint64_t nreq;
    const uint64_t* first;
    const int64_t *ledger_ids, *first_entry_ids;
    const uint32_t* flags;
    uint64_t* first_bad;
    const int64_t *exp_lid = nullptr, *exp_eid = nullptr;
    const uint32_t* req_of = nullptr;
};

// rq (bkd_digest_verify_requests): per-request ledger ids, first entry ids, skip flags and verified
// prefixes instead of ledger_id / first_entry_id / id_checks / d_first_bad. One more launch at the
// head (request_expand_kernel: the CSR into per-entry expectations in the stream's scratch, the CSR
// checked, the prefixes initialised); then the same gate, the same two routes and the same kernels,
// instantiated for bkd::RequestIds where one read's are for bkd::OneRead.
int verify_framed(DeviceState& ds, hipStream_t st, int algo, int64_t ledger_id, int64_t first_entry_id,
                  int id_checks, const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                  const uint32_t* d_lengths, uint64_t n, int32_t* d_status, uint64_t* d_first_bad,
                  const Requests* rq = nullptr) {
    const uint32_t mac = mac_len(algo);
    if (n == 0) {
        if (!rq) BKD_HIP(hipMemsetAsync(d_first_bad, 0, sizeof(uint64_t), st));
        else if (rq->nreq) BKD_HIP(hipMemsetAsync(rq->first_bad, 0, rq->nreq * sizeof(uint64_t), st));
        return BKD_OK;
    }
    const uint32_t* x32tab = ds.tables[algo][lane_index(4)] + 1024;  // x^32 operator, 4 x 256
    const unsigned blocks = (unsigned)((n + 255) / 256);
    Carver cv;
    const size_t o_seeds = cv.take(n * 4), o_plen = cv.take(n * 4), o_poff = cv.take(n * 8), o_exp = cv.take(n * 4),
                 o_pre = cv.take(n * 4);
    // requests: expected ledger and entry id and the request (bit 31: skip the entry-id check) per
    // entry, and the word the gate stores n into in d_first_bad's place
    const bool expand = rq && !rq->exp_lid;
    const size_t o_xlid = cv.take(expand ? n * 8 : 0), o_xeid = cv.take(expand ? n * 8 : 0),
                 o_req = cv.take(expand ? n * 4 : 0), o_fbw = cv.take(rq ? 8 : 0);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // held across the nested plan (slot 0)
    uint8_t* sb = nullptr;
    hipError_t e = sc.get(1, cv.used, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("verify scratch: ") + hipGetErrorString(e));
    uint32_t* seeds = Carver::at<uint32_t>(sb, o_seeds);
    uint32_t* plen = Carver::at<uint32_t>(sb, o_plen);
    uint64_t* poff = Carver::at<uint64_t>(sb, o_poff);
    uint32_t* expect = Carver::at<uint32_t>(sb, o_exp);
    uint32_t* pre = Carver::at<uint32_t>(sb, o_pre);
    bkd::RequestIds rids{};
    if (rq) d_first_bad = Carver::at<uint64_t>(sb, o_fbw);
    if (rq && !expand) rids = bkd::RequestIds{rq->exp_lid, rq->exp_eid, rq->req_of, rq->first, (unsigned long long*)rq->first_bad};
    if (expand) {
        uint32_t* err = nullptr;
        const int rc = bounds_flag(ds, st, &err);
        if (rc) return rc;
        int64_t *xlid = Carver::at<int64_t>(sb, o_xlid), *xeid = Carver::at<int64_t>(sb, o_xeid);
        uint32_t* req_of = Carver::at<uint32_t>(sb, o_req);
        rids = bkd::RequestIds{xlid, xeid, req_of, rq->first, (unsigned long long*)rq->first_bad};
        const unsigned xblocks =
            (unsigned)std::min<uint64_t>((std::max(n, rq->nreq) + 255) / 256, 8u * (uint64_t)ds.cus);
        hipLaunchKernelGGL(bkd::request_expand_kernel, dim3(xblocks), dim3(256), 0, st, rq->first, rq->nreq, n,
                           rq->ledger_ids, rq->first_entry_ids, rq->flags, xlid, xeid, req_of,
                           (unsigned long long*)rq->first_bad, err);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(BKD_ERR_HIP, hipGetErrorString(e));
    }
    // the fused route where the payloads would take the plan (large batches; the direct kernel's small
    // ones keep the three-kernel sequence)
    // — and, as the plan's own near-uniform gate, only where one frame per group uses the plan's lane
    // count: a few huge frames need the plan's chunks to fill the chip
    // the payloads' route, decided once for the whole call (a second read of the plan mode
    // could send them to the direct kernel, which ignores the gate, after the fused kernel ran)
    const int route = indexed_direct(framed_size) ? 0 : 1;
    const int fused_lanes = auto_lanes(framed_size / n, n, ds.cus);
    const bool fused = route == 1 && fused_lanes == g_plan_lanes.load();
    uint32_t* vflag = nullptr;
    uint32_t vepoch = 0;
    if (fused) {
        e = sc.word(sc.vflag, st);
        if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("verify gate: ") + hipGetErrorString(e));
        vflag = sc.vflag;
        if (++sc.vepoch == 0u) ++sc.vepoch;  // 0 is the word's initial value
        vepoch = sc.vepoch;
        const unsigned gblocks = (unsigned)std::min<uint64_t>((n + 1023) / 1024, (uint64_t)ds.cus);
        hipLaunchKernelGGL(bkd::verify_gate_kernel, dim3(gblocks), dim3(1024), 0, st, d_lengths, n, d_first_bad, vflag,
                           vepoch);
    }
    // the launches that take the ids, written once for either source
    auto run = [&](auto ids) -> int {
        using Ids = decltype(ids);
        if (fused) {
            // one kernel per lane count (crc_verify_fused_kernel); a forced one-lane geometry takes its
            // narrowest group, 4
            const int rc = with_lanes<4>(fused_lanes == 1 ? 4 : fused_lanes, [&](auto g) -> int {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL((bkd::crc_verify_fused_kernel<G, kPF, kNT, Ids>), dim3(group_blocks(ds, n, G)),
                                   dim3(bkd::kBlock), 0, st, (const uint8_t*)d_framed, framed_size, d_offsets, d_lengths,
                                   n, mac, ids, ds.tables[algo][lane_index(G)], d_status, vflag, vepoch,
                                   g_fold_sched.load());
                const hipError_t le = hipGetLastError();
                return le == hipSuccess ? BKD_OK : fail(BKD_ERR_HIP, hipGetErrorString(le));
            });
            if (rc) return rc;
        }
        const unsigned hblocks = (unsigned)std::min<uint64_t>((n + 1023) / 1024, 2u * (uint64_t)ds.cus);
        hipLaunchKernelGGL(bkd::verify_header_kernel<Ids>, dim3(hblocks), dim3(1024), 0, st, x32tab,
                           (const uint8_t*)d_framed, framed_size, d_offsets, d_lengths, n, mac, ids, seeds, poff, plen,
                           expect, pre, vflag, vepoch);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(BKD_ERR_HIP, hipGetErrorString(e));
        // payload CRCs land in d_status, then verify_finish turns them into status codes
        const int rc = indexed_batch(ds, algo, (const uint8_t*)d_framed, framed_size, poff, plen, n, seeds, 0,
                                     reinterpret_cast<uint32_t*>(d_status), st, vflag, vepoch, route);
        if (rc) return rc;
        hipLaunchKernelGGL(bkd::verify_finish_kernel<Ids>, dim3(blocks), dim3(256), 0, st, expect, pre, n, d_status, ids,
                           vflag, vepoch);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(BKD_ERR_HIP, hipGetErrorString(e));
        return BKD_OK;
    };
    return rq ? run(rids)
              : run(bkd::OneRead{ledger_id, first_entry_id, id_checks, (unsigned long long*)d_first_bad});
}

// Reframe (bkd_digest_reframe_batch): the verify sequence above (unless trusted), then one thread per
// frame writes the new LAC and old digest ^ R(LAC difference) * x^(8 * payload length) for the frames
// whose status is OK (reframe_frame_kernel) — no second pass over the payloads. Trusted: the kernel
// takes the status from each header itself and no payload byte is read at all.
int reframe_framed(DeviceState& ds, hipStream_t st, int algo, int64_t ledger_id, int64_t first_entry_id,
                   int id_checks, bool trusted, void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                   const uint32_t* d_lengths, uint64_t n, const int64_t* d_new_lacs, void* d_out_frames,
                   uint64_t frame_stride, uint32_t* d_digests, int32_t* d_status, uint64_t* d_first_bad) {
    const uint32_t mac = mac_len(algo);
    if (n == 0) {
        BKD_HIP(hipMemsetAsync(d_first_bad, 0, sizeof(uint64_t), st));
        return BKD_OK;
    }
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // verify and reframe enqueued as one sequence
    if (!trusted) {
        const int rc = verify_framed(ds, st, algo, ledger_id, first_entry_id, id_checks, d_framed, framed_size,
                                     d_offsets, d_lengths, n, d_status, d_first_bad);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(bkd::reframe_first_bad_kernel, dim3(1), dim3(1), 0, st, d_first_bad, n);
        BKD_HIP(hipGetLastError());
    }
    const uint32_t* x32tab = ds.tables[algo][lane_index(4)] + 1024;  // x^32 operator, 4 x 256
    const uint64_t ntiles = (n + bkd::kReframeBlock - 1) / bkd::kReframeBlock;
    const unsigned blocks = (unsigned)std::min<uint64_t>(ntiles, 8u * (uint64_t)ds.cus);
    hipLaunchKernelGGL(trusted ? bkd::reframe_frame_kernel<true> : bkd::reframe_frame_kernel<false>, dim3(blocks),
                       dim3(bkd::kReframeBlock), 0, st, x32tab, ds.xp8[algo], bkd::gf2::poly(algo), (uint8_t*)d_framed,
                       framed_size, d_offsets, d_lengths, n, mac, d_new_lacs, ledger_id, first_entry_id, id_checks,
                       (uint8_t*)d_out_frames, frame_stride, d_digests, d_status, (unsigned long long*)d_first_bad);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// ---- host-resident framed batches (BatchedReadOp's ByteBufList, PendingAddOp's payloads) ----
// Entries are separate host buffers. Segments of <= kSeg bytes / kSegEntries entries are gathered
// back to back into the slot's pinned buffer on the copy pool, copied H2D on the slot's stream,
// run through the device sequence, and the per-entry results copied D2H; slot k % 2 alternates
// so one segment's gather and H2D overlap the other's kernels and D2H.
template <class Seg, class Drain>
int host_segments(HostStage& hs, const uint32_t* h_lengths, uint64_t n, uint64_t max_entries, Seg&& seg,
                  Drain&& drain_slot) {
    // every entry fits a segment, checked before any work is enqueued
    for (uint64_t i = 0; i < n; ++i)
        if (h_lengths[i] > HostStage::kSeg)
            return fail(BKD_ERR_INVALID_ARG, "host entry " + std::to_string(i) + " is larger than 64 MiB");
    auto cut = [&](uint64_t i0, uint64_t* bytes) {  // by summed lengths: the entries are gathered back to back
        uint64_t i1 = i0;
        while (i1 < n && i1 - i0 < max_entries && (i1 == i0 || *bytes + h_lengths[i1] <= HostStage::kSeg))
            *bytes += h_lengths[i1++];
        return i1;
    };
    return staged_pipeline(hs, n, cut, seg, drain_slot);
}

// A segment of separate entry buffers into slot s: gathered back to back into the pinned buffer,
// then the bytes, where each entry landed and the lengths copied H2D on the slot's stream.
int stage_entries(HostStage& hs, int s, const void* const* ptrs, const uint32_t* lens, uint64_t i0, uint64_t cnt,
                  uint64_t bytes) {
    gather_entries(ptrs + i0, lens + i0, cnt, hs.h_pin[s], hs.h_off[s]);
    BKD_HIP(hipMemcpyAsync(hs.d_buf[s], hs.h_pin[s], bytes, hipMemcpyHostToDevice, hs.st[s]));
    BKD_HIP(hipMemcpyAsync(hs.d_off[s], hs.h_off[s], cnt * 8, hipMemcpyHostToDevice, hs.st[s]));
    BKD_HIP(hipMemcpyAsync(hs.d_len[s], lens + i0, cnt * 4, hipMemcpyHostToDevice, hs.st[s]));
    return BKD_OK;
}

// Folds slot s's first_bad (relative to its segment [i0, i0 + cnt)) into the call's.
void merge_first_bad(const HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t* h_first_bad) {
    const uint64_t fb = *hs.h_fb[s];
    if (fb < cnt && i0 + fb < *h_first_bad) *h_first_bad = i0 + fb;
}

// ---- per-call resume (IntHash.resume) -------------------------------------------------------
// Host buffers up to this many bytes take the CPU route (host_crc.cpp); larger ones the GPU
// through pinned staging. Default from the per-call sweep (profiles/r02_call_latency.log): 4 MiB
// with the 128-bit fold (one core ~210 us vs ~230 us by gather + PCIe + launch for a pageable
// buffer), 64 MiB with the AVX-512 fold (one core then keeps pace with PCIe). UINT64_MAX = unset.
std::atomic<uint64_t> g_cpu_route_max{UINT64_MAX};

uint64_t cpu_route_max() {
    const uint64_t v = g_cpu_route_max.load(std::memory_order_relaxed);
    if (v != UINT64_MAX) return v;
    return bkd::host::has_wide_fold() ? (64ull << 20) : (4ull << 20);
}

// Per-call resumes longer than this run as consecutive pieces, each resuming from the last
// (entry lengths are 32-bit in the batch kernels).
constexpr uint64_t kResumePiece = 1ull << 31;

// Route of the host-resident batches (bkd_crc_batch_host, bkd_digest_*_batch_host): 0 automatic,
// 1 CPU (host_batch.cpp over the host pool), 2 GPU (pinned staging, PCIe, the device sequence).
std::atomic<int> g_host_route{0};

// The automatic choice, from the measured crossover (profiles/r03_host_route.log): a
// host-resident batch through the GPU is bound by PCIe (~51 GiB/s) and, for separate entry buffers,
// by the host gather into pinned staging; the CPU route scales with the cores until host memory
// bandwidth. EPYC 9575F, 1M framed 4 KiB entries: GPU route 46.6 GiB/s verify / 50.6 contiguous;
// CPU route 19.0 / 36.9 / 68.3 / 130 / 228 GiB/s verify at 1 / 2 / 4 / 8 / 16 threads (contiguous
// 30.9 / 61.6 / 106 / 172 / 244) -> the CPU route from 3 threads with the AVX-512 fold. Without it
// (128-bit fold, unmeasured on the box) from 4. BKD_HOST_ROUTE_MIN_THREADS overrides.
int cpu_route_min_threads() {
    static const int t = [] {
        if (const char* v = getenv("BKD_HOST_ROUTE_MIN_THREADS")) return std::max(1, atoi(v));
        return bkd::host::has_wide_fold() ? 3 : 4;
    }();
    return t;
}

// 1 = CPU, 2 = GPU, < 0 = error (a GPU route forced without a device).
// oversize: the batch holds an entry longer than a staging segment, which the framed GPU route
// refuses; the automatic route then takes the CPU (the provider never fails where it can compute).
int host_route(bool oversize = false) {
    const int r = g_host_route.load(std::memory_order_relaxed);
    if (r == 1 || (r == 0 && oversize)) return 1;
    if (visible_devices() <= 0)  // the provider never fails for lack of a device
        return r == 2 ? fail(BKD_ERR_NO_DEVICE, "no HIP device (host batch route forced to the GPU)") : 1;
    if (r == 2) return 2;
    return bkd::host::Pool::get().active() >= cpu_route_min_threads() ? 1 : 2;
}

// The framed host routes' choice (host_route): oversize when an entry is longer than a staging segment.
int framed_host_route(const uint32_t* lengths, uint64_t n) {
    bool oversize = false;
    for (uint64_t i = 0; i < n && !oversize; ++i) oversize = lengths[i] > HostStage::kSeg;
    return host_route(oversize);
}

int cpu_resume(int algo, uint32_t current, const void* p, uint64_t len, uint32_t* out) {
    *out = ~bkd::host::fold(algo, ~current, (const uint8_t*)p, len);  // >= 4 MiB: over the host pool
    return BKD_OK;
}

// Device scratch of one synchronous per-call resume, pooled per device (no per-thread state
// that outlives its thread, no allocation on the hot path after the first calls).
struct CallScratch {
    uint64_t* d_off = nullptr;
    uint32_t* d_len = nullptr;
    uint32_t* h_out = nullptr;  // pinned: [0] result, [1] length for the plan path
};
struct CallPool {
    std::mutex mu;
    std::vector<CallScratch*> free;
};
CallPool g_call_pool[kMaxDevices];

int call_acquire(int dev, hipStream_t st, CallScratch** out) {
    CallPool& p = g_call_pool[dev];
    {
        std::lock_guard<std::mutex> lk(p.mu);
        if (!p.free.empty()) {
            *out = p.free.back();
            p.free.pop_back();
            return BKD_OK;
        }
    }
    std::unique_ptr<CallScratch> c(new CallScratch());
    BKD_HIP(hipMalloc((void**)&c->d_off, 8));
    BKD_HIP(hipMalloc((void**)&c->d_len, 4));
    BKD_HIP(hipHostMalloc((void**)&c->h_out, 8, hipHostMallocDefault));
    BKD_HIP(hipMemsetAsync(c->d_off, 0, 8, st));
    *out = c.release();
    return BKD_OK;
}

void call_release(int dev, CallScratch* c) {
    std::lock_guard<std::mutex> lk(g_call_pool[dev].mu);
    g_call_pool[dev].free.push_back(c);
}

int resume_device(int algo, uint32_t current, const void* ptr, uint64_t len, hipStream_t st, uint32_t* out) {
    Call call(st);
    int rc = call.rc;
    if (rc) return rc;
    DeviceState* const ds = call.ds;
    const int dev = (int)(ds - g_dev);
    CallScratch* c = nullptr;
    if ((rc = call_acquire(dev, st, &c))) return rc;
    const uint32_t l32 = (uint32_t)len;
    // the kernel stores the digest straight into the pinned host word (no D2H copy on the call's
    // critical path; visible to the host once the stream has synchronised)
    uint32_t* res = c->h_out;
    if (len < (1u << 20)) {  // one group: the entry as a uniform batch of one
        bkd::UniformSrc src{1, len, l32, nullptr, current, res};
        rc = dispatch_lanes(*ds, auto_lanes(len, 1, ds->cus), algo, (const uint8_t*)ptr, src, 1, st);
    } else {  // large: the chunked plan spreads it over the chip
        c->h_out[1] = l32;
        const hipError_t e = hipMemcpyAsync(c->d_len, c->h_out + 1, 4, hipMemcpyHostToDevice, st);
        rc = e == hipSuccess ? launch_plan(*ds, algo, (const uint8_t*)ptr, len, c->d_off, c->d_len, 1, nullptr,
                                           current, res, st, false, false)
                             : fail(BKD_ERR_HIP, hipGetErrorString(e));
    }
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(BKD_ERR_HIP, std::string("resume: ") + hipGetErrorString(e));
        else *out = __atomic_load_n(c->h_out, __ATOMIC_ACQUIRE);
    }
    call_release(dev, c);
    return rc;
}

// stage_entries as the `stage` argument of the staged routes below: entry i is the one buffer ptrs[i].
auto entry_buffers(const void* const* ptrs, const uint32_t* lens) {
    return [=](HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t bytes) {
        return stage_entries(hs, s, ptrs, lens, i0, cnt, bytes);
    };
}

// Composite entries of a host-resident call (bkd_digest_package_batch_segments_host,
// bkd_crc_batch_segments_host): entry i = segments first[i] .. first[i+1]-1, segment k its own host
// buffer. at[k] = where segment k starts in the concatenation of the whole batch, so an entry's bytes
// are at[first[i+1]] - at[first[i]] (entry_len[i], saturated at 2^32 - 1) and a staged run of entries
// is one run of segments laid end to end: every staged entry is contiguous.
struct HostSegments {
    const void* const* ptrs;
    const uint32_t* lens;
    const uint64_t* first;
    std::vector<uint64_t> at;
    std::vector<uint32_t> entry_len;
    HostSegments(const void* const* ptrs_, const uint32_t* lens_, uint64_t nseg, const uint64_t* first_, uint64_t n)
        : ptrs(ptrs_), lens(lens_), first(first_), at(nseg + 1), entry_len(n) {
        at[0] = 0;
        for (uint64_t k = 0; k < nseg; ++k) at[k + 1] = at[k] + lens[k];
        for (uint64_t i = 0; i < n; ++i)
            entry_len[i] = (uint32_t)std::min<uint64_t>(at[first[i + 1]] - at[first[i]], 0xFFFFFFFFu);
    }
    // The `stage` argument of the staged routes: entries [i0, i0 + cnt) gathered into slot s's pinned
    // buffer on the copy pool (split by bytes), then the bytes, where each entry landed and the
    // entries' summed lengths copied H2D on the slot's stream.
    int operator()(HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t bytes) const {
        const uint64_t k0 = first[i0], k1 = first[i0 + cnt], b0 = at[k0];
        for (uint64_t j = 0; j < cnt; ++j) hs.h_off[s][j] = at[first[i0 + j]] - b0;
        uint8_t* dst = hs.h_pin[s];
        const int parts = (int)std::min<uint64_t>((uint64_t)copy_threads(), std::max<uint64_t>(1, bytes / copy_part_bytes()));
        const uint64_t per = (bytes + parts - 1) / parts;
        bkd::host::Pool::get().run(parts, [&](int p) {
            // segments whose first byte lies in [b0 + p*per, b0 + (p+1)*per)
            const uint64_t lo = b0 + per * (uint64_t)p, hi = lo + per;
            uint64_t k = (uint64_t)(std::lower_bound(at.data() + k0, at.data() + k1, lo) - at.data());
            for (; k < k1 && at[k] < hi; ++k)
                if (lens[k]) memcpy(dst + (at[k] - b0), ptrs[k], lens[k]);
        });
        if (bytes) BKD_HIP(hipMemcpyAsync(hs.d_buf[s], hs.h_pin[s], bytes, hipMemcpyHostToDevice, hs.st[s]));
        BKD_HIP(hipMemcpyAsync(hs.d_off[s], hs.h_off[s], cnt * 8, hipMemcpyHostToDevice, hs.st[s]));
        BKD_HIP(hipMemcpyAsync(hs.d_len[s], entry_len.data() + i0, cnt * 4, hipMemcpyHostToDevice, hs.st[s]));
        return BKD_OK;
    }
};

// The CSR of a host-resident call, before any work: `name` (req_first, seg_first) starts at 0, never
// decreases over its `count` units (`noun`: a request, an entry) and ends at `total` (BKD_ERR_INVALID_ARG
// otherwise); `count_name` and `total_name` are what the header calls the two.
int check_csr(const char* name, const char* noun, const uint64_t* first, uint64_t count, const char* count_name,
              uint64_t total, const char* total_name) {
    if (first[0] != 0u) return fail(BKD_ERR_INVALID_ARG, std::string(name) + "[0] is not 0");
    for (uint64_t i = 0; i < count; ++i)
        if (first[i + 1] < first[i])
            return fail(BKD_ERR_INVALID_ARG, std::string(name) + " decreases at " + noun + " " + std::to_string(i));
    if (first[count] != total)
        return fail(BKD_ERR_INVALID_ARG, std::string(name) + "[" + count_name + "] is not " + total_name);
    return BKD_OK;
}

// Every index names a row of a table of nkeys keys; `noun`: what an index belongs to (a request, an entry).
int check_key_index(const char* noun, const uint32_t* index, uint64_t count, uint64_t nkeys) {
    for (uint64_t i = 0; i < count; ++i)
        if (index[i] >= nkeys)
            return fail(BKD_ERR_INVALID_ARG, std::string(noun) + " " + std::to_string(i) + " names a key outside the table");
    return BKD_OK;
}

// Null-pointer checks and the CSR of the host-resident composite calls, before any work.
int check_host_segments(const void* const* h_seg_ptrs, const uint32_t* h_seg_lengths, uint64_t nseg,
                        const uint64_t* h_seg_first, uint64_t n) {
    if (!h_seg_first || (nseg && (!h_seg_ptrs || !h_seg_lengths))) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_csr("seg_first", "entry", h_seg_first, n, "n", nseg, "nseg")) return rc;
    for (uint64_t k = 0; k < nseg; ++k)
        if (h_seg_lengths[k] && !h_seg_ptrs[k]) return fail(BKD_ERR_INVALID_ARG, "null segment " + std::to_string(k));
    return BKD_OK;
}

// A null entry pointer is legal only for an empty entry; `noun` is what the form calls its entries.
int check_host_entries(const char* noun, const void* const* ptrs, const uint32_t* lens, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i] && !ptrs[i]) return fail(BKD_ERR_INVALID_ARG, std::string("null ") + noun + " " + std::to_string(i));
    return BKD_OK;
}

// The V2 forms' scalars, device- and host-resident, CRC and MAC: checked before n, so an empty batch too.
int check_v2_args(uint64_t key_stride, uint32_t flags) {
    if (key_stride != 0u && key_stride < 20u) return fail(BKD_ERR_INVALID_ARG, "key_stride must be 0 or at least 20");
    return flags > 0xFFFFu ? fail(BKD_ERR_INVALID_ARG, "flags must fit 16 bits") : BKD_OK;
}

// The V2 host forms' entries: a payload as check_host_entries has it, and every entry a request buffer
// (not check_host_entries: the first fault of either kind is the one named).
int check_v2_entries(const void* const* payloads, const uint32_t* lens, void* const* requests, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && !payloads[i]) return fail(BKD_ERR_INVALID_ARG, "null payload " + std::to_string(i));
        if (!requests[i]) return fail(BKD_ERR_INVALID_ARG, "null request " + std::to_string(i));
    }
    return BKD_OK;
}

// A frame's `head` = 32 + digest length bytes fit frame_stride; bounded (the host-resident forms, whose
// GPU route lands the frames in the kAux-byte staging buffers): and frame_stride is at most 4096.
int check_frame_stride(uint64_t head, uint64_t frame_stride, bool bounded) {
    if (bounded && (frame_stride < head || frame_stride > 4096u))
        return fail(BKD_ERR_INVALID_ARG, "frame_stride must be in [32 + digest length, 4096]");
    return frame_stride < head ? fail(BKD_ERR_INVALID_ARG, "frame_stride < 32 + digest length") : BKD_OK;
}

// The GPU route of the host-resident package forms, CRC and MAC (h_ledger_ids: one ledger id per entry,
// staged as a fourth aux array; else the launch's one ledger for all). stage(hs, s, i0, cnt, bytes) puts
// entries [i0, i0 + cnt) back to back into slot s (entry_buffers, HostSegments); h_lengths[i] = entry i's bytes.
// launch(ds, hs, s, d_ids, d_ledger_ids, cnt, bytes, dev_stride) enqueues the device sequence over slot s
// (crc_package, bkd_digest_package_batch_mac_host's): entry ids, LACs and length fields at d_ids, d_ids + cnt,
// d_ids + 2 * cnt, frame j to d_frm + j * dev_stride, digests (if it makes any: `digests`) to d_res.
// out(frames, digests, i0, cnt) takes a finished segment's results from the pinned landing buffers:
// frame j of entries [i0, i0 + cnt) at frames + j * dev_stride (host_frames: into the caller's frame array;
// bkd_digest_package_batch_v2_host: into its requests).
template <class Stage, class Launch, class Out>
int package_host_staged(const int64_t* h_ledger_ids, const int64_t* h_entry_ids, const int64_t* h_lacs,
                        const int64_t* h_length_fields, const Stage& stage, const uint32_t* h_lengths, uint64_t n,
                        const Launch& launch, uint64_t dev_stride, bool digests, const Out& out) {
    StagedCall call(&HostStage::init_package);
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    const uint64_t fields = h_ledger_ids ? 4 : 3;
    const uint64_t max_entries = std::min<uint64_t>(HostStage::kSegEntries, HostStage::kAux / dev_stride);
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        const hipStream_t st = hs.st[s];
        int r = stage(hs, s, i0, cnt, bytes);
        if (r) return r;
        int64_t* aux = reinterpret_cast<int64_t*>(hs.h_aux[s]);
        memcpy(aux, h_entry_ids + i0, cnt * 8);
        memcpy(aux + cnt, h_lacs + i0, cnt * 8);
        memcpy(aux + 2 * cnt, h_length_fields + i0, cnt * 8);
        if (h_ledger_ids) memcpy(aux + 3 * cnt, h_ledger_ids + i0, cnt * 8);
        BKD_HIP(hipMemcpyAsync(hs.d_aux[s], aux, cnt * 8 * fields, hipMemcpyHostToDevice, st));
        const int64_t* d_aux = reinterpret_cast<const int64_t*>(hs.d_aux[s]);
        r = launch(*call.ds, hs, s, d_aux, h_ledger_ids ? d_aux + 3 * cnt : nullptr, cnt, bytes, dev_stride);
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_frm[s], hs.d_frm[s], cnt * dev_stride, hipMemcpyDeviceToHost, st));
        if (digests) BKD_HIP(hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        out(hs.h_frm[s], hs.h_res[s], i0, cnt);
        return BKD_OK;
    };
    return host_segments(hs, h_lengths, n, max_entries, seg, drain);
}

// package_host_staged's `launch` of the CRC forms.
auto crc_package(int algo, int64_t ledger_id) {
    return [=](DeviceState& ds, HostStage& hs, int s, const int64_t* d_ids, const int64_t* d_ledger_ids, uint64_t cnt,
               uint64_t bytes, uint64_t stride) {
        return package_framed(ds, hs.st[s], algo, ledger_id, d_ids, d_ids + cnt, d_ids + 2 * cnt, hs.d_buf[s], bytes,
                              hs.d_off[s], hs.d_len[s], cnt, hs.d_frm[s], stride, hs.d_res[s], d_ledger_ids);
    };
}

// package_host_staged's `out` for the calls that return a frame array (and the digests, unless h_digests
// is null): each frame's `hl` = 32 + mac bytes, `src_stride` apart where they landed.
auto host_frames(uint64_t hl, uint64_t src_stride, void* h_frames, uint64_t frame_stride, uint32_t* h_digests) {
    return [=](const uint8_t* frm, const uint32_t* res, uint64_t i0, uint64_t cnt) {
        // packed frames in one copy; with a wider stride only each frame's 32 + mac bytes (the bytes
        // between frames are the caller's, and the device never wrote them)
        uint8_t* dst = (uint8_t*)h_frames + i0 * frame_stride;
        if (frame_stride == hl && src_stride == hl) memcpy(dst, frm, cnt * hl);
        else
            for (uint64_t j = 0; j < cnt; ++j) memcpy(dst + j * frame_stride, frm + j * src_stride, hl);
        if (h_digests) memcpy(h_digests + i0, res, cnt * 4);
    };
}

// The GPU route of bkd_digest_verify_batch_host and bkd_digest_verify_batch_mac_host.
// launch(ds, hs, s, i0, cnt, bytes) enqueues the verify sequence over slot s's staged frames, entries
// [i0, i0 + cnt): statuses to d_res, the segment's first_bad to d_fb. *h_first_bad: n on entry.
template <class Launch>
int verify_host_staged(const Launch& launch, const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                       int32_t* h_status, uint64_t* h_first_bad) {
    StagedCall call(&HostStage::init_verify);
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        const hipStream_t st = hs.st[s];
        int r = stage_entries(hs, s, h_frames, h_lengths, i0, cnt, bytes);
        if (r) return r;
        r = launch(*call.ds, hs, s, i0, cnt, bytes);
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st));
        BKD_HIP(hipMemcpyAsync(hs.h_fb[s], hs.d_fb[s], 8, hipMemcpyDeviceToHost, st));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        memcpy(h_status + i0, hs.h_res[s], cnt * 4);
        merge_first_bad(hs, s, i0, cnt, h_first_bad);
        return BKD_OK;
    };
    return host_segments(hs, h_lengths, n, HostStage::kSegEntries, seg, drain);
}

// ---- MAC ledgers (HMAC-SHA1): one lane per entry (mac_kernels.hpp) ---------------------------------

bkd::MacKey mac_key(const uint32_t* key_state) {
    bkd::MacKey k;
    memcpy(k.s, key_state, sizeof(k.s));
    return k;
}

unsigned mac_blocks(uint64_t n) { return (unsigned)((n + bkd::kMacBlock - 1) / bkd::kMacBlock); }

// One block of kMacBlock lanes per kMacBlock entries: the grid's 2^31 - 1 blocks bound a batch.
constexpr uint64_t kMacMaxBatch = 0x7FFFFFFFull * bkd::kMacBlock;

int mac_raw(DeviceState& ds, hipStream_t st, const uint32_t* key_state, const void* d_base, uint64_t size,
            const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, uint8_t* d_out) {
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    hipLaunchKernelGGL(bkd::mac_batch_kernel, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, mac_key(key_state),
                       (const uint8_t*)d_base, size, d_offsets, d_lengths, n, d_out, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// The package kernel over `who` (bkd::MacOneLedger: one ledger's key and id; bkd::MacLedgers: a key table
// and a ledger id per entry).
template <class Who>
int mac_package(DeviceState& ds, hipStream_t st, const Who& who, const int64_t* d_entry_ids, const int64_t* d_lacs,
                const int64_t* d_length_fields, const void* d_payload, uint64_t size, const uint64_t* d_offsets,
                const uint32_t* d_lengths, uint64_t n, void* d_frames, uint64_t stride) {
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    hipLaunchKernelGGL(bkd::mac_package_kernel<Who>, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who, d_entry_ids,
                       d_lacs, d_length_fields, (const uint8_t*)d_payload, size, d_offsets, d_lengths, n,
                       (uint8_t*)d_frames, stride, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// Composite payloads (bkd_digest_package_batch_segments_mac): the package kernel over the entries'
// segments, one launch; each payload byte is read once and none is copied.
int mac_package_segments(DeviceState& ds, hipStream_t st, const bkd::MacLedgersOr& who, const int64_t* d_entry_ids,
                         const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload, uint64_t size,
                         const uint64_t* d_seg_offsets, const uint32_t* d_seg_lengths, uint64_t nseg,
                         const uint64_t* d_seg_first, uint64_t n, void* d_frames, uint64_t stride) {
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    const bkd::MacSegments src{(const uint8_t*)d_payload, size, d_seg_offsets, d_seg_lengths, nseg, d_seg_first, n};
    hipLaunchKernelGGL((bkd::mac_package_adds_kernel<bkd::MacLedgersOr, bkd::MacSegments, bkd::MacFrames>),
                       dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who, d_entry_ids, d_lacs, d_length_fields, src, n,
                       bkd::MacFrames{(uint8_t*)d_frames, stride}, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// V2 add requests (bkd_digest_package_batch_v2_mac): the package kernel writes every request's 80-byte head
// and, into the stream's scratch (slot 3, package_v2's), the bytes to copy in behind it; then
// package_v2_copy_kernel as for the CRC digests, with those lengths. Two launches, no host sync.
int mac_package_v2(DeviceState& ds, hipStream_t st, const bkd::MacLedgersOr& who, const int64_t* d_entry_ids,
                   const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload, uint64_t size,
                   const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, const uint8_t* d_keys,
                   uint64_t key_stride, uint32_t packet_header, uint32_t small_threshold, void* d_requests,
                   uint64_t requests_size, const uint64_t* d_request_offsets) {
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // the scratch and the two launches as one sequence
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    uint8_t* sb = nullptr;
    const hipError_t e = sc.get(3, (size_t)n * 4, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("package_v2 scratch: ") + hipGetErrorString(e));
    uint32_t* copy_len = reinterpret_cast<uint32_t*>(sb);
    const bkd::V2Requests rq{(uint8_t*)d_requests, requests_size, d_request_offsets, bkd::host::kMacLen, small_threshold};
    hipLaunchKernelGGL((bkd::mac_package_adds_kernel<bkd::MacLedgersOr, bkd::MacRanges, bkd::MacV2Heads>), dim3(mac_blocks(n)),
                       dim3(bkd::kMacBlock), 0, st, who, d_entry_ids, d_lacs, d_length_fields,
                       bkd::MacRanges{(const uint8_t*)d_payload, size, d_offsets, d_lengths}, n,
                       bkd::MacV2Heads{rq, d_keys, key_stride, packet_header, copy_len}, err);
    BKD_HIP(hipGetLastError());
    if (small_threshold == 0u) return BKD_OK;
    return with_lanes<4>(v2_copy_lanes(size / n), [&](auto g) -> int {
        constexpr int G = decltype(g)::value;
        const uint64_t per_block = 256 / G;
        const unsigned cblocks = (unsigned)std::min<uint64_t>((n + per_block - 1) / per_block, 8u * (uint64_t)ds.cus);
        hipLaunchKernelGGL(bkd::package_v2_copy_kernel<G>, dim3(cblocks), dim3(256), 0, st, (const uint8_t*)d_payload, size,
                           d_offsets, copy_len, n, rq);
        BKD_HIP(hipGetLastError());
        return BKD_OK;
    });
}

// *d_first_bad = n (reframe_first_bad_kernel, as the trusted reframe initialises it), then the verify
// kernel lowers it.
int mac_verify(DeviceState& ds, hipStream_t st, const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id,
               int id_checks, const void* d_framed, uint64_t size, const uint64_t* d_offsets, const uint32_t* d_lengths,
               uint64_t n, int32_t* d_status, uint64_t* d_first_bad) {
    if (n == 0) {
        BKD_HIP(hipMemsetAsync(d_first_bad, 0, sizeof(uint64_t), st));
        return BKD_OK;
    }
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // the two launches as one sequence
    hipLaunchKernelGGL(bkd::reframe_first_bad_kernel, dim3(1), dim3(1), 0, st, d_first_bad, n);
    BKD_HIP(hipGetLastError());
    const bkd::MacOneRead who{mac_key(key_state), ledger_id, first_entry_id, id_checks, (unsigned long long*)d_first_bad};
    hipLaunchKernelGGL(bkd::mac_verify_kernel<bkd::MacOneRead>, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who,
                       (const uint8_t*)d_framed, size, d_offsets, d_lengths, n, d_status, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// A key table in device memory and who indexes it: per request (verify) or per entry (package).
struct MacKeys {
    const uint32_t* states;
    uint64_t nkeys;
    const uint32_t* index;
};

// A host key table on the current device for the length of one host-resident call: one allocation and one
// blocking copy, so every staged segment of the call, on either slot's stream, finds it there.
struct DeviceTable {
    uint32_t* d = nullptr;
    int upload(const uint32_t* h_key_states, uint64_t nkeys) {
        if (d || nkeys == 0) return BKD_OK;
        const hipError_t e = hipMalloc((void**)&d, nkeys * 10u * sizeof(uint32_t));
        if (e != hipSuccess) {
            d = nullptr;
            return fail(BKD_ERR_NOMEM, std::string("key table: ") + hipGetErrorString(e));
        }
        BKD_HIP(hipMemcpy(d, h_key_states, nkeys * 10u * sizeof(uint32_t), hipMemcpyHostToDevice));
        return BKD_OK;
    }
    ~DeviceTable() {
        if (d) (void)hipFree(d);
    }
};

// The GPU route of the MAC package forms that take a key table (many ledgers, composite payloads, V2):
// package_host_staged with the `stage` and `launch` they share. inner(hs, s, i0, cnt, bytes) stages the
// entries (entry_buffers, HostSegments); each segment's key rows h_key_of[i0 ..] travel in the seeds buffer
// beside them, and the table is uploaded once, by the first segment (the staged call has entered the device
// by then). The device writes packed 52-byte frames and no digest words; `out` puts them where the form
// wants them.
template <class Inner, class Out>
int mac_package_host_staged(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_key_of,
                            const int64_t* h_ledger_ids, const int64_t* h_entry_ids, const int64_t* h_lacs,
                            const int64_t* h_length_fields, const Inner& inner, const uint32_t* h_lengths, uint64_t n,
                            const Out& out) {
    DeviceTable keys;
    auto stage = [&](HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        int r = keys.upload(h_key_states, nkeys);
        if (r) return r;
        r = inner(hs, s, i0, cnt, bytes);
        if (r) return r;
        memcpy(hs.h_seed[s], h_key_of + i0, cnt * 4);
        BKD_HIP(hipMemcpyAsync(hs.d_seed[s], hs.h_seed[s], cnt * 4, hipMemcpyHostToDevice, hs.st[s]));
        return BKD_OK;
    };
    auto launch = [&](DeviceState& ds, HostStage& hs, int s, const int64_t* d_ids, const int64_t* d_ledger_ids,
                      uint64_t cnt, uint64_t bytes, uint64_t stride) {
        return mac_package(ds, hs.st[s], bkd::MacLedgers{keys.d, nkeys, hs.d_seed[s], d_ledger_ids}, d_ids, d_ids + cnt,
                           d_ids + 2 * cnt, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt, hs.d_frm[s], stride);
    };
    return package_host_staged(h_ledger_ids, h_entry_ids, h_lacs, h_length_fields, stage, h_lengths, n, launch,
                               bkd::host::kMacFrameHead, false, out);
}

// Read requests of MAC ledgers (bkd_digest_verify_requests_mac, bkd_digest_reframe_requests_mac; rq as
// verify_framed takes it, keys.index per request): the CSR expanded into the stream's verify scratch and
// checked and the prefixes initialised by request_expand_kernel, then launch(who, err) enqueues the call's
// kernel over bkd::MacRequests.
template <class Launch>
int mac_requests(DeviceState& ds, hipStream_t st, const MacKeys& keys, uint64_t n, const Requests& rq,
                 const Launch& launch) {
    if (n == 0) {
        if (rq.nreq) BKD_HIP(hipMemsetAsync(rq.first_bad, 0, rq.nreq * sizeof(uint64_t), st));
        return BKD_OK;
    }
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    Carver cv;
    const size_t o_xlid = cv.take(n * 8), o_xeid = cv.take(n * 8), o_req = cv.take(n * 4);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // the scratch and the two launches as one sequence
    uint8_t* sb = nullptr;
    const hipError_t e = sc.get(1, cv.used, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("verify scratch: ") + hipGetErrorString(e));
    int64_t *xlid = Carver::at<int64_t>(sb, o_xlid), *xeid = Carver::at<int64_t>(sb, o_xeid);
    uint32_t* req_of = Carver::at<uint32_t>(sb, o_req);
    const unsigned xblocks = (unsigned)std::min<uint64_t>((std::max(n, rq.nreq) + 255) / 256, 8u * (uint64_t)ds.cus);
    hipLaunchKernelGGL(bkd::request_expand_kernel, dim3(xblocks), dim3(256), 0, st, rq.first, rq.nreq, n, rq.ledger_ids,
                       rq.first_entry_ids, rq.flags, xlid, xeid, req_of, (unsigned long long*)rq.first_bad, err);
    BKD_HIP(hipGetLastError());
    launch(bkd::MacRequests{keys.states, keys.nkeys, keys.index,
                            bkd::RequestIds{xlid, xeid, req_of, rq.first, (unsigned long long*)rq.first_bad}},
           err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

int mac_verify_requests(DeviceState& ds, hipStream_t st, const MacKeys& keys, const void* d_framed, uint64_t size,
                        const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, int32_t* d_status,
                        const Requests& rq) {
    return mac_requests(ds, st, keys, n, rq, [&](const bkd::MacRequests& who, uint32_t* err) {
        hipLaunchKernelGGL(bkd::mac_verify_kernel<bkd::MacRequests>, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who,
                           (const uint8_t*)d_framed, size, d_offsets, d_lengths, n, d_status, err);
    });
}

// The reframe kernel over n frames: in place, or apart into d_out_frames at `stride` (mac_kernels.hpp).
template <class Who>
void mac_reframe_launch(hipStream_t st, const Who& who, bool trusted, void* d_framed, uint64_t size,
                        const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, const int64_t* d_new_lacs,
                        void* d_out_frames, uint64_t stride, int32_t* d_status, uint32_t* err) {
    if (trusted)
        hipLaunchKernelGGL((bkd::mac_reframe_kernel<Who, true>), dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who,
                           (uint8_t*)d_framed, size, d_offsets, d_lengths, n, d_new_lacs, (uint8_t*)d_out_frames, stride,
                           d_status, err);
    else
        hipLaunchKernelGGL((bkd::mac_reframe_kernel<Who, false>), dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who,
                           (uint8_t*)d_framed, size, d_offsets, d_lengths, n, d_new_lacs, (uint8_t*)d_out_frames, stride,
                           d_status, err);
}

// The verify kernel over one staged segment of the host form: who holds the segment's expectations.
int mac_verify_expected(DeviceState& ds, hipStream_t st, const bkd::MacExpected& who, const void* d_framed,
                        uint64_t size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                        int32_t* d_status) {
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    hipLaunchKernelGGL(bkd::mac_verify_kernel<bkd::MacExpected>, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, who,
                       (const uint8_t*)d_framed, size, d_offsets, d_lengths, n, d_status, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// The reframe kernel over one staged segment of the host form: out-frames apart, packed at 52 bytes.
int mac_reframe_expected(DeviceState& ds, hipStream_t st, const bkd::MacExpected& who, bool trusted, void* d_framed,
                         uint64_t size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                         const int64_t* d_new_lacs, void* d_out_frames, int32_t* d_status) {
    uint32_t* err = nullptr;
    const int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    mac_reframe_launch(st, who, trusted, d_framed, size, d_offsets, d_lengths, n, d_new_lacs, d_out_frames,
                       bkd::host::kMacFrameHead, d_status, err);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// Route of the host-resident MAC batches: 1 = CPU, 2 = GPU, < 0 = error. Automatic: the GPU whenever a
// device is visible (derived from ~0.5 GB/s of SHA-1 per core against ~51 GiB/s of PCIe, then measured:
// 41.8 against 7.9 GB/s on 16 threads); a batch with an entry over BKD_MAC_MAX_ENTRY takes
// the CPU route, or fails when the GPU is forced.
int mac_host_route(const uint32_t* lengths, uint64_t n) {
    const int r = g_host_route.load(std::memory_order_relaxed);
    if (r == 1) return 1;
    if (visible_devices() <= 0)
        return r == 2 ? fail(BKD_ERR_NO_DEVICE, "no HIP device (host batch route forced to the GPU)") : 1;
    for (uint64_t i = 0; i < n; ++i)
        if (lengths[i] > BKD_MAC_MAX_ENTRY)
            return r == 2 ? fail(BKD_ERR_INVALID_ARG, "host entry " + std::to_string(i) +
                                                          " is longer than BKD_MAC_MAX_ENTRY (GPU route forced)")
                          : 1;
    return 2;
}

// One staged segment's expectations, as verify_requests_host has put them on the device: a ledger id, an
// entry id and a flag word (bkd::host::kSkipEntryId or 0) per entry, then one zero u64 on an 8-byte boundary.
// req_of: the host's request index | skip bit of the segment's entries; first: the call's index of entry 0.
struct StagedRequests {
    const int64_t *d_lid, *d_eid;
    const uint32_t* d_flag;
    const uint64_t* d_zero;
    const uint32_t* req_of;
    uint64_t first;
};

// What a verify form has left to do with a drained segment: nothing.
struct NothingDrained {
    int operator()(HostStage&, int, uint64_t, uint64_t) const { return BKD_OK; }
};

// bkd_digest_verify_requests_host and bkd_digest_verify_requests_mac_host. Checked before any work, in this
// order: the request count, the request arrays, the MAC form's key table and per-request rows (`keys`; null
// for CRC), the CSR, the entry buffers, each frame; a violation writes nothing. Then the requests become
// per-entry expectations, which the CPU route checks frame by frame and the GPU route stages beside the
// frames, and each request's verified prefix is its first non-zero status: the statuses come back to the
// host on either route, so a request that straddles two staged segments gets the minimum over both parts.
// host(xlid, xeid, req_of) returns the form's route (< 0: its error) and, where that is 1, has verified every
// frame on the CPU. launch(ds, hs, s, cnt, bytes, x) enqueues the verify sequence over slot s's staged frames
// and expectations x, statuses to d_res. drained(hs, s, i0, cnt): the segment's statuses are in h_status and
// whatever else the launch had copied back is in slot s (the MAC reframe's out-frames). init...: the
// StagedCall groups the launch needs.
template <class Host, class Launch, class Drained, class... Init>
int verify_requests_host(const MacKeys* keys, const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                         const uint64_t* h_req_first, uint64_t nreq, const int64_t* h_req_ledger_ids,
                         const int64_t* h_req_first_entry_ids, const uint32_t* h_req_flags, int32_t* h_status,
                         uint64_t* h_req_first_bad, const Host& host, const Launch& launch, const Drained& drained,
                         Init... init) {
    if (nreq >= 0x80000000ull) return fail(BKD_ERR_INVALID_ARG, "a call holds fewer than 2^31 requests");
    if (nreq == 0) return n ? fail(BKD_ERR_INVALID_ARG, "entries without a request") : BKD_OK;
    if ((keys && !keys->index) || !h_req_first || !h_req_ledger_ids || !h_req_first_entry_ids || !h_req_flags ||
        !h_req_first_bad)
        return fail(BKD_ERR_INVALID_ARG, "null request array");
    if (keys && keys->nkeys && !keys->states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (keys)
        if (int rc = check_key_index("request", keys->index, nreq, keys->nkeys)) return rc;
    if (int rc = check_csr("req_first", "request", h_req_first, nreq, "nreq", n, "n")) return rc;
    if (n && (!h_frames || !h_lengths || !h_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_host_entries("frame", h_frames, h_lengths, n)) return rc;
    for (uint64_t r = 0; r < nreq; ++r) h_req_first_bad[r] = h_req_first[r + 1] - h_req_first[r];
    if (n == 0) return BKD_OK;
    std::vector<int64_t> xlid(n), xeid(n);
    std::vector<uint32_t> req_of(n);
    for (uint64_t r = 0; r < nreq; ++r)
        for (uint64_t i = h_req_first[r]; i < h_req_first[r + 1]; ++i) {
            xlid[i] = h_req_ledger_ids[r];
            xeid[i] = (int64_t)((uint64_t)h_req_first_entry_ids[r] + (i - h_req_first[r]));
            req_of[i] = (uint32_t)r | ((h_req_flags[r] & 1u) ? bkd::host::kSkipEntryId : 0u);
        }
    auto prefixes = [&] {
        for (uint64_t r = 0; r < nreq; ++r)
            for (uint64_t i = h_req_first[r]; i < h_req_first[r + 1]; ++i)
                if (h_status[i] != 0) {
                    h_req_first_bad[r] = i - h_req_first[r];
                    break;
                }
    };
    const int route = host(xlid.data(), xeid.data(), req_of.data());
    if (route < 0) return route;
    if (route == 1) {
        prefixes();
        return BKD_OK;
    }
    StagedCall call(init...);
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        const hipStream_t st = hs.st[s];
        int r = stage_entries(hs, s, h_frames, h_lengths, i0, cnt, bytes);
        if (r) return r;
        // [ledger ids][entry ids][flag words][pad to 8][one zero u64]
        const size_t o_eid = cnt * 8, o_flag = cnt * 16, o_zero = (cnt * 20 + 7) & ~(size_t)7;
        memcpy(hs.h_rq[s], xlid.data() + i0, cnt * 8);
        memcpy(hs.h_rq[s] + o_eid, xeid.data() + i0, cnt * 8);
        uint32_t* flag = reinterpret_cast<uint32_t*>(hs.h_rq[s] + o_flag);
        for (uint64_t j = 0; j < cnt; ++j) flag[j] = req_of[i0 + j] & bkd::host::kSkipEntryId;
        memset(hs.h_rq[s] + cnt * 20, 0, o_zero + 8 - cnt * 20);
        BKD_HIP(hipMemcpyAsync(hs.d_rq[s], hs.h_rq[s], o_zero + 8, hipMemcpyHostToDevice, st));
        const uint8_t* d = hs.d_rq[s];
        r = launch(*call.ds, hs, s, cnt, bytes,
                   StagedRequests{reinterpret_cast<const int64_t*>(d), reinterpret_cast<const int64_t*>(d + o_eid),
                                  reinterpret_cast<const uint32_t*>(d + o_flag),
                                  reinterpret_cast<const uint64_t*>(d + o_zero), req_of.data() + i0, i0});
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        memcpy(h_status + i0, hs.h_res[s], cnt * 4);
        return drained(hs, s, i0, cnt);
    };
    const int rc = host_segments(hs, h_lengths, n, HostStage::kSegEntries, seg, drain);
    if (rc == BKD_OK) prefixes();
    return rc;
}

// ---- the mixed-ledger entry-log scrub (scrub_kernels.hpp) -------------------------------------------

std::atomic<int> g_scrub_order{0};  // bkd_set_scrub_order: 0 binned, 1 index order

// The ledger table of bkd_entrylog_verify_ledgers and the key table its HMAC rows index.
struct ScrubArgs {
    const int64_t* ids;
    const uint32_t* types;
    const uint32_t* keys;
    uint64_t nledgers;
    const uint32_t* key_states;
    uint64_t nkeys;
    uint32_t mask;
};

// What every form of the call refuses before it looks for a device.
int scrub_args_check(const void* log, const void* offsets, const void* lengths, uint64_t n, const ScrubArgs& a,
                     const void* status, const void* first_bad) {
    if (!first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    if (n > 0 && (!log || !offsets || !lengths || !status)) return fail(BKD_ERR_INVALID_ARG, "null array");
    if (n > 0xFFFFFFFFull) return fail(BKD_ERR_INVALID_ARG, "more than 2^32 - 1 entries");
    if (a.nledgers > 0 && (!a.ids || !a.types)) return fail(BKD_ERR_INVALID_ARG, "null ledger table");
    if (a.mask & ~bkd::scrub::kTypeMaskAll) return fail(BKD_ERR_INVALID_ARG, "types has bits above BKD_DIGEST_DUMMY");
    if ((a.mask >> bkd::scrub::kHmac) & 1u) {
        if (!a.key_states || a.nkeys == 0) return fail(BKD_ERR_INVALID_ARG, "the HMAC bit needs a key table");
        if (a.nledgers > 0 && !a.keys) return fail(BKD_ERR_INVALID_ARG, "the HMAC bit needs the ledgers' key rows");
    }
    return BKD_OK;
}

// The scrub's carve of the stream's scratch slot 4: what classify, scan and scatter write, then one set of
// arrays per CRC class in the mask. `own_outputs` adds a status array and a first_bad word for a caller that
// has none of its own (bkd_entrylog_scrub_lanes).
struct ScrubCarve {
    bool has[2], has_mac;
    size_t o_tag, o_krow, o_perm, o_counts, o_off[2], o_len[2], o_st[2], o_fb[2], o_status, o_first, used;
    uint32_t *tag, *krow, *perm, *counts, *nmac;
    bkd::ScrubClass cls[2];
    int32_t* cst[2];

    ScrubCarve(uint64_t n, uint32_t mask, bool own_outputs) {
        has[0] = ((mask >> bkd::scrub::kCrc32c) & 1u) != 0;
        has[1] = ((mask >> bkd::scrub::kCrc32) & 1u) != 0;
        has_mac = ((mask >> bkd::scrub::kHmac) & 1u) != 0;
        Carver cv;
        o_tag = cv.take(n * 4);
        o_krow = cv.take(has_mac ? n * 4 : 0);
        o_perm = cv.take(has_mac ? n * 4 : 0);
        o_counts = cv.take((bkd::scrub::kBins + 1) * 4);
        for (int c = 0; c < 2; ++c) {
            o_off[c] = cv.take(has[c] ? n * 8 : 0);
            o_len[c] = cv.take(has[c] ? n * 4 : 0);
            o_st[c] = cv.take(has[c] ? n * 4 : 0);
            o_fb[c] = cv.take(has[c] ? 8 : 0);
        }
        o_status = cv.take(own_outputs ? n * 4 : 0);
        o_first = cv.take(own_outputs ? 8 : 0);
        used = cv.used;
    }
    void bind(uint8_t* sb) {
        tag = Carver::at<uint32_t>(sb, o_tag);
        krow = has_mac ? Carver::at<uint32_t>(sb, o_krow) : nullptr;
        perm = has_mac ? Carver::at<uint32_t>(sb, o_perm) : nullptr;
        counts = Carver::at<uint32_t>(sb, o_counts);
        nmac = counts + bkd::scrub::kBins;
        for (int c = 0; c < 2; ++c) {
            cls[c] = bkd::ScrubClass{has[c] ? Carver::at<uint64_t>(sb, o_off[c]) : nullptr,
                                     has[c] ? Carver::at<uint32_t>(sb, o_len[c]) : nullptr};
            cst[c] = has[c] ? Carver::at<int32_t>(sb, o_st[c]) : nullptr;
        }
    }
};

// classify -> scan -> scatter in stream order: every entry's tag (and final status where it has one), the
// HMAC frames' lanes in cv.perm[0, *cv.nmac) in the order bkd_set_scrub_order asks for, *d_first_bad = n.
// Shared by the full call and bkd_entrylog_scrub_lanes.
int scrub_order_lanes(hipStream_t st, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                      const uint32_t* d_lengths, uint64_t n, const ScrubArgs& a, const ScrubCarve& cv, uint32_t* err,
                      int32_t* d_status, uint64_t* d_first_bad) {
    const int order = g_scrub_order.load(std::memory_order_relaxed);
    const unsigned blocks = (unsigned)((n + bkd::kScrubBlock - 1) / bkd::kScrubBlock);
    BKD_HIP(hipMemsetAsync(cv.counts, 0, (bkd::scrub::kBins + 1) * 4, st));
    const bkd::ScrubTable tab{a.ids, a.types, a.keys, a.nledgers, a.nkeys, a.mask};
    hipLaunchKernelGGL(bkd::scrub_classify_kernel, dim3(blocks), dim3(bkd::kScrubBlock), 0, st, (const uint8_t*)d_log,
                       log_size, d_offsets, d_lengths, n, tab, cv.cls[0], cv.cls[1], cv.tag, cv.krow, cv.counts, d_status,
                       err);
    BKD_HIP(hipGetLastError());
    hipLaunchKernelGGL(bkd::scrub_scan_kernel, dim3(1), dim3(1), 0, st, cv.counts, cv.nmac, n, order, d_first_bad);
    BKD_HIP(hipGetLastError());
    if (cv.has_mac) {
        hipLaunchKernelGGL(bkd::scrub_scatter_kernel, dim3(blocks), dim3(bkd::kScrubBlock), 0, st, cv.tag, n, order,
                           cv.counts, cv.perm);
        BKD_HIP(hipGetLastError());
    }
    return BKD_OK;
}

// classify -> scan -> scatter -> one lane per HMAC frame -> verify_framed per CRC class in the mask ->
// merge. All in stream order under the stream's lock; the HMAC count stays on the device (the grid of
// mac_scrub_kernel is sized by n).
int scrub_ledgers(DeviceState& ds, hipStream_t st, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                  const uint32_t* d_lengths, uint64_t n, const ScrubArgs& a, int32_t* d_status, uint64_t* d_first_bad) {
    if (n == 0) {
        BKD_HIP(hipMemsetAsync(d_first_bad, 0, sizeof(uint64_t), st));
        return BKD_OK;
    }
    uint32_t* err = nullptr;
    int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    ScrubCarve cv(n, a.mask, false);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // held across the nested verify sequences (slots 1 and 0)
    uint8_t* sb = nullptr;
    const hipError_t e = sc.get(4, cv.used, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("scrub scratch: ") + hipGetErrorString(e));
    cv.bind(sb);
    rc = scrub_order_lanes(st, d_log, log_size, d_offsets, d_lengths, n, a, cv, err, d_status, d_first_bad);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n + bkd::kScrubBlock - 1) / bkd::kScrubBlock);
    if (cv.has_mac) {
        hipLaunchKernelGGL(bkd::mac_scrub_kernel, dim3(mac_blocks(n)), dim3(bkd::kMacBlock), 0, st, cv.perm, cv.nmac,
                           cv.tag, cv.krow, a.key_states, a.nkeys, (const uint8_t*)d_log, d_offsets, d_lengths, n,
                           d_status);
        BKD_HIP(hipGetLastError());
    }
    for (int c = 0; c < 2; ++c) {
        if (!cv.has[c]) continue;
        const int vr = verify_framed(ds, st, c, 0, 0, 2, d_log, log_size, cv.cls[c].off, cv.cls[c].len, n, cv.cst[c],
                                     Carver::at<uint64_t>(sb, cv.o_fb[c]));
        if (vr) return vr;
    }
    hipLaunchKernelGGL(bkd::scrub_merge_kernel, dim3(blocks), dim3(bkd::kScrubBlock), 0, st, cv.tag, cv.cst[0], cv.cst[1],
                       n, d_status, (unsigned long long*)d_first_bad);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

// bkd_entrylog_scrub_lanes: the three launches above, then the lane array and the lane count copied out.
int scrub_lanes(DeviceState& ds, hipStream_t st, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                const uint32_t* d_lengths, uint64_t n, const ScrubArgs& a, uint32_t* d_lanes, uint32_t* d_nlanes) {
    if (n == 0) {
        BKD_HIP(hipMemsetAsync(d_nlanes, 0, sizeof(uint32_t), st));
        return BKD_OK;
    }
    uint32_t* err = nullptr;
    int rc = bounds_flag(ds, st, &err);
    if (rc) return rc;
    ScrubCarve cv(n, a.mask, true);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);
    uint8_t* sb = nullptr;
    const hipError_t e = sc.get(4, cv.used, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("scrub scratch: ") + hipGetErrorString(e));
    cv.bind(sb);
    rc = scrub_order_lanes(st, d_log, log_size, d_offsets, d_lengths, n, a, cv, err, Carver::at<int32_t>(sb, cv.o_status),
                           Carver::at<uint64_t>(sb, cv.o_first));
    if (rc) return rc;
    BKD_HIP(hipMemcpyAsync(d_lanes, cv.perm, n * 4, hipMemcpyDeviceToDevice, st));
    BKD_HIP(hipMemcpyAsync(d_nlanes, cv.nmac, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return BKD_OK;
}

// bkd_entrylog_scrub_report: scrub_ledgers as it is, then row init -> one lane per entry -> the scan of the
// blocks' bad counts -> the bad list, over slot 4 carved as ScrubCarve with outputs of its own (the statuses
// when the caller keeps none, the first_bad word) and the block counts behind it. The lock is taken here
// and again by scrub_ledgers (it is recursive), whose smaller carve of slot 4 is a prefix of this one.
int scrub_report(DeviceState& ds, hipStream_t st, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                 const uint32_t* d_lengths, uint64_t n, const ScrubArgs& a, int32_t* d_status, uint64_t* d_report,
                 uint32_t* d_bad, uint64_t bad_capacity, uint64_t* d_nbad) {
    const uint64_t rows = a.nledgers + 1;
    const unsigned init_blocks = (unsigned)((rows * bkd::scrub::kReportWords + bkd::kReportBlock - 1) / bkd::kReportBlock);
    hipLaunchKernelGGL(bkd::scrub_report_init_kernel, dim3(init_blocks), dim3(bkd::kReportBlock), 0, st, d_report, rows, n);
    BKD_HIP(hipGetLastError());
    if (n == 0) {
        BKD_HIP(hipMemsetAsync(d_nbad, 0, sizeof(uint64_t), st));
        return BKD_OK;
    }
    const uint64_t blocks = (n + bkd::kReportBlock - 1) / bkd::kReportBlock;
    ScrubCarve cv(n, a.mask, true);
    Carver more;
    more.used = cv.used;
    const size_t o_blocks = more.take(blocks * 4);
    StreamScratch& sc = scratch_for(ds, st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);
    uint8_t* sb = nullptr;
    const hipError_t e = sc.get(4, more.used, st, &sb);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("scrub scratch: ") + hipGetErrorString(e));
    int32_t* status = d_status ? d_status : Carver::at<int32_t>(sb, cv.o_status);
    const int rc = scrub_ledgers(ds, st, d_log, log_size, d_offsets, d_lengths, n, a, status,
                                 Carver::at<uint64_t>(sb, cv.o_first));
    if (rc) return rc;
    uint32_t* block_bad = Carver::at<uint32_t>(sb, o_blocks);
    hipLaunchKernelGGL(bkd::scrub_report_kernel, dim3((unsigned)blocks), dim3(bkd::kReportBlock), 0, st,
                       (const uint8_t*)d_log, log_size, d_offsets, d_lengths, n, a.ids, a.nledgers, status,
                       (unsigned long long*)d_report, block_bad);
    BKD_HIP(hipGetLastError());
    hipLaunchKernelGGL(bkd::scrub_report_scan_kernel, dim3(1), dim3(bkd::kReportScanBlock), 0, st, block_bad, blocks,
                       d_nbad);
    BKD_HIP(hipGetLastError());
    if (bad_capacity) {
        hipLaunchKernelGGL(bkd::scrub_report_scatter_kernel, dim3((unsigned)blocks), dim3(bkd::kReportBlock), 0, st, status,
                           n, block_bad, d_bad, bad_capacity);
        BKD_HIP(hipGetLastError());
    }
    return BKD_OK;
}

// The extra argument checks of the report calls, after scrub_args_check.
int report_args_check(const void* report, const void* bad, uint64_t bad_capacity, const void* nbad) {
    if (!report) return fail(BKD_ERR_INVALID_ARG, "null report");
    if (!nbad) return fail(BKD_ERR_INVALID_ARG, "null nbad");
    if (bad_capacity > 0 && !bad) return fail(BKD_ERR_INVALID_ARG, "null bad list with a capacity above 0");
    return BKD_OK;
}

// The host forms' upload into plain allocations on a stream of the call's own, so that its bounds flag is
// its own; everything is freed when the call returns.
struct HostUpload {
    std::vector<void*> ptrs;
    hipStream_t st = nullptr;
    bool failed = false;
    ~HostUpload() {
        for (void* p : ptrs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    void* get(size_t bytes) {  // nullptr on failure (or for no bytes)
        if (!bytes) return nullptr;
        void* d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            failed = true;
            return nullptr;
        }
        ptrs.push_back(d);
        return d;
    }
    void* put(const void* h, size_t bytes) {  // nullptr on failure (or for nothing to copy)
        if (!h) return nullptr;
        void* d = get(bytes);
        if (d && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) failed = true;
        return d;
    }
};

// The report outputs of bkd_entrylog_scrub_report_host in host memory.
struct HostReport {
    uint64_t* report;
    uint32_t* bad;
    uint64_t capacity;
    uint64_t* nbad;
};

// bkd_entrylog_verify_ledgers_host (rep null) and bkd_entrylog_scrub_report_host (h_status and h_first_bad
// may be null) after their argument checks: the table check, the route, and everything written before
// BKD_ERR_BOUNDS is returned.
int scrub_host(const void* h_log, uint64_t log_size, const uint64_t* h_offsets, const uint32_t* h_lengths, uint64_t n,
               const ScrubArgs& a, int32_t* h_status, uint64_t* h_first_bad, const HostReport* rep) {
    const bkd::host::ScrubLedgers t{a.ids, a.types, a.keys, a.nledgers, a.key_states, a.nkeys, a.mask};
    if (const uint64_t bad = bkd::host::scrub_table_check(t))
        return fail(BKD_ERR_INVALID_ARG, "ledger table row " + std::to_string(bad - 1) +
                                             ": ids must ascend strictly and an HMAC row's key index be < nkeys");
    uint64_t first_bad_word = 0;
    if (!h_first_bad) h_first_bad = &first_bad_word;
    if (n == 0) {
        *h_first_bad = 0;
        if (rep)  // the initial rows, *nbad = 0
            bkd::host::scrub_report(nullptr, log_size, nullptr, nullptr, 0, t, nullptr, rep->report, rep->bad,
                                    rep->capacity, rep->nbad);
        return BKD_OK;
    }
    const int route = bkd_get_scrub_host_route(a.types, a.nledgers, a.mask);
    if (route == 1) {
        std::vector<int32_t> own;
        if (!h_status) {
            own.resize(n);
            h_status = own.data();
        }
        const bool unreadable =
            bkd::host::scrub_entries((const uint8_t*)h_log, log_size, h_offsets, h_lengths, n, t, h_status, h_first_bad);
        if (rep)
            bkd::host::scrub_report((const uint8_t*)h_log, log_size, h_offsets, h_lengths, n, t, h_status, rep->report,
                                    rep->bad, rep->capacity, rep->nbad);
        return unreadable ? fail(BKD_ERR_BOUNDS, kBoundsMsg) : BKD_OK;
    }
    if (visible_devices() <= 0) return fail(BKD_ERR_NO_DEVICE, "no HIP device (host batch route forced to the GPU)");
    // one upload into plain allocations on a stream of the call's own, so that its bounds flag is its own
    HostUpload dev;
    BKD_HIP(hipStreamCreateWithFlags(&dev.st, hipStreamNonBlocking));
    // the log rounded up to whole dwords: the last entry's last aligned dword lies inside the allocation
    const size_t log_alloc = ((size_t)log_size + 3u) & ~(size_t)3u;
    void* d_log = nullptr;
    if (log_alloc) {
        if (hipMalloc(&d_log, log_alloc) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BKD_ERR_NOMEM, "scrub: device allocation for the log failed");
        }
        dev.ptrs.push_back(d_log);
        BKD_HIP(hipMemcpy(d_log, h_log, log_size, hipMemcpyHostToDevice));
    }
    const uint64_t* d_off = (const uint64_t*)dev.put(h_offsets, n * 8);
    const uint32_t* d_len = (const uint32_t*)dev.put(h_lengths, n * 4);
    const ScrubArgs da{(const int64_t*)dev.put(a.ids, a.nledgers * 8),
                       (const uint32_t*)dev.put(a.types, a.nledgers * 4),
                       (const uint32_t*)dev.put(a.keys, a.nledgers * 4),
                       a.nledgers,
                       (const uint32_t*)dev.put(a.key_states, a.nkeys * 40),
                       a.nkeys,
                       a.mask};
    int32_t* d_status = nullptr;
    if (h_status) {
        std::vector<int32_t> none(n, 0);
        d_status = (int32_t*)dev.put(none.data(), n * 4);
    }
    uint64_t* d_fb = rep ? nullptr : (uint64_t*)dev.put(&n, 8);
    const uint64_t rows = a.nledgers + 1, list = rep ? std::min(rep->capacity, n) : 0;
    uint64_t* d_report = rep ? (uint64_t*)dev.get(rows * bkd::scrub::kReportWords * 8) : nullptr;
    uint32_t* d_bad = rep ? (uint32_t*)dev.get(list * 4) : nullptr;
    uint64_t* d_nbad = rep ? (uint64_t*)dev.get(8) : nullptr;
    if (dev.failed) return fail(BKD_ERR_NOMEM, "scrub: device allocation or upload failed");
    int rc;
    {
        Call call((void*)dev.st);
        if (call.rc) return call.rc;
        rc = rep ? scrub_report(*call.ds, call.st, d_log, log_size, d_off, d_len, n, da, d_status, d_report, d_bad, list,
                                d_nbad)
                 : scrub_ledgers(*call.ds, call.st, d_log, log_size, d_off, d_len, n, da, d_status, d_fb);
    }
    // waits for the stream, frees its scratch and reports its bounds flag, whatever the launches answered
    const int rel = bkd_stream_release((void*)dev.st);
    if (rc) return rc;
    if (rel && rel != BKD_ERR_BOUNDS) return rel;
    if (h_status) BKD_HIP(hipMemcpy(h_status, d_status, n * 4, hipMemcpyDeviceToHost));
    if (!rep) {
        BKD_HIP(hipMemcpy(h_first_bad, d_fb, 8, hipMemcpyDeviceToHost));
        return rel;
    }
    BKD_HIP(hipMemcpy(rep->report, d_report, rows * bkd::scrub::kReportWords * 8, hipMemcpyDeviceToHost));
    BKD_HIP(hipMemcpy(rep->nbad, d_nbad, 8, hipMemcpyDeviceToHost));
    const uint64_t listed = std::min(*rep->nbad, list);
    if (listed) BKD_HIP(hipMemcpy(rep->bad, d_bad, listed * 4, hipMemcpyDeviceToHost));
    return rel;
}

}  // namespace

extern "C" {

int bkd_abi_version(void) { return BKD_ABI_VERSION; }

int bkd_device_count(void) { return std::max(0, visible_devices()); }

int bkd_init(int device) {
    int count = bkd_device_count();
    if (count <= 0) return fail(BKD_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count || device >= kMaxDevices) return fail(BKD_ERR_INVALID_ARG, "bad device");
    std::lock_guard<std::mutex> lk(g_mu);
    return init_device_locked(device);
}

const char* bkd_last_error(void) { return t_err.c_str(); }

int bkd_set_fold_schedule(int schedule) {
    if (schedule < 0 || schedule > 2) return fail(BKD_ERR_INVALID_ARG, "fold schedule must be 0, 1 or 2");
    g_fold_sched.store(schedule);
    return BKD_OK;
}

int bkd_set_group_lanes(int lanes) {
    if (lanes != 0 && lane_index(lanes) < 0) return fail(BKD_ERR_INVALID_ARG, "lanes must be 0, 1, 4, 8, 16, 32 or 64");
    g_forced_lanes.store(lanes);
    return BKD_OK;
}

int bkd_set_plan_mode(int mode) {
    if (mode < 0 || mode > 2)
        return fail(BKD_ERR_INVALID_ARG, "plan mode must be 0 (auto), 1 (direct) or 2 (plan)");
    g_plan_mode.store(mode);
    return BKD_OK;
}

int bkd_set_plan_prefetch(int loads_in_flight) {
    if (loads_in_flight != 2 && loads_in_flight != 4 && loads_in_flight != 8)
        return fail(BKD_ERR_INVALID_ARG, "prefetch depth must be 2, 4 or 8");
    g_plan_pf.store(loads_in_flight);
    return BKD_OK;
}

int bkd_set_plan_geometry(int lanes, int steps_per_chunk, int merge_bytes) {
    if (lanes < 4 || lane_index(lanes) < 0) return fail(BKD_ERR_INVALID_ARG, "plan lanes must be 4, 8, 16, 32 or 64");
    if (steps_per_chunk < 1) return fail(BKD_ERR_INVALID_ARG, "steps_per_chunk must be >= 1");
    const uint32_t step = 16u * (uint32_t)lanes, ch = step * (uint32_t)steps_per_chunk;
    if (ch > 32768u) return fail(BKD_ERR_INVALID_ARG, "chunk size must be <= 32 KiB");
    if (merge_bytes < 16 || (uint32_t)merge_bytes > ch) return fail(BKD_ERR_INVALID_ARG, "merge must be in [16, chunk]");
    const uint32_t nbins = (ch + (uint32_t)merge_bytes - 1u + step - 1u) / step + 1u;
    if (nbins + 1u > (uint32_t)bkd::kMaxJC + 2u) return fail(BKD_ERR_INVALID_ARG, "too many step bins");
    g_plan_lanes.store(lanes);
    g_plan_jc.store(steps_per_chunk);
    g_plan_merge.store(merge_bytes);
    return BKD_OK;
}

int bkd_set_short_class_mean(uint64_t max_bytes_per_entry) {
    g_short_mean_max.store(max_bytes_per_entry);
    return BKD_OK;
}

int bkd_set_plan_small(uint32_t max_bytes) {
    if (max_bytes > kSmallMaxBytes || (max_bytes && max_bytes < 16u))
        return fail(BKD_ERR_INVALID_ARG, "short-entry class bound must be 0 or 16.." + std::to_string(kSmallMaxBytes));
    g_plan_small.store(max_bytes);
    return BKD_OK;
}

int bkd_set_plan_serial(uint32_t max_bytes) {
    if (max_bytes < 16u || max_bytes > bkd::kSerialMax)
        return fail(BKD_ERR_INVALID_ARG, "serial bound must be 16.." + std::to_string(bkd::kSerialMax));
    g_plan_serial.store(max_bytes);
    return BKD_OK;
}

int bkd_get_group_lanes(int algo, uint64_t mean_len) {
    (void)algo;
    return auto_lanes(mean_len);
}

int bkd_crc_batch_uniform(int algo, const void* d_base, uint64_t stride, uint32_t entry_len, uint64_t n,
                          const uint32_t* d_seeds, uint32_t seed_all, uint32_t* d_out, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n && (!d_base || !d_out)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n > 1 && stride < entry_len) return fail(BKD_ERR_INVALID_ARG, "stride < entry_len");
    Call call(stream);
    if (call.rc) return call.rc;
    bkd::UniformSrc src{n, stride, entry_len, d_seeds, seed_all, d_out};
    // entries of 16..48 B: one lane per entry, both loads of an entry in flight with the next
    // entry's (uniform_small_loop): 2.2x the 4-lane rate at 32 B; from 64 B on 4 lanes win
    int lanes = auto_lanes(entry_len, n, call.ds->cus);
    if (g_forced_lanes.load() == 0 && entry_len >= 16u && entry_len <= 48u && n >= (uint64_t)call.ds->cus * bkd::kBlock)
        lanes = 1;
    // 256..511 B: 8 lanes (two to four 128-byte steps; the three-set short loop up to 384 B) beat 4
    // lanes since the short loop's waits are countable: 256 B 0.934 vs 1.028 ms, 512 B 0.826 vs
    // 0.915 ms per 4 GiB (profiles/r03v_size_sweep.log); indexed batches keep auto_lanes
    if (g_forced_lanes.load() == 0 && lanes == 4 && entry_len >= 256u && entry_len < 512u) lanes = 8;
    if (lanes == 8 && entry_len >= bkd::kTailUncondSteps * 16u * 8u)  // measured at 8 lanes only
        return dispatch_lanes(*call.ds, lanes, algo, (const uint8_t*)d_base, bkd::UniformLongSrc{src}, n, call.st);
    return dispatch_lanes(*call.ds, lanes, algo, (const uint8_t*)d_base, src, n, call.st);
}

int bkd_crc_batch(int algo, const void* d_base, uint64_t base_size, const uint64_t* d_offsets,
                  const uint32_t* d_lengths, uint64_t n, const uint32_t* d_seeds, uint32_t seed_all,
                  uint32_t* d_out, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n && (!d_offsets || !d_lengths || !d_out)) return fail(BKD_ERR_INVALID_ARG, "null index/out");
    if (n && !d_base && base_size) return fail(BKD_ERR_INVALID_ARG, "null base");
    Call call(stream);
    if (call.rc) return call.rc;
    return indexed_batch(*call.ds, algo, (const uint8_t*)d_base, base_size, d_offsets, d_lengths, n, d_seeds, seed_all,
                         d_out, call.st);
}

int bkd_stream_sync(void* stream) {
    Call call(stream);
    if (call.rc) return call.rc;
    StreamScratch* scp = scratch_find(*call.ds, call.st);  // (no entry for streams that only sync)
    if (!scp) {
        BKD_HIP(hipStreamSynchronize(call.st));
        return BKD_OK;
    }
    StreamScratch& sc = *scp;
    std::lock_guard<std::recursive_mutex> lk(sc.mu);
    if (!sc.err) {  // nothing indexed was ever enqueued on this stream
        BKD_HIP(hipStreamSynchronize(call.st));
        return BKD_OK;
    }
    // read and clear this stream's flag in stream order, after the work it guards
    BKD_HIP(hipMemcpyAsync(sc.h_err, sc.err, sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
    BKD_HIP(hipMemsetAsync(sc.err, 0, sizeof(uint32_t), call.st));
    BKD_HIP(hipStreamSynchronize(call.st));
    if (*sc.h_err) return fail(BKD_ERR_BOUNDS, kBoundsMsg);
    return BKD_OK;
}

int bkd_stream_release(void* stream) {
    Call call(stream);
    if (call.rc) return call.rc;
    std::unique_ptr<StreamScratch> sc;
    {
        std::unique_lock<std::shared_mutex> wr(call.ds->maps_mu);
        auto it = call.ds->scratch.find(call.st);
        if (it == call.ds->scratch.end()) {
            BKD_HIP(hipStreamSynchronize(call.st));
            return BKD_OK;
        }
        sc = std::move(it->second);
        call.ds->scratch.erase(it);
    }
    int status = BKD_OK;
    {
        std::lock_guard<std::recursive_mutex> lk(sc->mu);
        BKD_HIP(hipStreamSynchronize(call.st));  // the stream's kernels are done with the scratch
        if (sc->err) {
            BKD_HIP(hipMemcpy(sc->h_err, sc->err, sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (*sc->h_err) status = fail(BKD_ERR_BOUNDS, kBoundsMsg);
        }
        BKD_HIP(hipStreamSynchronize(call.st));  // the stream's own work is done with them
        for (int k = 0; k < StreamScratch::kSlots; ++k)
            if (sc->buf[k]) BKD_HIP(hipFree(sc->buf[k]));
        for (uint32_t* w : {sc->err, sc->run, sc->uni, sc->vflag})
            if (w) BKD_HIP(hipFree(w));
        if (sc->h_err) BKD_HIP(hipHostFree(sc->h_err));
    }
    return status;
}

int bkd_crc_batch_host(int algo, const void* h_base, uint64_t base_size, const uint64_t* h_offsets,
                       const uint32_t* h_lengths, uint64_t n, const uint32_t* h_seeds, uint32_t seed_all,
                       uint32_t* h_out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!h_offsets || !h_lengths || !h_out || (!h_base && base_size)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    bool sorted = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (h_offsets[i] > base_size || (uint64_t)h_lengths[i] > base_size - h_offsets[i])
            return fail(BKD_ERR_BOUNDS, "entry " + std::to_string(i) + " exceeds base buffer");
        if (i && h_offsets[i] < h_offsets[i - 1]) sorted = false;
    }
    const int route = host_route();
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::crc_indexed(algo, (const uint8_t*)h_base, h_offsets, h_lengths, n, h_seeds, seed_all, h_out);
        return BKD_OK;
    }
    StagedCall call;
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    if (!sorted) return host_batch_oneshot(*call.ds, hs, algo, (const uint8_t*)h_base, base_size, h_offsets, h_lengths, n,
                                           h_seeds, seed_all, h_out);
    uint64_t pieces = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (h_lengths[i] > HostStage::kSeg) pieces += (h_lengths[i] + HostStage::kSeg - 1) / HostStage::kSeg - 1;
    if (pieces == 0)
        return host_batch_pipelined(*call.ds, hs, algo, (const uint8_t*)h_base, h_offsets, h_lengths, n, h_seeds, seed_all,
                                    h_out);
    // Entries longer than a staging segment go through the pipeline as segment-sized pieces (the
    // first with the entry's seed, the others with seed ~0, i.e. their zero-initialised registers)
    // and are joined here, reg = reg * x^(8 len) ^ raw, as the device plan joins its chunks.
    const uint64_t m = n + pieces;
    std::vector<uint64_t> off2(m);
    std::vector<uint32_t> len2(m), seed2(m), out2(m);
    for (uint64_t i = 0, j = 0; i < n; ++i) {
        uint64_t o = h_offsets[i], left = h_lengths[i];
        seed2[j] = h_seeds ? h_seeds[i] : seed_all;
        do {
            const uint32_t l = (uint32_t)std::min<uint64_t>(left, HostStage::kSeg);
            off2[j] = o;
            len2[j] = l;
            if (o != h_offsets[i]) seed2[j] = 0xFFFFFFFFu;
            o += l;
            left -= l;
            ++j;
        } while (left);
    }
    // the pipeline walks offsets in order: an entry that starts inside a long entry's later pieces
    // (overlapping entries are legal, only bounds are checked) breaks that order, so such a
    // batch takes the one-copy route instead
    for (uint64_t j = 1; j < m; ++j)
        if (off2[j] < off2[j - 1])
            return host_batch_oneshot(*call.ds, hs, algo, (const uint8_t*)h_base, base_size, h_offsets, h_lengths, n,
                                      h_seeds, seed_all, h_out);
    const int rc = host_batch_pipelined(*call.ds, hs, algo, (const uint8_t*)h_base, off2.data(), len2.data(), m, seed2.data(),
                                        0, out2.data());
    if (rc) return rc;
    const uint32_t xseg = bkd::gf2::xpow(algo, 8ull * HostStage::kSeg);
    for (uint64_t i = 0, j = 0; i < n; ++i) {
        uint32_t reg = ~out2[j++];
        for (uint64_t at = HostStage::kSeg; at < h_lengths[i]; at += HostStage::kSeg, ++j)
            reg = bkd::gf2::mul(algo, reg, len2[j] == HostStage::kSeg ? xseg : bkd::gf2::xpow(algo, 8ull * len2[j])) ^
                  ~out2[j];
        h_out[i] = h_lengths[i] > HostStage::kSeg ? ~reg : out2[j - 1];
    }
    return BKD_OK;
}

int bkd_cpu_resume(int algo, uint32_t current, const void* h_ptr, uint64_t len, uint32_t* out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!out) return fail(BKD_ERR_INVALID_ARG, "null out");
    if (len && !h_ptr) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    return cpu_resume(algo, current, h_ptr, len, out);
}

int bkd_resume_host(int algo, uint32_t current, const void* h_ptr, uint64_t len, uint32_t* out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!out) return fail(BKD_ERR_INVALID_ARG, "null out");
    if (len == 0) {  // crc32c_sse42.cpp:211-213: resume of nothing returns the seed
        *out = current;
        return BKD_OK;
    }
    if (!h_ptr) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (len <= cpu_route_max() || visible_devices() <= 0)
        return cpu_resume(algo, current, h_ptr, len, out);
    // entries are indexed with 32-bit lengths: a longer buffer resumes piece by piece
    // (Sse42Crc32C.resume takes a long length, Sse42Crc32C.java:105-107)
    const uint8_t* p = (const uint8_t*)h_ptr;
    uint32_t r = current;
    for (uint64_t at = 0; at < len;) {
        const uint64_t off = 0;
        const uint32_t l32 = (uint32_t)std::min<uint64_t>(len - at, kResumePiece);
        const int rc = bkd_crc_batch_host(algo, p + at, l32, &off, &l32, 1, nullptr, r, &r);
        if (rc == BKD_ERR_HIP || rc == BKD_ERR_NOMEM || rc == BKD_ERR_NO_DEVICE)
            // a device that fails (init, allocation, a copy) degrades to the CPU route, never to an
            // error: the reference's provider chain never throws (Crc32cIntChecksum.java:28-36)
            return cpu_resume(algo, current, h_ptr, len, out);
        if (rc) return rc;
        at += l32;
    }
    *out = r;
    return BKD_OK;
}

int bkd_resume_device(int algo, uint32_t current, const void* d_ptr, uint64_t len, void* stream, uint32_t* out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!out) return fail(BKD_ERR_INVALID_ARG, "null out");
    if (len == 0) {
        *out = current;
        return BKD_OK;
    }
    if (!d_ptr) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    const uint8_t* p = (const uint8_t*)d_ptr;
    for (uint64_t at = 0; at < len;) {  // 32-bit entry lengths: longer buffers piece by piece
        const uint64_t l = std::min<uint64_t>(len - at, kResumePiece);
        const int rc = resume_device(algo, current, p + at, l, (hipStream_t)stream, &current);
        if (rc) return rc;
        at += l;
    }
    *out = current;
    return BKD_OK;
}

int bkd_resume(int algo, uint32_t current, const void* ptr, uint64_t len, uint32_t* out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!out) return fail(BKD_ERR_INVALID_ARG, "null out");
    if (len == 0) {
        *out = current;
        return BKD_OK;
    }
    if (!ptr) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    // a device buffer runs on the null stream, which orders the call after the work queued on
    // the blocking streams (PyTorch's default stream among them) that may still be writing it
    int pdev = -1;
    const hipMemoryType where = visible_devices() > 0 ? pointer_type(ptr, &pdev) : hipMemoryTypeUnregistered;
    if (where == hipMemoryTypeDevice || where == hipMemoryTypeManaged) {
        // on the null stream of the device that holds the buffer (not whichever is current)
        int cur = 0;
        BKD_HIP(hipGetDevice(&cur));
        DeviceScope scope;
        if (pdev >= 0 && pdev != cur) {
            BKD_HIP(hipSetDevice(pdev));
            scope.prev = cur;
        }
        return bkd_resume_device(algo, current, ptr, len, nullptr, out);
    }
    return bkd_resume_host(algo, current, ptr, len, out);
}

int bkd_circe_supported(void) { return 1; }

int64_t bkd_circe_alloc_config(const int32_t* chunk_words, int32_t len) {
    constexpr int32_t kMinWords = 4;  // chunk_config::min_words (crc32c_sse42.hpp:22)
    if (!chunk_words || len < 1 || chunk_words[0] < kMinWords) return 0;
    for (int32_t i = 1; i < len; ++i)
        if (chunk_words[i] < kMinWords || chunk_words[i] >= chunk_words[i - 1]) return 0;  // strictly decreasing
    int32_t* cfg = new (std::nothrow) int32_t[(size_t)len + 1];
    if (!cfg) return 0;
    cfg[0] = len;
    memcpy(cfg + 1, chunk_words, (size_t)len * sizeof(int32_t));
    return (int64_t)(intptr_t)cfg;
}

void bkd_circe_free_config(int64_t config) { delete[] (int32_t*)(intptr_t)config; }

int bkd_set_cpu_route_max(uint64_t bytes) {
    g_cpu_route_max.store(bytes);
    return BKD_OK;
}

uint64_t bkd_get_cpu_route_max(void) { return cpu_route_max(); }

const char* bkd_cpu_impl(void) { return bkd::host::impl_name(); }

int bkd_set_host_batch_route(int route) {
    if (route < 0 || route > 2) return fail(BKD_ERR_INVALID_ARG, "host batch route must be 0 (auto), 1 (CPU) or 2 (GPU)");
    g_host_route.store(route);
    return BKD_OK;
}

int bkd_get_host_batch_route(void) {
    const int r = host_route();
    return r < 0 ? 2 : r;
}

int bkd_set_host_threads(int threads) {
    if (threads < 0) return fail(BKD_ERR_INVALID_ARG, "threads must be >= 0");
    bkd::host::Pool::get().set_active(threads);
    return BKD_OK;
}

int bkd_get_host_threads(void) { return bkd::host::Pool::get().active(); }

int bkd_host_release(void) {
    for (int d = 0; d < kMaxDevices; ++d) {
        StagePool& pool = g_stages[d];
        std::vector<std::unique_ptr<HostStage>> gone;
        {
            std::lock_guard<std::mutex> lk(pool.mu);
            for (HostStage* hs : pool.idle) {
                auto it = std::find_if(pool.all.begin(), pool.all.end(),
                                       [&](const std::unique_ptr<HostStage>& p) { return p.get() == hs; });
                if (it != pool.all.end()) {
                    gone.push_back(std::move(*it));
                    pool.all.erase(it);
                }
            }
            pool.idle.clear();
        }
        if (!gone.empty()) {
            int prev = 0;
            if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(d) == hipSuccess) {
                gone.clear();  // frees the pinned and device buffers, streams and events
                (void)hipSetDevice(prev);
            }
        }
        pool.cv.notify_all();  // callers waiting for a set may create one again
    }
    return BKD_OK;
}

int bkd_digest_package_batch(int algo, int64_t ledger_id, const int64_t* d_entry_ids, const int64_t* d_lacs,
                             const int64_t* d_length_fields, const void* d_payload, uint64_t payload_size,
                             const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, void* d_frames,
                             uint64_t frame_stride, uint32_t* d_digests, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths || !d_frames || !d_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(32u + mac_len(algo), frame_stride, false)) return rc;
    Call call(stream);
    if (call.rc) return call.rc;
    return package_framed(*call.ds, call.st, algo, ledger_id, d_entry_ids, d_lacs, d_length_fields, d_payload, payload_size,
                          d_offsets, d_lengths, n, d_frames, frame_stride, d_digests);
}

int bkd_digest_verify_batch(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                            const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                            const uint32_t* d_lengths, uint64_t n, int32_t* d_status, uint64_t* d_first_bad,
                            void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!d_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    Call call(stream);
    if (call.rc) return call.rc;
    return verify_framed(*call.ds, call.st, algo, ledger_id, first_entry_id, skip_entry_check ? 1 : 0, d_framed, framed_size,
                         d_offsets, d_lengths, n, d_status, d_first_bad);
}

int bkd_digest_package_batch_ledgers(int algo, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                     const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                     uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                                     uint64_t n, void* d_frames, uint64_t frame_stride, uint32_t* d_digests,
                                     void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!d_ledger_ids || !d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths || !d_frames ||
        !d_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(32u + mac_len(algo), frame_stride, false)) return rc;
    Call call(stream);
    if (call.rc) return call.rc;
    return package_framed(*call.ds, call.st, algo, 0, d_entry_ids, d_lacs, d_length_fields, d_payload, payload_size,
                          d_offsets, d_lengths, n, d_frames, frame_stride, d_digests, d_ledger_ids);
}

int bkd_digest_verify_requests(int algo, const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                               const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first, uint64_t nreq,
                               const int64_t* d_req_ledger_ids, const int64_t* d_req_first_entry_ids,
                               const uint32_t* d_req_flags, int32_t* d_status, uint64_t* d_req_first_bad,
                               void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (nreq >= 0x80000000ull) return fail(BKD_ERR_INVALID_ARG, "a call holds fewer than 2^31 requests");
    if (nreq == 0) return n ? fail(BKD_ERR_INVALID_ARG, "entries without a request") : BKD_OK;
    if (!d_req_first || !d_req_ledger_ids || !d_req_first_entry_ids || !d_req_flags || !d_req_first_bad)
        return fail(BKD_ERR_INVALID_ARG, "null request array");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    Call call(stream);
    if (call.rc) return call.rc;
    const Requests rq{nreq, d_req_first, d_req_ledger_ids, d_req_first_entry_ids, d_req_flags, d_req_first_bad};
    return verify_framed(*call.ds, call.st, algo, 0, 0, 0, d_framed, framed_size, d_offsets, d_lengths, n, d_status,
                         nullptr, &rq);
}

int bkd_digest_verify_batch_host(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                                 const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                 int32_t* h_status, uint64_t* h_first_bad) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!h_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    *h_first_bad = n;
    if (n == 0) return BKD_OK;
    if (!h_frames || !h_lengths || !h_status) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_host_entries("frame", h_frames, h_lengths, n)) return rc;
    const int route = framed_host_route(h_lengths, n);
    if (route < 0) return route;
    const int id_checks = skip_entry_check ? 1 : 0;
    if (route == 1) {
        *h_first_bad = bkd::host::verify_frames(algo, ledger_id, first_entry_id, id_checks,
                                                (const uint8_t* const*)h_frames, h_lengths, n, h_status);
        return BKD_OK;
    }
    return verify_host_staged(
        [&](DeviceState& ds, HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t bytes) {
            return verify_framed(ds, hs.st[s], algo, ledger_id, first_entry_id + (int64_t)i0, id_checks, hs.d_buf[s],
                                 bytes, hs.d_off[s], hs.d_len[s], cnt, reinterpret_cast<int32_t*>(hs.d_res[s]),
                                 hs.d_fb[s]);
        },
        h_frames, h_lengths, n, h_status, h_first_bad);
}

int bkd_digest_package_batch_host(int algo, int64_t ledger_id, const int64_t* h_entry_ids, const int64_t* h_lacs,
                                  const int64_t* h_length_fields, const void* const* h_payloads,
                                  const uint32_t* h_lengths, uint64_t n, void* h_frames, uint64_t frame_stride,
                                  uint32_t* h_digests) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    const uint64_t hl = 32u + mac_len(algo);
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths || !h_frames || !h_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    if (int rc = check_host_entries("payload", h_payloads, h_lengths, n)) return rc;
    const int route = framed_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::package_frames(algo, ledger_id, h_entry_ids, h_lacs, h_length_fields,
                                  (const uint8_t* const*)h_payloads, h_lengths, n, (uint8_t*)h_frames, frame_stride,
                                  h_digests);
        return BKD_OK;
    }
    return package_host_staged(nullptr, h_entry_ids, h_lacs, h_length_fields, entry_buffers(h_payloads, h_lengths),
                               h_lengths, n, crc_package(algo, ledger_id), frame_stride, true,
                               host_frames(hl, frame_stride, h_frames, frame_stride, h_digests));
}

int bkd_digest_package_batch_v2(int algo, int64_t ledger_id, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                const uint8_t* d_master_keys, uint64_t key_stride, uint32_t flags,
                                uint32_t small_threshold, void* d_requests, uint64_t requests_size,
                                const uint64_t* d_request_offsets, uint32_t* d_digests, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (int rc = check_v2_args(key_stride, flags)) return rc;
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths || !d_master_keys || !d_requests ||
        !d_request_offsets || !d_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    Call call(stream);
    if (call.rc) return call.rc;
    return package_v2(*call.ds, call.st, algo, ledger_id, d_ledger_ids, d_entry_ids, d_lacs, d_length_fields, d_payload,
                      payload_size, d_offsets, d_lengths, n, d_master_keys, key_stride,
                      bkd::host::v2_packet_header(flags), small_threshold, d_requests, requests_size,
                      d_request_offsets, d_digests);
}

int bkd_digest_package_batch_v2_host(int algo, int64_t ledger_id, const int64_t* h_ledger_ids,
                                     const int64_t* h_entry_ids, const int64_t* h_lacs, const int64_t* h_length_fields,
                                     const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                     const uint8_t* h_master_keys, uint64_t key_stride, uint32_t flags,
                                     uint32_t small_threshold, void* const* h_requests, uint32_t* h_digests) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (int rc = check_v2_args(key_stride, flags)) return rc;
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths || !h_master_keys || !h_requests ||
        !h_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_v2_entries(h_payloads, h_lengths, h_requests, n)) return rc;
    const int route = framed_host_route(h_lengths, n);
    if (route < 0) return route;
    const bkd::host::V2Head head{h_master_keys, key_stride, bkd::host::v2_packet_header(flags), small_threshold};
    const uint8_t* const* payloads = (const uint8_t* const*)h_payloads;
    uint8_t* const* requests = (uint8_t* const*)h_requests;
    if (route == 1) {
        bkd::host::package_requests_v2(algo, ledger_id, h_ledger_ids, h_entry_ids, h_lacs, h_length_fields, payloads,
                                       h_lengths, n, head, requests, h_digests);
        return BKD_OK;
    }
    // GPU: staged and digested as bkd_digest_package_batch_host; each finished segment's packed frames
    // go into the requests behind the prefix the host writes, the small payloads from their sources
    const uint64_t hl = 32u + mac_len(algo);
    return package_host_staged(h_ledger_ids, h_entry_ids, h_lacs, h_length_fields, entry_buffers(h_payloads, h_lengths),
                               h_lengths, n, crc_package(algo, ledger_id), hl, true,
                               [&](const uint8_t* frm, const uint32_t* res, uint64_t i0, uint64_t cnt) {
                                   bkd::host::finish_requests_v2(algo, frm, payloads + i0, h_lengths + i0, cnt, head, i0,
                                                                 requests + i0, copy_threads());
                                   memcpy(h_digests + i0, res, cnt * 4);
                               });
}

int bkd_digest_verify_requests_host(int algo, const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                    const uint64_t* h_req_first, uint64_t nreq, const int64_t* h_req_ledger_ids,
                                    const int64_t* h_req_first_entry_ids, const uint32_t* h_req_flags,
                                    int32_t* h_status, uint64_t* h_req_first_bad) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    return verify_requests_host(
        nullptr, h_frames, h_lengths, n, h_req_first, nreq, h_req_ledger_ids, h_req_first_entry_ids, h_req_flags, h_status,
        h_req_first_bad,
        [&](const int64_t* xlid, const int64_t* xeid, const uint32_t* req_of) {
            const int route = framed_host_route(h_lengths, n);
            if (route == 1)
                bkd::host::verify_frames_expected(algo, xlid, xeid, req_of, (const uint8_t* const*)h_frames, h_lengths, n,
                                                  h_status);
            return route;
        },
        // every staged entry belongs to the segment's one request 0, which starts at its entry 0 (x.d_zero)
        [&](DeviceState& ds, HostStage& hs, int s, uint64_t cnt, uint64_t bytes, const StagedRequests& x) {
            Requests rq{1, x.d_zero, nullptr, nullptr, nullptr, hs.d_fb[s]};
            rq.exp_lid = x.d_lid;
            rq.exp_eid = x.d_eid;
            rq.req_of = x.d_flag;
            return verify_framed(ds, hs.st[s], algo, 0, 0, 0, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt,
                                 reinterpret_cast<int32_t*>(hs.d_res[s]), nullptr, &rq);
        },
        NothingDrained{}, &HostStage::init_verify, &HostStage::init_requests);
}

int bkd_digest_package_batch_ledgers_host(int algo, const int64_t* h_ledger_ids, const int64_t* h_entry_ids,
                                          const int64_t* h_lacs, const int64_t* h_length_fields,
                                          const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                          void* h_frames, uint64_t frame_stride, uint32_t* h_digests) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    const uint64_t hl = 32u + mac_len(algo);
    if (n == 0) return BKD_OK;
    if (!h_ledger_ids || !h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths || !h_frames ||
        !h_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    if (int rc = check_host_entries("payload", h_payloads, h_lengths, n)) return rc;
    const int route = framed_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::package_frames_ledgers(algo, h_ledger_ids, h_entry_ids, h_lacs, h_length_fields,
                                          (const uint8_t* const*)h_payloads, h_lengths, n, (uint8_t*)h_frames,
                                          frame_stride, h_digests);
        return BKD_OK;
    }
    return package_host_staged(h_ledger_ids, h_entry_ids, h_lacs, h_length_fields, entry_buffers(h_payloads, h_lengths),
                               h_lengths, n, crc_package(algo, 0), frame_stride, true,
                               host_frames(hl, frame_stride, h_frames, frame_stride, h_digests));
}

int bkd_digest_reframe_batch(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check, uint32_t flags,
                             void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                             const uint32_t* d_lengths, uint64_t n, const int64_t* d_new_lacs, void* d_out_frames,
                             uint64_t frame_stride, uint32_t* d_digests, int32_t* d_status, uint64_t* d_first_bad,
                             void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (flags & ~BKD_REFRAME_TRUSTED) return fail(BKD_ERR_INVALID_ARG, "unknown reframe flags");
    if (!d_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    if (n && !d_new_lacs) return fail(BKD_ERR_INVALID_ARG, "null new_lacs");
    const uint32_t mac = mac_len(algo);
    if (n && d_out_frames) {
        if (int rc = check_frame_stride(32u + mac, frame_stride, false)) return rc;
        const uint64_t fr0 = (uint64_t)(uintptr_t)d_out_frames, fr1 = fr0 + (n - 1u) * frame_stride + 32u + mac;
        const uint64_t in0 = (uint64_t)(uintptr_t)d_framed, in1 = in0 + framed_size;
        if (fr0 < in1 && in0 < fr1) return fail(BKD_ERR_INVALID_ARG, "out_frames overlaps the framed buffer");
    }
    Call call(stream);
    if (call.rc) return call.rc;
    return reframe_framed(*call.ds, call.st, algo, ledger_id, first_entry_id, skip_entry_check ? 1 : 0,
                          (flags & BKD_REFRAME_TRUSTED) != 0, d_framed, framed_size, d_offsets, d_lengths, n, d_new_lacs,
                          d_out_frames, frame_stride, d_digests, d_status, d_first_bad);
}

int bkd_digest_reframe_batch_host(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                                  uint32_t flags, void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                  const int64_t* h_new_lacs, uint32_t* h_digests, int32_t* h_status,
                                  uint64_t* h_first_bad) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (flags & ~BKD_REFRAME_TRUSTED) return fail(BKD_ERR_INVALID_ARG, "unknown reframe flags");
    if (!h_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    *h_first_bad = n;
    if (n == 0) return BKD_OK;
    if (!h_frames || !h_lengths || !h_status) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (!h_new_lacs) return fail(BKD_ERR_INVALID_ARG, "null new_lacs");
    if (int rc = check_host_entries("frame", h_frames, h_lengths, n)) return rc;
    const bool trusted = (flags & BKD_REFRAME_TRUSTED) != 0;
    const int id_checks = skip_entry_check ? 1 : 0;
    const int route = framed_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        *h_first_bad = bkd::host::reframe_frames(algo, ledger_id, first_entry_id, id_checks, trusted,
                                                 (uint8_t* const*)h_frames, h_lengths, n, h_new_lacs, h_digests,
                                                 h_status);
        return BKD_OK;
    }
    StagedCall call(&HostStage::init_verify, &HostStage::init_reframe);
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    // staged as verify; the device reframes its copy in place and only status and digests come back
    // (d_seed / h_seed carry the digests), then the host threads write each OK frame's 12 bytes
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        const hipStream_t st = hs.st[s];
        int r = stage_entries(hs, s, h_frames, h_lengths, i0, cnt, bytes);
        if (r) return r;
        memcpy(hs.h_lac[s], h_new_lacs + i0, cnt * 8);
        BKD_HIP(hipMemcpyAsync(hs.d_lac[s], hs.h_lac[s], cnt * 8, hipMemcpyHostToDevice, st));
        uint64_t* d_fb = hs.d_fb[s];
        r = reframe_framed(*call.ds, st, algo, ledger_id, first_entry_id + (int64_t)i0, id_checks, trusted, hs.d_buf[s],
                           bytes, hs.d_off[s], hs.d_len[s], cnt, hs.d_lac[s], nullptr, 0, hs.d_seed[s],
                           reinterpret_cast<int32_t*>(hs.d_res[s]), d_fb);
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st));
        BKD_HIP(hipMemcpyAsync(hs.h_seed[s], hs.d_seed[s], cnt * 4, hipMemcpyDeviceToHost, st));
        BKD_HIP(hipMemcpyAsync(hs.h_fb[s], d_fb, 8, hipMemcpyDeviceToHost, st));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        memcpy(h_status + i0, hs.h_res[s], cnt * 4);
        if (h_digests) memcpy(h_digests + i0, hs.h_seed[s], cnt * 4);
        bkd::host::apply_reframe(algo, (uint8_t* const*)h_frames + i0, cnt, h_new_lacs + i0,
                                 reinterpret_cast<const int32_t*>(hs.h_res[s]), hs.h_seed[s]);
        merge_first_bad(hs, s, i0, cnt, h_first_bad);
        return BKD_OK;
    };
    return host_segments(hs, h_lengths, n, HostStage::kSegEntries, seg, drain);
}

// ---- MAC ledgers (HMAC-SHA1) ------------------------------------------------------------------

int bkd_mac_gen_digest(const char* pad, const void* passwd, uint64_t passwd_len, uint8_t* out20) {
    if (!pad || !out20 || (passwd_len && !passwd)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    bkd::host::mac_gen_digest(pad, (const uint8_t*)passwd, passwd_len, out20);
    return BKD_OK;
}

int bkd_mac_key_init(const void* passwd, uint64_t passwd_len, uint32_t* key_state10) {
    if (!key_state10 || (passwd_len && !passwd)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    bkd::host::mac_key_init((const uint8_t*)passwd, passwd_len, key_state10);
    return BKD_OK;
}

int bkd_mac_key_state(const void* key, uint64_t key_len, uint32_t* key_state10) {
    if (!key_state10 || (key_len && !key)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (key_len > 64u) return fail(BKD_ERR_INVALID_ARG, "an HMAC key longer than a block is hashed first: pass its SHA-1");
    bkd::host::mac_key_state((const uint8_t*)key, (size_t)key_len, key_state10);
    return BKD_OK;
}

int bkd_mac_cpu(const uint32_t* key_state, const void* h_ptr, uint64_t len, uint8_t* out20) {
    if (!key_state || !out20 || (len && !h_ptr)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    bkd::host::mac_one(key_state, nullptr, 0, (const uint8_t*)h_ptr, len, out20);
    return BKD_OK;
}

int bkd_mac_batch(const uint32_t* key_state, const void* d_base, uint64_t base_size, const uint64_t* d_offsets,
                  const uint32_t* d_lengths, uint64_t n, uint8_t* d_out, void* stream) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (n == 0) return BKD_OK;
    if (!d_offsets || !d_lengths || !d_out) return fail(BKD_ERR_INVALID_ARG, "null index/out");
    if (!d_base && base_size) return fail(BKD_ERR_INVALID_ARG, "null base");
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_raw(*call.ds, call.st, key_state, d_base, base_size, d_offsets, d_lengths, n, d_out);
}

int bkd_digest_package_batch_mac(const uint32_t* key_state, int64_t ledger_id, const int64_t* d_entry_ids,
                                 const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                 uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                 void* d_frames, uint64_t frame_stride, void* stream) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths || !d_frames)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(bkd::host::kMacFrameHead, frame_stride, false)) return rc;
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_package(*call.ds, call.st, bkd::MacOneLedger{mac_key(key_state), ledger_id}, d_entry_ids, d_lacs,
                       d_length_fields, d_payload, payload_size, d_offsets, d_lengths, n, d_frames, frame_stride);
}

int bkd_digest_verify_batch_mac(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id,
                                int skip_entry_check, const void* d_framed, uint64_t framed_size,
                                const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, int32_t* d_status,
                                uint64_t* d_first_bad, void* stream) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (!d_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_verify(*call.ds, call.st, key_state, ledger_id, first_entry_id, skip_entry_check ? 1 : 0, d_framed,
                      framed_size, d_offsets, d_lengths, n, d_status, d_first_bad);
}

int bkd_mac_batch_host(const uint32_t* key_state, const void* const* h_entries, const uint32_t* h_lengths, uint64_t n,
                       uint8_t* h_out) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (n == 0) return BKD_OK;
    if (!h_entries || !h_lengths || !h_out) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_host_entries("entry", h_entries, h_lengths, n)) return rc;
    const int route = mac_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::mac_list(key_state, (const uint8_t* const*)h_entries, h_lengths, n, h_out);
        return BKD_OK;
    }
    StagedCall call(&HostStage::init_package);  // the MACs come back through the frame buffers (20 B per entry)
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        int r = stage_entries(hs, s, h_entries, h_lengths, i0, cnt, bytes);
        if (r) return r;
        r = mac_raw(*call.ds, hs.st[s], key_state, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt, hs.d_frm[s]);
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_frm[s], hs.d_frm[s], cnt * bkd::host::kMacLen, hipMemcpyDeviceToHost, hs.st[s]));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        memcpy(h_out + i0 * bkd::host::kMacLen, hs.h_frm[s], cnt * bkd::host::kMacLen);
        return BKD_OK;
    };
    return host_segments(hs, h_lengths, n, HostStage::kSegEntries, seg, drain);
}

int bkd_digest_package_batch_mac_host(const uint32_t* key_state, int64_t ledger_id, const int64_t* h_entry_ids,
                                      const int64_t* h_lacs, const int64_t* h_length_fields,
                                      const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                      void* h_frames, uint64_t frame_stride) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths || !h_frames)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    constexpr uint64_t hl = bkd::host::kMacFrameHead;
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    if (int rc = check_host_entries("entry", h_payloads, h_lengths, n)) return rc;
    const int route = mac_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::mac_package_frames(key_state, ledger_id, h_entry_ids, h_lacs, h_length_fields,
                                      (const uint8_t* const*)h_payloads, h_lengths, n, (uint8_t*)h_frames, frame_stride);
        return BKD_OK;
    }
    // the device writes packed 52-byte frames and no digest words; the host puts each frame at its stride
    auto launch = [=](DeviceState& ds, HostStage& hs, int s, const int64_t* d_ids, const int64_t*, uint64_t cnt,
                      uint64_t bytes, uint64_t stride) {
        return mac_package(ds, hs.st[s], bkd::MacOneLedger{mac_key(key_state), ledger_id}, d_ids, d_ids + cnt,
                           d_ids + 2 * cnt, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt, hs.d_frm[s], stride);
    };
    return package_host_staged(nullptr, h_entry_ids, h_lacs, h_length_fields, entry_buffers(h_payloads, h_lengths),
                               h_lengths, n, launch, hl, false, host_frames(hl, hl, h_frames, frame_stride, nullptr));
}

int bkd_digest_verify_batch_mac_host(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id,
                                     int skip_entry_check, const void* const* h_frames, const uint32_t* h_lengths,
                                     uint64_t n, int32_t* h_status, uint64_t* h_first_bad) {
    if (!key_state) return fail(BKD_ERR_INVALID_ARG, "null key state");
    if (!h_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    *h_first_bad = n;
    if (n == 0) return BKD_OK;
    if (!h_frames || !h_lengths || !h_status) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_host_entries("entry", h_frames, h_lengths, n)) return rc;
    const int route = mac_host_route(h_lengths, n);
    if (route < 0) return route;
    const int id_checks = skip_entry_check ? 1 : 0;
    if (route == 1) {
        *h_first_bad = bkd::host::mac_verify_frames(key_state, ledger_id, first_entry_id, id_checks,
                                                    (const uint8_t* const*)h_frames, h_lengths, n, h_status);
        return BKD_OK;
    }
    return verify_host_staged(
        [&](DeviceState& ds, HostStage& hs, int s, uint64_t i0, uint64_t cnt, uint64_t bytes) {
            return mac_verify(ds, hs.st[s], key_state, ledger_id, first_entry_id + (int64_t)i0, id_checks, hs.d_buf[s],
                              bytes, hs.d_off[s], hs.d_len[s], cnt, reinterpret_cast<int32_t*>(hs.d_res[s]), hs.d_fb[s]);
        },
        h_frames, h_lengths, n, h_status, h_first_bad);
}

int bkd_digest_verify_requests_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_req_keys,
                                   const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                                   const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first, uint64_t nreq,
                                   const int64_t* d_req_ledger_ids, const int64_t* d_req_first_entry_ids,
                                   const uint32_t* d_req_flags, int32_t* d_status, uint64_t* d_req_first_bad,
                                   void* stream) {
    if (nreq >= 0x80000000ull) return fail(BKD_ERR_INVALID_ARG, "a call holds fewer than 2^31 requests");
    if (nreq == 0) return n ? fail(BKD_ERR_INVALID_ARG, "entries without a request") : BKD_OK;
    if (!d_req_keys || !d_req_first || !d_req_ledger_ids || !d_req_first_entry_ids || !d_req_flags || !d_req_first_bad)
        return fail(BKD_ERR_INVALID_ARG, "null request array");
    if (nkeys && !d_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    const Requests rq{nreq, d_req_first, d_req_ledger_ids, d_req_first_entry_ids, d_req_flags, d_req_first_bad};
    return mac_verify_requests(*call.ds, call.st, MacKeys{d_key_states, nkeys, d_req_keys}, d_framed, framed_size,
                               d_offsets, d_lengths, n, d_status, rq);
}

int bkd_digest_package_batch_ledgers_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                         const int64_t* d_ledger_ids, const int64_t* d_entry_ids, const int64_t* d_lacs,
                                         const int64_t* d_length_fields, const void* d_payload, uint64_t payload_size,
                                         const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                         void* d_frames, uint64_t frame_stride, void* stream) {
    if (n == 0) return BKD_OK;
    if (!d_key_of || !d_ledger_ids || !d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths ||
        !d_frames)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !d_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (int rc = check_frame_stride(bkd::host::kMacFrameHead, frame_stride, false)) return rc;
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_package(*call.ds, call.st, bkd::MacLedgers{d_key_states, nkeys, d_key_of, d_ledger_ids}, d_entry_ids,
                       d_lacs, d_length_fields, d_payload, payload_size, d_offsets, d_lengths, n, d_frames, frame_stride);
}

int bkd_digest_verify_requests_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_req_keys,
                                        const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                        const uint64_t* h_req_first, uint64_t nreq, const int64_t* h_req_ledger_ids,
                                        const int64_t* h_req_first_entry_ids, const uint32_t* h_req_flags,
                                        int32_t* h_status, uint64_t* h_req_first_bad) {
    const MacKeys keys{h_key_states, nkeys, h_req_keys};
    DeviceTable table;  // uploaded once, by the first segment (the staged call has entered the device by then)
    return verify_requests_host(
        &keys, h_frames, h_lengths, n, h_req_first, nreq, h_req_ledger_ids, h_req_first_entry_ids, h_req_flags, h_status,
        h_req_first_bad,
        [&](const int64_t* xlid, const int64_t* xeid, const uint32_t* req_of) {
            const int route = mac_host_route(h_lengths, n);
            if (route == 1)
                bkd::host::mac_verify_frames_expected(h_key_states, h_req_keys, xlid, xeid, req_of,
                                                      (const uint8_t* const*)h_frames, h_lengths, n, h_status);
            return route;
        },
        // each entry's key row travels in the seeds buffer
        [&](DeviceState& ds, HostStage& hs, int s, uint64_t cnt, uint64_t bytes, const StagedRequests& x) -> int {
            if (int rc = table.upload(h_key_states, nkeys)) return rc;
            for (uint64_t j = 0; j < cnt; ++j) hs.h_seed[s][j] = h_req_keys[x.req_of[j] & ~bkd::host::kSkipEntryId];
            BKD_HIP(hipMemcpyAsync(hs.d_seed[s], hs.h_seed[s], cnt * 4, hipMemcpyHostToDevice, hs.st[s]));
            return mac_verify_expected(ds, hs.st[s], bkd::MacExpected{table.d, nkeys, hs.d_seed[s], x.d_lid, x.d_eid, x.d_flag},
                                       hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt,
                                       reinterpret_cast<int32_t*>(hs.d_res[s]));
        },
        NothingDrained{}, &HostStage::init_requests);
}

int bkd_digest_reframe_requests_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_req_keys,
                                    uint32_t flags, void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                                    const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first, uint64_t nreq,
                                    const int64_t* d_req_ledger_ids, const int64_t* d_req_first_entry_ids,
                                    const uint32_t* d_req_flags, const int64_t* d_new_lacs, void* d_out_frames,
                                    uint64_t frame_stride, int32_t* d_status, uint64_t* d_req_first_bad, void* stream) {
    if (flags & ~BKD_REFRAME_TRUSTED) return fail(BKD_ERR_INVALID_ARG, "unknown reframe flags");
    if (nreq >= 0x80000000ull) return fail(BKD_ERR_INVALID_ARG, "a call holds fewer than 2^31 requests");
    if (d_out_frames) {
        if (int rc = check_frame_stride(bkd::host::kMacFrameHead, frame_stride, false)) return rc;
    } else if (frame_stride != 0) {
        return fail(BKD_ERR_INVALID_ARG, "a frame stride without out_frames");
    }
    if (nreq == 0) return n ? fail(BKD_ERR_INVALID_ARG, "entries without a request") : BKD_OK;
    if (!d_req_keys || !d_req_first || !d_req_ledger_ids || !d_req_first_entry_ids || !d_req_flags || !d_req_first_bad)
        return fail(BKD_ERR_INVALID_ARG, "null request array");
    if (nkeys && !d_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_framed) return fail(BKD_ERR_INVALID_ARG, "null framed buffer");
    if (n && !d_new_lacs) return fail(BKD_ERR_INVALID_ARG, "null new_lacs");
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    if (n && d_out_frames) {
        const uint64_t fr0 = (uint64_t)(uintptr_t)d_out_frames, fr1 = fr0 + (n - 1u) * frame_stride + bkd::host::kMacFrameHead;
        const uint64_t in0 = (uint64_t)(uintptr_t)d_framed, in1 = in0 + framed_size;
        if (fr0 < in1 && in0 < fr1) return fail(BKD_ERR_INVALID_ARG, "out_frames overlaps the framed buffer");
    }
    Call call(stream);
    if (call.rc) return call.rc;
    const Requests rq{nreq, d_req_first, d_req_ledger_ids, d_req_first_entry_ids, d_req_flags, d_req_first_bad};
    const hipStream_t st = call.st;
    return mac_requests(*call.ds, st, MacKeys{d_key_states, nkeys, d_req_keys}, n, rq,
                        [&](const bkd::MacRequests& who, uint32_t* err) {
                            mac_reframe_launch(st, who, (flags & BKD_REFRAME_TRUSTED) != 0, d_framed, framed_size, d_offsets,
                                               d_lengths, n, d_new_lacs, d_out_frames, frame_stride, d_status, err);
                        });
}

int bkd_digest_reframe_requests_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_req_keys,
                                         uint32_t flags, void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                         const uint64_t* h_req_first, uint64_t nreq, const int64_t* h_req_ledger_ids,
                                         const int64_t* h_req_first_entry_ids, const uint32_t* h_req_flags,
                                         const int64_t* h_new_lacs, int32_t* h_status, uint64_t* h_req_first_bad) {
    if (flags & ~BKD_REFRAME_TRUSTED) return fail(BKD_ERR_INVALID_ARG, "unknown reframe flags");
    if (n && !h_new_lacs) return fail(BKD_ERR_INVALID_ARG, "null new_lacs");
    const bool trusted = (flags & BKD_REFRAME_TRUSTED) != 0;
    const MacKeys keys{h_key_states, nkeys, h_req_keys};
    DeviceTable table;  // uploaded once, by the first segment (the staged call has entered the device by then)
    constexpr uint64_t hl = bkd::host::kMacFrameHead;
    return verify_requests_host(
        &keys, h_frames, h_lengths, n, h_req_first, nreq, h_req_ledger_ids, h_req_first_entry_ids, h_req_flags, h_status,
        h_req_first_bad,
        [&](const int64_t* xlid, const int64_t* xeid, const uint32_t* req_of) {
            const int route = mac_host_route(h_lengths, n);
            if (route == 1)
                bkd::host::mac_reframe_frames_expected(h_key_states, h_req_keys, xlid, xeid, req_of, trusted,
                                                       (uint8_t* const*)h_frames, h_lengths, n, h_new_lacs, h_status);
            return route;
        },
        // staged as verify with the new LACs beside; the device leaves its copy of the frames alone and writes
        // packed 52-byte out-frames, which come back with the statuses
        [&](DeviceState& ds, HostStage& hs, int s, uint64_t cnt, uint64_t bytes, const StagedRequests& x) -> int {
            if (int rc = table.upload(h_key_states, nkeys)) return rc;
            const hipStream_t st = hs.st[s];
            for (uint64_t j = 0; j < cnt; ++j) hs.h_seed[s][j] = h_req_keys[x.req_of[j] & ~bkd::host::kSkipEntryId];
            BKD_HIP(hipMemcpyAsync(hs.d_seed[s], hs.h_seed[s], cnt * 4, hipMemcpyHostToDevice, st));
            memcpy(hs.h_lac[s], h_new_lacs + x.first, cnt * 8);
            BKD_HIP(hipMemcpyAsync(hs.d_lac[s], hs.h_lac[s], cnt * 8, hipMemcpyHostToDevice, st));
            const int rc = mac_reframe_expected(ds, st, bkd::MacExpected{table.d, nkeys, hs.d_seed[s], x.d_lid, x.d_eid, x.d_flag},
                                                trusted, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt, hs.d_lac[s],
                                                hs.d_frm[s], reinterpret_cast<int32_t*>(hs.d_res[s]));
            if (rc) return rc;
            BKD_HIP(hipMemcpyAsync(hs.h_frm[s], hs.d_frm[s], cnt * hl, hipMemcpyDeviceToHost, st));
            return BKD_OK;
        },
        // the host writes bytes 16..23 and 32..51 of each OK frame
        [&](HostStage& hs, int s, uint64_t i0, uint64_t cnt) -> int {
            bkd::host::mac_apply_reframe((uint8_t* const*)h_frames + i0, cnt, hs.h_frm[s],
                                         reinterpret_cast<const int32_t*>(hs.h_res[s]));
            return BKD_OK;
        },
        &HostStage::init_requests, &HostStage::init_reframe, &HostStage::init_package);
}

int bkd_digest_package_batch_ledgers_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_key_of,
                                              const int64_t* h_ledger_ids, const int64_t* h_entry_ids,
                                              const int64_t* h_lacs, const int64_t* h_length_fields,
                                              const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                              void* h_frames, uint64_t frame_stride) {
    if (n == 0) return BKD_OK;
    if (!h_key_of || !h_ledger_ids || !h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths ||
        !h_frames)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !h_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    constexpr uint64_t hl = bkd::host::kMacFrameHead;
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    if (int rc = check_key_index("entry", h_key_of, n, nkeys)) return rc;  // before any work: no frame is written
    if (int rc = check_host_entries("entry", h_payloads, h_lengths, n)) return rc;
    const int route = mac_host_route(h_lengths, n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::mac_package_frames_ledgers(h_key_states, h_key_of, h_ledger_ids, h_entry_ids, h_lacs,
                                              h_length_fields, (const uint8_t* const*)h_payloads, h_lengths, n,
                                              (uint8_t*)h_frames, frame_stride);
        return BKD_OK;
    }
    return mac_package_host_staged(h_key_states, nkeys, h_key_of, h_ledger_ids, h_entry_ids, h_lacs, h_length_fields,
                                   entry_buffers(h_payloads, h_lengths), h_lengths, n,
                                   host_frames(hl, hl, h_frames, frame_stride, nullptr));
}

int bkd_digest_package_batch_segments_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                          int64_t ledger_id, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                          const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                          uint64_t payload_size, const uint64_t* d_seg_offsets,
                                          const uint32_t* d_seg_lengths, uint64_t nseg, const uint64_t* d_seg_first,
                                          uint64_t n, void* d_frames, uint64_t frame_stride, void* stream) {
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_seg_first || !d_frames ||
        (nseg && (!d_seg_offsets || !d_seg_lengths)))
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !d_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (nseg && !d_payload && payload_size) return fail(BKD_ERR_INVALID_ARG, "null payload");
    if (int rc = check_frame_stride(bkd::host::kMacFrameHead, frame_stride, false)) return rc;
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_package_segments(*call.ds, call.st, bkd::MacLedgersOr{d_key_states, nkeys, d_key_of, d_ledger_ids, ledger_id},
                                d_entry_ids, d_lacs, d_length_fields, d_payload, payload_size, d_seg_offsets,
                                d_seg_lengths, nseg, d_seg_first, n, d_frames, frame_stride);
}

int bkd_digest_package_batch_v2_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                    int64_t ledger_id, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                    const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                    uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                                    uint64_t n, const uint8_t* d_master_keys, uint64_t key_stride, uint32_t flags,
                                    uint32_t small_threshold, void* d_requests, uint64_t requests_size,
                                    const uint64_t* d_request_offsets, void* stream) {
    if (int rc = check_v2_args(key_stride, flags)) return rc;
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_offsets || !d_lengths || !d_master_keys || !d_requests ||
        !d_request_offsets)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !d_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (n > kMacMaxBatch) return fail(BKD_ERR_INVALID_ARG, "batch too large");
    Call call(stream);
    if (call.rc) return call.rc;
    return mac_package_v2(*call.ds, call.st, bkd::MacLedgersOr{d_key_states, nkeys, d_key_of, d_ledger_ids, ledger_id},
                          d_entry_ids, d_lacs, d_length_fields, d_payload, payload_size, d_offsets, d_lengths, n,
                          d_master_keys, key_stride, bkd::host::v2_packet_header(flags), small_threshold, d_requests,
                          requests_size, d_request_offsets);
}

namespace {

// The key rows and ledger ids of a host-resident composite or V2 MAC call as the arrays the many-ledger
// device sequence takes: the caller's, or row 0 / ledger_id for every entry where it passed none. The key
// indices are checked against the table here, before any work.
struct MacHostIds {
    std::vector<uint32_t> rows;
    std::vector<int64_t> lids;
    const uint32_t* key_of;
    const int64_t* ledger_ids;
    int rc = BKD_OK;
    MacHostIds(uint64_t nkeys, const uint32_t* h_key_of, int64_t ledger_id, const int64_t* h_ledger_ids, uint64_t n)
        : key_of(h_key_of), ledger_ids(h_ledger_ids) {
        if (h_key_of) rc = check_key_index("entry", h_key_of, n, nkeys);
        else if (nkeys == 0) rc = fail(BKD_ERR_INVALID_ARG, "an empty key table");
    }
    // the GPU route's arrays, made only there
    void materialise(int64_t ledger_id, uint64_t n) {
        if (!key_of) {
            rows.assign(n, 0u);
            key_of = rows.data();
        }
        if (!ledger_ids) {
            lids.assign(n, ledger_id);
            ledger_ids = lids.data();
        }
    }
};

}  // namespace

int bkd_digest_package_batch_segments_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_key_of,
                                               int64_t ledger_id, const int64_t* h_ledger_ids,
                                               const int64_t* h_entry_ids, const int64_t* h_lacs,
                                               const int64_t* h_length_fields, const void* const* h_seg_ptrs,
                                               const uint32_t* h_seg_lengths, uint64_t nseg, const uint64_t* h_seg_first,
                                               uint64_t n, void* h_frames, uint64_t frame_stride) {
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_frames) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !h_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    constexpr uint64_t hl = bkd::host::kMacFrameHead;
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    MacHostIds ids(nkeys, h_key_of, ledger_id, h_ledger_ids, n);  // before any work, so no frame is written
    if (ids.rc) return ids.rc;
    if (int rc = check_host_segments(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n)) return rc;
    const HostSegments segs(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n);
    const int route = mac_host_route(segs.entry_len.data(), n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::mac_package_frames_segments(h_key_states, h_key_of, ledger_id, h_ledger_ids, h_entry_ids, h_lacs,
                                               h_length_fields, (const uint8_t* const*)h_seg_ptrs, h_seg_lengths,
                                               h_seg_first, segs.entry_len.data(), n, (uint8_t*)h_frames, frame_stride);
        return BKD_OK;
    }
    // each entry's segments end to end in the staging buffer (HostSegments: an entry is never split between
    // two staged segments), then bkd_digest_package_batch_ledgers_mac's device sequence
    ids.materialise(ledger_id, n);
    return mac_package_host_staged(h_key_states, nkeys, ids.key_of, ids.ledger_ids, h_entry_ids, h_lacs, h_length_fields,
                                   segs, segs.entry_len.data(), n, host_frames(hl, hl, h_frames, frame_stride, nullptr));
}

int bkd_digest_package_batch_v2_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_key_of,
                                         int64_t ledger_id, const int64_t* h_ledger_ids, const int64_t* h_entry_ids,
                                         const int64_t* h_lacs, const int64_t* h_length_fields,
                                         const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                         const uint8_t* h_master_keys, uint64_t key_stride, uint32_t flags,
                                         uint32_t small_threshold, void* const* h_requests) {
    if (int rc = check_v2_args(key_stride, flags)) return rc;
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_payloads || !h_lengths || !h_master_keys || !h_requests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nkeys && !h_key_states) return fail(BKD_ERR_INVALID_ARG, "null key table");
    if (int rc = check_v2_entries(h_payloads, h_lengths, h_requests, n)) return rc;
    MacHostIds ids(nkeys, h_key_of, ledger_id, h_ledger_ids, n);  // before any work, so no request is written
    if (ids.rc) return ids.rc;
    const int route = mac_host_route(h_lengths, n);
    if (route < 0) return route;
    const bkd::host::MacV2Head head{h_master_keys, key_stride, bkd::host::v2_packet_header(flags), small_threshold};
    const uint8_t* const* payloads = (const uint8_t* const*)h_payloads;
    uint8_t* const* requests = (uint8_t* const*)h_requests;
    if (route == 1) {
        bkd::host::mac_package_requests_v2(h_key_states, h_key_of, ledger_id, h_ledger_ids, h_entry_ids, h_lacs,
                                           h_length_fields, payloads, h_lengths, n, head, requests);
        return BKD_OK;
    }
    // GPU: staged and packaged into 52-byte frames as bkd_digest_package_batch_ledgers_mac_host; each finished
    // segment's frames go into the requests behind the prefix the host writes, the small payloads from their
    // sources
    ids.materialise(ledger_id, n);
    return mac_package_host_staged(h_key_states, nkeys, ids.key_of, ids.ledger_ids, h_entry_ids, h_lacs, h_length_fields,
                                   entry_buffers(h_payloads, h_lengths), h_lengths, n,
                                   [&](const uint8_t* frm, const uint32_t*, uint64_t i0, uint64_t cnt) {
                                       bkd::host::mac_finish_requests_v2(frm, payloads + i0, h_lengths + i0, cnt, head, i0,
                                                                         requests + i0);
                                   });
}

int bkd_host_segments_length_capped(const uint32_t* h_seg_lengths, uint64_t nseg, uint64_t cap, uint64_t* bytes) {
    const bkd::SegLength r = bkd::segments_length_capped(h_seg_lengths, 0, nseg, cap);
    if (bytes) *bytes = r.bytes;
    return r.over ? 1 : 0;
}

int bkd_entrylog_verify(int algo, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                        const uint32_t* d_lengths, uint64_t n, int32_t* d_status, uint64_t* d_first_bad,
                        void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (!d_first_bad) return fail(BKD_ERR_INVALID_ARG, "null first_bad");
    if (n && (!d_offsets || !d_lengths || !d_status)) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (n && !d_log) return fail(BKD_ERR_INVALID_ARG, "null log buffer");
    Call call(stream);
    if (call.rc) return call.rc;
    return verify_framed(*call.ds, call.st, algo, 0, 0, 2, d_log, log_size, d_offsets, d_lengths, n, d_status, d_first_bad);
}

int bkd_entrylog_verify_ledgers(const void* d_log, uint64_t log_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                                uint64_t n, const int64_t* d_ledger_ids, const uint32_t* d_ledger_types,
                                const uint32_t* d_ledger_keys, uint64_t nledgers, const uint32_t* d_key_states,
                                uint64_t nkeys, uint32_t types, int32_t* d_status, uint64_t* d_first_bad, void* stream) {
    const ScrubArgs a{d_ledger_ids, d_ledger_types, d_ledger_keys, nledgers, d_key_states, nkeys, types};
    const int rc = scrub_args_check(d_log, d_offsets, d_lengths, n, a, d_status, d_first_bad);
    if (rc) return rc;
    Call call(stream);
    if (call.rc) return call.rc;
    return scrub_ledgers(*call.ds, call.st, d_log, log_size, d_offsets, d_lengths, n, a, d_status, d_first_bad);
}

int bkd_entrylog_verify_ledgers_host(const void* h_log, uint64_t log_size, const uint64_t* h_offsets,
                                     const uint32_t* h_lengths, uint64_t n, const int64_t* h_ledger_ids,
                                     const uint32_t* h_ledger_types, const uint32_t* h_ledger_keys, uint64_t nledgers,
                                     const uint32_t* h_key_states, uint64_t nkeys, uint32_t types, int32_t* h_status,
                                     uint64_t* h_first_bad) {
    const ScrubArgs a{h_ledger_ids, h_ledger_types, h_ledger_keys, nledgers, h_key_states, nkeys, types};
    const int rc = scrub_args_check(h_log, h_offsets, h_lengths, n, a, h_status, h_first_bad);
    if (rc) return rc;
    return scrub_host(h_log, log_size, h_offsets, h_lengths, n, a, h_status, h_first_bad, nullptr);
}

int bkd_entrylog_scrub_report(const void* d_log, uint64_t log_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                              uint64_t n, const int64_t* d_ledger_ids, const uint32_t* d_ledger_types,
                              const uint32_t* d_ledger_keys, uint64_t nledgers, const uint32_t* d_key_states,
                              uint64_t nkeys, uint32_t types, int32_t* d_status, uint64_t* d_report, uint32_t* d_bad,
                              uint64_t bad_capacity, uint64_t* d_nbad, void* stream) {
    const ScrubArgs a{d_ledger_ids, d_ledger_types, d_ledger_keys, nledgers, d_key_states, nkeys, types};
    int rc = report_args_check(d_report, d_bad, bad_capacity, d_nbad);
    if (rc) return rc;
    rc = scrub_args_check(d_log, d_offsets, d_lengths, n, a, d_report, d_nbad);  // d_status may be null
    if (rc) return rc;
    Call call(stream);
    if (call.rc) return call.rc;
    return scrub_report(*call.ds, call.st, d_log, log_size, d_offsets, d_lengths, n, a, d_status, d_report, d_bad,
                        bad_capacity, d_nbad);
}

int bkd_entrylog_scrub_report_host(const void* h_log, uint64_t log_size, const uint64_t* h_offsets,
                                   const uint32_t* h_lengths, uint64_t n, const int64_t* h_ledger_ids,
                                   const uint32_t* h_ledger_types, const uint32_t* h_ledger_keys, uint64_t nledgers,
                                   const uint32_t* h_key_states, uint64_t nkeys, uint32_t types, int32_t* h_status,
                                   uint64_t* h_report, uint32_t* h_bad, uint64_t bad_capacity, uint64_t* h_nbad) {
    const ScrubArgs a{h_ledger_ids, h_ledger_types, h_ledger_keys, nledgers, h_key_states, nkeys, types};
    int rc = report_args_check(h_report, h_bad, bad_capacity, h_nbad);
    if (rc) return rc;
    rc = scrub_args_check(h_log, h_offsets, h_lengths, n, a, h_report, h_nbad);  // h_status may be null
    if (rc) return rc;
    const HostReport rep{h_report, h_bad, bad_capacity, h_nbad};
    return scrub_host(h_log, log_size, h_offsets, h_lengths, n, a, h_status, nullptr, &rep);
}

int bkd_entrylog_ledgers_map(const void* h_log, uint64_t log_size, int64_t* h_ledger_ids, int64_t* h_sizes,
                             uint64_t capacity, uint64_t* h_count, int32_t* h_version, int64_t* h_map_offset,
                             int32_t* h_ledgers_count, int32_t* h_state) {
    if (!h_count || !h_state || (log_size && !h_log) || (capacity && (!h_ledger_ids || !h_sizes)))
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    const bkd::host::LedgersMap m =
        bkd::host::read_ledgers_map((const uint8_t*)h_log, log_size, h_ledger_ids, h_sizes, capacity);
    *h_count = m.count;
    *h_state = m.state;
    if (h_version) *h_version = m.version;
    if (h_map_offset) *h_map_offset = m.map_offset;
    if (h_ledgers_count) *h_ledgers_count = m.ledgers_count;
    if (m.state == BKD_LEDGERS_MAP_MALFORMED) (void)fail(BKD_OK, std::string("ledgers map: ") + m.why);
    if (m.over) return fail(BKD_ERR_BOUNDS, "ledgers map capacity exceeded");
    return BKD_OK;
}

int bkd_set_scrub_order(int order) {
    if (order != 0 && order != 1) return fail(BKD_ERR_INVALID_ARG, "scrub order is 0 (binned) or 1 (index order)");
    g_scrub_order.store(order);
    return BKD_OK;
}

int bkd_get_scrub_order(void) { return g_scrub_order.load(); }

// automatic: the GPU only where the log has HMAC work for it; CRC stays on the host (§5)
int bkd_get_scrub_host_route(const uint32_t* h_ledger_types, uint64_t nledgers, uint32_t types) {
    const int r = g_host_route.load(std::memory_order_relaxed);
    if (r != 0) return r;
    bool mac = false;
    if ((types >> bkd::scrub::kHmac) & 1u)
        for (uint64_t k = 0; h_ledger_types && k < nledgers && !mac; ++k) mac = h_ledger_types[k] == bkd::scrub::kHmac;
    return (mac && visible_devices() > 0) ? 2 : 1;
}

int bkd_entrylog_scrub_lanes(const void* d_log, uint64_t log_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                             uint64_t n, const int64_t* d_ledger_ids, const uint32_t* d_ledger_types,
                             const uint32_t* d_ledger_keys, uint64_t nledgers, const uint32_t* d_key_states,
                             uint64_t nkeys, uint32_t types, uint32_t* d_lanes, uint32_t* d_nlanes, void* stream) {
    if (!d_nlanes) return fail(BKD_ERR_INVALID_ARG, "null nlanes");
    if (n > 0 && !d_lanes) return fail(BKD_ERR_INVALID_ARG, "null lanes");
    const ScrubArgs a{d_ledger_ids, d_ledger_types, d_ledger_keys, nledgers, d_key_states, nkeys, types};
    const int rc = scrub_args_check(d_log, d_offsets, d_lengths, n, a, d_lanes, d_nlanes);
    if (rc) return rc;
    if (!((types >> bkd::scrub::kHmac) & 1u))
        return fail(BKD_ERR_INVALID_ARG, "the lanes are the HMAC frames': types needs the HMAC bit");
    Call call(stream);
    if (call.rc) return call.rc;
    return scrub_lanes(*call.ds, call.st, d_log, log_size, d_offsets, d_lengths, n, a, d_lanes, d_nlanes);
}

uint32_t bkd_host_scrub_bin(uint32_t frame_len) { return bkd::scrub::bin(frame_len); }

int64_t bkd_host_scrub_lookup(const int64_t* ids, uint64_t nledgers, int64_t id) {
    if (nledgers > 0 && !ids) return -1;
    return bkd::scrub::lookup(ids, nledgers, id);
}

int bkd_crc_batch_segments(int algo, const void* d_base, uint64_t base_size, const uint64_t* d_seg_offsets,
                           const uint32_t* d_seg_lengths, uint64_t nseg, const uint64_t* d_seg_first, uint64_t n,
                           const uint32_t* d_seeds, uint32_t seed_all, uint32_t* d_out, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!d_seg_first || !d_out || (nseg && (!d_seg_offsets || !d_seg_lengths)))
        return fail(BKD_ERR_INVALID_ARG, "null index/out");
    if (nseg && !d_base && base_size) return fail(BKD_ERR_INVALID_ARG, "null base");
    Call call(stream);
    if (call.rc) return call.rc;
    StreamScratch& sc = scratch_for(*call.ds, call.st);
    std::lock_guard<std::recursive_mutex> lk(sc.mu);  // held across the nested plan (slot 0)
    uint8_t* seg = nullptr;
    hipError_t e = sc.get(2, (size_t)std::max<uint64_t>(nseg, 1) * 4, call.st, &seg);
    if (e != hipSuccess) return fail(BKD_ERR_NOMEM, std::string("segment scratch: ") + hipGetErrorString(e));
    uint32_t* segcrc = reinterpret_cast<uint32_t*>(seg);
    // every segment's raw register reg(0, segment), as ~resume(~0, segment)
    if (nseg) {
        const int rc = indexed_batch(*call.ds, algo, (const uint8_t*)d_base, base_size, d_seg_offsets, d_seg_lengths,
                                     nseg, nullptr, 0xFFFFFFFFu, segcrc, call.st);
        if (rc) return rc;
    }
    bkd::XPow8 pw;
    for (int b = 0; b < 32; ++b) pw.p[b] = bkd::gf2::xpow(algo, 8ull << b);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(bkd::segments_combine_kernel, dim3(blocks), dim3(256), 0, call.st, d_seg_lengths, segcrc,
                       d_seg_first, n, nseg, d_seeds, seed_all, pw, bkd::gf2::poly(algo), d_out);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

int bkd_digest_package_batch_segments(int algo, int64_t ledger_id, const int64_t* d_ledger_ids,
                                      const int64_t* d_entry_ids, const int64_t* d_lacs, const int64_t* d_length_fields,
                                      const void* d_payload, uint64_t payload_size, const uint64_t* d_seg_offsets,
                                      const uint32_t* d_seg_lengths, uint64_t nseg, const uint64_t* d_seg_first, uint64_t n,
                                      void* d_frames, uint64_t frame_stride, uint32_t* d_digests, void* stream) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!d_entry_ids || !d_lacs || !d_length_fields || !d_seg_first || !d_frames || !d_digests ||
        (nseg && (!d_seg_offsets || !d_seg_lengths)))
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (nseg && !d_payload && payload_size) return fail(BKD_ERR_INVALID_ARG, "null payload");
    if (int rc = check_frame_stride(32u + mac_len(algo), frame_stride, false)) return rc;
    Call call(stream);
    if (call.rc) return call.rc;
    return package_segments(*call.ds, call.st, algo, ledger_id, d_ledger_ids, d_entry_ids, d_lacs, d_length_fields,
                            d_payload, payload_size, d_seg_offsets, d_seg_lengths, nseg, d_seg_first, n, d_frames,
                            frame_stride, d_digests);
}

int bkd_digest_package_batch_segments_host(int algo, int64_t ledger_id, const int64_t* h_ledger_ids,
                                           const int64_t* h_entry_ids, const int64_t* h_lacs,
                                           const int64_t* h_length_fields, const void* const* h_seg_ptrs,
                                           const uint32_t* h_seg_lengths, uint64_t nseg, const uint64_t* h_seg_first,
                                           uint64_t n, void* h_frames, uint64_t frame_stride, uint32_t* h_digests) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    const uint64_t hl = 32u + mac_len(algo);
    if (n == 0) return BKD_OK;
    if (!h_entry_ids || !h_lacs || !h_length_fields || !h_frames || !h_digests)
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_frame_stride(hl, frame_stride, true)) return rc;
    if (int rc = check_host_segments(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n)) return rc;
    const HostSegments segs(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n);
    const int route = framed_host_route(segs.entry_len.data(), n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::package_frames_segments(algo, ledger_id, h_ledger_ids, h_entry_ids, h_lacs, h_length_fields,
                                           (const uint8_t* const*)h_seg_ptrs, h_seg_lengths, h_seg_first,
                                           segs.entry_len.data(), n, (uint8_t*)h_frames, frame_stride, h_digests);
        return BKD_OK;
    }
    return package_host_staged(h_ledger_ids, h_entry_ids, h_lacs, h_length_fields, segs, segs.entry_len.data(), n,
                               crc_package(algo, ledger_id), frame_stride, true,
                               host_frames(hl, frame_stride, h_frames, frame_stride, h_digests));
}

int bkd_crc_batch_segments_host(int algo, const void* const* h_seg_ptrs, const uint32_t* h_seg_lengths, uint64_t nseg,
                                const uint64_t* h_seg_first, uint64_t n, const uint32_t* h_seeds, uint32_t seed_all,
                                uint32_t* h_out) {
    if (!valid_algo(algo)) return fail(BKD_ERR_INVALID_ARG, "unknown algorithm");
    if (n == 0) return BKD_OK;
    if (!h_out) return fail(BKD_ERR_INVALID_ARG, "null out");
    int rc = check_host_segments(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n);
    if (rc) return rc;
    const HostSegments segs(h_seg_ptrs, h_seg_lengths, nseg, h_seg_first, n);
    const int route = framed_host_route(segs.entry_len.data(), n);
    if (route < 0) return route;
    if (route == 1) {
        bkd::host::crc_segments(algo, (const uint8_t* const*)h_seg_ptrs, h_seg_lengths, h_seg_first,
                                segs.entry_len.data(), n, h_seeds, seed_all, h_out);
        return BKD_OK;
    }
    StagedCall call;
    if (call.rc) return call.rc;
    HostStage& hs = **call.lease;
    auto seg = [&](int s, uint64_t i0, uint64_t cnt, uint64_t bytes) -> int {
        const hipStream_t st = hs.st[s];
        int r = segs(hs, s, i0, cnt, bytes);
        if (r) return r;
        if (h_seeds) {
            memcpy(hs.h_seed[s], h_seeds + i0, cnt * 4);
            BKD_HIP(hipMemcpyAsync(hs.d_seed[s], hs.h_seed[s], cnt * 4, hipMemcpyHostToDevice, st));
        }
        r = indexed_batch(*call.ds, algo, hs.d_buf[s], bytes, hs.d_off[s], hs.d_len[s], cnt,
                          h_seeds ? hs.d_seed[s] : nullptr, seed_all, hs.d_res[s], st);
        if (r) return r;
        BKD_HIP(hipMemcpyAsync(hs.h_res[s], hs.d_res[s], cnt * 4, hipMemcpyDeviceToHost, st));
        return BKD_OK;
    };
    auto drain = [&](int s, uint64_t i0, uint64_t cnt) -> int {
        memcpy(h_out + i0, hs.h_res[s], cnt * 4);
        return BKD_OK;
    };
    return host_segments(hs, segs.entry_len.data(), n, HostStage::kSegEntries, seg, drain);
}

int bkd_host_segments_range(uint64_t first_i, uint64_t first_i1, uint64_t i, uint64_t n, uint64_t nseg,
                            uint64_t* k0, uint64_t* k1) {
    const bkd::SegRange r = bkd::segments_range(first_i, first_i1, i, n, nseg);
    if (k0) *k0 = r.k0;
    if (k1) *k1 = r.k1;
    return r.bad ? 1 : 0;
}

int bkd_host_segment_bytewise(uint64_t offset, uint32_t length, uint64_t payload_size) {
    return bkd::segment_joined_bytewise(offset, length, payload_size) ? 1 : 0;
}

int bkd_entrylog_index(const void* h_log, uint64_t log_size, uint64_t start, uint64_t* h_offsets,
                       uint32_t* h_lengths, int64_t* h_ledger_ids, uint64_t capacity, uint64_t* h_count,
                       uint64_t* h_end) {
    if (!h_count || (log_size && !h_log) || (capacity && (!h_offsets || !h_lengths)))
        return fail(BKD_ERR_INVALID_ARG, "null buffer");
    const uint8_t* p = (const uint8_t*)h_log;
    auto be32 = [&](uint64_t at) {
        return (int32_t)(((uint32_t)p[at] << 24) | ((uint32_t)p[at + 1] << 16) | ((uint32_t)p[at + 2] << 8) |
                         (uint32_t)p[at + 3]);
    };
    auto be64 = [&](uint64_t at) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v = (v << 8) | p[at + k];
        return (int64_t)v;
    };
    uint64_t pos = start, count = 0;
    int rc = BKD_OK;
    while (pos < log_size) {
        if (log_size - pos < 12) break;  // short read of [size, ledgerId]: the scan stops
        const int32_t entry_size = be32(pos);
        if (entry_size <= 0) {  // padding
            ++pos;
            continue;
        }
        const int64_t ledger_id = be64(pos + 4);
        pos += 4;
        if (ledger_id == -1) {  // INVALID_LID: ledgers-map record, not an entry
            pos += (uint64_t)entry_size;
            continue;
        }
        if ((uint64_t)entry_size > log_size - pos) break;  // short read of the entry: the scan stops
        if (count < capacity) {
            h_offsets[count] = pos;
            h_lengths[count] = (uint32_t)entry_size;
            if (h_ledger_ids) h_ledger_ids[count] = ledger_id;
        } else {
            rc = fail(BKD_ERR_BOUNDS, "entry-log index capacity exceeded");
            break;
        }
        ++count;
        pos += (uint64_t)entry_size;
    }
    *h_count = count;
    if (h_end) *h_end = pos;
    return rc;
}

int bkd_fill_splitmix64(void* d_dst, uint64_t nbytes, uint64_t seed, uint64_t first_word, void* stream) {
    if (nbytes == 0) return BKD_OK;
    if (!d_dst) return fail(BKD_ERR_INVALID_ARG, "null buffer");
    Call call(stream);
    if (call.rc) return call.rc;
    const uint64_t nw = std::max<uint64_t>(1, nbytes / 8);
    const unsigned blocks = (unsigned)std::min<uint64_t>((nw + 255) / 256, (uint64_t)call.ds->cus * 16);
    hipLaunchKernelGGL(bkd::fill_splitmix64_kernel, dim3(blocks), dim3(256), 0, call.st,
                       (uint8_t*)d_dst, nbytes, seed, first_word);
    BKD_HIP(hipGetLastError());
    return BKD_OK;
}

int64_t bkd_host_tables(int algo, int lanes, uint32_t* out, uint64_t out_words) {
    if (!valid_algo(algo) || lane_index(lanes) < 0) return fail(BKD_ERR_INVALID_ARG, "bad algo/lanes");
    const int64_t need = bkd::gf2::compact_words(lanes);
    if (!out || out_words < (uint64_t)need) return fail(BKD_ERR_INVALID_ARG, "output too small");
    return bkd::gf2::build_compact(algo, lanes, out);
}

uint32_t bkd_host_gf_mul(int algo, uint32_t a, uint32_t b) { return bkd::gf2::mul(algo, a, b); }

uint32_t bkd_host_xpow8n(int algo, uint64_t nbytes) { return bkd::gf2::xpow(algo, nbytes * 8); }

}  // extern "C"
