// Kernels of the scrub report (bkd_entrylog_scrub_report): after bkd_entrylog_verify_ledgers's own sequence
// (scrub_kernels.hpp, unchanged) has left every entry's status, the rows of the per-ledger report and the
// ascending list of bad entries, all in stream order, no host synchronisation.
//
//   scrub_report_init_kernel     (nledgers + 1) x 8 words to their initial values (scrub_report_rules.hpp).
//   scrub_report_kernel          one lane per entry: the status, the row (the ledger id looked up again) and
//                                the entry id. The lanes of a wave that share a row are found by a loop over
//                                the wave's distinct rows (ballot, the first live lane's row broadcast); the
//                                counts are popcounts of ballots, the byte sum and the signed min / max of the
//                                bad entry ids cross-lane reductions taken only where a row has more than one
//                                lane. Then the lowest lane of every row issues that row's atomics, all rows
//                                of the wave in the same instructions; a block whose 16 waves all sit on one
//                                row folds them in LDS first and issues one set (a one-ledger log would
//                                otherwise send every wave's atomics to one address). Leaves each block's
//                                count of bad entries.
//   scrub_report_scan_kernel     one block: the block counts -> where each block's bad indices start; *nbad.
//   scrub_report_scatter_kernel  each block's bad indices in lane order (ballot, prefix popcount) from its
//                                start, clipped to the list's capacity.
//
// Loads: every load of log bytes is an aligned dword that holds a byte of the entry it is loaded for
// (MacStream over the entry's first 8 or 16 bytes); the table search probes only rows [0, nledgers). Stores:
// a report word of row <= nledgers, a block count of this block, bad[pos] with pos < capacity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mac_kernels.hpp"
#include "scrub_report_rules.hpp"

namespace bkd {

constexpr int kReportBlock = 1024;  // 16 waves: a one-row block folds them into one set of atomics
constexpr int kReportWaves = kReportBlock / 64;
constexpr int kReportScanBlock = 1024;

__global__ void __launch_bounds__(kReportBlock) scrub_report_init_kernel(uint64_t* __restrict__ report, uint64_t rows,
                                                                         uint64_t n) {
    const uint64_t w = (uint64_t)blockIdx.x * kReportBlock + threadIdx.x;
    if (w < rows * scrub::kReportWords) report[w] = scrub::initial_word((uint32_t)(w % scrub::kReportWords), n);
}

// Cross-lane reductions over the whole wave; every lane ends with the result.
__device__ __forceinline__ uint64_t report_wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}
__device__ __forceinline__ int64_t report_wave_min(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int64_t report_wave_max(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// A row's word as it travels from a wave to the report: what leaves it unchanged, how two partial values
// combine, and the one atomic that adds a partial value to the row in global memory.
constexpr uint64_t kReportNoLanes = ~0ull, kReportManyRows = ~0ull - 1u;  // no row: rows are <= nledgers < 2^61
__device__ __forceinline__ uint64_t report_neutral(uint32_t w) {
    return w == BKD_REPORT_MIN_BAD_ENTRY ? (uint64_t)INT64_MAX
           : w == BKD_REPORT_MAX_BAD_ENTRY ? (uint64_t)INT64_MIN
           : w == BKD_REPORT_FIRST_BAD_INDEX ? ~0ull
                                             : 0u;
}
__device__ __forceinline__ uint64_t report_combine(uint32_t w, uint64_t a, uint64_t b) {
    if (w == BKD_REPORT_MIN_BAD_ENTRY) return (int64_t)b < (int64_t)a ? b : a;
    if (w == BKD_REPORT_MAX_BAD_ENTRY) return (int64_t)b > (int64_t)a ? b : a;
    if (w == BKD_REPORT_FIRST_BAD_INDEX) return b < a ? b : a;
    return a + b;
}
__device__ __forceinline__ void report_issue(unsigned long long* row, uint32_t w, uint64_t v) {
    if (v == report_neutral(w)) return;
    if (w == BKD_REPORT_MIN_BAD_ENTRY) atomicMin((long long*)(row + w), (long long)v);
    else if (w == BKD_REPORT_MAX_BAD_ENTRY) atomicMax((long long*)(row + w), (long long)v);
    else if (w == BKD_REPORT_FIRST_BAD_INDEX) atomicMin(row + w, (unsigned long long)v);
    else atomicAdd(row + w, (unsigned long long)v);
}

__global__ void __launch_bounds__(kReportBlock) scrub_report_kernel(
    const uint8_t* __restrict__ log, uint64_t size, const uint64_t* __restrict__ offsets,
    const uint32_t* __restrict__ lengths, uint64_t n, const int64_t* __restrict__ ids, uint64_t nledgers,
    const int32_t* __restrict__ status, unsigned long long* __restrict__ report, uint32_t* __restrict__ block_bad) {
    __shared__ uint32_t wave_bad[kReportWaves];
    __shared__ uint64_t wave_row[kReportWaves];  // the wave's only row, kReportManyRows or kReportNoLanes
    __shared__ uint64_t part[kReportWaves][scrub::kReportWords];
    const uint64_t i = (uint64_t)blockIdx.x * kReportBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    uint64_t row = nledgers;
    int32_t st = 0;
    uint32_t l = 0;
    int64_t eid = 0;
    bool with_id = false;
    if (live) {
        const uint64_t o = offsets[i];
        l = lengths[i];
        st = status[i];
        const bool in_log = scrub::in_range(o, l, size);
        if (scrub::has_ledger_id(in_log, l)) {
            with_id = scrub::has_entry_id(in_log, l);
            const MacStream in(log + o, with_id ? 16u : 8u);  // dwords that hold a byte of [0, 8) or [0, 16)
            uint32_t d[5];
            in.load<5>(0u, d);
            const int64_t lid = (int64_t)(((uint64_t)in.word(d[0], d[1]) << 32) | in.word(d[1], d[2]));
            eid = (int64_t)(((uint64_t)in.word(d[2], d[3]) << 32) | in.word(d[3], d[4]));
            row = scrub::report_row(scrub::lookup(ids, nledgers, lid), nledgers);
        }
    }
    const uint32_t word = scrub::status_word(st);
    const uint64_t ok_m = __ballot(live && word == BKD_REPORT_OK);
    const uint64_t bad_m = __ballot(live && word == BKD_REPORT_BAD);
    const uint64_t id_m = __ballot(live && word == BKD_REPORT_BAD && with_id);  // bad entries whose id counts

    // peers = the lanes of this lane's row; at the row's lowest lane: bytes, lo and hi over the row
    uint64_t peers = 0;
    uint64_t bytes = scrub::report_bytes(l);
    int64_t lo = eid, hi = eid;
    uint64_t todo = __ballot(live);
    while (todo) {  // wave-uniform: one round per distinct row
        const int lead = __ffsll((long long)todo) - 1;
        const uint64_t lead_row = (uint64_t)__shfl((unsigned long long)row, lead);
        const bool mine = live && row == lead_row;
        const uint64_t grp = __ballot(mine);
        if (mine) peers = grp;
        if (grp & (grp - 1)) {  // more than one lane
            const uint64_t b = report_wave_sum(mine ? scrub::report_bytes(l) : 0u);
            if (lane == (uint32_t)lead) bytes = b;
            if (grp & id_m) {
                const bool counts = mine && word == BKD_REPORT_BAD && with_id;
                const int64_t a = report_wave_min(counts ? eid : INT64_MAX);
                const int64_t z = report_wave_max(counts ? eid : INT64_MIN);
                if (lane == (uint32_t)lead) {
                    lo = a;
                    hi = z;
                }
            }
        }
        todo &= ~grp;
    }
    // what the row's lowest lane holds for its row and wave, word by word (neutral where nothing counts)
    const bool leader = live && lane == (uint32_t)(__ffsll((long long)peers) - 1);
    const uint32_t all = (uint32_t)__popcll(peers), ok = (uint32_t)__popcll(peers & ok_m);
    const uint32_t bad = (uint32_t)__popcll(peers & bad_m);
    uint64_t v[scrub::kReportWords];
    v[BKD_REPORT_ENTRIES] = all;
    v[BKD_REPORT_BYTES] = bytes;
    v[BKD_REPORT_OK] = ok;
    v[BKD_REPORT_BAD] = bad;
    v[BKD_REPORT_NOT_CHECKED] = all - ok - bad;
    v[BKD_REPORT_MIN_BAD_ENTRY] = (peers & id_m) ? (uint64_t)lo : report_neutral(BKD_REPORT_MIN_BAD_ENTRY);
    v[BKD_REPORT_MAX_BAD_ENTRY] = (peers & id_m) ? (uint64_t)hi : report_neutral(BKD_REPORT_MAX_BAD_ENTRY);
    v[BKD_REPORT_FIRST_BAD_INDEX] = bad ? i - lane + (uint64_t)(__ffsll((long long)(peers & bad_m)) - 1)
                                        : report_neutral(BKD_REPORT_FIRST_BAD_INDEX);

    // A block whose waves all sit on one row (a log of one ledger, or a long run of one) combines them in
    // LDS and issues that row's atomics once; every other block issues them per row and wave.
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t live_m = __ballot(live);
    if (!live_m && lane == 0u) wave_row[wave] = kReportNoLanes;
    if (live_m && lane == (uint32_t)(__ffsll((long long)live_m) - 1)) {  // the wave's first live lane leads its row
        const bool one_row = peers == live_m;
        wave_row[wave] = one_row ? row : kReportManyRows;
        if (one_row) {
#pragma unroll
            for (uint32_t w = 0; w < scrub::kReportWords; ++w) part[wave][w] = v[w];
        }
    }
    if (lane == 0u) wave_bad[wave] = (uint32_t)__popcll(bad_m);
    __syncthreads();
    uint64_t block_row = kReportNoLanes;
    bool one_row = true;
    for (int w = 0; w < kReportWaves; ++w) {
        const uint64_t r = wave_row[w];
        if (r == kReportNoLanes) continue;
        if (r == kReportManyRows || (block_row != kReportNoLanes && r != block_row)) one_row = false;
        block_row = r;
    }
    if (one_row) {  // block-uniform; block_row <= nledgers: wave 0 has live lanes
        if (threadIdx.x < scrub::kReportWords) {
            uint64_t sum = report_neutral(threadIdx.x);
            for (int w = 0; w < kReportWaves; ++w)
                if (wave_row[w] != kReportNoLanes) sum = report_combine(threadIdx.x, sum, part[w][threadIdx.x]);
            report_issue(report + block_row * scrub::kReportWords, threadIdx.x, sum);
        }
    } else if (leader) {
        unsigned long long* r = report + row * scrub::kReportWords;  // row <= nledgers
#pragma unroll
        for (uint32_t w = 0; w < scrub::kReportWords; ++w) report_issue(r, w, v[w]);
    }
    if (threadIdx.x == 0u) {
        uint32_t s = 0u;
        for (int w = 0; w < kReportWaves; ++w) s += wave_bad[w];
        block_bad[blockIdx.x] = s;
    }
}

// counts[b] -> the number of bad entries in blocks [0, b); *nbad = all of them (at most n < 2^32). One
// block: thread t owns a run of consecutive counts.
__global__ void __launch_bounds__(kReportScanBlock) scrub_report_scan_kernel(uint32_t* __restrict__ counts,
                                                                             uint64_t nblocks,
                                                                             uint64_t* __restrict__ nbad) {
    __shared__ uint32_t part[kReportScanBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (nblocks + kReportScanBlock - 1) / kReportScanBlock;
    const uint64_t b0 = t * per < nblocks ? t * per : nblocks;
    const uint64_t b1 = b0 + per < nblocks ? b0 + per : nblocks;
    uint32_t mine = 0u;
    for (uint64_t b = b0; b < b1; ++b) mine += counts[b];
    part[t] = mine;
    __syncthreads();
    for (uint32_t off = 1u; off < (uint32_t)kReportScanBlock; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - mine;
    for (uint64_t b = b0; b < b1; ++b) {
        const uint32_t c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (t == (uint32_t)kReportScanBlock - 1u) *nbad = part[t];
}

__global__ void __launch_bounds__(kReportBlock) scrub_report_scatter_kernel(const int32_t* __restrict__ status,
                                                                            uint64_t n,
                                                                            const uint32_t* __restrict__ block_base,
                                                                            uint32_t* __restrict__ bad,
                                                                            uint64_t capacity) {
    __shared__ uint32_t wave_bad[kReportWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kReportBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool is_bad = i < n && scrub::status_word(status[i]) == BKD_REPORT_BAD;
    const uint64_t m = __ballot(is_bad);
    if (lane == 0u) wave_bad[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0u; w < wave; ++w) before += wave_bad[w];
    const uint64_t pos = (uint64_t)block_base[blockIdx.x] + before + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (is_bad && pos < capacity) bad[pos] = (uint32_t)i;
}

}  // namespace bkd
