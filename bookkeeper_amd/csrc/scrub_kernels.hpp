// Kernels of the mixed-ledger entry-log scrub (bkd_entrylog_verify_ledgers): a whole entry-log index
// across ledgers and digest types in one launch sequence, no host synchronisation.
//
//   scrub_classify_kernel   one lane per entry: range check, the entry's ledger id (its first 8 bytes),
//                           a binary search of the ledger table (scrub_rules.hpp), type and key row.
//                           Entries that need no digest (unreadable, short, unlisted, masked, DUMMY, bad
//                           key row, over the cap) get their final status; CRC entries are marked for
//                           their class and copied into its offset / length arrays (everyone else is
//                           (0, 0) there); HMAC frames get a length bin and are counted: an LDS histogram
//                           per block, then one global add per bin the block saw.
//   scrub_scan_kernel       73 counts -> where each bin starts, longest bin first; the HMAC count.
//   scrub_scatter_kernel    each HMAC entry's index into a slot of its bin (ranks from an LDS histogram,
//                           one global add per bin and block). Order 1: the identity permutation.
//   mac_scrub_kernel        lane s hashes entry perm[s] as mac_verify_kernel does, without id checks.
//   scrub_merge_kernel      picks each CRC entry's status from its class's array and lowers *first_bad.
//
// Why bins. One lane hashes one entry, so a wave runs as long as its longest entry (mac_kernels.hpp). In
// arrival order a Zipf-length log keeps ~12 % of its MAC lanes busy; with the lanes of a wave taken from
// one bin (lengths within 1.25x from four blocks on) ~92 %. Bins run longest first, so the
// longest entries' lanes are not the launch's tail.
//
// Loads: every load of log bytes is an aligned dword that holds a byte of the entry it is loaded for
// (MacStream); the table search probes only rows [0, nledgers); a key row is loaded only when it is
// < nkeys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bkdigest.h"
#include "mac_kernels.hpp"
#include "scrub_rules.hpp"

namespace bkd {

constexpr int kScrubBlock = 256;

// An entry's tag word: bits 0..1 its class, bits 8..15 its bin (HMAC only).
constexpr uint32_t kScrubFinal = 0u;   // the status is in d_status already
constexpr uint32_t kScrubCrc32c = 1u;  // the status comes from the CRC32C class's array
constexpr uint32_t kScrubCrc32 = 2u;   // ... from the CRC32 class's
constexpr uint32_t kScrubHmac = 3u;    // mac_scrub_kernel writes it

// The ledger table and what of it this call verifies.
struct ScrubTable {
    const int64_t* __restrict__ ids;
    const uint32_t* __restrict__ types;
    const uint32_t* __restrict__ keys;  // may be null when the HMAC bit of `mask` is clear
    uint64_t nledgers;
    uint64_t nkeys;
    uint32_t mask;
};

// One CRC class's arrays in the stream's scratch (null when the class is not in the mask).
struct ScrubClass {
    uint64_t* __restrict__ off;
    uint32_t* __restrict__ len;
};

__global__ void __launch_bounds__(kScrubBlock) scrub_classify_kernel(
    const uint8_t* __restrict__ log, uint64_t size, const uint64_t* __restrict__ offsets,
    const uint32_t* __restrict__ lengths, uint64_t n, ScrubTable tab, ScrubClass c32c, ScrubClass c32,
    uint32_t* __restrict__ tag, uint32_t* __restrict__ krow, uint32_t* __restrict__ counts,
    int32_t* __restrict__ status, uint32_t* __restrict__ err) {
    __shared__ uint32_t hist[scrub::kBins];
    for (uint32_t b = threadIdx.x; b < scrub::kBins; b += kScrubBlock) hist[b] = 0u;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kScrubBlock + threadIdx.x;
    if (i < n) {
        const uint64_t o = offsets[i];
        const uint32_t l = lengths[i];
        uint32_t t = kScrubFinal;
        int32_t st = BKD_VERIFY_NOT_CHECKED;
        if (!(o <= size && (uint64_t)l <= size - o)) {
            st = 1;
            atomicOr(err, 1u);
        } else if (l < 8u) {
            st = 1;
        } else {
            const MacStream in(log + o, 8u);  // the ledger id: dwords that hold one of its 8 bytes
            uint32_t d[3];
            in.load<3>(0u, d);
            const int64_t lid = (int64_t)(((uint64_t)in.word(d[0], d[1]) << 32) | in.word(d[1], d[2]));
            const int64_t r = scrub::lookup(tab.ids, tab.nledgers, lid);
            const uint32_t type = r >= 0 ? tab.types[r] : 4u;
            if (type <= 3u && ((tab.mask >> type) & 1u)) {
                if (type == scrub::kDummy) {
                    st = l >= 32u ? 0 : 1;  // no digest bytes: only the 32-byte header is required
                } else if (type == scrub::kHmac) {
                    const uint32_t k = tab.keys[r];
                    if (k >= tab.nkeys || l > BKD_MAC_MAX_ENTRY) {  // unreadable: never hashed
                        st = 1;
                        atomicOr(err, 1u);
                    } else if (l < 52u) {
                        st = 1;
                    } else {
                        const uint32_t b = scrub::bin(l);
                        t = kScrubHmac | (b << 8);
                        krow[i] = k;
                        atomicAdd(&hist[b], 1u);
                    }
                } else {
                    t = type == scrub::kCrc32c ? kScrubCrc32c : kScrubCrc32;
                }
            }
        }
        tag[i] = t;
        if (t == kScrubFinal) status[i] = st;
        if (c32c.off) {
            c32c.off[i] = t == kScrubCrc32c ? o : 0u;
            c32c.len[i] = t == kScrubCrc32c ? l : 0u;
        }
        if (c32.off) {
            c32.off[i] = t == kScrubCrc32 ? o : 0u;
            c32.len[i] = t == kScrubCrc32 ? l : 0u;
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < scrub::kBins; b += kScrubBlock)
        if (hist[b]) atomicAdd(counts + b, hist[b]);
}

// counts[b] -> the first slot of bin b, bins descending; *nmac = the lanes mac_scrub_kernel runs (order 1:
// all n, each looking at its own entry's tag); *first_bad = n for the merge to lower.
__global__ void scrub_scan_kernel(uint32_t* __restrict__ counts, uint32_t* __restrict__ nmac, uint64_t n, int order,
                                  uint64_t* __restrict__ first_bad) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t run = 0u;
    for (int b = (int)scrub::kBins - 1; b >= 0; --b) {
        const uint32_t c = counts[b];
        counts[b] = run;
        run += c;
    }
    *nmac = order == 1 ? (uint32_t)n : run;
    *first_bad = n;
}

__global__ void __launch_bounds__(kScrubBlock) scrub_scatter_kernel(const uint32_t* __restrict__ tag, uint64_t n,
                                                                    int order, uint32_t* __restrict__ cursor,
                                                                    uint32_t* __restrict__ perm) {
    const uint64_t i = (uint64_t)blockIdx.x * kScrubBlock + threadIdx.x;
    if (order == 1) {  // index order: the same kernels over the identity permutation
        if (i < n) perm[i] = (uint32_t)i;
        return;
    }
    __shared__ uint32_t hist[scrub::kBins], first[scrub::kBins];
    for (uint32_t b = threadIdx.x; b < scrub::kBins; b += kScrubBlock) hist[b] = 0u;
    __syncthreads();
    const uint32_t t = i < n ? tag[i] : kScrubFinal;
    const bool mac = (t & 3u) == kScrubHmac;
    const uint32_t b = mac ? (t >> 8) & 0xFFu : 0u;  // < kBins: scrub_classify_kernel wrote it
    uint32_t rank = 0u;
    if (mac) rank = atomicAdd(&hist[b], 1u);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < scrub::kBins; k += kScrubBlock)
        if (hist[k]) first[k] = atomicAdd(cursor + k, hist[k]);
    __syncthreads();
    if (mac) perm[first[b] + rank] = (uint32_t)i;  // < the HMAC count <= n
}

// Lane s verifies HMAC frame perm[s]: mac_verify_kernel's hash and compare, the key from row krow[i] of
// the table, no id checks. The grid is sized by n (the host does not know the HMAC count); lanes at or
// past *nmac return at once.
__global__ void __launch_bounds__(kMacBlock) mac_scrub_kernel(
    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ nmac, const uint32_t* __restrict__ tag,
    const uint32_t* __restrict__ krow, const uint32_t* __restrict__ key_states, uint64_t nkeys,
    const uint8_t* __restrict__ log, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lengths,
    uint64_t n, int32_t* __restrict__ status) {
    const uint64_t s = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (s >= n || s >= (uint64_t)*nmac) return;
    const uint32_t i = perm[s];
    if ((tag[i] & 3u) != kScrubHmac) return;  // index order: an entry of another class
    // in range, 52 <= l <= BKD_MAC_MAX_ENTRY and the row inside the table: scrub_classify_kernel checked
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    const MacKeyRow key{key_states, nkeys, krow[i]};
    const MacStream in(log + o, l);
    uint32_t d[14], hw[13];  // bytes [0, 52): dword 13 is read only where the frame reaches into it
    in.load<14>(0u, d);
#pragma unroll
    for (int t = 0; t < 13; ++t) hw[t] = in.word(d[t], d[t + 1]);
    uint32_t pre[8], mac[5];
#pragma unroll
    for (int t = 0; t < 8; ++t) pre[t] = hw[t];
    mac_entry<true>(key, pre, in, 13u, l - 52u, mac);
    uint32_t diff = 0u;
#pragma unroll
    for (int k = 0; k < 5; ++k) diff |= mac[k] ^ hw[8 + k];
    status[i] = diff ? 2 : 0;
}

// status[i] of a CRC entry from its class's array; the lowest index with a status above 0 lowers
// *first_bad, one atomic per wave that holds one (lanes of a wave are consecutive indices).
__global__ void __launch_bounds__(kScrubBlock) scrub_merge_kernel(const uint32_t* __restrict__ tag,
                                                                  const int32_t* __restrict__ st32c,
                                                                  const int32_t* __restrict__ st32, uint64_t n,
                                                                  int32_t* __restrict__ status,
                                                                  unsigned long long* __restrict__ first_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * kScrubBlock + threadIdx.x;
    int32_t st = 0;
    if (i < n) {
        const uint32_t c = tag[i] & 3u;
        if (c == kScrubCrc32c) status[i] = st = st32c[i];
        else if (c == kScrubCrc32) status[i] = st = st32[i];
        else st = status[i];
    }
    const unsigned long long bad = __ballot(st > 0);
    if (bad && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)bad) - 1)) atomicMin(first_bad, (unsigned long long)i);
}

}  // namespace bkd
