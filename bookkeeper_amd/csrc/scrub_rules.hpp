// The two rules of the mixed-ledger entry-log scrub (bkd_entrylog_verify_ledgers) that the device
// kernels (scrub_kernels.hpp) and the host route (host_scrub.cpp) share, the way mac_segments.hpp is
// shared: which row of the ledger table an entry belongs to, and which length bin an HMAC frame's lane
// runs in. Plain C++ over mac_sha1.hpp: no host or device calls.
#pragma once
#include <stdint.h>

#include "mac_sha1.hpp"

namespace bkd {
namespace scrub {

// Digest types of a ledger-table row (DataFormats.proto:45-50), in the order of BKD_DIGEST_*.
constexpr uint32_t kCrc32c = 0, kCrc32 = 1, kHmac = 2, kDummy = 3;
constexpr uint32_t kTypeMaskAll = 0xFu;

// The row of `id` in ids[0, nledgers) (strictly ascending as signed values), or -1. A lower-bound
// search whose probes stay inside [0, nledgers) whatever the array holds: an unsorted table may hide a
// listed ledger, it never sends a load outside the array.
BKD_HD int64_t lookup(const int64_t* ids, uint64_t nledgers, int64_t id) {
    uint64_t lo = 0, hi = nledgers;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nledgers && ids[lo] == id) ? (int64_t)lo : -1;
}

// SHA-1 compressions of the inner hash of an HMAC frame of frame_len >= 52 bytes: the 32-byte header
// and the payload, padded.
BKD_HD uint32_t blocks(uint32_t frame_len) { return (uint32_t)(sha1::padded_bytes((uint64_t)frame_len - 20u) >> 6); }

// The length bin of B >= 1 compressions: four bins per power of two, 4 e + the two bits below B's
// leading bit e (a bit that B does not have counts as 0). 1 -> 0, 2 -> 4, 3 -> 6, 4 -> 8, 5 -> 9,
// 7 -> 11, 8 and 9 -> 12; from B = 4 on the longest entry of a bin is under 1.25 times its shortest.
BKD_HD uint32_t bin_of_blocks(uint32_t b) {
    const uint32_t e = 31u - (uint32_t)__builtin_clz(b);
    const uint32_t two = e >= 2u ? (b >> (e - 2u)) & 3u : (b << (2u - e)) & 3u;
    return 4u * e + two;
}

// BKD_MAC_MAX_ENTRY (16 MiB) has 2^18 compressions: bin 72 is the last.
constexpr uint32_t kBins = 73;

// The bin of a frame; frames under 52 bytes are never hashed and have none (0 here).
BKD_HD uint32_t bin(uint32_t frame_len) { return frame_len < 52u ? 0u : bin_of_blocks(blocks(frame_len)); }

}  // namespace scrub
}  // namespace bkd
