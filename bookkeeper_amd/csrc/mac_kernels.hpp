// HMAC-SHA1 batch kernels for MAC ledgers (MacDigestManager, $BK/proto/checksum/MacDigestManager.java).
//
// SHA-1 is serial inside an entry and entries are independent, so one lane hashes one entry: no tables,
// no LDS, 32-bit VALU only. The 80 rounds are unrolled (mac_sha1.hpp), so the 16-word schedule window is
// statically indexed and stays in VGPRs; the kernels use no scratch.
//
// Loads. A lane reads its entry as naturally aligned dwords, each holding at least one byte of the
// entry (so no page is touched that the entry does not touch), and realigns in registers: one
// v_perm_b32 per message word funnels the two neighbouring dwords by the entry's byte alignment and
// swaps to big-endian at once. The 16 dwords of block k + 1 are issued before block k is compressed.
// The last partial block and the padding are built in registers (sha1::padded_word): bytes of the edge
// dwords that lie outside the entry never reach the hash.
//
// Ragged batches: lanes whose entry is finished idle until the wave's longest entry ends (the entry-log
// scrub bins its lanes by length instead, scrub_kernels.hpp).
//
// Keys and ids. The package and verify kernels are templates over a policy that supplies, per entry, the
// key state and the ledger id (package) or the expected ids and the verified-prefix word (verify), as
// OneRead / RequestIds do for the CRC verify kernels: MacOneLedger / MacOneRead are one ledger's key as
// a kernel argument (SGPRs); MacLedgers / MacRequests index a table of key states in device memory, so a
// batch spans ledgers with a key each. A table row's inner words are loaded into the hash state before
// the first block and its outer words only after the inner hash, so neither is held across the rounds.
//
// Sources and destinations. The package body (mac_package_lane) is also a template over where an entry's
// bytes lie (MacRanges: one range of the payload; MacSegments: the entry's segments, hashed as one stream
// by the walker of mac_segments.hpp, which the host route shares) and over what is written for it
// (MacFrames: a frame at a stride; MacV2Heads: the 80-byte head of a V2 add request);
// mac_package_adds_kernel launches it for the composite and V2 calls. The kernel is ALU-bound — some
// 40 000 VALU instructions per 4 KiB entry — so the lane that hashed an entry stores its frame or head
// itself; the reason the CRC streaming kernels keep their frame stores in a pass of their own (stores
// between the loads of a bandwidth-bound loop) does not apply.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bkdigest.h"
#include "crc_kernels.hpp"
#include "mac_segments.hpp"
#include "mac_sha1.hpp"
#include "plan_kernels.hpp"

namespace bkd {

constexpr int kMacBlock = 256;

// The ledger's key state (bkd_mac_key_init), a kernel argument: [0..4] inner, [5..9] outer.
struct MacKey {
    uint32_t s[10];
    __device__ __forceinline__ const uint32_t* inner() const { return s; }
    __device__ __forceinline__ const uint32_t* outer() const { return s + 5; }
};

// Row k of a key table (nkeys x 10 words in device memory, each row what bkd_mac_key_init writes), or no
// row when k >= nkeys: such an entry is unreadable, and no word outside the table is ever loaded. A lane
// holds the index (one VGPR; the table is the wave's, in SGPRs) and forms the address where it loads.
struct MacKeyRow {
    const uint32_t* __restrict__ states;
    uint64_t nkeys;
    uint32_t k;
    __device__ __forceinline__ bool valid() const { return k < nkeys; }
    __device__ __forceinline__ const uint32_t* inner() const { return states + (uint64_t)k * 10u; }
    __device__ __forceinline__ const uint32_t* outer() const { return inner() + 5; }
};

// An entry's bytes as a stream of aligned dwords: dword k is a[k], valid (it holds a byte of the
// range) for k < na; shift = the range's byte offset inside a[0].
struct MacStream {
    const uint32_t* a;
    uint32_t shift;
    uint32_t na;
    __device__ __forceinline__ MacStream(const uint8_t* p, uint32_t len) {
        shift = (uint32_t)((uintptr_t)p & 3u);
        a = (const uint32_t*)(p - shift);  // pointer arithmetic, not an integer cast: the loads stay global_load
        na = len ? (shift + len + 3u) >> 2 : 0u;  // len <= BKD_MAC_MAX_ENTRY: no overflow
    }
    // d[0..N) = dwords k0 .. k0 + N - 1, zero where the dword holds no byte of the range
    template <int N>
    __device__ __forceinline__ void load(uint32_t k0, uint32_t (&d)[N]) const {
        if (k0 + (uint32_t)N <= na) {
#pragma unroll
            for (int i = 0; i < N; ++i) d[i] = a[k0 + i];
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) d[i] = k0 + (uint32_t)i < na ? a[k0 + i] : 0u;
        }
    }
    // The big-endian message word whose first byte is byte `shift` of lo: byte funnel and swap in one
    // v_perm_b32 (selector bytes 0-3 pick from lo, 4-7 from hi).
    __device__ __forceinline__ uint32_t word(uint32_t lo, uint32_t hi) const {
        return __builtin_amdgcn_perm(hi, lo, 0x00010203u + 0x01010101u * shift);
    }
};

// mac[5] = HMAC over pre[0..8) (PREFIX: the 32-byte frame header as big-endian words) followed by the
// len bytes of the stream that start at its dword k0 (byte `shift` of it). key: MacKey or MacKeyRow; the
// outer words are read only after the inner hash.
template <bool PREFIX, class Key>
__device__ __forceinline__ void mac_entry(const Key& key, const uint32_t (&pre)[8], const MacStream& in,
                                          uint32_t k0, uint32_t len, uint32_t (&mac)[5]) {
    const uint64_t m = (uint64_t)len + (PREFIX ? 32u : 0u);
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = sha1::hmac_inner_bits(m);
    uint32_t h[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = key.inner()[k];
    uint64_t pos = 0;
    uint32_t edge;  // the dword the next block's first word starts in
    {
        uint32_t first[1];
        in.load<1>(k0, first);
        edge = first[0];
    }
    ++k0;
    if (PREFIX) {  // block 0: the header and the first 32 bytes of the stream
        uint32_t d[8], w[16];
        in.load<8>(k0, d);
#pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = pre[t];
#pragma unroll
        for (int t = 0; t < 8; ++t) w[8 + t] = in.word(t == 0 ? edge : d[t - 1], d[t]);
        if (m < 64u) {
#pragma unroll
            for (int t = 8; t < 16; ++t) w[t] = sha1::padded_word(w[t], 4u * t, m, padded, bits);
        }
        sha1::compress(h, w);
        edge = d[7];
        k0 += 8u;
        pos = 64u;
    }
    if (pos < padded) {
        uint32_t d[16];
        in.load<16>(k0, d);
        for (;;) {
            uint32_t w[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) w[t] = in.word(t == 0 ? edge : d[t - 1], d[t]);
            edge = d[15];
            k0 += 16u;
            const bool last = pos + 64u >= padded;
            if (!last) in.load<16>(k0, d);  // block k + 1's loads in flight during block k's rounds
            if (pos + 64u > m) {
#pragma unroll
                for (int t = 0; t < 16; ++t) w[t] = sha1::padded_word(w[t], pos + 4u * t, m, padded, bits);
            }
            sha1::compress(h, w);
            if (last) break;
            pos += 64u;
        }
    }
    sha1::hmac_outer(key.outer(), h, mac);
}

// In range and under the cap: the only entries that are read.
__device__ __forceinline__ bool mac_readable(uint64_t o, uint32_t l, uint64_t size) {
    return o <= size && (uint64_t)l <= size - o && l <= BKD_MAC_MAX_ENTRY;
}

// 4 n bytes of big-endian words to p: dword stores where p is 4-byte aligned, bytes otherwise.
template <int N>
__device__ __forceinline__ void store_be_words(uint8_t* p, const uint32_t (&w)[N]) {
    if (((uintptr_t)p & 3u) == 0u) {
#pragma unroll
        for (int k = 0; k < N; ++k) ((uint32_t*)p)[k] = __builtin_bswap32(w[k]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            p[4 * k] = (uint8_t)(w[k] >> 24);
            p[4 * k + 1] = (uint8_t)(w[k] >> 16);
            p[4 * k + 2] = (uint8_t)(w[k] >> 8);
            p[4 * k + 3] = (uint8_t)w[k];
        }
    }
}

// out + 20 i = HMAC(entry i); an entry out of range or over the cap is not read, gets zeros and raises err.
__global__ void __launch_bounds__(kMacBlock) mac_batch_kernel(MacKey key, const uint8_t* __restrict__ base,
                                                              uint64_t size, const uint64_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ lengths, uint64_t n,
                                                              uint8_t* __restrict__ out, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    uint32_t mac[5] = {0u, 0u, 0u, 0u, 0u};
    if (mac_readable(o, l, size)) {
        const uint32_t none[8] = {};
        const MacStream in(base + o, l);
        mac_entry<false>(key, none, in, 0u, l, mac);
    } else {
        atomicOr(err, 1u);
    }
    store_be_words(out + i * 20u, mac);
}

// ---- who keys and frames entry i of a package call ------------------------------------------------
//   const auto x = who.entry(i);
//   x.keyed()       the entry has a key (a table index inside the table)
//   x.key()         MacKey or MacKeyRow
//   x.ledger_id()   the ledger id its header carries

// One ledger (bkd_digest_package_batch_mac): its key state and id as kernel arguments.
struct MacOneLedger {
    MacKey k;
    int64_t lid;
    __device__ __forceinline__ const MacOneLedger& entry(uint64_t) const { return *this; }
    __device__ __forceinline__ bool keyed() const { return true; }
    __device__ __forceinline__ const MacKey& key() const { return k; }
    __device__ __forceinline__ int64_t ledger_id() const { return lid; }
};

// A ledger per entry (bkd_digest_package_batch_ledgers_mac): entry i is framed for ledger_ids[i] and
// keyed with row key_of[i] of the table.
struct MacLedgers {
    const uint32_t* __restrict__ key_states;
    uint64_t nkeys;
    const uint32_t* __restrict__ key_of;
    const int64_t* __restrict__ ledger_ids;
    struct Entry {
        MacKeyRow k;
        int64_t lid;
        __device__ __forceinline__ bool keyed() const { return k.valid(); }
        __device__ __forceinline__ const MacKeyRow& key() const { return k; }
        __device__ __forceinline__ int64_t ledger_id() const { return lid; }
    };
    __device__ __forceinline__ Entry entry(uint64_t i) const {
        return Entry{MacKeyRow{key_states, nkeys, key_of[i]}, ledger_ids[i]};
    }
};

// MacLedgers for the composite and V2 calls (bkd_digest_package_batch_segments_mac, _v2_mac), whose index
// arrays are optional: a null key_of keys every entry with row 0, a null ledger_ids frames every entry
// for ledger_id.
struct MacLedgersOr {
    const uint32_t* __restrict__ key_states;
    uint64_t nkeys;
    const uint32_t* __restrict__ key_of;
    const int64_t* __restrict__ ledger_ids;
    int64_t ledger_id;
    __device__ __forceinline__ MacLedgers::Entry entry(uint64_t i) const {
        return MacLedgers::Entry{MacKeyRow{key_states, nkeys, key_of ? key_of[i] : 0u},
                                 ledger_ids ? ledger_ids[i] : ledger_id};
    }
};

// ---- where entry i of a package call lies ------------------------------------------------------------
//   const auto e = src.entry(i, err);   (a malformed index raises err here)
//   e.readable()            in range and under the cap: the only entries that are read
//   e.length()              its bytes
//   e.hash(key, hdr, mac)   mac[5] = HMAC(hdr || the entry's bytes)

// One range of the payload per entry (bkd_digest_package_batch_mac, _ledgers_mac, _v2_mac).
struct MacRanges {
    const uint8_t* __restrict__ payload;
    uint64_t size;
    const uint64_t* __restrict__ offsets;
    const uint32_t* __restrict__ lengths;
    struct Entry {
        const uint8_t* __restrict__ payload;
        uint64_t size, o;
        uint32_t l;
        __device__ __forceinline__ bool readable() const { return mac_readable(o, l, size); }
        __device__ __forceinline__ uint32_t length() const { return l; }
        template <class Key>
        __device__ __forceinline__ void hash(const Key& key, const uint32_t (&hdr)[8], uint32_t (&mac)[5]) const {
            const MacStream in(payload + o, l);
            mac_entry<true>(key, hdr, in, 0u, l, mac);
        }
    };
    __device__ __forceinline__ Entry entry(uint64_t i, uint32_t*) const {
        return Entry{payload, size, offsets[i], lengths[i]};
    }
};

// The load primitive of the segment walker on the device: the aligned dword itself. The walker asks only
// for dwords that hold a byte of the segment.
struct MacDwordLoad {
    __device__ __forceinline__ uint32_t operator()(const uint8_t* at, const uint8_t*, uint32_t) const {
        return *(const uint32_t*)at;
    }
};

// The entry's segments (bkd_digest_package_batch_segments_mac): entry i = segments first[i] ..
// first[i + 1] - 1 of the CSR, clamped by segments_range (a malformed one raises err), empty ones skipped.
// Its length is their 64-bit sum, given up once it passes the cap (segments_length_capped); an entry
// over the cap or with a non-empty segment out of range is unreadable, and none of its bytes is loaded.
struct MacSegments {
    const uint8_t* __restrict__ payload;
    uint64_t size;
    const uint64_t* __restrict__ seg_offsets;
    const uint32_t* __restrict__ seg_lengths;
    uint64_t nseg;
    const uint64_t* __restrict__ first;
    uint64_t n;
    // The non-empty segments of one entry in order, for the walker.
    struct Cursor {
        const uint8_t* __restrict__ payload;
        const uint64_t* __restrict__ seg_offsets;
        const uint32_t* __restrict__ seg_lengths;
        uint64_t k, k1;
        __device__ __forceinline__ bool next(const uint8_t*& p, uint32_t& len) {
            while (k < k1) {
                len = seg_lengths[k];
                const uint64_t o = seg_offsets[k];
                ++k;
                if (len) {
                    p = payload + o;
                    return true;
                }
            }
            return false;
        }
    };
    struct Entry {
        const MacSegments& s;
        uint64_t k0, k1;
        uint32_t total;
        bool ok;
        __device__ __forceinline__ bool readable() const { return ok; }
        __device__ __forceinline__ uint32_t length() const { return total; }
        template <class Key>
        __device__ __forceinline__ void hash(const Key& key, const uint32_t (&hdr)[8], uint32_t (&mac)[5]) const {
            Cursor segs{s.payload, s.seg_offsets, s.seg_lengths, k0, k1};
            macseg::hmac(key, hdr, segs, total, MacDwordLoad{}, mac);
        }
    };
    __device__ __forceinline__ Entry entry(uint64_t i, uint32_t* err) const {
        const SegRange sr = segments_range(first[i], first[i + 1], i, n, nseg);
        if (sr.bad) atomicOr(err, 1u);
        const SegLength sl = segments_length_capped(seg_lengths, sr.k0, sr.k1, BKD_MAC_MAX_ENTRY);
        bool ok = !sl.over;
        if (ok) {
            for (uint64_t k = sr.k0; k < sr.k1; ++k) {
                const uint32_t len = seg_lengths[k];
                if (!len) continue;  // an empty segment is skipped wherever it says it lies
                const uint64_t o = seg_offsets[k];
                ok = ok && o <= size && (uint64_t)len <= size - o;
            }
        }
        return Entry{*this, sr.k0, sr.k1, (uint32_t)sl.bytes, ok};
    }
};

// ---- what is written for entry i of a package call ---------------------------------------------------
//   dst.store(i, len, hashed, hdr, mac, err)   hashed: the entry was read (mac holds zeros otherwise)

// frames + i * stride = [32 B header][20 B mac]; no other byte of the stride is written.
struct MacFrames {
    uint8_t* __restrict__ frames;
    uint64_t stride;
    __device__ __forceinline__ void store(uint64_t i, uint32_t, bool, const uint32_t (&hdr)[8], const uint32_t (&mac)[5],
                                          uint32_t*) const {
        uint8_t* f = frames + i * stride;
        store_be_words(f, hdr);
        store_be_words(f + 32, mac);
    }
};

// The head of V2 add request i (bkd_digest_package_batch_v2_mac; the layout of package_v2_head_kernel
// with a 20-byte digest): [int32 BE 76 + len][int32 BE packet header][20 B master key][32 B header]
// [20 B mac], 80 bytes as twenty big-endian words, by dword stores when the request is 4-byte aligned and
// by bytes otherwise. A request that does not fit the request buffer raises err and is left alone.
// copy_len[i] = the bytes package_v2_copy_kernel is to copy in behind the head: len for an entry that was
// hashed, 0 for an unreadable one (the copy kernel itself skips lengths at or over the threshold).
struct MacV2Heads {
    V2Requests rq;
    const uint8_t* __restrict__ keys;
    uint64_t key_stride;
    uint32_t packet_header;
    uint32_t* __restrict__ copy_len;
    __device__ __forceinline__ void store(uint64_t i, uint32_t len, bool hashed, const uint32_t (&hdr)[8],
                                          const uint32_t (&mac)[5], uint32_t* err) const {
        copy_len[i] = hashed ? len : 0u;
        uint8_t* r = rq.at(i, hashed ? len : 0u);
        if (!r) {
            atomicOr(err, 1u);
            return;
        }
        uint32_t w[20];
        w[0] = rq.head() - 4u + len;  // headersSize + payloadSize (Java int arithmetic)
        w[1] = packet_header;
        const uint8_t* key = keys + i * key_stride;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            w[2 + k] = ((uint32_t)key[4 * k] << 24) | ((uint32_t)key[4 * k + 1] << 16) | ((uint32_t)key[4 * k + 2] << 8) |
                       (uint32_t)key[4 * k + 3];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[7 + k] = hdr[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) w[15 + k] = mac[k];
        store_be_words(r, w);
    }
};

// Entry i's header [ledger id, entry_ids[i], lacs[i], length_fields[i] as BE longs] and the MAC over it
// and the entry's bytes (DigestManager.java:146-155, 172-178), written where dst puts them. An unreadable
// entry (out of range, over the cap, or without a key): the header is written, the MAC bytes are zero,
// err is raised.
template <class Who, class Src, class Dst>
__device__ __forceinline__ void mac_package_lane(const Who& who, const int64_t* __restrict__ entry_ids,
                                                 const int64_t* __restrict__ lacs,
                                                 const int64_t* __restrict__ length_fields, const Src& src, uint64_t n,
                                                 const Dst& dst, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const auto e = src.entry(i, err);
    const auto x = who.entry(i);
    const uint64_t f4[4] = {(uint64_t)x.ledger_id(), (uint64_t)entry_ids[i], (uint64_t)lacs[i],
                            (uint64_t)length_fields[i]};
    uint32_t hdr[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hdr[2 * k] = (uint32_t)(f4[k] >> 32);
        hdr[2 * k + 1] = (uint32_t)f4[k];
    }
    uint32_t mac[5] = {0u, 0u, 0u, 0u, 0u};
    const bool hashed = x.keyed() && e.readable();
    if (hashed) e.hash(x.key(), hdr, mac);
    else atomicOr(err, 1u);
    dst.store(i, e.length(), hashed, hdr, mac, err);
}

// One range per entry into frames at a stride — MacRanges into MacFrames — with its arguments flat, as the
// single-ledger and many-ledger package calls have always launched it. It keeps its own body: through
// mac_package_lane the compiler scheduled the same work differently (2 690 -> 2 645 instructions for
// MacLedgers), and these two instantiations are to stay the machine code they were
// (profiles/mac_adds_kernel_disasm.txt).
template <class Who>
__global__ void __launch_bounds__(kMacBlock) mac_package_kernel(
    Who who, const int64_t* __restrict__ entry_ids, const int64_t* __restrict__ lacs,
    const int64_t* __restrict__ length_fields, const uint8_t* __restrict__ payload, uint64_t size,
    const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lengths, uint64_t n,
    uint8_t* __restrict__ frames, uint64_t stride, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    const auto x = who.entry(i);
    const uint64_t f4[4] = {(uint64_t)x.ledger_id(), (uint64_t)entry_ids[i], (uint64_t)lacs[i],
                            (uint64_t)length_fields[i]};
    uint32_t hdr[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hdr[2 * k] = (uint32_t)(f4[k] >> 32);
        hdr[2 * k + 1] = (uint32_t)f4[k];
    }
    uint32_t mac[5] = {0u, 0u, 0u, 0u, 0u};
    if (x.keyed() && mac_readable(o, l, size)) {
        const MacStream in(payload + o, l);
        mac_entry<true>(x.key(), hdr, in, 0u, l, mac);
    } else {
        atomicOr(err, 1u);
    }
    uint8_t* f = frames + i * stride;
    store_be_words(f, hdr);
    store_be_words(f + 32, mac);
}

// Any source into any destination: the composite and V2 calls.
template <class Who, class Src, class Dst>
__global__ void __launch_bounds__(kMacBlock) mac_package_adds_kernel(
    Who who, const int64_t* __restrict__ entry_ids, const int64_t* __restrict__ lacs,
    const int64_t* __restrict__ length_fields, Src src, uint64_t n, Dst dst, uint32_t* __restrict__ err) {
    mac_package_lane(who, entry_ids, lacs, length_fields, src, n, dst, err);
}

// ---- who keys frame i of a verify call and what it must carry ---------------------------------------
//   const auto x = who.entry(i);
//   x.keyed(), x.key()    as above
//   x.id_status(hw, i)    0, 3 (ledger id) or 4 (entry id) from the header's first four words (values)
//   x.failed(i)           entry i failed: lowers the verified-prefix word it belongs to

// One read (bkd_digest_verify_batch_mac): one key, one ledger id, entry ids first_entry_id + i (id_checks
// 0 only), one verified-prefix word, initialised to n by an earlier launch.
struct MacOneRead {
    MacKey k;
    int64_t ledger_id, first_entry_id;
    int id_checks;
    unsigned long long* first_bad;
    __device__ __forceinline__ const MacOneRead& entry(uint64_t) const { return *this; }
    __device__ __forceinline__ bool keyed() const { return true; }
    __device__ __forceinline__ const MacKey& key() const { return k; }
    __device__ __forceinline__ int32_t id_status(const uint32_t* hw, uint64_t i) const {
        const int64_t lid = (int64_t)(((uint64_t)hw[0] << 32) | hw[1]);
        const int64_t eid = (int64_t)(((uint64_t)hw[2] << 32) | hw[3]);
        if (lid != ledger_id) return 3;
        if (id_checks == 0 && eid != first_entry_id + (int64_t)i) return 4;
        return 0;
    }
    __device__ __forceinline__ void failed(uint64_t i) const { atomicMin(first_bad, (unsigned long long)i); }
};

// Read requests (bkd_digest_verify_requests_mac): the per-entry expectations request_expand_kernel wrote
// (RequestIds, crc_kernels.hpp) and row req_keys[r] of the table for the entries of request r. A lane
// keeps its request word and its row across the hash; the expected ids are loaded after it, where they
// are compared. Entries of one request are neighbouring lanes, so their key loads mostly hit one line.
struct MacRequests {
    const uint32_t* __restrict__ key_states;
    uint64_t nkeys;
    const uint32_t* __restrict__ req_keys;
    RequestIds ids;
    struct Entry {
        MacKeyRow k;
        uint32_t req;
        const RequestIds& ids;
        __device__ __forceinline__ bool keyed() const { return k.valid(); }
        __device__ __forceinline__ const MacKeyRow& key() const { return k; }
        __device__ __forceinline__ int32_t id_status(const uint32_t* hw, uint64_t i) const {
            const uint64_t lid = (uint64_t)ids.exp_lid[i], eid = (uint64_t)ids.exp_eid[i];
            const uint32_t dl = (hw[0] ^ (uint32_t)(lid >> 32)) | (hw[1] ^ (uint32_t)lid);
            const uint32_t de = (hw[2] ^ (uint32_t)(eid >> 32)) | (hw[3] ^ (uint32_t)eid);
            return dl ? 3 : ((de && !(req & kReqSkipEntryId)) ? 4 : 0);
        }
        __device__ __forceinline__ void failed(uint64_t i) const {
            const uint32_t r = req & ~kReqSkipEntryId;
            atomicMin(ids.req_first_bad + r, (unsigned long long)(i - ids.req_first[r]));
        }
    };
    __device__ __forceinline__ Entry entry(uint64_t i) const {
        const uint32_t req = ids.req_of[i];  // < nreq, whatever the CSR holds (request_expand_kernel)
        return Entry{MacKeyRow{key_states, nkeys, req_keys[req & ~kReqSkipEntryId]}, req, ids};
    }
};

// A staged segment of the host form (bkd_digest_verify_requests_mac_host): the host expanded the requests
// itself, so entry i has its key row key_of[i], its expected ids and its flag word (bit 31: skip the
// entry-id check) side by side. No prefix word: a request may straddle two segments, and the host takes
// each request's prefix from the statuses.
struct MacExpected {
    const uint32_t* __restrict__ key_states;
    uint64_t nkeys;
    const uint32_t* __restrict__ key_of;
    const int64_t* __restrict__ exp_lid;
    const int64_t* __restrict__ exp_eid;
    const uint32_t* __restrict__ flags;
    struct Entry {
        MacKeyRow k;
        const MacExpected& p;
        __device__ __forceinline__ bool keyed() const { return k.valid(); }
        __device__ __forceinline__ const MacKeyRow& key() const { return k; }
        __device__ __forceinline__ int32_t id_status(const uint32_t* hw, uint64_t i) const {
            const uint64_t lid = (uint64_t)p.exp_lid[i], eid = (uint64_t)p.exp_eid[i];
            const uint32_t dl = (hw[0] ^ (uint32_t)(lid >> 32)) | (hw[1] ^ (uint32_t)lid);
            const uint32_t de = (hw[2] ^ (uint32_t)(eid >> 32)) | (hw[3] ^ (uint32_t)eid);
            return dl ? 3 : ((de && !(p.flags[i] & kReqSkipEntryId)) ? 4 : 0);
        }
        __device__ __forceinline__ void failed(uint64_t) const {}
    };
    __device__ __forceinline__ Entry entry(uint64_t i) const {
        return Entry{MacKeyRow{key_states, nkeys, key_of[i]}, *this};
    }
};

// Frame i = [32 B header][20 B mac][payload] (DigestManager.verifyDigest, DigestManager.java:226-283):
// status 1 too short (or unreadable: out of range, over the cap or without a key, which also raises err),
// 2 the MAC over [0, 32) || [52, len) differs from the stored one, 3 ledger id, 4 entry id; the first
// failing index lowers the verified-prefix word of `who`.
template <class Who>
__global__ void __launch_bounds__(kMacBlock) mac_verify_kernel(
    Who who, const uint8_t* __restrict__ framed, uint64_t size, const uint64_t* __restrict__ offsets,
    const uint32_t* __restrict__ lengths, uint64_t n, int32_t* __restrict__ status, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    const auto x = who.entry(i);
    int32_t st;
    if (!x.keyed() || !mac_readable(o, l, size)) {
        st = 1;
        atomicOr(err, 1u);
    } else if (l < 52u) {
        st = 1;
    } else {
        const MacStream in(framed + o, l);
        uint32_t d[14], hw[13];  // bytes [0, 52): dword 13 is read only where the frame reaches into it
        in.load<14>(0u, d);
#pragma unroll
        for (int t = 0; t < 13; ++t) hw[t] = in.word(d[t], d[t + 1]);
        uint32_t pre[8], mac[5];
#pragma unroll
        for (int t = 0; t < 8; ++t) pre[t] = hw[t];
        mac_entry<true>(x.key(), pre, in, 13u, l - 52u, mac);
        uint32_t diff = 0u;
#pragma unroll
        for (int k = 0; k < 5; ++k) diff |= mac[k] ^ hw[8 + k];
        st = diff ? 2 : x.id_status(hw, i);
    }
    status[i] = st;
    if (st != 0) x.failed(i);
}

// ---- re-framing with a new LAC (bkd_digest_reframe_requests_mac) -------------------------------------
// HMAC has no algebra that carries a digest from one header to another (the CRC reframe's GF(2)
// correction), so a MAC reframe hashes again. The old and the new frame differ only in header bytes
// 16..23, words 4 and 5 of the first block; every later block of the inner hash holds the same words for
// both. mac_entry2 therefore walks the stream once — one set of loads, one v_perm_b32 per word, one
// schedule expansion per block — and runs two round chains on it (sha1::compress2): chain V from the
// header as it lies, chain N from the header with the new LAC. Block 0 and the outer hashes differ in their
// words and are compressed per chain.
template <class Key>
__device__ __forceinline__ void mac_entry2(const Key& key, const uint32_t (&pre)[8], uint32_t lac_hi, uint32_t lac_lo,
                                           const MacStream& in, uint32_t k0, uint32_t len, uint32_t (&mac_v)[5],
                                           uint32_t (&mac_n)[5]) {
    const uint64_t m = (uint64_t)len + 32u;
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = sha1::hmac_inner_bits(m);
    uint32_t hv[5], hn[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) hv[k] = hn[k] = key.inner()[k];
    uint32_t edge;  // the dword the next block's first word starts in
    {
        uint32_t first[1];
        in.load<1>(k0, first);
        edge = first[0];
    }
    ++k0;
    {  // block 0: the header and the first 32 bytes of the stream, once per header
        uint32_t d[8], w[16], w2[16];
        in.load<8>(k0, d);
#pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = pre[t];
#pragma unroll
        for (int t = 0; t < 8; ++t) w[8 + t] = in.word(t == 0 ? edge : d[t - 1], d[t]);
        if (m < 64u) {
#pragma unroll
            for (int t = 8; t < 16; ++t) w[t] = sha1::padded_word(w[t], 4u * t, m, padded, bits);
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) w2[t] = w[t];
        w2[4] = lac_hi;
        w2[5] = lac_lo;
        sha1::compress(hv, w);
        sha1::compress(hn, w2);
        edge = d[7];
        k0 += 8u;
    }
    uint64_t pos = 64u;
    if (pos < padded) {
        uint32_t d[16];
        in.load<16>(k0, d);
        for (;;) {
            uint32_t w[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) w[t] = in.word(t == 0 ? edge : d[t - 1], d[t]);
            edge = d[15];
            k0 += 16u;
            const bool last = pos + 64u >= padded;
            if (!last) in.load<16>(k0, d);  // block k + 1's loads in flight during block k's rounds
            if (pos + 64u > m) {
#pragma unroll
                for (int t = 0; t < 16; ++t) w[t] = sha1::padded_word(w[t], pos + 4u * t, m, padded, bits);
            }
            sha1::compress2(hv, hn, w);
            if (last) break;
            pos += 64u;
        }
    }
    sha1::hmac_outer(key.outer(), hv, mac_v);
    sha1::hmac_outer(key.outer(), hn, mac_n);
}

// Frame i as mac_verify_kernel reads it, re-framed with new_lacs[i] where its status is 0.
//
// Default (TRUSTED == false): status, precedence, the verified-prefix word of `who` and the bounds flag are
// those of mac_verify_kernel<Who> on the same input; the MAC under the new header comes from the same pass
// (mac_entry2) and is written only for status 0.
// TRUSTED: the caller has verified the frames. One chain (mac_entry<true>, the new header as prefix); the
// status is what the header alone decides — 1 too short, unreadable or no key row, else the policy's
// id_status — never 2. Unlike the CRC trusted reframe, which carries a wrong digest over into a digest
// that is wrong again, the MAC written here is valid for the bytes as they lie: a frame whose payload was
// damaged comes out verifying. The caller vouches for the bytes.
//
// Output, status 0 only; no byte of any other frame or out-frame is written.
//   apart (out_frames != null): [32 B header with the new LAC][20 B MAC] at out_frames + i * stride.
//   in place: bytes 16..23 and 32..51 of the frame itself.
// Frames start at any byte address and may lie back to back, so a lane's aligned edge dwords can hold bytes
// of a neighbour's frame that the neighbour's lane rewrites in this launch. The loads do not mind: bytes
// outside the frame never reach the hash. The stores never read-modify-write: store_be_words writes whole
// dwords only where the range is 4-byte aligned (its dwords then lie inside it) and single bytes otherwise.
// The lane holds bytes [0, 52) in registers before its first store (the status depends on them).
template <class Who, bool TRUSTED>
__global__ void __launch_bounds__(kMacBlock) mac_reframe_kernel(
    Who who, uint8_t* framed, uint64_t size, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lengths,
    uint64_t n, const int64_t* __restrict__ new_lacs, uint8_t* out_frames, uint64_t stride,
    int32_t* __restrict__ status, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    const auto x = who.entry(i);
    int32_t st;
    if (!x.keyed() || !mac_readable(o, l, size)) {
        st = 1;
        atomicOr(err, 1u);
    } else if (l < 52u) {
        st = 1;
    } else {
        const MacStream in(framed + o, l);
        const uint64_t lac = (uint64_t)new_lacs[i];
        uint32_t d[14], hw[13];  // bytes [0, 52), as mac_verify_kernel holds them
        in.load<14>(0u, d);
#pragma unroll
        for (int t = 0; t < 13; ++t) hw[t] = in.word(d[t], d[t + 1]);
        uint32_t hdr[8], mac[5];
#pragma unroll
        for (int t = 0; t < 8; ++t) hdr[t] = hw[t];
        if (TRUSTED) {
            hdr[4] = (uint32_t)(lac >> 32);
            hdr[5] = (uint32_t)lac;
            mac_entry<true>(x.key(), hdr, in, 13u, l - 52u, mac);
            st = x.id_status(hw, i);
        } else {
            uint32_t old[5];
            mac_entry2(x.key(), hdr, (uint32_t)(lac >> 32), (uint32_t)lac, in, 13u, l - 52u, old, mac);
            uint32_t diff = 0u;
#pragma unroll
            for (int k = 0; k < 5; ++k) diff |= old[k] ^ hw[8 + k];
            st = diff ? 2 : x.id_status(hw, i);
            hdr[4] = (uint32_t)(lac >> 32);
            hdr[5] = (uint32_t)lac;
        }
        if (st == 0) {
            if (out_frames) {
                uint8_t* f = out_frames + i * stride;
                store_be_words(f, hdr);
                store_be_words(f + 32, mac);
            } else {
                uint8_t* f = framed + o;
                const uint32_t lw[2] = {hdr[4], hdr[5]};
                store_be_words(f + 16, lw);
                store_be_words(f + 32, mac);
            }
        }
    }
    status[i] = st;
    if (st != 0) x.failed(i);
}

}  // namespace bkd
