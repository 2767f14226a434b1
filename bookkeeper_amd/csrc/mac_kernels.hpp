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
// Ragged batches: lanes whose entry is finished idle until the wave's longest entry ends.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bkdigest.h"
#include "mac_sha1.hpp"

namespace bkd {

constexpr int kMacBlock = 256;

// The ledger's key state (bkd_mac_key_init), a kernel argument: [0..4] inner, [5..9] outer.
struct MacKey {
    uint32_t s[10];
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
// len bytes of the stream that start at its dword k0 (byte `shift` of it).
template <bool PREFIX>
__device__ __forceinline__ void mac_entry(const MacKey& key, const uint32_t (&pre)[8], const MacStream& in,
                                          uint32_t k0, uint32_t len, uint32_t (&mac)[5]) {
    const uint64_t m = (uint64_t)len + (PREFIX ? 32u : 0u);
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = sha1::hmac_inner_bits(m);
    uint32_t h[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = key.s[k];
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
    sha1::hmac_outer(key.s + 5, h, mac);
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

// frames + i * stride = [ledger id, entry_ids[i], lacs[i], length_fields[i] as BE longs][20 B mac]
// (DigestManager.java:146-155, 172-178); no other byte of the stride is written. An unreadable payload:
// the header is written, the MAC bytes are zero, err is raised.
__global__ void __launch_bounds__(kMacBlock) mac_package_kernel(
    MacKey key, int64_t ledger_id, const int64_t* __restrict__ entry_ids, const int64_t* __restrict__ lacs,
    const int64_t* __restrict__ length_fields, const uint8_t* __restrict__ payload, uint64_t size,
    const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lengths, uint64_t n,
    uint8_t* __restrict__ frames, uint64_t stride, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    const uint64_t f4[4] = {(uint64_t)ledger_id, (uint64_t)entry_ids[i], (uint64_t)lacs[i], (uint64_t)length_fields[i]};
    uint32_t hdr[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hdr[2 * k] = (uint32_t)(f4[k] >> 32);
        hdr[2 * k + 1] = (uint32_t)f4[k];
    }
    uint32_t mac[5] = {0u, 0u, 0u, 0u, 0u};
    if (mac_readable(o, l, size)) {
        const MacStream in(payload + o, l);
        mac_entry<true>(key, hdr, in, 0u, l, mac);
    } else {
        atomicOr(err, 1u);
    }
    uint8_t* f = frames + i * stride;
    store_be_words(f, hdr);
    store_be_words(f + 32, mac);
}

// Frame i = [32 B header][20 B mac][payload] (DigestManager.verifyDigest, DigestManager.java:226-283):
// status 1 too short (or unreadable: out of range or over the cap, which also raises err), 2 the MAC over
// [0, 32) || [52, len) differs from the stored one, 3 ledger id, 4 entry id (id_checks 0 only);
// *first_bad (initialised to n by an earlier launch) is lowered to the first failing index.
__global__ void __launch_bounds__(kMacBlock) mac_verify_kernel(
    MacKey key, int64_t ledger_id, int64_t first_entry_id, int id_checks, const uint8_t* __restrict__ framed,
    uint64_t size, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lengths, uint64_t n,
    int32_t* __restrict__ status, unsigned long long* first_bad, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kMacBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = offsets[i];
    const uint32_t l = lengths[i];
    int32_t st;
    if (!mac_readable(o, l, size)) {
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
        mac_entry<true>(key, pre, in, 13u, l - 52u, mac);
        uint32_t diff = 0u;
#pragma unroll
        for (int k = 0; k < 5; ++k) diff |= mac[k] ^ hw[8 + k];
        const int64_t lid = (int64_t)(((uint64_t)hw[0] << 32) | hw[1]);
        const int64_t eid = (int64_t)(((uint64_t)hw[2] << 32) | hw[3]);
        if (diff) st = 2;
        else if (lid != ledger_id) st = 3;
        else if (id_checks == 0 && eid != first_entry_id + (int64_t)i) st = 4;
        else st = 0;
    }
    status[i] = st;
    if (st != 0) atomicMin(first_bad, (unsigned long long)i);
}

}  // namespace bkd
