// SHA-1 / HMAC-SHA1 arithmetic shared by the host route (host_mac.cpp) and the device kernels
// (mac_kernels.hpp): the compression function and the padding and bit-length logic, so that the CPU
// suite exercises the same length arithmetic the GPU runs. Plain C++ only: no host or device calls.
//
// MacDigestManager ($BK/proto/checksum/MacDigestManager.java:61,79-84) keys HmacSHA1 with
// SHA1("mac" || passwd): 20 bytes, shorter than one SHA-1 block, so the states after compressing
// key ^ ipad and key ^ opad are fixed per ledger (the "key state": five inner words, five outer words).
// An entry's MAC is then
//   inner = SHA1 continued from the inner state over the message, padded with bit length 8 (64 + M)
//   mac   = one compression from the outer state over inner || 0x80 || 0.. || bit length 8 * 84.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_HD __host__ __device__ __forceinline__
#else
#define BKD_HD inline
#endif

namespace bkd {
namespace sha1 {

constexpr uint32_t kInit[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};

BKD_HD uint32_t rol(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// The three-input bit operations of the rounds and the schedule. The compiler turns rol into
// v_alignbit_b32 and the three-term sums into v_add3_u32 by itself, but left these as chains of two-input
// xor / and (gfx9 has no v_xor3_b32, and its v_bfi_b32 was not picked), so on gfx950 they name the
// three-input v_bitop3_b32 through its builtin; the truth table is the expression over a = 0xF0,
// b = 0xCC, c = 0xAA.
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
BKD_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
BKD_HD uint32_t bitsel(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xCA); }
BKD_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
#else
BKD_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
BKD_HD uint32_t bitsel(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (~a & c); }  // a ? b : c, per bit
BKD_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }
#endif

// One block: w[16] = the block's words as big-endian values (clobbered: it is the rolling schedule
// window, statically indexed once the 80 rounds are unrolled).
BKD_HD void compress(uint32_t (&h)[5], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < 80; ++t) {
        uint32_t x;
        if (t < 16) {
            x = w[t];
        } else {
            x = rol(xor3(w[(t + 13) & 15], w[(t + 8) & 15], w[(t + 2) & 15]) ^ w[t & 15], 1);
            w[t & 15] = x;
        }
        uint32_t f, k;
        if (t < 20) {
            f = bitsel(b, c, d);
            k = 0x5A827999u;
        } else if (t < 40) {
            f = xor3(b, c, d);
            k = 0x6ED9EBA1u;
        } else if (t < 60) {
            f = maj(b, c, d);
            k = 0x8F1BBCDCu;
        } else {
            f = xor3(b, c, d);
            k = 0xCA62C1D6u;
        }
        const uint32_t tmp = rol(a, 5) + f + (e + k + x);
        e = d;
        d = c;
        c = rol(b, 30);
        b = a;
        a = tmp;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}

// One block into two states: the block's words are the same for both (a reframe hashes every block behind
// the first under the old and under the new header, HMAC's inner states differing from block 0 on), so the
// schedule window w is expanded once and feeds two round chains, which are independent of each other and
// interleave. w is clobbered as in compress.
BKD_HD void compress2(uint32_t (&hA)[5], uint32_t (&hB)[5], uint32_t (&w)[16]) {
    uint32_t a = hA[0], b = hA[1], c = hA[2], d = hA[3], e = hA[4];
    uint32_t p = hB[0], q = hB[1], r = hB[2], s = hB[3], u = hB[4];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < 80; ++t) {
        uint32_t x;
        if (t < 16) {
            x = w[t];
        } else {
            x = rol(xor3(w[(t + 13) & 15], w[(t + 8) & 15], w[(t + 2) & 15]) ^ w[t & 15], 1);
            w[t & 15] = x;
        }
        uint32_t f, g, k;
        if (t < 20) {
            f = bitsel(b, c, d);
            g = bitsel(q, r, s);
            k = 0x5A827999u;
        } else if (t < 40) {
            f = xor3(b, c, d);
            g = xor3(q, r, s);
            k = 0x6ED9EBA1u;
        } else if (t < 60) {
            f = maj(b, c, d);
            g = maj(q, r, s);
            k = 0x8F1BBCDCu;
        } else {
            f = xor3(b, c, d);
            g = xor3(q, r, s);
            k = 0xCA62C1D6u;
        }
        const uint32_t kx = k + x;  // shared by the two chains
        const uint32_t tmpA = rol(a, 5) + f + (e + kx);
        const uint32_t tmpB = rol(p, 5) + g + (u + kx);
        e = d;
        d = c;
        c = rol(b, 30);
        b = a;
        a = tmpA;
        u = s;
        s = r;
        r = rol(q, 30);
        q = p;
        p = tmpB;
    }
    hA[0] += a;
    hA[1] += b;
    hA[2] += c;
    hA[3] += d;
    hA[4] += e;
    hB[0] += p;
    hB[1] += q;
    hB[2] += r;
    hB[3] += s;
    hB[4] += u;
}

// Bytes of a message of m bytes once padded (0x80, zeros, the 8-byte bit length): a multiple of 64.
BKD_HD uint64_t padded_bytes(uint64_t m) { return (m + 9u + 63u) & ~(uint64_t)63; }

// The word at byte position pos (a multiple of 4) of the padded message. m: the message's bytes;
// padded = padded_bytes(m); bits: the bit length the padding carries (it counts what was hashed in front
// of this message too, HMAC's key block). w: the big-endian word of the message's bytes [pos, pos + 4),
// of which only the bytes below m are looked at — the others may hold anything.
BKD_HD uint32_t padded_word(uint32_t w, uint64_t pos, uint64_t m, uint64_t padded, uint64_t bits) {
    if (pos + 4u <= m) return w;
    if (pos == padded - 8u) return (uint32_t)(bits >> 32);
    if (pos == padded - 4u) return (uint32_t)bits;
    if (pos > m) return 0u;
    const uint32_t r = (uint32_t)(m - pos) * 8u;  // 0, 8, 16 or 24 message bits in this word
    return (w & ~(0xFFFFFFFFu >> r)) | (0x80000000u >> r);
}

// Bit length carried by the padding of an HMAC inner hash over m message bytes: the 64-byte key block
// counts. 64-bit: a message of 2^29 bytes already passes 2^32 bits.
BKD_HD uint64_t hmac_inner_bits(uint64_t m) { return (m + 64u) * 8u; }

// mac[5] = the outer hash: one compression from the outer state over the 20-byte inner digest.
BKD_HD void hmac_outer(const uint32_t* outer_state, const uint32_t (&inner)[5], uint32_t (&mac)[5]) {
    uint32_t w[16] = {inner[0], inner[1], inner[2], inner[3], inner[4], 0x80000000u, 0u, 0u,
                      0u,       0u,       0u,       0u,       0u,       0u,          0u, (64u + 20u) * 8u};
    for (int k = 0; k < 5; ++k) mac[k] = outer_state[k];
    compress(mac, w);
}

}  // namespace sha1
}  // namespace bkd
