// HMAC-SHA1 over a composite entry: the message header || seg0 || seg1 || ... hashed as one byte stream
// without joining the segments (bkd_digest_package_batch_segments_mac). Shared by the device kernel
// (mac_kernels.hpp) and the host route (host_mac.cpp): the cut and carry logic below is the same code on
// both, and only the load primitive differs. Plain C++ over mac_sha1.hpp: no host or device calls.
//
// The stream. SHA-1 eats 16-word blocks, and a segment may start and end at any byte of the message, so
// words and blocks straddle the cuts. Inside a segment the message words are the words of an ordinary
// aligned-dword stream at the virtual address seg - h, where h (0..3) is the number of message bytes
// pending from earlier segments: word j of the segment is the funnel of dwords j and j + 1 of that
// stream, exactly as for a contiguous entry. Only the words at a cut are merged by byte masks:
//   * word 0 of a segment takes its first h bytes from the carry;
//   * the last (h + len) & 3 bytes of a segment become the carry of the next one; a segment shorter
//     than the word it lands in only adds its bytes to the carry.
// Whole blocks inside a segment therefore keep the contiguous kernel's shape: 17 dword loads (the block's
// 16 words touch 17 dwords) issued a block ahead, one funnel per word, no masks. Blocks that hold a cut
// are filled word by word (two loads per word); many tiny segments take that path for every word, which
// is correct and slow.
//
// Loads. load(at, seg, len) returns the little-endian dword at the 4-byte aligned address `at`, and is
// only called for a dword that holds at least one byte of [seg, seg + len) — in particular never for
// the virtual first dword when it lies wholly in front of the segment. The device loads the aligned
// dword; the host builds it from the segment's own bytes (zeros elsewhere), so a sanitizer sees every
// byte the walker depends on. Bytes of an edge dword outside the segment never reach the hash: the
// funnel drops them or the cut masks do.
#pragma once
#include <stdint.h>

#include "mac_sha1.hpp"

namespace bkd {
namespace macseg {

// The big-endian message word whose first byte is byte `shift` of lo and whose last is byte shift - 1 of
// hi (little-endian dwords, as loaded): on the device one v_perm_b32, as MacStream::word.
BKD_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x00010203u + 0x01010101u * shift);
#else
    const uint32_t v = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * shift));
    return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
#endif
}

// The first b bytes (0..3) of a big-endian word.
BKD_HD uint32_t head_mask(uint32_t b) { return b ? ~(0xFFFFFFFFu >> (8u * b)) : 0u; }

// w[t] = x for a t known only at run time, with w kept in registers: sixteen selects, no indexing.
BKD_HD void put(uint32_t (&w)[16], uint32_t t, uint32_t x) {
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 16u; ++k) w[k] = k == t ? x : w[k];
}

// One non-empty segment as message words, h message bytes pending in front of it.
template <class Load>
struct Words {
    const uint8_t* a;    // the aligned address of dword 0 of the virtual stream at seg - h
    const uint8_t* seg;  // the segment itself, for the load primitive
    uint32_t len;
    uint32_t shift;      // (seg - h) & 3
    uint32_t k_lo, na;   // dwords [k_lo, na) hold a byte of the segment; k_lo is 0 or 1
    uint32_t h;          // message bytes in front of word 0's first segment byte
    uint32_t nfull;      // whole words: (h + len) / 4 (word 0 counts: the carry completes it)
    uint32_t tail;       // (h + len) & 3 bytes behind them
    BKD_HD void open(const uint8_t* p, uint32_t l, uint32_t pending) {
        const uint8_t* v = p - pending;  // pointer arithmetic, not an integer cast (MacStream); never dereferenced
        seg = p;
        len = l;
        h = pending;
        shift = (uint32_t)((uintptr_t)v & 3u);
        a = v - shift;
        k_lo = (shift + h) >> 2;
        // 64-bit sums: the host route has no cap, and a segment may be 2^32 - 1 bytes long
        na = (uint32_t)(((uint64_t)shift + h + l + 3u) >> 2);
        nfull = (uint32_t)(((uint64_t)h + l) >> 2);
        tail = (h + l) & 3u;
    }
    BKD_HD uint32_t dword(const Load& load, uint32_t k) const {
        return (k >= k_lo && k < na) ? load(a + 4u * (uint64_t)k, seg, len) : 0u;
    }
    // d[0..N) = dwords k0 .. k0 + N - 1, zero where the dword holds no byte of the segment
    template <int N>
    BKD_HD void dwords(const Load& load, uint32_t k0, uint32_t (&d)[N]) const {
        if (k0 >= k_lo && k0 + (uint32_t)N <= na) {
#if defined(__clang__)
#pragma unroll
#endif
            for (int i = 0; i < N; ++i) d[i] = load(a + 4u * (uint64_t)(k0 + (uint32_t)i), seg, len);
        } else {
#if defined(__clang__)
#pragma unroll
#endif
            for (int i = 0; i < N; ++i) d[i] = dword(load, k0 + (uint32_t)i);
        }
    }
    // Message word j of the segment, j <= nfull (the last one holds `tail` bytes when j == nfull).
    BKD_HD uint32_t word(const Load& load, uint32_t j) const {
        return funnel(dword(load, j), dword(load, j + 1u), shift);
    }
};

// The walker's state between blocks: the open segment and the bytes that wait for the next one.
template <class Segs, class Load>
struct Walker {
    Segs& segs;
    const Load& load;
    Words<Load> cur;
    bool have = false;   // cur is open and not yet finished
    uint32_t j = 0;      // the next word of cur
    uint32_t carry = 0;  // the pending message bytes, first in the word, zeros behind them
    uint32_t hb = 0;     // how many (0..3)
    BKD_HD Walker(Segs& s, const Load& l) : segs(s), load(l) {}

    BKD_HD bool advance() {
        const uint8_t* p;
        uint32_t l;
        if (!segs.next(p, l)) return false;
        cur.open(p, l, hb);
        j = 0;
        return true;
    }
    // Word 0 of a segment gets its first bytes from the carry.
    BKD_HD uint32_t merged(uint32_t x) {
        x = carry | (x & ~head_mask(cur.h));
        carry = 0u;
        hb = 0u;
        return x;
    }
    BKD_HD uint32_t whole_left() const { return have ? cur.nfull - j : 0u; }
    // The open segment has no whole word left: its last bytes wait for the next one; a segment that ends
    // inside the word it started in (j == 0) adds them to the bytes that waited already.
    BKD_HD void finish() {
        if (cur.tail) {
            uint32_t x = cur.word(load, j) & head_mask(cur.tail);
            if (j == 0u && cur.h) x = merged(x);
            carry = x;
            hb = cur.tail;
        }
        have = false;
    }
    // Leaves a segment that is used up and opens the next one, so that a block which starts where a
    // segment starts takes the whole-word path.
    BKD_HD void settle() {
        if (have && j == cur.nfull) finish();
        if (!have) have = advance();
    }

    // Sixteen whole words of the open segment (whole_left() >= 16) from d = its dwords j .. j + 16.
    BKD_HD void block(const uint32_t (&d)[17], uint32_t (&w)[16]) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int t = 0; t < 16; ++t) w[t] = funnel(d[t], d[t + 1], cur.shift);
        if (j == 0u && cur.h) w[0] = merged(w[0]);
        j += 16u;
    }

    // Fills w[T0, 16) with the next message words, as far as the message goes; words behind its end hold
    // anything (sha1::padded_word looks only at the message's bytes).
    template <int T0>
    BKD_HD void fill(uint32_t (&w)[16]) {
        uint32_t t = (uint32_t)T0;
        settle();
        // the whole words the open segment still has, from a position known at compile time
        const uint32_t c = whole_left() < 16u - T0 ? whole_left() : 16u - T0;
        if (c) {
            uint32_t d[17 - T0];
            cur.template dwords<17 - T0>(load, j, d);
#if defined(__clang__)
#pragma unroll
#endif
            for (int i = 0; i < 16 - T0; ++i) w[T0 + i] = funnel(d[i], d[i + 1], cur.shift);
            if (j == 0u && cur.h) w[T0] = merged(w[T0]);
            j += c;
            t += c;
        }
        // across the cuts, word by word
        while (t < 16u) {
            if (!have) {
                have = advance();
                if (!have) break;
            }
            if (j < cur.nfull) {
                uint32_t x = cur.word(load, j);
                if (j == 0u && cur.h) x = merged(x);
                put(w, t, x);
                ++t;
                ++j;
            } else {
                finish();
            }
        }
        if (t < 16u && hb) {  // the message ends inside this word
            put(w, t, carry);
            carry = 0u;
            hb = 0u;
        }
    }
};

// mac[5] = HMAC over pre[0..8) (the 32-byte frame header as big-endian words) followed by the `total`
// bytes of the non-empty segments segs.next(p, len) yields, in order. key: inner() / outer() as MacKey;
// the outer words are read only after the inner hash. total: the sum of the lengths, which the caller has
// added up before (the device: and checked against BKD_MAC_MAX_ENTRY).
template <class Key, class Segs, class Load>
BKD_HD void hmac(const Key& key, const uint32_t (&pre)[8], Segs& segs, uint64_t total, const Load& load,
                 uint32_t (&mac)[5]) {
    const uint64_t m = total + 32u;
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = sha1::hmac_inner_bits(m);
    uint32_t h[5];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 5; ++k) h[k] = key.inner()[k];
    Walker<Segs, Load> wk(segs, load);
    uint32_t w[16];
    {  // block 0: the header and the first 32 bytes of the stream
#if defined(__clang__)
#pragma unroll
#endif
        for (int t = 0; t < 8; ++t) w[t] = pre[t];
#if defined(__clang__)
#pragma unroll
#endif
        for (int t = 8; t < 16; ++t) w[t] = 0u;
        wk.template fill<8>(w);
        if (m < 64u) {
#if defined(__clang__)
#pragma unroll
#endif
            for (int t = 8; t < 16; ++t) w[t] = sha1::padded_word(w[t], 4u * t, m, padded, bits);
        }
        sha1::compress(h, w);
    }
    uint64_t pos = 64u;
    while (pos < padded) {
        wk.settle();
        if (wk.whole_left() >= 16u) {
            // whole blocks inside one segment: the contiguous kernel's loop, block k + 1's loads in flight
            // during block k's rounds. 64 message bytes lie in each, so none holds padding.
            uint32_t d[17];
            wk.cur.template dwords<17>(load, wk.j, d);
            for (;;) {
                wk.block(d, w);
                const bool more = wk.whole_left() >= 16u;
                if (more) wk.cur.template dwords<17>(load, wk.j, d);
                sha1::compress(h, w);
                pos += 64u;
                if (!more) break;
            }
            continue;
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (int t = 0; t < 16; ++t) w[t] = 0u;
        wk.template fill<0>(w);
        if (pos + 64u > m) {
#if defined(__clang__)
#pragma unroll
#endif
            for (int t = 0; t < 16; ++t) w[t] = sha1::padded_word(w[t], pos + 4u * t, m, padded, bits);
        }
        sha1::compress(h, w);
        pos += 64u;
    }
    sha1::hmac_outer(key.outer(), h, mac);
}

// The load primitive of the host: the dword at `at` from the bytes of [seg, seg + len) alone.
struct HostLoad {
    uint32_t operator()(const uint8_t* at, const uint8_t* seg, uint32_t len) const {
        uint32_t v = 0u;
        for (int b = 0; b < 4; ++b) {
            const uint8_t* q = at + b;
            if (q >= seg && q < seg + len) v |= (uint32_t)*q << (8 * b);
        }
        return v;
    }
};

}  // namespace macseg
}  // namespace bkd
