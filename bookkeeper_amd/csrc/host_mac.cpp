// Host HMAC-SHA1 for MAC ledgers (host_mac.hpp): portable C++ over mac_sha1.hpp.
#include "host_mac.hpp"

#include <string.h>

#include <algorithm>
#include <atomic>

#include "host_batch.hpp"
#include "mac_segments.hpp"
#include "mac_sha1.hpp"

namespace bkd {
namespace host {

namespace {

inline uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

inline void put_be64(uint8_t* p, uint64_t v) {
    put_be32(p, (uint32_t)(v >> 32));
    put_be32(p + 4, (uint32_t)v);
}

// Continues h over the message pre[0, pre_len) || p[0, len) and finishes it: padding with the bit
// length of prior_bytes + the message. Blocks that lie whole inside p are read in place; the others
// (the prefix's, the tail's, the padding's) are built in a zeroed 64-byte buffer from the message's own
// bytes and go through sha1::padded_word, as the device builds them in registers. Aligned: where its loop
// falls in a 64-byte line moves the CPU route by 13 %, and without this the linker decides.
__attribute__((aligned(64)))
void hash_message(uint32_t (&h)[5], const uint8_t* pre, uint64_t pre_len, const uint8_t* p, uint64_t len,
                  uint64_t prior_bytes) {
    const uint64_t m = pre_len + len;
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = (prior_bytes + m) * 8u;
    uint32_t w[16];
    for (uint64_t pos = 0; pos < padded; pos += 64u) {
        if (pos >= pre_len && pos + 64u <= m) {
            const uint8_t* q = p + (pos - pre_len);
            for (int t = 0; t < 16; ++t) w[t] = be32(q + 4 * t);
        } else {
            uint8_t buf[64] = {0};
            const uint64_t end = std::min(pos + 64u, m);
            if (pos < pre_len) memcpy(buf, pre + pos, (size_t)(std::min(end, pre_len) - pos));
            const uint64_t d0 = std::max(pos, pre_len);
            if (end > d0) memcpy(buf + (d0 - pos), p + (d0 - pre_len), (size_t)(end - d0));
            for (int t = 0; t < 16; ++t) w[t] = sha1::padded_word(be32(buf + 4 * t), pos + 4u * t, m, padded, bits);
        }
        sha1::compress(h, w);
    }
}

// f(i) for i in [0, n), one entry per task from a shared counter over the host pool; small batches inline.
template <class F>
void each_entry(uint64_t n, const uint32_t* lens, F&& f) {
    if (n == 0) return;
    Pool& pool = Pool::get();
    const int threads = pool.active();
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n && bytes < (1u << 16); ++i) bytes += lens[i] + 64u;
    if (threads == 1 || n == 1 || bytes < (1u << 16)) {
        for (uint64_t i = 0; i < n; ++i) f(i);
        return;
    }
    std::atomic<uint64_t> next{0};
    pool.run((int)std::min<uint64_t>((uint64_t)threads, n), [&](int) {
        for (;;) {
            const uint64_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n) return;
            f(i);
        }
    });
}

}  // namespace

void mac_gen_digest(const char* pad, const uint8_t* passwd, uint64_t passwd_len, uint8_t* out20) {
    uint32_t h[5];
    for (int k = 0; k < 5; ++k) h[k] = sha1::kInit[k];
    hash_message(h, (const uint8_t*)pad, strlen(pad), passwd, passwd_len, 0);
    for (int k = 0; k < 5; ++k) put_be32(out20 + 4 * k, h[k]);
}

void mac_key_state(const uint8_t* key, size_t key_len, uint32_t* key_state10) {
    uint8_t block[64] = {0};
    memcpy(block, key, std::min<size_t>(key_len, 64));
    for (int half = 0; half < 2; ++half) {
        const uint8_t x = half == 0 ? 0x36 : 0x5C;  // ipad, opad
        uint32_t w[16], h[5];
        for (int t = 0; t < 16; ++t) w[t] = be32(block + 4 * t) ^ (0x01010101u * x);
        for (int k = 0; k < 5; ++k) h[k] = sha1::kInit[k];
        sha1::compress(h, w);
        for (int k = 0; k < 5; ++k) key_state10[5 * half + k] = h[k];
    }
}

void mac_key_init(const uint8_t* passwd, uint64_t passwd_len, uint32_t* key_state10) {
    uint8_t key[20];
    mac_gen_digest("mac", passwd, passwd_len, key);
    mac_key_state(key, sizeof(key), key_state10);
}

void mac_one(const uint32_t* key_state, const uint8_t* pre, uint32_t pre_len, const uint8_t* p, uint64_t len,
             uint8_t* out20) {
    uint32_t inner[5], mac[5];
    for (int k = 0; k < 5; ++k) inner[k] = key_state[k];
    hash_message(inner, pre, pre_len, p, len, 64);
    sha1::hmac_outer(key_state + 5, inner, mac);
    for (int k = 0; k < 5; ++k) put_be32(out20 + 4 * k, mac[k]);
}

void mac_list(const uint32_t* key_state, const uint8_t* const* ptrs, const uint32_t* lens, uint64_t n, uint8_t* out) {
    each_entry(n, lens, [&](uint64_t i) { mac_one(key_state, nullptr, 0, ptrs[i], lens[i], out + i * kMacLen); });
}

// DigestManager.verifyDigest for one MAC frame (DigestManager.java:226-283): too short, digest, ledger
// id, entry id (unless skipped), in that order.
static int32_t mac_verify_one(const uint32_t* key_state, const uint8_t* f, uint32_t l, int64_t ledger_id, int64_t entry_id,
                              bool skip_entry_id) {
    if (l < kMacFrameHead) return 1;
    uint8_t mac[kMacLen];
    mac_one(key_state, f, 32, f + kMacFrameHead, l - kMacFrameHead, mac);
    const int64_t lid = (int64_t)(((uint64_t)be32(f) << 32) | be32(f + 4));
    const int64_t eid = (int64_t)(((uint64_t)be32(f + 8) << 32) | be32(f + 12));
    if (memcmp(mac, f + 32, kMacLen) != 0) return 2;
    if (lid != ledger_id) return 3;
    return (!skip_entry_id && eid != entry_id) ? 4 : 0;
}

inline void put_header(uint8_t* f, int64_t ledger_id, int64_t entry_id, int64_t lac, int64_t length_field) {
    put_be64(f, (uint64_t)ledger_id);
    put_be64(f + 8, (uint64_t)entry_id);
    put_be64(f + 16, (uint64_t)lac);
    put_be64(f + 24, (uint64_t)length_field);
}

// The header and the MAC of one entry into f (DigestManager.java:146-155, 172-178): 52 bytes.
static void mac_package_one(const uint32_t* key_state, int64_t ledger_id, int64_t entry_id, int64_t lac, int64_t length_field,
                            const uint8_t* payload, uint32_t len, uint8_t* f) {
    put_header(f, ledger_id, entry_id, lac, length_field);
    mac_one(key_state, f, 32, payload, len, f + 32);
}

uint64_t mac_verify_frames(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id, int id_checks,
                           const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status) {
    each_entry(n, lens, [&](uint64_t i) {
        status[i] = mac_verify_one(key_state, frames[i], lens[i], ledger_id, first_entry_id + (int64_t)i, id_checks != 0);
    });
    for (uint64_t i = 0; i < n; ++i)
        if (status[i] != 0) return i;
    return n;
}

void mac_package_frames(const uint32_t* key_state, int64_t ledger_id, const int64_t* entry_ids, const int64_t* lacs,
                        const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                        uint64_t n, uint8_t* frames, uint64_t stride) {
    each_entry(n, lens, [&](uint64_t i) {
        mac_package_one(key_state, ledger_id, entry_ids[i], lacs[i], length_fields[i], payloads[i], lens[i],
                        frames + i * stride);
    });
}

void mac_verify_frames_expected(const uint32_t* key_states, const uint32_t* req_keys, const int64_t* ledger_ids,
                                const int64_t* entry_ids, const uint32_t* req_of, const uint8_t* const* frames,
                                const uint32_t* lens, uint64_t n, int32_t* status) {
    each_entry(n, lens, [&](uint64_t i) {
        const uint32_t* key = key_states + (uint64_t)req_keys[req_of[i] & ~kSkipEntryId] * 10u;
        status[i] = mac_verify_one(key, frames[i], lens[i], ledger_ids[i], entry_ids[i], (req_of[i] & kSkipEntryId) != 0);
    });
}

void mac_package_frames_ledgers(const uint32_t* key_states, const uint32_t* key_of, const int64_t* ledger_ids,
                                const int64_t* entry_ids, const int64_t* lacs, const int64_t* length_fields,
                                const uint8_t* const* payloads, const uint32_t* lens, uint64_t n, uint8_t* frames,
                                uint64_t stride) {
    each_entry(n, lens, [&](uint64_t i) {
        mac_package_one(key_states + (uint64_t)key_of[i] * 10u, ledger_ids[i], entry_ids[i], lacs[i], length_fields[i],
                        payloads[i], lens[i], frames + i * stride);
    });
}

// ---- re-framing with a new LAC ----

namespace {

// Block `pos` of the padded message pre[0, 32) || p[0, len) as hash_message builds it: read in place where
// it lies whole inside p, else put together from the message's own bytes and padded. (hash_message keeps
// its own loop: how it falls in a cache line is measured, see above, and the package and verify routes are
// to stay the machine code they were.)
inline void frame_block(uint32_t (&w)[16], const uint8_t* pre, const uint8_t* p, uint64_t pos, uint64_t m,
                        uint64_t padded, uint64_t bits) {
    if (pos >= 32u && pos + 64u <= m) {
        const uint8_t* q = p + (pos - 32u);
        for (int t = 0; t < 16; ++t) w[t] = be32(q + 4 * t);
        return;
    }
    uint8_t buf[64] = {0};
    const uint64_t end = std::min(pos + 64u, m);
    if (pos < 32u) memcpy(buf, pre + pos, (size_t)(std::min<uint64_t>(end, 32u) - pos));
    const uint64_t d0 = std::max<uint64_t>(pos, 32u);
    if (end > d0) memcpy(buf + (d0 - pos), p + (d0 - 32u), (size_t)(end - d0));
    for (int t = 0; t < 16; ++t) w[t] = sha1::padded_word(be32(buf + 4 * t), pos + 4u * t, m, padded, bits);
}

// mac_v / mac_n = HMAC over pre_v / pre_n (32 bytes each) || p[0, len): block 0 per header, every later
// block expanded once for both chains (sha1::compress2), as the device's mac_entry2.
void mac_two_headers(const uint32_t* key_state, const uint8_t* pre_v, const uint8_t* pre_n, const uint8_t* p,
                     uint64_t len, uint8_t* mac_v, uint8_t* mac_n) {
    const uint64_t m = 32u + len;
    const uint64_t padded = sha1::padded_bytes(m);
    const uint64_t bits = sha1::hmac_inner_bits(m);
    uint32_t hv[5], hn[5], w[16], ov[5], on[5];
    for (int k = 0; k < 5; ++k) hv[k] = hn[k] = key_state[k];
    frame_block(w, pre_v, p, 0, m, padded, bits);
    sha1::compress(hv, w);
    frame_block(w, pre_n, p, 0, m, padded, bits);
    sha1::compress(hn, w);
    for (uint64_t pos = 64u; pos < padded; pos += 64u) {
        frame_block(w, pre_v, p, pos, m, padded, bits);
        sha1::compress2(hv, hn, w);
    }
    sha1::hmac_outer(key_state + 5, hv, ov);
    sha1::hmac_outer(key_state + 5, hn, on);
    for (int k = 0; k < 5; ++k) {
        put_be32(mac_v + 4 * k, ov[k]);
        put_be32(mac_n + 4 * k, on[k]);
    }
}

// One frame, as the device's mac_reframe_kernel: the status of mac_verify_one (trusted: what the header
// alone decides, never 2), bytes 16..23 and 32..51 rewritten where it is 0.
int32_t mac_reframe_one(const uint32_t* key_state, uint8_t* f, uint32_t l, int64_t ledger_id, int64_t entry_id,
                        bool skip_entry_id, bool trusted, int64_t new_lac) {
    if (l < kMacFrameHead) return 1;
    uint8_t hdr[32], mac_v[kMacLen], mac_n[kMacLen];
    memcpy(hdr, f, 32);
    put_be64(hdr + 16, (uint64_t)new_lac);
    const int64_t lid = (int64_t)(((uint64_t)be32(f) << 32) | be32(f + 4));
    const int64_t eid = (int64_t)(((uint64_t)be32(f + 8) << 32) | be32(f + 12));
    if (trusted) {
        mac_one(key_state, hdr, 32, f + kMacFrameHead, l - kMacFrameHead, mac_n);
    } else {
        mac_two_headers(key_state, f, hdr, f + kMacFrameHead, l - kMacFrameHead, mac_v, mac_n);
        if (memcmp(mac_v, f + 32, kMacLen) != 0) return 2;
    }
    if (lid != ledger_id) return 3;
    if (!skip_entry_id && eid != entry_id) return 4;
    memcpy(f + 16, hdr + 16, 8);
    memcpy(f + 32, mac_n, kMacLen);
    return 0;
}

}  // namespace

void mac_reframe_frames_expected(const uint32_t* key_states, const uint32_t* req_keys, const int64_t* ledger_ids,
                                 const int64_t* entry_ids, const uint32_t* req_of, bool trusted, uint8_t* const* frames,
                                 const uint32_t* lens, uint64_t n, const int64_t* new_lacs, int32_t* status) {
    each_entry(n, lens, [&](uint64_t i) {
        const uint32_t* key = key_states + (uint64_t)req_keys[req_of[i] & ~kSkipEntryId] * 10u;
        status[i] = mac_reframe_one(key, frames[i], lens[i], ledger_ids[i], entry_ids[i], (req_of[i] & kSkipEntryId) != 0,
                                    trusted, new_lacs[i]);
    });
}

void mac_apply_reframe(uint8_t* const* frames, uint64_t n, const uint8_t* out_frames, const int32_t* status) {
    for (uint64_t i = 0; i < n; ++i) {
        if (status[i] != 0) continue;
        const uint8_t* o = out_frames + i * kMacFrameHead;
        memcpy(frames[i] + 16, o + 16, 8);
        memcpy(frames[i] + 32, o + 32, kMacLen);
    }
}

// ---- composite entries and V2 add requests ----

namespace {

struct HostKey {
    const uint32_t* s;
    const uint32_t* inner() const { return s; }
    const uint32_t* outer() const { return s + 5; }
};

// The non-empty segments [k, k1) in order, for the walker.
struct HostCursor {
    const uint8_t* const* ptrs;
    const uint32_t* lens;
    uint64_t k, k1;
    bool next(const uint8_t*& p, uint32_t& len) {
        for (; k < k1; ++k)
            if (lens[k]) {
                p = ptrs[k];
                len = lens[k];
                ++k;
                return true;
            }
        return false;
    }
};

inline void put_v2_prefix(uint8_t* r, uint32_t len, const MacV2Head& head, uint64_t i) {
    put_be32(r, kMacV2Head - 4u + len);  // Java int arithmetic
    put_be32(r + 4, head.packet_header);
    memcpy(r + 8, head.keys + i * head.key_stride, 20);
}

}  // namespace

void mac_one_segments(const uint32_t* key_state, const uint8_t* pre32, const uint8_t* const* seg_ptrs,
                      const uint32_t* seg_lens, uint64_t k0, uint64_t k1, uint8_t* out20) {
    uint64_t total = 0;
    for (uint64_t k = k0; k < k1; ++k) total += seg_lens[k];
    uint32_t pre[8], mac[5];
    for (int t = 0; t < 8; ++t) pre[t] = be32(pre32 + 4 * t);
    HostCursor segs{seg_ptrs, seg_lens, k0, k1};
    macseg::hmac(HostKey{key_state}, pre, segs, total, macseg::HostLoad{}, mac);
    for (int k = 0; k < 5; ++k) put_be32(out20 + 4 * k, mac[k]);
}

void mac_package_frames_segments(const uint32_t* key_states, const uint32_t* key_of, int64_t ledger_id,
                                 const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                                 const int64_t* length_fields, const uint8_t* const* seg_ptrs, const uint32_t* seg_lens,
                                 const uint64_t* seg_first, const uint32_t* entry_lens, uint64_t n, uint8_t* frames,
                                 uint64_t stride) {
    each_entry(n, entry_lens, [&](uint64_t i) {
        uint8_t* f = frames + i * stride;
        put_header(f, ledger_ids ? ledger_ids[i] : ledger_id, entry_ids[i], lacs[i], length_fields[i]);
        mac_one_segments(key_states + (uint64_t)(key_of ? key_of[i] : 0u) * 10u, f, seg_ptrs, seg_lens, seg_first[i],
                         seg_first[i + 1], f + 32);
    });
}

void mac_package_requests_v2(const uint32_t* key_states, const uint32_t* key_of, int64_t ledger_id,
                             const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                             const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                             uint64_t n, const MacV2Head& head, uint8_t* const* requests) {
    each_entry(n, lens, [&](uint64_t i) {
        uint8_t* r = requests[i];
        put_v2_prefix(r, lens[i], head, i);
        mac_package_one(key_states + (uint64_t)(key_of ? key_of[i] : 0u) * 10u, ledger_ids ? ledger_ids[i] : ledger_id,
                        entry_ids[i], lacs[i], length_fields[i], payloads[i], lens[i], r + 28);
        // copied while the hash has it in the cache (isSmallEntry, DigestManager.java:128, 160-163)
        if (lens[i] && lens[i] < head.small) memcpy(r + kMacV2Head, payloads[i], lens[i]);
    });
}

void mac_finish_requests_v2(const uint8_t* frames, const uint8_t* const* payloads, const uint32_t* lens, uint64_t n,
                            const MacV2Head& head, uint64_t first, uint8_t* const* requests) {
    each_entry(n, lens, [&](uint64_t i) {
        uint8_t* r = requests[i];
        put_v2_prefix(r, lens[i], head, first + i);
        memcpy(r + 28, frames + i * kMacFrameHead, kMacFrameHead);
        if (lens[i] && lens[i] < head.small) memcpy(r + kMacV2Head, payloads[i], lens[i]);
    });
}

}  // namespace host
}  // namespace bkd
