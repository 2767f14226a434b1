// The host side of the MAC digest type (MacDigestManager: HMAC-SHA1 keyed with SHA1("mac" || passwd),
// $BK/proto/checksum/MacDigestManager.java:46-107): key setup, the per-call MAC, and the CPU route of
// the host-resident MAC batches (one entry per task over the library's host pool, host_batch.hpp).
// Portable C++ over mac_sha1.hpp, the arithmetic the device kernels share.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bkd {
namespace host {

constexpr uint32_t kMacLen = 20;           // MacDigestManager.getMacCodeLength
constexpr uint32_t kMacFrameHead = 32 + kMacLen;  // [32 B header][20 B mac]

// out20 = SHA1(pad || passwd) (MacDigestManager.genDigest, :79-84); pad is a C string.
void mac_gen_digest(const char* pad, const uint8_t* passwd, uint64_t passwd_len, uint8_t* out20);
// key_state[0..4] / [5..9] = the SHA-1 states after compressing key ^ ipad / key ^ opad for an HMAC key
// of at most 64 bytes; mac_key_init: key = SHA1("mac" || passwd) (:61).
void mac_key_state(const uint8_t* key, size_t key_len, uint32_t* key_state10);
void mac_key_init(const uint8_t* passwd, uint64_t passwd_len, uint32_t* key_state10);
// out20 = HMAC over pre[0, pre_len) || p[0, len) (pre_len <= 64; the frame header, or nothing). No
// byte at or past p + len is read.
void mac_one(const uint32_t* key_state, const uint8_t* pre, uint32_t pre_len, const uint8_t* p, uint64_t len,
             uint8_t* out20);
// out + 20 i = HMAC(entry i), entry i its own buffer.
void mac_list(const uint32_t* key_state, const uint8_t* const* ptrs, const uint32_t* lens, uint64_t n, uint8_t* out);
// DigestManager.verifyDigest per frame [32 B header][20 B mac][payload] (DigestManager.java:226-283);
// id_checks: 0 ledger + entry ids, 1 ledger id only. Returns the first failing index (n when none).
uint64_t mac_verify_frames(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id, int id_checks,
                           const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status);
// The 32-byte BE header and the MAC of entry i into frames + i * stride (DigestManager.java:146-155,
// 172-178); no other byte of the stride is written.
void mac_package_frames(const uint32_t* key_state, int64_t ledger_id, const int64_t* entry_ids, const int64_t* lacs,
                        const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                        uint64_t n, uint8_t* frames, uint64_t stride);
// Batches that span ledgers (bkd_digest_verify_requests_mac_host, bkd_digest_package_batch_ledgers_mac_host):
// key_states is a table of ten-word rows. Verify: frame i against ledger_ids[i] and entry_ids[i], keyed
// with row req_keys[r] for its request r = req_of[i] & ~kSkipEntryId (host_batch.hpp; the bit skips the
// entry-id check), as verify_frames_expected. Package: entry i framed for ledger_ids[i] and keyed with row
// key_of[i], as package_frames_ledgers. Every index is the caller's to check against the table's rows.
void mac_verify_frames_expected(const uint32_t* key_states, const uint32_t* req_keys, const int64_t* ledger_ids,
                                const int64_t* entry_ids, const uint32_t* req_of, const uint8_t* const* frames,
                                const uint32_t* lens, uint64_t n, int32_t* status);
void mac_package_frames_ledgers(const uint32_t* key_states, const uint32_t* key_of, const int64_t* ledger_ids,
                                const int64_t* entry_ids, const int64_t* lacs, const int64_t* length_fields,
                                const uint8_t* const* payloads, const uint32_t* lens, uint64_t n, uint8_t* frames,
                                uint64_t stride);

// Re-framing with a new LAC (bkd_digest_reframe_requests_mac_host): frame i, a writable buffer, checked as
// mac_verify_frames_expected checks it and, where its status is 0, rewritten in place for new_lacs[i]: header
// bytes 16..23 and the MAC at 32..51. One pass over the payload: every block behind the first is expanded
// once and compressed into both chains (sha1::compress2). trusted: one chain under the new header, the
// status what the header alone decides (never 2) — the MAC is valid for the bytes as they lie.
void mac_reframe_frames_expected(const uint32_t* key_states, const uint32_t* req_keys, const int64_t* ledger_ids,
                                 const int64_t* entry_ids, const uint32_t* req_of, bool trusted, uint8_t* const* frames,
                                 const uint32_t* lens, uint64_t n, const int64_t* new_lacs, int32_t* status);
// The GPU route's last step: bytes 16..23 and 32..51 of the packed 52-byte out-frame i into frames[i],
// where status[i] is 0.
void mac_apply_reframe(uint8_t* const* frames, uint64_t n, const uint8_t* out_frames, const int32_t* status);

// Composite entries and V2 add requests (bkd_digest_package_batch_segments_mac_host,
// bkd_digest_package_batch_v2_mac_host). key_of (may be null: row 0 for all) and ledger_ids (may be null:
// ledger_id for all) as above.
// out20 = HMAC over pre[0, 32) || the non-empty segments ptrs[k], k in [k0, k1), in order: the segment
// walker the device kernel runs (mac_segments.hpp) over the segments' own bytes, nothing joined. No byte
// outside a segment is read.
void mac_one_segments(const uint32_t* key_state, const uint8_t* pre32, const uint8_t* const* seg_ptrs,
                      const uint32_t* seg_lens, uint64_t k0, uint64_t k1, uint8_t* out20);
// Entry i = segments seg_first[i] .. seg_first[i + 1] - 1, each its own host buffer; entry_lens[i] its
// bytes (saturated at 2^32 - 1: only the work is split by it). Frames as mac_package_frames_ledgers.
void mac_package_frames_segments(const uint32_t* key_states, const uint32_t* key_of, int64_t ledger_id,
                                 const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                                 const int64_t* length_fields, const uint8_t* const* seg_ptrs, const uint32_t* seg_lens,
                                 const uint64_t* seg_first, const uint32_t* entry_lens, uint64_t n, uint8_t* frames,
                                 uint64_t stride);
// Request i into requests[i]: [int32 BE 76 + len][int32 BE packet header][20 B key][32 B header][20 B mac]
// and the payload behind it when it is shorter than `small`, copied right after it is hashed. keys: entry
// i's 20-byte master key at keys + i * key_stride.
struct MacV2Head {
    const uint8_t* keys;
    uint64_t key_stride;
    uint32_t packet_header;
    uint32_t small;
};
constexpr uint32_t kMacV2Head = 28 + kMacFrameHead;  // 80 bytes in front of the payload
void mac_package_requests_v2(const uint32_t* key_states, const uint32_t* key_of, int64_t ledger_id,
                             const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                             const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                             uint64_t n, const MacV2Head& head, uint8_t* const* requests);
// The GPU route's last step for entries [first, first + n) (the arrays start at entry `first`, the keys at
// entry 0): the prefix, frame i of the packed 52-byte frames the device returned, and the small payloads
// from their sources.
void mac_finish_requests_v2(const uint8_t* frames, const uint8_t* const* payloads, const uint32_t* lens, uint64_t n,
                            const MacV2Head& head, uint64_t first, uint8_t* const* requests);

}  // namespace host
}  // namespace bkd
