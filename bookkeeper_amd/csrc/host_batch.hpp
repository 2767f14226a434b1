// Host-side batch machinery of libbkdigest.so (host_batch.cpp, plain C++):
//  * Pool — the library's host worker threads: the copies into pinned staging of the GPU route, and
//    the CPU route of host-resident batches;
//  * the CPU route of host-resident batches: one CRC / DigestManager verify / package per entry over
//    the pool, with host_crc.cpp's folding. BookKeeper holds these entries in host memory
//    (BatchedReadOp's ByteBufList, $BK/client/BatchedReadOp.java:164-190; PendingAddOp's payloads,
//    $BK/client/PendingAddOp.java:261), where the reference verifies them one crc32c() call at a time
//    ($CN/cpp/crc32c_sse42.cpp:184-217); a PCIe round trip through the GPU only pays where a core
//    cannot keep pace with the link (the measured crossover).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace bkd {
namespace host {

// Cores this process may run on: the affinity mask, capped by a cgroup v2 cpu.max quota (a quota
// of Q cores makes more than Q threads time-slice, not run in parallel).
int usable_cores();

class Pool {
  public:
    static Pool& get();
    // Runs f(part) for part = 0..parts-1 on up to threads() threads (part 0 on the calling thread)
    // and waits for all. One job at a time: a caller that finds the pool busy runs its parts itself.
    void run(int parts, const std::function<void(int)>& f);
    int threads() const;         // the pool's width: BKD_HOST_THREADS, else usable_cores()
    int active() const;          // threads a job may use (bkd_set_host_threads; <= threads())
    void set_active(int n);      // 0 = threads()
    ~Pool();

  private:
    Pool();
    void loop(int part);
    std::vector<std::thread> workers_;
    std::mutex mu_, call_mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    int parts_ = 0, pending_ = 0;
    std::atomic<int> active_{0};  // set_active() may run while other threads submit work
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// Bytes of the digest after a frame's 32-byte header: CRC32C writes an int, CRC32 a long
// (CRC32CDigestManager.java:44-46, CRC32DigestManager.java:60-63).
inline uint32_t mac_len(int algo) { return algo == 0 ? 4u : 8u; }

// ---- the CPU route of host-resident batches (semantics of include/bkdigest.h) ----
// The register after folding p[0, len) onto reg; from 4 MiB on in 1 MiB pieces over the pool,
// joined with x^(8 * piece) (one long buffer uses every core, not one).
uint32_t fold(int algo, uint32_t reg, const uint8_t* p, uint64_t len);
// out[i] = resume(seed_i, entry i): entry i at ptrs[i] (list) or base + offsets[i] (indexed).
void crc_list(int algo, const uint8_t* const* ptrs, const uint32_t* lens, uint64_t n, const uint32_t* seeds,
              uint32_t seed_all, uint32_t* out);
void crc_indexed(int algo, const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, uint64_t n,
                 const uint32_t* seeds, uint32_t seed_all, uint32_t* out);
// DigestManager.verifyDigest per frame ($BK/proto/checksum/DigestManager.java:226-283); id_checks:
// 0 ledger + entry ids, 1 ledger id only. Returns the first failing index (n when all verified).
uint64_t verify_frames(int algo, int64_t ledger_id, int64_t first_entry_id, int id_checks,
                       const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status);
// The same with per-entry expectations (bkd_digest_verify_requests_host, its requests expanded by the
// caller): frame i against ledger_ids[i] and entry_ids[i]; req_of[i] bit 31 (kSkipEntryId) = the
// frame's request skips the entry-id check, the low bits its request (not read here).
constexpr uint32_t kSkipEntryId = 0x80000000u;
void verify_frames_expected(int algo, const int64_t* ledger_ids, const int64_t* entry_ids, const uint32_t* req_of,
                            const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status);
// DigestManager.computeDigestAndPackageForSending per entry (DigestManager.java:117-181): the 32-byte
// BE header and the digest into frames + i*stride, the digest value into digests[i].
void package_frames(int algo, int64_t ledger_id, const int64_t* entry_ids, const int64_t* lacs,
                    const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens, uint64_t n,
                    uint8_t* frames, uint64_t stride, uint32_t* digests);
// The same with ledger_ids[i] framing entry i (bkd_digest_package_batch_ledgers_host).
void package_frames_ledgers(int algo, const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                            const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                            uint64_t n, uint8_t* frames, uint64_t stride, uint32_t* digests);
// Composite payloads (bkd_digest_package_batch_segments_host, bkd_crc_batch_segments_host): entry i is
// the concatenation of segments seg_first[i] .. seg_first[i+1]-1, segment k its own buffer seg_ptrs[k]
// of seg_lens[k] bytes; the digest is chained over the non-empty ones (DigestManager.java:62-72,
// 380-392), no bytes are copied together. seg_first is a valid CSR (the caller checked it).
// entry_lens[i] = entry i's summed bytes, saturated at 2^32 - 1 (the caller has them from choosing the
// route). ledger_ids[i] frames entry i when it is not null, else ledger_id.
void package_frames_segments(int algo, int64_t ledger_id, const int64_t* ledger_ids, const int64_t* entry_ids,
                             const int64_t* lacs, const int64_t* length_fields, const uint8_t* const* seg_ptrs,
                             const uint32_t* seg_lens, const uint64_t* seg_first, const uint32_t* entry_lens,
                             uint64_t n, uint8_t* frames, uint64_t stride, uint32_t* digests);
// V2 add requests (bkd_digest_package_batch_v2_host; DigestManager.computeDigestAndPackageForSendingV2,
// DigestManager.java:126-167): request i = [int32 BE 56 + mac + lens[i]][int32 BE packet header]
// [20 B master key][32 B header][digest], then the payload when lens[i] < small (:128, :160-163).
// PacketHeader.toInt(CURRENT_PROTOCOL_VERSION = 2, ADDENTRY = 1, flags) ($BK/proto/BookieProtocol.java:47,
// 75-83, 114).
inline uint32_t v2_packet_header(uint32_t flags) { return (2u << 24) | (1u << 16) | (flags & 0xFFFFu); }
struct V2Head {
    const uint8_t* keys;   // entry i's 20-byte key at keys + i*key_stride (key_stride 0: one key for all)
    uint64_t key_stride;
    uint32_t packet_header;
    uint32_t small;        // payloads shorter than this are copied into the request
};
// The CPU route: package_frames' arithmetic per entry with the frame at requests[i] + 28, the prefix in
// front of it, and the payload copied in right after it was folded (ledger_ids as package_frames_segments).
void package_requests_v2(int algo, int64_t ledger_id, const int64_t* ledger_ids, const int64_t* entry_ids,
                         const int64_t* lacs, const int64_t* length_fields, const uint8_t* const* payloads,
                         const uint32_t* lens, uint64_t n, const V2Head& head, uint8_t* const* requests,
                         uint32_t* digests);
// The GPU route's last step for entries [first, first + n) (the arrays start at entry `first`, the keys
// at entry 0): the prefix, frame i of the packed [32 B header][digest] frames the device returned, and
// the small payloads from their sources, on at most `threads` pool threads.
void finish_requests_v2(int algo, const uint8_t* frames, const uint8_t* const* payloads, const uint32_t* lens,
                        uint64_t n, const V2Head& head, uint64_t first, uint8_t* const* requests, int threads);
// out[i] = resume(seed_i, entry i's segments in order).
void crc_segments(int algo, const uint8_t* const* seg_ptrs, const uint32_t* seg_lens, const uint64_t* seg_first,
                  const uint32_t* entry_lens, uint64_t n, const uint32_t* seeds, uint32_t seed_all, uint32_t* out);
// Re-frames verified frames in place with new LACs (LedgerFragmentReplicator.java:436-442): status as
// verify_frames (trusted: from the header alone, no payload byte read); a frame that is OK gets
// new_lacs[i] at bytes 16..23 and the digest old ^ R(LAC difference) * x^(8 * payload length); the
// others stay untouched with digests[i] = 0 (digests may be null). Returns the first failing index.
uint64_t reframe_frames(int algo, int64_t ledger_id, int64_t first_entry_id, int id_checks, bool trusted,
                        uint8_t* const* frames, const uint32_t* lens, uint64_t n, const int64_t* new_lacs,
                        uint32_t* digests, int32_t* status);
// The GPU route's last step: writes new_lacs[i] and digests[i] into every frame whose status is 0.
void apply_reframe(int algo, uint8_t* const* frames, uint64_t n, const int64_t* new_lacs, const int32_t* status,
                   const uint32_t* digests);

}  // namespace host
}  // namespace bkd
