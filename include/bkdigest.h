/*
 * bkdigest — MI355X-native ledger-entry digest engine (CRC32C / CRC32) for Apache BookKeeper.
 *
 * The drop-in boundary: a C-ABI shared library (bookkeeper_amd/libbkdigest.so) with plain
 * pointers and sizes. Every entry point names the reference interface it replaces
 * (paths relative to /root/reference; $CN = circe-checksum/src/main/circe,
 * $CJ = circe-checksum/src/main/java/com/scurrilous/circe,
 * $BK = bookkeeper-server/src/main/java/org/apache/bookkeeper).
 *
 * Semantics shared by every CRC entry point (identical to the reference):
 *   - `current` / seeds are FINALIZED CRCs: resume(prev, x) = ~raw(~prev, x)
 *     ($CN/cpp/crc32c_sse42.cpp:187,213; $CJ/crc/AbstractIntCrc.java:55-57);
 *   - calculate(x) == resume(0, x) ($CJ/checksum/JniIntHash.java:40-42);
 *   - a zero-length entry returns its seed unchanged ($CN/cpp/crc32c_sse42.cpp:211-213);
 *   - the value is the u32 bit pattern of the Java `int` the reference returns.
 * Algorithms: BKD_CRC32C = CRC-32C (Castagnoli, reflected 0x82F63B78, $CN/cpp/crc32c_sse42.cpp:85),
 *             BKD_CRC32  = CRC-32 (ISO-HDLC, reflected 0xEDB88320, java.util.zip.CRC32 as used by
 *                          $BK/proto/checksum/CRC32DigestManager.java:28-87).
 *
 * Errors are return codes only (the reference native never throws, circe-checksum/pom.xml:87);
 * a human-readable message for the calling thread is available from bkd_last_error().
 * All entry points are thread-safe. Device-resident batch calls are asynchronous on the
 * caller's HIP stream (hipStream_t passed as void*, NULL = the null stream) and run on that
 * stream's device (the calling thread's current device for the null stream); buffers are
 * borrowed only until the stream reaches the end of the call's work.
 * Device-resident batch entry points always run on the GPU (BKD_ERR_NO_DEVICE without one).
 * Host-resident batches (bkd_crc_batch_host, bkd_digest_*_batch_host) take the GPU through pinned
 * staging or the library's own threaded CPU route, by the measured crossover (bkd_set_host_batch_route).
 * The per-call host-buffer resumes (bkd_resume / bkd_resume_host) take the CPU route for
 * buffers up to bkd_get_cpu_route_max() bytes and whenever no device is visible, so the
 * provider never fails for lack of a GPU, as the reference's class-init selection never does
 * ($CJ/checksum/Crc32cIntChecksum.java:28-36).
 */
#ifndef BKDIGEST_H_
#define BKDIGEST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BKD_ABI_VERSION 6

/* only the entry points below are exported (the library is built with -fvisibility=hidden) */
#ifndef BKD_API
#define BKD_API __attribute__((visibility("default")))
#endif

/* return codes */
#define BKD_OK 0
#define BKD_ERR_INVALID_ARG (-1)
#define BKD_ERR_NO_DEVICE (-2)
#define BKD_ERR_HIP (-3)
#define BKD_ERR_BOUNDS (-4)
#define BKD_ERR_NOMEM (-5)

/* algorithms */
#define BKD_CRC32C 0
#define BKD_CRC32 1

/* verify status codes (one per entry), mirroring DigestManager.verifyDigest's failure modes
 * ($BK/proto/checksum/DigestManager.java:226-283) */
#define BKD_VERIFY_OK 0
#define BKD_VERIFY_TOO_SHORT 1      /* :229-235 (METADATA_LENGTH + macCodeLength) > readableBytes */
#define BKD_VERIFY_DIGEST_MISMATCH 2 /* :241-261 */
#define BKD_VERIFY_LEDGER_MISMATCH 3 /* :267-273 */
#define BKD_VERIFY_ENTRY_MISMATCH 4  /* :275-281 */

BKD_API int bkd_abi_version(void);

/* Number of visible HIP devices (0 when none). Replaces the capability probe
 * Sse42Crc32C.isSupported() -> nativeSupported() ($CJ/crc/Sse42Crc32C.java:31-47,
 * $CN/cpp/crc32c_sse42_jni.cpp:20-24). */
BKD_API int bkd_device_count(void);

/* Uploads the CRC fold tables to `device` (idempotent, thread-safe). Replaces the
 * allocConfig chunk/shift-table construction ($CN/cpp/crc32c_sse42_jni.cpp:50-72,
 * $CN/cpp/crc32c_sse42.cpp:74-90). Optional: every call below initialises lazily. */
BKD_API int bkd_init(int device);

/* Message describing the last failure on the calling thread ("" if none). */
BKD_API const char* bkd_last_error(void);

/* ---- device-resident batches: THE HOT PATH ---------------------------------------------
 * One CRC per entry, all entries in one launch. Entry i is the byte range
 *   uniform:  d_base + i*stride, entry_len bytes
 *   indexed:  d_base + d_offsets[i], d_lengths[i] bytes (any alignment, any order)
 * seeded with d_seeds[i] (finalized CRC) or, when d_seeds is NULL, with seed_all.
 * d_out[i] receives the finalized CRC. All pointers are device pointers of the current
 * HIP device. Replaces N calls of Sse42Crc32C.resume(int,long,long) -> nativeUnsafe
 * ($CJ/crc/Sse42Crc32C.java:105-107, $CN/cpp/crc32c_sse42_jni.cpp:44-48) which the
 * reference makes once per entry from DigestManager.update ($BK/proto/checksum/DigestManager.java:62-72).
 * The indexed form checks offset+length <= base_size for every entry on the device and returns
 * BKD_ERR_BOUNDS from the NEXT synchronous call on this stream if any entry was out of range
 * (those entries get out = 0 and are not read). */
BKD_API int bkd_crc_batch_uniform(int algo, const void* d_base, uint64_t stride, uint32_t entry_len, uint64_t n,
                          const uint32_t* d_seeds, uint32_t seed_all, uint32_t* d_out, void* stream);

BKD_API int bkd_crc_batch(int algo, const void* d_base, uint64_t base_size, const uint64_t* d_offsets,
                  const uint32_t* d_lengths, uint64_t n, const uint32_t* d_seeds, uint32_t seed_all,
                  uint32_t* d_out, void* stream);

/* Composite entries (a Netty CompositeByteBuf / ByteBufList visited leaf by leaf): entry i is the
 * concatenation, in order, of segments d_seg_first[i] .. d_seg_first[i+1]-1, segment k being the
 * byte range d_base + d_seg_offsets[k], d_seg_lengths[k] bytes; empty segments are skipped. out[i] =
 * resume(seed_i, concatenation) — the digest DigestManager.update chains over ByteBufVisitor's
 * leaves ($BK/proto/checksum/DigestManager.java:62-72,380-392, $BK/util/ByteBufVisitor.java:72-191),
 * without copying the pieces together. d_seg_first holds n + 1 non-decreasing indices
 * (d_seg_first[n] = nseg). Segments take the indexed path (bounds reported as for bkd_crc_batch);
 * one GF(2) combine per segment joins them. Device pointers; asynchronous on `stream`. */
BKD_API int bkd_crc_batch_segments(int algo, const void* d_base, uint64_t base_size, const uint64_t* d_seg_offsets,
                           const uint32_t* d_seg_lengths, uint64_t nseg, const uint64_t* d_seg_first, uint64_t n,
                           const uint32_t* d_seeds, uint32_t seed_all, uint32_t* d_out, void* stream);

/* Waits for `stream` and reports (BKD_ERR_BOUNDS) any bounds violation recorded by the indexed
 * batches enqueued on THIS stream since its previous bkd_stream_sync; the flag is per stream, so
 * concurrent callers on other streams neither see nor clear it. */
BKD_API int bkd_stream_sync(void* stream);

/* Waits for `stream`, then frees the scratch the library keeps for it (plan arena, bounds flag,
 * run words) and forgets the stream; returns BKD_ERR_BOUNDS as bkd_stream_sync would. Call it
 * before hipStreamDestroy on a stream that ran indexed batches, with no other call on that stream
 * in progress; a later call on the same handle starts afresh. The reference has no per-stream state
 * (its natives are stateless, $CN/cpp/crc32c_sse42_jni.cpp:26-48): this is the lifetime rule a
 * long-lived caller that creates and drops streams needs so that their scratch does not pile up. */
BKD_API int bkd_stream_release(void* stream);

/* ---- host-resident batches (the end-to-end path: Netty buffers in, digests out) -------
 * Synchronous. Same semantics as bkd_crc_batch (bounds checked on the host: BKD_ERR_BOUNDS before
 * any work). GPU route: the payload goes through pinned staging buffers with hipMemcpyAsync
 * (double-buffered H2D -> kernel -> D2H). CPU route: one fold per entry on the library's host
 * threads (host_batch.cpp). */
BKD_API int bkd_crc_batch_host(int algo, const void* h_base, uint64_t base_size, const uint64_t* h_offsets,
                       const uint32_t* h_lengths, uint64_t n, const uint32_t* h_seeds, uint32_t seed_all,
                       uint32_t* h_out);
/* Route of the host-resident batches: 0 = automatic (the CPU route when at least the measured
 * crossover's number of host threads is available: a batch that starts in host memory is bound by
 * PCIe and the host gather through the GPU; the CPU route also whenever no device is
 * visible), 1 = always the CPU route, 2 = always the GPU (BKD_ERR_NO_DEVICE without one).
 * get: the route the next host-resident batch takes (1 or 2). The reference verifies these entries
 * one crc32c() call at a time on its caller's thread ($BK/client/BatchedReadOp.java:164-190). */
BKD_API int bkd_set_host_batch_route(int route);
BKD_API int bkd_get_host_batch_route(void);
/* Host threads the CPU route and the staging copies may use (0 = all of the pool: BKD_HOST_THREADS,
 * else the cores this process may run on, capped by a cgroup CPU quota). */
BKD_API int bkd_set_host_threads(int threads);
BKD_API int bkd_get_host_threads(void);
/* Frees the idle pinned staging sets of the GPU route (host and device memory, streams); sets in use
 * by a running call are kept. A later host-resident batch through the GPU creates them again. */
BKD_API int bkd_host_release(void);

/* ---- per-call drop-in (IntHash.resume) ---------------------------------------------------
 * resume(current, ptr, len) for ONE buffer, synchronous. Replaces Sse42Crc32C.nativeUnsafe /
 * nativeArray / nativeDirectBuffer ($CN/cpp/crc32c_sse42_jni.cpp:26-48) and IntHash.resume
 * ($CJ/checksum/IntHash.java:28-32). len == 0 returns `current` (crc32c_sse42.cpp:211-213).
 *
 * bkd_resume_host: a host buffer. Up to bkd_get_cpu_route_max() bytes, or with no device, the
 *   CPU route (PCLMUL folding / SSE4.2 crc32, host_crc.cpp); above, the GPU through pinned staging
 *   (the CPU route again if the device fails: init, allocation or copy errors never surface here).
 * bkd_resume_device: a device buffer, on the caller's `stream` (ordered after the work that
 *   produced the bytes), synchronous. One launch per call: batch callers use bkd_crc_batch.
 * bkd_resume: either; the pointer kind is looked up (hipPointerGetAttributes), and a device
 *   buffer runs on the null stream of the device that holds it, which orders it after work on
 *   that device's blocking streams.
 * bkd_cpu_resume: always the CPU route (no device needed). */
BKD_API int bkd_resume(int algo, uint32_t current, const void* ptr, uint64_t len, uint32_t* out);
BKD_API int bkd_resume_host(int algo, uint32_t current, const void* h_ptr, uint64_t len, uint32_t* out);
BKD_API int bkd_resume_device(int algo, uint32_t current, const void* d_ptr, uint64_t len, void* stream,
                              uint32_t* out);
BKD_API int bkd_cpu_resume(int algo, uint32_t current, const void* h_ptr, uint64_t len, uint32_t* out);
/* Host buffers up to this many bytes take the CPU route in bkd_resume / bkd_resume_host
 * (0 = always the GPU when one is visible). Default by CPU, from profiles/r02_call_latency.log:
 * 64 MiB where the AVX-512 VPCLMULQDQ fold runs (a core keeps pace with PCIe), else 4 MiB. */
BKD_API int bkd_set_cpu_route_max(uint64_t bytes);
BKD_API uint64_t bkd_get_cpu_route_max(void);
/* The CPU route's implementation on this host: "vpclmul512+pclmul+sse4.2", "pclmul+sse4.2", "pclmul"
 * or "slice8". */
BKD_API const char* bkd_cpu_impl(void);

/* ---- circe-checksum compatibility (the Sse42Crc32C natives, $CN/cpp/crc32c_sse42_jni.cpp) -----
 * Backing for a drop-in libcirce-checksum.so (native/jni/bkdigest_jni.c). The chunk-word config
 * only tunes the reference's SSE4.2 loop; results never depend on it, so it is validated and
 * kept as an opaque handle. alloc: 0 unless len >= 1, every word >= 4 and the words strictly
 * decrease (:50-72); free: releases a non-zero handle (:74-78). supported: 1 (the library
 * always has a route: GPU or CPU), replacing nativeSupported (:20-24). */
BKD_API int bkd_circe_supported(void);
BKD_API int64_t bkd_circe_alloc_config(const int32_t* chunk_words, int32_t len);
BKD_API void bkd_circe_free_config(int64_t config);

/* ---- DigestManager batch framing (§8f rows 1-2) --------------------------------------
 * Package: for entry i with payload d_payload + d_offsets[i], d_lengths[i] bytes, write the
 * 32-byte big-endian header [ledger_id, entry_ids[i], lacs[i], lengths_field[i]]
 * ($BK/proto/checksum/DigestManager.java:146-149) followed by the digest
 * (CRC32C: 4 B BE int, CRC32CDigestManager.java:44-46; CRC32: 8 B BE long zero-extended,
 * CRC32DigestManager.java:60-63) into d_frames + i*frame_stride (frame_stride >= 32 + mac).
 * digest = update(update(0, header), payload) (DigestManager.java:152-153, :177-178).
 * Device pointers; asynchronous on `stream`. An out-of-range payload entry gets digest 0 and is
 * reported by the next bkd_stream_sync on `stream` (BKD_ERR_BOUNDS). */
BKD_API int bkd_digest_package_batch(int algo, int64_t ledger_id, const int64_t* d_entry_ids, const int64_t* d_lacs,
                             const int64_t* d_length_fields, const void* d_payload, uint64_t payload_size,
                             const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                             void* d_frames, uint64_t frame_stride, uint32_t* d_digests, void* stream);

/* Verify: entry i is a framed buffer [32 B header][mac][payload] at d_framed + d_offsets[i],
 * d_lengths[i] bytes. Writes a BKD_VERIFY_* code per entry to d_status and the index of the first
 * failing entry (n if none) to *d_first_bad — the verified-prefix rule of BatchedReadOp
 * ($BK/client/BatchedReadOp.java:164-190). expected entry id for entry i = first_entry_id + i
 * (DigestManager.verifyDigestAndReturnData(entryId, buf), :333-338); skip_entry_check mirrors
 * verifyDigest(buf) with skipEntryIdCheck (:206-208). Device pointers; asynchronous. */
BKD_API int bkd_digest_verify_batch(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                            const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                            const uint32_t* d_lengths, uint64_t n, int32_t* d_status, uint64_t* d_first_bad,
                            void* stream);

/* Host-resident framed batches (SURVEY §8f rows 1-2 with the entries in host memory, BASELINE
 * config 5): entry i is its own host buffer h_frames[i] / h_payloads[i] of h_lengths[i] bytes,
 * as BatchedReadOp's ByteBufList ($BK/client/BatchedReadOp.java:164-190) and PendingAddOp's
 * payloads ($BK/client/PendingAddOp.java:261) hold them. Route as bkd_crc_batch_host: GPU = the
 * library gathers them into pinned staging (segments of <= 64 MiB, double-buffered, host copies on
 * a thread pool), copies H2D, runs the device sequence of the device-resident call and copies the
 * results back; CPU = DigestManager's per-entry arithmetic on the host threads. Synchronous.
 * verify: h_status[i] and *h_first_bad as bkd_digest_verify_batch (n if all verified).
 * package: writes frame i's [32 B header][digest] to h_frames + i*frame_stride
 * (32 + mac <= frame_stride <= 4096) and the digest value to h_digests[i]. Only those 32 + mac bytes of a
 * frame's stride are written, on both routes. (Changed with the composite calls, for
 * bkd_digest_package_batch_host and bkd_digest_package_batch_ledgers_host too: the GPU route used to copy
 * whole strides back, so with frame_stride > 32 + mac it overwrote the bytes between frames with
 * unspecified values; it now leaves them to the caller, as the CPU route always did.) */
BKD_API int bkd_digest_verify_batch_host(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                                         const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                         int32_t* h_status, uint64_t* h_first_bad);
BKD_API int bkd_digest_package_batch_host(int algo, int64_t ledger_id, const int64_t* h_entry_ids,
                                          const int64_t* h_lacs, const int64_t* h_length_fields,
                                          const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                          void* h_frames, uint64_t frame_stride, uint32_t* h_digests);

/* ---- batches that span many ledgers (an aggregation queue across pending adds and reads) ----
 * The calls above are bound to one ledger: one BatchedReadOp ($BK/client/BatchedReadOp.java:164-190)
 * or one ledger's adds ($BK/client/PendingAddOp.java:261). A client that serves thousands of open
 * ledgers has a few reads or adds outstanding on each and can only form large batches ACROSS ledgers
 * (SURVEY.md §8f rank 2); these calls take such a batch whole, one launch sequence for all of it.
 *
 * Verify: entries are the framed buffers of bkd_digest_verify_batch, grouped into nreq read requests
 * in CSR form: request r owns entries [d_req_first[r], d_req_first[r+1]). d_req_first holds nreq + 1
 * non-decreasing values, d_req_first[0] == 0 and d_req_first[nreq] == n; empty requests are legal
 * anywhere. Entry i of request r is verified exactly as DigestManager.verifyDigest does
 * ($BK/proto/checksum/DigestManager.java:226-283) with ledger id d_req_ledger_ids[r] and expected entry
 * id d_req_first_entry_ids[r] + (i - d_req_first[r]); d_req_flags[r] bit 0 skips the entry-id check
 * (skipEntryIdCheck, DigestManager.java:206-208). d_status[i]: the BKD_VERIFY_* code, same precedence
 * (too short, digest, ledger, entry). d_req_first_bad[r]: the index WITHIN request r of its first
 * failing entry, or the request's entry count if none failed — BatchedReadOp's verified prefix, per
 * request. n == 0 writes zeros to d_req_first_bad. nreq < 2^31; nreq == 0 requires n == 0.
 * Device pointers; asynchronous on `stream`; no host synchronisation. A malformed CSR is detected on
 * the device: it raises the stream's bounds flag (BKD_ERR_BOUNDS from the next bkd_stream_sync), never
 * causes an access outside the caller's arrays, and leaves the outputs unspecified. */
#define BKD_REQUEST_SKIP_ENTRY_ID 1u /* d_req_flags bit 0 */
BKD_API int bkd_digest_verify_requests(int algo, const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                                       const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first,
                                       uint64_t nreq, const int64_t* d_req_ledger_ids,
                                       const int64_t* d_req_first_entry_ids, const uint32_t* d_req_flags,
                                       int32_t* d_status, uint64_t* d_req_first_bad, void* stream);
/* Package: bkd_digest_package_batch with d_ledger_ids[i] framing entry i in place of the one ledger_id
 * (DigestManager.java:146-149); routes, d_digests and bounds reporting are the same. */
BKD_API int bkd_digest_package_batch_ledgers(int algo, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                             const int64_t* d_lacs, const int64_t* d_length_fields,
                                             const void* d_payload, uint64_t payload_size, const uint64_t* d_offsets,
                                             const uint32_t* d_lengths, uint64_t n, void* d_frames,
                                             uint64_t frame_stride, uint32_t* d_digests, void* stream);
/* Host-resident forms: buffers as bkd_digest_verify_batch_host / bkd_digest_package_batch_host, the
 * request arrays / ledger ids in host memory; route by bkd_set_host_batch_route. The CSR is validated
 * before any work (BKD_ERR_INVALID_ARG). Synchronous. */
BKD_API int bkd_digest_verify_requests_host(int algo, const void* const* h_frames, const uint32_t* h_lengths,
                                            uint64_t n, const uint64_t* h_req_first, uint64_t nreq,
                                            const int64_t* h_req_ledger_ids, const int64_t* h_req_first_entry_ids,
                                            const uint32_t* h_req_flags, int32_t* h_status,
                                            uint64_t* h_req_first_bad);
BKD_API int bkd_digest_package_batch_ledgers_host(int algo, const int64_t* h_ledger_ids, const int64_t* h_entry_ids,
                                                  const int64_t* h_lacs, const int64_t* h_length_fields,
                                                  const void* const* h_payloads, const uint32_t* h_lengths,
                                                  uint64_t n, void* h_frames, uint64_t frame_stride,
                                                  uint32_t* h_digests);

/* ---- packaging composite payloads (a CompositeByteBuf add, digested leaf by leaf) -------------
 * The add path hands DigestManager.computeDigestAndPackageForSending a composite payload — a Pulsar
 * add is a CompositeByteBuf of a command/metadata buffer and the message payload — and the reference
 * digests it leaf by leaf through ByteBufVisitor without copying the leaves together
 * ($BK/proto/checksum/DigestManager.java:62-72, 126-181, 380-392; $BK/util/ByteBufVisitor.java:72-191).
 * These calls take a batch of such adds whole, of one ledger or of many.
 *
 * Entry i's payload is the concatenation, in order, of segments seg_first[i] .. seg_first[i+1]-1
 * (seg_first: n + 1 values from 0 to nseg, never decreasing). Empty segments are skipped, as the
 * visitor skips empty leaves; an entry with no segments or only empty ones has an empty payload.
 * Segments may be unaligned, in any order, overlapping, and shared between entries.
 * Frame i = [32 B BE header: ledger id, entry_ids[i], lacs[i], length_fields[i]][digest] at
 * frames + i*frame_stride (frame_stride >= 32 + mac; bytes of the stride past 32 + mac are not
 * written), the ledger id being ledger_ids[i] or, when ledger_ids is NULL, ledger_id for all.
 * digest = update(update(0, header), payload) (DigestManager.java:146-153, 172-178), written as
 * bkd_digest_package_batch writes it, its value also to digests[i]. length_fields[i] is the caller's
 * value as in bkd_digest_package_batch: it is not derived from the segments.
 *
 * Device-resident: segment k is d_payload + d_seg_offsets[k], d_seg_lengths[k] bytes. Asynchronous on
 * `stream`, no host synchronisation; every payload byte is read once and none is copied (the segments
 * take the indexed path; one kernel folds each header and joins its entry's segments in GF(2)). No
 * byte of a frame may overlap a byte of a segment (the result is undefined otherwise); frames in front
 * of their payloads inside d_payload are legal. A segment with offset + length > payload_size is not
 * read and raises the stream's bounds flag (BKD_ERR_BOUNDS from the next bkd_stream_sync): that
 * entry's digest is unspecified, its header is still written, every other entry is exact. A malformed
 * d_seg_first (a decrease, a value past nseg, a first value that is not 0, a last that is not nseg) is
 * clamped so that nothing outside the caller's arrays is read; it raises the same flag and leaves the
 * outputs unspecified. n == 0 launches nothing; nseg == 0 with n > 0 is legal (all payloads empty).
 * Short segments: the indexed path's short-entry launch loads whole 16-byte blocks for entries under
 * 16 bytes, which at the very end of a buffer lie past it (bkd_crc_batch and bkd_crc_batch_segments have
 * that property). This call does not: a segment shorter than 16 bytes, an empty one included, is never
 * handed to that launch; the join kernel reads its own bytes and no others. An empty segment at
 * offset == payload_size (an empty leaf at the writer index) and a short segment that ends on the
 * payload's last byte are as legal as any. */
BKD_API int bkd_digest_package_batch_segments(int algo, int64_t ledger_id, const int64_t* d_ledger_ids,
                                              const int64_t* d_entry_ids, const int64_t* d_lacs,
                                              const int64_t* d_length_fields, const void* d_payload,
                                              uint64_t payload_size, const uint64_t* d_seg_offsets,
                                              const uint32_t* d_seg_lengths, uint64_t nseg,
                                              const uint64_t* d_seg_first, uint64_t n, void* d_frames,
                                              uint64_t frame_stride, uint32_t* d_digests, void* stream);
/* Host-resident: segment k is its own host buffer h_seg_ptrs[k] of h_seg_lengths[k] bytes — each
 * CompositeByteBuf component's memoryAddress() and readableBytes(). Synchronous. The CSR is validated
 * before any work (BKD_ERR_INVALID_ARG). Route as bkd_digest_package_batch_host
 * (bkd_set_host_batch_route): CPU = the header's register, then the fold chained over the entry's
 * non-empty segments, on the host threads, nothing copied together; GPU = an entry's segments laid end
 * to end in pinned staging, then the device sequence of bkd_digest_package_batch. An entry whose
 * segments sum to more than a staging segment (64 MiB) takes the CPU route, or returns
 * BKD_ERR_INVALID_ARG when the GPU route is forced. 32 + mac <= frame_stride <= 4096. Short and empty
 * segments are legal anywhere here too: the CPU route reads a segment's own bytes only, and the GPU
 * route's staging buffer is allocated with room for the last 16-byte block. */
BKD_API int bkd_digest_package_batch_segments_host(int algo, int64_t ledger_id, const int64_t* h_ledger_ids,
                                                   const int64_t* h_entry_ids, const int64_t* h_lacs,
                                                   const int64_t* h_length_fields, const void* const* h_seg_ptrs,
                                                   const uint32_t* h_seg_lengths, uint64_t nseg,
                                                   const uint64_t* h_seg_first, uint64_t n, void* h_frames,
                                                   uint64_t frame_stride, uint32_t* h_digests);
/* bkd_crc_batch_segments for segments in host memory: h_out[i] = resume(seed_i, the concatenation of
 * entry i's segments) (DigestManager.java:62-72, 380-392). Segments, CSR validation and routes as
 * bkd_digest_package_batch_segments_host (GPU: the staged entries through the indexed path). */
BKD_API int bkd_crc_batch_segments_host(int algo, const void* const* h_seg_ptrs, const uint32_t* h_seg_lengths,
                                        uint64_t nseg, const uint64_t* h_seg_first, uint64_t n,
                                        const uint32_t* h_seeds, uint32_t seed_all, uint32_t* h_out);

/* ---- V2 add requests, packaged whole (the wire protocol Pulsar's brokers set) -----------------
 * With useV2Protocol, computeDigestAndPackageForSending does not return [header][digest] beside the
 * payload but one request buffer ($BK/proto/checksum/DigestManager.java:126-167):
 *   [int32 BE  headersSize + payloadSize]   headersSize = 4 + 20 + 32 + mac (:130-134, :138)
 *   [int32 BE  PacketHeader.toInt(CURRENT_PROTOCOL_VERSION = 2, ADDENTRY = 1, flags)]
 *                                           (:139-141; $BK/proto/BookieProtocol.java:47, 75-83, 114)
 *   [20 B      master key]                  (:142; MASTER_KEY_LENGTH, BookieProtocol.java:65)
 *   [32 B      ledger id, entry id, LAC, length, BE]   (:146-149)
 *   [mac B     digest = update(update(0, header), payload)]   (:152-155)
 *   [payload]  only when it is shorter than SMALL_ENTRY_SIZE_THRESHOLD (:128, :160-163;
 *              $BK/proto/BookieProtoEncoding.java:48); a larger payload follows the 60 + mac bytes as the
 *              second buffer of a ByteBufList (:165), and is not copied.
 * Request i is written at d_requests + d_request_offsets[i], at any alignment: 60 + mac bytes, and
 * d_lengths[i] payload bytes behind them when d_lengths[i] < small_threshold. No other byte is written:
 * not between requests, not behind the digest of an entry at or over the threshold. small_threshold is
 * the caller's (BKD_V2_SMALL_ENTRY_THRESHOLD for the reference's; 0 copies nothing). The ledger id is
 * d_ledger_ids[i], or ledger_id for all when d_ledger_ids is NULL; the length field is the caller's, as
 * in bkd_digest_package_batch. Entry i's master key is the 20 bytes at d_master_keys + i*key_stride;
 * key_stride == 0 is one key for all, key_stride in 1..19 and flags over 16 bits are
 * BKD_ERR_INVALID_ARG. d_digests[i] receives the digest value. Requests must not overlap each other or
 * the payload (the result is undefined otherwise).
 * Device pointers; asynchronous on `stream`, no host synchronisation; n == 0 launches nothing. The
 * digests come as bkd_digest_package_batch computes them; one kernel then writes every request's 60 +
 * mac bytes and one copies the payloads under the threshold, a lane group per entry. An out-of-range
 * payload gets digest 0, its 60 + mac bytes are still written, nothing is copied, and the stream's
 * bounds flag is raised (BKD_ERR_BOUNDS from the next bkd_stream_sync); a request whose range does not
 * lie inside requests_size is not written at all and raises the same flag; every other entry is exact. */
#define BKD_V2_SMALL_ENTRY_THRESHOLD 16384u
BKD_API int bkd_digest_package_batch_v2(int algo, int64_t ledger_id, const int64_t* d_ledger_ids,
                                        const int64_t* d_entry_ids, const int64_t* d_lacs,
                                        const int64_t* d_length_fields, const void* d_payload, uint64_t payload_size,
                                        const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                        const uint8_t* d_master_keys, uint64_t key_stride, uint32_t flags,
                                        uint32_t small_threshold, void* d_requests, uint64_t requests_size,
                                        const uint64_t* d_request_offsets, uint32_t* d_digests, void* stream);
/* Host-resident: payload i is its own host buffer, h_requests[i] the caller's buffer for request i —
 * the allocator.buffer(bufferSize) of DigestManager.java:135-137, 60 + mac (+ h_lengths[i]) bytes.
 * Synchronous; route by bkd_set_host_batch_route. CPU: DigestManager's arithmetic per entry on the
 * host threads, the payload copied in right after it is folded; it needs no device. GPU: staged and
 * digested as bkd_digest_package_batch_host; the host writes each prefix, the returned header and
 * digest, and copies the small payloads from their sources, so no payload byte comes back over PCIe. */
BKD_API int bkd_digest_package_batch_v2_host(int algo, int64_t ledger_id, const int64_t* h_ledger_ids,
                                             const int64_t* h_entry_ids, const int64_t* h_lacs,
                                             const int64_t* h_length_fields, const void* const* h_payloads,
                                             const uint32_t* h_lengths, uint64_t n, const uint8_t* h_master_keys,
                                             uint64_t key_stride, uint32_t flags, uint32_t small_threshold,
                                             void* const* h_requests, uint32_t* h_digests);
/* ---- re-framing verified entries with a new LAC (re-replication) -----------------------
 * LedgerFragmentReplicator frames every entry it has just read and verified a second time with the
 * ledger's current LAC: computeDigestAndPackageForSending(entryId, lh.getLastAddConfirmed(),
 * entry.getLength(), data, ...) ($BK/client/LedgerFragmentReplicator.java:436-442, 506-511) — the same
 * ledger id, entry id, length field and payload. CRC is affine over GF(2): for headers H, H' of equal
 * length, crc(H' || P) = crc(H || P) ^ R(H ^ H') * x^(8 |P|) (mod P), R(D) the register after folding
 * D from a zero register. So a frame that verified is re-framed from its old header, its stored digest,
 * the new LAC and the payload LENGTH: no payload byte is read again.
 *
 * Entry i is the framed buffer of bkd_digest_verify_batch. Default (flags == 0): the call verifies
 * exactly as bkd_digest_verify_batch does (d_status, *d_first_bad bit for bit the same), then re-frames
 * every entry whose status is BKD_VERIFY_OK. BKD_REFRAME_TRUSTED: the caller has verified these frames
 * (the usual flow: the read op did); no payload byte is read and no digest recomputed, the status is
 * what the header alone decides in verifyDigest's order (1 too short / out of range, 2 a non-zero high
 * word of CRC32's 8-byte digest, 3 / 4 the id checks) — a frame whose stored digest was wrong gets a
 * digest that is wrong again.
 * Output, OK entries only (no byte of any other entry's frame or out-frame is written):
 *   apart    (d_out_frames != NULL): [32 B header with d_new_lacs[i]][digest] at d_out_frames +
 *            i*frame_stride (frame_stride >= 32 + mac; the range must not overlap d_framed);
 *   in place (d_out_frames == NULL): header bytes 16..23 and the digest of the frame itself. Frames
 *            must not overlap one another: the result for overlapping frames is undefined.
 * d_digests (may be NULL): the new digest per entry, 0 for an entry that is not OK.
 * Device pointers; asynchronous on `stream`; no host synchronisation. */
#define BKD_REFRAME_TRUSTED 1u /* do not recompute digests: the caller verified these frames */
BKD_API int bkd_digest_reframe_batch(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                                     uint32_t flags, void* d_framed, uint64_t framed_size,
                                     const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                     const int64_t* d_new_lacs, void* d_out_frames, uint64_t frame_stride,
                                     uint32_t* d_digests, int32_t* d_status, uint64_t* d_first_bad, void* stream);
/* Host-resident: entry i is its own writable host buffer h_frames[i] of h_lengths[i] bytes, re-framed in
 * place. Route as bkd_digest_verify_batch_host (bkd_set_host_batch_route). CPU: verifyDigest's arithmetic
 * per entry (skipped when trusted), then the GF(2) correction — one payload pass at most, and it needs
 * no device. GPU: staged as verify; status and digests come back and the host writes each OK frame's
 * 8 LAC bytes and digest. Synchronous. h_digests may be NULL. */
BKD_API int bkd_digest_reframe_batch_host(int algo, int64_t ledger_id, int64_t first_entry_id, int skip_entry_check,
                                          uint32_t flags, void* const* h_frames, const uint32_t* h_lengths,
                                          uint64_t n, const int64_t* h_new_lacs, uint32_t* h_digests,
                                          int32_t* h_status, uint64_t* h_first_bad);

/* ---- bookie-side entry-log scrub (§8f row 4) ------------------------------------------
 * An entry log is a 1024-byte file header (LOGFILE_HEADER_SIZE, DefaultEntryLogger.java:256)
 * followed by records [int32 BE size][entry bytes], an entry starting with its BE ledger id.
 *
 * Index: walks the records of a HOST buffer from byte `start` exactly like
 * DefaultEntryLogger.scanEntryLog ($BK/bookie/DefaultEntryLogger.java:995-1060): size <= 0 is
 * padding (advance one byte), ledger id -1 (INVALID_LID) is a ledgers-map record (skipped), a
 * short read of the 12-byte [size, ledgerId] header or of the entry ends the scan. Writes each
 * entry's offset (first byte after the size field), length and ledger id; *h_end = the position
 * where the walk stopped. BKD_ERR_BOUNDS when more than `capacity` entries are found.
 * Host-only control logic: it reads 12 bytes per record and computes no digest. */
BKD_API int bkd_entrylog_index(const void* h_log, uint64_t log_size, uint64_t start, uint64_t* h_offsets,
                       uint32_t* h_lengths, int64_t* h_ledger_ids, uint64_t capacity, uint64_t* h_count,
                       uint64_t* h_end);

/* Verify: the digest of every indexed entry of a DEVICE-resident log, as
 * DigestManager.verifyDigest would (DigestManager.java:226-283: CRC of [0,32) || [32+mac, len)
 * against the stored digest at 32) without ledger/entry id checks (the ledger id comes from the
 * entry itself). Status codes as bkd_digest_verify_batch (0 ok, 1 too short, 2 digest mismatch);
 * *d_first_bad = first failing index or n. One digest type per call (the ledger's, from its
 * metadata; bkd_entrylog_verify_ledgers below takes a log that mixes types, MAC ledgers included).
 * Asynchronous on `stream`; ragged batches go through the chunked plan. */
BKD_API int bkd_entrylog_verify(int algo, const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                        const uint32_t* d_lengths, uint64_t n, int32_t* d_status, uint64_t* d_first_bad,
                        void* stream);

/* Verify across ledgers and digest types: a whole entry-log index in one call. An entry log interleaves
 * the entries of every ledger that was open while it was written; each ledger has its own digest type
 * (DataFormats.proto:45-50) and a MAC ledger its own key. Entry i is d_log + d_offsets[i], d_lengths[i]
 * bytes, as bkd_entrylog_index found it; its ledger id is its own first 8 bytes (big-endian), looked up in
 * the ledger table d_ledger_ids[nledgers] (strictly ascending as signed values) by binary search. Row r has
 * digest type d_ledger_types[r] (BKD_DIGEST_*) and, for HMAC, key row d_ledger_keys[r] of the nkeys x 10
 * table bkd_mac_key_init fills (several ledgers may share a row). `types` is a mask of 1u << BKD_DIGEST_*:
 * the types this call verifies; d_ledger_keys and d_key_states may be NULL when its HMAC bit is clear.
 *
 * d_status[i], with no ledger-id or entry-id checks:
 *   offset + length > log_size: 1, not read, and the stream's bounds flag is raised (BKD_ERR_BOUNDS from
 *     the next bkd_stream_sync); shorter than 8 bytes: 1;
 *   ledger not in the table, a type value outside 0..3, or a type not in `types`: BKD_VERIFY_NOT_CHECKED;
 *   CRC32C / CRC32: what bkd_entrylog_verify gives the entry (1 under 36 / 40 bytes, 2 digest mismatch);
 *   HMAC: what bkd_digest_verify_batch_mac gives it without the id checks (1 under 52 bytes, 2 when any of
 *     the 20 MAC bytes differs); longer than BKD_MAC_MAX_ENTRY or key row >= nkeys: not read, 1, and the
 *     flag is raised; no word outside the key table is loaded;
 *   DUMMY: 0 from 32 bytes on, else 1 (its digest is empty, DummyDigestManager.java:35-43,
 *     DigestManager.java:229-235).
 * *d_first_bad = the lowest index whose status is above 0, n when there is none. n == 0 writes 0 and
 * launches nothing else; nledgers == 0 is legal (every readable entry of 8 bytes or more is
 * BKD_VERIFY_NOT_CHECKED). n < 2^32. Asynchronous on `stream`, no host synchronisation.
 *
 * Device sequence (scrub_kernels.hpp): classify (one lane per entry) -> the HMAC frames
 * counted into 73 length bins, four per power of two of their SHA-1 block count, and scattered bin by bin,
 * longest first, so that the lanes of a wave hash entries of nearly one length (bkd_set_scrub_order) ->
 * one lane per HMAC frame -> bkd_entrylog_verify's sequence once per CRC type in `types`, over the entries
 * of that type -> merge. Every load of log bytes outside the CRC sequence is an aligned dword that holds a
 * byte of the entry it is loaded for. The device does not validate the table's order: an unsorted table may
 * make a listed ledger look unlisted, it never causes a load outside the three table arrays.
 * Argument errors (a null array with n > 0 or nledgers > 0, `types` with bits above 3, the HMAC bit with a
 * null key array or nkeys == 0, n >= 2^32) return BKD_ERR_INVALID_ARG before the device is looked for. */
#define BKD_DIGEST_CRC32C 0 /* == BKD_CRC32C */
#define BKD_DIGEST_CRC32 1  /* == BKD_CRC32 */
#define BKD_DIGEST_HMAC 2
#define BKD_DIGEST_DUMMY 3
#define BKD_VERIFY_NOT_CHECKED (-1)
BKD_API int bkd_entrylog_verify_ledgers(const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                                        const uint32_t* d_lengths, uint64_t n, const int64_t* d_ledger_ids,
                                        const uint32_t* d_ledger_types, const uint32_t* d_ledger_keys,
                                        uint64_t nledgers, const uint32_t* d_key_states, uint64_t nkeys,
                                        uint32_t types, int32_t* d_status, uint64_t* d_first_bad, void* stream);
/* Host-resident form: the log, the index, the tables and the outputs in host memory. Synchronous. The
 * table's order and every HMAC row's key index (when the HMAC bit is in `types`) are checked before any
 * work: a violation returns BKD_ERR_INVALID_ARG and writes nothing. Route (bkd_set_host_batch_route):
 * 1 the CPU (the same lookup, DigestManager's arithmetic per entry on the host threads; no device needed),
 * 2 the GPU (one upload of the log and the tables into plain allocations, the device call, the statuses
 * copied back; BKD_ERR_NOMEM when an allocation fails), 0 automatic: the GPU when a device is visible and
 * the table lists an HMAC ledger whose bit is in `types` (41.8 against 7.9 GB/s), else the
 * CPU (the CRC crossover of DESIGN.md §5). Both routes write every status and *h_first_bad and then return
 * BKD_ERR_BOUNDS when some entry was unreadable (out of range, over BKD_MAC_MAX_ENTRY, key row >= nkeys). */
BKD_API int bkd_entrylog_verify_ledgers_host(const void* h_log, uint64_t log_size, const uint64_t* h_offsets,
                                             const uint32_t* h_lengths, uint64_t n, const int64_t* h_ledger_ids,
                                             const uint32_t* h_ledger_types, const uint32_t* h_ledger_keys,
                                             uint64_t nledgers, const uint32_t* h_key_states, uint64_t nkeys,
                                             uint32_t types, int32_t* h_status, uint64_t* h_first_bad);
/* Which entries the HMAC lanes of bkd_entrylog_verify_ledgers take: 0 (default) binned by length, longest
 * bin first; 1 index order, through the same kernels with an identity permutation. Results are identical;
 * only the speed differs (tools/scrub_ab.py times both in one process). get: the current order. */
BKD_API int bkd_set_scrub_order(int order);
BKD_API int bkd_get_scrub_order(void);
/* The route bkd_entrylog_verify_ledgers_host takes for this table and mask (1 the CPU, 2 the GPU): the
 * forced route when one is set, else the automatic choice described above. */
BKD_API int bkd_get_scrub_host_route(const uint32_t* h_ledger_types, uint64_t nledgers, uint32_t types);
/* Host-only, for the CPU suite: the length bin of an HMAC frame of frame_len bytes (0..72; 0 under 52
 * bytes, which are never hashed), and the row of `id` in the ascending table ids[0, nledgers) or -1 — the
 * two rules the device applies (scrub_rules.hpp). */
BKD_API uint32_t bkd_host_scrub_bin(uint32_t frame_len);
BKD_API int64_t bkd_host_scrub_lookup(const int64_t* ids, uint64_t nledgers, int64_t id);
/* A hook for tests and tools: which entries the HMAC lanes of bkd_entrylog_verify_ledgers would take, and in
 * which order. The arguments of that call without d_status and d_first_bad; `types` must hold the HMAC bit
 * (BKD_ERR_INVALID_ARG otherwise, and for what that call refuses). Runs that call's classify, scan and
 * scatter launches on `stream` (its status array comes from the stream's scratch), honours
 * bkd_set_scrub_order and raises the stream's bounds flag as that call does; nothing is hashed. Then, on the
 * stream: *d_nlanes = the lanes mac_scrub_kernel would run (order 0: the HMAC frames that are hashed; order
 * 1: n) and d_lanes[0, n) = the permutation array, of which [0, *d_nlanes) is meaningful: lane s takes entry
 * d_lanes[s] (order 0: bins descending, arbitrary inside a bin; order 1: the identity, lanes of other classes
 * return at once). n == 0 writes *d_nlanes = 0. */
BKD_API int bkd_entrylog_scrub_lanes(const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                                     const uint32_t* d_lengths, uint64_t n, const int64_t* d_ledger_ids,
                                     const uint32_t* d_ledger_types, const uint32_t* d_ledger_keys,
                                     uint64_t nledgers, const uint32_t* d_key_states, uint64_t nkeys,
                                     uint32_t types, uint32_t* d_lanes, uint32_t* d_nlanes, void* stream);

/* Scrub report: bkd_entrylog_verify_ledgers, then what a scrub is read for, all on the device: one row per
 * ledger and the ascending list of bad entries. Every input has the meaning it has in that call (the
 * log, the index, the ledger table, the key table, `types`, `stream`); the statuses are that call's.
 *
 * d_status: n statuses as in that call, or NULL (they then live in the stream's scratch only).
 * d_report: (nledgers + 1) x BKD_SCRUB_REPORT_WORDS uint64 words, row r for table row r. An entry that is in
 *   range and at least 8 bytes long belongs to the row of its ledger id; an entry that is out of range,
 *   shorter than 8 bytes or of a ledger the table does not list belongs to the last row. A ledger whose
 *   type is masked out keeps its own row (its entries count in NOT_CHECKED). Words of a row:
 *     BKD_REPORT_ENTRIES          entries of the row; == OK + BAD + NOT_CHECKED
 *     BKD_REPORT_BYTES            sum of length + 4 over them, 64 bits wide: what EntryLogMetadata keeps per
 *                                 ledger (DefaultEntryLogger.java:1191, readableBytes() + 4)
 *     BKD_REPORT_OK / BAD / NOT_CHECKED   entries with status 0 / above 0 / BKD_VERIFY_NOT_CHECKED
 *     BKD_REPORT_MIN_BAD_ENTRY / MAX_BAD_ENTRY   lowest / highest entry id (bytes [8, 16) big-endian, compared
 *                                 as signed 64-bit values, stored as bits) of a bad entry that is in range
 *                                 and at least 16 bytes long; INT64_MAX / INT64_MIN when there is none
 *     BKD_REPORT_FIRST_BAD_INDEX  lowest index i of a bad entry of the row, n when there is none
 * d_bad, bad_capacity, d_nbad: *d_nbad = the entries with a status above 0 (it may exceed the capacity);
 *   d_bad[0, min(*d_nbad, bad_capacity)) = their indices ascending, so d_bad[0] is that call's first_bad and
 *   a truncated list holds the lowest ones; nothing is written at or behind min(*d_nbad, bad_capacity).
 *   bad_capacity == 0 with a NULL d_bad is legal.
 * n == 0: the rows get their initial values (zeros, INT64_MAX, INT64_MIN, 0), *d_nbad = 0, nothing else
 * is launched. nledgers == 0 is legal: the only row is the catch-all row.
 *
 * Device sequence (scrub_report_kernels.hpp): that call's kernels unchanged, then row init ->
 * one lane per entry (lanes of a wave that share a row combine in the wave; one lane per row and wave issues
 * the 64-bit atomics, one per block where all of a block's waves sit on one row) -> a one-block scan of the blocks' bad counts -> the bad indices scattered in lane
 * order. Asynchronous on `stream`, no host synchronisation; the bounds flag is raised exactly as by that
 * call. Argument errors: that call's, a null d_report or d_nbad, bad_capacity > 0 with a null d_bad. */
#define BKD_SCRUB_REPORT_WORDS 8
#define BKD_REPORT_ENTRIES 0
#define BKD_REPORT_BYTES 1
#define BKD_REPORT_OK 2
#define BKD_REPORT_BAD 3
#define BKD_REPORT_NOT_CHECKED 4
#define BKD_REPORT_MIN_BAD_ENTRY 5
#define BKD_REPORT_MAX_BAD_ENTRY 6
#define BKD_REPORT_FIRST_BAD_INDEX 7
BKD_API int bkd_entrylog_scrub_report(const void* d_log, uint64_t log_size, const uint64_t* d_offsets,
                                      const uint32_t* d_lengths, uint64_t n, const int64_t* d_ledger_ids,
                                      const uint32_t* d_ledger_types, const uint32_t* d_ledger_keys,
                                      uint64_t nledgers, const uint32_t* d_key_states, uint64_t nkeys,
                                      uint32_t types, int32_t* d_status, uint64_t* d_report, uint32_t* d_bad,
                                      uint64_t bad_capacity, uint64_t* d_nbad, void* stream);
/* Host-resident form: the arguments of bkd_entrylog_verify_ledgers_host with host outputs as above; h_status
 * may be NULL. Synchronous. The table checks, the routes (bkd_get_scrub_host_route answers for this call too)
 * and the rule that everything is written before BKD_ERR_BOUNDS is returned are that call's. Route 1: the CPU
 * route's statuses, then one serial pass with the rules the device applies (scrub_report_rules.hpp); no
 * device needed. Route 2: one upload, the device call on a stream of its own, then the report, the list and
 * *h_nbad copied back, and the statuses only when h_status is given. */
BKD_API int bkd_entrylog_scrub_report_host(const void* h_log, uint64_t log_size, const uint64_t* h_offsets,
                                           const uint32_t* h_lengths, uint64_t n, const int64_t* h_ledger_ids,
                                           const uint32_t* h_ledger_types, const uint32_t* h_ledger_keys,
                                           uint64_t nledgers, const uint32_t* h_key_states, uint64_t nkeys,
                                           uint32_t types, int32_t* h_status, uint64_t* h_report, uint32_t* h_bad,
                                           uint64_t bad_capacity, uint64_t* h_nbad);
/* The ledgers map of an entry log in a HOST buffer, read as getHeaderForLogId and
 * extractEntryLogMetadataFromIndex do (DefaultEntryLogger.java:881-906, :1089-1176): the header's version
 * (byte 4, int32 BE), ledgersMapOffset (byte 8, int64) and ledgersCount (byte 16, int32); from the offset,
 * records [int32 size][int64 -1][int64 -2][int32 count][(int64 ledger, int64 size) x count] until a size
 * <= 0 or the end of the buffer. Writes the pairs as they lie (duplicates included) to h_ledger_ids /
 * h_sizes up to `capacity` (*h_count = the pairs found; BKD_ERR_BOUNDS when that is more than `capacity`, the
 * first `capacity` of them written and the map checked all the same), the three header fields
 * (each pointer may be NULL) and *h_state: BKD_LEDGERS_MAP_READ; BKD_LEDGERS_MAP_ABSENT (version < 1 or
 * offset 0: the reference falls back to scanning); BKD_LEDGERS_MAP_MALFORMED wherever the reference throws,
 * bkd_last_error naming the case: a record's ledger id != -1, its entry id != -2, a record longer or shorter
 * than its count implies, a short read, distinct ledgers != the header's count, a header count of 0. The
 * return value is BKD_OK for all three states. Host-only control logic: it computes no digest. */
#define BKD_LEDGERS_MAP_READ 0
#define BKD_LEDGERS_MAP_ABSENT 1
#define BKD_LEDGERS_MAP_MALFORMED 2
BKD_API int bkd_entrylog_ledgers_map(const void* h_log, uint64_t log_size, int64_t* h_ledger_ids, int64_t* h_sizes,
                                     uint64_t capacity, uint64_t* h_count, int32_t* h_version,
                                     int64_t* h_map_offset, int32_t* h_ledgers_count, int32_t* h_state);

/* ---- MAC ledgers: batched HMAC-SHA1 (DigestType.MAC, MacDigestManager) ------------------
 * MacDigestManager ($BK/proto/checksum/MacDigestManager.java:46-107) digests with HmacSHA1 keyed with
 * SHA1("mac" || passwd) (:61, :79-84); the digest is 20 bytes (:67-69) written after the 32-byte header
 * (DigestManager.java:146-155, 172-178). SHA-1 is serial inside an entry and entries are independent:
 * the device kernels hash one entry per lane (mac_kernels.hpp), the CPU route one entry per host task.
 *
 * Key setup (host only, no device). gen_digest: out20 = SHA1(pad || passwd), MacDigestManager.genDigest
 * — with pad "ledger" it is a ledger's master key (:48-55), with "mac" the HMAC key. key_init writes ten
 * words: the SHA-1 state after compressing key ^ ipad (words 0..4) and key ^ opad (5..9) for
 * key = SHA1("mac" || passwd). key_state: the same for a raw HMAC key of at most 64 bytes. Every MAC call
 * takes the ten words as a host pointer and reads them during the call. */
BKD_API int bkd_mac_gen_digest(const char* pad, const void* passwd, uint64_t passwd_len, uint8_t* out20);
BKD_API int bkd_mac_key_init(const void* passwd, uint64_t passwd_len, uint32_t* key_state10);
BKD_API int bkd_mac_key_state(const void* key, uint64_t key_len, uint32_t* key_state10);
/* out20 = HMAC of one host buffer, always on the CPU (no device needed), any length. */
BKD_API int bkd_mac_cpu(const uint32_t* key_state, const void* h_ptr, uint64_t len, uint8_t* out20);

/* One lane hashes one entry serially, so an entry's length bounds the kernel's run time: the device
 * calls refuse entries (verify: frames) longer than this. The reference's largest entry is its Netty
 * frame limit, 5 MiB ($BK/conf/AbstractConfiguration.java:147). */
#define BKD_MAC_MAX_ENTRY (16u << 20)

/* Device-resident batches. Asynchronous on `stream`, no host synchronisation; n == 0 launches nothing
 * (verify then writes 0 to *d_first_bad). Entries are indexed as in bkd_crc_batch, frames laid out and
 * statuses decided as in bkd_digest_package_batch / bkd_digest_verify_batch with a 20-byte digest
 * (frame_stride >= 52; only the 52 bytes of a stride are written; verify compares all 20 bytes of
 * [0, 32) || [52, len)'s MAC, precedence too short, digest, ledger, entry). An entry with
 * offset + length > size or length > BKD_MAC_MAX_ENTRY is not read: its MAC bytes are zero (the
 * package call still writes its header), verify gives it BKD_VERIFY_TOO_SHORT, and the stream's bounds
 * flag is raised (BKD_ERR_BOUNDS from the next bkd_stream_sync). Every load is an aligned dword that
 * holds a byte of the entry: no byte outside [d_base, d_base + size) rounded out to dwords is read.
 *   bkd_mac_batch: d_out + 20 i = HMAC(entry i). */
BKD_API int bkd_mac_batch(const uint32_t* key_state, const void* d_base, uint64_t base_size, const uint64_t* d_offsets,
                          const uint32_t* d_lengths, uint64_t n, uint8_t* d_out, void* stream);
BKD_API int bkd_digest_package_batch_mac(const uint32_t* key_state, int64_t ledger_id, const int64_t* d_entry_ids,
                                         const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                         uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                                         uint64_t n, void* d_frames, uint64_t frame_stride, void* stream);
BKD_API int bkd_digest_verify_batch_mac(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id,
                                        int skip_entry_check, const void* d_framed, uint64_t framed_size,
                                        const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                        int32_t* d_status, uint64_t* d_first_bad, void* stream);
/* Host-resident forms, shaped as their CRC siblings (entry i its own host buffer; package: 52 <=
 * frame_stride <= 4096, only 52 bytes of a stride written). Synchronous. Route by
 * bkd_set_host_batch_route: 1 the CPU route (one entry per task on the host threads; no device needed),
 * 2 the GPU (pinned staging, then the kernels above), 0 automatic: the GPU whenever a device is visible
 * — measured 41.8 GB/s against the CPU route's 7.9 GB/s on 16 threads, 64K entries of 4 KiB
 * (DESIGN.md §5f). A batch that holds an entry over BKD_MAC_MAX_ENTRY takes the CPU route, or returns
 * BKD_ERR_INVALID_ARG when the GPU is forced. */
BKD_API int bkd_mac_batch_host(const uint32_t* key_state, const void* const* h_entries, const uint32_t* h_lengths,
                               uint64_t n, uint8_t* h_out);
BKD_API int bkd_digest_package_batch_mac_host(const uint32_t* key_state, int64_t ledger_id, const int64_t* h_entry_ids,
                                              const int64_t* h_lacs, const int64_t* h_length_fields,
                                              const void* const* h_payloads, const uint32_t* h_lengths, uint64_t n,
                                              void* h_frames, uint64_t frame_stride);
BKD_API int bkd_digest_verify_batch_mac_host(const uint32_t* key_state, int64_t ledger_id, int64_t first_entry_id,
                                             int skip_entry_check, const void* const* h_frames,
                                             const uint32_t* h_lengths, uint64_t n, int32_t* h_status,
                                             uint64_t* h_first_bad);

/* MAC batches that span many ledgers. One lane hashes one entry, so the device is full only with some
 * 260 000 entries in flight, and no single ledger has a batch of that size; a MAC ledger also has its
 * own password, hence its own key. These calls take a key table — nkeys x 10 uint32_t, row k what
 * bkd_mac_key_init / bkd_mac_key_state writes, in device memory for the device calls and in host memory
 * for the _host forms — and an index into it per request (verify) or per entry (package). Several
 * requests or entries may name one row.
 *
 * Verify requests: the CSR, the ledger ids, the first entry ids, BKD_REQUEST_SKIP_ENTRY_ID, d_status and
 * d_req_first_bad exactly as in bkd_digest_verify_requests (n == 0 writes zeros; nreq == 0 requires
 * n == 0); frames and status codes exactly as in bkd_digest_verify_batch_mac; request r is keyed with row
 * d_req_keys[r]. Package: frames as in bkd_digest_package_batch_mac, entry i framed for d_ledger_ids[i]
 * and keyed with row d_key_of[i].
 *
 * A key index >= nkeys on the device: the entry counts as unreadable and is not read — verify gives it
 * BKD_VERIFY_TOO_SHORT, package writes its header and zero MAC bytes — and the stream's bounds flag is
 * raised; no row outside the table is loaded. A malformed CSR on the device behaves as in
 * bkd_digest_verify_requests: the flag is raised, the outputs are unspecified, no access leaves the
 * caller's arrays. Asynchronous on `stream`, no host synchronisation. */
BKD_API int bkd_digest_verify_requests_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_req_keys,
                                           const void* d_framed, uint64_t framed_size, const uint64_t* d_offsets,
                                           const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first,
                                           uint64_t nreq, const int64_t* d_req_ledger_ids,
                                           const int64_t* d_req_first_entry_ids, const uint32_t* d_req_flags,
                                           int32_t* d_status, uint64_t* d_req_first_bad, void* stream);
BKD_API int bkd_digest_package_batch_ledgers_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                                 const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                                 const int64_t* d_lacs, const int64_t* d_length_fields,
                                                 const void* d_payload, uint64_t payload_size,
                                                 const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n,
                                                 void* d_frames, uint64_t frame_stride, void* stream);
/* Host-resident forms, shaped as bkd_digest_verify_requests_host / bkd_digest_package_batch_ledgers_host
 * with the key table, nkeys and the index array (host memory) in front, and no digest words out.
 * Synchronous; the route as for the MAC host forms above. The index array (every value < nkeys) and the
 * CSR are checked before any work: a violation returns BKD_ERR_INVALID_ARG and writes nothing. The GPU
 * route uploads the table once per call and stages entries in segments of at most 64 MiB; a request that
 * straddles two segments gets the minimum of both parts as its verified prefix. */
BKD_API int bkd_digest_verify_requests_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_req_keys,
                                                const void* const* h_frames, const uint32_t* h_lengths, uint64_t n,
                                                const uint64_t* h_req_first, uint64_t nreq,
                                                const int64_t* h_req_ledger_ids, const int64_t* h_req_first_entry_ids,
                                                const uint32_t* h_req_flags, int32_t* h_status,
                                                uint64_t* h_req_first_bad);
BKD_API int bkd_digest_package_batch_ledgers_mac_host(const uint32_t* h_key_states, uint64_t nkeys,
                                                      const uint32_t* h_key_of, const int64_t* h_ledger_ids,
                                                      const int64_t* h_entry_ids, const int64_t* h_lacs,
                                                      const int64_t* h_length_fields, const void* const* h_payloads,
                                                      const uint32_t* h_lengths, uint64_t n, void* h_frames,
                                                      uint64_t frame_stride);

/* MAC reframe: re-replication of MAC ledgers (the flow of bkd_digest_reframe_batch above). HMAC has no
 * affine shortcut, so a frame is hashed again; but the old and the new frame differ only in header bytes
 * 16..23, so every 64-byte block behind the first is loaded, realigned and expanded once and compressed
 * into two chains, one per header: verify and re-frame in one pass, one launch sequence and no host round
 * trip. One ledger is one request; there is no single-ledger entry point.
 *
 * The key table, the CSR, d_req_flags, a key index >= nkeys, unreadable entries (out of range, over
 * BKD_MAC_MAX_ENTRY), a malformed CSR, n == 0 and nreq == 0 exactly as in bkd_digest_verify_requests_mac.
 * flags == 0: d_status, d_req_first_bad and the bounds flag are bit for bit those of
 * bkd_digest_verify_requests_mac on the same input, and every entry whose status is BKD_VERIFY_OK is
 * re-framed with d_new_lacs[i]. BKD_REFRAME_TRUSTED: the caller has verified these frames; only the MAC under
 * the new header is computed, and the status is what the header alone decides: 1 too short, unreadable or
 * no key row, else 3 / 4 by the id checks, never 2. Unlike the CRC trusted reframe, whose result for a
 * frame with a wrong digest is wrong again, the MAC written is VALID for the bytes as they lie — a frame
 * whose payload was damaged comes out verifying. The caller vouches for the bytes. Any other flag bit:
 * BKD_ERR_INVALID_ARG.
 * Output, OK entries only (no byte of any other entry's frame or out-frame is written):
 *   apart    (d_out_frames != NULL): [32 B header with d_new_lacs[i]][20 B MAC] at d_out_frames +
 *            i*frame_stride (frame_stride >= 52; only those 52 bytes are written; the range must not
 *            overlap d_framed);
 *   in place (d_out_frames == NULL, frame_stride == 0): bytes 16..23 and 32..51 of the frame itself. Frames
 *            may start at any byte address and lie back to back; they must not overlap one another.
 * Refused before any launch: a null array with n > 0, a null d_new_lacs, d_out_frames with frame_stride
 * < 52, a frame_stride without d_out_frames. Device pointers; asynchronous on `stream`; no host
 * synchronisation. */
BKD_API int bkd_digest_reframe_requests_mac(
    const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_req_keys, uint32_t flags, void* d_framed,
    uint64_t framed_size, const uint64_t* d_offsets, const uint32_t* d_lengths, uint64_t n, const uint64_t* d_req_first,
    uint64_t nreq, const int64_t* d_req_ledger_ids, const int64_t* d_req_first_entry_ids, const uint32_t* d_req_flags,
    const int64_t* d_new_lacs, void* d_out_frames, uint64_t frame_stride, int32_t* d_status, uint64_t* d_req_first_bad,
    void* stream);
/* Host-resident: entry i is its own writable host buffer h_frames[i], re-framed in place. Synchronous; the
 * route as for the MAC host forms above. flags and h_new_lacs, then everything
 * bkd_digest_verify_requests_mac_host checks, in its order, before any work: a violation returns
 * BKD_ERR_INVALID_ARG and writes nothing. CPU: one frame per host task, the two chains over one schedule
 * as on the device; no device needed. GPU: staged as bkd_digest_verify_requests_mac_host with the new LACs
 * beside; the device writes packed 52-byte out-frames, which come back with the statuses, and the host
 * writes bytes 16..23 and 32..51 of each OK frame. A request that straddles two staged segments gets the
 * minimum of both parts as its prefix. */
BKD_API int bkd_digest_reframe_requests_mac_host(
    const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_req_keys, uint32_t flags, void* const* h_frames,
    const uint32_t* h_lengths, uint64_t n, const uint64_t* h_req_first, uint64_t nreq, const int64_t* h_req_ledger_ids,
    const int64_t* h_req_first_entry_ids, const uint32_t* h_req_flags, const int64_t* h_new_lacs, int32_t* h_status,
    uint64_t* h_req_first_bad);

/* MAC adds: composite payloads and V2 add requests, the two add-path shapes of a MAC ledger behind a
 * Pulsar broker. Both span ledgers through the key table of bkd_digest_package_batch_ledgers_mac (one
 * ledger: a table of one row): entry i is keyed with row d_key_of[i] and framed for d_ledger_ids[i];
 * d_key_of == NULL keys every entry with row 0, d_ledger_ids == NULL frames every entry for ledger_id.
 *
 * An entry is unreadable when its key index is >= nkeys, when a non-empty segment (or its payload range)
 * does not lie inside [0, payload_size), or when its length is over BKD_MAC_MAX_ENTRY. Its payload is not
 * read; its 32-byte header is still written, with 20 zero MAC bytes, and the stream's bounds flag is
 * raised (BKD_ERR_BOUNDS from the next bkd_stream_sync). Every load is an aligned dword that holds at
 * least one byte of the segment it is loaded for, and no byte outside a segment's own bytes reaches the
 * hash. Asynchronous on `stream`, no host synchronisation; n == 0 launches nothing.
 *
 * Segments: the segment arrays, the CSR d_seg_first and the frames exactly as in
 * bkd_digest_package_batch_segments with a 20-byte digest (frame_stride >= 52, only 52 bytes of a stride
 * written). Empty segments are skipped, wherever they say they lie; segments may be unaligned, overlap
 * and be shared between entries; nseg == 0 with n > 0 is legal. A malformed d_seg_first is clamped as
 * there (bkd_host_segments_range): the flag is raised and nothing outside the caller's arrays is read.
 * HMAC has no algebra to join per-segment digests with, so one lane hashes its entry's segments as one
 * byte stream, the SHA-1 blocks straddling the cuts; each payload byte is read once and none is copied.
 * A composite entry's length is the 64-bit sum of its segments, given up as soon as it passes the cap
 * (bkd_host_segments_length_capped), so no number of listings wraps to a short entry.
 *
 * V2: request i = [int32 BE 76 + len][int32 BE packet header][20 B master key][32 B header][20 B MAC]
 * and the len payload bytes behind it when len < small_threshold, at d_requests + d_request_offsets[i]
 * at any alignment; no other byte is written. key_stride (0 or >= 20), flags (16 bits) and
 * small_threshold as in bkd_digest_package_batch_v2. An unreadable entry gets its 80-byte head and
 * nothing is copied; a request whose range (the head, and the payload where it is copied) does not fit
 * requests_size is not written at all and raises the flag. */
BKD_API int bkd_digest_package_batch_segments_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                                  int64_t ledger_id, const int64_t* d_ledger_ids,
                                                  const int64_t* d_entry_ids, const int64_t* d_lacs,
                                                  const int64_t* d_length_fields, const void* d_payload,
                                                  uint64_t payload_size, const uint64_t* d_seg_offsets,
                                                  const uint32_t* d_seg_lengths, uint64_t nseg,
                                                  const uint64_t* d_seg_first, uint64_t n, void* d_frames,
                                                  uint64_t frame_stride, void* stream);
BKD_API int bkd_digest_package_batch_v2_mac(const uint32_t* d_key_states, uint64_t nkeys, const uint32_t* d_key_of,
                                            int64_t ledger_id, const int64_t* d_ledger_ids, const int64_t* d_entry_ids,
                                            const int64_t* d_lacs, const int64_t* d_length_fields, const void* d_payload,
                                            uint64_t payload_size, const uint64_t* d_offsets, const uint32_t* d_lengths,
                                            uint64_t n, const uint8_t* d_master_keys, uint64_t key_stride, uint32_t flags,
                                            uint32_t small_threshold, void* d_requests, uint64_t requests_size,
                                            const uint64_t* d_request_offsets, void* stream);
/* Host-resident forms, shaped as bkd_digest_package_batch_segments_host / bkd_digest_package_batch_v2_host
 * with the key table, nkeys and the index array (host memory; the index may be NULL) in front and no
 * digest words out. Synchronous; the route as for the MAC host forms above. The index array (every value
 * < nkeys) and the CSR (starts at 0, never decreases, ends at nseg) are checked before any work: a
 * violation returns BKD_ERR_INVALID_ARG and writes nothing. CPU: the inner hash chained over an entry's
 * non-empty segments, nothing joined; V2 copies a small payload right after hashing it. GPU: composite
 * entries are laid end to end in pinned staging (an entry is never split between two staged segments)
 * and go through bkd_digest_package_batch_ledgers_mac's device sequence; V2 is staged and packaged into
 * 52-byte frames, and the host writes each prefix, key, header and MAC and copies the small payloads
 * from their sources, so no payload byte comes back over PCIe. A batch that holds an entry over
 * BKD_MAC_MAX_ENTRY takes the CPU route, or returns BKD_ERR_INVALID_ARG when the GPU is forced. */
BKD_API int bkd_digest_package_batch_segments_mac_host(const uint32_t* h_key_states, uint64_t nkeys,
                                                       const uint32_t* h_key_of, int64_t ledger_id,
                                                       const int64_t* h_ledger_ids, const int64_t* h_entry_ids,
                                                       const int64_t* h_lacs, const int64_t* h_length_fields,
                                                       const void* const* h_seg_ptrs, const uint32_t* h_seg_lengths,
                                                       uint64_t nseg, const uint64_t* h_seg_first, uint64_t n,
                                                       void* h_frames, uint64_t frame_stride);
BKD_API int bkd_digest_package_batch_v2_mac_host(const uint32_t* h_key_states, uint64_t nkeys, const uint32_t* h_key_of,
                                                 int64_t ledger_id, const int64_t* h_ledger_ids,
                                                 const int64_t* h_entry_ids, const int64_t* h_lacs,
                                                 const int64_t* h_length_fields, const void* const* h_payloads,
                                                 const uint32_t* h_lengths, uint64_t n, const uint8_t* h_master_keys,
                                                 uint64_t key_stride, uint32_t flags, uint32_t small_threshold,
                                                 void* const* h_requests);
/* Host-only: the capped length of a composite MAC entry of segments h_seg_lengths[0, nseg): *bytes = their
 * 64-bit sum where the summation stopped, which is as soon as it passed `cap`; returns 1 when it did (the
 * entry is unreadable), else 0 (*bytes is the entry's length). The rule the device applies, for the CPU
 * suite. */
BKD_API int bkd_host_segments_length_capped(const uint32_t* h_seg_lengths, uint64_t nseg, uint64_t cap,
                                            uint64_t* bytes);

/* ---- synthetic input + test helpers --------------------------------------------------- */

/* Fills nbytes of device memory with the little-endian splitmix64 stream
 * word_i = mix(seed + (first_word + i + 1) * 0x9E3779B97F4A7C15) (SURVEY.md §8d input definition). */
BKD_API int bkd_fill_splitmix64(void* d_dst, uint64_t nbytes, uint64_t seed, uint64_t first_word, void* stream);

/* Host-only (no GPU needed): the compact fold-table image the kernels load into LDS for
 * `algo` and a group width of `lanes` (4, 8, 16, 32 or 64); returns words written or <0.
 * Layout documented in DESIGN.md §3. */
BKD_API int64_t bkd_host_tables(int algo, int lanes, uint32_t* out, uint64_t out_words);

/* Host-only: GF(2) product a*b mod P in the reflected representation, and x^(8*nbytes) mod P. */
BKD_API uint32_t bkd_host_gf_mul(int algo, uint32_t a, uint32_t b);
BKD_API uint32_t bkd_host_xpow8n(int algo, uint64_t nbytes);
/* Host-only: the clamp the device applies to entry i's two values of d_seg_first in
 * bkd_digest_package_batch_segments (first_i = d_seg_first[i], first_i1 = d_seg_first[i + 1]):
 * *k0 <= *k1 <= nseg is the range of segments the entry reads, whatever the values are; returns 1 when
 * they break the CSR (the stream's bounds flag is raised), else 0. */
BKD_API int bkd_host_segments_range(uint64_t first_i, uint64_t first_i1, uint64_t i, uint64_t n, uint64_t nseg,
                                    uint64_t* k0, uint64_t* k1);
/* Host-only: 1 when bkd_digest_package_batch_segments' join kernel folds this segment from its own
 * bytes (in range and shorter than 16 bytes; it then reaches the indexed path as offset 0, length 0),
 * else 0: the other bounds decision of that call, for the CPU suite. */
BKD_API int bkd_host_segment_bytewise(uint64_t offset, uint32_t length, uint64_t payload_size);

/* Tuning: lanes per entry group (0 = automatic, else 1/4/8/16/32/64); prefetch is fixed at build. */
BKD_API int bkd_set_group_lanes(int lanes);
/* Indexed-batch strategy: 0 = automatic (one entry per lane group when the base buffer is <= 256 KiB,
 * else the chunked plan with the short-entry class when the buffer holds at most 1 KiB per entry),
 * 1 = one entry per lane group, 2 = always the chunked plan. Any other value (the removed stream
 * route was mode 3) returns BKD_ERR_INVALID_ARG. */
BKD_API int bkd_set_plan_mode(int mode);
/* Chunked-plan geometry: lanes per group (4, 8, 16, 32 or 64), steps per full chunk (chunk = 16 * lanes *
 * steps bytes, <= 32 KiB) and the head-merge threshold in bytes (a head chunk shorter than this
 * joins its neighbour; >= 16). Default 8, 32, 16 (4 KiB chunks; tools/tune_plan.py). */
BKD_API int bkd_set_plan_geometry(int lanes, int steps_per_chunk, int merge_bytes);
/* Short-entry class of indexed batches that take the plan: entries of <= max_bytes (16..512; 0 = no
 * class) run in their own launch, loading the next entries while folding the current one (4-lane
 * groups up to 192 B, 8-lane groups above), and skip the plan's count/emit/chunk/combine work
 * (DESIGN.md §3). Used when the base buffer holds at most bkd_set_short_class_mean() bytes per entry
 * (default 1 KiB: short entries dominate). Default 192. */
BKD_API int bkd_set_plan_small(uint32_t max_bytes);
/* The short-entry class's gate: base-buffer bytes per entry at most this (default 1024; UINT64_MAX:
 * whenever a class bound is set). */
BKD_API int bkd_set_short_class_mean(uint64_t max_bytes_per_entry);
/* Entries of the plan shorter than `bytes` (16..64, default 16) skip the chunk kernel: the
 * combine kernel computes each with one thread (slice-by-16 over its 16-byte windows). */
BKD_API int bkd_set_plan_serial(uint32_t bytes);
/* Register double-buffer depth of the plan's chunk kernel (2, 4 or 8 loads per lane). */
BKD_API int bkd_set_plan_prefetch(int loads_in_flight);
/* Fold schedule of the one-entry-per-group kernels (uniform, direct indexed, package payloads):
 * 0 = chosen per launch from the shader clock the kernel measures (the low-clock schedule below
 * 2 GHz), 1 = always the compiler's schedule, 2 = always the low-clock schedule
 * (16 table lookups in flight per step). Results are identical; only the speed differs. */
BKD_API int bkd_set_fold_schedule(int schedule);
BKD_API int bkd_get_group_lanes(int algo, uint64_t mean_len);

#ifdef __cplusplus
}
#endif

#endif /* BKDIGEST_H_ */
