// Host worker pool and the CPU route of host-resident batches (host_batch.hpp). Clean-room: the
// arithmetic is host_crc.cpp's folding; the framing follows DigestManager (cited per function).
#include "host_batch.hpp"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>

#include "crc_tables.hpp"
#include "host_crc.hpp"

namespace bkd {
namespace host {

int usable_cores() {
    static const int n = [] {
        int cores = (int)std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) cores = std::max(1, CPU_COUNT(&set));
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64] = {0};
            long long period = 0;
            if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long long quota = atoll(q);
                const int cap = (int)std::max(1LL, (quota + period - 1) / period);
                cores = std::min(cores, cap);
            }
            fclose(f);
        }
        return cores;
    }();
    return n;
}

Pool& Pool::get() {
    static Pool pool;
    return pool;
}

Pool::Pool() {
    int want = usable_cores();
    if (const char* v = getenv("BKD_HOST_THREADS")) want = std::max(1, std::min(256, atoi(v)));
    active_ = want;
    for (int w = 1; w < want; ++w) workers_.emplace_back([this, w] { loop(w); });
}

Pool::~Pool() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
}

int Pool::threads() const { return (int)workers_.size() + 1; }

int Pool::active() const { return std::max(1, std::min(active_.load(std::memory_order_relaxed), threads())); }

void Pool::set_active(int n) { active_ = n <= 0 ? threads() : std::min(n, threads()); }

void Pool::run(int parts, const std::function<void(int)>& f) {
    parts = std::max(1, std::min(parts, active()));
    std::unique_lock<std::mutex> call(call_mu_, std::try_to_lock);
    if (parts == 1 || !call.owns_lock()) {  // one part, or another caller holds the workers
        for (int p = 0; p < parts; ++p) f(p);
        return;
    }
    {
        std::lock_guard<std::mutex> lk(mu_);
        job_ = &f;
        parts_ = parts;
        pending_ = parts - 1;
        ++gen_;
    }
    cv_.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
}

void Pool::loop(int part) {
    uint64_t seen = 0;
    for (;;) {
        const std::function<void(int)>* f = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            if (part >= parts_) continue;
            f = job_;
        }
        (*f)(part);
        std::lock_guard<std::mutex> lk(mu_);
        if (--pending_ == 0) done_.notify_all();
    }
}

namespace {

// Batches below this many payload bytes run on the calling thread (waking the pool costs more).
constexpr uint64_t kInlineBytes = 512u << 10;

// Runs body(i0, i1) over [0, n) in chunks taken from a shared counter, so ragged entry sizes
// balance without a serial prefix sum. Batches of fewer than 4096 entries and under kInlineBytes
// run inline.
template <class Body>
void for_chunks(uint64_t n, const uint32_t* lens, Body&& body) {
    if (n == 0) return;
    Pool& pool = Pool::get();
    const int threads = pool.active();
    bool inline_run = threads == 1;
    if (!inline_run && n < 4096) {  // small batches: sum their bytes to decide
        uint64_t bytes = 0;
        for (uint64_t i = 0; lens && i < n; ++i) bytes += lens[i];  // (no lengths: a few bytes per entry)
        inline_run = bytes < kInlineBytes;
    }
    if (inline_run) return body((uint64_t)0, n);
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(4096, n / ((uint64_t)threads * 16)));
    const uint64_t nchunks = (n + chunk - 1) / chunk;
    std::atomic<uint64_t> next{0};
    pool.run((int)std::min<uint64_t>((uint64_t)threads, nchunks), [&](int) {
        for (;;) {
            const uint64_t c = next.fetch_add(1, std::memory_order_relaxed);
            if (c >= nchunks) return;
            const uint64_t i0 = c * chunk;
            body(i0, std::min(n, i0 + chunk));
        }
    });
}

// Entries of at least kSplitBytes are folded in kPieceBytes pieces on the whole pool, each piece's
// register from zero, joined by Horner with x^(8 * piece) (the device plan's join,
// plan_kernels.hpp): a long entry is not left to one core while the others idle.
constexpr uint64_t kPieceBytes = 1u << 20;
constexpr uint64_t kSplitBytes = 4u << 20;

inline bool is_big(uint64_t len) { return len >= kSplitBytes; }

// The walk of every batch: one(i, whole_pool, ctx) for the entries below kSplitBytes in chunks over
// the pool (whole_pool = false; a fresh Ctx per chunk), then for the others one after another, each
// folded on the whole pool (split = false: all in the chunks, as with one thread). Returns the
// smallest i whose one() returned non-zero, n when none did.
template <class Ctx = char, class One>
uint64_t walk(uint64_t n, const uint32_t* lens, bool split, One&& one) {
    split = split && Pool::get().active() > 1;
    std::atomic<bool> big{false};
    std::atomic<uint64_t> first_bad{n};
    auto note_bad = [&](uint64_t bad) {
        uint64_t cur = first_bad.load(std::memory_order_relaxed);
        while (bad < cur && !first_bad.compare_exchange_weak(cur, bad, std::memory_order_relaxed)) {
        }
    };
    for_chunks(n, lens, [&](uint64_t i0, uint64_t i1) {
        uint64_t bad = n;
        Ctx ctx{};
        for (uint64_t i = i0; i < i1; ++i) {
            if (split && is_big(lens[i])) {
                big.store(true, std::memory_order_relaxed);
                continue;
            }
            if (one(i, false, ctx) != 0 && i < bad) bad = i;
        }
        note_bad(bad);
    });
    if (big.load()) {
        Ctx ctx{};
        for (uint64_t i = 0; i < n; ++i)
            if (is_big(lens[i]) && one(i, true, ctx) != 0) note_bad(i);
    }
    return first_bad.load();
}

// out[i] = resume(seed_i, the lens[i] bytes at at(i))
template <class At>
void crc_entries(int algo, At&& at, const uint32_t* lens, uint64_t n, const uint32_t* seeds, uint32_t seed_all,
                 uint32_t* out) {
    walk(n, lens, true, [&](uint64_t i, bool whole_pool, char&) {
        const uint32_t seed = seeds ? seeds[i] : seed_all;
        out[i] = !lens[i] ? seed : whole_pool ? ~fold(algo, ~seed, at(i), lens[i]) : ~crc_raw(algo, ~seed, at(i), lens[i]);
        return 0;
    });
}

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

// DigestManager.verifyDigest of one frame ($BK/proto/checksum/DigestManager.java:226-283), in its
// order: too short (:229-235), digest = update(update(0, [0, 32)), [32 + mac, len)) against getInt(32)
// / getLong(32) (:236-261), ledger id (:267-273), entry id (:275-281). payload = false: what the
// header alone decides (CRC32's non-zero high digest word still fails; no payload byte is read).
inline int32_t frame_status(int algo, uint32_t mac, int64_t ledger_id, int64_t entry_id, int id_checks,
                            const uint8_t* f, uint32_t l, bool whole_pool, bool payload) {
    if (l < 32u + mac) return 1;
    const uint32_t hi = mac == 8u ? be32(f + 32) : 0u;
    if (payload) {
        uint32_t reg = crc_raw(algo, 0xFFFFFFFFu, f, 32);  // update(0, header)
        reg = whole_pool ? fold(algo, reg, f + 32 + mac, l - 32u - mac) : crc_raw(algo, reg, f + 32 + mac, l - 32u - mac);
        if (hi != 0u || ~reg != be32(f + 32 + (mac - 4u))) return 2;
    } else if (hi != 0u) {
        return 2;
    }
    const int64_t lid = (int64_t)(((uint64_t)be32(f) << 32) | be32(f + 4));
    const int64_t eid = (int64_t)(((uint64_t)be32(f + 8) << 32) | be32(f + 12));
    if (id_checks < 2 && lid != ledger_id) return 3;
    if (id_checks == 0 && eid != entry_id) return 4;
    return 0;
}

// x^(8 * len) mod P, the last length's power kept: replicated fragments hold runs of equal lengths.
struct PowCache {
    uint64_t len = 0;
    uint32_t xp = 0x80000000u;  // x^0
    uint32_t get(int algo, uint64_t l) {
        if (l != len) {
            xp = gf2::xpow(algo, 8ull * l);
            len = l;
        }
        return xp;
    }
};

// A verified frame's digest under a new LAC, without its payload: CRC is affine over GF(2), so
// crc(H' || P) = crc(H || P) ^ R(H ^ H') * x^(8 |P|), R(D) the register after folding the header
// difference D from zero. D is non-zero in bytes 16..23 only: the fold starts there.
inline uint32_t reframed_digest(int algo, uint32_t mac, const uint8_t* f, uint32_t l, const uint8_t* new_lac_be,
                                PowCache& pw) {
    uint8_t d[16] = {0};
    for (int k = 0; k < 8; ++k) d[k] = f[16 + k] ^ new_lac_be[k];
    uint32_t delta = crc_raw(algo, 0u, d, 16);
    if (delta) delta = gf2::mul(algo, delta, pw.get(algo, l - 32u - mac));
    return be32(f + 32 + (mac - 4u)) ^ delta;
}

// verify_frames / verify_frames_expected: expected(i, &ledger_id, &entry_id) -> id_checks of frame i.
template <class Expected>
uint64_t verify_frames_by(int algo, Expected&& expected, const uint8_t* const* frames, const uint32_t* lens, uint64_t n,
                          int32_t* status) {
    const uint32_t mac = mac_len(algo);
    return walk(n, lens, true, [&](uint64_t i, bool whole_pool, char&) {
        int64_t lid, eid;
        const int id_checks = expected(i, &lid, &eid);
        return status[i] = frame_status(algo, mac, lid, eid, id_checks, frames[i], lens[i], whole_pool, true);
    });
}

// package_frames / package_frames_ledgers: ledger(i) = the ledger id that frames entry i.
// DigestManager.computeDigestAndPackageForSending (:117-181): header [ledgerId, entryId, LAC, length]
// BE (:146-149), digest = update(update(0, header), payload) (:152-153), written after the header
// (CRC32CDigestManager.java:44-46 writeInt; CRC32DigestManager.java:60-63 writeLong, zero-extended).
// payload(i, reg, whole_pool) = the register after folding entry i's payload onto reg: one buffer
// (one_buffer) or a composite's segments in order (Segments); lens[i] = the payload's bytes (the walk's
// balance and its long-entry split). frame_at(i) = where entry i's [32 B header][digest] goes.
template <class Ledger, class Payload, class FrameAt>
void package_frames_at(int algo, Ledger&& ledger, const int64_t* entry_ids, const int64_t* lacs,
                       const int64_t* length_fields, Payload&& payload, const uint32_t* lens, uint64_t n,
                       FrameAt&& frame_at, uint32_t* digests) {
    const uint32_t mac = mac_len(algo);
    walk(n, lens, true, [&](uint64_t i, bool whole_pool, char&) {
        uint8_t* f = frame_at(i);
        put_be64(f, (uint64_t)ledger(i));
        put_be64(f + 8, (uint64_t)entry_ids[i]);
        put_be64(f + 16, (uint64_t)lacs[i]);
        put_be64(f + 24, (uint64_t)length_fields[i]);
        const uint32_t reg = payload(i, crc_raw(algo, 0xFFFFFFFFu, f, 32), whole_pool);
        const uint32_t d = ~reg;
        if (mac == 8u) put_be32(f + 32, 0u);
        put_be32(f + 32 + (mac - 4u), d);
        digests[i] = d;
        return 0;
    });
}

template <class Ledger, class Payload>
void package_frames_by(int algo, Ledger&& ledger, const int64_t* entry_ids, const int64_t* lacs,
                       const int64_t* length_fields, Payload&& payload, const uint32_t* lens, uint64_t n,
                       uint8_t* frames, uint64_t stride, uint32_t* digests) {
    package_frames_at(algo, ledger, entry_ids, lacs, length_fields, payload, lens, n,
                      [=](uint64_t i) { return frames + i * stride; }, digests);
}

// The 28 bytes in front of a V2 request's header (DigestManager.java:138-142): headersSize + payloadSize
// (Java int arithmetic: 4 + 20 + 32 + mac + len), the packet header, the master key.
constexpr uint32_t kV2Prefix = 28;
inline void put_v2_prefix(uint8_t* r, uint32_t mac, uint32_t len, const V2Head& head, uint64_t i) {
    put_be32(r, 56u + mac + len);
    put_be32(r + 4, head.packet_header);
    memcpy(r + 8, head.keys + i * head.key_stride, 20);
}

}  // namespace

uint32_t fold(int algo, uint32_t reg, const uint8_t* p, uint64_t len) {
    Pool& pool = Pool::get();
    const int threads = pool.active();
    if (threads == 1 || !is_big(len)) return crc_raw(algo, reg, p, (size_t)len);
    const uint64_t np = (len + kPieceBytes - 1) / kPieceBytes;
    std::vector<uint32_t> raw(np);
    std::atomic<uint64_t> next{0};
    pool.run((int)std::min<uint64_t>((uint64_t)threads, np), [&](int) {
        for (;;) {
            const uint64_t k = next.fetch_add(1, std::memory_order_relaxed);
            if (k >= np) return;
            const uint64_t at = k * kPieceBytes;
            raw[k] = crc_raw(algo, k == 0 ? reg : 0u, p + at, (size_t)std::min(kPieceBytes, len - at));
        }
    });
    const uint32_t xp = gf2::xpow(algo, 8ull * kPieceBytes);
    uint32_t r = raw[0];
    for (uint64_t k = 1; k < np; ++k) {
        const uint64_t l = std::min(kPieceBytes, len - k * kPieceBytes);
        r = gf2::mul(algo, r, l == kPieceBytes ? xp : gf2::xpow(algo, 8ull * l)) ^ raw[k];
    }
    return r;
}

void crc_list(int algo, const uint8_t* const* ptrs, const uint32_t* lens, uint64_t n, const uint32_t* seeds,
              uint32_t seed_all, uint32_t* out) {
    crc_entries(algo, [&](uint64_t i) { return ptrs[i]; }, lens, n, seeds, seed_all, out);
}

void crc_indexed(int algo, const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, uint64_t n,
                 const uint32_t* seeds, uint32_t seed_all, uint32_t* out) {
    crc_entries(algo, [&](uint64_t i) { return base + offsets[i]; }, lens, n, seeds, seed_all, out);
}

// DigestManager.verifyDigest per frame (frame_status).
uint64_t verify_frames(int algo, int64_t ledger_id, int64_t first_entry_id, int id_checks,
                       const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status) {
    return verify_frames_by(algo, [&](uint64_t i, int64_t* lid, int64_t* eid) {
        *lid = ledger_id;
        *eid = first_entry_id + (int64_t)i;
        return id_checks;
    }, frames, lens, n, status);
}

void verify_frames_expected(int algo, const int64_t* ledger_ids, const int64_t* entry_ids, const uint32_t* req_of,
                            const uint8_t* const* frames, const uint32_t* lens, uint64_t n, int32_t* status) {
    verify_frames_by(algo, [&](uint64_t i, int64_t* lid, int64_t* eid) {
        *lid = ledger_ids[i];
        *eid = entry_ids[i];
        return (req_of[i] & kSkipEntryId) ? 1 : 0;
    }, frames, lens, n, status);
}

namespace {

// Entry i's payload as one buffer of lens[i] bytes.
auto one_buffer(int algo, const uint8_t* const* payloads, const uint32_t* lens) {
    return [=](uint64_t i, uint32_t reg, bool whole_pool) {
        if (!lens[i]) return reg;
        return whole_pool ? fold(algo, reg, payloads[i], lens[i]) : crc_raw(algo, reg, payloads[i], lens[i]);
    };
}

// Composite payloads: entry i = segments first[i] .. first[i+1]-1 in order, the register chained over
// the non-empty ones as DigestManager.update chains it over ByteBufVisitor's leaves
// (DigestManager.java:62-72, 380-392; ByteBufVisitor.java:100-103 skips empty buffers). Nothing is
// copied together.
struct Segments {
    int algo;
    const uint8_t* const* ptrs;
    const uint32_t* lens;
    const uint64_t* first;
    uint32_t operator()(uint64_t i, uint32_t reg, bool whole_pool) const {
        for (uint64_t k = first[i]; k < first[i + 1]; ++k)
            if (lens[k]) reg = whole_pool ? fold(algo, reg, ptrs[k], lens[k]) : crc_raw(algo, reg, ptrs[k], lens[k]);
        return reg;
    }
};

}  // namespace

void package_frames(int algo, int64_t ledger_id, const int64_t* entry_ids, const int64_t* lacs,
                    const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens, uint64_t n,
                    uint8_t* frames, uint64_t stride, uint32_t* digests) {
    package_frames_by(algo, [&](uint64_t) { return ledger_id; }, entry_ids, lacs, length_fields,
                      one_buffer(algo, payloads, lens), lens, n, frames, stride, digests);
}

void package_frames_ledgers(int algo, const int64_t* ledger_ids, const int64_t* entry_ids, const int64_t* lacs,
                            const int64_t* length_fields, const uint8_t* const* payloads, const uint32_t* lens,
                            uint64_t n, uint8_t* frames, uint64_t stride, uint32_t* digests) {
    package_frames_by(algo, [&](uint64_t i) { return ledger_ids[i]; }, entry_ids, lacs, length_fields,
                      one_buffer(algo, payloads, lens), lens, n, frames, stride, digests);
}

void package_frames_segments(int algo, int64_t ledger_id, const int64_t* ledger_ids, const int64_t* entry_ids,
                             const int64_t* lacs, const int64_t* length_fields, const uint8_t* const* seg_ptrs,
                             const uint32_t* seg_lens, const uint64_t* seg_first, const uint32_t* entry_lens,
                             uint64_t n, uint8_t* frames, uint64_t stride, uint32_t* digests) {
    const Segments segs{algo, seg_ptrs, seg_lens, seg_first};
    package_frames_by(algo, [&](uint64_t i) { return ledger_ids ? ledger_ids[i] : ledger_id; }, entry_ids, lacs,
                      length_fields, segs, entry_lens, n, frames, stride, digests);
}

void package_requests_v2(int algo, int64_t ledger_id, const int64_t* ledger_ids, const int64_t* entry_ids,
                         const int64_t* lacs, const int64_t* length_fields, const uint8_t* const* payloads,
                         const uint32_t* lens, uint64_t n, const V2Head& head, uint8_t* const* requests,
                         uint32_t* digests) {
    const uint32_t mac = mac_len(algo);
    const auto fold_one = one_buffer(algo, payloads, lens);
    package_frames_at(
        algo, [&](uint64_t i) { return ledger_ids ? ledger_ids[i] : ledger_id; }, entry_ids, lacs, length_fields,
        [&](uint64_t i, uint32_t reg, bool whole_pool) {
            uint8_t* r = requests[i];
            put_v2_prefix(r, mac, lens[i], head, i);
            reg = fold_one(i, reg, whole_pool);
            // copied while the fold has it in the cache (isSmallEntry, :128, :160-163)
            if (lens[i] && lens[i] < head.small) memcpy(r + kV2Prefix + 32u + mac, payloads[i], lens[i]);
            return reg;
        },
        lens, n, [=](uint64_t i) { return requests[i] + kV2Prefix; }, digests);
}

void finish_requests_v2(int algo, const uint8_t* frames, const uint8_t* const* payloads, const uint32_t* lens,
                        uint64_t n, const V2Head& head, uint64_t first, uint8_t* const* requests, int threads) {
    const uint32_t mac = mac_len(algo), hl = 32u + mac;
    // split by bytes written, as the staging gather is: the head counts for every entry
    std::vector<uint64_t> at(n + 1);
    at[0] = 0;
    for (uint64_t i = 0; i < n; ++i) at[i + 1] = at[i] + kV2Prefix + hl + (lens[i] < head.small ? lens[i] : 0u);
    const int parts = (int)std::min<uint64_t>((uint64_t)std::max(1, threads), std::max<uint64_t>(1, at[n] >> 20));
    const uint64_t per = (at[n] + parts - 1) / parts;
    Pool::get().run(parts, [&](int p) {
        const uint64_t lo = per * (uint64_t)p, hi = lo + per;
        uint64_t i = (uint64_t)(std::lower_bound(at.begin(), at.begin() + n, lo) - at.begin());
        for (; i < n && at[i] < hi; ++i) {
            uint8_t* r = requests[i];
            put_v2_prefix(r, mac, lens[i], head, first + i);
            memcpy(r + kV2Prefix, frames + i * hl, hl);
            if (lens[i] && lens[i] < head.small) memcpy(r + kV2Prefix + hl, payloads[i], lens[i]);
        }
    });
}

void crc_segments(int algo, const uint8_t* const* seg_ptrs, const uint32_t* seg_lens, const uint64_t* seg_first,
                  const uint32_t* entry_lens, uint64_t n, const uint32_t* seeds, uint32_t seed_all, uint32_t* out) {
    const Segments segs{algo, seg_ptrs, seg_lens, seg_first};
    walk(n, entry_lens, true, [&](uint64_t i, bool whole_pool, char&) {
        out[i] = ~segs(i, ~(seeds ? seeds[i] : seed_all), whole_pool);
        return 0;
    });
}

// LedgerFragmentReplicator's second framing of an entry it has read and verified
// ($BK/client/LedgerFragmentReplicator.java:436-442, 506-511: the same ids, length and payload, the
// ledger's current LAC): verifyDigest per frame (the header's part only when `trusted`), then the new
// LAC and the digest by reframed_digest into the frames that are OK. One pass over a payload at most.
uint64_t reframe_frames(int algo, int64_t ledger_id, int64_t first_entry_id, int id_checks, bool trusted,
                        uint8_t* const* frames, const uint32_t* lens, uint64_t n, const int64_t* new_lacs,
                        uint32_t* digests, int32_t* status) {
    const uint32_t mac = mac_len(algo);
    // (a trusted frame's payload is not read: nothing to split)
    return walk<PowCache>(n, lens, !trusted, [&](uint64_t i, bool whole_pool, PowCache& pw) {
        uint8_t* f = frames[i];
        const int32_t st = frame_status(algo, mac, ledger_id, first_entry_id + (int64_t)i, id_checks, f, lens[i],
                                        whole_pool, !trusted);
        uint32_t d = 0u;
        if (st == 0) {
            uint8_t lac[8];
            put_be64(lac, (uint64_t)new_lacs[i]);
            d = reframed_digest(algo, mac, f, lens[i], lac, pw);
            memcpy(f + 16, lac, 8);
            put_be32(f + 32 + (mac - 4u), d);  // (CRC32's high word is zero in a frame that is OK)
        }
        if (digests) digests[i] = d;
        return status[i] = st;
    });
}

void apply_reframe(int algo, uint8_t* const* frames, uint64_t n, const int64_t* new_lacs, const int32_t* status,
                   const uint32_t* digests) {
    const uint32_t mac = mac_len(algo);
    for_chunks(n, nullptr, [&](uint64_t i0, uint64_t i1) {
        for (uint64_t i = i0; i < i1; ++i) {
            if (status[i] != 0) continue;
            put_be64(frames[i] + 16, (uint64_t)new_lacs[i]);
            put_be32(frames[i] + 32 + (mac - 4u), digests[i]);
        }
    });
}

}  // namespace host
}  // namespace bkd
