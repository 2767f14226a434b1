// The CPU route of the mixed-ledger entry-log scrub (host_scrub.hpp).
#include "host_scrub.hpp"

#include <algorithm>
#include <vector>

#include "../../include/bkdigest.h"
#include "host_batch.hpp"
#include "host_mac.hpp"
#include "scrub_report_rules.hpp"
#include "scrub_rules.hpp"

namespace bkd {
namespace host {

uint64_t scrub_table_check(const ScrubLedgers& t) {
    for (uint64_t r = 0; r < t.nledgers; ++r) {
        if (r && !(t.ids[r - 1] < t.ids[r])) return r + 1;
        if (t.types[r] == scrub::kHmac && ((t.mask >> scrub::kHmac) & 1u) && (!t.keys || t.keys[r] >= t.nkeys))
            return r + 1;
    }
    return 0;
}

namespace {

// The members of one digest class, compacted: what the per-frame verify functions take.
struct Members {
    std::vector<uint64_t> index;
    std::vector<const uint8_t*> frames;
    std::vector<uint32_t> lens;
    void add(uint64_t i, const uint8_t* f, uint32_t l) {
        index.push_back(i);
        frames.push_back(f);
        lens.push_back(l);
    }
};

}  // namespace

bool scrub_entries(const uint8_t* log, uint64_t log_size, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                   const ScrubLedgers& t, int32_t* status, uint64_t* first_bad) {
    bool unreadable = false;
    Members crc[2], mac;
    std::vector<uint32_t> mac_rows;
    std::vector<int64_t> mac_lids;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t o = offsets[i];
        const uint32_t l = lengths[i];
        int32_t st = BKD_VERIFY_NOT_CHECKED;
        if (!(o <= log_size && (uint64_t)l <= log_size - o)) {
            st = 1;
            unreadable = true;
        } else if (l < 8u) {
            st = 1;
        } else {
            const uint8_t* f = log + o;
            uint64_t be = 0;
            for (int k = 0; k < 8; ++k) be = (be << 8) | f[k];
            const int64_t lid = (int64_t)be;
            const int64_t r = scrub::lookup(t.ids, t.nledgers, lid);
            const uint32_t type = r >= 0 ? t.types[r] : 4u;
            if (type <= 3u && ((t.mask >> type) & 1u)) {
                if (type == scrub::kDummy) {
                    st = l >= 32u ? 0 : 1;
                } else if (type == scrub::kHmac) {
                    const uint32_t k = t.keys[r];
                    if (k >= t.nkeys || l > BKD_MAC_MAX_ENTRY) {
                        st = 1;
                        unreadable = true;
                    } else if (l < kMacFrameHead) {
                        st = 1;
                    } else {
                        mac.add(i, f, l);
                        mac_rows.push_back(k);
                        mac_lids.push_back(lid);
                    }
                } else {
                    crc[type].add(i, f, l);
                }
            }
        }
        status[i] = st;
    }
    std::vector<int32_t> st;
    for (int algo = 0; algo < 2; ++algo) {
        const Members& m = crc[algo];
        const uint64_t k = m.index.size();
        if (!k) continue;
        st.assign(k, 0);
        verify_frames(algo, 0, 0, 2, m.frames.data(), m.lens.data(), k, st.data());  // digest only, as the scrub
        for (uint64_t j = 0; j < k; ++j) status[m.index[j]] = st[j];
    }
    // HMAC: the frame against its own ledger id, the entry id not looked at, the key of its table row
    constexpr uint64_t kPiece = 1u << 30;  // the request word keeps 31 bits for an index
    for (uint64_t j0 = 0; j0 < mac.index.size(); j0 += kPiece) {
        const uint64_t k = std::min<uint64_t>(kPiece, mac.index.size() - j0);
        std::vector<uint32_t> req(k);
        for (uint64_t j = 0; j < k; ++j) req[j] = (uint32_t)j | kSkipEntryId;
        st.assign(k, 0);
        mac_verify_frames_expected(t.key_states, mac_rows.data() + j0, mac_lids.data() + j0, mac_lids.data() + j0,
                                   req.data(), mac.frames.data() + j0, mac.lens.data() + j0, k, st.data());
        for (uint64_t j = 0; j < k; ++j) status[mac.index[j0 + j]] = st[j];
    }
    uint64_t fb = n;
    for (uint64_t i = 0; i < n; ++i)
        if (status[i] > 0) {
            fb = i;
            break;
        }
    *first_bad = fb;
    return unreadable;
}

void scrub_report(const uint8_t* log, uint64_t log_size, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                  const ScrubLedgers& t, const int32_t* status, uint64_t* report, uint32_t* bad, uint64_t capacity,
                  uint64_t* nbad) {
    for (uint64_t r = 0; r <= t.nledgers; ++r)
        for (uint32_t w = 0; w < scrub::kReportWords; ++w) report[r * scrub::kReportWords + w] = scrub::initial_word(w, n);
    uint64_t found = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t o = offsets[i];
        const uint32_t l = lengths[i];
        const bool in_log = scrub::in_range(o, l, log_size);
        int64_t looked_up = -1;
        if (scrub::has_ledger_id(in_log, l)) {
            uint64_t be = 0;
            for (int k = 0; k < 8; ++k) be = (be << 8) | log[o + k];
            looked_up = scrub::lookup(t.ids, t.nledgers, (int64_t)be);
        }
        uint64_t* r = report + scrub::report_row(looked_up, t.nledgers) * scrub::kReportWords;
        const uint32_t word = scrub::status_word(status[i]);
        r[BKD_REPORT_ENTRIES] += 1;
        r[BKD_REPORT_BYTES] += scrub::report_bytes(l);
        r[word] += 1;
        if (word != BKD_REPORT_BAD) continue;
        if (found < capacity) bad[found] = (uint32_t)i;
        ++found;
        if (i < r[BKD_REPORT_FIRST_BAD_INDEX]) r[BKD_REPORT_FIRST_BAD_INDEX] = i;
        if (scrub::has_entry_id(in_log, l)) {
            uint64_t be = 0;
            for (int k = 8; k < 16; ++k) be = (be << 8) | log[o + k];
            const int64_t eid = (int64_t)be;
            if (eid < (int64_t)r[BKD_REPORT_MIN_BAD_ENTRY]) r[BKD_REPORT_MIN_BAD_ENTRY] = (uint64_t)eid;
            if (eid > (int64_t)r[BKD_REPORT_MAX_BAD_ENTRY]) r[BKD_REPORT_MAX_BAD_ENTRY] = (uint64_t)eid;
        }
    }
    *nbad = found;
}

LedgersMap read_ledgers_map(const uint8_t* log, uint64_t log_size, int64_t* ledger_ids, int64_t* sizes,
                            uint64_t capacity) {
    LedgersMap m;
    auto be32 = [&](uint64_t at) {
        return (int32_t)(((uint32_t)log[at] << 24) | ((uint32_t)log[at + 1] << 16) | ((uint32_t)log[at + 2] << 8) |
                         (uint32_t)log[at + 3]);
    };
    auto be64 = [&](uint64_t at) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v = (v << 8) | log[at + k];
        return (int64_t)v;
    };
    auto malformed = [&](const char* why) {
        m.state = BKD_LEDGERS_MAP_MALFORMED;
        m.why = why;
        return m;
    };
    if (log_size < 20) return malformed("short read of the log header");
    m.version = be32(4);
    m.map_offset = be64(8);
    m.ledgers_count = be32(16);
    if (m.version < 1 || m.map_offset == 0) {
        m.state = BKD_LEDGERS_MAP_ABSENT;
        return m;
    }
    if (m.map_offset < 0) return malformed("short read: a negative ledgers map offset");
    std::vector<int64_t> seen;
    uint64_t offset = (uint64_t)m.map_offset;
    while (offset < log_size) {
        if (log_size - offset < 4) return malformed("short read of a record's size");
        const int32_t map_size = be32(offset);
        if (map_size <= 0) break;
        const uint64_t body = offset + 4, len = (uint64_t)map_size;
        if (len > log_size - body) return malformed("short read: a record cut by the end of the buffer");
        // inside the record, in the order the reference reads it
        if (len < 8) return malformed("a record shorter than its fields");
        if (be64(body) != -1) return malformed("a record's ledger id is not -1");
        if (len < 16) return malformed("a record shorter than its fields");
        if (be64(body + 8) != -2) return malformed("a record's entry id is not -2");
        if (len < 20) return malformed("a record shorter than its fields");
        const int32_t count = be32(body + 16);
        uint64_t at = 20;
        for (int32_t k = 0; k < count; ++k, at += 16) {
            if (len - at < 16) return malformed("a record shorter than its count implies");
            const int64_t lid = be64(body + at), sz = be64(body + at + 8);
            if (m.count < capacity) {
                ledger_ids[m.count] = lid;
                sizes[m.count] = sz;
            } else {
                m.over = true;
            }
            ++m.count;
            seen.push_back(lid);
        }
        if (at != len) return malformed("a record longer than its count implies");
        offset = body + len;
    }
    std::sort(seen.begin(), seen.end());
    const uint64_t distinct = (uint64_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
    if ((int64_t)distinct != (int64_t)m.ledgers_count)
        return malformed("the distinct ledgers of the map are not as many as the header's count");
    if (m.ledgers_count == 0) return malformed("a header count of 0");
    return m;
}

}  // namespace host
}  // namespace bkd
