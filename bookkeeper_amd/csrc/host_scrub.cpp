// The CPU route of the mixed-ledger entry-log scrub (host_scrub.hpp).
#include "host_scrub.hpp"

#include <algorithm>
#include <vector>

#include "../../include/bkdigest.h"
#include "host_batch.hpp"
#include "host_mac.hpp"
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

}  // namespace host
}  // namespace bkd
