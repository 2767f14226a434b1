// The CPU route of the mixed-ledger entry-log scrub (bkd_entrylog_verify_ledgers_host): per entry on the
// host pool, with the table lookup the device runs (scrub_rules.hpp), host_batch.cpp's verify
// arithmetic for the CRC types and host_mac.cpp's for HMAC. Plain C++; needs no device.
#pragma once
#include <stdint.h>

namespace bkd {
namespace host {

// The ledger table of a scrub call in host memory (include/bkdigest.h).
struct ScrubLedgers {
    const int64_t* ids;
    const uint32_t* types;
    const uint32_t* keys;  // may be null when the HMAC bit of `mask` is clear
    uint64_t nledgers;
    const uint32_t* key_states;
    uint64_t nkeys;
    uint32_t mask;
};

// 0 when ids ascend strictly and every HMAC row's key index is < nkeys (rows of other types are not
// looked at), else 1 + the first offending row.
uint64_t scrub_table_check(const ScrubLedgers& t);

// status[i] for every entry as the device call decides it; *first_bad = the lowest index with a status
// above 0, n when none. Returns true when some entry was unreadable (out of range, over
// BKD_MAC_MAX_ENTRY or keyed outside the table): what raises the bounds flag on the device.
bool scrub_entries(const uint8_t* log, uint64_t log_size, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                   const ScrubLedgers& t, int32_t* status, uint64_t* first_bad);

// The report of bkd_entrylog_scrub_report from the statuses above, one serial pass with the rules the device
// applies (scrub_report_rules.hpp): report[(nledgers + 1) x 8], bad[0, min(*nbad, capacity)) ascending.
void scrub_report(const uint8_t* log, uint64_t log_size, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                  const ScrubLedgers& t, const int32_t* status, uint64_t* report, uint32_t* bad, uint64_t capacity,
                  uint64_t* nbad);

// What bkd_entrylog_ledgers_map reads (include/bkdigest.h). `why` names the case of a malformed map.
struct LedgersMap {
    int32_t version = 0;
    int64_t map_offset = 0;
    int32_t ledgers_count = 0;
    int32_t state = 0;     // BKD_LEDGERS_MAP_*
    uint64_t count = 0;    // pairs written
    bool over = false;     // more pairs than the capacity
    const char* why = "";
};
LedgersMap read_ledgers_map(const uint8_t* log, uint64_t log_size, int64_t* ledger_ids, int64_t* sizes,
                            uint64_t capacity);

}  // namespace host
}  // namespace bkd
