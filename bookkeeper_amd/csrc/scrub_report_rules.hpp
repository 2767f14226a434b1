// The rules of the scrub report (bkd_entrylog_scrub_report) that the device kernels
// (scrub_report_kernels.hpp) and the host route (host_scrub.cpp) share, the way scrub_rules.hpp is shared:
// which row of the report an entry belongs to, when its entry id is read, what a row starts as and what a
// status adds to which word. Plain C++: no host or device calls.
#pragma once
#include <stdint.h>

#include "../../include/bkdigest.h"
#include "scrub_rules.hpp"

namespace bkd {
namespace scrub {

constexpr uint32_t kReportWords = BKD_SCRUB_REPORT_WORDS;

// An entry inside the log: what scrub_classify_kernel checks before it reads a byte.
BKD_HD bool in_range(uint64_t offset, uint32_t length, uint64_t log_size) {
    return offset <= log_size && (uint64_t)length <= log_size - offset;
}

// The ledger id is read from an entry that is in range and at least 8 bytes long; everyone else, and an
// id that the table does not list (lookup() == -1), belongs to the catch-all row nledgers.
BKD_HD bool has_ledger_id(bool in_log, uint32_t length) { return in_log && length >= 8u; }
BKD_HD uint64_t report_row(int64_t looked_up, uint64_t nledgers) {
    return looked_up >= 0 ? (uint64_t)looked_up : nledgers;
}

// The entry id (bytes [8, 16), big-endian) is read only from an entry that is in range and holds all of it.
BKD_HD bool has_entry_id(bool in_log, uint32_t length) { return in_log && length >= 16u; }

// What an entry adds to BKD_REPORT_BYTES: the reference's readableBytes() + 4, the record's size field.
BKD_HD uint64_t report_bytes(uint32_t length) { return (uint64_t)length + 4u; }

// The count word a status belongs to: above 0 bad, 0 ok, below 0 (BKD_VERIFY_NOT_CHECKED) not checked.
BKD_HD uint32_t status_word(int32_t status) {
    return status > 0 ? (uint32_t)BKD_REPORT_BAD : status == 0 ? (uint32_t)BKD_REPORT_OK : (uint32_t)BKD_REPORT_NOT_CHECKED;
}

// A row before any entry: zeros, INT64_MAX / INT64_MIN as bits, first bad index n.
BKD_HD uint64_t initial_word(uint32_t w, uint64_t n) {
    return w == BKD_REPORT_MIN_BAD_ENTRY ? (uint64_t)INT64_MAX
           : w == BKD_REPORT_MAX_BAD_ENTRY ? (uint64_t)INT64_MIN
           : w == BKD_REPORT_FIRST_BAD_INDEX ? n
                                             : 0u;
}

}  // namespace scrub
}  // namespace bkd
