// Stand-alone program for tests/test_scrub_report_cpu.py: the scrub report's shared rules
// (scrub_report_rules.hpp), the CPU route's report pass and the ledgers-map reader (host_scrub.cpp), built with
// -fsanitize=address,undefined. Every array is copied into an allocation of exactly its size, so a read past an
// entry, the log, a table row or a map record is reported. Input: a case file the test writes —
//   u64 log_size, n, nledgers, nkeys, mask, capacity, map_log_size; then log bytes, offsets u64[n], lengths u32[n],
//   ids i64[nledgers], types u32[nledgers], keys u32[nledgers], key states u32[10 nkeys], the map log's bytes.
// Output: "report w0 w1 ..." (unsigned words), "bad <nbad> i0 i1 ...", "map <state> <count> l0 s0 l1 s1 ...",
// "prefixes s1024 s1025 ..." (the state of every prefix of the map log from its 1024-byte header on).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../bookkeeper_amd/csrc/host_scrub.hpp"
#include "../bookkeeper_amd/csrc/scrub_report_rules.hpp"

template <class T>
static T* exact(FILE* f, uint64_t count) {  // an allocation of exactly count elements (none: one byte, unused)
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[7];
    if (fread(h, 8, 7, f) != 7) return 2;
    const uint64_t log_size = h[0], n = h[1], nledgers = h[2], nkeys = h[3], capacity = h[5], map_size = h[6];
    const uint32_t mask = (uint32_t)h[4];
    uint8_t* log = exact<uint8_t>(f, log_size);
    uint64_t* offsets = exact<uint64_t>(f, n);
    uint32_t* lengths = exact<uint32_t>(f, n);
    int64_t* ids = exact<int64_t>(f, nledgers);
    uint32_t* types = exact<uint32_t>(f, nledgers);
    uint32_t* keys = exact<uint32_t>(f, nledgers);
    uint32_t* states = exact<uint32_t>(f, nkeys * 10);
    uint8_t* map_log = exact<uint8_t>(f, map_size);
    fclose(f);

    const bkd::host::ScrubLedgers t{ids, types, keys, nledgers, states, nkeys, mask};
    if (bkd::host::scrub_table_check(t)) return 3;
    int32_t* status = (int32_t*)malloc(n ? n * 4 : 1);
    uint64_t first_bad = 0;
    (void)bkd::host::scrub_entries(log, log_size, offsets, lengths, n, t, status, &first_bad);
    const uint64_t words = (nledgers + 1) * bkd::scrub::kReportWords;
    uint64_t* report = (uint64_t*)malloc(words * 8);
    uint32_t* bad = (uint32_t*)malloc(capacity ? capacity * 4 : 1);
    uint64_t nbad = 0;
    bkd::host::scrub_report(log, log_size, offsets, lengths, n, t, status, report, bad, capacity, &nbad);
    printf("report");
    for (uint64_t w = 0; w < words; ++w) printf(" %llu", (unsigned long long)report[w]);
    printf("\nbad %llu", (unsigned long long)nbad);
    for (uint64_t k = 0; k < capacity && k < nbad; ++k) printf(" %u", bad[k]);

    const uint64_t pairs = map_size / 16;  // more than the map can hold
    int64_t* lids = (int64_t*)malloc(pairs ? pairs * 8 : 1);
    int64_t* sizes = (int64_t*)malloc(pairs ? pairs * 8 : 1);
    const bkd::host::LedgersMap m = bkd::host::read_ledgers_map(map_log, map_size, lids, sizes, pairs);
    printf("\nmap %d %llu", m.state, (unsigned long long)m.count);
    for (uint64_t k = 0; k < m.count; ++k) printf(" %lld %lld", (long long)lids[k], (long long)sizes[k]);
    printf("\nprefixes");
    for (uint64_t cut = 1024; cut <= map_size; ++cut) {  // each prefix in an allocation of exactly its size
        uint8_t* part = (uint8_t*)malloc(cut);
        memcpy(part, map_log, cut);
        printf(" %d", bkd::host::read_ledgers_map(part, cut, lids, sizes, pairs).state);
        free(part);
    }
    printf("\n");
    for (void* p : {(void*)log, (void*)offsets, (void*)lengths, (void*)ids, (void*)types, (void*)keys, (void*)states,
                    (void*)map_log, (void*)status, (void*)report, (void*)bad, (void*)lids, (void*)sizes})
        free(p);
    return 0;
}
