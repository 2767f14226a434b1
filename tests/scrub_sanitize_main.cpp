// Stand-alone program for tests/test_scrub_ledgers_cpu.py: the table lookup and the bin rule
// (scrub_rules.hpp) and the scrub's CPU route (host_scrub.cpp), built with -fsanitize=address,undefined.
// Every array is copied into an allocation of exactly its size, so a read past an entry, the log or a
// table row is reported. Input: a case file the test writes —
//   u64 log_size, n, nledgers, nkeys, mask, nprobes; then log bytes, offsets u64[n], lengths u32[n],
//   ids i64[nledgers], types u32[nledgers], keys u32[nledgers], key states u32[10 nkeys], probes i64[nprobes].
// Output: "status <first_bad> <unreadable> s0 s1 ...", "lookup r0 r1 ...", "bins <xor-sum over 52..70000> <bin at the cap>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../bookkeeper_amd/csrc/host_scrub.hpp"
#include "../bookkeeper_amd/csrc/scrub_rules.hpp"

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
    uint64_t h[6];
    if (fread(h, 8, 6, f) != 6) return 2;
    const uint64_t log_size = h[0], n = h[1], nledgers = h[2], nkeys = h[3], nprobes = h[5];
    const uint32_t mask = (uint32_t)h[4];
    uint8_t* log = exact<uint8_t>(f, log_size);
    uint64_t* offsets = exact<uint64_t>(f, n);
    uint32_t* lengths = exact<uint32_t>(f, n);
    int64_t* ids = exact<int64_t>(f, nledgers);
    uint32_t* types = exact<uint32_t>(f, nledgers);
    uint32_t* keys = exact<uint32_t>(f, nledgers);
    uint32_t* states = exact<uint32_t>(f, nkeys * 10);
    int64_t* probes = exact<int64_t>(f, nprobes);
    fclose(f);

    const bkd::host::ScrubLedgers t{ids, types, keys, nledgers, states, nkeys, mask};
    if (bkd::host::scrub_table_check(t)) return 3;
    int32_t* status = (int32_t*)malloc(n ? n * 4 : 1);
    uint64_t first_bad = 0;
    const bool unreadable = bkd::host::scrub_entries(log, log_size, offsets, lengths, n, t, status, &first_bad);
    printf("status %llu %d", (unsigned long long)first_bad, (int)unreadable);
    for (uint64_t i = 0; i < n; ++i) printf(" %d", status[i]);
    printf("\nlookup");
    for (uint64_t k = 0; k < nprobes; ++k) printf(" %lld", (long long)bkd::scrub::lookup(ids, nledgers, probes[k]));
    uint32_t x = 0;
    for (uint32_t l = 52; l <= 70000; ++l) x ^= bkd::scrub::bin(l) * (l | 1u);
    printf("\nbins %u %u\n", x, bkd::scrub::bin(16u << 20));
    for (void* p : {(void*)log, (void*)offsets, (void*)lengths, (void*)ids, (void*)types, (void*)keys, (void*)states,
                    (void*)probes, (void*)status})
        free(p);
    return 0;
}
