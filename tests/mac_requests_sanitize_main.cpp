// Stand-alone program for tests/test_mac_requests_cpu.py: host_mac.cpp's two many-ledger batch walkers
// (mac_package_frames_ledgers, mac_verify_frames_expected) under AddressSanitizer and UBSan. Requests with
// empty, 1-byte and block-edge entries, every payload, every frame and every index array allocated to its
// exact length, so a read past an entry, a row past the key table or an index past an array is a heap
// overflow the sanitizer reports. Prints one line per entry: "i request key-row length mac-hex", for the
// test to compare with hmac; then verifies the frames it made.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bookkeeper_amd/csrc/host_batch.hpp"
#include "../bookkeeper_amd/csrc/host_mac.hpp"

template <class T>
static T* exact(size_t count) {
    return (T*)malloc(count ? count * sizeof(T) : 1);
}

int main() {
    using namespace bkd::host;
    // payload lengths: with the 32-byte header in front, 23 / 24 is where the padding takes a second block
    // and 32 and 96 are where the message ends on a block edge
    const uint32_t lens_all[] = {0, 1, 23, 24, 31, 32, 33, 63, 64, 65, 87, 88, 95, 96, 97, 119, 120, 200, 0, 1, 64};
    const uint64_t sizes[] = {0, 5, 1, 0, 9, 6, 0};  // requests, empty ones first, in the middle and last
    enum { NREQ = 7, NKEYS = 3 };
    const uint64_t n = sizeof(lens_all) / sizeof(lens_all[0]);

    uint32_t* table = exact<uint32_t>(NKEYS * 10);
    for (int k = 0; k < NKEYS; ++k) {
        char pw[8];
        snprintf(pw, sizeof(pw), "pw%d", k);
        mac_key_init((const uint8_t*)pw, strlen(pw), table + 10 * k);
    }
    uint32_t* req_keys = exact<uint32_t>(NREQ);
    for (int r = 0; r < NREQ; ++r) req_keys[r] = (uint32_t)((r * 2 + 1) % NKEYS);

    uint32_t* lens = exact<uint32_t>(n);
    uint32_t *key_of = exact<uint32_t>(n), *req_of = exact<uint32_t>(n);
    int64_t *lids = exact<int64_t>(n), *eids = exact<int64_t>(n), *lacs = exact<int64_t>(n), *lfs = exact<int64_t>(n);
    uint8_t** payloads = exact<uint8_t*>(n);
    uint64_t i = 0;
    for (int r = 0; r < NREQ; ++r)
        for (uint64_t j = 0; j < sizes[r]; ++j, ++i) {
            lens[i] = lens_all[i];
            key_of[i] = req_keys[r];
            req_of[i] = (uint32_t)r | (r == 4 ? kSkipEntryId : 0u);
            lids[i] = 1000 + r;
            eids[i] = 10 * r + (int64_t)i;
            lacs[i] = (int64_t)i - 1;
            lfs[i] = lens[i];
            payloads[i] = exact<uint8_t>(lens[i]);
            for (uint32_t b = 0; b < lens[i]; ++b) payloads[i][b] = (uint8_t)(b * 131u + lens[i] * 7u + i);
        }
    if (i != n) return 2;

    uint8_t* heads = exact<uint8_t>(n * 52);
    mac_package_frames_ledgers(table, key_of, lids, eids, lacs, lfs, (const uint8_t* const*)payloads, lens, n, heads, 52);
    for (i = 0; i < n; ++i) {
        printf("%llu %u %u %u ", (unsigned long long)i, req_of[i] & ~kSkipEntryId, key_of[i], lens[i]);
        for (int b = 0; b < 20; ++b) printf("%02x", heads[52 * i + 32 + b]);
        printf("\n");
    }

    // the frames whole, each its own exact allocation; request 4 skips the entry-id check and its entry ids
    // are off by one, one frame of request 5 has a flipped last byte, one of request 1 is cut to 51 bytes
    uint8_t** frames = exact<uint8_t*>(n);
    uint32_t* flens = exact<uint32_t>(n);
    int32_t* want = exact<int32_t>(n);
    for (i = 0; i < n; ++i) {
        flens[i] = 52 + lens[i];
        want[i] = 0;
        if (i == 2) {
            flens[i] = 51;
            want[i] = 1;
        }
        frames[i] = exact<uint8_t>(flens[i]);
        memcpy(frames[i], heads + 52 * i, flens[i] < 52 ? flens[i] : 52);
        if (flens[i] > 52) memcpy(frames[i] + 52, payloads[i], lens[i]);
        if ((req_of[i] & ~kSkipEntryId) == 4) eids[i] += 1;
        if (i == n - 2) {
            frames[i][flens[i] - 1] ^= 1;
            want[i] = 2;
        }
    }
    int32_t* status = exact<int32_t>(n);
    mac_verify_frames_expected(table, req_keys, lids, eids, req_of, (const uint8_t* const*)frames, flens, n, status);
    int bad = 0;
    for (i = 0; i < n; ++i) bad |= status[i] != want[i];
    // the same frames against a neighbouring key row: every frame long enough to have a MAC fails on it
    for (int r = 0; r < NREQ; ++r) req_keys[r] = (req_keys[r] + 1) % NKEYS;
    mac_verify_frames_expected(table, req_keys, lids, eids, req_of, (const uint8_t* const*)frames, flens, n, status);
    for (i = 0; i < n; ++i) bad |= status[i] != (flens[i] < 52 ? 1 : 2);

    for (i = 0; i < n; ++i) {
        free(payloads[i]);
        free(frames[i]);
    }
    void* all[] = {table, req_keys, lens, key_of, req_of, lids, eids, lacs, lfs, payloads, heads, frames, flens, want, status};
    for (void* p : all) free(p);
    printf("verify %s\n", bad ? "mismatch" : "ok");
    return bad ? 1 : 0;
}
