// Stand-alone program for tests/test_mac_reframe_cpu.py: host_mac.cpp's reframe walker
// (mac_reframe_frames_expected) and sha1::compress2 under AddressSanitizer and UBSan. Frames of 0, 51, 52,
// 53, 75, 76 and 4 148 bytes, each in a heap buffer that ends exactly where the frame ends and starts 0..3
// bytes behind the allocation, so a read or write past a frame is a heap overflow the sanitizer reports.
// Prints one line per re-framed frame, "mode offset length lac head-hex" (head: the 52 bytes in front of
// the payload), for the test to compare with hmac; frames too short for a MAC must come back untouched.
// Then compress2(hA, hB, w) against two compress calls on 1 000 random blocks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bookkeeper_amd/csrc/host_batch.hpp"
#include "../bookkeeper_amd/csrc/host_mac.hpp"
#include "../bookkeeper_amd/csrc/mac_sha1.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

int main() {
    using namespace bkd::host;
    const uint32_t flens_all[] = {0, 51, 52, 53, 75, 76, 4148};
    enum { NLEN = 7, NOFF = 4, N = NLEN * NOFF, NKEYS = 2 };
    uint32_t table[NKEYS * 10];
    mac_key_init((const uint8_t*)"pw0", 3, table);
    mac_key_init((const uint8_t*)"pw1", 3, table + 10);
    const uint32_t req_keys[2] = {1, 0};

    int bad = 0;
    for (int trusted = 0; trusted < 2; ++trusted) {
        uint8_t *bufs[N], *frames[N], *before[N];
        uint32_t flens[N], req_of[N];
        int64_t lids[N], eids[N], lacs[N];
        for (int i = 0; i < N; ++i) {
            const uint32_t l = flens_all[i / NOFF], off = (uint32_t)(i % NOFF);
            flens[i] = l;
            req_of[i] = (uint32_t)(i & 1);
            lids[i] = 7000 + (i & 1);
            eids[i] = 100 + i;
            lacs[i] = i % 5 == 0 ? -1 : ((int64_t)1 << 40) + i;
            bufs[i] = (uint8_t*)malloc(l + off ? l + off : 1);
            frames[i] = bufs[i] + off;
            before[i] = (uint8_t*)malloc(l ? l : 1);
            uint8_t whole[52 + 4096];
            const uint32_t plen = l >= 52 ? l - 52 : 0;
            for (uint32_t b = 0; b < plen; ++b) whole[52 + b] = (uint8_t)(b * 131u + l * 7u + (uint32_t)i);
            const uint32_t key_of = req_keys[i & 1];
            const int64_t lac0 = eids[i] - 1, lf = plen;
            const uint8_t* payload = whole + 52;
            mac_package_frames_ledgers(table, &key_of, &lids[i], &eids[i], &lac0, &lf, &payload, &plen, 1, whole, 52);
            memcpy(frames[i], whole, l);  // a frame under 52 bytes is a cut head
            memcpy(before[i], frames[i], l);
        }
        int32_t status[N];
        mac_reframe_frames_expected(table, req_keys, lids, eids, req_of, trusted != 0, frames, flens, N, lacs, status);
        for (int i = 0; i < N; ++i) {
            if (flens[i] < 52) {
                bad |= status[i] != 1 || memcmp(frames[i], before[i], flens[i]) != 0;
                continue;
            }
            bad |= status[i] != 0;
            bad |= memcmp(frames[i] + 52, before[i] + 52, flens[i] - 52) != 0;
            printf("%d %d %u %lld ", trusted, i % NOFF, flens[i], (long long)lacs[i]);
            for (int b = 0; b < 52; ++b) printf("%02x", frames[i][b]);
            printf("\n");
        }
        // the reframed frames verify, and reframing them for the same LAC again changes nothing
        int32_t again[N];
        mac_verify_frames_expected(table, req_keys, lids, eids, req_of, (const uint8_t* const*)frames, flens, N, again);
        for (int i = 0; i < N; ++i) bad |= again[i] != (flens[i] < 52 ? 1 : 0);
        for (int i = 0; i < N; ++i) memcpy(before[i], frames[i], flens[i]);
        mac_reframe_frames_expected(table, req_keys, lids, eids, req_of, trusted != 0, frames, flens, N, lacs, status);
        for (int i = 0; i < N; ++i) bad |= memcmp(frames[i], before[i], flens[i]) != 0;
        for (int i = 0; i < N; ++i) {
            free(bufs[i]);
            free(before[i]);
        }
    }
    printf("reframe %s\n", bad ? "mismatch" : "ok");

    int bad2 = 0;
    for (int it = 0; it < 1000; ++it) {
        uint32_t w[16], w1[16], w2[16], ha[5], hb[5], xa[5], xb[5];
        for (int t = 0; t < 16; ++t) w[t] = w1[t] = w2[t] = rnd();
        for (int k = 0; k < 5; ++k) {
            ha[k] = xa[k] = rnd();
            hb[k] = xb[k] = rnd();
        }
        bkd::sha1::compress2(ha, hb, w);
        bkd::sha1::compress(xa, w1);
        bkd::sha1::compress(xb, w2);
        for (int k = 0; k < 5; ++k) bad2 |= ha[k] != xa[k] || hb[k] != xb[k];
        for (int t = 0; t < 16; ++t) bad2 |= w[t] != w1[t];
    }
    printf("compress2 %s\n", bad2 ? "mismatch" : "ok");
    return (bad || bad2) ? 1 : 0;
}
