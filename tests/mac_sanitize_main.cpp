// Stand-alone program for tests/test_mac_cpu.py: host_mac.cpp's SHA-1 / HMAC under AddressSanitizer and
// UBSan. Every length 0..200 is hashed from a heap buffer allocated at exactly the bytes used, at byte
// offsets 0..3 inside it, so a read at or past the entry's end is a heap overflow the sanitizer reports.
// Prints one line per (offset, length): the MAC in hex, for the test to compare with hmac.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../bookkeeper_amd/csrc/host_mac.hpp"

int main() {
    uint32_t ks[10];
    bkd::host::mac_key_init((const uint8_t*)"testPasswd", 10, ks);
    for (unsigned off = 0; off < 4; ++off) {
        for (unsigned len = 0; len <= 200; ++len) {
            uint8_t* buf = (uint8_t*)malloc(off + len ? off + len : 1);
            for (unsigned k = 0; k < off + len; ++k) buf[k] = (uint8_t)(k * 131u + len * 7u + off);
            uint8_t mac[20], fmac[20];
            bkd::host::mac_one(ks, nullptr, 0, buf + off, len, mac);
            // the framed form: a 32-byte prefix from its own exact allocation
            uint8_t* pre = (uint8_t*)malloc(32);
            memset(pre, (int)len, 32);
            bkd::host::mac_one(ks, pre, 32, buf + off, len, fmac);
            printf("%u %u ", off, len);
            for (int k = 0; k < 20; ++k) printf("%02x", mac[k]);
            printf(" ");
            for (int k = 0; k < 20; ++k) printf("%02x", fmac[k]);
            printf("\n");
            free(pre);
            free(buf);
        }
    }
    // the batch walkers over the host pool, exact allocations again
    enum { N = 64 };
    uint8_t* bufs[N];
    const uint8_t* ptrs[N];
    uint32_t lens[N];
    for (int i = 0; i < N; ++i) {
        lens[i] = (uint32_t)(i * 37 % 500);
        bufs[i] = (uint8_t*)malloc(lens[i] ? lens[i] : 1);
        memset(bufs[i], i, lens[i]);
        ptrs[i] = bufs[i];
    }
    uint8_t* out = (uint8_t*)malloc(N * 20);
    bkd::host::mac_list(ks, ptrs, lens, N, out);
    uint8_t one[20];
    int bad = 0;
    for (int i = 0; i < N; ++i) {
        bkd::host::mac_one(ks, nullptr, 0, bufs[i], lens[i], one);
        bad |= memcmp(one, out + 20 * i, 20);
        free(bufs[i]);
    }
    free(out);
    printf("batch %s\n", bad ? "mismatch" : "ok");
    return bad ? 1 : 0;
}
