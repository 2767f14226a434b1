// Stand-alone program for tests/test_mac_adds_cpu.py: the segment walker the composite MAC kernel runs
// (mac_segments.hpp) and the CPU route over it (host_mac.cpp), built with -fsanitize=address,undefined.
// Every segment is its own exact-size heap allocation, so a byte read in front of or behind a segment
// is a heap-buffer-overflow. Prints one line per case for the test to compare with Python's hmac:
//   "cut L c mac"    entry of L bytes cut into [0, c) and [c, L), header (L, c, -1, L), L in 0..140
//   "leaves mac"     70 one-byte segments with empty ones at head, middle and tail, header (7, 8, 9, 70)
// and "batch ok" once the CPU route over all of them as one batch gave the same frames.
// Byte k of an entry of L bytes is (k * 131 + L * 7) & 0xFF.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../bookkeeper_amd/csrc/host_mac.hpp"

namespace {

void put_be64(uint8_t* p, uint64_t v) {
    for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (56 - 8 * k));
}

struct Batch {
    std::vector<std::unique_ptr<uint8_t[]>> owned;
    std::vector<const uint8_t*> ptrs;
    std::vector<uint32_t> lens;
    std::vector<uint64_t> first{0};
    std::vector<int64_t> lids, eids, lacs, lfs;
    // one segment = bytes [from, from + len) of the entry of L bytes, in an allocation of exactly len bytes
    void segment(uint32_t L, uint32_t from, uint32_t len) {
        uint8_t* p = nullptr;
        if (len) {
            owned.emplace_back(new uint8_t[len]);
            p = owned.back().get();
            for (uint32_t k = 0; k < len; ++k) p[k] = (uint8_t)(((from + k) * 131u + L * 7u) & 0xFFu);
        }
        ptrs.push_back(p);
        lens.push_back(len);
    }
    void end_entry(int64_t lid, int64_t eid, int64_t lac, int64_t lf) {
        first.push_back(ptrs.size());
        lids.push_back(lid);
        eids.push_back(eid);
        lacs.push_back(lac);
        lfs.push_back(lf);
    }
};

void hex(const uint8_t* p, int n) {
    for (int k = 0; k < n; ++k) printf("%02x", p[k]);
}

}  // namespace

int main() {
    const uint8_t passwd[] = "testPasswd";
    uint32_t ks[10];
    bkd::host::mac_key_init(passwd, 10, ks);
    Batch b;
    for (uint32_t L = 0; L <= 140; ++L)
        for (uint32_t c = 0; c <= L; ++c) {
            b.segment(L, 0, c);
            b.segment(L, c, L - c);
            b.end_entry(L, c, -1, L);
        }
    const uint64_t leaves_at = b.lids.size();
    b.segment(70, 0, 0);
    for (uint32_t k = 0; k < 70; ++k) {
        b.segment(70, k, 1);
        if (k == 30 || k == 31) b.segment(70, k, 0);
    }
    b.segment(70, 70, 0);
    b.end_entry(7, 8, 9, 70);
    const uint64_t n = b.lids.size();

    // the walker, entry by entry
    std::vector<uint8_t> want(n * 52);
    for (uint64_t i = 0; i < n; ++i) {
        uint8_t* f = want.data() + i * 52;
        put_be64(f, (uint64_t)b.lids[i]);
        put_be64(f + 8, (uint64_t)b.eids[i]);
        put_be64(f + 16, (uint64_t)b.lacs[i]);
        put_be64(f + 24, (uint64_t)b.lfs[i]);
        bkd::host::mac_one_segments(ks, f, b.ptrs.data(), b.lens.data(), b.first[i], b.first[i + 1], f + 32);
        if (i < leaves_at) printf("cut %lld %lld ", (long long)b.lids[i], (long long)b.eids[i]);
        else printf("leaves ");
        hex(f + 32, 20);
        printf("\n");
    }

    // the CPU route over the whole batch, frames at a stride of 64 with sentinels between them
    std::vector<uint32_t> entry_lens(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t sum = 0;
        for (uint64_t k = b.first[i]; k < b.first[i + 1]; ++k) sum += b.lens[k];
        entry_lens[i] = (uint32_t)sum;
    }
    std::vector<uint8_t> frames(n * 64, 0xEE);
    bkd::host::mac_package_frames_segments(ks, nullptr, 0, b.lids.data(), b.eids.data(), b.lacs.data(), b.lfs.data(),
                                           b.ptrs.data(), b.lens.data(), b.first.data(), entry_lens.data(), n,
                                           frames.data(), 64);
    for (uint64_t i = 0; i < n; ++i) {
        if (memcmp(frames.data() + i * 64, want.data() + i * 52, 52) != 0) {
            printf("batch differs at %llu\n", (unsigned long long)i);
            return 1;
        }
        for (int k = 52; k < 64; ++k)
            if (frames[i * 64 + k] != 0xEE) {
                printf("batch wrote behind frame %llu\n", (unsigned long long)i);
                return 1;
            }
    }
    printf("batch ok\n");
    return 0;
}
