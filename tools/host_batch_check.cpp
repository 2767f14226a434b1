// Stand-alone sanitizer target for the CPU route of host-resident batches (host_batch.cpp over the
// host pool): crc_list, crc_indexed, package_frames, verify_frames, reframe_frames and apply_reframe
// on 5 000 entries, two of them >= 4 MiB, so both the chunks over the pool and the whole-pool fold of a
// long entry run, on 4 pool threads (BKD_HOST_THREADS=4); every result is compared with the same call
// on one thread (set_active(1)). No HIP, no Python, nothing preloaded; CPU only.
// Build (from the repository root), once per sanitizer, and run ./tools/host_batch_check:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -o tools/host_batch_check \
//       tools/host_batch_check.cpp bookkeeper_amd/csrc/host_batch.cpp bookkeeper_amd/csrc/host_crc.cpp
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o tools/host_batch_check \
//       tools/host_batch_check.cpp bookkeeper_amd/csrc/host_batch.cpp bookkeeper_amd/csrc/host_crc.cpp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../bookkeeper_amd/csrc/host_batch.hpp"

namespace bh = bkd::host;

static int g_failures = 0;

template <class T>
static void same(const char* what, int algo, const std::vector<T>& a, const std::vector<T>& b) {
    if (a == b) return;
    size_t i = 0;
    while (i < a.size() && a[i] == b[i]) ++i;
    fprintf(stderr, "MISMATCH %s (algo %d): first at %zu\n", what, algo, i);
    ++g_failures;
}

// f(threads) with the whole pool, then with one thread
template <class F>
static void both(F&& f) {
    bh::Pool::get().set_active(0);
    f(0);
    bh::Pool::get().set_active(1);
    f(1);
    bh::Pool::get().set_active(0);
}

int main() {
    setenv("BKD_HOST_THREADS", "4", 1);
    if (bh::Pool::get().threads() != 4) {
        fprintf(stderr, "pool has %d threads, expected 4\n", bh::Pool::get().threads());
        return 2;
    }
    const uint64_t n = 5000;
    std::vector<uint32_t> lens(n), seeds(n);
    std::vector<uint64_t> offs(n);
    uint64_t state = 0x9E3779B97F4A7C15ull, total = 0;
    auto rnd = [&] {
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        return state;
    };
    for (uint64_t i = 0; i < n; ++i) {
        lens[i] = (uint32_t)(rnd() % 3000);
        seeds[i] = (uint32_t)rnd();
    }
    lens[0] = 0, lens[1] = 1, lens[2] = 15, lens[3] = 16;
    lens[777] = (4u << 20) + 3;  // the two long entries: folded in pieces on the whole pool
    lens[4100] = (5u << 20) + 1;
    for (uint64_t i = 0; i < n; ++i) offs[i] = total, total += lens[i];
    std::vector<uint8_t> data(total);
    for (uint64_t i = 0; i + 8 <= total; i += 8) {
        const uint64_t v = rnd();
        memcpy(&data[i], &v, 8);
    }
    std::vector<const uint8_t*> ptrs(n);
    std::vector<int64_t> ids(n), lacs(n), lenf(n), new_lacs(n);
    for (uint64_t i = 0; i < n; ++i) {
        ptrs[i] = data.data() + offs[i];
        ids[i] = 100 + (int64_t)i, lacs[i] = ids[i] - 1, lenf[i] = (int64_t)offs[i], new_lacs[i] = ids[i] + 50;
    }
    for (int algo = 0; algo < 2; ++algo) {
        const uint32_t hl = 32u + bh::mac_len(algo);
        std::vector<uint32_t> out[2], idx[2], dig[2], rdig[2];
        std::vector<uint8_t> hdr[2];
        both([&](int k) {
            out[k].assign(n, 0), idx[k].assign(n, 0), dig[k].assign(n, 0), hdr[k].assign(n * hl, 0);
            bh::crc_list(algo, ptrs.data(), lens.data(), n, seeds.data(), 0, out[k].data());
            bh::crc_indexed(algo, data.data(), offs.data(), lens.data(), n, nullptr, 0x1234ABCDu, idx[k].data());
            bh::package_frames(algo, 7, ids.data(), lacs.data(), lenf.data(), ptrs.data(), lens.data(), n,
                               hdr[k].data(), hl, dig[k].data());
        });
        same("crc_list", algo, out[0], out[1]);
        same("crc_indexed", algo, idx[0], idx[1]);
        same("package_frames digests", algo, dig[0], dig[1]);
        same("package_frames frames", algo, hdr[0], hdr[1]);
        // whole frames (header, digest, payload), some corrupted: a payload byte of a short and of a
        // long frame, a digest byte, an entry id (part of the digest's header: fails the digest first)
        std::vector<uint8_t> blob(total + n * hl);
        std::vector<uint32_t> flens(n);
        std::vector<uint64_t> foffs(n);
        for (uint64_t i = 0, at = 0; i < n; ++i) {
            foffs[i] = at, flens[i] = hl + lens[i];
            memcpy(&blob[at], &hdr[0][i * hl], hl);
            if (lens[i]) memcpy(&blob[at + hl], ptrs[i], lens[i]);
            at += flens[i];
        }
        blob[foffs[4100] + hl + (3u << 20)] ^= 0x10;
        blob[foffs[3000] + hl] ^= 0x01;
        blob[foffs[2500] + 33] ^= 0x80;
        blob[foffs[2000] + 15] ^= 0x04;
        std::vector<int32_t> vst[2], rst[2];
        std::vector<uint64_t> fb[2];
        std::vector<uint8_t> reframed[2], applied[2];
        both([&](int k) {
            vst[k].assign(n, -1), rst[k].assign(n, -1), rdig[k].assign(n, 0);
            std::vector<const uint8_t*> fr(n);
            for (uint64_t i = 0; i < n; ++i) fr[i] = blob.data() + foffs[i];
            fb[k].push_back(bh::verify_frames(algo, 7, 100, 0, fr.data(), flens.data(), n, vst[k].data()));
            for (int trusted = 0; trusted < 2; ++trusted) {
                std::vector<uint8_t> copy = blob;
                std::vector<uint8_t*> w(n);
                for (uint64_t i = 0; i < n; ++i) w[i] = copy.data() + foffs[i];
                fb[k].push_back(bh::reframe_frames(algo, 7, 100, 0, trusted != 0, w.data(), flens.data(), n,
                                                   new_lacs.data(), rdig[k].data(), rst[k].data()));
                if (trusted) continue;
                reframed[k] = copy;
                applied[k] = blob;  // the GPU route's last step, from the statuses and digests above
                for (uint64_t i = 0; i < n; ++i) w[i] = applied[k].data() + foffs[i];
                bh::apply_reframe(algo, w.data(), n, new_lacs.data(), rst[k].data(), rdig[k].data());
                same("apply_reframe against reframe_frames", algo, applied[k], reframed[k]);
            }
        });
        same("verify_frames status", algo, vst[0], vst[1]);
        same("first_bad", algo, fb[0], fb[1]);
        same("reframe_frames frames", algo, reframed[0], reframed[1]);
        same("apply_reframe frames", algo, applied[0], applied[1]);
        if (fb[0][0] != 2000 || vst[0][2000] != 2 || vst[0][2500] != 2 || vst[0][3000] != 2 || vst[0][4100] != 2 ||
            vst[0][777] != 0) {
            fprintf(stderr, "verify_frames (algo %d): first_bad %llu, statuses %d %d %d %d %d\n", algo,
                    (unsigned long long)fb[0][0], vst[0][2000], vst[0][2500], vst[0][3000], vst[0][4100], vst[0][777]);
            ++g_failures;
        }
    }
    printf(g_failures ? "host_batch_check: %d FAILURES\n" : "host_batch_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
