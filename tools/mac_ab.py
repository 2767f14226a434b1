"""MAC ledgers (HMAC-SHA1) timed in ONE process with seeded inputs:

  device   MacDigestManager.package_batch and verify_batch on 1M device-resident entries of 4 KiB, HIP events
  host     package_batch_host and verify_batch_host on 64K host entries of 4 KiB, on the CPU route and on the
           GPU route (synchronous C calls: wall clock, pointer arrays built outside the timed region)
  python   hmac.digest(key, header + payload, "sha1") over the same host batch on 16 threads: the stand-in
           for the reference's javax.crypto Mac where no JDK exists (0.52 GB/s per core)

Before timing, sampled frames must equal hmac's and every packaged frame must verify. The last line says
whether the device-resident rates exceed the 16-thread python rate (the one hard expectation).

Usage (GPU box): python3 tools/mac_ab.py   Environment: MAC_AB_N (device entries, default 1M), MAC_AB_HOST_N
(host entries, default 64K), MAC_AB_REPS (5), MAC_AB_LOG (default profiles/mac_ab_1m4k.log).
"""
import hmac
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("MAC_AB_N", str(1 << 20)))
HOST_N = int(os.environ.get("MAC_AB_HOST_N", str(1 << 16)))
REPS = int(os.environ.get("MAC_AB_REPS", "5"))
LOG = os.environ.get("MAC_AB_LOG", os.path.join(ROOT, "profiles", "mac_ab_1m4k.log"))
L4K, LEDGER, PASSWD, THREADS = 4096, 7, b"mac_ab", 16


def main():
    import hashlib
    import struct

    import numpy as np
    import torch

    from bookkeeper_amd import checksum as ck
    from bookkeeper_amd import digest as dg

    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log = open(LOG, "w")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    mgr = dg.MacDigestManager(LEDGER, PASSWD)
    key = hashlib.sha1(b"mac" + PASSWD).digest()
    say(f"mac_ab: {torch.cuda.get_device_name(0)}, host threads {ck.get_host_threads()}, reps {REPS}")

    # ---- device-resident ----
    payload = torch.empty(N * L4K, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(payload, 2024)
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    lacs = ids - 1
    lenf = torch.full((N,), L4K, dtype=torch.int64, device=dev)
    off = ids * L4K
    ln = torch.full((N,), L4K, dtype=torch.int32, device=dev)
    frames, _ = mgr.package_batch(ids, lacs, lenf, payload, off, ln, sync_check=True)
    sample = [0, 1, N // 3, N - 1]
    for i in sample:
        hdr = struct.pack(">qqqq", LEDGER, i, i - 1, L4K)
        want = hdr + hmac.digest(key, hdr + payload[i * L4K:(i + 1) * L4K].cpu().numpy().tobytes(), "sha1")
        assert frames[i].cpu().numpy().tobytes() == want, f"frame {i} differs from hmac"
    framed = torch.cat([frames, payload.view(N, L4K)], dim=1).contiguous().view(-1)
    FL = 52 + L4K
    foff = ids * FL
    fln = torch.full((N,), FL, dtype=torch.int32, device=dev)
    status, fb = mgr.verify_batch(framed, foff, fln, 0)
    assert int(fb.item()) == N and int(status.abs().sum().item()) == 0, "packaged frames do not verify"
    say(f"parity ok: {len(sample)} sampled frames equal hmac's, all {N} frames verify")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)[len(ms) // 2], min(ms)

    gb = N * L4K / 1e9
    rates = {}
    for name, fn in (("device package_batch", lambda: mgr.package_batch(ids, lacs, lenf, payload, off, ln)),
                     ("device verify_batch", lambda: mgr.verify_batch(framed, foff, fln, 0))):
        med, best = timed(fn)
        rates[name] = gb / (med / 1e3)
        say(f"{name:28s} {N} x {L4K} B: median {med:9.3f} ms (min {best:.3f})  {rates[name]:9.1f} GB/s of payload")
    del framed, frames, payload
    torch.cuda.empty_cache()

    # ---- host-resident: the C calls alone, the pointer arrays built once outside the timed region ----
    import ctypes
    from bookkeeper_amd import _native
    Lb = _native.lib()
    vp = ctypes.c_void_p
    rng = np.random.default_rng(2024)
    host = rng.integers(0, 256, (HOST_N, L4K), dtype=np.uint8)
    hid = np.arange(HOST_N, dtype=np.int64)
    hlac, hlen = hid - 1, np.full(HOST_N, L4K, dtype=np.int64)
    pptr = (host.ctypes.data + np.arange(HOST_N, dtype=np.uint64) * L4K).astype(np.uint64)
    plen = np.full(HOST_N, L4K, dtype=np.uint32)
    hframes = np.zeros((HOST_N, FL), dtype=np.uint8)  # frame i = [header][mac][payload], its own row
    hframes[:, 52:] = host
    fptr = (hframes.ctypes.data + np.arange(HOST_N, dtype=np.uint64) * FL).astype(np.uint64)
    flen = np.full(HOST_N, FL, dtype=np.uint32)
    status = np.zeros(HOST_N, dtype=np.int32)
    fbad = ctypes.c_uint64(0)
    ksp = vp(mgr.key_state.ctypes.data)
    hgb = HOST_N * L4K / 1e9
    heads = {}
    for route, rname in ((ck.HOST_ROUTE_CPU, "CPU route"), (ck.HOST_ROUTE_GPU, "GPU route")):
        heads[route] = np.zeros((HOST_N, 52), dtype=np.uint8)

        def package():
            return Lb.bkd_digest_package_batch_mac_host(ksp, LEDGER, vp(hid.ctypes.data), vp(hlac.ctypes.data),
                                                        vp(hlen.ctypes.data), vp(pptr.ctypes.data), vp(plen.ctypes.data),
                                                        HOST_N, vp(heads[route].ctypes.data), 52)

        def verify():
            return Lb.bkd_digest_verify_batch_mac_host(ksp, LEDGER, 0, 0, vp(fptr.ctypes.data), vp(flen.ctypes.data), HOST_N,
                                                       vp(status.ctypes.data), ctypes.byref(fbad))

        with ck.host_batch_route(route):
            assert package() == 0  # warm-up (the GPU route's staging buffers)
            hframes[:, :52] = heads[route]
            for name, fn in ((f"host package ({rname})", package), (f"host verify ({rname})", verify)):
                assert fn() == 0
                ts = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append(time.perf_counter() - t0)
                    assert rc == 0
                if "verify" in name:
                    assert fbad.value == HOST_N and not status.any()
                med = sorted(ts)[len(ts) // 2]
                rates[name] = hgb / med
                say(f"{name:28s} {HOST_N} x {L4K} B: median {med * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f})  "
                    f"{rates[name]:9.1f} GB/s")
    assert (heads[ck.HOST_ROUTE_CPU] == heads[ck.HOST_ROUTE_GPU]).all(), "host routes disagree"

    # ---- python hmac on 16 threads over the same host batch ----
    hdrs = [struct.pack(">qqqq", LEDGER, i, i - 1, L4K) for i in range(HOST_N)]
    msgs = [hdrs[i] + host[i].tobytes() for i in range(HOST_N)]

    def part(p):
        return [hmac.digest(key, m, "sha1") for m in msgs[p::THREADS]]

    with ThreadPoolExecutor(THREADS) as pool:
        ts = []
        for _ in range(max(2, REPS)):
            t0 = time.perf_counter()
            parts = list(pool.map(part, range(THREADS)))
            ts.append(time.perf_counter() - t0)
    assert parts[0][0] == heads[ck.HOST_ROUTE_CPU][0, 32:52].tobytes()
    med = sorted(ts)[len(ts) // 2]
    rates["python"] = hgb / med
    say(f"{'python hmac, 16 threads':28s} {HOST_N} x {L4K} B: median {med * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f})  "
        f"{rates['python']:9.1f} GB/s")
    ok = True
    for name in ("device package_batch", "device verify_batch"):
        ratio = rates[name] / rates["python"]
        ok = ok and ratio > 1.0
        say(f"{name} / python hmac x16 = {ratio:.1f}x")
    say("structural expectation (device-resident faster than 16-thread hashlib): " + ("met" if ok else "MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
