"""A/B of verifying and packaging a MAC (HMAC-SHA1) batch that spans many ledgers, in ONE process on the
same device bytes: 1M framed 4 KiB entries, HIP events on the stream, median of 5.

  verify a    MacDigestManager.verify_batch, one ledger and one key (the existing single-key kernel: the yardstick)
  verify b    verify_requests_mac: the same payloads as 1 024 requests of 1 024 ledgers, each with a key of its
              own, in one call
  verify c    what a caller does without it: one bkd_digest_verify_batch_mac call per ledger on one stream
  package a / b / c   the same three for MacDigestManager.package_batch, package_batch_ledgers_mac and one
              bkd_digest_package_batch_mac call per ledger

Before timing, sampled frames of both framings must equal hmac's, every frame must verify on every leg and
the per-ledger legs must write the bytes the one-call legs write.

Usage (GPU box): python3 tools/mac_requests_ab.py   Environment: MAC_RQ_N (entries, a multiple of 1 024,
default 1M), MAC_RQ_REPS (5), MAC_RQ_LOG (default profiles/mac_requests_ab_1m4k.log).
"""
import ctypes
import hmac
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("MAC_RQ_N", str(1 << 20)))
REPS = int(os.environ.get("MAC_RQ_REPS", "5"))
LOG = os.environ.get("MAC_RQ_LOG", os.path.join(ROOT, "profiles", "mac_requests_ab_1m4k.log"))
L4K, FL, NLEDGERS, LEDGER, PASSWD = 4096, 52 + 4096, 1024, 7, b"mac_ab"


def main():
    import hashlib

    import numpy as np
    import torch

    from bookkeeper_amd import _native
    from bookkeeper_amd import checksum as ck
    from bookkeeper_amd import digest as dg

    assert N % NLEDGERS == 0
    per = N // NLEDGERS
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log = open(LOG, "w")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    L = _native.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    i64 = dict(dtype=torch.int64, device=dev)
    say(f"mac_requests_ab: {torch.cuda.get_device_name(0)}, {N} entries of {L4K} B, {NLEDGERS} ledgers, reps {REPS}")

    mgr = dg.MacDigestManager(LEDGER, PASSWD)
    passwords = [b"ledger-%d" % k for k in range(NLEDGERS)]
    table_h = dg.mac_key_table(passwords)
    table = torch.from_numpy(table_h.view(np.int32).copy()).to(dev)
    payload = torch.empty(N * L4K, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(payload, 2024)
    idx = torch.arange(N, **i64)
    lenf = torch.full((N,), L4K, **i64)
    off, ln = idx * L4K, torch.full((N,), L4K, dtype=torch.int32, device=dev)
    ledger_of = 1000 + (idx // per) * 0x100000001  # distinct in both words
    key_of = (idx // per).to(torch.int32)
    ids_m = idx % per                               # entry ids restart in every ledger
    ledgers_h = (1000 + np.arange(NLEDGERS, dtype=np.int64) * 0x100000001).tolist()

    # ---- the frames of both framings, checked against hmac; then laid out in front of their payloads ----
    heads1, _ = mgr.package_batch(idx, idx - 1, lenf, payload, off, ln, sync_check=True)
    headsm, _ = dg.package_batch_ledgers_mac(table, key_of, ledger_of, ids_m, ids_m - 1, lenf, payload, off, ln,
                                             sync_check=True)
    key1 = hashlib.sha1(b"mac" + PASSWD).digest()
    for i in (0, 1, per - 1, per, N // 3, N - 1):
        body = payload[i * L4K:(i + 1) * L4K].cpu().numpy().tobytes()
        hdr = struct.pack(">qqqq", LEDGER, i, i - 1, L4K)
        assert heads1[i].cpu().numpy().tobytes() == hdr + hmac.digest(key1, hdr + body, "sha1"), f"frame {i} (one ledger)"
        k = i // per
        hdr = struct.pack(">qqqq", ledgers_h[k], i % per, i % per - 1, L4K)
        keyk = hashlib.sha1(b"mac" + passwords[k]).digest()
        assert headsm[i].cpu().numpy().tobytes() == hdr + hmac.digest(keyk, hdr + body, "sha1"), f"frame {i} (ledger {k})"
    F1 = torch.cat([heads1, payload.view(N, L4K)], dim=1).contiguous().view(-1)
    FM = torch.cat([headsm, payload.view(N, L4K)], dim=1).contiguous().view(-1)
    foff, fln = idx * FL, torch.full((N,), FL, dtype=torch.int32, device=dev)
    rq = dict(first=torch.arange(NLEDGERS + 1, **i64) * per, ledgers=torch.tensor(ledgers_h, **i64),
              firsts=torch.zeros(NLEDGERS, **i64), keys=torch.arange(NLEDGERS, dtype=torch.int32, device=dev))
    status = torch.empty(N, dtype=torch.int32, device=dev)
    fb = torch.empty(1, **i64)
    out = torch.empty((N, 52), dtype=torch.uint8, device=dev)
    keys_h = [ctypes.c_void_p(table_h[k].ctypes.data) for k in range(NLEDGERS)]

    def verify_a():
        return mgr.verify_batch(F1, foff, fln, 0)

    def verify_b():
        return dg.verify_requests_mac(table, rq["keys"], FM, foff, fln, rq["first"], rq["ledgers"], rq["firsts"])

    def verify_c():
        for k in range(NLEDGERS):
            rc = L.bkd_digest_verify_batch_mac(keys_h[k], ledgers_h[k], 0, 0, ptr(FM), FM.numel(), ptr(foff, 8 * k * per),
                                               ptr(fln, 4 * k * per), per, ptr(status, 4 * k * per), ptr(fb), sp)
            assert rc == 0

    def package_a():
        return mgr.package_batch(idx, idx - 1, lenf, payload, off, ln, out_frames=out)

    def package_b():
        return dg.package_batch_ledgers_mac(table, key_of, ledger_of, ids_m, ids_m - 1, lenf, payload, off, ln)

    lacs_m = ids_m - 1

    def package_c():
        for k in range(NLEDGERS):
            o8, o4 = 8 * k * per, 4 * k * per
            rc = L.bkd_digest_package_batch_mac(keys_h[k], ledgers_h[k], ptr(ids_m, o8), ptr(lacs_m, o8), ptr(lenf, o8),
                                                ptr(payload), payload.numel(), ptr(off, o8), ptr(ln, o4), per,
                                                ptr(out, 52 * k * per), 52, sp)
            assert rc == 0

    s, f = verify_a()
    assert int(f.item()) == N and not s.any(), "verify a"
    s, p = verify_b()
    ck.stream_sync(st)
    assert not s.any() and bool((p == per).all()), "verify b"
    status.fill_(-1)
    verify_c()
    ck.stream_sync(st)
    assert not status.any() and int(fb.item()) == per, "verify c"
    out.fill_(0)
    package_c()
    ck.stream_sync(st)
    assert torch.equal(out, headsm) and torch.equal(package_b()[0], headsm), "package c / b"
    assert torch.equal(package_a()[0], heads1), "package a"
    say(f"parity ok: sampled frames equal hmac's, all {N} frames verify on every leg, package legs agree")

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
    med = {}
    for name, fn in (("verify a  one ledger, one call", verify_a), ("verify b  1024 requests, one call", verify_b),
                     ("verify c  1024 calls", verify_c), ("package a  one ledger, one call", package_a),
                     ("package b  1024 ledgers, one call", package_b), ("package c  1024 calls", package_c)):
        m, best = timed(fn)
        med[name.split("  ")[0]] = m
        say(f"{name:36s} median {m:9.3f} ms (min {best:.3f})  {gb / (m / 1e3):9.1f} GB/s of payload")
    for op in ("verify", "package"):
        say(f"{op}: b / a = {med[op + ' b'] / med[op + ' a']:.4f}   c / b = {med[op + ' c'] / med[op + ' b']:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
