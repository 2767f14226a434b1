"""A/B several builds of libbkdigest.so in ONE process on the host-resident many-ledger forms, both routes:
the four MAC forms that take a key table (verify requests, package per-entry ledgers, composite payloads, V2
add requests) and the CRC verify-requests and V2 forms they share their glue with. Interleaved rounds on the
same host buffers, as tools/ab_host_route.py does for the single-ledger forms; every library's results must
equal the first library's, bit for bit.

Usage: python3 tools/ab_host_forms.py lib.so [lib.so ...]
Pass two or three copies of each build and compare the groups, not single libraries (ab_host_route.py says why).
Environment: AB_N (entries, default 65536), AB_ROUNDS (7), AB_ROUTES (default "1,2": CPU, GPU), AB_LOG (a file
that receives the lines as well).
"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("AB_N", "65536"))
ROUNDS = int(os.environ.get("AB_ROUNDS", "7"))
ROUTES = [int(r) for r in os.environ.get("AB_ROUTES", "1,2").split(",")]
META, MSG, NKEYS, PER_REQUEST = 96, 4000, 64, 64
PLEN = META + MSG


def main(paths):
    from bookkeeper_amd import _native
    from bookkeeper_amd import digest as dg
    log = open(os.environ["AB_LOG"], "w") if os.environ.get("AB_LOG") else None

    def say(msg):
        print(msg, flush=True)
        if log:
            log.write(msg + "\n")
            log.flush()

    libs = {}
    for p in paths:
        L = ctypes.CDLL(os.path.abspath(p))
        for fn, (res, args) in _native.PROTOTYPES.items():
            if hasattr(L, fn):
                getattr(L, fn).restype = res
                getattr(L, fn).argtypes = args
        libs[os.path.basename(p) + "#" + str(len(libs))] = L
    first = next(iter(libs.values()))
    n, vp = N, ctypes.c_void_p
    p = lambda a: vp(a.ctypes.data)
    rng = np.random.default_rng(7)
    payload = rng.integers(0, 256, (n, PLEN), dtype=np.uint8)
    table = dg.mac_key_table([b"ledger-%d" % k for k in range(NKEYS)])
    key_of = (np.arange(n) % NKEYS).astype(np.uint32)
    lids, ids = (1000 + key_of).astype(np.int64), np.arange(n, dtype=np.int64)
    lacs, lf = ids - 1, np.full(n, PLEN, dtype=np.int64)
    pay_ptrs = (payload.ctypes.data + ids.astype(np.uint64) * PLEN).astype(np.uint64)
    pay_lens = np.full(n, PLEN, dtype=np.uint32)
    seg_ptrs = np.stack([pay_ptrs, pay_ptrs + META], axis=1).reshape(-1).copy()
    seg_lens = np.tile(np.array([META, MSG], dtype=np.uint32), n)
    seg_first = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    master = np.frombuffer(bytes(range(20)), dtype=np.uint8)

    # read requests: PER_REQUEST consecutive entries of one ledger each, framed by the first library's CPU route
    first.bkd_set_host_batch_route(1)
    nreq = n // PER_REQUEST
    req_first = np.arange(0, n + 1, PER_REQUEST, dtype=np.uint64)
    req_keys = (np.arange(nreq) % NKEYS).astype(np.uint32)
    req_lids, req_eids = (1000 + req_keys).astype(np.int64), req_first[:-1].astype(np.int64)
    req_flags = np.zeros(nreq, dtype=np.uint32)
    rq_key_of, rq_lids = np.repeat(req_keys, PER_REQUEST), np.repeat(req_lids, PER_REQUEST)
    framed = {}
    for kind, head in (("mac", 52), ("crc", 36)):
        heads, dig = np.zeros((n, head), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
        if kind == "mac":
            rc = first.bkd_digest_package_batch_ledgers_mac_host(p(table), NKEYS, p(rq_key_of), p(rq_lids), p(ids), p(lacs),
                                                                 p(lf), p(pay_ptrs), p(pay_lens), n, p(heads), head)
        else:
            rc = first.bkd_digest_package_batch_ledgers_host(_native.CRC32C, p(rq_lids), p(ids), p(lacs), p(lf), p(pay_ptrs),
                                                             p(pay_lens), n, p(heads), head, p(dig))
        assert rc == 0, (first.bkd_last_error() or b"").decode()
        buf = np.concatenate([heads, payload], axis=1)
        framed[kind] = (buf, (buf.ctypes.data + ids.astype(np.uint64) * (head + PLEN)).astype(np.uint64),
                        np.full(n, head + PLEN, dtype=np.uint32))

    status, req_fb = np.zeros(n, dtype=np.int32), np.zeros(nreq, dtype=np.uint64)
    frames, dig = np.zeros((n, 52), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    requests = np.zeros((n, 80 + PLEN), dtype=np.uint8)
    rptr = (requests.ctypes.data + ids.astype(np.uint64) * (80 + PLEN)).astype(np.uint64)
    mf, cf = framed["mac"], framed["crc"]
    forms = {  # name -> (call(L) -> rc, the arrays it writes)
        "verify_requests_mac": (lambda L: L.bkd_digest_verify_requests_mac_host(
            p(table), NKEYS, p(req_keys), p(mf[1]), p(mf[2]), n, p(req_first), nreq, p(req_lids), p(req_eids), p(req_flags),
            p(status), p(req_fb)), (status, req_fb)),
        "package_ledgers_mac": (lambda L: L.bkd_digest_package_batch_ledgers_mac_host(
            p(table), NKEYS, p(key_of), p(lids), p(ids), p(lacs), p(lf), p(pay_ptrs), p(pay_lens), n, p(frames), 52), (frames,)),
        "package_segments_mac": (lambda L: L.bkd_digest_package_batch_segments_mac_host(
            p(table), NKEYS, p(key_of), 0, p(lids), p(ids), p(lacs), p(lf), p(seg_ptrs), p(seg_lens), 2 * n, p(seg_first), n,
            p(frames), 52), (frames,)),
        "package_v2_mac": (lambda L: L.bkd_digest_package_batch_v2_mac_host(
            p(table), NKEYS, p(key_of), 0, p(lids), p(ids), p(lacs), p(lf), p(pay_ptrs), p(pay_lens), n, p(master), 0, 0,
            16384, p(rptr)), (requests,)),
        "verify_requests_crc": (lambda L: L.bkd_digest_verify_requests_host(
            _native.CRC32C, p(cf[1]), p(cf[2]), n, p(req_first), nreq, p(req_lids), p(req_eids), p(req_flags), p(status),
            p(req_fb)), (status, req_fb)),
        "package_v2_crc": (lambda L: L.bkd_digest_package_batch_v2_host(
            _native.CRC32C, 0, p(lids), p(ids), p(lacs), p(lf), p(pay_ptrs), p(pay_lens), n, p(master), 0, 0, 16384, p(rptr),
            p(dig)), (requests, dig)),
    }
    say(f"ab_host_forms: {n} entries of {META} + {MSG} B, {NKEYS} keys, {nreq} requests, rounds {ROUNDS}, "
        f"libraries {' '.join(libs)}")
    for route in ROUTES:
        times, want = {}, {}
        for rnd in range(ROUNDS + 1):  # round 0 warms every library up (staging sets, key uploads) and is dropped
            for lname, L in libs.items():
                L.bkd_set_host_batch_route(route)
                for fname, (call, outs) in forms.items():
                    for o in outs:
                        o.fill(0xA5 if o.dtype == np.uint8 else 7)
                    t0 = time.perf_counter()
                    rc = call(L)
                    dt = time.perf_counter() - t0
                    assert rc == 0, (lname, fname, (L.bkd_last_error() or b"").decode())
                    got = [o.copy() for o in outs]
                    if fname not in want:
                        want[fname] = got
                        if "verify" in fname:
                            assert not status.any() and (req_fb == PER_REQUEST).all(), fname
                    assert all(np.array_equal(g, w) for g, w in zip(got, want[fname])), (lname, fname, "results differ")
                    if rnd:
                        times.setdefault((fname, lname), []).append(dt * 1e3)
        for fname in forms:
            med = {}
            for lname in sorted(libs):
                t = times[(fname, lname)]
                med[lname] = float(np.median(t))
                say(f"route {route} {fname:22s} {lname:16s} median {med[lname]:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}")
            groups = {}
            for lname, m in med.items():
                groups.setdefault(lname.split("_")[0], []).append(m)
            say(f"route {route} {fname:22s} " + "; ".join(
                f"{g}: medians {min(v):.3f}-{max(v):.3f}, their median {float(np.median(v)):.3f}" for g, v in sorted(groups.items())))


if __name__ == "__main__":
    main(sys.argv[1:])
