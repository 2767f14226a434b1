"""Python-level calls (sys.setprofile: call and c_call events) that the composite, V2 and read-request host
bindings make on the CPU route, CRC and MAC: per entry = (calls at 128 entries - calls at 64) / 64, per batch =
the rest at 64 entries. Timing a 64-entry call moves by up to 2x from run to run on a shared CPU; the counts do
not (profiles/requests_fold_binding_calls.log).

Usage: python3 tools/binding_calls.py [CHECKOUT]   (default: this one; another checkout must be built)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

T = dg.DigestType.CRC32C
table = dg.mac_key_table([b"a", b"b"])
dm = dg.DigestManager.instantiate(7, b"", T)
KEY = bytes(range(20))


def args(n):
    ids = np.arange(n, dtype=np.int64)
    pay = [bytes([i % 251]) * 256 for i in range(n)]
    return ids, ids - 1, np.full(n, 256, dtype=np.int64), ids + 100, pay, (np.arange(n) % 2).astype(np.uint32)


def forms(n):
    ids, lacs, lf, lids, pay, key_of = args(n)
    crc_heads, _ = dg.package_batch_ledgers_host(T, lids, ids, lacs, lf, pay)
    mac_heads, _ = dg.package_batch_ledgers_mac_host(table, key_of, lids, ids, lacs, lf, pay)
    cf = [crc_heads[i].tobytes() + pay[i] for i in range(n)]
    mf = [mac_heads[i].tobytes() + pay[i] for i in range(n)]
    rf = list(range(0, n + 1, 1))
    return {
        "dm.package_batch_segments_host": lambda: dm.package_batch_segments_host(ids, lacs, lf, pay),
        "dm.package_batch_v2_host": lambda: dm.package_batch_v2_host(ids, lacs, lf, pay, KEY),
        "dg.package_batch_segments_host": lambda: dg.package_batch_segments_host(T, lids, ids, lacs, lf, pay),
        "dg.package_batch_v2_host": lambda: dg.package_batch_v2_host(T, lids, ids, lacs, lf, pay, KEY),
        "dg.verify_requests_host": lambda: dg.verify_requests_host(T, cf, rf, lids, ids),
        "dg.package_batch_segments_mac_host": lambda: dg.package_batch_segments_mac_host(table, key_of, lids, ids, lacs, lf, pay),
        "dg.package_batch_v2_mac_host": lambda: dg.package_batch_v2_mac_host(table, key_of, lids, ids, lacs, lf, pay, KEY),
        "dg.verify_requests_mac_host": lambda: dg.verify_requests_mac_host(table, key_of, mf, rf, lids, ids),
        "dg.package_batch_ledgers_mac_host": lambda: dg.package_batch_ledgers_mac_host(table, key_of, lids, ids, lacs, lf, pay),
    }


def count(fn):
    c = [0]
    def prof(frame, event, arg):
        if event in ("call", "c_call"):
            c[0] += 1
    fn()  # warm: imports, the library
    sys.setprofile(prof)
    try:
        fn()
    finally:
        sys.setprofile(None)
    return c[0] - 1  # (the closing sys.setprofile)


with ck.host_batch_route(ck.HOST_ROUTE_CPU):
    f64, f128 = forms(64), forms(128)
    for name in f64:
        c64, c128 = count(f64[name]), count(f128[name])
        per = (c128 - c64) / 64
        print(f"{name:38s} per entry {per:5.2f}  per batch {c64 - 64 * per:5.0f}  (calls at 64 entries {c64}, at 128 {c128})")
