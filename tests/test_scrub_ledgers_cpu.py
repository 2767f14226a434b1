"""The mixed-ledger entry-log scrub (bkd_entrylog_verify_ledgers) without a device: the bin rule and the
lane model it is derived from, the table lookup, the host form's CPU route status by status against
oracle.verify_entry / hmac / the DUMMY length rule, the argument checks, LedgerTable, and the host code under
a sanitizer as a stand-alone program."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import bench
import scrub_util as su
from bookkeeper_amd import checksum as ck, entrylog as el
from bookkeeper_amd._native import lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bookkeeper_amd", "csrc")


@pytest.fixture(scope="module")
def mixed():
    return su.mixed_case()


@pytest.fixture()
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


# ---- the bin rule ----

def test_bin_rule_every_length():
    L = lib()
    assert [su.bin_of(52 + 64 * (b - 1)) for b in (1, 2, 3, 4, 5, 7, 8, 9, 16)] == [0, 4, 6, 8, 9, 11, 12, 12, 16]
    prev = 0
    for n in range(52, 70001):
        got = L.bkd_host_scrub_bin(n)
        assert got == su.bin_of(n), n
        assert got >= prev, n  # monotone in length
        prev = got
    assert L.bkd_host_scrub_bin(su.MAC_MAX_ENTRY) == su.bin_of(su.MAC_MAX_ENTRY) == 72  # the largest bin
    assert L.bkd_host_scrub_bin(su.MAC_MAX_ENTRY - 64) <= 72
    assert all(L.bkd_host_scrub_bin(n) == 0 for n in range(0, 52))
    # within a bin, longest / shortest block count is under 1.25 from four blocks on
    lo, hi = {}, {}
    for n in range(52, 70001):
        b, k = su.sha1_blocks(n), su.bin_of(n)
        lo.setdefault(k, b)
        hi[k] = b
    assert all(hi[k] / lo[k] < 1.25 for k in lo if lo[k] >= 4)


def test_lane_model_occupancy():
    """The bound the bins exist for: bench.zipf_index lengths as 52-byte-framed entries. The rule alone gives
    0.920 binned (stable counting sort, bins descending) and 0.118 in arrival order."""
    _, lens = bench.zipf_index(65536)
    frames = lens + 52
    blocks = np.array([su.sha1_blocks(int(n)) for n in frames])
    bins = np.array([lib().bkd_host_scrub_bin(int(n)) for n in frames])
    arrival = su.lane_occupancy(blocks, np.arange(blocks.size))
    binned = su.lane_occupancy(blocks, np.argsort(-bins, kind="stable"))
    print(f"lane occupancy: arrival {arrival:.3f}, binned {binned:.3f}")
    assert binned >= 0.90
    assert arrival < 0.2


# ---- the table lookup ----

def test_lookup_every_row_and_gap():
    L = lib()
    sizes = set()
    for ids, probes in su.lookup_tables():
        sizes.add(ids.size)
        rows = {int(v): r for r, v in enumerate(ids)}
        for p in probes:
            got = L.bkd_host_scrub_lookup(ctypes.c_void_p(ids.ctypes.data), ids.size, p)
            assert got == rows.get(p, -1), (ids.size, p)
    assert sizes == {1, 2, 3, 1000, 1025}
    assert L.bkd_host_scrub_lookup(None, 0, 5) == -1


# ---- the host form, CPU route ----

def test_host_mixed_log(mixed, cpu_route):
    buf, expect, specs, table, want = mixed
    offs = np.array([e[2] for e in expect], dtype=np.uint64)
    lens = np.array([e[3] for e in expect], dtype=np.uint32)
    rc, status, fb = su.run_host(buf, offs, lens, table)
    assert rc == 0
    assert (status == want).all(), np.nonzero(status != want)[0][:10]
    assert fb == su.want_first_bad(want)
    assert {-1, 0, 2} <= set(want.tolist()) and (want == 2).sum() >= 20
    # through the Python surface: the record walk finds the same entries
    scan, st2, fb2 = el.EntryLogScrubber.verify_ledgers_host(buf, table)
    assert (scan.offsets == offs).all() and (st2 == want).all() and fb2 == fb
    # a mask: masked types are not checked
    rc, status, fb = su.run_host(buf, offs, lens, table, types=su.TYPE_BIT["HMAC"] | su.TYPE_BIT["DUMMY"])
    listed = {l: s for l, s in specs.items() if l != 99}
    want_m = np.array([su.want_status(buf[o:o + n], listed.get(lid), su.TYPE_BIT["HMAC"] | su.TYPE_BIT["DUMMY"])
                       for lid, eid, o, n in expect], dtype=np.int32)
    assert rc == 0 and (status == want_m).all() and fb == su.want_first_bad(want_m)


def test_host_short_entries(cpu_route):
    entries, want, table = su.short_entries()
    buf, offs, lens = su.pack_entries(entries)
    rc, status, fb = su.run_host(buf, offs, lens, table)
    assert rc == 0 and (status == want).all() and fb == su.want_first_bad(want) == 0


def test_host_rejects_bad_tables(mixed, cpu_route):
    buf, expect, specs, table, want = mixed
    offs = np.array([e[2] for e in expect[:20]], dtype=np.uint64)
    lens = np.array([e[3] for e in expect[:20]], dtype=np.uint32)
    unsorted = table.ids.copy()
    unsorted[[2, 3]] = unsorted[[3, 2]]
    dup = table.ids.copy()
    dup[4] = dup[3]
    bad_key = table.keys.copy()
    bad_key[np.nonzero(table.types == el.DIGEST_HMAC)[0][0]] = table.nkeys
    for kw in (dict(ids=unsorted), dict(ids=dup), dict(keys=bad_key)):
        rc, status, fb = su.run_host(buf, offs, lens, table, **kw)
        assert rc == su.BKD_ERR_INVALID_ARG, kw
        assert (status == 77).all() and fb == 0xDEAD  # outputs untouched
    # the key row of a ledger whose type is masked out is not looked at
    rc, status, fb = su.run_host(buf, offs, lens, table, keys=bad_key, types=su.ALL & ~su.TYPE_BIT["HMAC"])
    assert rc == 0


def test_host_unreadable_entries(cpu_route):
    table = el.LedgerTable.from_ledgers({1: "CRC32C", 3: ("HMAC", b"pw")})
    good = su.frame_for("CRC32C", 1, 0, b"x" * 100)
    buf, offs, lens = su.pack_entries([good, good])
    offs[1], lens[1] = buf.size - 10, 11  # one byte past the log
    rc, status, fb = su.run_host(buf, offs, lens, table)
    assert rc == su.BKD_ERR_BOUNDS and status.tolist() == [0, 1] and fb == 1
    rc, status, fb = su.run_host(buf, offs[:0], lens[:0], table)
    assert rc == 0 and fb == 0  # n == 0


_NO_DEVICE_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import scrub_util as su
from bookkeeper_amd import _native, checksum as ck
assert _native.device_count() == 0
buf, expect, specs, table, want = su.mixed_case(n_entries=120, corruptions=9)
offs = np.array([e[2] for e in expect], dtype=np.uint64)
lens = np.array([e[3] for e in expect], dtype=np.uint32)
rc, status, fb = su.run_host(buf, offs, lens, table)  # automatic: HMAC ledgers, but no device -> the CPU route
assert rc == 0 and (status == want).all() and fb == su.want_first_bad(want), (rc, fb)
with ck.host_batch_route(ck.HOST_ROUTE_GPU):
    rc, status, fb = su.run_host(buf, offs, lens, table)
    assert rc == su.BKD_ERR_NO_DEVICE and (status == 77).all()
p = 1 << 20  # the device-resident call is GPU work only
assert _native.lib().bkd_entrylog_verify_ledgers(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == su.BKD_ERR_NO_DEVICE
assert _native.lib().bkd_entrylog_scrub_lanes(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == su.BKD_ERR_NO_DEVICE
print("scrub without a device")
"""


def test_scrub_without_a_device():
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "scrub without a device" in r.stdout, r.stderr[-2000:]


# ---- argument checks of the device call: answered before the device is looked for ----

def test_device_call_argument_checks():
    L, p = lib(), 1 << 20
    call = L.bkd_entrylog_verify_ledgers
    inv = su.BKD_ERR_INVALID_ARG
    assert call(None, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null log, n > 0
    assert call(p, 64, None, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null offsets
    assert call(p, 64, p, None, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null lengths
    assert call(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, None, p, None) == inv     # null status
    assert call(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, None, None) == inv     # null first_bad
    assert call(p, 64, p, p, 1, None, p, p, 1, p, 1, 15, p, p, None) == inv     # null ledger ids, nledgers > 0
    assert call(p, 64, p, p, 1, p, p, p, 1, p, 1, 16, p, p, None) == inv        # a type bit above 3
    assert call(p, 64, p, p, 1, p, p, None, 1, p, 1, 15, p, p, None) == inv     # HMAC bit, null key rows
    assert call(p, 64, p, p, 1, p, p, p, 1, None, 1, 15, p, p, None) == inv     # HMAC bit, null key table
    assert call(p, 64, p, p, 1, p, p, p, 1, p, 0, 15, p, p, None) == inv        # HMAC bit, nkeys == 0
    assert call(p, 64, p, p, 1 << 32, p, p, p, 1, p, 1, 15, p, p, None) == inv  # n >= 2^32
    lanes = L.bkd_entrylog_scrub_lanes  # the same checks, d_lanes / d_nlanes for d_status / d_first_bad
    assert lanes(None, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null log, n > 0
    assert lanes(p, 64, None, p, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null offsets
    assert lanes(p, 64, p, None, 1, p, p, p, 1, p, 1, 15, p, p, None) == inv     # null lengths
    assert lanes(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, None, p, None) == inv     # null lanes, n > 0
    assert lanes(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, None, None) == inv     # null nlanes
    assert lanes(p, 64, p, p, 0, p, p, p, 1, p, 1, 15, None, None, None) == inv  # null nlanes, n == 0
    assert lanes(p, 64, p, p, 1, None, p, p, 1, p, 1, 15, p, p, None) == inv     # null ledger ids, nledgers > 0
    assert lanes(p, 64, p, p, 1, p, p, p, 1, p, 1, 16 | 4, p, p, None) == inv    # a type bit above 3
    assert lanes(p, 64, p, p, 1, p, p, None, 1, p, 1, 15, p, p, None) == inv     # null key rows
    assert lanes(p, 64, p, p, 1, p, p, p, 1, None, 1, 15, p, p, None) == inv     # null key table
    assert lanes(p, 64, p, p, 1, p, p, p, 1, p, 0, 15, p, p, None) == inv        # nkeys == 0
    assert lanes(p, 64, p, p, 1 << 32, p, p, p, 1, p, 1, 15, p, p, None) == inv  # n >= 2^32
    for mask in (0, 1, 2, 8, 11):                                                # without the HMAC bit: no lanes
        assert lanes(p, 64, p, p, 1, p, p, p, 1, p, 1, mask, p, p, None) == inv, mask
        assert lanes(p, 64, p, p, 0, p, p, p, 1, p, 1, mask, p, p, None) == inv, mask
    assert L.bkd_set_scrub_order(2) == inv and L.bkd_set_scrub_order(-1) == inv
    assert L.bkd_set_scrub_order(1) == 0 and L.bkd_get_scrub_order() == 1
    assert L.bkd_set_scrub_order(0) == 0 and L.bkd_get_scrub_order() == 0
    assert L.bkd_abi_version() == 6


# ---- LedgerTable ----

def test_ledger_table_rows():
    t = el.LedgerTable.from_ledgers({9: ("HMAC", b"a"), -4: "CRC32", 5: ("HMAC", b"b"), 1 << 40: ("HMAC", b"a"),
                                     0: "DUMMY", 2: "CRC32C"})
    assert t.ids.tolist() == [-4, 0, 2, 5, 9, 1 << 40]
    assert t.types.tolist() == [el.DIGEST_CRC32, el.DIGEST_DUMMY, el.DIGEST_CRC32C, el.DIGEST_HMAC, el.DIGEST_HMAC,
                                el.DIGEST_HMAC]
    assert t.nkeys == 2 and t.keys[4] == t.keys[5] != t.keys[3]  # a shared password shares a row
    assert (t.key_states[t.keys[4]] == ck.mac_key_init(b"a")).all()
    assert (t.key_states[t.keys[3]] == ck.mac_key_init(b"b")).all()
    with pytest.raises(ValueError):
        el.LedgerTable.from_ledgers({1: "HMAC"})
    with pytest.raises(ValueError):
        el.LedgerTable.from_ledgers({1: "MD5"})


# ---- the lookup, the bin rule and the CPU route under a sanitizer: a stand-alone program ----

def test_host_scrub_under_address_sanitizer(tmp_path, mixed):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "scrub_sanitize")
    srcs = [os.path.join(here, "scrub_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                               ("host_scrub.cpp", "host_mac.cpp", "host_batch.cpp",
                                                                "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    buf, expect, specs, table, want = mixed
    # the mixed log's first 150 entries, the short entries behind them, and an entry that ends on the log's last byte
    entries, _, _ = su.short_entries()
    listed = {l: s for l, s in specs.items() if l != 99}
    listed.update({1: "CRC32C", 2: "CRC32", 4: "DUMMY"})  # 3 is CRC32C in the mixed log: its short HMAC frames fail
    t2 = el.LedgerTable.from_ledgers(listed)
    sbuf, soffs, slens = su.pack_entries(entries)
    log = np.concatenate([buf, sbuf[:int(soffs[-1] + slens[-1])]])
    offs = np.concatenate([np.array([e[2] for e in expect[:150]], dtype=np.uint64), soffs + np.uint64(buf.size)])
    lens = np.concatenate([np.array([e[3] for e in expect[:150]], dtype=np.uint32), slens])
    assert int(offs[-1]) + int(lens[-1]) == log.size
    want2 = np.array([su.want_status(log[int(o):int(o) + int(n)],
                                     listed.get(int.from_bytes(bytes(log[int(o):int(o) + 8]), "big", signed=True))
                                     if n >= 8 else None) for o, n in zip(offs, lens)], dtype=np.int32)
    probes = np.array([int(v) for v in t2.ids] + [-(1 << 63), (1 << 63) - 1, 4, 6, 100], dtype=np.int64)
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(struct.pack("<6Q", log.size, offs.size, len(t2), t2.nkeys, su.ALL, probes.size))
        for a in (log, offs, lens, t2.ids, t2.types, t2.keys, t2.key_states, probes):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    st_line, lk_line, bin_line = run.stdout.splitlines()
    st = [int(x) for x in st_line.split()[1:]]
    assert st[0] == su.want_first_bad(want2) and st[1] == 0 and st[2:] == want2.tolist()
    rows = {int(v): r for r, v in enumerate(t2.ids)}
    assert [int(x) for x in lk_line.split()[1:]] == [rows.get(int(p), -1) for p in probes]
    x = 0
    for n in range(52, 70001):
        x ^= (su.bin_of(n) * (n | 1)) & 0xFFFFFFFF
    assert bin_line.split() == ["bins", str(x), "72"]
