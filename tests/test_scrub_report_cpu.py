"""The scrub report without a device: the host form's CPU route against the plain-Python reference of
scrub_report_util on the logs the GPU suite runs, the new argument checks, the process without a device,
ScrubReport and compare_ledgers_map on logs with a real header and ledgers map, bkd_entrylog_ledgers_map on read,
absent and malformed maps, and the shared rules, the route-1 pass and the map reader under a sanitizer as a
stand-alone program."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import scrub_report_util as ru
import scrub_util as su
from bookkeeper_amd import checksum as ck, entrylog as el
from bookkeeper_amd._native import last_error, lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bookkeeper_amd", "csrc")
INV = su.BKD_ERR_INVALID_ARG


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def check_host(log, sync_want=0, **kw):
    rc, report, nbad, bad, status = ru.run_host(*log[:4], **kw)
    assert rc == sync_want, last_error()
    return ru.check((report, nbad, bad, status), log, capacity=kw.get("capacity"))


# ---- route 1 against the reference ----

def test_mixed_log_with_and_without_status():
    log = su.mixed_log5()
    rows = check_host(log)
    assert (rows[:, ru.BAD] > 0).sum() >= 5 and rows[-1, ru.ENTRIES] > 0 and rows[-1, ru.NOT_CHECKED] == rows[-1, ru.ENTRIES]
    check_host(log, with_status=False)


@pytest.mark.parametrize("kind", su.FB_KINDS)
@pytest.mark.parametrize("p", su.FB_POSITIONS)
def test_list_at_wave_and_block_edges(p, kind):
    check_host(su.first_bad_log(p, kind))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_cuts_of_one_log(n):
    check_host(ru.cut(su.mixed_log5(), n))


def test_every_entry_bad():
    log = ru.all_bad_log()
    rows = check_host(log)
    assert rows[:, ru.BAD].sum() == len(log[1])


def test_row_sharing_shapes():
    for log in [ru.one_ledger_log(), ru.one_ledger_blocks_log(), ru.all_distinct_log(), ru.round_robin_log(),
                ru.sparse_table_log()] + ru.runs_log():
        rows = check_host(log)
        n = len(log[1])
        for r in ru.untouched_rows(log):
            assert rows[r].tolist() == ru.initial_row(n)
    assert len(ru.untouched_rows(ru.sparse_table_log())) == 1022


def test_signed_entry_ids():
    one, spread = ru.signed_ids_logs()
    rows = check_host(one)
    i7, i8, i9 = 0, 1, 2  # the table's rows of ledgers 7, 8 and 9
    for r in (i7, i8):
        assert rows[r, ru.MIN_BAD] == ru.I64_MIN & ru.U64 and rows[r, ru.MAX_BAD] == ru.I64_MAX
    assert rows[i9, ru.BAD] == 2 and rows[i9, ru.MIN_BAD:ru.FIRST_BAD].tolist() == ru.initial_row(0)[ru.MIN_BAD:ru.FIRST_BAD]
    assert rows[-1, ru.BAD] == 2 and rows[-1, ru.MIN_BAD] == ru.I64_MAX  # the entries under 8 bytes
    rows = check_host(spread)
    assert rows[i7, ru.MIN_BAD] == ru.I64_MIN & ru.U64 and rows[i7, ru.MAX_BAD] == (1 << 32) + 1
    assert rows[i8, ru.MIN_BAD] == -1 & ru.U64 and rows[i8, ru.MAX_BAD] == ru.I64_MAX


def test_byte_sum_is_64_bits_wide():
    rows = check_host(ru.big_sum_log())
    assert rows[0, ru.BYTES] == 4097 * ((1 << 20) + 4) > 1 << 32


def test_catch_all_row():
    log = ru.catch_all_log()
    rows = check_host(log, sync_want=su.BKD_ERR_BOUNDS)  # everything is written, then the out-of-range entry reported
    assert rows[-1].tolist()[:5] == [5, sum(int(l) + 4 for l in log[2][[1, 2, 3, 5, 7]]), 0, 3, 2]
    assert rows[-1, ru.FIRST_BAD] == 2 and rows[-1, ru.MIN_BAD] == ru.I64_MAX  # the out-of-range entry's id is not read
    empty = el.LedgerTable.from_ledgers({})
    check_host(log[:3] + (empty, su.want_of_index(*log[:3], {})), sync_want=su.BKD_ERR_BOUNDS)
    none = (log[0], log[1][:0], log[2][:0], log[3], log[4][:0])
    rows = check_host(none)
    assert all(r.tolist() == ru.initial_row(0) for r in rows)


def test_capacity():
    log = su.mixed_log5()
    nbad = int((log[4] > 0).sum())
    assert nbad > 6
    for cap in (nbad - 1, nbad, nbad + 5):
        check_host(log, capacity=cap)
    rc, report, got, bad, _ = ru.run_host(*log[:4], capacity=0, null_bad=True)
    assert rc == 0 and got == nbad
    ru.check((report, got, np.full(4, ru.SENTINEL32, dtype=np.uint32), None), log, capacity=0)


def test_masks():
    buf, offs, lens, table, _ = su.mixed_log5()
    specs = su.mixed_case()[2]
    listed = {l: s for l, s in specs.items() if l != 99}
    for mask in (su.ALL & ~su.TYPE_BIT["HMAC"], su.TYPE_BIT["CRC32C"] | su.TYPE_BIT["CRC32"]):
        want = su.want_of_index(buf, offs, lens, listed, mask)
        rows = check_host((buf, offs, lens, table, want), types=mask, keys=None, nkeys=0)
        for r, t in enumerate(table.types):
            if not (mask >> int(t)) & 1:  # masked out: the ledger keeps its row, nothing of it is checked
                assert rows[r, ru.ENTRIES] == rows[r, ru.NOT_CHECKED] > 0 and rows[r, ru.BAD] == 0


def test_shape_steps_and_thread_logs():
    for log, types, null_keys, sync_want in su.shape_steps():
        check_host(log, sync_want=sync_want, types=types, **({"keys": None, "nkeys": 0} if null_keys else {}))
    for k in range(4):
        check_host(su.thread_log(k))


# ---- argument checks: each refuses with nothing written ----

def test_argument_checks():
    log = su.mixed_log5()
    for kw in ({"null_report": True}, {"null_nbad": True}, {"null_bad": True}):
        rc, report, nbad, bad, status = ru.run_host(*log[:4], **kw)
        assert rc == INV, kw
        assert (report == ru.SENTINEL64).all() and nbad == ru.SENTINEL64 and (bad == ru.SENTINEL32).all() and (status == 77).all()
    L = lib()
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(256)))
    dev, host = L.bkd_entrylog_scrub_report, L.bkd_entrylog_scrub_report_host
    for f, tail in ((dev, (None,)), (host, ())):
        assert f(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, None, p, 1, p, *tail) == INV   # null report
        assert f(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, p, 1, None, *tail) == INV   # null nbad
        assert f(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, None, 1, p, *tail) == INV   # capacity with a null list
        assert f(None, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, p, 1, p, *tail) == INV   # what the plain call refuses
        assert f(p, 64, p, p, 1, None, p, p, 1, p, 1, 15, p, p, p, 1, p, *tail) == INV
        assert f(p, 64, p, p, 1, p, p, p, 1, p, 1, 16, p, p, p, 1, p, *tail) == INV
        assert f(p, 64, p, p, 1, p, p, p, 1, None, 1, 15, p, p, p, 1, p, *tail) == INV
        assert f(p, 64, p, p, 1 << 32, p, p, p, 1, p, 1, 15, p, p, p, 1, p, *tail) == INV
    # the host form checks the table before any work
    rc, report, nbad, _, _ = ru.run_host(*log[:4], ids=log[3].ids[::-1])
    assert rc == INV and (report == ru.SENTINEL64).all() and nbad == ru.SENTINEL64
    assert L.bkd_abi_version() == 6


_NO_DEVICE_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import scrub_report_util as ru
import scrub_util as su
from bookkeeper_amd import _native, checksum as ck
assert _native.device_count() == 0
log = su.mixed_log5()
rc, report, nbad, bad, status = ru.run_host(*log[:4])  # automatic: HMAC ledgers, but no device -> the CPU route
assert rc == 0, rc
ru.check((report, nbad, bad, status), log)
with ck.host_batch_route(ck.HOST_ROUTE_GPU):
    rc, report, nbad, bad, status = ru.run_host(*log[:4])
    assert rc == su.BKD_ERR_NO_DEVICE and (report == ru.SENTINEL64).all() and nbad == ru.SENTINEL64
p = 1 << 20  # the device-resident call is GPU work only
rc = _native.lib().bkd_entrylog_scrub_report(p, 64, p, p, 1, p, p, p, 1, p, 1, 15, p, p, p, 1, p, None)
assert rc == su.BKD_ERR_NO_DEVICE, rc
print("report without a device")
"""


def test_process_without_a_device():
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "report without a device" in r.stdout, r.stderr[-2000:]


# ---- ScrubReport and the ledgers map ----

def pairs_of(sizes):
    return sorted(sizes.items())


def test_report_and_compare_ledgers_map():
    log, expect, specs, sizes = ru.mapped_log()
    pairs = pairs_of(sizes)
    table = el.LedgerTable.from_ledgers(specs)
    full = ru.with_header(log, [ru.map_record(pairs)], count=len(pairs))
    rep = el.EntryLogScrubber.report_ledgers_host(full, table)
    assert len(rep.scan) == len(expect) and rep.nbad == 0 and rep.bad.size == 0 and rep.status is None
    assert {int(l): int(b) for l, b in zip(table.ids, rep.rows["bytes"])} == sizes
    assert int(rep.other["entries"]) == 0 and rep.damaged() == {} and rep.bad_entries() == []
    m = el.read_ledgers_map(full)
    assert m.state == el.LEDGERS_MAP_READ and m.version == 1 and m.map_offset == len(log) and m.ledgers_count == len(pairs)
    assert list(zip(m.ledger_ids.tolist(), m.sizes.tolist())) == pairs
    assert rep.compare_ledgers_map(m) == ({}, [], [])
    # one size off by one
    off = [(l, s + (l == 7)) for l, s in pairs]
    m = el.read_ledgers_map(ru.with_header(log, [ru.map_record(off)], count=len(pairs)))
    assert rep.compare_ledgers_map(m) == ({7: (sizes[7], sizes[7] + 1)}, [], [])
    # a ledger in the map only; a ledger in the table only
    m = el.read_ledgers_map(ru.with_header(log, [ru.map_record(pairs + [(555, 40)])], count=len(pairs) + 1))
    assert rep.compare_ledgers_map(m) == ({}, [555], [])
    m = el.read_ledgers_map(ru.with_header(log, [ru.map_record([p for p in pairs if p[0] != 12])], count=len(pairs) - 1))
    assert rep.compare_ledgers_map(m) == ({}, [], [12])
    # duplicate map rows add up, as addLedgerSize does
    dup = [(l, s) for l, s in pairs if l != 20] + [(20, sizes[20] - 9), (20, 9)]
    m = el.read_ledgers_map(ru.with_header(log, [ru.map_record(dup)], count=len(pairs)))
    assert m.state == el.LEDGERS_MAP_READ and len(m.ledger_ids) == len(pairs) + 1
    assert rep.compare_ledgers_map(m) == ({}, [], [])


def test_report_python_damaged_and_bad_entries():
    buf, expect, specs, table, want = su.mixed_case()
    rep = el.EntryLogScrubber.report_ledgers_host(buf, table, max_bad=10, want_status=True)
    offs, lens = su.index_of(expect)
    assert (rep.scan.offsets == offs).all() and (rep.status == want).all()
    rows, nbad, bad = ru.want_report(buf, offs, lens, table, want)
    assert rep.nbad == nbad > 10 and rep.bad.tolist() == bad[:10].tolist()
    assert (rep.rows.view(np.uint64).reshape(-1, 8) == rows[:-1]).all() and (rep.other.reshape(1).view(np.uint64) == rows[-1]).all()
    assert rep.bad_entries() == [(expect[i][0], int.from_bytes(bytes(buf[expect[i][2] + 8:expect[i][2] + 16]), "big", signed=True),
                                  expect[i][2], expect[i][3]) for i in bad[:10]]
    signed = rows.view(np.int64)
    assert rep.damaged() == {int(table.ids[r]): (int(rows[r, ru.BAD]), int(signed[r, ru.MIN_BAD]), int(signed[r, ru.MAX_BAD]))
                             for r in range(len(table)) if rows[r, ru.BAD]}
    assert len(rep.damaged()) >= 5


def read_map(full, capacity=64):
    lids, sizes = np.full(capacity, -7, dtype=np.int64), np.full(capacity, -7, dtype=np.int64)
    count = ctypes.c_uint64(99)
    version, lcount, state = ctypes.c_int32(99), ctypes.c_int32(99), ctypes.c_int32(99)
    offset = ctypes.c_int64(99)
    buf = np.frombuffer(full, dtype=np.uint8).copy()  # an allocation of exactly the log's size
    rc = lib().bkd_entrylog_ledgers_map(ru._p(buf), buf.size, ru._p(lids), ru._p(sizes), capacity, ctypes.byref(count),
                                        ctypes.byref(version), ctypes.byref(offset), ctypes.byref(lcount), ctypes.byref(state))
    k = min(int(count.value), capacity)
    assert (lids[k:] == -7).all() and (sizes[k:] == -7).all()
    return rc, list(zip(lids[:k].tolist(), sizes[:k].tolist())), int(count.value), (version.value, offset.value, lcount.value), state.value


def test_ledgers_map_reads():
    log, _, _, sizes = ru.mapped_log()
    pairs = pairs_of(sizes)
    hdr = (1, len(log), len(pairs))
    one = ru.with_header(log, [ru.map_record(pairs)], count=len(pairs))  # the record ends on the log's last byte
    assert read_map(one) == (0, pairs, len(pairs), hdr, el.LEDGERS_MAP_READ)
    two = ru.with_header(log, [ru.map_record(pairs[:4]), ru.map_record(pairs[4:])], count=len(pairs))
    assert read_map(two) == (0, pairs, len(pairs), hdr, el.LEDGERS_MAP_READ)
    for tail in (1, 3, 4, 40):  # a zero tail: a size of 0 ends the map; under four bytes of it are a short read
        got = read_map(ru.with_header(log, [ru.map_record(pairs)], count=len(pairs), tail=tail))
        assert got == (0, pairs, len(pairs), hdr, el.LEDGERS_MAP_READ if tail >= 4 else el.LEDGERS_MAP_MALFORMED), tail
    rc, got, count, _, state = read_map(one, capacity=len(pairs) - 1)
    assert rc == su.BKD_ERR_BOUNDS and got == pairs[:-1] and count == len(pairs) and state == el.LEDGERS_MAP_READ
    assert el.read_ledgers_map(ru.with_header(log, [ru.map_record([(l, l) for l in range(100)])], count=100)).sizes.tolist() == list(range(100))


def test_ledgers_map_absent():
    log, _, _, sizes = ru.mapped_log()
    pairs = pairs_of(sizes)
    v0 = ru.with_header(log, [ru.map_record(pairs)], version=0, count=len(pairs))
    assert read_map(v0) == (0, [], 0, (0, len(log), len(pairs)), el.LEDGERS_MAP_ABSENT)
    no_offset = ru.with_header(log, [ru.map_record(pairs)], offset=0, count=len(pairs))
    assert read_map(no_offset) == (0, [], 0, (1, 0, len(pairs)), el.LEDGERS_MAP_ABSENT)
    assert el.read_ledgers_map(no_offset).state == el.LEDGERS_MAP_ABSENT


@pytest.mark.parametrize("case, says", [
    ("ledger", "ledger id is not -1"), ("entry", "entry id is not -2"), ("long", "longer than its count"),
    ("short", "shorter than its count"), ("cut", "cut by the end of the buffer"), ("count", "distinct ledgers"),
    ("zero", "header count of 0")])
def test_ledgers_map_malformed(case, says):
    log, _, _, sizes = ru.mapped_log()
    pairs = pairs_of(sizes)
    n = len(pairs)
    full = {
        "ledger": lambda: ru.with_header(log, [ru.map_record(pairs, lid=5)], count=n),
        "entry": lambda: ru.with_header(log, [ru.map_record(pairs, eid=-3)], count=n),
        "long": lambda: ru.with_header(log, [ru.map_record(pairs, extra=16)], count=n),
        "short": lambda: ru.with_header(log, [ru.map_record(pairs, extra=-16)], count=n),
        "cut": lambda: ru.with_header(log, [ru.map_record(pairs)], count=n)[:-5],
        "count": lambda: ru.with_header(log, [ru.map_record(pairs)], count=n + 1),
        "zero": lambda: ru.with_header(log, [ru.map_record([])], count=0),  # a record of no pairs: 0 distinct ledgers
    }[case]()
    rc, got, count, hdr, state = read_map(full)
    assert rc == 0 and state == el.LEDGERS_MAP_MALFORMED
    assert says in last_error(), last_error()
    m = el.read_ledgers_map(full)
    assert m.state == el.LEDGERS_MAP_MALFORMED and says in m.why


# ---- the shared rules, the route-1 pass and the map reader under a sanitizer: a stand-alone program ----

def test_scrub_report_under_address_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "scrub_report_sanitize")
    srcs = [os.path.join(here, "scrub_report_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                      ("host_scrub.cpp", "host_mac.cpp", "host_batch.cpp",
                                                                       "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    # the mixed log's first 200 entries, the signed-id log behind them, and an entry that ends on the log's last byte
    buf, expect, specs, _, _ = su.mixed_case()
    sbuf, soffs, slens, _, _ = ru.signed_ids_logs()[1]
    listed = {l: s for l, s in specs.items() if l != 99}
    listed.update({8: "DUMMY", 9: "DUMMY"})  # 7 is CRC32 in the mixed log: the signed-id log's CRC32C frames fail there
    table = el.LedgerTable.from_ledgers(listed)
    log = np.concatenate([buf, sbuf[:int(soffs.max() + slens[soffs.argmax()])]])
    offs = np.concatenate([np.array([e[2] for e in expect[:200]], dtype=np.uint64), soffs + np.uint64(buf.size)])
    lens = np.concatenate([np.array([e[3] for e in expect[:200]], dtype=np.uint32), slens])
    assert int((offs + lens).max()) == log.size
    want = su.want_of_index(log, offs, lens, listed)
    rows, nbad, bad = ru.want_report(log, offs, lens, table, want)
    capacity = nbad - 3
    # map cases: a record that ends on the buffer's last byte, and the malformed ones cut at every length
    mlog, _, _, sizes = ru.mapped_log()
    pairs = pairs_of(sizes)
    good = ru.with_header(mlog[:ru.HEADER], [ru.map_record(pairs[:2]), ru.map_record(pairs[2:])], count=len(pairs))
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(struct.pack("<7Q", log.size, offs.size, len(table), table.nkeys, su.ALL, capacity, len(good)))
        for a in (log, offs, lens, table.ids, table.types, table.keys, table.key_states, np.frombuffer(good, dtype=np.uint8)):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert [int(x) for x in lines[0].split()[1:]] == [int(w) for w in rows.reshape(-1)]
    got = [int(x) for x in lines[1].split()[1:]]
    assert got[0] == nbad and got[1:] == bad[:capacity].tolist()
    assert lines[2].split() == ["map", "0", str(len(pairs))] + [str(v) for p in pairs for v in p]
    # every prefix of the good map log read from an allocation of exactly its size: states only, no report
    states = [int(x) for x in lines[3].split()[1:]]
    assert len(states) == len(good) - ru.HEADER + 1 and states[-1] == 0 and states[0] == 2 and set(states) <= {0, 2}
