"""The scrub report on the GPU (bkd_entrylog_scrub_report): the per-ledger rows, the count and the ascending list
of bad entries against the plain-Python reference of scrub_report_util, whose statuses are scrub_util's (oracle,
hmac, the DUMMY rule). The list at the edges of waves and blocks, rows shared inside a wave in every way the
aggregation distinguishes, signed 64-bit entry ids, a byte sum over 2^32, the catch-all row, the list's capacity,
type masks, one stream over changing shapes, four threads on four streams, and the host form's two routes.
test_scrub_report_cpu.py runs the same logs through the CPU route."""
import threading

import numpy as np
import pytest

import scrub_report_util as ru
import scrub_util as su
from bookkeeper_amd import checksum as ck, entrylog as el
from bookkeeper_amd._native import lib

pytestmark = pytest.mark.gpu


def check_device(gpu, log, sync_want=0, **kw):
    got = ru.run_device(gpu, *log[:4], **kw)
    assert got[0] == sync_want
    return ru.check(got[1:], log, capacity=kw.get("capacity"), log_size=kw.get("log_size"))


# ---- the mixed log ----

def test_mixed_log(gpu):
    log = su.mixed_log5()
    buf, offs, lens, table, want = log
    rows = check_device(gpu, log)  # with d_status: the statuses are the reference's ...
    sync, status, first_bad = su.run_device(gpu, buf, offs, lens, table)
    got = ru.run_device(gpu, buf, offs, lens, table)
    assert sync == 0 and (got[4] == status).all()  # ... and bkd_entrylog_verify_ledgers's
    assert got[3][0] == first_bad == rows[:, ru.FIRST_BAD].min()  # the list's head is the old first_bad
    check_device(gpu, log, with_status=False)
    try:
        assert lib().bkd_set_scrub_order(1) == 0
        check_device(gpu, log)
        check_device(gpu, log, with_status=False)
    finally:
        lib().bkd_set_scrub_order(0)


def test_mixed_log_python(gpu):
    buf, expect, specs, table, want = su.mixed_case()
    offs, lens = su.index_of(expect)
    rows, nbad, bad = ru.want_report(buf, offs, lens, table, want)
    for rep in (el.EntryLogScrubber.report_ledgers(buf, table, max_bad=10),
                el.EntryLogScrubber.report_ledgers(buf, table, want_status=True)):
        cap = 10 if rep.status is None else len(offs)
        assert (rep.scan.offsets == offs).all() and rep.nbad == nbad and rep.bad.tolist() == bad[:cap].tolist()
        assert rep.status is None or (rep.status == want).all()
        assert (rep.rows.view(np.uint64).reshape(-1, 8) == rows[:-1]).all()
        assert (rep.other.reshape(1).view(np.uint64) == rows[-1]).all() and int(rep.other["not_checked"]) > 0
        assert rep.bad_entries() == [
            (expect[i][0], int.from_bytes(bytes(buf[expect[i][2] + 8:expect[i][2] + 16]), "big", signed=True),
             expect[i][2], expect[i][3]) for i in bad[:cap]]
        signed = rows.view(np.int64)
        assert rep.damaged() == {int(table.ids[r]): (int(rows[r, ru.BAD]), int(signed[r, ru.MIN_BAD]), int(signed[r, ru.MAX_BAD]))
                                 for r in range(len(table)) if rows[r, ru.BAD]}
        assert len(rep.damaged()) >= 5


# ---- wave and block edges of the list ----

@pytest.mark.parametrize("kind", su.FB_KINDS)
@pytest.mark.parametrize("p", su.FB_POSITIONS)
def test_list_at_wave_and_block_edges(gpu, p, kind):
    log = su.first_bad_log(p, kind)
    rows = check_device(gpu, log)
    assert rows[:, ru.BAD].sum() == (log[4] > 0).sum() == (1 if p == su.FB_N - 1 else 3)
    assert rows[:, ru.FIRST_BAD].min() == p


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_cuts_of_one_log(gpu, n):
    check_device(gpu, ru.cut(su.mixed_log5(), n))


@pytest.mark.parametrize("n", (1023, 1024, 1025))
def test_cuts_at_the_block_edge(gpu, n):
    """The report and scatter kernels' blocks are 1 024 lanes (test_every_entry_bad puts bad entries on both
    sides of the edge)."""
    check_device(gpu, ru.cut(su.shape_steps()[0][0], n))


def test_every_entry_bad(gpu):
    log = ru.all_bad_log()
    rows = check_device(gpu, log)
    assert rows[:, ru.BAD].sum() == len(log[1]) == 300
    check_device(gpu, log, capacity=257)
    log = ru.all_bad_log(1100)  # over a block edge
    check_device(gpu, log)
    check_device(gpu, log, capacity=1030)


# ---- row sharing inside a wave ----

@pytest.mark.parametrize("name", ("one_ledger", "one_ledger_blocks", "all_distinct", "round_robin", "sparse_table", "runs"))
def test_row_sharing(gpu, name):
    logs = ru.runs_log() if name == "runs" else [getattr(ru, name + "_log")()]
    for log in logs:
        rows = check_device(gpu, log)
        assert rows[:, ru.BAD].sum() > 0
        for r in ru.untouched_rows(log):
            assert rows[r].tolist() == ru.initial_row(len(log[1]))
    if name == "sparse_table":
        assert len(logs[0][3]) == 1025 and len(ru.untouched_rows(logs[0])) == 1022
    if name == "all_distinct":
        assert len(ru.untouched_rows(logs[0])) == 0 and (rows[:-1, ru.ENTRIES] == 1).all()


# ---- signed 64-bit entry ids; the 64-bit byte sum ----

def test_signed_entry_ids(gpu):
    one, spread = ru.signed_ids_logs()
    rows = check_device(gpu, one)
    for r in (0, 1):  # ledgers 7 and 8 hold every id of ENTRY_IDS
        assert rows[r, ru.MIN_BAD] == ru.I64_MIN & ru.U64 and rows[r, ru.MAX_BAD] == ru.I64_MAX
    # ledger 9's bad entries are 8 and 15 bytes long, the catch-all row's under 8: counted, the ids left alone
    assert rows[2, ru.BAD] == 2 and rows[2, ru.MIN_BAD] == ru.I64_MAX and rows[2, ru.MAX_BAD] == ru.I64_MIN & ru.U64
    assert rows[-1, ru.BAD] == 2 and rows[-1, ru.MIN_BAD] == ru.I64_MAX and rows[-1, ru.MAX_BAD] == ru.I64_MIN & ru.U64
    rows = check_device(gpu, spread)
    assert rows[0, ru.MIN_BAD] == ru.I64_MIN & ru.U64 and rows[0, ru.MAX_BAD] == (1 << 32) + 1
    assert rows[1, ru.MIN_BAD] == -1 & ru.U64 and rows[1, ru.MAX_BAD] == ru.I64_MAX


def test_byte_sum_is_64_bits_wide(gpu):
    rows = check_device(gpu, ru.big_sum_log())
    assert rows[0, ru.BYTES] == 4097 * ((1 << 20) + 4) > 1 << 32


# ---- the catch-all row ----

def test_catch_all_row(gpu):
    log = ru.catch_all_log()
    other = torch_stream()
    call = ru.DeviceCall(gpu, *su.mixed_log5()[:4], stream=other)  # another stream's call is not told
    rows = check_device(gpu, log, sync_want=su.BKD_ERR_BOUNDS)     # the report is complete all the same
    assert call.rc == 0 and call.sync() == 0
    assert lib().bkd_stream_sync(None) == 0  # the flag was read and cleared
    assert rows[-1].tolist()[:5] == [5, sum(int(l) + 4 for l in log[2][[1, 2, 3, 5, 7]]), 0, 3, 2]
    assert rows[-1, ru.FIRST_BAD] == 2 and rows[-1, ru.MIN_BAD] == ru.I64_MAX  # the out-of-range entry's id is not read
    empty = el.LedgerTable.from_ledgers({})
    rows = check_device(gpu, log[:3] + (empty, su.want_of_index(*log[:3], {})), sync_want=su.BKD_ERR_BOUNDS)
    assert rows.shape[0] == 1 and rows[0, ru.ENTRIES] == len(log[1])


def torch_stream():
    import torch
    return torch.cuda.Stream()


def test_no_entries(gpu):
    log = su.mixed_log5()
    none = (log[0], log[1][:0], log[2][:0], log[3], log[4][:0])
    got = ru.run_device(gpu, *none[:4])
    rows = ru.check(got[1:], none)
    assert got[0] == 0 and all(r.tolist() == ru.initial_row(0) for r in rows)


# ---- capacity ----

def test_capacity(gpu):
    log = su.mixed_log5()
    nbad = int((log[4] > 0).sum())
    assert nbad > 6
    for cap in (nbad - 1, nbad, nbad + 5):  # nbad - 1: the lowest indices are kept
        check_device(gpu, log, capacity=cap)
    check_device(gpu, log, capacity=0, null_bad=True)
    check_device(gpu, log, capacity=0)


# ---- masks ----

def test_masks(gpu):
    buf, offs, lens, table, _ = su.mixed_log5()
    listed = {l: s for l, s in su.mixed_case()[2].items() if l != 99}
    for mask in (su.ALL & ~su.TYPE_BIT["HMAC"], su.TYPE_BIT["CRC32C"] | su.TYPE_BIT["CRC32"]):
        want = su.want_of_index(buf, offs, lens, listed, mask)
        rows = check_device(gpu, (buf, offs, lens, table, want), types=mask, null_keys=True)
        for r, t in enumerate(table.types):
            if not (mask >> int(t)) & 1:  # masked out: the ledger keeps its row, nothing of it is checked
                assert rows[r, ru.ENTRIES] == rows[r, ru.NOT_CHECKED] > 0 and rows[r, ru.BAD] == 0


# ---- one stream, changing shapes; four threads on four streams ----

def test_one_stream_changing_shapes(gpu):
    stream = torch_stream()
    steps = su.shape_steps()
    calls = [ru.DeviceCall(gpu, *log[:4], types=types, null_keys=null_keys, stream=stream, with_status=k % 2 == 0)
             for k, (log, types, null_keys, _) in enumerate(steps)]  # no sync between the calls
    assert all(c.rc == 0 for c in calls)
    assert calls[-1].sync() == su.BKD_ERR_BOUNDS  # the fourth log's out-of-range entry
    for call, (log, _, _, _) in zip(calls, steps):
        ru.check(call.result(), log)
    assert calls[-1].sync() == 0


def test_four_threads_four_streams(gpu):
    import torch
    streams = [torch.cuda.Stream() for _ in range(4)]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(gpu)
            for _ in range(3):
                got = ru.run_device(gpu, *su.thread_log(k)[:4], stream=streams[k])
                assert got[0] == 0
                ru.check(got[1:], su.thread_log(k))
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((k, repr(e)))

    for k in range(4):
        su.thread_log(k)  # built once, before the threads
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- the host form ----

def test_host_form_routes_agree(gpu):
    for log, want_rc in ((su.mixed_log5(), 0), (ru.catch_all_log(), su.BKD_ERR_BOUNDS), (ru.signed_ids_logs()[1], 0)):
        dev = ru.run_device(gpu, *log[:4])
        for with_status in (True, False):
            with ck.host_batch_route(ck.HOST_ROUTE_GPU):
                rc2, *two = ru.run_host(*log[:4], with_status=with_status)
            with ck.host_batch_route(ck.HOST_ROUTE_CPU):
                rc1, *one = ru.run_host(*log[:4], with_status=with_status)
            assert rc1 == rc2 == dev[0] == want_rc
            ru.check(tuple(two), log)
            for a, b, c in zip(one[:3], two[:3], dev[1:4]):  # word for word
                assert np.array_equal(a, b) and np.array_equal(b, c)
            assert (two[3] is None) == (not with_status)
    log = su.mixed_log5()
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        nbad = int((log[4] > 0).sum())
        rc, *got = ru.run_host(*log[:4], capacity=nbad - 1)
        assert rc == 0
        ru.check(tuple(got), log, capacity=nbad - 1)
        rep = el.EntryLogScrubber.report_ledgers_host(log[0], log[3])
        assert rep.nbad == nbad
