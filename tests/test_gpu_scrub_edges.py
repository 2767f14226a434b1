"""The mixed-ledger scrub on the GPU at its edges: the lane order itself (bkd_entrylog_scrub_lanes against the
bin rule restated in scrub_util), every alignment against every length across two SHA-1 block boundaries with
flipped tail bytes and two fillers, the first failure pinned to the ends of waves and blocks for every class
that can fail, bins up to the cap frame's bin 72, one stream over changing shapes and masks, four threads on
four streams, and indexes the record walk never produces. Every expected status comes from hmac,
oracle.verify_entry and the DUMMY length rule (scrub_util); test_scrub_edges_cpu.py runs the same logs through
the CPU route."""
import ctypes
import threading
import time

import numpy as np
import pytest

import scrub_util as su
from bookkeeper_amd import checksum as ck, entrylog as el
from bookkeeper_amd._native import lib

pytestmark = pytest.mark.gpu


@pytest.fixture()
def both_orders():
    """Runs fn(order) for the binned and the index order and puts the default back."""
    def run(fn):
        try:
            out = []
            for order in (0, 1):
                assert lib().bkd_set_scrub_order(order) == 0
                out.append(fn(order))
            return out
        finally:
            lib().bkd_set_scrub_order(0)
    return run


def check_status(got, want, sync_want=0):
    sync, status, fb = got
    assert sync == sync_want
    assert (status == want).all(), np.nonzero(status != want)[0][:10]
    assert fb == su.want_first_bad(want)
    return status


# ---- 1. the lane order ----

def check_lanes(gpu, log, order, types=su.ALL, sync_want=0, **kw):
    """Order 0: the lanes are exactly the entries the reference says are hashed, bins non-increasing (the order
    inside a bin comes from atomics). Order 1: the identity over all n. Returns the bins in lane order."""
    buf, offs, lens, table, _ = log
    ref = su.hashed_entries(buf, offs, lens, table, types, log_size=kw.get("log_size"))
    sync, lanes, nlanes = su.run_lanes(gpu, buf, offs, lens, table, types, **kw)
    assert sync == sync_want
    n = len(offs)
    if order == 1:
        assert nlanes == n and (lanes == np.arange(n)).all()
        return []
    assert nlanes == len(ref)
    assert sorted(lanes[:nlanes].tolist()) == ref.tolist()  # a permutation: no duplicate, no stranger
    bins = [su.bin_of(int(lens[i])) for i in lanes[:nlanes]]
    assert all(a >= b for a, b in zip(bins, bins[1:])), bins[:40]
    return bins


def prefix(log, n):
    buf, offs, lens, table, want = log
    return buf, offs[:n], lens[:n], table, want[:n]


def test_lanes_bins_and_wave_cuts(gpu, both_orders):
    log = su.bins_log()
    bins = both_orders(lambda order: check_lanes(gpu, log, order))[0]
    assert len(bins) == len(log[1]) and len(set(bins)) >= 12
    counts = sorted(bins.count(b) for b in set(bins))
    assert {1, 63, 64, 65} == set(counts)


def test_lanes_mixed_log(gpu, both_orders):
    log = su.mixed_log5()
    bins = both_orders(lambda order: check_lanes(gpu, log, order))[0]
    assert 100 < len(bins) < len(log[1]) - 100 and len(set(bins)) >= 8  # HMAC among CRC, DUMMY, unlisted
    # HMAC only: the same lanes
    assert both_orders(lambda order: check_lanes(gpu, log, order, types=su.TYPE_BIT["HMAC"]))[0] == bins


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_lanes_block_edges(gpu, both_orders, n):
    bins = both_orders(lambda order: check_lanes(gpu, prefix(su.bins_log(), n), order))[0]
    assert len(bins) == n


def test_lanes_one_bin_three_blocks(gpu, both_orders):
    """600 frames of one length: every rank comes from the global cursor of one bin."""
    bins = both_orders(lambda order: check_lanes(gpu, su.one_length_log(), order))[0]
    assert len(bins) == 600 and len(set(bins)) == 1


def test_lanes_short_unreadable_and_none(gpu, both_orders):
    # lengths 0-60 of every type: of the HMAC ledger's, only 52-60 are lanes
    entries, _, table = su.short_entries()
    buf, offs, lens = su.pack_entries(entries)
    bins = both_orders(lambda order: check_lanes(gpu, (buf, offs, lens, table, None), order))[0]
    assert len(bins) == 9
    # a ledger whose key row is >= nkeys and an entry past the log: no lanes, and the flag is raised
    buf, offs, lens, table, _ = su.mixed_log5()
    keys = table.keys.copy()
    row = int(np.nonzero(table.types == el.DIGEST_HMAC)[0][1])
    keys[row] = table.nkeys
    bad = el.LedgerTable(table.ids, table.types, keys, table.key_states)
    offs2 = np.concatenate([[np.uint64(buf.size - 60)], offs]).astype(np.uint64)
    lens2 = np.concatenate([[np.uint32(61)], lens]).astype(np.uint32)
    ok = both_orders(lambda order: check_lanes(gpu, (buf, offs, lens, table, None), order))[0]
    fewer = both_orders(lambda order: check_lanes(gpu, (buf, offs2, lens2, bad, None), order,
                                                  sync_want=su.BKD_ERR_BOUNDS))[0]
    assert 0 < len(fewer) < len(ok)
    # no HMAC entry at all: the HMAC ledgers of the log are not listed, the one listed HMAC ledger wrote nothing
    none = el.LedgerTable.from_ledgers({3: "CRC32C", 7: "CRC32", 20: "DUMMY", 555: ("HMAC", b"unused")})
    bins = both_orders(lambda order: check_lanes(gpu, (buf, offs, lens, none, None), order))[0]
    assert bins == []


def test_lanes_two_calls_one_stream(gpu, both_orders):
    """The counts and cursors are reset per call: large, the same again, small, large on one stream."""
    import torch
    st = torch.cuda.Stream(gpu)
    big, small = su.bins_log(), prefix(su.mixed_log5(), 70)

    def run(order):
        first = check_lanes(gpu, big, order, stream=st)
        assert check_lanes(gpu, big, order, stream=st) == first
        check_lanes(gpu, small, order, stream=st)
        assert check_lanes(gpu, big, order, stream=st) == first
    both_orders(run)
    ck.release_stream(st)


# ---- 2. alignment x length ----

@pytest.mark.parametrize("end_mod", [None, 1, 2, 3])
def test_alignment_length_sweep(gpu, both_orders, end_mod):
    """Every length over two block boundaries at every alignment, a third with the last byte flipped, a third
    with byte 8 flipped; filler 0x00 and 0xFF between the entries and behind log_size give the same statuses.
    end_mod: the last entry ends on the last byte of a log of that size mod 4."""
    zeros, ones = su.sweep_log(0x00, end_mod), su.sweep_log(0xFF, end_mod)
    want = zeros[4]
    assert (want == ones[4]).all() and (zeros[1] == ones[1]).all()
    assert zeros[0].size % 4 == (end_mod or zeros[0].size % 4)

    def run(order):
        for buf, offs, lens, table, _ in (zeros, ones):
            for pad in (0x00, 0xFF):
                check_status(su.run_device(gpu, buf, offs, lens, table, pad=pad), want)
    both_orders(run)
    for buf, offs, lens, table, _ in (zeros, ones):
        with ck.host_batch_route(ck.HOST_ROUTE_GPU):
            rc_g, st_g, fb_g = su.run_host(buf, offs, lens, table)
        with ck.host_batch_route(ck.HOST_ROUTE_CPU):
            rc_c, st_c, fb_c = su.run_host(buf, offs, lens, table)
        assert rc_g == 0 and rc_c == 0
        assert st_g.tobytes() == st_c.tobytes() == want.tobytes() and fb_g == fb_c == su.want_first_bad(want)


# ---- 3. where the first failure is ----

@pytest.mark.parametrize("kind", su.FB_KINDS)
@pytest.mark.parametrize("p", su.FB_POSITIONS)
def test_first_bad_placement(gpu, both_orders, p, kind):
    """The first failure at the ends of waves and blocks, for every class that writes a failing status (HMAC from
    mac_scrub_kernel, CRC32C and CRC32 through the merge, final statuses from classify), with a later lane of the
    same wave and an entry of a later block failing too."""
    buf, offs, lens, table, want = su.first_bad_log(p, kind)
    assert su.want_first_bad(want) == p and want[p] == su.FB_KIND_STATUS[kind]
    if kind == "hmac":
        both_orders(lambda order: check_status(su.run_device(gpu, buf, offs, lens, table), want))
    else:
        check_status(su.run_device(gpu, buf, offs, lens, table), want)


def test_first_bad_none(gpu, both_orders):
    buf, offs, lens, table, want = su.first_bad_log()
    for sync, status, fb in both_orders(lambda order: su.run_device(gpu, buf, offs, lens, table)):
        assert sync == 0 and not status.any() and fb == len(want) == su.FB_N


# ---- 4. long bins ----

def test_long_bins_and_cap_frames(gpu, both_orders):
    """Bins 27 .. 58 and the cap's bin 72: two frames of exactly BKD_MAC_MAX_ENTRY (one with its last byte
    flipped) and an entry of cap + 1 next to them, in both orders."""
    import torch
    log = su.long_bins_log()
    buf, offs, lens, table, want = log
    assert su.bin_of(su.MAC_MAX_ENTRY) == 72 and (lens == su.MAC_MAX_ENTRY).sum() == 2
    assert len({su.bin_of(int(n)) for n in lens if n <= su.MAC_MAX_ENTRY}) >= 30
    cap = np.nonzero(lens >= su.MAC_MAX_ENTRY)[0]
    assert want[cap].tolist() == [0, 2, 1] and cap.tolist() == [20, 21, 22]
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros(-buf.size % 4, dtype=np.uint8)])).to(gpu)
    kw = dict(d_buf=d_buf, log_size=buf.size)

    def run(order):
        bins = check_lanes(gpu, log, order, sync_want=su.BKD_ERR_BOUNDS, **kw)
        assert order == 1 or (bins[:2] == [72, 72] and len(bins) == len(want) - 1)
        t = time.perf_counter()
        check_status(su.run_device(gpu, buf, offs, lens, table, **kw), want, su.BKD_ERR_BOUNDS)
        print(f"long bins, order {order}: {time.perf_counter() - t:.3f} s")
    both_orders(run)


# ---- 5. one stream, changing shapes ----

def test_one_stream_changing_shapes(gpu, both_orders):
    import torch
    st = torch.cuda.Stream(gpu)
    sp = ctypes.c_void_p(int(st.cuda_stream))
    steps = su.shape_steps()
    assert [len(s[0][4]) for s in steps] == [2000, 5, 700, 3, 2000]

    def run(order):
        seen = []
        for (buf, offs, lens, table, want), types, null_keys, sync_want in steps:
            got = su.run_device(gpu, buf, offs, lens, table, types=types, null_keys=null_keys, stream=st)
            seen.append(check_status(got, want, sync_want))
            assert lib().bkd_stream_sync(sp) == 0  # a raised flag is reported once
        assert (seen[0] == seen[4]).all()
    both_orders(run)
    assert lib().bkd_stream_release(sp) == 0


# ---- 6. four threads, four streams ----

def test_four_threads_four_streams(gpu):
    """Four host threads at once, each with its own stream, log, ledger table and passwords: five calls each
    (the whole log and a prefix alternating), every status and first_bad against the reference. The lane order
    is a process-wide switch and stays at its default."""
    import torch
    logs = [su.thread_log(k) for k in range(4)]
    for log in logs:
        log[3].on(gpu)
    torch.cuda.synchronize()
    assert lib().bkd_get_scrub_order() == 0
    errors = []

    def worker(k):
        try:
            st = torch.cuda.Stream(device=gpu)
            buf, offs, lens, table, want = logs[k]
            for r in range(5):
                n = len(want) if r % 2 == 0 else 100 + 31 * k + r
                sync, status, fb = su.run_device(gpu, buf, offs[:n], lens[:n], table, stream=st)
                assert sync == 0, ("sync", k, r)
                assert (status == want[:n]).all(), ("status", k, r, np.nonzero(status != want[:n])[0][:10])
                assert fb == su.want_first_bad(want[:n]), ("first_bad", k, r)
            ck.release_stream(st)
        except BaseException as e:  # surfaced below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert errors == []
    for log in logs:
        assert {-1, 0, 2} <= set(log[4].tolist())


# ---- 7. index shapes ----

def test_index_shapes(gpu, both_orders):
    """Descending offsets, entries listed three times, frames inside another frame's payload."""
    for buf, offs, lens, table, want in su.index_shapes():
        both_orders(lambda order: check_status(su.run_device(gpu, buf, offs, lens, table), want))
        both_orders(lambda order: check_lanes(gpu, (buf, offs, lens, table, want), order))
