"""The mixed-ledger entry-log scrub on the GPU (bkd_entrylog_verify_ledgers): every status against
oracle.verify_entry (CRC), hmac (HMAC) and the length rule (DUMMY); the length bins and their wave cuts in
both lane orders; short and unreadable entries; the table search; type masks; equivalence with the
single-type calls; the host form's two routes."""
import ctypes

import numpy as np
import pytest

import bench
import scrub_util as su
from bookkeeper_amd import checksum as ck, entrylog as el
from bookkeeper_amd._native import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    return su.mixed_case()


def index_of(expect):
    return (np.array([e[2] for e in expect], dtype=np.uint64), np.array([e[3] for e in expect], dtype=np.uint32))


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


# ---- 1. the mixed log ----

def test_mixed_log(gpu, mixed, both_orders):
    buf, expect, specs, table, want = mixed
    offs, lens = index_of(expect)
    for sync, status, fb in both_orders(lambda order: su.run_device(gpu, buf, offs, lens, table)):
        assert sync == 0
        assert (status == want).all(), np.nonzero(status != want)[0][:10]
        assert fb == su.want_first_bad(want)
    assert {-1, 0, 2} <= set(want.tolist()) and (want == 2).sum() >= 20
    # the Python surface walks the records itself
    scan, status = el.EntryLogScrubber.verify_ledgers(buf, table)
    assert (scan.offsets == offs).all() and (status == want).all()
    # EntryLogScrubber.verify on the CRC ledgers agrees where both check
    crc = {l: s for l, s in specs.items() if l != 99 and s in ("CRC32C", "CRC32")}
    _, old = el.EntryLogScrubber(lambda lid: crc.get(lid)).verify(buf)
    both = old != -1
    assert both.sum() > 100 and (old[both] == status[both]).all()


# ---- 2. bins and wave cuts ----

def test_bins_and_wave_cuts(gpu, both_orders):
    """Frames at both ends of B = 1 .. 65 compressions; bins of 1, 63, 64 and 65 entries interleaved in arrival
    order (a bin that ends inside a wave, on its edge, one past it); a corrupt frame in every bin (su.bins_log)."""
    buf, offs, lens, table, want = su.bins_log()
    by_bin = {su.bin_of(int(n)) for n in lens}
    assert (want == 2).sum() == len(by_bin) and len(by_bin) >= 12
    results = both_orders(lambda o: su.run_device(gpu, buf, offs, lens, table))
    for sync, status, fb in results:
        assert sync == 0 and (status == want).all(), np.nonzero(status != want)[0][:10]
        assert fb == su.want_first_bad(want)


def test_zipf_lengths_and_one_long_entry(gpu, both_orders):
    """4 096 entries of bench.zipf_index lengths and one 1 MiB entry among them: both orders equal hmac's."""
    rng = np.random.default_rng(33)
    _, plens = bench.zipf_index(4096)
    plens = [int(x) for x in plens]
    plens[1777] = (1 << 20) - 52
    ledgers = {10 + k: ("HMAC", b"key%d" % k) for k in range(7)}
    table = el.LedgerTable.from_ledgers(ledgers)
    blob = rng.integers(0, 256, max(plens), dtype=np.uint8).tobytes()
    entries = []
    for i, n in enumerate(plens):
        lid = 10 + i % 7
        s = int(rng.integers(0, len(blob) - n + 1))
        e = su.frame_for(ledgers[lid], lid, i, blob[s:s + n])
        if i % 97 == 5:
            e = e[:40] + bytes([e[40] ^ 1]) + e[41:]
        entries.append(e)
    buf, offs, lens = su.pack_entries(entries)
    want = np.array([su.want_status(e, ledgers[10 + i % 7]) for i, e in enumerate(entries)], dtype=np.int32)
    assert (want == 2).sum() == len(range(5, 4096, 97))
    results = both_orders(lambda o: su.run_device(gpu, buf, offs, lens, table))
    assert (results[0][1] == results[1][1]).all()
    for sync, status, fb in results:
        assert sync == 0 and (status == want).all() and fb == su.want_first_bad(want)


# ---- 3. short entries ----

def test_short_entries(gpu, both_orders):
    entries, want, table = su.short_entries()
    buf, offs, lens = su.pack_entries(entries)
    for sync, status, fb in both_orders(lambda o: su.run_device(gpu, buf, offs, lens, table)):
        assert sync == 0 and (status == want).all(), np.nonzero(status != want)[0][:10]
        assert fb == 0


# ---- 4. the table search on the device ----

def test_table_search(gpu):
    """The CPU lookup cases as entries of a log: an even row is a DUMMY ledger (33 bytes: 0), an odd row a
    CRC32C ledger (33 bytes: too short, 1), an id in a gap is not checked (-1)."""
    for ids, probes in su.lookup_tables() + [(np.zeros(0, dtype=np.int64), [0, -1, 5])]:
        types = np.where(np.arange(ids.size) % 2 == 0, el.DIGEST_DUMMY, el.DIGEST_CRC32C).astype(np.uint32)
        table = el.LedgerTable(ids, types, np.zeros(ids.size, dtype=np.uint32), np.zeros((0, 10), dtype=np.uint32))
        rows = {int(v): r for r, v in enumerate(ids)}
        entries = [int(p).to_bytes(8, "big", signed=True) + bytes(25) for p in probes]
        buf, offs, lens = su.pack_entries(entries, gap=3)
        want = np.array([-1 if int(p) not in rows else rows[int(p)] % 2 for p in probes], dtype=np.int32)
        sync, status, fb = su.run_device(gpu, buf, offs, lens, table, types=su.ALL & ~su.TYPE_BIT["HMAC"], null_keys=True)
        assert sync == 0 and (status == want).all(), (ids.size, np.nonzero(status != want)[0][:10])
        assert fb == su.want_first_bad(want)


# ---- 5. unreadable entries ----

def test_unreadable_entries(gpu):
    import torch
    specs = {1: "CRC32C", 2: ("HMAC", b"a"), 3: ("HMAC", b"b"), 4: ("HMAC", b"c"), 5: "DUMMY"}
    table = el.LedgerTable.from_ledgers(specs)
    keys = table.keys.copy()
    keys[2] = table.nkeys      # ledger 3
    keys[3] = 0xFFFFFFFF       # ledger 4
    pay = b"p" * 300
    huge = (2).to_bytes(8, "big") + bytes(su.MAC_MAX_ENTRY + 1 - 8)  # in range, over the cap: never hashed
    entries = [su.frame_for(specs[1], 1, 0, pay), su.frame_for(specs[2], 2, 0, pay), su.frame_for(specs[3], 3, 0, pay),
               su.frame_for(specs[4], 4, 0, pay), huge, su.frame_for(specs[5], 5, 0, pay), su.frame_for(specs[2], 2, 1, pay),
               su.frame_for(specs[1], 1, 1, pay)]
    buf, offs, lens = su.pack_entries(entries)
    offs = np.append(offs, np.uint64(buf.size - 20))  # an entry that runs past log_size
    lens = np.append(lens, np.uint32(21))
    want = [0, 0, 1, 1, 1, 0, 0, 0, 1]
    other = torch.cuda.Stream(gpu)
    mine = torch.cuda.Stream(gpu)
    sync, status, fb = su.run_device(gpu, buf, offs, lens, table, keys=keys, stream=mine)
    assert sync == su.BKD_ERR_BOUNDS
    assert status.tolist() == want and fb == 2
    assert lib().bkd_stream_sync(ctypes.c_void_p(int(other.cuda_stream))) == 0  # a second stream's flag stays clear
    assert lib().bkd_stream_sync(ctypes.c_void_p(int(mine.cuda_stream))) == 0   # read and cleared
    # without the bad rows and the two unreadable entries the flag stays clear
    keep = [0, 1, 5, 6, 7]
    sync, status, fb = su.run_device(gpu, buf, offs[keep], lens[keep], table, stream=mine)
    assert sync == 0 and status.tolist() == [0] * 5 and fb == 5
    for s in (mine, other):
        assert lib().bkd_stream_release(ctypes.c_void_p(int(s.cuda_stream))) == 0


# ---- 6. type masks ----

def test_type_masks(gpu, mixed):
    buf, expect, specs, table, want = mixed
    offs, lens = index_of(expect)
    listed = {l: s for l, s in specs.items() if l != 99}
    bit = su.TYPE_BIT
    for mask in (0, bit["CRC32C"], bit["CRC32"], bit["HMAC"], bit["DUMMY"], bit["CRC32C"] | bit["HMAC"],
                 bit["CRC32"] | bit["DUMMY"] | bit["CRC32C"]):
        want_m = np.array([su.want_status(buf[o:o + n], listed.get(lid), mask) for lid, eid, o, n in expect], dtype=np.int32)
        sync, status, fb = su.run_device(gpu, buf, offs, lens, table, types=mask, null_keys=not (mask & bit["HMAC"]))
        assert sync == 0 and (status == want_m).all(), (mask, np.nonzero(status != want_m)[0][:10])
        assert fb == su.want_first_bad(want_m)
    sync, status, fb = su.run_device(gpu, buf, offs[:0], lens[:0], table)  # n == 0
    assert sync == 0 and fb == 0


# ---- 7. equivalence with the existing calls ----

@pytest.mark.parametrize("lo,hi", [(0, 6000), (4096, 4096)])  # ragged: the plan; one length: the fused route
def test_pure_crc32c_log_equals_entrylog_verify(gpu, lo, hi):
    import torch
    rng = np.random.default_rng(41)
    ledgers = {3: "CRC32C", 8: "CRC32C", 1 << 35: "CRC32C"}
    log, expect = su.make_mixed_log(rng, 3000, ledgers, max_payload=hi, min_payload=lo)
    buf = np.frombuffer(log, dtype=np.uint8).copy()
    for k in rng.choice(len(expect), 25, replace=False):
        buf[expect[k][2] + int(rng.integers(8, expect[k][3]))] ^= 4
    table = el.LedgerTable.from_ledgers(ledgers)
    dev = torch.from_numpy(np.concatenate([buf, np.zeros(-buf.size % 4, dtype=np.uint8)])).to(gpu)
    _, old = el.EntryLogScrubber().verify(buf, dev[:buf.size])
    offs, lens = index_of(expect)
    sync, new, fb = su.run_device(gpu, buf, offs, lens, table, types=su.TYPE_BIT["CRC32C"], null_keys=True)
    assert sync == 0 and (new == old).all() and (new == 2).sum() == 25 and fb == su.want_first_bad(old)


def test_one_ledger_hmac_log_equals_verify_batch_mac(gpu):
    import torch
    rng = np.random.default_rng(43)
    spec = ("HMAC", b"single")
    log, expect = su.make_mixed_log(rng, 700, {77: spec}, max_payload=3000)
    buf = np.frombuffer(log, dtype=np.uint8).copy()
    for k in rng.choice(len(expect), 12, replace=False):
        buf[expect[k][2] + int(rng.integers(8, expect[k][3]))] ^= 0x80
    table = el.LedgerTable.from_ledgers({77: spec})
    offs, lens = index_of(expect)
    sync, new, fb = su.run_device(gpu, buf, offs, lens, table)
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros(-buf.size % 4, dtype=np.uint8)])).to(gpu)
    d_off = torch.from_numpy(offs.view(np.int64)).to(gpu)
    d_len = torch.from_numpy(lens.view(np.int32)).to(gpu)
    d_st = torch.empty(len(expect), dtype=torch.int32, device=gpu)
    d_fb = torch.empty(1, dtype=torch.int64, device=gpu)
    ks = ck.mac_key_init(b"single")
    sp = ctypes.c_void_p(int(torch.cuda.current_stream(gpu).cuda_stream))
    assert lib().bkd_digest_verify_batch_mac(ctypes.c_void_p(ks.ctypes.data), 77, 0, 1, ctypes.c_void_p(d_buf.data_ptr()),
                                             buf.size, ctypes.c_void_p(d_off.data_ptr()), ctypes.c_void_p(d_len.data_ptr()),
                                             len(expect), ctypes.c_void_p(d_st.data_ptr()), ctypes.c_void_p(d_fb.data_ptr()),
                                             sp) == 0
    assert lib().bkd_stream_sync(sp) == 0
    old = d_st.cpu().numpy()
    assert sync == 0 and (new == old).all() and (new == 2).sum() == 12 and fb == int(d_fb.cpu().numpy()[0])


# ---- 8. the host form ----

def test_host_form_routes_agree(gpu, mixed):
    buf, expect, specs, table, want = mixed
    offs, lens = index_of(expect)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        rc_g, st_g, fb_g = su.run_host(buf, offs, lens, table)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        rc_c, st_c, fb_c = su.run_host(buf, offs, lens, table)
    assert rc_g == 0 and rc_c == 0
    assert st_g.tobytes() == st_c.tobytes() == want.tobytes() and fb_g == fb_c == su.want_first_bad(want)
    # an unreadable entry: both routes write every status, then report it
    offs2, lens2 = np.append(offs, np.uint64(buf.size)), np.append(lens, np.uint32(9))
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        rc_g, st_g, fb_g = su.run_host(buf, offs2, lens2, table)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        rc_c, st_c, fb_c = su.run_host(buf, offs2, lens2, table)
    assert rc_g == rc_c == su.BKD_ERR_BOUNDS and st_g.tobytes() == st_c.tobytes() and st_g[-1] == 1 and fb_g == fb_c
    # the automatic choice: the GPU only when the table lists an HMAC ledger whose bit is in the mask
    route = lib().bkd_get_scrub_host_route
    crc_only = el.LedgerTable.from_ledgers({1: "CRC32C", 2: "CRC32", 3: "DUMMY"})
    with ck.host_batch_route(ck.HOST_ROUTE_AUTO):
        assert route(ctypes.c_void_p(table.types.ctypes.data), len(table), su.ALL) == 2
        assert route(ctypes.c_void_p(table.types.ctypes.data), len(table), su.ALL & ~su.TYPE_BIT["HMAC"]) == 1
        assert route(ctypes.c_void_p(crc_only.types.ctypes.data), len(crc_only), su.ALL) == 1
        rc, st, fb = su.run_host(buf, offs, lens, table)
        assert rc == 0 and (st == want).all()
        scan, st2, fb2 = el.EntryLogScrubber.verify_ledgers_host(buf, table)
        assert (st2 == want).all() and fb2 == fb
