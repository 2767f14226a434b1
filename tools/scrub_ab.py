"""A/B of the mixed-ledger entry-log scrub (bkd_entrylog_verify_ledgers), in ONE process on the same device
bytes: HIP events on the stream, median of 5, every group of legs in both orders.

  1  1M HMAC frames with bench.zipf_index lengths (64 B - 64 KiB payloads) over 1 024 ledgers, a key each,
     entries of all ledgers interleaved as a log holds them:
       a   the new call, lanes binned by length (the default)
       b   the new call with bkd_set_scrub_order(1): the same kernels in index order
       c   the route without it: the index sorted by ledger on the host, one request per ledger, through
           bkd_digest_verify_requests_mac with BKD_REQUEST_SKIP_ENTRY_ID — through this library and through
           the parent commit's (SCRUB_AB_PARENT_LIB). Device time only; the host sort is reported apart.
  2  a pure CRC32C log of 1M x 4 KiB: the new call against bkd_entrylog_verify (the cost of classify and merge)
  3  a log mixing all four types: workload 1's bytes with the ledgers' types rotated

Before timing, every frame of workload 1 must verify on every leg, sampled frames must equal hmac's, and the
legs of workloads 2 and 3 must agree status for status.

Usage (GPU box): python3 tools/scrub_ab.py   Environment: SCRUB_AB_N (entries, default 1M), SCRUB_AB_REPS (5),
SCRUB_AB_PARENT_LIB (the parent commit's libbkdigest.so; its legs are left out when unset), SCRUB_AB_LOG
(default profiles/scrub_ab_1m.log).
"""
import ctypes
import hashlib
import hmac
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("SCRUB_AB_N", str(1 << 20)))
REPS = int(os.environ.get("SCRUB_AB_REPS", "5"))
PARENT = os.environ.get("SCRUB_AB_PARENT_LIB", "")
LOG = os.environ.get("SCRUB_AB_LOG", os.path.join(ROOT, "profiles", "scrub_ab_1m.log"))
NLEDGERS = 1024


def main():
    import numpy as np
    import torch

    import bench
    from bookkeeper_amd import _native
    from bookkeeper_amd import checksum as ck
    from bookkeeper_amd import digest as dg
    from bookkeeper_amd import entrylog as el

    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log = open(LOG, "w")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    L = _native.lib()
    parent = None
    if PARENT:
        parent = ctypes.CDLL(PARENT)
        for name in ("bkd_digest_verify_requests_mac", "bkd_stream_sync"):
            res, args = _native.PROTOTYPES[name]
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, args
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    say(f"scrub_ab: {torch.cuda.get_device_name(0)}, {N} entries, {NLEDGERS} ledgers, reps {REPS}, "
        f"parent library {'loaded' if parent else 'not given'}")

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
        return sorted(ms)

    def run_legs(title, legs, gb):
        """Every leg in the given order and in the reverse one; per leg the samples of both passes."""
        samples = {name: [] for name, _ in legs}
        for order in (legs, legs[::-1]):
            for name, fn in order:
                samples[name].append(timed(fn))
        med = {}
        for name, _ in legs:
            both = sorted(samples[name][0] + samples[name][1])
            meds = [s[len(s) // 2] for s in samples[name]]
            med[name] = sum(meds) / 2
            say(f"{title} {name:44s} median {meds[0]:9.3f} / {meds[1]:9.3f} ms (first / reverse pass)  "
                f"min {both[0]:9.3f} max {both[-1]:9.3f}  {gb / (med[name] / 1e3):7.1f} GB/s")
        return med, {name: (min(s[0] + s[1]), max(s[0] + s[1])) for name, s in samples.items()}

    # ---- workload 1: the log ----
    _, plens = bench.zipf_index(N)
    plens = plens.astype(np.int64)
    flens = plens + 52
    foffs = np.zeros(N, dtype=np.int64)
    np.cumsum(flens[:-1] + 4, out=foffs[1:])  # [int32 size][entry] records
    foffs += 1024 + 4
    log_size = int(foffs[-1] + flens[-1])
    ledger_row = ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(NLEDGERS)
    ledger_row = ledger_row.astype(np.int64)
    ledger_ids = 1000 + np.arange(NLEDGERS, dtype=np.int64) * 0x100000001  # ascending, distinct in both words
    passwords = [b"ledger-%d" % k for k in range(NLEDGERS)]
    table = el.LedgerTable.from_ledgers({int(l): ("HMAC", p) for l, p in zip(ledger_ids, passwords)})
    assert (table.ids == ledger_ids).all()
    d_ids, d_types, d_keys, d_states = table.on(dev)
    d_log = torch.empty((log_size + 3) & ~3, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(d_log, 2025)
    d_foff = torch.from_numpy(foffs).to(dev)
    d_flen = torch.from_numpy(flens.astype(np.int32)).to(dev)
    d_row = torch.from_numpy(ledger_row).to(dev)
    idx = torch.arange(N, **i64)
    heads, _ = dg.package_batch_ledgers_mac(d_states, d_keys[d_row].contiguous(), d_ids[d_row].contiguous(), idx, idx - 1,
                                            torch.from_numpy(plens).to(dev), d_log, d_foff + 52,
                                            torch.from_numpy(plens.astype(np.int32)).to(dev), sync_check=True)
    where = (d_foff[:, None] + torch.arange(52, **i64)[None, :]).view(-1)
    d_log[where] = heads.view(-1)
    del where, heads
    torch.cuda.synchronize()
    gb1 = float(flens.sum()) / 1e9
    say(f"workload 1: log of {log_size} bytes, frames {int(flens.min())}..{int(flens.max())} B, {gb1:.2f} GB of frames")
    for i in (0, 1, N // 3, N - 1):
        e = d_log[int(foffs[i]):int(foffs[i] + flens[i])].cpu().numpy().tobytes()
        key = hashlib.sha1(b"mac" + passwords[int(ledger_row[i])]).digest()
        assert int.from_bytes(e[:8], "big") == int(ledger_ids[ledger_row[i]])
        assert hmac.digest(key, e[:32] + e[52:], "sha1") == e[32:52], f"frame {i}"

    status = torch.empty(N, **i32)
    fb = torch.empty(1, **i64)

    def scrub(types_t=d_types, mask=el.DIGEST_ALL, out=status):
        rc = L.bkd_entrylog_verify_ledgers(ptr(d_log), log_size, ptr(d_foff), ptr(d_flen), N, ptr(d_ids), ptr(types_t),
                                           ptr(d_keys), NLEDGERS, ptr(d_states), NLEDGERS, mask, ptr(out), ptr(fb), sp)
        assert rc == 0, rc

    def leg_a():
        L.bkd_set_scrub_order(0)
        scrub()

    def leg_b():
        L.bkd_set_scrub_order(1)
        scrub()
        L.bkd_set_scrub_order(0)

    # the parent's route: the index sorted by ledger on the host, one request per ledger
    t0 = time.perf_counter()
    order = np.argsort(ledger_row, kind="stable")
    s_off, s_len = foffs[order], flens[order].astype(np.int32)
    counts = np.bincount(ledger_row, minlength=NLEDGERS)
    req_first = np.zeros(NLEDGERS + 1, dtype=np.int64)
    np.cumsum(counts, out=req_first[1:])
    sort_ms = (time.perf_counter() - t0) * 1e3
    say(f"workload 1: host sort of the index by ledger (argsort, gather, CSR) {sort_ms:.1f} ms, not in leg c")
    d_soff, d_slen = torch.from_numpy(s_off).to(dev), torch.from_numpy(s_len).to(dev)
    d_first = torch.from_numpy(req_first).to(dev)
    d_zero = torch.zeros(NLEDGERS, **i64)
    d_flags = torch.ones(NLEDGERS, **i32)  # BKD_REQUEST_SKIP_ENTRY_ID
    d_rkeys = torch.arange(NLEDGERS, **i32)
    sstatus = torch.empty(N, **i32)
    prefix = torch.empty(NLEDGERS, **i64)

    def leg_c(lib):
        def run():
            rc = lib.bkd_digest_verify_requests_mac(ptr(d_states), NLEDGERS, ptr(d_rkeys), ptr(d_log), log_size, ptr(d_soff),
                                                    ptr(d_slen), N, ptr(d_first), NLEDGERS, ptr(d_ids), ptr(d_zero),
                                                    ptr(d_flags), ptr(sstatus), ptr(prefix), sp)
            assert rc == 0, rc
        return run

    leg_a()
    assert L.bkd_stream_sync(sp) == 0 and not status.any() and int(fb.item()) == N, "leg a"
    status.fill_(-7)
    leg_b()
    assert L.bkd_stream_sync(sp) == 0 and not status.any() and int(fb.item()) == N, "leg b"
    for lib in [L] + ([parent] if parent else []):
        sstatus.fill_(-7)
        leg_c(lib)()
        assert lib.bkd_stream_sync(sp) == 0 and not sstatus.any() and bool((prefix.cpu() == torch.from_numpy(counts)).all()), "leg c"
    say(f"parity ok: sampled frames equal hmac's, all {N} frames verify on every leg")
    legs = [("a  new call, binned", leg_a), ("b  new call, index order", leg_b),
            ("c  sorted by ledger, requests_mac, this library", leg_c(L))]
    if parent:
        legs.append(("c' sorted by ledger, requests_mac, parent library", leg_c(parent)))
    med, spread = run_legs("1", legs, gb1)
    a, b, c = med[legs[0][0]], med[legs[1][0]], med[legs[2][0]]
    say(f"workload 1: b / a = {b / a:.3f}   c / a = {c / a:.3f}   (lane model: 0.922 / 0.117 = 7.9)")
    if parent:
        cp = med[legs[3][0]]
        gap = cp - a
        widest = max(spread[legs[0][0]][1] - spread[legs[0][0]][0], spread[legs[3][0]][1] - spread[legs[3][0]][0])
        say(f"workload 1: parent c' / a = {cp / a:.3f}; gap {gap:.3f} ms against the wider leg's spread {widest:.3f} ms: "
            f"{'a is faster beyond the spread' if gap > widest else 'NOT beyond the spread'}")

    # ---- workload 3: the same bytes, the ledgers' types rotated over all four ----
    mixed_types = torch.from_numpy((np.array([2, 0, 1, 3])[np.arange(NLEDGERS) % 4]).astype(np.int32)).to(dev)
    st3 = [torch.empty(N, **i32), torch.empty(N, **i32)]
    for o in (0, 1):
        L.bkd_set_scrub_order(o)
        scrub(mixed_types, out=st3[o])
    L.bkd_set_scrub_order(0)
    assert L.bkd_stream_sync(sp) == 0 and torch.equal(st3[0], st3[1])
    t_of = mixed_types[d_row]
    s3 = st3[0]
    assert not s3[t_of == 2].any() and not s3[t_of == 3].any() and bool((s3[t_of < 2] == 2).all()), "workload 3 statuses"
    del st3

    def leg3(o):
        def run():
            L.bkd_set_scrub_order(o)
            scrub(mixed_types)
            L.bkd_set_scrub_order(0)
        return run
    say("workload 3: HMAC / CRC32C / CRC32 / DUMMY ledgers in turn over workload 1's bytes (the CRC frames fail their "
        "digests: status 2 on both orders)")
    run_legs("3", [("new call, binned", leg3(0)), ("new call, index order", leg3(1))], gb1)
    del d_log, d_soff, d_slen, sstatus
    torch.cuda.empty_cache()

    # ---- workload 2: a pure CRC32C log of N x 4 KiB ----
    FL = 4096
    log2_size = 1024 + N * (FL + 4)
    d_log2 = torch.empty((log2_size + 3) & ~3, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(d_log2, 7)
    off2 = 1024 + 4 + torch.arange(N, **i64) * (FL + 4)
    len2 = torch.full((N,), FL, **i32)
    lid_bytes = torch.tensor(list((1000).to_bytes(8, "big")), dtype=torch.uint8, device=dev)
    d_log2[(off2[:, None] + torch.arange(8, **i64)[None, :]).view(-1)] = lid_bytes.repeat(N)
    crc_types = torch.zeros(NLEDGERS, **i32)
    st_new, st_old = torch.empty(N, **i32), torch.empty(N, **i32)

    def new2():
        rc = L.bkd_entrylog_verify_ledgers(ptr(d_log2), log2_size, ptr(off2), ptr(len2), N, ptr(d_ids), ptr(crc_types),
                                           None, NLEDGERS, None, 0, 1, ptr(st_new), ptr(fb), sp)
        assert rc == 0, rc

    def old2():
        rc = L.bkd_entrylog_verify(0, ptr(d_log2), log2_size, ptr(off2), ptr(len2), N, ptr(st_old), ptr(fb), sp)
        assert rc == 0, rc

    new2()
    old2()
    assert L.bkd_stream_sync(sp) == 0 and torch.equal(st_new, st_old) and bool((st_new == 2).all()), "workload 2"
    say(f"workload 2: {N} x {FL} B CRC32C frames of one listed ledger (random digests: status 2 from both calls)")
    med2, _ = run_legs("2", [("bkd_entrylog_verify_ledgers", new2), ("bkd_entrylog_verify", old2)], N * FL / 1e9)
    say(f"workload 2: new / old = {med2['bkd_entrylog_verify_ledgers'] / med2['bkd_entrylog_verify']:.3f} "
        f"(classify, scan and merge over {N} entries)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
