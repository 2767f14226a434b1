"""A/B of the scrub report (bkd_entrylog_scrub_report) against what a caller does without it, in ONE process on
the same device bytes: HIP events for device time, wall clock for whole legs, median of 5, legs in both orders.

Workloads, SCRUB_REPORT_AB_N entries each (default 1M):
  1  4 KiB CRC32C frames of one ledger (every lane of every wave on one row)
  2  the same frames over 1 024 interleaved ledgers (up to 64 distinct rows per wave)
  3  tools/scrub_ab.py's workload 3: HMAC frames with bench.zipf_index lengths over 1 024 ledgers whose types
     rotate over HMAC / CRC32C / CRC32 / DUMMY (the CRC ledgers' frames fail their digests: half the log is bad)
Legs:
  a  bkd_entrylog_scrub_report with a NULL d_status, then the report, nbad and a 4 096-entry list copied to the host
  b  bkd_entrylog_verify_ledgers, n statuses copied to the host, then the same eight words per row by
     np.searchsorted on the scan's ledger ids and np.bincount / np.minimum.at / np.maximum.at
  c  bkd_entrylog_verify_ledgers alone (device time)
Before timing, leg a's report must equal leg b's rows word for word and its list the lowest bad indices.

Usage (GPU box): python3 tools/scrub_report_ab.py   Environment: SCRUB_REPORT_AB_N, SCRUB_REPORT_AB_REPS (5),
SCRUB_REPORT_AB_LOG (default profiles/scrub_report_ab_1m.log).
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("SCRUB_REPORT_AB_N", str(1 << 20)))
REPS = int(os.environ.get("SCRUB_REPORT_AB_REPS", "5"))
LOG = os.environ.get("SCRUB_REPORT_AB_LOG", os.path.join(ROOT, "profiles", "scrub_report_ab_1m.log"))
NLEDGERS = 1024
LIST = 4096


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
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    say(f"scrub_report_ab: {torch.cuda.get_device_name(0)}, {N} entries, reps {REPS}, list of {LIST}")

    ledger_ids = 1000 + np.arange(NLEDGERS, dtype=np.int64) * 0x100000001  # ascending, distinct in both words
    ledger_row = (((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(NLEDGERS)).astype(np.int64)
    entry_ids = np.arange(N, dtype=np.int64)

    class Work:
        """One workload on the device: the log, the index, the table, and the host's view of the scan."""

        def __init__(self, name, d_log, log_size, foffs, flens, table, types_t, mask, rows_of_entries, gb):
            self.name, self.d_log, self.log_size, self.table, self.mask, self.gb = name, d_log, log_size, table, mask, gb
            self.d_off = torch.from_numpy(foffs).to(dev)
            self.d_len = torch.from_numpy(flens.astype(np.int32)).to(dev)
            self.h_len = flens.astype(np.int64)
            self.d_ids, _, self.d_keys, self.d_states = table.on(dev)
            self.d_types = types_t
            self.scan_lids = table.ids[rows_of_entries]  # what scan_entry_log gives the caller
            self.nl = len(table)
            self.status = torch.empty(N, **i32)
            self.h_status = torch.empty(N, dtype=torch.int32).pin_memory()
            self.fb = torch.empty(1, **i64)
            self.report = torch.empty((self.nl + 1) * 8, **i64)
            self.h_report = torch.empty((self.nl + 1) * 8, dtype=torch.int64).pin_memory()
            self.bad = torch.empty(LIST, **i32)
            self.h_bad = torch.empty(LIST, dtype=torch.int32).pin_memory()
            self.nbad = torch.empty(1, **i64)
            self.h_nbad = torch.empty(1, dtype=torch.int64).pin_memory()

        def keys(self):
            mac = (self.mask >> el.DIGEST_HMAC) & 1
            return (ptr(self.d_keys), self.nl, ptr(self.d_states), self.table.nkeys) if mac else (None, self.nl, None, 0)

        def verify(self):
            rc = L.bkd_entrylog_verify_ledgers(ptr(self.d_log), self.log_size, ptr(self.d_off), ptr(self.d_len), N,
                                               ptr(self.d_ids), ptr(self.d_types), *self.keys(), self.mask,
                                               ptr(self.status), ptr(self.fb), sp)
            assert rc == 0, rc

        def report_call(self):
            rc = L.bkd_entrylog_scrub_report(ptr(self.d_log), self.log_size, ptr(self.d_off), ptr(self.d_len), N,
                                             ptr(self.d_ids), ptr(self.d_types), *self.keys(), self.mask, None,
                                             ptr(self.report), ptr(self.bad), LIST, ptr(self.nbad), sp)
            assert rc == 0, rc

        def leg_a(self):
            self.report_call()
            self.h_report.copy_(self.report, non_blocking=True)
            self.h_nbad.copy_(self.nbad, non_blocking=True)
            self.h_bad.copy_(self.bad, non_blocking=True)
            assert L.bkd_stream_sync(sp) == 0
            return self.h_report.numpy().view(np.uint64).reshape(-1, 8), int(self.h_nbad[0]), self.h_bad.numpy().view(np.uint32)

        def leg_b(self):
            self.verify()
            self.h_status.copy_(self.status, non_blocking=True)
            assert L.bkd_stream_sync(sp) == 0
            s = self.h_status.numpy()
            nl = self.nl
            r = np.searchsorted(self.table.ids, self.scan_lids)
            r = np.where((r < nl) & (self.table.ids[np.minimum(r, nl - 1)] == self.scan_lids), r, nl)
            rows = np.zeros((nl + 1, 8), dtype=np.uint64)
            rows[:, 0] = np.bincount(r, minlength=nl + 1)
            rows[:, 1] = np.bincount(r, weights=self.h_len + 4, minlength=nl + 1).astype(np.uint64)  # exact under 2^53
            bad = s > 0
            rows[:, 2] = np.bincount(r[s == 0], minlength=nl + 1)
            rows[:, 3] = np.bincount(r[bad], minlength=nl + 1)
            rows[:, 4] = np.bincount(r[s < 0], minlength=nl + 1)
            lo = np.full(nl + 1, np.iinfo(np.int64).max, dtype=np.int64)
            hi = np.full(nl + 1, np.iinfo(np.int64).min, dtype=np.int64)
            first = np.full(nl + 1, N, dtype=np.int64)
            where = np.nonzero(bad)[0]
            np.minimum.at(lo, r[where], entry_ids[where])
            np.maximum.at(hi, r[where], entry_ids[where])
            np.minimum.at(first, r[where], where)
            rows[:, 5], rows[:, 6], rows[:, 7] = lo.view(np.uint64), hi.view(np.uint64), first.view(np.uint64)
            return rows, int(where.size), where[:LIST].astype(np.uint32)

    def device_ms(fn):
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

    def wall_ms(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return sorted(ms)

    def run(work):
        rows_a, nbad_a, bad_a = work.leg_a()
        rows_b, nbad_b, bad_b = work.leg_b()
        k = min(nbad_b, LIST)
        assert nbad_a == nbad_b and np.array_equal(bad_a[:k], bad_b[:k]) and np.array_equal(rows_a, rows_b), work.name
        say(f"{work.name}: {work.gb:.2f} GB of entries, {nbad_a} bad; leg a's report equals leg b's rows word for word")
        legs = [("a  scrub_report, report + nbad + list to the host (wall)", lambda: wall_ms(work.leg_a)),
                ("b  verify_ledgers, statuses to the host, numpy rows (wall)", lambda: wall_ms(work.leg_b)),
                ("a  scrub_report (device)", lambda: device_ms(work.report_call)),
                ("c  verify_ledgers (device)", lambda: device_ms(work.verify))]
        samples = {name: [] for name, _ in legs}
        for order in (legs, legs[::-1]):
            for name, fn in order:
                samples[name].append(fn())
        med = {}
        for name, _ in legs:
            meds = [s[len(s) // 2] for s in samples[name]]
            both = sorted(samples[name][0] + samples[name][1])
            med[name] = sum(meds) / 2
            say(f"{work.name} {name:60s} median {meds[0]:9.3f} / {meds[1]:9.3f} ms (first / reverse pass)  "
                f"min {both[0]:9.3f} max {both[-1]:9.3f}")
        a, b, ad, c = (med[name] for name, _ in legs)
        say(f"{work.name}: b / a (wall) = {b / a:.2f}   a - c (device) = {ad - c:.3f} ms over {N} entries")
        return ad - c

    # ---- workloads 1 and 2: N x 4 KiB CRC32C frames, of one ledger and of 1 024 interleaved ----
    FL = 4096
    PL = FL - 36
    foffs = 1024 + 4 + np.arange(N, dtype=np.int64) * (FL + 4)
    flens = np.full(N, FL, dtype=np.int64)
    log_size = int(foffs[-1] + FL)
    d_log = torch.empty((log_size + 3) & ~3, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(d_log, 7)
    d_foff = torch.from_numpy(foffs).to(dev)
    idx = torch.arange(N, **i64)
    plen64, plen32 = torch.full((N,), PL, **i64), torch.full((N,), PL, **i32)
    crc_table = el.LedgerTable.from_ledgers({int(l): "CRC32C" for l in ledger_ids})
    crc_types = crc_table.on(dev)[1]
    head_at = (d_foff[:, None] + torch.arange(36, **i64)[None, :]).view(-1)
    delta = {}
    for name, rows in (("1 one ledger", np.zeros(N, dtype=np.int64)), ("2 1 024 ledgers", ledger_row)):
        lids = torch.from_numpy(ledger_ids[rows]).to(dev)
        heads, _ = dg.package_batch_ledgers(dg.DigestType.CRC32C, lids, idx, idx - 1, plen64, d_log, d_foff + 36, plen32, sync_check=True)
        d_log[head_at] = heads.view(-1)
        for i in (5, N // 2):  # a few payload bytes flipped: the report has bad entries to find
            d_log[int(foffs[i]) + 100] ^= 1
        torch.cuda.synchronize()
        delta[name] = run(Work(name, d_log, log_size, foffs, flens, crc_table, crc_types, 1, rows, N * FL / 1e9))
    del d_log, head_at, heads
    torch.cuda.empty_cache()

    # ---- workload 3: scrub_ab.py's: HMAC frames of Zipf lengths, the ledgers' types rotated over all four ----
    _, plens = bench.zipf_index(N)
    plens = plens.astype(np.int64)
    flens = plens + 52
    foffs = np.zeros(N, dtype=np.int64)
    np.cumsum(flens[:-1] + 4, out=foffs[1:])
    foffs += 1024 + 4
    log_size = int(foffs[-1] + flens[-1])
    table = el.LedgerTable.from_ledgers({int(l): ("HMAC", b"ledger-%d" % k) for k, l in enumerate(ledger_ids)})
    d_ids, _, d_keys, d_states = table.on(dev)
    d_log = torch.empty((log_size + 3) & ~3, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(d_log, 2025)
    d_foff = torch.from_numpy(foffs).to(dev)
    d_row = torch.from_numpy(ledger_row).to(dev)
    heads, _ = dg.package_batch_ledgers_mac(d_states, d_keys[d_row].contiguous(), d_ids[d_row].contiguous(), idx, idx - 1,
                                            torch.from_numpy(plens).to(dev), d_log, d_foff + 52,
                                            torch.from_numpy(plens.astype(np.int32)).to(dev), sync_check=True)
    d_log[(d_foff[:, None] + torch.arange(52, **i64)[None, :]).view(-1)] = heads.view(-1)
    del heads
    torch.cuda.synchronize()
    mixed_types = torch.from_numpy((np.array([2, 0, 1, 3])[np.arange(NLEDGERS) % 4]).astype(np.int32)).to(dev)
    name = "3 mixed types, Zipf lengths"
    delta[name] = run(Work(name, d_log, log_size, foffs, flens, table, mixed_types, el.DIGEST_ALL, ledger_row,
                           float(flens.sum()) / 1e9))
    say("a - c per workload: " + ", ".join(f"{k}: {v:.3f} ms" for k, v in delta.items()) +
        "  (the plain call's classify, scan and merge: 0.24 ms per 1M entries, DESIGN.md §5g workload 2)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
