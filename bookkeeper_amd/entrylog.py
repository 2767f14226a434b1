"""Bookie-side entry-log scrub.

The reference writes entries into entry-log files as ``[int32 BE size][entry]`` records after a
1024-byte header (``DefaultEntryLogger.java:256``, ``addEntryForCompaction`` :626-642) and reads
them back with ``scanEntryLog`` (:995-1060). It never re-verifies their digests on the bookie
(``BookieProtoEncoding.java:152-175``); this module adds that bulk check as a new feature:

* ``scan_entry_log`` — the record walk (host control logic, ``bkd_entrylog_index``), with the
  reference's padding / ledgers-map / short-read rules;
* ``EntryLogScrubber.verify`` — every entry's digest recomputed on the GPU
  (``bkd_entrylog_verify``) from a device-resident copy of the log, grouped by digest type;
* ``LedgerTable`` / ``EntryLogScrubber.verify_ledgers`` — a log that mixes CRC32C, CRC32, HMAC and DUMMY
  ledgers in one device call (``bkd_entrylog_verify_ledgers``): the ledger of every entry is looked up on
  the device and the HMAC frames are hashed in lanes binned by length; ``verify_ledgers_host`` from host
  memory;
* ``EntryLogScrubber.report_ledgers`` / ``ScrubReport`` — the same scrub with its per-ledger rows (entries,
  bytes, ok / bad / not checked, the range of bad entry ids) and the ascending list of bad entries made on
  the device (``bkd_entrylog_scrub_report``); ``read_ledgers_map`` reads the log's own ledgers map
  (``bkd_entrylog_ledgers_map``) and ``ScrubReport.compare_ledgers_map`` holds the two against each other.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import checksum as _ck
from ._native import CRC32, CRC32C, check, last_error, lib

BKD_ERR_BOUNDS = -4

LOGFILE_HEADER_SIZE = 1024  # DefaultEntryLogger.java:256
INVALID_LID = -1            # DefaultEntryLogger.java:277

VERIFY_OK = 0
VERIFY_TOO_SHORT = 1
VERIFY_DIGEST_MISMATCH = 2


class ScanResult:
    """Entries found by the walk: offsets of the entry bytes, lengths, ledger ids; `end` = where
    the walk stopped (== log size unless a short read ended it)."""

    def __init__(self, offsets: np.ndarray, lengths: np.ndarray, ledger_ids: np.ndarray, end: int):
        self.offsets = offsets
        self.lengths = lengths
        self.ledger_ids = ledger_ids
        self.end = end

    def __len__(self) -> int:
        return int(self.offsets.size)


def scan_entry_log(log, start: int = LOGFILE_HEADER_SIZE) -> ScanResult:
    """DefaultEntryLogger.scanEntryLog (:995-1060) over a host buffer, accepting every ledger."""
    buf = _ck._host_view(log)
    size = buf.size
    # a record takes at least 5 bytes (size field + 1 entry byte), so size // 5 + 1 always fits; start
    # smaller (ledger entries are rarely tiny) and grow when the walk finds more records than that
    cap = min(size // 5 + 1, max(64, size // 256))
    count = ctypes.c_uint64(0)
    end = ctypes.c_uint64(0)
    while True:
        offs = np.empty(cap, dtype=np.uint64)
        lens = np.empty(cap, dtype=np.uint32)
        lids = np.empty(cap, dtype=np.int64)
        rc = lib().bkd_entrylog_index(buf.ctypes.data if size else None, size, start, offs.ctypes.data,
                                      lens.ctypes.data, lids.ctypes.data, cap, ctypes.byref(count), ctypes.byref(end))
        if rc == BKD_ERR_BOUNDS and cap < size // 5 + 1:
            cap = min(size // 5 + 1, cap * 4)
            continue
        check(rc)
        break
    k = int(count.value)
    return ScanResult(offs[:k].copy(), lens[:k].copy(), lids[:k].copy(), int(end.value))


DIGEST_CRC32C, DIGEST_CRC32, DIGEST_HMAC, DIGEST_DUMMY = 0, 1, 2, 3  # BKD_DIGEST_*
DIGEST_ALL = 0xF
VERIFY_NOT_CHECKED = -1  # BKD_VERIFY_NOT_CHECKED


class LedgerTable:
    """The ledger table of ``bkd_entrylog_verify_ledgers``: ids ascending (int64), each row's digest type
    (uint32, DIGEST_*) and, for HMAC rows, its row of the key table (uint32[nkeys, 10], what
    ``bkd_mac_key_init`` writes). In BookKeeper the types and passwords come from the ledgers' metadata."""

    _TYPES = {"CRC32C": DIGEST_CRC32C, "CRC32": DIGEST_CRC32, "HMAC": DIGEST_HMAC, "DUMMY": DIGEST_DUMMY}

    def __init__(self, ids: np.ndarray, types: np.ndarray, keys: np.ndarray, key_states: np.ndarray):
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.types = np.ascontiguousarray(types, dtype=np.uint32)
        self.keys = np.ascontiguousarray(keys, dtype=np.uint32)
        self.key_states = np.ascontiguousarray(key_states, dtype=np.uint32).reshape(-1, 10)
        self._device = {}

    @classmethod
    def from_ledgers(cls, ledgers: dict) -> "LedgerTable":
        """``{ledger_id: "CRC32C" | "CRC32" | "DUMMY" | ("HMAC", passwd)}``: rows sorted by id, one key row
        per distinct password (ledgers with the same password share it)."""
        ids = sorted(int(l) for l in ledgers)
        types = np.zeros(len(ids), dtype=np.uint32)
        keys = np.zeros(len(ids), dtype=np.uint32)
        rows: dict[bytes, int] = {}
        for r, lid in enumerate(ids):
            spec = ledgers[lid]
            name, passwd = (spec, None) if isinstance(spec, str) else (spec[0], bytes(spec[1]))
            if name not in cls._TYPES or (name == "HMAC") != (passwd is not None):
                raise ValueError(f"ledger {lid}: digest type {spec!r}")
            types[r] = cls._TYPES[name]
            if passwd is not None:
                keys[r] = rows.setdefault(passwd, len(rows))
        states = np.zeros((len(rows), 10), dtype=np.uint32)
        for passwd, k in rows.items():
            states[k] = _ck.mac_key_init(passwd)
        return cls(np.array(ids, dtype=np.int64), types, keys, states)

    def __len__(self) -> int:
        return int(self.ids.size)

    @property
    def nkeys(self) -> int:
        return int(self.key_states.shape[0])

    def on(self, device):
        """(ids, types, keys, key_states) as tensors on `device`, uploaded once per device."""
        import torch
        if device not in self._device:
            self._device[device] = tuple(
                torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
                for a in (self.ids, self.types, self.keys, self.key_states.reshape(-1)))
        return self._device[device]


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data if a.size else 0)


def _default_mask(table: LedgerTable, types) -> int:
    mask = DIGEST_ALL if types is None else int(types)
    if types is None and not table.nkeys:
        mask &= ~(1 << DIGEST_HMAC)  # no HMAC ledger listed: the call needs no key table
    return mask


REPORT_WORDS = 8  # BKD_SCRUB_REPORT_WORDS
DEFAULT_MAX_BAD = 4096
# a row of the report as a structured record; the entry ids are signed (BKD_REPORT_*)
REPORT_DTYPE = np.dtype([("entries", np.uint64), ("bytes", np.uint64), ("ok", np.uint64), ("bad", np.uint64),
                         ("not_checked", np.uint64), ("min_bad_entry", np.int64), ("max_bad_entry", np.int64),
                         ("first_bad_index", np.uint64)])
LEDGERS_MAP_READ, LEDGERS_MAP_ABSENT, LEDGERS_MAP_MALFORMED = 0, 1, 2  # BKD_LEDGERS_MAP_*


class LedgersMap:
    """What ``read_ledgers_map`` found: the (ledger id, size) pairs as they lie in the log, the header's
    version, ledgersMapOffset and ledgersCount, the state (LEDGERS_MAP_*) and, for a malformed map, why."""

    def __init__(self, ledger_ids, sizes, version: int, map_offset: int, ledgers_count: int, state: int, why: str):
        self.ledger_ids = ledger_ids
        self.sizes = sizes
        self.version = version
        self.map_offset = map_offset
        self.ledgers_count = ledgers_count
        self.state = state
        self.why = why

    def totals(self) -> dict:
        """{ledger id: size}, the sizes of duplicate rows added up as EntryLogMetadata.addLedgerSize does."""
        out: dict[int, int] = {}
        for lid, size in zip(self.ledger_ids.tolist(), self.sizes.tolist()):
            out[lid] = out.get(lid, 0) + size
        return out


def read_ledgers_map(log) -> LedgersMap:
    """The log's ledgers map (``bkd_entrylog_ledgers_map``), read as
    DefaultEntryLogger.extractEntryLogMetadataFromIndex (:1089-1176) reads it. Host control logic."""
    buf = _ck._host_view(log)
    count = ctypes.c_uint64(0)
    version, ledgers_count, state = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    map_offset = ctypes.c_int64(0)
    cap = 64
    while True:
        lids = np.zeros(cap, dtype=np.int64)
        sizes = np.zeros(cap, dtype=np.int64)
        rc = lib().bkd_entrylog_ledgers_map(_ptr(buf), buf.size, _ptr(lids), _ptr(sizes), cap, ctypes.byref(count),
                                            ctypes.byref(version), ctypes.byref(map_offset),
                                            ctypes.byref(ledgers_count), ctypes.byref(state))
        if rc == BKD_ERR_BOUNDS and int(count.value) > cap:
            cap = int(count.value)
            continue
        check(rc)
        break
    why = last_error() if state.value == LEDGERS_MAP_MALFORMED else ""
    k = int(count.value)
    return LedgersMap(lids[:k].copy(), sizes[:k].copy(), int(version.value), int(map_offset.value),
                      int(ledgers_count.value), int(state.value), why)


class ScrubReport:
    """A scrub as it is read (``bkd_entrylog_scrub_report``): `scan`; `rows`, one REPORT_DTYPE record per row
    of `table` (rows[r] belongs to table.ids[r]); `other`, the catch-all row (unlisted ledgers, entries out of
    range or under 8 bytes); `nbad`, all bad entries; `bad`, the lowest indices of them, ascending; `status`,
    the n statuses when they were asked for."""

    def __init__(self, scan: ScanResult, table: LedgerTable, words: np.ndarray, nbad: int, bad: np.ndarray,
                 log_host=None, status=None):
        recs = np.ascontiguousarray(words, dtype=np.uint64).view(REPORT_DTYPE)
        self.scan = scan
        self.table = table
        self.rows = recs[:len(table)]
        self.other = recs[len(table)]
        self.nbad = int(nbad)
        self.bad = np.asarray(bad, dtype=np.uint32)
        self.status = status
        self._log = log_host

    def bad_entries(self) -> list:
        """(ledger id, entry id, offset, length) of every listed bad entry, from the scan and the host log;
        the entry id is None where the entry is shorter than 16 bytes."""
        buf = _ck._host_view(self._log)
        out = []
        for i in self.bad.tolist():
            o, n = int(self.scan.offsets[i]), int(self.scan.lengths[i])
            eid = int.from_bytes(bytes(buf[o + 8:o + 16]), "big", signed=True) if n >= 16 and o + n <= buf.size else None
            out.append((int(self.scan.ledger_ids[i]), eid, o, n))
        return out

    def damaged(self) -> dict:
        """{ledger id: (bad entries, lowest bad entry id, highest)} for the table's rows with bad entries."""
        return {int(self.table.ids[r]): (int(row["bad"]), int(row["min_bad_entry"]), int(row["max_bad_entry"]))
                for r, row in enumerate(self.rows) if row["bad"] > 0}

    def compare_ledgers_map(self, ledgers_map: LedgersMap):
        """The scan against the log's own map: (ledgers whose scanned bytes differ from the map's size as
        {ledger id: (scanned, map)}, ledgers in the map only, ledgers in the table only), the last two sorted.
        A ledger of the table that the log holds no entry of counts as absent from the scan."""
        totals = ledgers_map.totals()
        scanned = {int(self.table.ids[r]): int(row["bytes"]) for r, row in enumerate(self.rows) if row["entries"] > 0}
        differ = {l: (scanned[l], totals[l]) for l in scanned if l in totals and scanned[l] != totals[l]}
        return differ, sorted(set(totals) - set(scanned)), sorted(set(scanned) - set(totals))


class EntryLogScrubber:
    """Verifies the digests of all entries of one entry log on the GPU.

    ``digest_type_of(ledger_id)`` returns "CRC32C", "CRC32" or None (skip: DUMMY / HMAC ledgers,
    whose digests are not CRC arithmetic) — in BookKeeper it comes from the ledger metadata."""

    _ALGOS = {"CRC32C": CRC32C, "CRC32": CRC32}

    def __init__(self, digest_type_of=lambda ledger_id: "CRC32C"):
        self.digest_type_of = digest_type_of

    def verify(self, log_host, log_device=None, start: int = LOGFILE_HEADER_SIZE, stream=None):
        """Returns (scan, status int32[n] on the host; -1 = not checked). `log_device` is the same
        bytes resident in HBM (uploaded here when omitted)."""
        import torch
        scan = scan_entry_log(log_host, start)
        n = len(scan)
        status = np.full(n, -1, dtype=np.int32)
        if n == 0:
            return scan, status
        if log_device is None:
            log_device = torch.from_numpy(np.array(_ck._host_view(log_host), copy=True)).cuda()
        dev = log_device.device
        types = np.array([self._ALGOS.get(self.digest_type_of(int(l)), -1) for l in scan.ledger_ids],
                         dtype=np.int32)
        for algo in (CRC32C, CRC32):
            idx = np.nonzero(types == algo)[0]
            if idx.size == 0:
                continue
            d_off = torch.from_numpy(scan.offsets[idx].astype(np.int64)).to(dev)
            d_len = torch.from_numpy(scan.lengths[idx].astype(np.int32)).to(dev)
            d_status = torch.empty(idx.size, dtype=torch.int32, device=dev)
            d_first = torch.empty(1, dtype=torch.int64, device=dev)
            check(lib().bkd_entrylog_verify(
                algo, _ck._dev_ptr(log_device, "log"), log_device.numel() * log_device.element_size(),
                _ck._dev_ptr(d_off, "offsets", torch.int64), _ck._dev_ptr(d_len, "lengths", torch.int32),
                idx.size, _ck._dev_ptr(d_status, "status"), _ck._dev_ptr(d_first, "first_bad"),
                _ck._stream_ptr(stream, log_device)))
            status[idx] = d_status.cpu().numpy()
        return scan, status

    @staticmethod
    def verify_ledgers(log_host, table: LedgerTable, log_device=None, types=None, stream=None,
                       start: int = LOGFILE_HEADER_SIZE):
        """The whole log across ledgers and digest types in one device call
        (``bkd_entrylog_verify_ledgers``): CRC32C, CRC32, HMAC and DUMMY ledgers by `table`; `types` is a
        mask of ``1 << DIGEST_*`` (default: all four). Returns (scan, status int32[n] on the host;
        VERIFY_NOT_CHECKED for a ledger that is not listed or a type that is masked out). Raises
        BkdError(BKD_ERR_BOUNDS) when an entry was unreadable (over MAC_MAX_ENTRY, key row outside the
        table). `log_device` is the same bytes resident in HBM (uploaded here when omitted)."""
        import torch
        scan = scan_entry_log(log_host, start)
        n = len(scan)
        if n == 0:
            return scan, np.zeros(0, dtype=np.int32)
        if log_device is None:
            host = _ck._host_view(log_host)
            padded = np.zeros((host.size + 3) & ~3, dtype=np.uint8)  # whole dwords: the last entry's last load
            padded[:host.size] = host
            log_device = torch.from_numpy(padded).cuda()
            log_size = host.size
        else:
            log_size = log_device.numel() * log_device.element_size()
        dev = log_device.device
        mask = DIGEST_ALL if types is None else int(types)
        if types is None and not table.nkeys:
            mask &= ~(1 << DIGEST_HMAC)  # no HMAC ledger listed: the call needs no key table
        d_ids, d_types, d_keys, d_states = table.on(dev)
        d_off = torch.from_numpy(scan.offsets.astype(np.int64)).to(dev)
        d_len = torch.from_numpy(scan.lengths.astype(np.int32)).to(dev)
        d_status = torch.empty(n, dtype=torch.int32, device=dev)
        d_first = torch.empty(1, dtype=torch.int64, device=dev)
        sp = _ck._stream_ptr(stream, log_device)
        with torch.cuda.device(dev):
            check(lib().bkd_entrylog_verify_ledgers(
                _ck._dev_ptr(log_device, "log"), log_size, _ck._dev_ptr(d_off, "offsets", torch.int64),
                _ck._dev_ptr(d_len, "lengths", torch.int32), n, _ck._dev_ptr(d_ids, "ledger ids", torch.int64),
                _ck._dev_ptr(d_types, "ledger types", torch.int32), _ck._dev_ptr(d_keys, "ledger keys", torch.int32),
                len(table), _ck._dev_ptr(d_states, "key states", torch.int32) if table.nkeys else None, table.nkeys,
                mask, _ck._dev_ptr(d_status, "status"), _ck._dev_ptr(d_first, "first_bad"), sp))
            check(lib().bkd_stream_sync(sp))
        return scan, d_status.cpu().numpy()

    @staticmethod
    def verify_ledgers_host(log_host, table: LedgerTable, types=None, start: int = LOGFILE_HEADER_SIZE):
        """The same from host memory (``bkd_entrylog_verify_ledgers_host``): the GPU when the table lists an
        HMAC ledger and a device is visible, else the library's host threads (``bkd_set_host_batch_route``
        forces either). Returns (scan, status, first_bad)."""
        scan = scan_entry_log(log_host, start)
        n = len(scan)
        buf = _ck._host_view(log_host)
        status = np.zeros(n, dtype=np.int32)
        first_bad = ctypes.c_uint64(0)
        mask = DIGEST_ALL if types is None else int(types)
        if types is None and not table.nkeys:
            mask &= ~(1 << DIGEST_HMAC)  # no HMAC ledger listed: the call needs no key table
        check(lib().bkd_entrylog_verify_ledgers_host(
            _ptr(buf), buf.size, _ptr(scan.offsets), _ptr(scan.lengths), n, _ptr(table.ids), _ptr(table.types),
            _ptr(table.keys), len(table), _ptr(table.key_states), table.nkeys, mask, _ptr(status),
            ctypes.byref(first_bad)))
        return scan, status, int(first_bad.value)

    @staticmethod
    def report_ledgers(log_host, table: LedgerTable, log_device=None, types=None, stream=None,
                       start: int = LOGFILE_HEADER_SIZE, max_bad: int = DEFAULT_MAX_BAD, want_status: bool = False):
        """The scrub of ``verify_ledgers`` with what it is read for made on the device
        (``bkd_entrylog_scrub_report``): one row per ledger and the ascending list of bad entries (the lowest
        `max_bad` of them). Only the rows, the count and the list come back from the device; the n statuses
        stay there unless `want_status`. Returns a ``ScrubReport``; raises BkdError(BKD_ERR_BOUNDS) as
        ``verify_ledgers`` does."""
        import torch
        scan = scan_entry_log(log_host, start)
        n = len(scan)
        if log_device is None:
            host = _ck._host_view(log_host)
            padded = np.zeros(max(4, (host.size + 3) & ~3), dtype=np.uint8)  # whole dwords: the last entry's last load
            padded[:host.size] = host
            log_device = torch.from_numpy(padded).cuda()
            log_size = host.size
        else:
            log_size = log_device.numel() * log_device.element_size()
        dev = log_device.device
        mask = _default_mask(table, types)
        d_ids, d_types, d_keys, d_states = table.on(dev)
        d_off = torch.from_numpy(scan.offsets.astype(np.int64)).to(dev)
        d_len = torch.from_numpy(scan.lengths.astype(np.int32)).to(dev)
        cap = min(int(max_bad), n)
        d_status = torch.empty(n, dtype=torch.int32, device=dev) if want_status and n else None
        d_report = torch.empty((len(table) + 1) * REPORT_WORDS, dtype=torch.int64, device=dev)
        d_bad = torch.empty(cap, dtype=torch.int32, device=dev) if cap else None
        d_nbad = torch.empty(1, dtype=torch.int64, device=dev)

        def ptr(t, what, dtype=None):
            return _ck._dev_ptr(t, what, dtype) if t is not None and t.numel() else None

        sp = _ck._stream_ptr(stream, log_device)
        with torch.cuda.device(dev):
            check(lib().bkd_entrylog_scrub_report(
                _ck._dev_ptr(log_device, "log"), log_size, ptr(d_off, "offsets", torch.int64),
                ptr(d_len, "lengths", torch.int32), n, ptr(d_ids, "ledger ids", torch.int64),
                ptr(d_types, "ledger types", torch.int32), ptr(d_keys, "ledger keys", torch.int32), len(table),
                ptr(d_states, "key states", torch.int32) if table.nkeys else None, table.nkeys, mask,
                ptr(d_status, "status"), _ck._dev_ptr(d_report, "report", torch.int64), ptr(d_bad, "bad list"), cap,
                _ck._dev_ptr(d_nbad, "nbad", torch.int64), sp))
            check(lib().bkd_stream_sync(sp))
        nbad = int(d_nbad.cpu().numpy()[0])
        listed = min(nbad, cap)
        bad = d_bad[:listed].cpu().numpy().view(np.uint32) if listed else np.zeros(0, dtype=np.uint32)
        status = d_status.cpu().numpy() if d_status is not None else None
        return ScrubReport(scan, table, d_report.cpu().numpy().view(np.uint64), nbad, bad, log_host, status)

    @staticmethod
    def report_ledgers_host(log_host, table: LedgerTable, types=None, start: int = LOGFILE_HEADER_SIZE,
                            max_bad: int = DEFAULT_MAX_BAD, want_status: bool = False):
        """The same from host memory (``bkd_entrylog_scrub_report_host``), by the route ``verify_ledgers_host``
        takes. Returns a ``ScrubReport``."""
        scan = scan_entry_log(log_host, start)
        n = len(scan)
        buf = _ck._host_view(log_host)
        cap = min(int(max_bad), n)
        status = np.zeros(n, dtype=np.int32) if want_status else None
        report = np.zeros((len(table) + 1) * REPORT_WORDS, dtype=np.uint64)
        bad = np.zeros(cap, dtype=np.uint32)
        nbad = ctypes.c_uint64(0)
        check(lib().bkd_entrylog_scrub_report_host(
            _ptr(buf), buf.size, _ptr(scan.offsets), _ptr(scan.lengths), n, _ptr(table.ids), _ptr(table.types),
            _ptr(table.keys), len(table), _ptr(table.key_states), table.nkeys, _default_mask(table, types),
            _ptr(status) if status is not None else None, _ptr(report), _ptr(bad), cap, ctypes.byref(nbad)))
        return ScrubReport(scan, table, report, int(nbad.value), bad[:min(int(nbad.value), cap)], log_host, status)
