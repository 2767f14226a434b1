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
  memory.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import checksum as _ck
from ._native import CRC32, CRC32C, check, lib

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
