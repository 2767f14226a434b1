"""Shared by the mixed-ledger scrub suites (bkd_entrylog_verify_ledgers): logs that mix the four digest
types, the references (oracle.verify_entry for CRC, hmac for HMAC, the length rule for DUMMY) and thin
wrappers over the C-ABI that take explicit index arrays, so that entries the record walk would never find
(shorter than 8 bytes, out of range) can be handed to the call."""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import oracle
from bookkeeper_amd import entrylog as el
from bookkeeper_amd._native import lib
from entrylog_util import HEADER, framed_entry
from mac_util import mac_key, mac_of_parts

BKD_ERR_INVALID_ARG, BKD_ERR_NO_DEVICE, BKD_ERR_BOUNDS = -1, -2, -4
MAC_MAX_ENTRY = 16 << 20
ALL = el.DIGEST_ALL
TYPE_BIT = {"CRC32C": 1, "CRC32": 2, "HMAC": 4, "DUMMY": 8}
THRESHOLD = {"CRC32C": 36, "CRC32": 40, "HMAC": 52, "DUMMY": 32}


def type_name(spec) -> str:
    return spec if isinstance(spec, str) else spec[0]


def frame_for(spec, ledger_id: int, entry_id: int, payload: bytes) -> bytes:
    """An entry of a ledger of digest type `spec` ("CRC32C" | "CRC32" | "DUMMY" | ("HMAC", passwd))."""
    name = type_name(spec)
    if name == "CRC32C":
        return framed_entry(oracle.CRC32C, ledger_id, entry_id, payload)
    if name == "CRC32":
        return framed_entry(oracle.CRC32, ledger_id, entry_id, payload)
    hdr = struct.pack(">qqqq", ledger_id, entry_id, entry_id - 1, len(payload))
    if name == "DUMMY":  # no digest bytes at all (DummyDigestManager.java:35-43)
        return hdr + payload
    return hdr + mac_of_parts((hdr, payload), mac_key(spec[1])) + payload


def make_mixed_log(rng, n_entries: int, ledgers: dict, max_payload: int = 9000, min_payload: int = 0):
    """Records like entrylog_util.make_entry_log, for all four digest types. ledgers: ledger id -> spec, for
    every ledger that writes (listed in the table or not). Returns (log bytes, [(ledger, entry id, entry
    offset, entry length)])."""
    out = bytearray(HEADER)
    out[0:4] = b"BKLO"
    out[4:8] = (1).to_bytes(4, "big")
    lids = list(ledgers)
    next_eid = {l: 0 for l in lids}
    expect = []
    for _ in range(n_entries):
        lid = lids[int(rng.integers(len(lids)))]
        eid = next_eid[lid]
        next_eid[lid] += 1
        plen = int(rng.integers(min_payload, max_payload + 1))
        f = frame_for(ledgers[lid], lid, eid, rng.integers(0, 256, plen, dtype=np.uint8).tobytes())
        out += len(f).to_bytes(4, "big")
        expect.append((lid, eid, len(out), len(f)))
        out += f
    out += bytes(int(rng.integers(0, 40)))  # preallocated zero tail
    return bytes(out), expect


def pack_entries(entries, gap: int = 0):
    """Raw entries laid end to end (`gap` bytes between them): (buffer uint8, offsets uint64, lengths uint32)."""
    offs, lens, parts, at = [], [], [], 0
    for e in entries:
        offs.append(at)
        lens.append(len(e))
        parts.append(bytes(e) + bytes(gap))
        at += len(e) + gap
    buf = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8).copy()
    return buf, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def want_status(entry: bytes, spec, mask: int = ALL) -> int:
    """What the call must give a readable entry whose ledger has digest type `spec` (None: not listed)."""
    entry = bytes(entry)
    if len(entry) < 8:
        return 1
    if spec is None or not (mask & TYPE_BIT[type_name(spec)]):
        return -1
    name = type_name(spec)
    if name == "DUMMY":
        return 0 if len(entry) >= 32 else 1
    if name == "HMAC":
        if len(entry) < 52:
            return 1
        return 0 if mac_of_parts((entry[:32], entry[52:]), mac_key(spec[1])) == entry[32:52] else 2
    lid = int.from_bytes(entry[:8], "big", signed=True)  # the ledger id is the entry's own: no id check
    return oracle.verify_entry(oracle.CRC32C if name == "CRC32C" else oracle.CRC32, entry, lid, 0, skip_entry_check=True)


def want_first_bad(status) -> int:
    bad = np.nonzero(np.asarray(status) > 0)[0]
    return int(bad[0]) if bad.size else len(status)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def run_host(buf, offsets, lengths, table, types: int = ALL, ids=None, ltypes=None, keys=None, nkeys=None,
             status_fill: int = 77):
    """bkd_entrylog_verify_ledgers_host -> (rc, status, first_bad); ids / ltypes / keys / nkeys override the table's."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    ids = table.ids if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
    ltypes = table.types if ltypes is None else np.ascontiguousarray(ltypes, dtype=np.uint32)
    keys = table.keys if keys is None else np.ascontiguousarray(keys, dtype=np.uint32)
    states = table.key_states
    n = offsets.size
    status = np.full(n, status_fill, dtype=np.int32)
    first_bad = ctypes.c_uint64(0xDEAD)
    rc = lib().bkd_entrylog_verify_ledgers_host(
        _p(buf), buf.size, _p(offsets), _p(lengths), n, _p(ids), _p(ltypes), _p(keys), ids.size, _p(states),
        table.nkeys if nkeys is None else nkeys, types, _p(status), ctypes.byref(first_bad))
    return rc, status, int(first_bad.value)


def run_device(gpu, buf, offsets, lengths, table, types: int = ALL, stream=None, log_size=None, null_keys=False,
               keys=None, nkeys=None, d_buf=None):
    """bkd_entrylog_verify_ledgers on `gpu`, then bkd_stream_sync -> (sync rc, status, first_bad)."""
    import torch
    if d_buf is None:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        padded = np.zeros((buf.size + 3) & ~3, dtype=np.uint8)
        padded[:buf.size] = buf
        d_buf = torch.from_numpy(padded).to(gpu)
        if log_size is None:
            log_size = buf.size
    n = len(offsets)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(gpu)
    d_len = torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.uint32).view(np.int32)).to(gpu)
    d_ids, d_types, d_keys, d_states = table.on(gpu)
    if keys is not None:
        d_keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).to(gpu)
    d_status = torch.full((max(n, 1),), 77, dtype=torch.int32, device=gpu)
    d_first = torch.full((1,), 0xDEAD, dtype=torch.int64, device=gpu)
    sp = ctypes.c_void_p(int(stream.cuda_stream)) if stream is not None else \
        ctypes.c_void_p(int(torch.cuda.current_stream(gpu).cuda_stream))

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t.numel() else None

    rc = lib().bkd_entrylog_verify_ledgers(
        ptr(d_buf), log_size, ptr(d_off), ptr(d_len), n, ptr(d_ids), ptr(d_types), None if null_keys else ptr(d_keys),
        len(table), None if null_keys else ptr(d_states), 0 if null_keys else (table.nkeys if nkeys is None else nkeys),
        types, ptr(d_status) if n else ctypes.c_void_p(d_status.data_ptr()), ctypes.c_void_p(d_first.data_ptr()), sp)
    assert rc == 0, rc
    sync = lib().bkd_stream_sync(sp)
    return sync, d_status.cpu().numpy()[:n], int(d_first.cpu().numpy()[0])


def mixed_case(seed: int = 21, n_entries: int = 600, corruptions: int = 40):
    """GPU case 1 and the host suites' shared log: ten ledgers (two CRC32C, two CRC32, three HMAC with three
    passwords, a fourth HMAC sharing a row, one DUMMY, one unlisted), payloads 0-9000 B, `corruptions`
    flipped bytes (payload, digest, header outside the ledger id). Returns (buf, expect, specs, table, want)."""
    rng = np.random.default_rng(seed)
    specs = {3: "CRC32C", 1 << 40: "CRC32C", 7: "CRC32", -5: "CRC32", 11: ("HMAC", b"alpha"), 12: ("HMAC", b"beta"),
             0x7FFFFFFF00000001: ("HMAC", b"gamma"), 13: ("HMAC", b"alpha"), 20: "DUMMY", 99: "CRC32C"}
    listed = {l: s for l, s in specs.items() if l != 99}
    log, expect = make_mixed_log(rng, n_entries, specs)
    buf = np.frombuffer(log, dtype=np.uint8).copy()
    picks = rng.choice(len(expect), corruptions, replace=False)
    for k, what in zip(picks, ["p", "d", "h"] * (corruptions // 3 + 1)):
        lid, eid, o, n = expect[k]
        pos = o + {"p": min(n - 1, 60 + int(rng.integers(0, max(1, n - 60)))), "d": 33, "h": 8 + int(rng.integers(0, 24))}[what]
        if pos < o + n:
            buf[pos] ^= 0x5A
    table = el.LedgerTable.from_ledgers(listed)
    want = np.array([want_status(buf[o:o + n], listed.get(lid)) for lid, eid, o, n in expect], dtype=np.int32)
    return buf, expect, specs, table, want


def short_entries():
    """Lengths 0-60 for each type; entries under 8 bytes hold garbage (no ledger id to read). Returns
    (entries, want, table)."""
    specs = {1: "CRC32C", 2: "CRC32", 3: ("HMAC", b"pw"), 4: "DUMMY"}
    rng = np.random.default_rng(8)
    entries, want = [], []
    for lid, spec in specs.items():
        least = THRESHOLD[type_name(spec)]
        for n in range(0, 61):
            if n < 8:
                e = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            elif n >= least:
                e = frame_for(spec, lid, n, rng.integers(0, 256, n - least, dtype=np.uint8).tobytes())
            else:
                e = frame_for(spec, lid, n, rng.integers(0, 256, 40, dtype=np.uint8).tobytes())[:n]
            assert len(e) == n
            entries.append(e)
            want.append(want_status(e, spec))
            if n >= 8:  # the thresholds are 32 / 36 / 40 / 52
                assert want[-1] == (0 if n >= least else 1), (spec, n)
    return entries, np.array(want, dtype=np.int32), el.LedgerTable.from_ledgers(specs)


def lookup_tables():
    """The table-search cases: (ids ascending int64, probes) for tables of 1, 2, 3, 1 000 and 1 025 rows with
    INT64_MIN, -1, 0, INT64_MAX and pairs that differ in the high word only; probes are every present id and
    ids in every gap below, between and above."""
    lo, hi = -(1 << 63), (1 << 63) - 1
    rng = np.random.default_rng(4)
    tables = [[0], [hi], [lo], [-1, 0], [lo, hi], [5, 5 + (1 << 32)], [-1, 0, 1], [lo, 0, hi], [7, 7 + (1 << 32), 7 + (2 << 32)]]
    for rows in (1000, 1025):
        ids = set(int(x) for x in rng.integers(lo, hi, rows - 8, dtype=np.int64))
        ids |= {lo, -1, 0, hi, 1 << 32, (1 << 32) + (1 << 33), 9, 9 + (1 << 32)}
        while len(ids) < rows:
            ids.add(int(rng.integers(lo, hi, dtype=np.int64)))
        tables.append(sorted(ids))
    out = []
    for t in tables:
        ids = np.array(t, dtype=np.int64)
        probes = set(t)
        for a, b in zip([None] + t, t + [None]):
            if a is None and b > lo:
                probes |= {lo, b - 1}
            elif b is None and a < hi:
                probes |= {hi, a + 1}
            elif a is not None and b is not None and b - a > 1:
                probes |= {a + 1, b - 1, a + (b - a) // 2}
        out.append((ids, sorted(probes)))
    return out


def lane_occupancy(blocks, order) -> float:
    """The lane model: compressions a wave's 64 lanes do over 64 x the longest lane, lanes taken in `order`."""
    b = np.asarray(blocks, dtype=np.int64)[np.asarray(order)]
    pad = (-b.size) % 64
    waves = np.concatenate([b, np.zeros(pad, dtype=np.int64)]).reshape(-1, 64)
    return float(b.sum()) / float(64 * waves.max(axis=1).sum())


def sha1_blocks(frame_len: int) -> int:
    return ((frame_len - 20) + 9 + 63) // 64


def bin_of(frame_len: int) -> int:
    """The bin rule, restated: 4 e + the two bits below the leading bit e of the block count."""
    b = sha1_blocks(frame_len)
    e = b.bit_length() - 1
    two = (b >> (e - 2)) & 3 if e >= 2 else (b << (2 - e)) & 3
    return 4 * e + two
