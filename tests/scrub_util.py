"""Shared by the mixed-ledger scrub suites (bkd_entrylog_verify_ledgers): logs that mix the four digest
types, the references (oracle.verify_entry for CRC, hmac for HMAC, the length rule for DUMMY) and thin
wrappers over the C-ABI that take explicit index arrays, so that entries the record walk would never find
(shorter than 8 bytes, out of range) can be handed to the call."""
from __future__ import annotations

import ctypes
import functools
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


def _upload(gpu, buf, offsets, lengths, table, stream, log_size, keys, d_buf, pad):
    """The device copies a device-form call takes: (d_buf, log_size, d_off, d_len, table tensors, stream pointer).
    The log is rounded up to a dword with `pad` bytes behind log_size."""
    import torch
    if d_buf is None:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        padded = np.full((buf.size + 3) & ~3, pad, dtype=np.uint8)
        padded[:buf.size] = buf
        d_buf = torch.from_numpy(padded).to(gpu)
        if log_size is None:
            log_size = buf.size
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(gpu)
    d_len = torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.uint32).view(np.int32)).to(gpu)
    d_ids, d_types, d_keys, d_states = table.on(gpu)
    if keys is not None:
        d_keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).to(gpu)
    sp = ctypes.c_void_p(int(stream.cuda_stream)) if stream is not None else \
        ctypes.c_void_p(int(torch.cuda.current_stream(gpu).cuda_stream))
    return d_buf, log_size, d_off, d_len, (d_ids, d_types, d_keys, d_states), sp


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def run_device(gpu, buf, offsets, lengths, table, types: int = ALL, stream=None, log_size=None, null_keys=False,
               keys=None, nkeys=None, d_buf=None, pad: int = 0):
    """bkd_entrylog_verify_ledgers on `gpu`, then bkd_stream_sync -> (sync rc, status, first_bad)."""
    import torch
    d_buf, log_size, d_off, d_len, (d_ids, d_types, d_keys, d_states), sp = _upload(
        gpu, buf, offsets, lengths, table, stream, log_size, keys, d_buf, pad)
    n = len(offsets)
    d_status = torch.full((max(n, 1),), 77, dtype=torch.int32, device=gpu)
    d_first = torch.full((1,), 0xDEAD, dtype=torch.int64, device=gpu)
    ptr = _dptr
    rc = lib().bkd_entrylog_verify_ledgers(
        ptr(d_buf), log_size, ptr(d_off), ptr(d_len), n, ptr(d_ids), ptr(d_types), None if null_keys else ptr(d_keys),
        len(table), None if null_keys else ptr(d_states), 0 if null_keys else (table.nkeys if nkeys is None else nkeys),
        types, ptr(d_status) if n else ctypes.c_void_p(d_status.data_ptr()), ctypes.c_void_p(d_first.data_ptr()), sp)
    assert rc == 0, rc
    sync = lib().bkd_stream_sync(sp)
    return sync, d_status.cpu().numpy()[:n], int(d_first.cpu().numpy()[0])


def run_lanes(gpu, buf, offsets, lengths, table, types: int = ALL, stream=None, log_size=None, keys=None, nkeys=None,
              d_buf=None):
    """bkd_entrylog_scrub_lanes on `gpu`, then bkd_stream_sync -> (sync rc, lanes uint32[n], nlanes)."""
    import torch
    d_buf, log_size, d_off, d_len, (d_ids, d_types, d_keys, d_states), sp = _upload(
        gpu, buf, offsets, lengths, table, stream, log_size, keys, d_buf, 0)
    n = len(offsets)
    d_lanes = torch.full((max(n, 1),), -1, dtype=torch.int32, device=gpu)
    d_nlanes = torch.full((1,), 0xDEAD, dtype=torch.int32, device=gpu)
    rc = lib().bkd_entrylog_scrub_lanes(
        _dptr(d_buf), log_size, _dptr(d_off), _dptr(d_len), n, _dptr(d_ids), _dptr(d_types), _dptr(d_keys), len(table),
        _dptr(d_states), table.nkeys if nkeys is None else nkeys, types, ctypes.c_void_p(d_lanes.data_ptr()),
        ctypes.c_void_p(d_nlanes.data_ptr()), sp)
    assert rc == 0, rc
    sync = lib().bkd_stream_sync(sp)
    return sync, d_lanes.cpu().numpy().view(np.uint32)[:n], int(d_nlanes.cpu().numpy().view(np.uint32)[0])


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


# ---- the edge logs: test_gpu_scrub_edges.py runs them on the device, test_scrub_edges_cpu.py on the CPU route ----
# Every helper returns (buf uint8, offsets uint64, lengths uint32, table, want int32) or a list of such logs.
# The cached ones are shared between tests: nobody writes into them.

def shortest(b: int) -> int:
    """The shortest frame of b SHA-1 compressions."""
    return max(52, 64 * (b - 1) + 12)


def longest(b: int) -> int:
    return 64 * b + 11


def ledger_of(buf, o: int) -> int:
    return int.from_bytes(bytes(buf[o:o + 8]), "big", signed=True)


def want_of_index(buf, offsets, lengths, specs, mask: int = ALL, log_size=None) -> np.ndarray:
    """want_status for an explicit index over `buf`: an entry that leaves the log or an HMAC frame over the cap
    is unreadable (1); the ledger is the entry's own first 8 bytes, looked up in specs (id -> spec, listed only)."""
    size = buf.size if log_size is None else log_size
    out = []
    for o, n in zip(offsets, lengths):
        o, n = int(o), int(n)
        if o + n > size:
            out.append(1)
            continue
        spec = specs.get(ledger_of(buf, o)) if n >= 8 else None
        if spec is not None and type_name(spec) == "HMAC" and (mask & TYPE_BIT["HMAC"]) and n > MAC_MAX_ENTRY:
            out.append(1)
            continue
        out.append(want_status(buf[o:o + n], spec, mask))
    return np.array(out, dtype=np.int32)


def hashed_entries(buf, offsets, lengths, table, types: int = ALL, log_size=None) -> np.ndarray:
    """The indices an HMAC lane hashes, ascending: the entry is in range, its ledger is listed, the row's type is
    HMAC and the HMAC bit is in the mask, its key row is < nkeys, and 52 <= length <= the cap."""
    size = buf.size if log_size is None else log_size
    rows = {int(v): r for r, v in enumerate(table.ids)}
    out = []
    for i, (o, n) in enumerate(zip(offsets, lengths)):
        o, n = int(o), int(n)
        if o + n > size or n < 52 or n > MAC_MAX_ENTRY or not (types & TYPE_BIT["HMAC"]):
            continue
        r = rows.get(ledger_of(buf, o))
        if r is not None and int(table.types[r]) == el.DIGEST_HMAC and int(table.keys[r]) < table.nkeys:
            out.append(i)
    return np.array(out, dtype=np.uint32)


def index_of(expect):
    return (np.array([e[2] for e in expect], dtype=np.uint64), np.array([e[3] for e in expect], dtype=np.uint32))


def lay_out(entries, aligns=None, filler: int = 0, tail: int = 7):
    """Entries laid out with one to four `filler` bytes before each, entry k at an offset = aligns[k] (mod 4),
    and `tail` filler bytes behind the last."""
    out = bytearray([filler] * 5)
    offs = []
    for k, e in enumerate(entries):
        out.append(filler)
        while aligns is not None and len(out) % 4 != aligns[k]:
            out.append(filler)
        offs.append(len(out))
        out += e
    out += bytes([filler] * tail)
    return (np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.array(offs, dtype=np.uint64),
            np.array([len(e) for e in entries], dtype=np.uint32))


def mixed_log(seed: int, n_entries: int, specs: dict, unlisted=(), corruptions: int = 0, mask: int = ALL,
              max_payload: int = 9000):
    """make_mixed_log over `specs` with `corruptions` entries that have one byte from 8 on flipped; ledgers in
    `unlisted` write but are not in the table."""
    rng = np.random.default_rng(seed)
    listed = {l: s for l, s in specs.items() if l not in unlisted}
    log, expect = make_mixed_log(rng, n_entries, specs, max_payload=max_payload)
    buf = np.frombuffer(log, dtype=np.uint8).copy()
    for k in rng.choice(len(expect), corruptions, replace=False):
        _, _, o, n = expect[k]
        buf[o + int(rng.integers(8, n))] ^= 0x5A
    offs, lens = index_of(expect)
    return buf, offs, lens, el.LedgerTable.from_ledgers(listed), want_of_index(buf, offs, lens, listed, mask)


@functools.lru_cache(maxsize=None)
def mixed_log5():
    """mixed_case() in the shape of the edge logs."""
    buf, expect, specs, table, want = mixed_case()
    offs, lens = index_of(expect)
    return buf, offs, lens, table, want


# B.1 / the existing bins test

@functools.lru_cache(maxsize=None)
def bins_log():
    """Frames at both ends of B = 1 .. 65 compressions; bins of 1, 63, 64 and 65 entries interleaved in arrival
    order (a bin that ends inside a wave, on its edge, one past it); a corrupt frame in every bin."""
    rng = np.random.default_rng(31)
    ledgers = {100 + k: ("HMAC", b"pw%d" % (k % 3)) for k in range(5)}
    table = el.LedgerTable.from_ledgers(ledgers)
    by_bin = {}
    for b in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        for n in (shortest(b), longest(b)):
            assert sha1_blocks(n) == b
            by_bin.setdefault(bin_of(n), []).append(n)
    assert sha1_blocks(shortest(2) - 1) == 1 and sha1_blocks(longest(2) + 1) == 3
    entries = []
    for k, (bn, lengths) in enumerate(sorted(by_bin.items())):
        count = (1, 63, 64, 65)[k % 4]
        bad = int(rng.integers(count))
        for j in range(count):
            n = lengths[j % len(lengths)]
            lid = 100 + int(rng.integers(5))
            e = bytearray(frame_for(ledgers[lid], lid, j, rng.integers(0, 256, n - 52, dtype=np.uint8).tobytes()))
            if j == bad:
                e[int(rng.integers(8, n))] ^= 0x10
            entries.append(bytes(e))
    order = rng.permutation(len(entries))
    entries = [entries[i] for i in order]
    buf, offs, lens = pack_entries(entries)
    want = np.array([want_status(e, ledgers[int.from_bytes(e[:8], "big")]) for e in entries], dtype=np.int32)
    return buf, offs, lens, table, want


@functools.lru_cache(maxsize=None)
def one_length_log(count: int = 600, length: int = 300):
    """`count` HMAC frames of one length: one bin over several blocks of the scatter."""
    rng = np.random.default_rng(37)
    specs = {5: ("HMAC", b"one"), 6: ("HMAC", b"length")}
    entries = [frame_for(specs[5 + i % 2], 5 + i % 2, i, rng.integers(0, 256, length - 52, dtype=np.uint8).tobytes())
               for i in range(count)]
    buf, offs, lens = pack_entries(entries)
    return buf, offs, lens, el.LedgerTable.from_ledgers(specs), want_of_index(buf, offs, lens, specs)


# B.2

SWEEP_SPECS = {3: "CRC32C", 1 << 40: "CRC32C", 7: "CRC32", -5: "CRC32", 11: ("HMAC", b"alpha"), 12: ("HMAC", b"beta"),
               0x7FFFFFFF00000001: ("HMAC", b"gamma"), 20: "DUMMY"}
SWEEP_RANGES = {"HMAC": (52, 183), "CRC32C": (36, 103), "CRC32": (40, 107), "DUMMY": (32, 40)}


@functools.lru_cache(maxsize=None)
def sweep_log(filler: int = 0, end_mod=None):
    """Every length of SWEEP_RANGES at every offset = 0, 1, 2, 3 (mod 4) for each type, `filler` bytes between
    the entries, ledgers interleaved. Cycling over the entries of a type: intact, last byte flipped, byte 8
    flipped. The entries and their order do not depend on `filler`. end_mod 1, 2, 3: one more HMAC frame that ends
    on the log's last byte, with the log's size = end_mod (mod 4); its last byte is flipped for end_mod 2."""
    rng = np.random.default_rng(52)
    items = []
    for name, (lo, hi) in SWEEP_RANGES.items():
        lids = [l for l, s in SWEEP_SPECS.items() if type_name(s) == name]
        k = 0
        for n in range(lo, hi + 1):
            for a in range(4):
                lid = lids[(k // 3) % len(lids)]
                pay = rng.integers(0, 256, n - THRESHOLD[name], dtype=np.uint8).tobytes()
                e = bytearray(frame_for(SWEEP_SPECS[lid], lid, k, pay))
                assert len(e) == n
                if k % 3 == 1:
                    e[-1] ^= 0x01
                elif k % 3 == 2:
                    e[8] ^= 0x80
                items.append((bytes(e), a))
                k += 1
    items = [items[i] for i in rng.permutation(len(items))]
    if end_mod is not None:
        # laid out last, one to four filler bytes behind its predecessor: pick the alignment, then the length
        base = {1: 76, 2: 116, 3: 140}[end_mod]  # 76: the header and payload end in the padding spill of block 1
        a = (end_mod - base) % 4
        e = bytearray(frame_for(SWEEP_SPECS[12], 12, 10 ** 6, rng.integers(0, 256, base - 52, dtype=np.uint8).tobytes()))
        if end_mod == 2:
            e[-1] ^= 0x40
        items.append((bytes(e), a))
    buf, offs, lens = lay_out([e for e, _ in items], [a for _, a in items], filler, tail=7 if end_mod is None else 0)
    if end_mod is not None:
        assert buf.size % 4 == end_mod and int(offs[-1]) + int(lens[-1]) == buf.size
    assert all(int(o) % 4 == a for o, (_, a) in zip(offs, items))
    want = want_of_index(buf, offs, lens, SWEEP_SPECS)
    for name in ("HMAC", "CRC32C", "CRC32"):  # every type with a digest has intact and failing frames
        mine = [type_name(SWEEP_SPECS[ledger_of(buf, int(o))]) == name for o in offs]
        assert set(want[mine].tolist()) == {0, 2}, name
    return buf, offs, lens, el.LedgerTable.from_ledgers(SWEEP_SPECS), want


# B.3

FB_N = 3 * 256 + 7
FB_POSITIONS = (0, 1, 63, 64, 255, 256, FB_N - 1)
FB_KINDS = ("hmac", "crc32c", "crc32", "dummy_short", "tiny")
FB_KIND_STATUS = {"hmac": 2, "crc32c": 2, "crc32": 2, "dummy_short": 1, "tiny": 1}
FB_SPECS = {3: "CRC32C", 7: "CRC32", 11: ("HMAC", b"alpha"), 12: ("HMAC", b"beta"), 20: "DUMMY"}


@functools.lru_cache(maxsize=None)
def _first_bad_base():
    rng = np.random.default_rng(61)
    lids = list(FB_SPECS)
    entries = []
    for i in range(FB_N):
        lid = lids[int(rng.integers(len(lids)))]
        plen = int(rng.integers(0, 300 - THRESHOLD[type_name(FB_SPECS[lid])] + 1))
        entries.append(frame_for(FB_SPECS[lid], lid, i, rng.integers(0, 256, plen, dtype=np.uint8).tobytes()))
    return entries, [want_status(e, FB_SPECS[int.from_bytes(e[:8], "big")]) for e in entries]


def _failing_entry(kind: str, i: int, rng) -> bytes:
    if kind == "tiny":  # under 8 bytes: no ledger id to read
        return rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8).tobytes()
    if kind == "dummy_short":
        return frame_for("DUMMY", 20, i, b"")[:int(rng.integers(8, 32))]
    lid = {"hmac": 12, "crc32c": 3, "crc32": 7}[kind]
    e = bytearray(frame_for(FB_SPECS[lid], lid, i, rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()))
    e[int(rng.integers(8, len(e)))] ^= 0x20
    return bytes(e)


def first_bad_log(p=None, kind=None):
    """FB_N good entries of at most 300 bytes over the four types. With p: entry p fails in the way `kind`
    names, entry p + 1 (where there is one) and entry 100 of the next block of 256 (where there is one) fail in
    the next two ways of FB_KINDS. The index of the first failure is p by construction."""
    entries, want = _first_bad_base()
    entries, want = list(entries), list(want)
    assert not any(want)
    if p is not None:
        rng = np.random.default_rng(1000 + 8 * p + FB_KINDS.index(kind))
        at = [p] + ([p + 1] if p + 1 < FB_N else []) + [q for q in ((p // 256 + 1) * 256 + 100,) if q < FB_N]
        for j, i in enumerate(at):
            k = FB_KINDS[(FB_KINDS.index(kind) + j) % len(FB_KINDS)]
            entries[i] = _failing_entry(k, i, rng)
            want[i] = want_status(entries[i], FB_SPECS.get(int.from_bytes(entries[i][:8], "big")) if len(entries[i]) >= 8 else None)
            assert want[i] == FB_KIND_STATUS[k], (i, k, want[i])
    buf, offs, lens = pack_entries(entries, gap=1)
    return buf, offs, lens, el.LedgerTable.from_ledgers(FB_SPECS), np.array(want, dtype=np.int32)


# B.4

def long_bins_log(cap=("good", "bad", "over")):
    """One HMAC ledger: frames of 2^e - 1, 2^e, 2^e + 1, 5 * 2^(e-2) and 3 * 2^(e-1) compressions for e = 7 .. 14
    (the fifth count is there to reach 30 bins: the first four give three bins per e), shortest and longest frame
    of the count alternating, every second frame with its last byte flipped. In the middle of the index, adjacent:
    a frame of exactly BKD_MAC_MAX_ENTRY ("good"), another with its last byte flipped ("bad"), and an entry of
    cap + 1 bytes ("over": unreadable). Payloads are cut from one random blob."""
    rng = np.random.default_rng(71)
    spec, lid = ("HMAC", b"long"), 41
    blob = rng.integers(0, 256, MAC_MAX_ENTRY, dtype=np.uint8).tobytes()
    entries = []
    for e in range(7, 15):
        for b in (2 ** e - 1, 2 ** e, 2 ** e + 1, 5 * 2 ** (e - 2), 3 * 2 ** (e - 1)):
            k = len(entries)
            n = shortest(b) if (k // 2) % 2 == 0 else longest(b)
            assert sha1_blocks(n) == b
            s = int(rng.integers(0, len(blob) - (n - 52) + 1))
            f = bytearray(frame_for(spec, lid, k, blob[s:s + n - 52]))
            if k % 2:
                f[-1] ^= 0x01
            entries.append(bytes(f))
    big = []
    for what in cap:
        if what == "over":
            big.append(lid.to_bytes(8, "big") + bytes(MAC_MAX_ENTRY + 1 - 8))
            continue
        s = {"good": 3, "bad": 40}[what]
        f = bytearray(frame_for(spec, lid, 10 ** 6 + s, blob[s:s + MAC_MAX_ENTRY - 52]))
        assert len(f) == MAC_MAX_ENTRY
        if what == "bad":
            f[-1] ^= 0x80
        big.append(bytes(f))
    entries[20:20] = big
    buf, offs, lens = pack_entries(entries)
    return buf, offs, lens, el.LedgerTable.from_ledgers({lid: spec}), want_of_index(buf, offs, lens, {lid: spec})


# B.5

@functools.lru_cache(maxsize=None)
def shape_steps():
    """One stream's calls in order: [(log, types, null key arguments, what bkd_stream_sync answers)]."""
    specs = {3: "CRC32C", 1 << 40: "CRC32C", 7: "CRC32", -5: "CRC32", 11: ("HMAC", b"alpha"), 12: ("HMAC", b"beta"),
             13: ("HMAC", b"alpha"), 20: "DUMMY", 99: "CRC32C"}
    big = mixed_log(81, 2000, specs, unlisted=(99,), corruptions=60, max_payload=4000)
    rng = np.random.default_rng(82)
    s5 = {11: ("HMAC", b"five"), 3: "CRC32C"}
    e5 = [frame_for(s5[11], 11, i, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for i, n in enumerate((0, 3, 700, 64))]
    e5[2] = e5[2][:99] + bytes([e5[2][99] ^ 2]) + e5[2][100:]
    e5.insert(1, frame_for("CRC32C", 3, 0, b"masked out"))
    b5, o5, l5 = pack_entries(e5, gap=3)
    hmac_only = TYPE_BIT["HMAC"]
    five = (b5, o5, l5, el.LedgerTable.from_ledgers(s5), want_of_index(b5, o5, l5, s5, hmac_only))
    crc_mask = TYPE_BIT["CRC32C"] | TYPE_BIT["CRC32"]
    crc = mixed_log(83, 700, {3: "CRC32C", 7: "CRC32", 11: ("HMAC", b"unseen"), 20: "DUMMY"}, corruptions=30,
                    mask=crc_mask, max_payload=3000)
    s3 = {3: "CRC32C", 11: ("HMAC", b"three")}
    b3, o3, l3 = pack_entries([frame_for("CRC32C", 3, 0, b"x" * 100), frame_for(s3[11], 11, 0, b"y" * 77)])
    o3 = np.array([o3[0], b3.size - 10, o3[1]], dtype=np.uint64)  # the second entry ends one byte past the log
    l3 = np.array([l3[0], 11, l3[1]], dtype=np.uint32)
    oob = (b3, o3, l3, el.LedgerTable.from_ledgers(s3), want_of_index(b3, o3, l3, s3))
    assert oob[4].tolist() == [0, 1, 0] and five[4].tolist() == [0, -1, 0, 2, 0]
    return [(big, ALL, False, 0), (five, hmac_only, False, 0), (crc, crc_mask, True, 0), (oob, ALL, False, BKD_ERR_BOUNDS),
            (big, ALL, False, 0)]


# B.6

@functools.lru_cache(maxsize=None)
def thread_log(k: int):
    """Thread k's log: ~400 entries, its own ledger ids and passwords."""
    specs = {10 * k + 3: "CRC32C", 10 * k + 4: "CRC32", 10 * k + 5: ("HMAC", b"thread %d a" % k),
             10 * k + 6: ("HMAC", b"thread %d b" % k), 10 * k + 7: "DUMMY", 10 * k + 8: "CRC32"}
    return mixed_log(90 + k, 390 + 7 * k, specs, unlisted=(10 * k + 8,), corruptions=25, max_payload=2000)


# B.7

@functools.lru_cache(maxsize=None)
def index_shapes():
    """Indexes the record walk never produces: [the mixed log's in descending offset order, the same with every
    tenth entry listed three times, frames that lie inside another frame's payload]."""
    buf, offs, lens, table, want = mixed_log5()
    down = np.argsort(-offs.astype(np.int64), kind="stable")
    thrice = np.array([i for k, i in enumerate(down) for _ in range(3 if k % 10 == 0 else 1)])
    out = [(buf, offs[down], lens[down], table, want[down]), (buf, offs[thrice], lens[thrice], table, want[thrice])]
    specs = {3: "CRC32C", 11: ("HMAC", b"outer"), 12: ("HMAC", b"inner")}
    rng = np.random.default_rng(97)
    parts, index = [], []  # index: (offset in the log, length)
    at = 0
    for eid, corrupt in enumerate((False, True)):
        a = bytearray(frame_for("CRC32C", 3, eid, rng.integers(0, 256, 333, dtype=np.uint8).tobytes()))
        b = frame_for(specs[12], 12, eid, rng.integers(0, 256, 1021, dtype=np.uint8).tobytes())
        pay = bytes(rng.integers(0, 256, 17, dtype=np.uint8)) + bytes(a) + bytes(rng.integers(0, 256, 6, dtype=np.uint8)) + b + b"tail"
        outer = bytearray(frame_for(specs[11], 11, eid, pay))
        o_a, o_b = 52 + 17, 52 + 17 + len(a) + 6
        assert outer[o_a:o_a + len(a)] == a and bytes(outer[o_b:o_b + len(b)]) == b
        if corrupt:  # a byte of the inner CRC32C frame: that frame and the outer one fail, the inner HMAC frame holds
            outer[o_a + 200] ^= 0x08
        index += [(at, len(outer)), (at + o_a, len(a)), (at + o_b, len(b))]
        parts.append(bytes(outer) + b"\xEE" * 3)
        at += len(outer) + 3
    nbuf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    noffs = np.array([o for o, _ in index], dtype=np.uint64)
    nlens = np.array([n for _, n in index], dtype=np.uint32)
    nwant = want_of_index(nbuf, noffs, nlens, specs)
    assert nwant.tolist() == [0, 0, 0, 2, 2, 0]
    out.append((nbuf, noffs, nlens, el.LedgerTable.from_ledgers(specs), nwant))
    return out
