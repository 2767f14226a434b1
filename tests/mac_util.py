"""Shared by the MAC (HMAC-SHA1) suites: the independent reference is Python's hmac / hashlib, which
compute what javax.crypto's HmacSHA1 and MessageDigest SHA-1 compute for MacDigestManager."""
import hashlib
import hmac
import struct

import numpy as np

PASSWD = b"testPasswd"
LEDGER = 0x0123456789ABCDEF
FIRST_ENTRY = 1000


def mac_key(passwd: bytes = PASSWD) -> bytes:
    return hashlib.sha1(b"mac" + passwd).digest()  # MacDigestManager.java:61


def mac_of(data: bytes, key: bytes | None = None) -> bytes:
    return hmac.new(mac_key() if key is None else key, data, "sha1").digest()


def mac_of_parts(parts, key: bytes | None = None) -> bytes:
    """mac_of(b"".join(parts)) without joining them: a 32-byte header in front of a 4 MiB payload."""
    h = hmac.new(mac_key() if key is None else key, digestmod="sha1")
    for part in parts:
        h.update(part)
    return h.digest()


def header(ledger: int, entry: int, lac: int, length: int) -> bytes:
    return struct.pack(">qqqq", ledger, entry, lac, length)


def frame(entry: int, payload: bytes, ledger: int = LEDGER, lac: int | None = None, key: bytes | None = None,
          length_field: int | None = None) -> bytes:
    """payload: bytes or a contiguous uint8 array (not copied before the frame is joined)."""
    hdr = header(ledger, entry, entry - 1 if lac is None else lac, len(payload) if length_field is None else length_field)
    return b"".join((hdr, mac_of_parts((hdr, payload), key), payload))


def payloads(lengths, seed: int = 5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


SWEEP = list(range(0, 201)) + list(range(4090, 4101))


# ---- SHA-1's compression function, to derive HMAC key states from hashlib-made keys ----
def _rol(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def sha1_compress(state, block: bytes):
    w = list(struct.unpack(">16I", block))
    for t in range(16, 80):
        w.append(_rol(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = state
    for t in range(80):
        if t < 20:
            f, k = (b & c) | (~b & d), 0x5A827999
        elif t < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif t < 60:
            f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (_rol(a, 5) + (f & 0xFFFFFFFF) + e + k + w[t]) & 0xFFFFFFFF, a, _rol(b, 30), c, d
    return [(s + v) & 0xFFFFFFFF for s, v in zip(state, (a, b, c, d, e))]


SHA1_INIT = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]


def key_state_of(key: bytes) -> np.ndarray:
    """The ten words bkd_mac_key_init / bkd_mac_key_state must produce for an HMAC key of <= 64 bytes."""
    block = key.ljust(64, b"\0")
    inner = sha1_compress(SHA1_INIT, bytes(x ^ 0x36 for x in block))
    outer = sha1_compress(SHA1_INIT, bytes(x ^ 0x5C for x in block))
    return np.array(inner + outer, dtype=np.uint32)


def failure_frames():
    """One frame of each kind DigestManager.verifyDigest tells apart (DigestManager.java:226-283), as
    frame i of a read that expects entry ids FIRST_ENTRY + i from LEDGER. Returns (frames, status,
    status when the entry-id check is skipped); precedence: too short, digest, ledger, entry."""
    rng = np.random.default_rng(11)
    frames, want, want_skip = [], [], []

    def add(f, st, st_skip=None):
        frames.append(bytes(f))
        want.append(st)
        want_skip.append(st if st_skip is None else st_skip)

    def good(extra=0, **kw):
        i = len(frames)
        return bytearray(frame(FIRST_ENTRY + i + extra, rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), **kw))

    def flipped(at):
        f = good()
        f[at] ^= 0x40
        return f

    add(good(), 0)
    add(b"", 1)
    add(good()[:51], 1)
    add(frame(FIRST_ENTRY + len(frames), b""), 0)  # exactly 52 bytes: an empty payload verifies
    add(flipped(20), 2)  # a header byte (the LAC)
    for word in range(5):  # every word of the stored MAC
        add(flipped(32 + 4 * word + word % 4), 2)
    add(flipped(52), 2)  # first payload byte
    add(flipped(-1), 2)  # last payload byte
    add(good(ledger=LEDGER + 1), 3)
    add(good(extra=7), 4, 0)
    # precedence
    f = good(ledger=LEDGER + 1)
    f[40] ^= 1
    add(f, 2)  # digest before ledger
    add(good(extra=3, ledger=LEDGER - 1), 3)  # ledger before entry
    add(good(extra=1, ledger=LEDGER + 1)[:51], 1)  # too short before everything
    add(good(), 0)
    return frames, np.array(want, dtype=np.int32), np.array(want_skip, dtype=np.int32)


def first_bad(status) -> int:
    bad = np.flatnonzero(np.asarray(status) != 0)
    return int(bad[0]) if bad.size else len(status)


def lay_out(entries, aligns, tail: int = 0):
    """The entries in one buffer in order, entry i starting at the next byte whose address is aligns[i]
    modulo 16 (None: back to back); the gaps and `tail` bytes behind the last entry hold 0xEE, which no
    result may depend on. Returns (uint8 array, offsets int64, lengths int32)."""
    parts, offs, at = [], [], 0
    for e, a in zip(entries, aligns):
        gap = 0 if a is None else (a - at) % 16
        parts.append(b"\xEE" * gap)
        at += gap
        offs.append(at)
        parts.append(e)
        at += len(e)
    parts.append(b"\xEE" * tail)
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return buf, np.array(offs, dtype=np.int64), np.array([len(e) for e in entries], dtype=np.int32)


def host_pointers(bufs):
    """What the C-ABI's host forms take for a list of host buffers: (the uint8 views, which own nothing and
    must outlive the call, their addresses uint64[n] with 0 for an empty one, their sizes uint32[n])."""
    views = [np.frombuffer(b, dtype=np.uint8) for b in bufs]
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    return views, ptrs, np.array([v.size for v in views], dtype=np.uint32)


# ---- host forms across staging segments ----
MIB = 1 << 20
SEGMENT = 64 * MIB  # the GPU route stages at most this many bytes per segment (bkdigest.h)


def prefix_bytes(lengths) -> np.ndarray:
    """prefix[i] = the bytes in front of entry i. An entry with prefix > k * SEGMENT cannot lie in the
    first k segments, whatever rule cuts them: that is all the segment tests assume about the cuts."""
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64))[:-1]))


def segment_batch():
    """4 551 payloads, 181.5 MiB: three repeats of 1 500 short entries, 15 of 4 MiB + 5 bytes, a 3-byte and
    an empty one. The repeats are views of the same 60.5 MiB, so their MACs are computed once."""
    part = [int(x) for x in np.random.default_rng(1).integers(0, 700, 1500)] + [4 * MIB + 5] * 15 + [3, 0]
    blob = np.random.default_rng(2).integers(0, 256, sum(part), dtype=np.uint8)
    ends = np.cumsum(part)
    views = [blob[int(e) - n:int(e)] for e, n in zip(ends, part)]
    lens = np.array(part * 3, dtype=np.int64)
    return dict(payloads=views * 3, lens=lens, prefix=prefix_bytes(lens), macs=[mac_of(v) for v in views] * 3)


def segment_package(seg, seed: int = 3):
    """Per-entry ids, LACs and length fields over the whole int64 range (ids and length fields >= 0, every
    seventh LAC -1) for segment_batch(), and the 52 bytes package must write for each."""
    n = len(seg["payloads"])
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 2**63, n, dtype=np.int64)
    lacs = rng.integers(0, 2**63, n, dtype=np.int64)
    lacs[::7] = -1
    lfs = rng.integers(0, 2**63, n, dtype=np.int64)
    heads = []
    for i, p in enumerate(seg["payloads"]):
        hdr = header(LEDGER, int(ids[i]), int(lacs[i]), int(lfs[i]))
        heads.append(hdr + mac_of_parts((hdr, p)))
    return dict(ids=ids, lacs=lacs, lfs=lfs, heads=heads)


def segment_verify(seg):
    """segment_batch() as frames with entry ids FIRST_ENTRY + i, and the verify calls over them: a list of
    (name, frames, first_entry_id, skip_entry_check, expected status). The failing frames are picked by the
    bytes in front of them alone: `late` past 2 * SEGMENT (a third segment or later), `mid` past SEGMENT."""
    good = [frame(FIRST_ENTRY + i, p) for i, p in enumerate(seg["payloads"])]
    n = len(good)
    flens = np.array([len(f) for f in good], dtype=np.int64)
    prefix = prefix_bytes(flens)
    late = np.flatnonzero(prefix > 2 * SEGMENT)
    big = [int(i) for i in late if flens[i] > 4 * MIB]
    small = [int(i) for i in late if flens[i] < 100]
    assert len(big) >= 8 and len(small) >= 2 and flens[small[-1]] == 52
    i_short, i_digest, i_ledger, i_entry = small[-1], big[2], small[0], big[7]
    i_mid = int(next(i for i in np.flatnonzero(prefix > SEGMENT) if flens[i] < 100 and prefix[i] < 2 * SEGMENT))
    i_early = 57

    def flipped(i, at):
        f = bytearray(good[i])
        f[at] ^= 0x10
        return bytes(f)

    late_bad = list(good)
    late_bad[i_short] = good[i_short][:51]  # the last frame: no other frame's prefix moves
    late_bad[i_digest] = flipped(i_digest, -1)
    late_bad[i_ledger] = frame(FIRST_ENTRY + i_ledger, seg["payloads"][i_ledger], ledger=LEDGER + 1)
    late_bad[i_entry] = frame(FIRST_ENTRY + i_entry + 9, seg["payloads"][i_entry])
    assert i_short == n - 1
    want_late = np.zeros(n, dtype=np.int32)
    want_late[[i_short, i_digest, i_ledger, i_entry]] = [1, 2, 3, 4]
    all_bad = list(late_bad)
    all_bad[i_mid] = flipped(i_mid, 40)
    all_bad[i_early] = flipped(i_early, 52)
    want_all = want_late.copy()
    want_all[[i_mid, i_early]] = 2
    want_skip = np.where(want_late == 4, 0, want_late).astype(np.int32)
    cases = [("all good", good, FIRST_ENTRY, False, np.zeros(n, dtype=np.int32)),
             ("late failures", late_bad, FIRST_ENTRY, False, want_late),
             ("late, mid and early failures", all_bad, FIRST_ENTRY, False, want_all),
             ("entry ids not checked", late_bad, FIRST_ENTRY + 12345, True, want_skip)]
    return dict(good=good, cases=cases, late=(i_short, i_digest, i_ledger, i_entry), mid=i_mid, early=i_early)


def wrong_rows(got, want) -> list:
    """Indices of the rows of a uint8 [n, w] array that differ from want[i] (w bytes each), first five."""
    want = np.frombuffer(b"".join(want), dtype=np.uint8).reshape(np.asarray(got).shape)
    return np.flatnonzero((np.asarray(got) != want).any(axis=1))[:5].tolist()


# The three segment checks, on whichever route of the host forms is selected: each compares with hmac and
# returns what the library gave, for the caller to compare routes with each other.
def check_segment_mac(ck, ks, seg):
    got = ck.mac_batch_host(ks, seg["payloads"])
    assert got.shape == (len(seg["payloads"]), 20)
    assert wrong_rows(got, seg["macs"]) == []
    return got


def check_segment_package(mgr, seg, pk, stride: int):
    got, macs = mgr.package_batch_host(pk["ids"], pk["lacs"], pk["lfs"], seg["payloads"], frame_stride=stride)
    assert got.shape == (len(seg["payloads"]), stride)
    assert wrong_rows(got[:, :52], pk["heads"]) == []
    assert not got[:, 52:].any()  # the wrapper's zeros
    assert (macs == got[:, 32:52]).all()
    return got


def check_segment_verify(mgr, case):
    name, frames, first, skip, want = case
    status, fb = mgr.verify_batch_host(frames, first, skip_entry_check=skip)
    bad = np.flatnonzero(status != want)
    assert bad.size == 0, (name, bad[:5].tolist(), status[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert fb == first_bad(want), name
    return status, fb


def count_batch():
    """2^20 + 300 entries that are pointers into 256 short buffers (payload lengths 0..255, and the same as
    good frames): short ones listed far more often than long ones, so that the first 2^20 entries are
    under SEGMENT bytes, as frames too, and only an entry-count rule can cut them. One more frame with a
    flipped payload byte is listed once, past entry 2^20."""
    n = (1 << 20) + 300
    rng = np.random.default_rng(32)
    idx = rng.integers(0, 6, n)
    wide = np.flatnonzero(rng.random(n) < 1 / 64)
    idx[wide] = rng.integers(0, 256, wide.size)
    assert np.unique(idx).size == 256
    ps = payloads(range(256), seed=31)
    frames = [frame(FIRST_ENTRY + j, p) for j, p in enumerate(ps)]
    bad = bytearray(frames[200])
    bad[52 + 77] ^= 1
    return dict(n=n, idx=idx, payloads=ps, macs=[mac_of(p) for p in ps], frames=frames + [bytes(bad)],
                bad_at=(1 << 20) + 123)


# ---- 64-bit header fields ----
WIDE_LEDGERS = [0, 1 << 32, (1 << 63) - 1]
WIDE_ENTRIES = [0, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 2]
WIDE_LACS = [-1, 0, 2**32, 2**63 - 1]
WIDE_LENGTH_FIELDS = [0, 2**32 - 1, 2**32, 2**63 - 1]
WIDE_FIRST = 2**32 - 3


def wide_ids():
    """28 rows in which every entry id, LAC and length field above stands at least once, for each of the
    three ledger ids: (ids, lacs, length fields, payloads, {ledger: the 52 bytes package writes per row})."""
    rows = range(28)
    ids = np.array([WIDE_ENTRIES[r % 7] for r in rows], dtype=np.int64)
    lacs = np.array([WIDE_LACS[r % 4] for r in rows], dtype=np.int64)
    lfs = np.array([WIDE_LENGTH_FIELDS[(r // 7) % 4] for r in rows], dtype=np.int64)
    assert set(ids.tolist()) == set(WIDE_ENTRIES) and set(lacs.tolist()) == set(WIDE_LACS)
    assert set(lfs.tolist()) == set(WIDE_LENGTH_FIELDS)
    ps = payloads([(37 * r) % 211 for r in rows], seed=33)
    heads = {led: [frame(int(ids[r]), ps[r], ledger=led, lac=int(lacs[r]), length_field=int(lfs[r]))[:52] for r in rows]
             for led in WIDE_LEDGERS}
    return dict(ids=ids, lacs=lacs, lfs=lfs, payloads=ps, heads=heads)


def wide_verify_cases(ledger: int):
    """Verify calls for a manager of `ledger` around entry id 2^32: (name, frames, first_entry_id, status)."""
    ps = payloads([0, 1, 60, 64, 100, 3, 300, 12], seed=34)
    good = [frame(WIDE_FIRST + i, p, ledger=ledger) for i, p in enumerate(ps)]
    high_entry = list(good)
    high_entry[5] = frame(WIDE_FIRST + 5 + 2**32, ps[5], ledger=ledger)
    high_ledger = list(good)
    high_ledger[2] = frame(WIDE_FIRST + 2, ps[2], ledger=ledger ^ (1 << 32))
    return [("ids in order across 2^32", good, WIDE_FIRST, [0] * 8),
            ("first entry id one lower", good, WIDE_FIRST - 1, [4] * 8),
            ("entry id off in its high word only", high_entry, WIDE_FIRST, [0, 0, 0, 0, 0, 4, 0, 0]),
            ("ledger id off in its high word only", high_ledger, WIDE_FIRST, [0, 0, 3, 0, 0, 0, 0, 0])]
