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


def header(ledger: int, entry: int, lac: int, length: int) -> bytes:
    return struct.pack(">qqqq", ledger, entry, lac, length)


def frame(entry: int, payload: bytes, ledger: int = LEDGER, lac: int | None = None, key: bytes | None = None) -> bytes:
    hdr = header(ledger, entry, entry - 1 if lac is None else lac, len(payload))
    return hdr + mac_of(hdr + payload, key) + payload


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
