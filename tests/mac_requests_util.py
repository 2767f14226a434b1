"""Shared by the suites of the MAC calls that span ledgers (verify_requests_mac, package_batch_ledgers_mac
and their host forms): read requests with a ledger, a first entry id and a key of their own, and what
Python's hmac says about them."""
import hmac
import struct

import numpy as np

import mac_util as mu


def password(k: int) -> bytes:
    return b"passwd-%d" % k


def key(k: int) -> bytes:
    """The HMAC key of key row k: SHA1("mac" || password(k))."""
    return mu.mac_key(password(k))


def ledger(r: int) -> int:
    return 0x0102030400000000 + 7 * r + 1  # distinct per request, both words in use


def first_entry(r: int) -> int:
    return 1000 * r + 5


def ref_status(f, key_bytes: bytes, ledger_id: int, entry_id: int, skip: bool) -> int:
    """DigestManager.verifyDigest's verdict on one MAC frame (DigestManager.java:226-283) from hmac alone."""
    f = bytes(f)
    if len(f) < 52:
        return 1
    if hmac.new(key_bytes, f[:32] + f[52:], "sha1").digest() != f[32:52]:
        return 2
    lid, eid = struct.unpack(">qq", f[:16])
    if lid != ledger_id:
        return 3
    return 4 if (not skip and eid != entry_id) else 0


class Requests:
    """Read requests of sizes[r] entries each. Request r reads ledger(r) from first_entry(r) and is keyed
    with row keys[r] (default r: a key of its own) of a table of password(0..nkeys); its frames are good
    frames with payloads of the given lengths. Tests then overwrite frames, lids, firsts, req_keys or
    flags and ask expected() what the reference makes of the result."""

    def __init__(self, sizes, lengths=None, seed: int = 0, keys=None, nkeys=None):
        self.sizes = [int(s) for s in sizes]
        self.nreq = len(self.sizes)
        self.n = sum(self.sizes)
        self.first = np.concatenate(([0], np.cumsum(self.sizes))).astype(np.int64)
        self.req_keys = np.array(list(range(self.nreq)) if keys is None else keys, dtype=np.int32)
        self.nkeys = (int(self.req_keys.max()) + 1 if self.nreq else 0) if nkeys is None else nkeys
        self.lids = np.array([ledger(r) for r in range(self.nreq)], dtype=np.int64)
        self.firsts = np.array([first_entry(r) for r in range(self.nreq)], dtype=np.int64)
        self.flags = np.zeros(self.nreq, dtype=np.int32)
        rng = np.random.default_rng(seed)
        if lengths is None:
            lengths = rng.integers(0, 349, self.n)
        self.payloads = mu.payloads(lengths, seed=seed + 1)
        self.frames = []
        for r in range(self.nreq):
            for j in range(self.sizes[r]):
                i = int(self.first[r]) + j
                self.frames.append(mu.frame(first_entry(r) + j, self.payloads[i], ledger=ledger(r),
                                            key=key(int(self.req_keys[r]))))

    def req_of(self, i: int) -> int:
        return int(np.searchsorted(self.first, i, side="right")) - 1

    def passwords(self):
        return [password(k) for k in range(self.nkeys)]

    def expected(self, frames=None):
        """(status int32[n], prefix int64[nreq]) by the reference, for the arrays as they stand now."""
        frames = self.frames if frames is None else frames
        status = np.zeros(self.n, dtype=np.int32)
        prefix = np.array(self.sizes, dtype=np.int64)
        for r in range(self.nreq):
            for j in range(self.sizes[r]):
                i = int(self.first[r]) + j
                k = int(self.req_keys[r])
                status[i] = 1 if not 0 <= k < self.nkeys else ref_status(
                    frames[i], key(k), int(self.lids[r]), int(self.firsts[r]) + j, bool(self.flags[r] & 1))
            bad = np.flatnonzero(status[int(self.first[r]):int(self.first[r + 1])])
            if bad.size:
                prefix[r] = int(bad[0])
        return status, prefix


# The CSR shapes every suite runs: name -> request sizes.
CSR_SHAPES = {
    "one request holds everything": [41],
    "one entry per request": [1] * 41,
    "empty requests first, in the middle and last": [0, 0, 5, 0, 0, 0, 9, 1, 0],
    "nreq == 1, one entry": [1],
    "n == 0, three empty requests": [0, 0, 0],
    "n == 0, nreq == 1": [0],
}


def package_fields(n: int, nkeys: int, seed: int = 7):
    """Per-entry ledger ids, key rows and header fields over the whole int64 range, mu.wide_ids()-style:
    dict(lids, key_of, ids, lacs, lfs)."""
    rng = np.random.default_rng(seed)
    lids = np.array([mu.WIDE_LEDGERS[i % 3] ^ (i // 3) for i in range(n)], dtype=np.int64)
    ids = np.array([mu.WIDE_ENTRIES[i % 7] for i in range(n)], dtype=np.int64)
    lacs = np.array([mu.WIDE_LACS[i % 4] for i in range(n)], dtype=np.int64)
    lfs = np.array([mu.WIDE_LENGTH_FIELDS[(i // 7) % 4] for i in range(n)], dtype=np.int64)
    return dict(lids=lids, key_of=rng.integers(0, nkeys, n).astype(np.int32), ids=ids, lacs=lacs, lfs=lfs)


def package_heads(f, payloads):
    """The 52 bytes package must write for each entry of package_fields()."""
    return [mu.frame(int(f["ids"][i]), p, ledger=int(f["lids"][i]), lac=int(f["lacs"][i]), key=key(int(f["key_of"][i])),
                     length_field=int(f["lfs"][i]))[:52] for i, p in enumerate(payloads)]
