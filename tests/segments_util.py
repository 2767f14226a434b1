"""Shared by test_package_segments_cpu.py and test_gpu_package_segments.py: one deterministic batch of
composite entries over a 1 MiB splitmix64 buffer, and what the oracle gives for it.

Entry i is the concatenation of segments first[i] .. first[i+1]-1, segment k = data[offs[k] : + lens[k]].
The batch holds every shape the composite package calls can meet: entries of 0, 1, 1, 2, 3 and 33
segments, then 0..8; lengths at the power-of-two and byte boundaries of the join's power table and
random ones below 3000; about 15 % empty segments (first, in the middle and last; one entry of empty
segments only); a short and an empty segment at the very end of the buffer; unaligned starts; byte ranges shared by two entries; overlapping segments; header
fields at their 64-bit corners. Expected digests and frames come from oracle.digest_entry over the
concatenation, never from the code under test.
"""
import ctypes
import functools

import numpy as np

import oracle
from bookkeeper_amd import _native

SIZE = 1 << 20
N = 600
MAC = {oracle.CRC32C: 4, oracle.CRC32: 8}
SPECIAL = (0, 1, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537)
CORNER_LEDGERS = (-2**63, 2**63 - 1, 2**32, -1)
ONE_LEDGER = {oracle.CRC32C: -2**63, oracle.CRC32: 2**63 - 1}
FIRST_ENTRY_ID = 2**32 - 200  # first + i carries into the high word inside the batch
LENGTH_FIELD_BASE = 2**40     # a running ledger length: never derived from the segments
SENTINEL = 0xA5
vp = ctypes.c_void_p
# the lengths whose power x^(8 len) exercises every byte of the table index (one, two, three and four
# non-zero bytes, and the carries between them)
POWER_LENGTHS = (1, 255, 256, 257, 65535, 65536, 65537, 0xFFFFFF, 0x1000000, 0x1000001, 0x01010101)


class Batch:
    def __init__(self):
        rng = np.random.default_rng(20260)
        self.data = oracle.fill_splitmix64(SIZE, 77)
        n = self.n = N
        counts = rng.integers(0, 9, n)
        counts[:6] = [0, 1, 1, 2, 3, 33]
        counts[6] = 3   # empty segments only
        counts[7] = 5   # empty first, in the middle and last
        counts[8] = counts[9] = 4   # entry 9 shares entry 8's byte ranges
        counts[10] = 4  # overlapping segments
        self.first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=self.first[1:])
        nseg = self.nseg = int(self.first[-1])
        lens = rng.integers(1, 3000, nseg)
        pick = rng.random(nseg) < 0.25
        lens[pick] = rng.choice(SPECIAL, int(pick.sum()))
        lens[rng.random(nseg) < 0.15] = 0
        f = self.first
        lens[f[1]] = 1
        lens[f[2]] = 4097
        lens[f[6]:f[7]] = 0
        lens[f[7]:f[8]] = [0, 5, 0, 700, 0]
        lens[f[8]:f[9]] = [96, 0, 4000, 17]
        lens[f[10]:f[11]] = [300, 300, 65537, 64]
        offs = np.array([int(rng.integers(0, SIZE - l + 1)) for l in lens], dtype=np.int64)
        lens[f[9]:f[10]] = lens[f[8]:f[9]]
        offs[f[9]:f[10]] = offs[f[8]:f[9]]
        o = int(offs[f[10]])
        o = min(o, SIZE - 70000)
        offs[f[10]:f[11]] = [o, o + 150, o + 100, o + 301]  # each starts inside another
        lens[nseg - 1] = 33
        offs[nseg - 1] = SIZE - 33  # a segment that ends on the buffer's last byte
        # the end of the buffer, where a load of a whole 16-byte block would leave it: a 5-byte segment on
        # the last bytes and an empty one at offset == SIZE (an empty leaf at the writer index)
        offs[f[7] + 1] = SIZE - 5
        offs[f[8] - 1] = SIZE
        assert lens[f[7] + 1] == 5 and lens[f[8] - 1] == 0
        assert (offs % 4 != 0).sum() > nseg // 2 and (offs + lens <= SIZE).all()
        empty = lens == 0
        assert 0.08 < empty.mean() < 0.25
        self.lens, self.offs = lens.astype(np.int64), offs
        self.ids = FIRST_ENTRY_ID + np.arange(n, dtype=np.int64)
        assert self.ids[0] < 2**32 <= self.ids[-1]
        self.lacs = rng.integers(-1, 2**63, n, dtype=np.int64)
        self.lacs[n // 3], self.lacs[2 * n // 3] = -1, 2**63 - 1
        self.lenf = LENGTH_FIELD_BASE + np.cumsum(rng.integers(0, 5000, n, dtype=np.int64))
        self.ledgers = rng.integers(-2**63, 2**63, n, dtype=np.int64)
        self.ledgers[::3] = np.resize(np.array(CORNER_LEDGERS, dtype=np.int64), self.ledgers[::3].size)
        self.seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.cat = [b"".join(self.data[offs[k]:offs[k] + lens[k]].tobytes() for k in range(f[i], f[i + 1]))
                    for i in range(n)]
        assert self.cat[6] == b"" and self.cat[0] == b"" and self.cat[8] == self.cat[9]

    def segment_views(self, data=None):
        """Segment k as a view of `data` (the host forms take one buffer per segment)."""
        data = self.data if data is None else data
        return [data[o:o + l] for o, l in zip(self.offs.tolist(), self.lens.tolist())]

    def payloads(self):
        """Entry i as the list of its segments' views (package_batch_segments_host's payload form)."""
        v = self.segment_views()
        return [v[self.first[i]:self.first[i + 1]] for i in range(self.n)]

    def ledger_of(self, algo, per_entry):
        return self.ledgers if per_entry else np.full(self.n, ONE_LEDGER[algo], dtype=np.int64)

    @functools.lru_cache(maxsize=None)
    def expected(self, algo, per_entry):
        """(digests uint32[n], heads uint8[n, 32 + mac]) from oracle.digest_entry over each concatenation."""
        return expected_frames(algo, self.ledger_of(algo, per_entry), self.ids, self.lacs, self.lenf, self.cat)


def expected_frames(algo, ledgers, ids, lacs, lenf, payloads):
    n = len(payloads)
    digests = np.zeros(n, dtype=np.uint32)
    heads = np.zeros((n, 32 + MAC[algo]), dtype=np.uint8)
    for i in range(n):
        d, hdr = oracle.digest_entry(algo, int(ledgers[i]), int(ids[i]), int(lacs[i]), int(lenf[i]), payloads[i])
        digests[i] = d
        heads[i] = np.frombuffer(hdr + oracle.digest_bytes(algo, d), dtype=np.uint8)
    return digests, heads


@functools.lru_cache(maxsize=1)
def batch():
    return Batch()


def check_frames(frames, digests, want_digests, want_heads, stride, skip=()):
    """Every digest, every frame byte and, past 32 + mac, the sentinel the caller filled the frames with.
    skip: entries whose digest is unspecified (their 32 header bytes are still checked)."""
    n, hl = want_heads.shape
    frames = np.asarray(frames).reshape(-1)[:n * stride].reshape(n, stride)
    keep = np.ones(n, dtype=bool)
    keep[list(skip)] = False
    assert (np.asarray(digests).view(np.uint32)[keep] == want_digests[keep]).all()
    assert (frames[keep, :hl] == want_heads[keep]).all()
    assert (frames[:, :32] == want_heads[:, :32]).all()
    assert (frames[:, hl:] == SENTINEL).all()


def package_host_raw(algo, ledger_id, ledger_ids, ids, lacs, lenf, views, first, stride, n=None, nseg=None):
    """bkd_digest_package_batch_segments_host through ctypes, the frames prefilled with the sentinel:
    (rc, frames uint8[n * stride], digests uint32[n])."""
    n = len(first) - 1 if n is None else n
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    lens = np.array([v.size for v in views], dtype=np.uint32)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    frames = np.full(max(n, 1) * stride, SENTINEL, dtype=np.uint8)
    digests = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32)
    ids, lacs, lenf = (np.ascontiguousarray(a, dtype=np.int64) for a in (ids, lacs, lenf))
    lids = None if ledger_ids is None else np.ascontiguousarray(ledger_ids, dtype=np.int64)
    rc = _native.lib().bkd_digest_package_batch_segments_host(
        algo, ledger_id, vp(0 if lids is None else lids.ctypes.data), vp(ids.ctypes.data), vp(lacs.ctypes.data),
        vp(lenf.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), len(views) if nseg is None else nseg,
        vp(first.ctypes.data), n, vp(frames.ctypes.data), stride, vp(digests.ctypes.data))
    return rc, frames, digests


# ---- malformed inputs of the device call, shared so that the CPU suite drives the clamp with exactly
# the arrays the GPU tests pass ----

def malformed_firsts(first, nseg):
    """Variants of a valid seg_first that break the CSR: {name: int64 array}."""
    n = first.size - 1
    out = {}
    a = first.copy(); a[0] = 1; out["first_not_zero"] = a
    a = first.copy(); a[n // 2] = a[n // 2 + 1] + 3; out["decrease"] = a
    a = first.copy(); a[n // 3] = nseg + 1000; out["past_nseg"] = a
    a = first.copy(); a[n] = nseg - 1; out["last_short"] = a
    a = first.copy(); a[1:] = np.iinfo(np.int64).max; out["huge"] = a
    a = first.copy(); a[n // 4] = -1; out["negative"] = a  # 2^64 - 1 as the library reads it
    return out


def out_of_range_segments(b):
    """(offs, lens, entries) of the batch with three out-of-range segments: in the first entry that has
    a segment, a middle and the last entry. One starts past the buffer, one ends a byte past it, one
    wraps offset + length past 2^64."""
    offs, lens = b.offs.copy(), b.lens.copy()
    has = np.nonzero(np.diff(b.first) > 0)[0]
    ents = [int(has[0]), int(has[has.size // 2]), int(has[-1])]
    k = [int(b.first[e]) for e in ents]
    offs[k[0]], lens[k[0]] = SIZE + 5, 10
    offs[k[1]], lens[k[1]] = SIZE - 99, 100
    offs[k[2]], lens[k[2]] = -64, 4096  # 2^64 - 64
    return offs, lens, ents
