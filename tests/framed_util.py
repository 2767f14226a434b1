"""Shared by test_framed_cases_cpu.py and test_gpu_framed_sweep.py: the framed length sweep.

One deterministic batch per (lane width G, algorithm, placement shift): every payload length at which
the one-entry-per-group fold (fold_range, crc_kernels.hpp) takes another path at that width, each
entry placed so that all 16 start residues meet every step count, with header fields that use their
64 bits. Headers, digests and expected statuses come from the oracle (oracle.batch for the header CRC
and the payload resumed from it: DigestManager.java:146-153; oracle.verify_entry frame by frame),
never from the code under test. Nothing here loops per entry in Python except where the oracle or
the host API takes one entry per call (verify_entry, the host routes' buffer lists).
"""
import functools

import numpy as np

import oracle

PF = 2  # loads in flight per lane: the committed default (BKD_PF, bkdigest.hip)
EDGE = 16 + 4 - 1  # a 16-byte lane block plus the 4-byte seed image, on both sides of a step boundary
LANES = (4, 8, 16, 32, 64)
SHIFTS = (0, 7, 13)
MAC = {oracle.CRC32C: 4, oracle.CRC32: 8}
LEDGER = {4: 61, 8: -2**63, 16: 2**63 - 1, 32: 2**32, 64: -1}
FIRST_ENTRY_ID = 2**32 - 200  # first + i carries into the high word inside every batch
LENGTH_FIELD_BASE = 2**40  # a running ledger length: never the payload's own length
KINDS = ("payload_first", "payload_last", "digest", "lac", "high", "ledger", "entry", "ledger_entry",
         "digest_ledger")


def lengths_for(G):
    """Ascending payload lengths for lane width G. With S = 16 G bytes per step, J = ceil(l / S) steps:
    * 0 .. (PF + 1) S + EDGE: the serial class (l < 16), J = 1, J = 2 .. PF (J - 1 < PF: the loop
      without the A/B buffer, where a late seed is applied in the else arm), J = PF + 1 (the A/B
      buffer with nothing left) and the first lengths of J = PF + 2;
    * m S - EDGE .. m S + EDGE for m = 2 PF .. 6 PF - 1: J = m and m + 1, so J up to 6 PF: the
      steady loop (2 PF steps a turn after the first PF) taken zero, one and two times, with tails of
      0 .. 2 PF - 1 steps after zero and one turn and of 0 .. 1 after two.
    EDGE puts a lane-block boundary and the seed's spill on both sides of every step boundary."""
    S = 16 * G
    parts = [np.arange(0, (PF + 1) * S + EDGE + 1)]
    for m in range(2 * PF, 6 * PF):
        parts.append(np.arange(m * S - EDGE, m * S + EDGE + 1))
    out = np.concatenate(parts).astype(np.int64)
    assert (np.diff(out) > 0).all()
    return out


def headers(ledger, ids, lacs, lenf):
    """The 32-byte BE headers [ledgerId, entryId, lastAddConfirmed, length] (DigestManager.java:146-149)."""
    n = len(ids)
    h = np.empty((n, 4), dtype=">i8")
    h[:, 0] = ledger
    h[:, 1] = ids
    h[:, 2] = lacs
    h[:, 3] = lenf
    return h.view(np.uint8).reshape(n, 32)


def digest_bytes(algo, digests):
    """[n, mac] digest bytes: a BE int (CRC32C) or the zero-extended BE long (CRC32)."""
    n = len(digests)
    out = np.zeros((n, MAC[algo]), dtype=np.uint8)
    out[:, -4:] = np.asarray(digests, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    return out


def _place(item_lens, shift):
    """Offsets of items packed in order, item i starting at a byte = (5 i + shift) mod 16 (the buffer's
    base is 16-byte aligned), in a slot of whole 16-byte blocks; (offsets, size) with the last item
    ending on the buffer's last byte."""
    n = len(item_lens)
    r = (5 * np.arange(n, dtype=np.int64) + shift) % 16
    slot = (r + item_lens + 15) // 16 * 16
    offs = np.cumsum(slot) - slot + r
    assert (offs[1:] >= offs[:-1] + item_lens[:-1]).all()
    return offs, int(offs[-1] + item_lens[-1])


class Case:
    """n entries of ledger LEDGER[G], ids FIRST_ENTRY_ID .., in one buffer `blob`.
    framed=False (package): blob holds the payloads alone, payload i at poffs[i].
    framed=True (verify): blob holds whole frames, frame i of flens[i] bytes at foffs[i]; five frames
    shorter than a header + digest come first (`short`; their bytes are whatever the fill left).
    head[i] = the [32 B header][digest] the oracle gives entry i; digests[i] its digest."""

    def __init__(self, G, algo, shift, framed):
        self.G, self.algo, self.shift, self.framed = G, algo, shift, framed
        self.mac = MAC[algo]
        self.hl = hl = 32 + self.mac
        self.ledger = LEDGER[G]
        self.first = FIRST_ENTRY_ID
        plens = lengths_for(G)
        if framed:
            too_short = np.array([0, 1, 31, 32, hl - 1], dtype=np.int64)
            self.flens = np.concatenate([too_short, plens + hl])
            self.short = self.flens < hl
            self.plens = np.where(self.short, 0, self.flens - hl)
            assert (np.diff(self.flens) >= 0).all()
        else:
            self.plens = plens
            self.short = np.zeros(plens.size, dtype=bool)
        self.n = n = self.plens.size
        rng = np.random.default_rng(1000 * G + 10 * algo + shift)
        self.ids = self.first + np.arange(n, dtype=np.int64)
        assert self.ids[0] < 2**32 <= self.ids[-1]
        self.lacs = rng.integers(-1, 2**63, n, dtype=np.int64)
        self.lacs[n // 3], self.lacs[2 * n // 3] = -1, 2**63 - 1
        self.lenf = LENGTH_FIELD_BASE + np.cumsum(self.plens)
        assert (self.lenf != self.plens).all()
        if framed:
            self.foffs, size = _place(self.flens, shift)
            self.poffs = self.foffs + hl
        else:
            self.poffs, size = _place(self.plens, shift)
        self.blob = oracle.fill_splitmix64(size, 7 + 100 * G + 10 * algo + shift)
        self.hdr = headers(self.ledger, self.ids, self.lacs, self.lenf)
        hcrc = oracle.batch(algo, self.hdr.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
        ok = ~self.short
        self.digests = np.zeros(n, dtype=np.uint32)
        self.digests[ok] = oracle.batch(algo, self.blob, self.poffs[ok].astype(np.uint64),
                                        self.plens[ok].astype(np.uint32), seeds=hcrc[ok])
        self.head = np.concatenate([self.hdr, digest_bytes(algo, self.digests)], axis=1)
        if framed:
            at = (self.foffs[ok, None] + np.arange(hl)).reshape(-1)
            self.blob[at] = self.head[ok].reshape(-1)
            assert size == self.foffs[-1] + self.flens[-1]
        else:
            assert size == self.poffs[-1] + self.plens[-1]
        self._check_residues()

    def _check_residues(self):
        """Every payload start residue mod 16 occurs in the serial class and in every step count
        1 .. 6 PF (the payload's start is what the fold sees, in package and in verify)."""
        S = 16 * self.G
        res = self.poffs % 16
        live = ~self.short
        serial = live & (self.plens < 16)
        assert set(res[serial].tolist()) == set(range(16))
        J = (self.plens + S - 1) // S
        for j in range(1, 6 * PF + 1):
            assert set(res[live & (self.plens >= 16) & (J == j)].tolist()) == set(range(16)), j
        assert J.max() == 6 * PF

    def frame(self, blob, i):
        return blob[self.foffs[i]:self.foffs[i] + self.flens[i]]

    def frame_views(self, blob):
        """Frame i as a view of blob (the host routes take one buffer per entry)."""
        return [blob[o:o + l] for o, l in zip(self.foffs.tolist(), self.flens.tolist())]

    def payload_views(self):
        return [self.blob[o:o + l] for o, l in zip(self.poffs.tolist(), self.plens.tolist())]

    def statuses(self, blob, skip_entry_check=False):
        """oracle.verify_entry of every frame of `blob`, frame by frame."""
        return np.array([oracle.verify_entry(self.algo, self.frame(blob, i), self.ledger, int(self.ids[i]),
                                             skip_entry_check) for i in range(self.n)], dtype=np.int32)


@functools.lru_cache(maxsize=3)
def package_case(G, algo, shift):
    return Case(G, algo, shift, False)


@functools.lru_cache(maxsize=3)
def verify_case(G, algo, shift):
    """(case, bands, picks, corrupted blob, clean statuses, corrupted statuses, the same with
    skip_entry_check)."""
    c = Case(G, algo, shift, True)
    bd = bands(c.flens)
    assert c.short[:5].all() and bd[0][0] == 0 and bd[0][1] > 5  # the too-short frames sit inside the first band
    pk = picks_for(c, bd)
    bad = corrupt(c, pk)
    clean, want = c.statuses(c.blob), c.statuses(bad)
    assert (clean == np.where(c.short, 1, 0)).all()
    for kind, st in zip(KINDS, (2, 2, 2, 2, 2, 3, 4, 3, 2)):
        assert all(want[i] == st for k, i in pk if k == kind), kind
    assert ((want != clean) == np.isin(np.arange(c.n), [i for _, i in pk])).all()
    return c, bd, pk, bad, clean, want, c.statuses(bad, True)


def bands(frame_lengths):
    """Greedy partition of the ascending frame lengths into runs the verify gate accepts: [(i0, i1)).
    A run's first (smallest) length is its reference; l belongs while l - ref <= ref // 16 + 64
    (PlanRun::in_band, crc_kernels.hpp; the gate compares every length with the call's first)."""
    fl = np.asarray(frame_lengths, dtype=np.int64)
    assert (np.diff(fl) >= 0).all()
    out, i0 = [], 0
    while i0 < fl.size:
        ref = int(fl[i0])
        i1 = int(np.searchsorted(fl, ref + ref // 16 + 64, side="right"))
        d = np.abs(fl[i0:i1] - ref)
        assert i1 > i0 and (d <= ref // 16 + 64).all()
        assert i1 == fl.size or fl[i1] - ref > ref // 16 + 64
        out.append((i0, i1))
        i0 = i1
    return out


def picks_for(case, band_list):
    """One frame per corruption kind in every band (fewer in a band of fewer frames): [(kind, index)],
    the frames spread evenly over the band's frames that have a payload (its first and last among
    them), the kinds rotated from band to band so that each meets other lengths and alignments."""
    picks = []
    for b, (i0, i1) in enumerate(band_list):
        idx = i0 + np.nonzero(case.plens[i0:i1] >= 1)[0]
        k = min(len(KINDS), idx.size)  # (the greedy partition can leave a run of a few frames)
        assert k >= 1, (b, i0, i1)
        at = idx[np.linspace(0, idx.size - 1, k).round().astype(np.int64)]
        assert np.unique(at).size == k
        picks += [(KINDS[(j + b) % len(KINDS)], int(i)) for j, i in enumerate(at)]
    assert {kind for kind, _ in picks} == set(KINDS)
    return picks


def corrupt(case, picks):
    """A copy of case.blob with one corruption per (kind, index). A wrong ledger or entry id carries
    a digest that is valid for it, so that the id check decides; `ledger` and `entry` differ from the
    right id in the high word alone (ids compared as 32-bit would pass), `ledger_entry` in the low
    words of both (ledger id decides: 3), `digest_ledger` has a wrong digest too (digest decides: 2).
    `high` is CRC32's zero high digest word; CRC32C's 4-byte digest has none, its top byte is flipped."""
    blob = case.blob.copy()
    hl, algo = case.hl, case.algo
    for kind, i in picks:
        f = case.frame(blob, i)
        assert f.size > hl
        if kind == "payload_first":
            f[hl] ^= 0x01
        elif kind == "payload_last":
            f[-1] ^= 0x80
        elif kind == "digest":
            f[hl - 1] ^= 0x01
        elif kind == "lac":
            f[16 + i % 8] ^= 0x20
        elif kind == "high":
            f[32 if algo == oracle.CRC32C else 32 + i % 4] ^= 0x10
        elif kind == "digest_ledger":
            f[7] ^= 0x02
            f[hl - 2] ^= 0x40
        else:
            lid, eid = np.int64(case.ledger), np.int64(case.ids[i])
            if kind == "ledger":
                lid ^= np.int64(1 << 32)
            elif kind == "entry":
                eid ^= np.int64(1 << 32)
            elif kind == "ledger_entry":
                lid ^= np.int64(1)
                eid += np.int64(5)
            else:
                raise KeyError(kind)
            d, hdr = oracle.digest_entry(algo, int(lid), int(eid), int(case.lacs[i]), int(case.lenf[i]), f[hl:])
            f[:hl] = np.frombuffer(hdr + oracle.digest_bytes(algo, d), dtype=np.uint8)
    return blob


@functools.lru_cache(maxsize=3)
def in_place_case(G, algo, shift):
    """package_case's payloads with room for each frame in front of its payload: (blob, frame offset
    of entry 0, stride, payload offsets). One stride for every frame (the package call takes one), = 5
    mod 16, so payload i again starts at a byte = (5 i + shift) mod 16; the last payload ends on the
    buffer's last byte."""
    c = package_case(G, algo, shift)
    n, hl = c.n, c.hl
    stride = int(hl + c.plens.max())
    stride += (5 - stride) % 16
    f0 = (shift - hl) % 16
    poffs = f0 + hl + stride * np.arange(n, dtype=np.int64)
    assert ((poffs % 16) == (5 * np.arange(n) + shift) % 16).all()
    blob = oracle.fill_splitmix64(int(poffs[-1] + c.plens[-1]), 9 + G + algo + shift)
    run = np.arange(int(c.plens.sum()), dtype=np.int64) - np.repeat(np.cumsum(c.plens) - c.plens, c.plens)
    blob[np.repeat(poffs, c.plens) + run] = c.blob[np.repeat(c.poffs, c.plens) + run]
    return blob, f0, stride, poffs
