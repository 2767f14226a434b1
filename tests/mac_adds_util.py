"""Shared by the MAC adds suites (composite payloads and V2 add requests of MAC ledgers): the batches both
the CPU and the GPU tests run, with what Python's hmac says they must give (mac_util)."""
import struct

import numpy as np

import mac_util as mu

PASSWORDS = [b"alpha", b"bravo-bravo", b""]
KEYS = [mu.mac_key(p) for p in PASSWORDS]
CAP = 16 << 20  # BKD_MAC_MAX_ENTRY
MASTER = bytes(range(100, 120))


class Batch:
    """Composite entries over one payload buffer. put() appends a piece behind at least one byte of 0xEE
    filler, at an address that is `mod` modulo 4 (the buffer itself is 16-byte aligned on the device);
    entry() lists segments (offset, length) of the buffer, in any order, shared or overlapping."""

    def __init__(self):
        self.buf = bytearray()
        self.offs, self.lens, self.first = [], [], [0]
        self.rows, self.lids, self.eids, self.lacs, self.lfs = [], [], [], [], []
        self.data = []  # what entry i's segments spell, or None for an entry that must not be read

    def put(self, data: bytes, mod=None):
        self.buf += b"\xEE"
        while mod is not None and len(self.buf) % 4 != mod:
            self.buf += b"\xEE"
        self.buf += data
        return len(self.buf) - len(data), len(data)

    def entry(self, segs, row=None, ids=None, readable=True):
        i = len(self.rows)
        for o, l in segs:
            self.offs.append(o)
            self.lens.append(l)
        self.first.append(len(self.offs))
        self.rows.append(i % len(KEYS) if row is None else row)
        lid, eid, lac, lf = ids or (mu.LEDGER + 7 * i, 1000 + i, 999 + i if i % 5 else -1, (1 << 33) + i)
        self.lids.append(lid)
        self.eids.append(eid)
        self.lacs.append(lac)
        self.lfs.append(lf)
        self.data.append(b"".join(bytes(self.buf[o:o + l]) for o, l in segs if l) if readable else None)
        return i

    def pieces(self, data: bytes, cuts, mods=None, **kw):
        """`data` cut at `cuts` into pieces, each put on its own, as one entry."""
        edges = [0] + list(cuts) + [len(data)]
        mods = mods or [None] * (len(edges) - 1)
        return self.entry([self.put(data[a:b], m) for a, b, m in zip(edges, edges[1:], mods)], **kw)

    @property
    def n(self):
        return len(self.rows)

    def header(self, i):
        return mu.header(self.lids[i], self.eids[i], self.lacs[i], self.lfs[i])

    def expected(self):
        """The 52 bytes package must write per entry: zero MAC bytes for an entry that must not be read."""
        out = []
        for i in range(self.n):
            hdr = self.header(i)
            ok = self.data[i] is not None and self.rows[i] < len(KEYS)
            out.append(hdr + (mu.mac_of_parts((hdr, self.data[i]), KEYS[self.rows[i]]) if ok else bytes(20)))
        return out

    def arrays(self):
        """(payload uint8, seg_offsets int64, seg_lengths int32, seg_first int64, rows int32, ledger ids,
        entry ids, LACs, length fields int64)."""
        i64 = np.int64
        return (np.frombuffer(bytes(self.buf), dtype=np.uint8), np.array(self.offs, dtype=i64),
                np.array(self.lens, dtype=np.uint32).view(np.int32), np.array(self.first, dtype=i64),
                np.array(self.rows, dtype=np.uint32).view(np.int32), np.array(self.lids, dtype=i64),
                np.array(self.eids, dtype=i64), np.array(self.lacs, dtype=i64), np.array(self.lfs, dtype=i64))

    def host_payloads(self):
        """Entry i as the list of its segments, views of one array (the host forms' composite payloads)."""
        whole = np.frombuffer(bytes(self.buf), dtype=np.uint8)
        return [[whole[self.offs[k]:self.offs[k] + self.lens[k]] for k in range(self.first[i], self.first[i + 1])]
                for i in range(self.n)]


def payload_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def cut_sweep():
    """Payload lengths 0..140 (the header block's second half and the padding edges at message lengths
    55/56/63/64 and 119/120/127/128), every two-segment cut, the two addresses through all 16 combinations
    modulo 4: 10 011 entries."""
    b, k = Batch(), 0
    for length in range(141):
        data = payload_bytes(length, 100 + length)
        for c in range(length + 1):
            b.pieces(data, [c], mods=[k % 4, (k // 4) % 4])
            k += 1
    return b


def three_segments():
    """A middle segment of 1, 2 or 3 bytes at every position of a message word, across word boundaries and
    across the block boundaries at message bytes 64 and 128 (payload bytes 32 and 96)."""
    b, k = Batch(), 0
    for len0 in list(range(0, 9)) + list(range(27, 37)) + list(range(91, 101)):
        for mid in (1, 2, 3):
            for len2 in (0, 5, 70):
                data = payload_bytes(len0 + mid + len2, 7 * len0 + mid)
                b.pieces(data, [len0, len0 + mid], mods=[k % 4, (k // 4) % 4, (k // 16) % 4])
                k += 1
    return b


def tiny_segments():
    """70 one-byte segments with empty ones at head, middle and tail; only empty segments; no segments."""
    b = Batch()
    data = payload_bytes(70, 9)
    segs = [(5, 0)]
    for j in range(70):
        segs.append(b.put(data[j:j + 1], j % 4))
        if j in (30, 31):
            segs.append((segs[-1][0], 0))
    segs.append((0, 0))
    b.entry(segs)
    b.entry([(0, 0), (3, 0), (1, 0)])
    b.entry([])
    b.pieces(payload_bytes(9, 10), [4])
    return b


def shared_and_edges():
    """Segments shared by two entries, overlapping, in descending address order; a segment that ends on the
    payload's last byte and an empty one at offset == payload size (no filler behind the last piece)."""
    b = Batch()
    a = b.put(payload_bytes(50, 21), 1)
    c = b.put(payload_bytes(33, 22), 3)
    d = b.put(payload_bytes(7, 23), 2)
    last = b.put(payload_bytes(41, 24), 2)
    size = len(b.buf)
    assert last[0] + last[1] == size
    b.entry([a, c])
    b.entry([c, a])  # shared, and in descending address order
    b.entry([(a[0], 30), (a[0] + 10, 40)])  # overlapping
    b.entry([d, c, a, d])
    b.entry([last, (size, 0)])
    b.entry([(size, 0), a, last])
    return b


def long_entries():
    """96 + 4 000 bytes, and a second segment of 4 090..4 100 bytes on either side of the 96."""
    b = Batch()
    data = payload_bytes(96 + 4100, 31)
    b.pieces(data[:4096], [96], mods=[0, 0])
    for k, l in enumerate(range(4090, 4101)):
        b.pieces(data[:96 + l], [96], mods=[k % 4, (k + 1) % 4])
        b.pieces(data[:96 + l], [l], mods=[(k + 2) % 4, k % 4])
    return b


def mixed(n: int, seed: int = 40):
    """n entries of two or three pieces, 0..300 bytes in all: the batch-size cases."""
    b = Batch()
    rng = np.random.default_rng(seed)
    for i in range(n):
        length = int(rng.integers(0, 301))
        cuts = sorted(int(x) for x in rng.integers(0, length + 1, 1 + i % 2))
        b.pieces(payload_bytes(length, seed + i), cuts, mods=[int(m) for m in rng.integers(0, 4, len(cuts) + 1)])
    return b


MALFORMED = ("decreasing", "past nseg", "first not zero")


def malformed_first(first, nseg: int, kind: str):
    """The three malformed CSRs of the CRC segments test, from a good seg_first of a batch of >= 4 entries."""
    first = np.array(first, dtype=np.int64)
    if kind == "decreasing":
        first[2] = first[1] - 1 if first[1] else first[3] + 1
    elif kind == "past nseg":
        first[-1] = nseg + 5
    else:
        first[0] = 1
    return first


# ---- V2 add requests ----

def packet_header(flags: int) -> int:
    return (2 << 24) | (1 << 16) | (flags & 0xFFFF)


def v2_request(hdr: bytes, mac: bytes, payload: bytes, master: bytes, flags: int, small: int) -> bytes:
    """[int32 BE 76 + len][int32 BE packet header][20 B master key][32 B header][20 B MAC] and the payload
    when it is shorter than `small` (DigestManager.java:126-167 with a 20-byte digest)."""
    head = struct.pack(">II", (76 + len(payload)) & 0xFFFFFFFF, packet_header(flags)) + master + hdr + mac
    assert len(head) == 80
    return head + (payload if len(payload) < small else b"")


def v2_expected(payloads, rows, lids, eids, lacs, lfs, masters, flags: int, small: int, readable=None):
    out = []
    for i, p in enumerate(payloads):
        hdr = mu.header(int(lids[i]), int(eids[i]), int(lacs[i]), int(lfs[i]))
        ok = (readable is None or readable[i]) and rows[i] < len(KEYS)
        mac = mu.mac_of_parts((hdr, p), KEYS[rows[i]]) if ok else bytes(20)
        out.append(v2_request(hdr, mac, bytes(p) if ok else b"\0" * len(p), masters[i], flags, small if ok else 0))
    return out


def ids_for(n: int, seed: int = 50):
    rng = np.random.default_rng(seed)
    lids = rng.integers(0, 2**63, n, dtype=np.int64)
    eids = rng.integers(0, 2**63, n, dtype=np.int64)
    lacs = rng.integers(0, 2**63, n, dtype=np.int64)
    lacs[::4] = -1
    lfs = rng.integers(0, 2**63, n, dtype=np.int64)
    rows = (np.arange(n) % len(KEYS)).astype(np.int32)
    return rows, lids, eids, lacs, lfs
