"""Shared by test_reframe_host.py and test_gpu_reframe.py: framed entries and their re-framed form, both
from the oracle's DigestManager framing (never from the code under test)."""
import numpy as np

import oracle

MAC = {0: 4, 1: 8}


def frame(algo, ledger, entry_id, lac, length_field, payload):
    """(frame bytes [32 B header][digest][payload], digest) as DigestManager packages the entry."""
    d, hdr = oracle.digest_entry(algo, ledger, int(entry_id), int(lac), int(length_field), payload)
    return hdr + oracle.digest_bytes(algo, d) + bytes(payload), d


class Batch:
    """n entries of ledger `ledger` with ids first .. first + n - 1, payload i of plens[i] bytes, framed
    with LAC id - 1 (`old`) and with new_lacs[i] (`new_head` = its [header][digest], new_frame(i) the
    whole frame); the length field is a running ledger length, not the payload's own."""

    def __init__(self, algo, ledger, first, plens, new_lacs, seed):
        self.algo, self.ledger, self.first = algo, ledger, first
        self.mac = MAC[algo]
        self.n = len(plens)
        data = oracle.fill_splitmix64(int(np.sum(plens)) + 8, seed)
        at = np.concatenate([[0], np.cumsum(plens)]).astype(np.int64)
        self.new_lacs = np.asarray(new_lacs, dtype=np.int64)
        self.lenf = 1000 + at[1:]
        self.old, self.new_head, self.old_digests, self.new_digests = [], [], [], []
        for i in range(self.n):
            p = data[at[i]:at[i + 1]].tobytes()
            f, d = frame(algo, ledger, first + i, first + i - 1, self.lenf[i], p)
            e, hdr = oracle.digest_entry(algo, ledger, first + i, int(self.new_lacs[i]), int(self.lenf[i]), p)
            self.old.append(f)
            self.new_head.append(hdr + oracle.digest_bytes(algo, e))
            self.old_digests.append(d)
            self.new_digests.append(e)
        self.new_digests = np.array(self.new_digests, dtype=np.uint32)

    def new_frame(self, i):
        return self.new_head[i] + self.old[i][32 + self.mac:]


def corrupt(b: Batch, where: dict):
    """Frames of b.old as bytearrays with one corruption per kind at the given indices
    (kind -> index): short, payload, digest, high (CRC32's zero high digest word), ledger, entry.
    A wrong ledger or entry id carries a digest that is valid for it, so that the id check decides."""
    frames = [bytearray(f) for f in b.old]
    hl = 32 + b.mac
    for kind, i in (where.items() if isinstance(where, dict) else where):  # (or (kind, index) pairs)
        if kind == "short":
            frames[i] = frames[i][:20]
        elif kind == "payload":
            assert len(frames[i]) > hl
            frames[i][hl + (len(frames[i]) - hl) // 2] ^= 0x40
        elif kind == "digest":
            frames[i][hl - 1] ^= 0x01
        elif kind == "high":
            if b.algo == 1:
                frames[i][33] ^= 0x10
        elif kind in ("ledger", "entry"):
            pay = bytes(frames[i][hl:])
            lid = b.ledger + (kind == "ledger")
            eid = b.first + i + 5 * (kind == "entry")
            frames[i] = bytearray(frame(b.algo, lid, eid, b.first + i - 1, b.lenf[i], pay)[0])
        else:
            raise KeyError(kind)
    return frames


def pack(frames, rng=None, misalign=(0,), lead=0):
    """One buffer holding the frames back to back, frame i moved so that its offset is congruent to
    misalign[i % len] modulo 8 (gaps of up to 7 bytes), after `lead` bytes: (blob, offsets, lengths)."""
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    offs = np.zeros(len(frames), dtype=np.int64)
    at = lead
    for i, f in enumerate(frames):
        at += (misalign[i % len(misalign)] - at) % 8
        offs[i] = at
        at += len(f)
    blob = np.zeros(at + 64, dtype=np.uint8)
    for i, f in enumerate(frames):
        blob[offs[i]:offs[i] + lens[i]] = np.frombuffer(bytes(f), dtype=np.uint8)
    return blob, offs, lens
