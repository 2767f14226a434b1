"""Shared by the MAC reframe suites (test_mac_reframe_cpu.py, test_gpu_mac_reframe.py): what Python's hmac
says a reframe must leave behind, on top of mac_util and mac_requests_util."""
import numpy as np

import mac_requests_util as mq
import mac_util as mu


def lac_of(i: int) -> int:
    """A new LAC per entry: every third one from WIDE_LACS (-1 and both high-word edges included)."""
    return mu.WIDE_LACS[(i // 3) % 4] if i % 3 == 0 else 10**12 + 17 * i


def reframed(f, lac: int, key: bytes) -> bytes:
    """The frame a reframe of f (a frame of at least 52 bytes) with `lac` must leave: header bytes 16..23 and
    the MAC at 32..51 anew, by hmac over the bytes as they lie."""
    f = bytes(f)
    hdr = f[:16] + lac.to_bytes(8, "big", signed=True) + f[24:32]
    return hdr + mu.mac_of_parts((hdr, f[52:]), key) + f[52:]


def entry_keys(b) -> list:
    """The HMAC key of each entry of a mac_requests_util.Requests (rows keyed with password(k))."""
    return [mq.key(int(b.req_keys[b.req_of(i)])) for i in range(b.n)]


def want_frames(frames, lacs, keys, status) -> list:
    """Every frame after the call: re-framed where its status is 0, byte for byte otherwise."""
    return [reframed(f, int(lacs[i]), keys[i]) if status[i] == 0 else bytes(f) for i, f in enumerate(frames)]


def header_status(b, frames) -> np.ndarray:
    """The trusted mode's statuses: 1 under 52 bytes, else what the ids alone decide; never 2."""
    out = []
    for i, f in enumerate(frames):
        r = b.req_of(i)
        if len(f) < 52:
            out.append(1)
            continue
        lid, eid = int.from_bytes(f[:8], "big", signed=True), int.from_bytes(f[8:16], "big", signed=True)
        exp = int(b.firsts[r]) + i - int(b.first[r])
        out.append(3 if lid != int(b.lids[r]) else (4 if (eid != exp and not int(b.flags[r]) & 1) else 0))
    return np.array(out, dtype=np.int32)


def failures(skip: int, before: int = 6):
    """mu.failure_frames() as request 2 of 4, among good neighbours with keys of their own: (the requests,
    the passwords of the key table, each entry's key, the first failure frame's index, their count)."""
    bad, _, _ = mu.failure_frames()
    b = mq.Requests([before, 0, len(bad), 7], seed=6, keys=[1, 2, 0, 3])
    lo = int(b.first[2])
    b.frames[lo:lo + len(bad)] = bad
    b.lids[2], b.firsts[2], b.flags[2] = mu.LEDGER, mu.FIRST_ENTRY, skip
    keys = [mq.key(1)] * before + [mu.mac_key()] * len(bad) + [mq.key(3)] * 7
    return b, [mu.PASSWD] + b.passwords()[1:], keys, lo, len(bad)  # failure_frames() are keyed with mac_util's password


def damaged_frames():
    """Among mu.failure_frames(): (the one frame with a flipped digest and a foreign ledger, the frames of
    the right ledger with one flipped byte — the LAC, five MAC words, the first and the last payload byte)."""
    bad, ref, _ = mu.failure_frames()
    foreign = mu.header(mu.LEDGER + 1, 0, 0, 0)[:8]
    both = [i for i, f in enumerate(bad) if ref[i] == 2 and f[:8] == foreign]
    damaged = [i for i, f in enumerate(bad) if ref[i] == 2 and f[:8] != foreign]
    assert len(both) == 1 and len(damaged) == 8
    return both[0], damaged
