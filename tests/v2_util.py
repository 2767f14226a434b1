"""Shared by test_package_v2_cpu.py and test_gpu_package_v2.py: what a V2 add request must hold.

Request i, as DigestManager.computeDigestAndPackageForSendingV2 builds it (DigestManager.java:126-167):
struct.pack(">ii", 4 + 20 + 32 + mac + length, PacketHeader.toInt(2, ADDENTRY, flags)), the 20-byte master
key, the 32-byte BE header, the digest bytes, and the payload when it is shorter than the threshold. The
header CRC and the payload resumed from it come from the oracle (oracle.batch, as framed_util's cases
take them; oracle.digest_entry entry by entry where a test says so), never from the library.
"""
import ctypes
import struct

import numpy as np

import framed_util as fu
import oracle

MAC = fu.MAC
PREFIX = 28
SENTINEL = 0xA5


def packet_header(flags):
    """BookieProtocol.PacketHeader.toInt(CURRENT_PROTOCOL_VERSION = 2, ADDENTRY = 1, flags)
    (BookieProtocol.java:47, 75-83, 114)."""
    return (2 << 24) | (1 << 16) | (flags & 0xFFFF)


def head_len(algo):
    return PREFIX + 32 + MAC[algo]


def key_of(keys, key_stride, i):
    return bytes(keys[i * key_stride:i * key_stride + 20])


def digests_for(algo, ledgers, ids, lacs, lenf, blob, poffs, plens):
    """(digests uint32[n], headers uint8[n, 32]) from the oracle: the header's CRC, the payload resumed
    from it (DigestManager.java:152-153)."""
    n = len(ids)
    hdr = fu.headers(ledgers, ids, lacs, lenf)
    hcrc = oracle.batch(algo, hdr.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
    dig = oracle.batch(algo, blob, np.asarray(poffs, dtype=np.uint64), np.asarray(plens, dtype=np.uint32), seeds=hcrc)
    return dig, hdr


def expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, key_stride, flags, small):
    """([request i as bytes], digests uint32[n])."""
    dig, hdr = digests_for(algo, ledgers, ids, lacs, lenf, blob, poffs, plens)
    mac = MAC[algo]
    pkt = packet_header(flags)
    out = []
    for i in range(len(ids)):
        l, o = int(plens[i]), int(poffs[i])
        r = struct.pack(">ii", 4 + 20 + 32 + mac + l, pkt) + key_of(keys, key_stride, i) + hdr[i].tobytes()
        r += oracle.digest_bytes(algo, int(dig[i]))
        if l < small:
            r += blob[o:o + l].tobytes()
        out.append(r)
    return out, dig


def ids_for(n, seed, per_entry):
    """Header fields that use their 64 bits: (ledger ids int64[n] or one id, entry ids with a carry into
    the high word, LACs, length fields that are not the payload's length)."""
    rng = np.random.default_rng(seed)
    ledgers = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) if per_entry else np.int64(-2**63 + 61)
    if per_entry and n > 2:
        ledgers[0], ledgers[n // 2], ledgers[-1] = -2**63, 2**63 - 1, 2**32
    ids = fu.FIRST_ENTRY_ID - n // 2 + np.arange(n, dtype=np.int64)
    lacs = rng.integers(-1, 2**63 - 1, n, dtype=np.int64)
    lenf = fu.LENGTH_FIELD_BASE + 3 * np.arange(n, dtype=np.int64)
    return ledgers, ids, lacs, lenf


def keys_for(n, key_stride, seed):
    """The master keys: 20 bytes for all (key_stride 0), or n keys key_stride bytes apart with other
    bytes between them."""
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, 20 if key_stride == 0 else n * key_stride, dtype=np.uint8)


def package_v2_host_raw(algo, ledger_id, ledger_ids, ids, lacs, lenf, views, keys, key_stride, flags, small, bufs):
    """bkd_digest_package_batch_v2_host with the caller's request buffers `bufs` (writable uint8 arrays):
    (rc, digests)."""
    from bookkeeper_amd import _native
    n = len(views)
    vp = ctypes.c_void_p
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    lens = np.array([v.size for v in views], dtype=np.uint32)
    rptr = np.array([b.ctypes.data for b in bufs], dtype=np.uint64)
    digests = np.zeros(n, dtype=np.uint32)
    lids = None if ledger_ids is None else np.ascontiguousarray(ledger_ids, dtype=np.int64)
    rc = _native.lib().bkd_digest_package_batch_v2_host(
        algo, int(ledger_id), vp(0 if lids is None else lids.ctypes.data), vp(ids.ctypes.data), vp(lacs.ctypes.data),
        vp(lenf.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(keys.ctypes.data), key_stride, flags,
        small, vp(rptr.ctypes.data), vp(digests.ctypes.data))
    return rc, digests


def sentinel_buffers(algo, plens, extra=16):
    """One request buffer per entry, every one long enough for head + payload + `extra` whether or not
    the payload is copied, filled with SENTINEL."""
    return [np.full(head_len(algo) + int(l) + extra, SENTINEL, dtype=np.uint8) for l in plens]


def check_buffer(buf, want, what):
    """buf holds `want` and then only sentinel bytes."""
    got = buf[:len(want)].tobytes()
    assert got == want, (what, "request bytes", next(k for k in range(len(want)) if got[k] != want[k]))
    assert (buf[len(want):] == SENTINEL).all(), (what, "bytes behind the request were written")
