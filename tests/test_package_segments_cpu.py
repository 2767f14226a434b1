"""CPU: packaging batches whose payloads are composite buffers (bkd_digest_package_batch_segments_host,
bkd_crc_batch_segments_host) on the library's CPU route, the clamp the device applies to seg_first
(bkd_host_segments_range) and a model of the device join with the byte-power table.

The expected value is always oracle.digest_entry over the concatenation of an entry's segments (digest
and every frame byte), for the digest-only call oracle.resume. Every entry of every batch is compared.
"""
import ctypes

import numpy as np
import pytest

import oracle
import segments_util as su
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd.bytebuf import CompositeBuffer
from test_bytebuf import scenarios

INVALID_ARG = -1
DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}


@pytest.fixture(autouse=True)
def _cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


@pytest.mark.parametrize("per_entry", [False, True], ids=["one_ledger", "ledger_ids"])
@pytest.mark.parametrize("stride", [None, 64], ids=["packed", "stride64"])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_host_package_cpu_route(algo, stride, per_entry):
    """The fixture batch through the host form on the CPU route: digests, every frame byte, and with
    stride 64 the sentinel in the 64 - 32 - mac bytes between frames."""
    b = su.batch()
    stride = stride or 32 + su.MAC[algo]
    want_d, want_h = b.expected(algo, per_entry)
    rc, frames, digests = su.package_host_raw(algo, su.ONE_LEDGER[algo], b.ledgers if per_entry else None, b.ids, b.lacs,
                                           b.lenf, b.segment_views(), b.first, stride)
    assert rc == 0, _native.last_error()
    su.check_frames(frames, digests, want_d, want_h, stride)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_python_host_surface(algo):
    """DigestManager.package_batch_segments_host and the module-level many-ledger form on the fixture
    batch (each payload a list of buffers), a bytes payload and a composite among them."""
    b = su.batch()
    payloads = b.payloads()
    payloads[3] = b.cat[3]                                    # bytes-like: one segment
    payloads[4] = CompositeBuffer([bytes(v) for v in payloads[4]])
    for per_entry in (False, True):
        want_d, want_h = b.expected(algo, per_entry)
        if per_entry:
            frames, digests = dg.package_batch_segments_host(DTYPE[algo], b.ledgers, b.ids, b.lacs, b.lenf, payloads)
        else:
            dm = dg.DigestManager.instantiate(su.ONE_LEDGER[algo], b"", DTYPE[algo])
            frames, digests = dm.package_batch_segments_host(b.ids, b.lacs, b.lenf, payloads)
        assert frames.shape == want_h.shape and (frames == want_h).all()
        assert (digests == want_d).all()
    with pytest.raises(ValueError):
        dg.package_batch_segments_host(DTYPE[algo], b.ledgers[:5], b.ids, b.lacs, b.lenf, payloads)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_crc_batch_segments_host(algo):
    """The digest-only host form with per-entry seeds and with seed_all, against oracle.resume."""
    b = su.batch()
    views = b.segment_views()
    got = ck.crc_batch_segments_host(algo, views, b.first, seeds=b.seeds)
    want = np.array([oracle.resume(algo, int(b.seeds[i]), b.cat[i]) for i in range(b.n)], dtype=np.uint32)
    assert (got == want).all()
    got = ck.crc_batch_segments_host(algo, views, b.first, seed_all=0x5EED1234)
    want = np.array([oracle.resume(algo, 0x5EED1234, c) for c in b.cat], dtype=np.uint32)
    assert (got == want).all()
    with pytest.raises(ValueError):
        ck.crc_batch_segments_host(algo, views, b.first, seeds=b.seeds[:3])


def test_long_segments_fold_over_the_pool():
    """Segments of >= 4 MiB take the pool's piecewise fold inside the chain (host_batch.cpp fold)."""
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, 12 << 20, dtype=np.uint8)
    M = 1 << 20
    views = [host[3:3 + 100], host[7:7 + 5 * M + 13], host[M:M + 4 * M], host[11:11 + 50], host[5:5 + 4 * M - 1]]
    first = [0, 3, 3, 5]
    for algo in (ck.CRC32C, ck.CRC32):
        got = ck.crc_batch_segments_host(algo, views, first, seed_all=9)
        cats = [b"".join(v.tobytes() for v in views[first[i]:first[i + 1]]) for i in range(3)]
        assert got.tolist() == [oracle.resume(algo, 9, c) for c in cats]


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_composite_wrappings(algo):
    """The reference's four wrappings (CompositeByteBufUnwrapBugReproduceTest, as tests/test_bytebuf.py
    builds them) through package_batch_segments_host: equal to computeDigestAndPackageForSending on the
    same CompositeBuffer, and to the SURVEY §8c framing vectors."""
    vectors = {(ck.CRC32C, 16383): 0x24656066, (ck.CRC32C, 16384): 0x6fa1a26b,
               (ck.CRC32, 16383): 0xdf2ebb5b, (ck.CRC32, 16384): 0x4512b34e}
    dm = dg.DigestManager.instantiate(1, b"", DTYPE[algo])
    hl = 32 + dm.macCodeLength
    for size in (16383, 16384):
        payload = bytes(i & 0xFF for i in range(size))
        sc = scenarios(payload)
        names = list(sc)
        n = len(names)
        frames, digests = dm.package_batch_segments_host([1] * n, [0] * n, [size] * n, [sc[k] for k in names])
        d, hdr = oracle.digest_entry(algo, 1, 1, 0, size, payload)
        assert d == vectors[algo, size]
        for j, name in enumerate(names):
            assert digests[j] == vectors[algo, size], name
            assert bytes(frames[j]) == hdr + oracle.digest_bytes(algo, d), name
            sent = dm.computeDigestAndPackageForSending(1, 0, size, sc[name])
            assert sent[:hl] == bytes(frames[j]) and sent[hl:] == payload, name


def test_csr_errors_write_nothing():
    """A seg_first that does not start at 0, decreases, or does not end at nseg: BKD_ERR_INVALID_ARG
    before any work, no frame byte and no digest written — both host calls."""
    b = su.batch()
    views = b.segment_views()
    bad = {k: v for k, v in su.malformed_firsts(b.first, b.nseg).items()
           if k in ("first_not_zero", "decrease", "last_short", "past_nseg")}
    assert len(bad) == 4
    for name, first in bad.items():
        rc, frames, digests = su.package_host_raw(ck.CRC32C, 1, None, b.ids, b.lacs, b.lenf, views, first, 36)
        assert rc == INVALID_ARG, name
        assert (frames == su.SENTINEL).all() and (digests == 0xDEADBEEF).all(), name
        with pytest.raises(_native.BkdError) as e:
            ck.crc_batch_segments_host(ck.CRC32C, views, first)
        assert e.value.code == INVALID_ARG, name


def test_degenerate_sizes():
    b = su.batch()
    # n == 0: nothing is read (null arrays) and nothing written
    rc = _native.lib().bkd_digest_package_batch_segments_host(0, 1, None, None, None, None, None, None, 0, None, 0,
                                                              None, 36, None)
    assert rc == 0
    assert _native.lib().bkd_crc_batch_segments_host(0, None, None, 0, None, 0, None, 0, None) == 0
    assert ck.crc_batch_segments_host(ck.CRC32C, [], [0]).size == 0
    # nseg == 0 with n > 0: every payload is empty
    n = 5
    for algo in (ck.CRC32C, ck.CRC32):
        rc, frames, digests = su.package_host_raw(algo, 7, None, b.ids[:n], b.lacs[:n], b.lenf[:n], [], np.zeros(n + 1), 64)
        assert rc == 0
        want_d, want_h = su.expected_frames(algo, [7] * n, b.ids, b.lacs, b.lenf, [b""] * n)
        su.check_frames(frames, digests, want_d, want_h, 64)
        got = ck.crc_batch_segments_host(algo, [], np.zeros(n + 1), seeds=b.seeds[:n])
        assert (got == b.seeds[:n]).all()  # resume of nothing returns the seed
    # argument checks as in the neighbouring calls
    rc, _, _ = su.package_host_raw(2, 7, None, b.ids[:n], b.lacs[:n], b.lenf[:n], [], np.zeros(n + 1), 64)
    assert rc == INVALID_ARG
    rc, _, _ = su.package_host_raw(ck.CRC32, 7, None, b.ids[:n], b.lacs[:n], b.lenf[:n], [], np.zeros(n + 1), 39)
    assert rc == INVALID_ARG  # stride < 32 + mac


def segments_range(first_i, first_i1, i, n, nseg):
    k0, k1 = ctypes.c_uint64(0), ctypes.c_uint64(0)
    m = 2**64 - 1
    bad = _native.lib().bkd_host_segments_range(int(first_i) & m, int(first_i1) & m, i, n, nseg, ctypes.byref(k0),
                                                ctypes.byref(k1))
    return k0.value, k1.value, bad


def test_clamp_function():
    """The __host__ __device__ clamp of the device call (plan_kernels.hpp segments_range), on the CPU,
    with the malformed seg_first arrays and the out-of-range batch of the GPU tests: the range it yields
    never leaves [0, nseg], a valid CSR passes through untouched and unflagged, and every malformed
    array is flagged at one entry at least."""
    b = su.batch()
    n, nseg = b.n, b.nseg
    for i in range(n):
        assert segments_range(b.first[i], b.first[i + 1], i, n, nseg) == (b.first[i], b.first[i + 1], 0)
    for name, first in su.malformed_firsts(b.first, nseg).items():
        flagged = 0
        for i in range(n):
            k0, k1, bad = segments_range(first[i], first[i + 1], i, n, nseg)
            assert 0 <= k0 <= k1 <= nseg, (name, i)
            flagged += bad
            if not bad:  # an entry whose two values are sound reads exactly its own range
                assert (k0, k1) == (first[i], first[i + 1]), (name, i)
        assert flagged >= 1, name
    # nseg == 0 and single-entry batches
    assert segments_range(0, 0, 0, 3, 0) == (0, 0, 0)
    assert segments_range(0, 5, 0, 1, 0) == (0, 0, 1)
    assert segments_range(2**64 - 1, 2**64 - 1, 1, 3, 10) == (10, 10, 1)
    # the out-of-range batch keeps a valid CSR: nothing to clamp (its segments are refused by the
    # indexed path's own check, offset > size or length > size - offset, which cannot wrap)
    offs, lens, ents = su.out_of_range_segments(b)
    m = 2**64
    for e in ents:
        k = int(b.first[e])
        o, l = int(offs[k]) % m, int(lens[k])
        assert o > su.SIZE or l > su.SIZE - o


def test_bytewise_decision():
    """The join kernel's other bounds decision (plan_kernels.hpp segment_joined_bytewise), on the CPU: a
    segment is folded from its own bytes exactly when it is in range and shorter than 16 bytes, so a
    byte it reads always lies inside [0, size); the range test does not wrap. Driven with every segment
    of the fixture batch and of the out-of-range batch of the GPU tests."""
    L = _native.lib()
    b = su.batch()
    m = 2**64
    oo, ol, _ = su.out_of_range_segments(b)
    cases = list(zip(b.offs.tolist(), b.lens.tolist())) + list(zip(oo.tolist(), ol.tolist()))
    cases += [(su.SIZE, 0), (su.SIZE, 1), (su.SIZE - 15, 15), (su.SIZE - 15, 16), (su.SIZE - 14, 15), (su.SIZE + 1, 0),
              (-1, 0), (-1, 1), (-8, 15), (0, 15), (0, 16), (0, 0)]
    for size in (su.SIZE, 10, 0):
        for o, l in cases:
            o %= m
            want = l < 16 and o <= size and l <= size - o
            assert L.bkd_host_segment_bytewise(o, l, size) == int(want), (o, l, size)
            if want:
                assert o + l <= size


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_join_model_short_segments_bytewise(algo):
    """Segments under 16 bytes are folded onto the running register byte by byte with the fourth quarter
    of the x^32 operator's tables (the plain byte table), between segments joined by multiplication."""
    L = _native.lib()
    tab = ck.host_tables(algo, 4)[1024 + 768:1024 + 1024]
    assert (tab == oracle.table(algo)).all()
    data = oracle.fill_splitmix64(4096, 8)
    for short in range(0, 16):
        segs = [data[3:3 + 100], data[200:200 + short], data[1000:1000 + 17], data[50:50 + short]]
        reg = ~oracle.resume(algo, 0, b"header-stand-in") & 0xFFFFFFFF
        for sg in segs:
            if sg.size == 0:
                continue
            if sg.size < 16:
                for byte in sg.tolist():
                    reg = int(tab[(reg ^ byte) & 0xFF]) ^ (reg >> 8)
            else:
                reg = L.bkd_host_gf_mul(algo, L.bkd_host_xpow8n(algo, sg.size), reg)
                reg ^= ~oracle.resume(algo, 0xFFFFFFFF, sg) & 0xFFFFFFFF
        cat = b"header-stand-in" + b"".join(x.tobytes() for x in segs)
        assert ~reg & 0xFFFFFFFF == oracle.resume(algo, 0, cat), short


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_join_model_with_byte_power_table(algo):
    """package_segments_join_kernel's arithmetic in Python from the library's own host helpers: the
    header's register, then per segment reg = reg * x^(8 len) ^ raw with x^(8 len) the product of the
    byte-power table's words XP[256 k + byte k of len] = x^(8 byte 256^k) (one product per non-zero
    byte), raw = ~resume(~0, segment). Equal to the oracle for the lengths where the table index
    changes bytes."""
    L = _native.lib()
    xp = [[L.bkd_host_xpow8n(algo, v << (8 * k)) for v in range(256)] for k in range(4)]
    for k in range(4):
        assert xp[k][1] == oracle.xpow8n(algo, 1 << (8 * k)) and xp[k][255] == oracle.xpow8n(algo, 255 << (8 * k))
    big = oracle.fill_splitmix64(max(su.POWER_LENGTHS) + 64, 3)
    head = big[5:45].tobytes()
    hdr_fields = (2**63 - 1, 2**32 + 1, -1, 2**40)
    for length in su.POWER_LENGTHS:
        seg = big[13:13 + length]
        raw_seg = ~oracle.resume(algo, 0xFFFFFFFF, seg) & 0xFFFFFFFF
        raw_head = ~oracle.resume(algo, 0xFFFFFFFF, head) & 0xFFFFFFFF
        hdr = oracle.digest_entry(algo, *hdr_fields, b"")[1]
        reg = ~oracle.resume(algo, 0, hdr) & 0xFFFFFFFF  # update(0, header), as a register
        for n, raw in ((len(head), raw_head), (length, raw_seg), (0, None), (len(head), raw_head)):
            if n == 0:
                continue  # an empty segment is skipped
            for k in range(4):
                v = (n >> (8 * k)) & 0xFF
                if v:
                    reg = L.bkd_host_gf_mul(algo, xp[k][v], reg)
            reg ^= raw
        want, _ = oracle.digest_entry(algo, *hdr_fields, head + seg.tobytes() + head)
        assert ~reg & 0xFFFFFFFF == want, length
