"""CPU: V2 add requests packaged whole (bkd_digest_package_batch_v2_host) on the library's CPU route.

Every request byte is compared with v2_util.expected_requests (struct.pack for the prefix, the key, the
oracle's header CRC / digest, the payload); request buffers are 16 bytes longer than the request and
filled with 0xA5, and for an entry at or over the threshold long enough that a copied payload would show.
"""
import ctypes

import numpy as np
import pytest

import oracle
import v2_util as vu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

INVALID_ARG = -1
DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}
REAL = dg.SMALL_ENTRY_SIZE_THRESHOLD


@pytest.fixture(autouse=True)
def _cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


@pytest.fixture(params=[1, 0], ids=["1thread", "all_threads"])
def threads(request):
    ck.set_host_threads(request.param)
    yield request.param
    ck.set_host_threads(0)


def _batch(small, seed):
    """Payload lengths 0 .. 600 and the threshold's three neighbours, at mixed alignments in one blob."""
    plens = np.concatenate([np.arange(0, 601), [small - 1, small, small + 1]]).astype(np.int64)
    n = plens.size
    poffs = np.cumsum(plens + (5 * np.arange(n)) % 16) - plens
    blob = oracle.fill_splitmix64(int(poffs[-1] + plens[-1]), 77 + seed)
    return plens, poffs, blob


@pytest.mark.parametrize("flags", [0, 0xFFFF])
@pytest.mark.parametrize("key_stride", [0, 20, 24])
@pytest.mark.parametrize("small", [256, REAL])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_host_v2_cpu_route(algo, small, key_stride, flags, threads):
    assert _native.V2_SMALL_ENTRY_THRESHOLD == REAL == 16384
    plens, poffs, blob = _batch(small, algo)
    n = plens.size
    per_entry = key_stride != 0  # one ledger with one key, per-entry 64-bit ledger ids with per-entry keys
    ledgers, ids, lacs, lenf = vu.ids_for(n, 3 + algo, per_entry)
    keys = vu.keys_for(n, key_stride, algo)
    want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, key_stride, flags, small)
    assert {len(w) - vu.head_len(algo) for w in want[-3:]} == {small - 1, 0}  # the two at / over it: head only
    views = [blob[o:o + l] for o, l in zip(poffs.tolist(), plens.tolist())]
    bufs = vu.sentinel_buffers(algo, plens)
    rc, digests = vu.package_v2_host_raw(algo, 0 if per_entry else ledgers, ledgers if per_entry else None, ids, lacs,
                                         lenf, views, keys, key_stride, flags, small, bufs)
    assert rc == 0, _native.last_error()
    assert (digests == want_d).all()
    for i in range(n):
        vu.check_buffer(bufs[i], want[i], (i, int(plens[i])))


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_equals_the_per_call_mirror_and_digest_entry(algo):
    """Small entries: the bytes DigestManager.computeDigestAndPackageForSending returns with
    useV2Protocol (digest.py's mirror of :126-167), and the digest oracle.digest_entry gives."""
    rng = np.random.default_rng(11 + algo)
    key = bytes(rng.integers(0, 256, 20, dtype=np.uint8))
    ledger = -2**62 + 5
    payloads = [bytes(rng.integers(0, 256, l, dtype=np.uint8)) for l in (0, 1, 15, 16, 17, 255, 4096, REAL - 1)]
    n = len(payloads)
    ids = np.arange(2**32 - 3, 2**32 - 3 + n, dtype=np.int64)
    lacs, lenf = ids - 1, 2**40 + ids
    dm = dg.DigestManager.instantiate(ledger, b"", DTYPE[algo], True)
    reqs, digests = dm.package_batch_v2_host(ids, lacs, lenf, payloads, key, flags=0x1234)
    for i, p in enumerate(payloads):
        want = dm.computeDigestAndPackageForSending(int(ids[i]), int(lacs[i]), int(lenf[i]), p, key, 0x1234)
        assert reqs[i].tobytes() == want, i
        d, hdr = oracle.digest_entry(algo, ledger, int(ids[i]), int(lacs[i]), int(lenf[i]), p)
        assert int(digests[i]) == d & 0xFFFFFFFF
        assert want[28:60] == hdr and want[60:60 + vu.MAC[algo]] == oracle.digest_bytes(algo, d)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_python_host_surface(algo):
    """DigestManager.package_batch_v2_host and the many-ledger module form: a large entry returns its
    60 + mac bytes alone; per-entry keys as rows; a small threshold of 0 copies nothing."""
    plens = np.array([0, 40, 300, REAL, REAL + 5, 7], dtype=np.int64)
    n = plens.size
    poffs = np.cumsum(plens) - plens
    blob = oracle.fill_splitmix64(int(plens.sum()), 5)
    views = [blob[o:o + l] for o, l in zip(poffs.tolist(), plens.tolist())]
    for per_entry, small in ((False, REAL), (True, REAL), (True, 0)):
        ledgers, ids, lacs, lenf = vu.ids_for(n, 21, per_entry)
        keys = vu.keys_for(n, 20 if per_entry else 0, 2)
        want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys,
                                            20 if per_entry else 0, 0, small)
        if per_entry:
            reqs, digests = dg.package_batch_v2_host(DTYPE[algo], ledgers, ids, lacs, lenf, views, keys.reshape(n, 20),
                                                     small_threshold=small)
        else:
            dm = dg.DigestManager.instantiate(int(ledgers), b"", DTYPE[algo], True)
            reqs, digests = dm.package_batch_v2_host(ids, lacs, lenf, views, bytes(keys))
        assert [r.tobytes() for r in reqs] == want
        assert (digests == want_d).all()
    with pytest.raises(ValueError):
        dg.package_batch_v2_host(DTYPE[algo], ledgers[:2], ids, lacs, lenf, views, bytes(20))
    with pytest.raises(ValueError):
        dg.package_batch_v2_host(DTYPE[algo], ledgers, ids, lacs, lenf, views, bytes(19))
    dummy = dg.DigestManager.instantiate(1, b"", dg.DigestType.DUMMY, True)
    with pytest.raises(NotImplementedError):
        dummy.package_batch_v2_host(ids, lacs, lenf, views, bytes(20))
    with pytest.raises(NotImplementedError):
        dummy.package_batch_v2(ids, lacs, lenf, None, None, None, bytes(20))


def test_argument_errors_and_empty_batch():
    plens = np.array([5, 0], dtype=np.int64)
    blob = oracle.fill_splitmix64(16, 1)
    views = [blob[:5], blob[5:5]]
    ledgers, ids, lacs, lenf = vu.ids_for(2, 1, True)
    keys = vu.keys_for(2, 24, 1)

    def call(algo=ck.CRC32C, key_stride=24, flags=0, n_views=views, bufs=None):
        bufs = bufs or vu.sentinel_buffers(ck.CRC32C, plens)
        rc, _ = vu.package_v2_host_raw(algo, 0, ledgers, ids, lacs, lenf, n_views, keys, key_stride, flags, 256, bufs)
        return rc, bufs

    assert call()[0] == 0
    for kw in ({"algo": 2}, {"key_stride": 19}, {"key_stride": 1}, {"flags": 0x10000}):
        rc, bufs = call(**kw)
        assert rc == INVALID_ARG, kw
        assert all((b == vu.SENTINEL).all() for b in bufs), kw
    L, vp = _native.lib(), ctypes.c_void_p
    good = dict(ids=vp(ids.ctypes.data), lacs=vp(lacs.ctypes.data), lenf=vp(lenf.ctypes.data), keys=vp(keys.ctypes.data))
    bufs = vu.sentinel_buffers(ck.CRC32C, plens)
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    lens = plens.astype(np.uint32)
    rptr = np.array([b.ctypes.data for b in bufs], dtype=np.uint64)
    dig = np.zeros(2, dtype=np.uint32)
    for null in ("ids", "lacs", "lenf", "keys", "payloads", "lens", "requests", "digests"):
        a = dict(good, payloads=vp(ptrs.ctypes.data), lens=vp(lens.ctypes.data), requests=vp(rptr.ctypes.data),
                 digests=vp(dig.ctypes.data))
        a[null] = vp(0)
        rc = L.bkd_digest_package_batch_v2_host(ck.CRC32C, 9, vp(0), a["ids"], a["lacs"], a["lenf"], a["payloads"],
                                                a["lens"], 2, a["keys"], 24, 0, 256, a["requests"], a["digests"])
        assert rc == INVALID_ARG, null
    rptr[1] = 0  # one null request buffer
    rc = L.bkd_digest_package_batch_v2_host(ck.CRC32C, 9, vp(0), good["ids"], good["lacs"], good["lenf"],
                                            vp(ptrs.ctypes.data), vp(lens.ctypes.data), 2, good["keys"], 24, 0, 256,
                                            vp(rptr.ctypes.data), vp(dig.ctypes.data))
    assert rc == INVALID_ARG
    # n == 0: nothing is read or written, whatever the pointers
    assert L.bkd_digest_package_batch_v2_host(ck.CRC32C, 9, vp(0), vp(0), vp(0), vp(0), vp(0), vp(0), 0, vp(0), 0, 0,
                                              256, vp(0), vp(0)) == 0
    dm = dg.DigestManager.instantiate(9, b"", dg.DigestType.CRC32C, True)
    reqs, digests = dm.package_batch_v2_host([], [], [], [], bytes(20))
    assert reqs == [] and digests.size == 0
    # the device form's argument checks come before any device work
    assert L.bkd_digest_package_batch_v2(ck.CRC32C, 9, vp(0), vp(8), vp(8), vp(8), vp(8), 0, vp(8), vp(8), 1, vp(8), 19,
                                         0, 256, vp(8), 0, vp(8), vp(8), vp(0)) == INVALID_ARG
    assert L.bkd_digest_package_batch_v2(ck.CRC32C, 9, vp(0), vp(8), vp(8), vp(8), vp(8), 0, vp(8), vp(8), 1, vp(8), 0,
                                         0x10000, 256, vp(8), 0, vp(8), vp(8), vp(0)) == INVALID_ARG
    assert L.bkd_digest_package_batch_v2(ck.CRC32C, 9, vp(0), vp(0), vp(0), vp(0), vp(0), 0, vp(0), vp(0), 0, vp(0), 0,
                                         0, 256, vp(0), 0, vp(0), vp(0), vp(0)) == 0
