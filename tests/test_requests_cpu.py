"""CPU: the host-resident batches that span many ledgers — bkd_digest_verify_requests_host and
bkd_digest_package_batch_ledgers_host on the CPU route (host_batch.cpp over the host pool) — against
the oracle (requests_util.py: empty requests, 64-bit ledger ids, an entry-id carry, skip flags, every
corruption kind placed by request), their agreement with the single-ledger calls, the CSR validation
and the argument checks. Needs no GPU; the GPU route of the same calls is in test_gpu_requests.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import requests_util as rq
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}
ALGOS = [ck.CRC32C, ck.CRC32]
INVALID_ARG = -1


@pytest.fixture(autouse=True, params=[1, 0], ids=["1-thread", "all-threads"])
def cpu_route(request):
    ck.set_host_threads(request.param)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        assert ck.get_host_batch_route() == ck.HOST_ROUTE_CPU
        yield request.param
    ck.set_host_threads(0)


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_requests_host_cpu_vs_oracle(algo):
    b = rq.ragged_batch(algo)
    st, fb = dg.verify_requests_host(DTYPE[algo], b.frame_views(), b.first, b.ledgers, b.firsts, b.flags)
    assert st.dtype == np.int32 and (st == b.want).all(), np.nonzero(st != b.want)[0][:8]
    assert (fb.astype(np.int64) == b.want_prefix).all(), (fb, b.want_prefix)
    # without the skip flags: the off-by-one entry of request 11 now fails, nothing else moves
    st2, fb2 = dg.verify_requests_host(DTYPE[algo], b.frame_views(), b.first, b.ledgers, b.firsts)
    want2 = np.array([oracle.verify_entry(algo, b.frame(i), int(b.lid[i]), int(b.ids[i]), False) for i in range(rq.N)])
    assert (want2 != b.want).sum() == 1 and (st2 == want2).all()
    assert (fb2.astype(np.int64) == rq.prefixes(want2, b.first)).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_package_batch_ledgers_host_cpu_vs_oracle(algo):
    b = rq.ragged_batch(algo)
    payloads = [b.blob[o:o + l] for o, l in zip(b.poffs.tolist(), b.plens.tolist())]
    for stride in (None, 64):
        frames, digests = dg.package_batch_ledgers_host(DTYPE[algo], b.lid, b.ids, b.lacs, b.lenf, payloads,
                                                        frame_stride=stride)
        want_d = np.array([oracle.digest_entry(algo, int(b.lid[i]), int(b.ids[i]), int(b.lacs[i]), int(b.lenf[i]),
                                               payloads[i])[0] for i in range(rq.N)], dtype=np.uint32)
        assert (digests == want_d).all()
        for i in range(rq.N):
            d, hdr = oracle.digest_entry(algo, int(b.lid[i]), int(b.ids[i]), int(b.lacs[i]), int(b.lenf[i]), payloads[i])
            assert bytes(frames[i, :b.hl]) == hdr + oracle.digest_bytes(algo, d), i
        assert not frames[:, b.hl:].any()


@pytest.mark.parametrize("algo", ALGOS)
def test_one_request_equals_the_single_ledger_calls(algo):
    """One request (one ledger id repeated): bit for bit verify_batch_host / package_batch_host."""
    b = rq.ragged_batch(algo)
    i0, i1 = int(b.first[7]), int(b.first[8])  # request 7: 257 frames, two of them corrupted
    views = b.frame_views()[i0:i1]
    ledger, first_id = rq.LEDGERS[7], rq.FIRSTS[7]
    dm = dg.DigestManager.instantiate(ledger, b"", DTYPE[algo])
    for skip in (False, True):
        st1, fb1 = dm.verify_batch_host(views, first_id, skip_entry_check=skip)
        st, fb = dg.verify_requests_host(DTYPE[algo], views, [0, i1 - i0], [ledger], [first_id], [int(skip)])
        assert (st == st1).all() and st.any() and fb.tolist() == [fb1] and fb1 == 100
    payloads = [b.blob[o:o + l] for o, l in zip(b.poffs[i0:i1].tolist(), b.plens[i0:i1].tolist())]
    f1, d1 = dm.package_batch_host(b.ids[i0:i1], b.lacs[i0:i1], b.lenf[i0:i1], payloads)
    f, d = dg.package_batch_ledgers_host(DTYPE[algo], np.full(i1 - i0, ledger), b.ids[i0:i1], b.lacs[i0:i1],
                                         b.lenf[i0:i1], payloads)
    assert (f == f1).all() and (d == d1).all() and f.any()


def _raw_verify(algo, views, first, ledgers, firsts, flags, n=None, nreq=None, null=()):
    """bkd_digest_verify_requests_host straight through ctypes: (rc, status, first_bad)."""
    vp = ctypes.c_void_p
    n = len(views) if n is None else n
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views] + [0], dtype=np.uint64)
    lens = np.array([v.size for v in views] + [0], dtype=np.uint32)
    first = np.asarray(first, dtype=np.uint64)
    nreq = first.size - 1 if nreq is None else nreq
    arr = {"first": first, "ledgers": np.asarray(ledgers, dtype=np.int64), "firsts": np.asarray(firsts, dtype=np.int64),
           "flags": np.asarray(flags, dtype=np.uint32), "status": np.full(n + 1, -7, dtype=np.int32),
           "first_bad": np.full(max(nreq, 0) + 1, 0xA5A5, dtype=np.uint64), "frames": ptrs, "lengths": lens}
    p = {k: (None if k in null else vp(a.ctypes.data)) for k, a in arr.items()}
    rc = ck.lib().bkd_digest_verify_requests_host(algo, p["frames"], p["lengths"], n, p["first"], nreq, p["ledgers"],
                                                  p["firsts"], p["flags"], p["status"], p["first_bad"])
    return rc, arr["status"], arr["first_bad"]


def test_malformed_csr_is_refused_before_any_work():
    b = rq.ragged_batch(ck.CRC32C)
    views = b.frame_views()[:10]
    ok = ([0, 4, 4, 10], [1, 2, 3], [0, 0, 0], [0, 0, 0])
    assert _raw_verify(0, views, *ok)[0] == 0
    for first in ([1, 4, 4, 10],      # does not start at 0
                  [0, 5, 4, 10],      # decreases
                  [0, 4, 4, 9],       # ends below n
                  [0, 4, 4, 11],      # ends above n
                  [0, 4, 12, 10]):    # passes n and comes back
        rc, st, fb = _raw_verify(0, views, first, *ok[1:])
        assert rc == INVALID_ARG, first
        assert (st == -7).all() and (fb == 0xA5A5).all()  # nothing was written
    assert "req_first" in ck._native.last_error()


def test_null_and_zero_size_arguments():
    b = rq.ragged_batch(ck.CRC32C)
    views = b.frame_views()[:6]
    good = ([0, 6], [rq.LEDGERS[1]], [rq.FIRSTS[1]], [0])
    for name in ("first", "ledgers", "firsts", "flags", "first_bad", "frames", "lengths", "status"):
        assert _raw_verify(0, views, *good, null=(name,))[0] == INVALID_ARG, name
    assert _raw_verify(7, views, *good)[0] == INVALID_ARG  # unknown algorithm
    assert _raw_verify(0, views, [0], [], [], [])[0] == INVALID_ARG  # entries without a request
    assert _raw_verify(0, views, [0, 6], [1], [0], [0], nreq=2**31)[0] == INVALID_ARG
    # no entries: every request empty, prefixes zero; no requests and no entries: nothing to do
    rc, st, fb = _raw_verify(0, [], [0, 0, 0], [1, 2], [0, 0], [0, 1], null=("frames", "lengths", "status"))
    assert rc == 0 and fb[:2].tolist() == [0, 0] and fb[2] == 0xA5A5
    assert _raw_verify(0, [], [0], [], [], [], null=("ledgers", "firsts", "flags", "first_bad"))[0] == 0
    # package: n == 0 is nothing; a NULL ledger id array is refused
    vp = ctypes.c_void_p
    L = ck.lib()
    assert L.bkd_digest_package_batch_ledgers_host(0, None, None, None, None, None, None, 0, None, 36, None) == 0
    a8 = np.zeros(4, dtype=np.int64)
    ptrs, lens = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    out, dig = np.zeros(64, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    args = lambda lid, stride: (0, lid, vp(a8.ctypes.data), vp(a8.ctypes.data), vp(a8.ctypes.data), vp(ptrs.ctypes.data),
                                vp(lens.ctypes.data), 1, vp(out.ctypes.data), stride, vp(dig.ctypes.data))
    assert L.bkd_digest_package_batch_ledgers_host(*args(None, 36)) == INVALID_ARG
    assert L.bkd_digest_package_batch_ledgers_host(*args(vp(a8.ctypes.data), 35)) == INVALID_ARG
    assert L.bkd_digest_package_batch_ledgers_host(*args(vp(a8.ctypes.data), 36)) == 0
    assert bytes(out[:36]) == oracle.digest_entry(0, 0, 0, 0, 0, b"")[1] + oracle.digest_bytes(0, int(dig[0]))
    with pytest.raises(ValueError):
        dg.verify_requests_host(dg.DigestType.CRC32C, views, [0, 6], [1, 2], [0])
    with pytest.raises(ValueError):
        dg.verify_requests_host(dg.DigestType.DUMMY, views, [0, 6], [1], [0])
    with pytest.raises(ValueError):
        dg.package_batch_ledgers_host(dg.DigestType.CRC32, [1], [1, 2], [0], [0], [b"x"])


_NO_DEVICE_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import requests_util as rq
from bookkeeper_amd import _native, digest as dg
assert _native.device_count() == 0
assert _native.lib().bkd_get_host_batch_route() == 1  # automatic: the CPU route
b = rq.ragged_batch(0)
st, fb = dg.verify_requests_host(dg.DigestType.CRC32C, b.frame_views(), b.first, b.ledgers, b.firsts, b.flags)
assert (st == b.want).all() and (fb.astype(np.int64) == b.want_prefix).all()
payloads = [b.blob[o:o + l] for o, l in zip(b.poffs.tolist(), b.plens.tolist())]
frames, digests = dg.package_batch_ledgers_host(dg.DigestType.CRC32C, b.lid, b.ids, b.lacs, b.lenf, payloads)
import oracle
for i in range(0, rq.N, 7):
    d, hdr = oracle.digest_entry(0, int(b.lid[i]), int(b.ids[i]), int(b.lacs[i]), int(b.lenf[i]), payloads[i])
    assert digests[i] == d and bytes(frames[i]) == hdr + oracle.digest_bytes(0, d), i
print("requests without a device")
"""


def test_requests_host_without_a_device():
    """With no device visible the automatic route is the CPU route and both calls succeed (a fresh
    process with the devices hidden, so the check also runs on a host that has one)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "requests without a device" in r.stdout, r.stderr[-2000:]
