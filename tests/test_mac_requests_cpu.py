"""CPU: the MAC calls that span ledgers, through the CPU route of their host forms, against Python's hmac;
argument checks; a process without a device; and the two new host functions under AddressSanitizer in a
stand-alone program. No GPU compute here."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mac_requests_util as mq
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd.build import CSRC

INVALID_ARG = -1
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def run_host(b, frames=None):
    table = dg.mac_key_table(b.passwords())
    status, prefix = dg.verify_requests_mac_host(table, b.req_keys, b.frames if frames is None else frames, b.first,
                                                 b.lids, b.firsts, b.flags)
    return status, prefix.astype(np.int64)


def test_mac_key_table():
    pws = [b"", b"a", mu.PASSWD, bytes(range(200))]
    table = dg.mac_key_table(pws)
    assert table.shape == (4, 10) and table.dtype == np.uint32
    for k, pw in enumerate(pws):
        assert (table[k] == mu.key_state_of(mu.mac_key(pw))).all(), k
    assert dg.mac_key_table([]).shape == (0, 10)


@pytest.mark.parametrize("shape", list(mq.CSR_SHAPES))
def test_csr_shapes_verify(shape):
    b = mq.Requests(mq.CSR_SHAPES[shape], seed=3)
    status, prefix = run_host(b)
    assert (status == 0).all() and prefix.tolist() == b.sizes
    if b.n == 0:
        return
    # the same frames under the wrong ledger, entry id and key, one request at a time
    r = max(range(b.nreq), key=lambda q: b.sizes[q])
    for field, shift, code in (("lids", 1 << 32, 3), ("firsts", 1 << 32, 4)):
        getattr(b, field)[r] += shift
        want, want_prefix = b.expected()
        assert set(want[b.first[r]:b.first[r + 1]].tolist()) == {code}
        status, prefix = run_host(b)
        assert (status == want).all() and (prefix == want_prefix).all(), (shape, field)
        getattr(b, field)[r] -= shift


@pytest.mark.parametrize("shape", list(mq.CSR_SHAPES))
def test_csr_shapes_package(shape):
    """Entry i of request r is framed for the request's ledger with the request's key row."""
    b = mq.Requests(mq.CSR_SHAPES[shape], seed=4)
    key_of = np.repeat(b.req_keys, b.sizes)
    lids = np.repeat(b.lids, b.sizes)
    ids = np.array([mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]) for i in range(b.n)], dtype=np.int64)
    frames, macs = dg.package_batch_ledgers_mac_host(dg.mac_key_table(b.passwords()), key_of, lids, ids, ids - 1,
                                                     [len(p) for p in b.payloads], b.payloads)
    assert frames.shape == (b.n, 52) and macs.shape == (b.n, 20)
    assert mu.wrong_rows(frames, [f[:52] for f in b.frames]) == [] if b.n else True
    assert (macs == frames[:, 32:]).all()


def test_key_is_per_request():
    """Two requests over byte-identical payloads under different passwords; then both under one row."""
    lens = [0, 1, 63, 64, 200] * 2
    b = mq.Requests([5, 5], lengths=lens, seed=5)
    b.payloads[5:] = b.payloads[:5]
    b.lids[1], b.firsts[1] = b.lids[0], b.firsts[0]
    b.frames[5:] = [mu.frame(mq.first_entry(0) + j, b.payloads[j], ledger=mq.ledger(0), key=mq.key(1)) for j in range(5)]
    assert all(x[:32] == y[:32] and x[52:] == y[52:] and x[32:52] != y[32:52] for x, y in zip(b.frames[:5], b.frames[5:]))
    status, prefix = run_host(b)
    assert (status == 0).all() and prefix.tolist() == [5, 5]
    b.req_keys[:] = [1, 0]
    status, prefix = run_host(b)
    assert (status == 2).all() and prefix.tolist() == [0, 0]
    b.req_keys[:] = [0, 0]
    status, prefix = run_host(b, b.frames[:5] * 2)
    assert (status == 0).all() and prefix.tolist() == [5, 5]


@pytest.mark.parametrize("skip", [0, 1])
def test_failure_kinds_inside_a_request(skip):
    """mac_util.failure_frames() as request 2 of 4; its neighbours stay untouched."""
    bad, want, want_skip = mu.failure_frames()
    b = mq.Requests([6, 0, len(bad), 7], seed=6, keys=[1, 2, 0, 3])
    assert mq.key(0) != mu.mac_key()
    lo = int(b.first[2])
    # failure_frames() are keyed with mac_util's password: row 0 gets that key instead of password(0)
    table = dg.mac_key_table([mu.PASSWD] + b.passwords()[1:])
    b.frames[lo:lo + len(bad)] = bad
    b.lids[2], b.firsts[2], b.flags[2] = mu.LEDGER, mu.FIRST_ENTRY, skip
    status, prefix = dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts, b.flags)
    exp = want_skip if skip else want
    assert status[lo:lo + len(bad)].tolist() == exp.tolist()
    assert (status[:lo] == 0).all() and (status[lo + len(bad):] == 0).all()
    assert prefix.tolist() == [6, 0, mu.first_bad(exp), 7] and mu.first_bad(exp) == 1
    # the skip flag is the request's own: its neighbour with entry ids off by one still fails on them
    b.firsts[3] += 1
    b.flags[3] = 0
    status, prefix = dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts, b.flags)
    assert (status[int(b.first[3]):] == 4).all() and prefix.tolist()[2:] == [1, 0]
    b.flags[3] = 1
    status, prefix = dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts, b.flags)
    assert (status[int(b.first[3]):] == 0).all() and prefix.tolist()[2:] == [1, 7]


@pytest.mark.parametrize("ledger", mu.WIDE_LEDGERS)
def test_wide_ids(ledger):
    """mac_util.wide_verify_cases: ids that differ in the high word only, one case per request."""
    cases = mu.wide_verify_cases(ledger)
    frames = [f for _, fr, _, _ in cases for f in fr]
    sizes = [len(fr) for _, fr, _, _ in cases]
    table = dg.mac_key_table([b"unused", mu.PASSWD])
    status, prefix = dg.verify_requests_mac_host(table, [1] * len(cases), frames, np.concatenate(([0], np.cumsum(sizes))),
                                                 [ledger] * len(cases), [c[2] for c in cases])
    want = [s for c in cases for s in c[3]]
    assert status.tolist() == want
    assert prefix.tolist() == [mu.first_bad(c[3]) for c in cases]


def test_package_ledgers_wide_fields_and_strides():
    ps = mu.payloads([(37 * r) % 211 for r in range(28)], seed=33)
    f = mq.package_fields(len(ps), nkeys=5)
    heads = mq.package_heads(f, ps)
    table = dg.mac_key_table([mq.password(k) for k in range(5)])
    for stride in (None, 64, 4096):
        frames, macs = dg.package_batch_ledgers_mac_host(table, f["key_of"], f["lids"], f["ids"], f["lacs"], f["lfs"], ps,
                                                         frame_stride=stride)
        assert frames.shape == (len(ps), stride or 52)
        assert mu.wrong_rows(frames[:, :52], heads) == [] and not frames[:, 52:].any()
        assert (macs == frames[:, 32:52]).all()
    # the same payload under two rows: two MACs
    frames, macs = dg.package_batch_ledgers_mac_host(table, [0, 1], [9, 9], [1, 1], [0, 0], [3, 3], [b"abc", b"abc"])
    assert frames[0, :32].tobytes() == frames[1, :32].tobytes() and macs[0].tobytes() != macs[1].tobytes()
    assert macs[1].tobytes() == mu.mac_of(mu.header(9, 1, 0, 3) + b"abc", mq.key(1))


# ---- argument checks: the raw C calls ----

def _raw_verify(b, table, req_keys, nkeys=None, first=None, nreq=None, null=()):
    """bkd_digest_verify_requests_mac_host over b's frames: (rc, status, req_first_bad), the outputs prefilled."""
    views, ptrs, lens = mu.host_pointers(b.frames)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    req_keys = np.ascontiguousarray(req_keys, dtype=np.uint32)
    first = np.ascontiguousarray(b.first if first is None else first, dtype=np.uint64)
    lids, firsts = b.lids.astype(np.int64), b.firsts.astype(np.int64)
    flags = b.flags.astype(np.uint32)
    status = np.full(max(b.n, 1), -7, dtype=np.int32)
    fb = np.full(max(b.nreq, 1), 0xA5A5, dtype=np.uint64)
    arg = lambda name, a: None if name in null else vp(a.ctypes.data)
    rc = _native.lib().bkd_digest_verify_requests_mac_host(
        arg("table", table), table.size // 10 if nkeys is None else nkeys, arg("req_keys", req_keys), arg("frames", ptrs),
        arg("lengths", lens), b.n, arg("first", first), b.nreq if nreq is None else nreq, arg("ledgers", lids),
        arg("firsts", firsts), arg("flags", flags), arg("status", status), arg("first_bad", fb))
    del views
    return rc, status, fb


def test_verify_argument_checks():
    b = mq.Requests([4, 0, 6], seed=8)
    table = dg.mac_key_table(b.passwords())
    rc, st, fb = _raw_verify(b, table, b.req_keys)
    assert rc == 0 and (st == 0).all() and fb.tolist() == [4, 0, 6]
    for name in ("table", "req_keys", "frames", "lengths", "first", "ledgers", "firsts", "flags", "status", "first_bad"):
        assert _raw_verify(b, table, b.req_keys, null=(name,))[0] == INVALID_ARG, name
    assert _raw_verify(b, table, b.req_keys, nreq=0)[0] == INVALID_ARG  # entries without a request
    assert _raw_verify(b, table, b.req_keys, nreq=2**31)[0] == INVALID_ARG
    # a key index >= nkeys, on an empty request too: refused before any work, nothing written
    for keys in ([0, 1, 3], [0, 3, 2], [0xFFFFFFFF, 1, 2]):
        rc, st, fb = _raw_verify(b, table, keys)
        assert rc == INVALID_ARG and (st == -7).all() and (fb == 0xA5A5).all(), keys
        assert "key" in _native.last_error()
    assert _raw_verify(b, table, b.req_keys, nkeys=2)[0] == INVALID_ARG
    for first in ([1, 4, 4, 10], [0, 5, 4, 10], [0, 4, 4, 9], [0, 4, 4, 11], [0, 4, 12, 10]):
        rc, st, fb = _raw_verify(b, table, b.req_keys, first=first)
        assert rc == INVALID_ARG and (st == -7).all() and (fb == 0xA5A5).all(), first
        assert "req_first" in _native.last_error()
    # no entries: every request's prefix is zero; no requests and no entries: nothing to do
    e = mq.Requests([0, 0], seed=8)
    rc, st, fb = _raw_verify(e, table, [0, 1], null=("frames", "lengths", "status"))
    assert rc == 0 and fb.tolist() == [0, 0]
    assert _raw_verify(mq.Requests([], seed=8), table, [], null=("req_keys", "ledgers", "firsts", "flags"))[0] == 0
    with pytest.raises(ValueError):
        dg.verify_requests_mac_host(table, [0, 1], b.frames, b.first, b.lids, b.firsts)  # one key per request
    with pytest.raises(ValueError):
        dg.verify_requests_mac_host(table.reshape(-1)[:-1], b.req_keys, b.frames, b.first, b.lids, b.firsts)


def test_package_argument_checks():
    L = _native.lib()
    table = dg.mac_key_table([b"a", b"b"])
    a8 = np.arange(3, dtype=np.int64)
    views, ptrs, lens = mu.host_pointers([b"x", b"", b"yz"])

    def call(key_of, stride=52, null=(), n=3, nkeys=2):
        key_of = np.ascontiguousarray(key_of, dtype=np.uint32)
        out = np.full((3, 64), 0xA5, dtype=np.uint8)
        arg = lambda name, a: None if name in null else vp(a.ctypes.data)
        rc = L.bkd_digest_package_batch_ledgers_mac_host(
            arg("table", table), nkeys, arg("key_of", key_of), arg("ledgers", a8), arg("ids", a8), arg("lacs", a8),
            arg("lfs", a8), arg("payloads", ptrs), arg("lengths", lens), n, arg("frames", out), stride)
        return rc, out

    rc, out = call([0, 1, 1], stride=64)
    assert rc == 0 and (out[:, 52:] == 0xA5).all()
    for i, (p, k) in enumerate(zip([b"x", b"", b"yz"], [0, 1, 1])):
        hdr = mu.header(i, i, i, i)
        assert out[i, :52].tobytes() == hdr + mu.mac_of(hdr + p, mu.mac_key(b"ab"[k:k + 1]))
    for name in ("table", "key_of", "ledgers", "ids", "lacs", "lfs", "payloads", "lengths", "frames"):
        assert call([0, 1, 1], null=(name,))[0] == INVALID_ARG, name
    for stride in (51, 4097):
        assert call([0, 1, 1], stride=stride)[0] == INVALID_ARG
    for key_of in ([0, 2, 1], [0, 1, 0xFFFFFFFF]):  # a key index >= nkeys: no frame is written
        rc, out = call(key_of)
        assert rc == INVALID_ARG and (out == 0xA5).all()
    assert call([0, 0, 0], nkeys=0)[0] == INVALID_ARG
    assert call([0, 1, 1], n=0, null=("table", "key_of", "ledgers", "ids", "lacs", "lfs", "payloads", "lengths",
                                      "frames"))[0] == 0
    with pytest.raises(ValueError):
        dg.package_batch_ledgers_mac_host(table, [0], [1, 2], [1, 2], [0, 0], [1, 1], [b"x", b"y"])
    del views


def test_manager_methods_and_algo_of_are_untouched():
    m = dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)
    with pytest.raises(NotImplementedError, match="MAC"):
        m.package_batch_v2()
    with pytest.raises(ValueError):
        dg.verify_requests_host(dg.DigestType.HMAC, [], [0], [], [])


# ---- no device ----

_NO_DEVICE_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import mac_requests_util as mq
import mac_util as mu
from bookkeeper_amd import _native, checksum as ck, digest as dg
assert _native.device_count() == 0
b = mq.Requests([3, 0, 4], seed=9)
table = dg.mac_key_table(b.passwords())
b.frames[5] = b.frames[5][:-1] + bytes([b.frames[5][-1] ^ 1])
want, want_prefix = b.expected()
st, fb = dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts)  # automatic: the CPU route
assert (st == want).all() and (fb.astype(np.int64) == want_prefix).all() and want.tolist() == [0, 0, 0, 0, 0, 2, 0]
frames, macs = dg.package_batch_ledgers_mac_host(table, [0, 2], [5, 6], [1, 2], [0, 1], [3, 0], [b"abc", b""])
assert frames[0].tobytes() == mu.frame(1, b"abc", ledger=5, lac=0, key=mq.key(0))[:52]
assert frames[1].tobytes() == mu.frame(2, b"", ledger=6, lac=1, key=mq.key(2))[:52]
with ck.host_batch_route(ck.HOST_ROUTE_GPU):
    for call in (lambda: dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts),
                 lambda: dg.package_batch_ledgers_mac_host(table, [0], [5], [1], [0], [3], [b"abc"])):
        try:
            call()
            raise SystemExit("the forced GPU route succeeded without a device")
        except _native.BkdError as e:
            assert e.code == -2, e  # BKD_ERR_NO_DEVICE
L, p = _native.lib(), 1 << 20  # device-resident calls are GPU work only
assert L.bkd_digest_verify_requests_mac(p, 1, p, p, 64, p, p, 1, p, 1, p, p, p, p, p, None) == -2
assert L.bkd_digest_package_batch_ledgers_mac(p, 1, p, p, p, p, p, p, 64, p, p, 1, p, 52, None) == -2
assert L.bkd_digest_package_batch_ledgers_mac(p, 1, p, p, p, p, p, p, 64, p, p, 1, p, 51, None) == -1
assert L.bkd_digest_verify_requests_mac(p, 1, p, p, 64, p, p, 1, p, 0, p, p, p, p, p, None) == -1
print("mac requests without a device")
"""


def test_mac_requests_without_a_device():
    """A fresh process with the devices hidden: the automatic route is the CPU route, the forced GPU route
    and the device-resident calls say BKD_ERR_NO_DEVICE."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "mac requests without a device" in r.stdout, r.stderr[-2000:]


# ---- the two host functions under a sanitizer: a stand-alone program, nothing loaded into Python ----

def test_host_mac_requests_under_address_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = str(tmp_path / "mac_requests_sanitize")
    here = os.path.dirname(os.path.abspath(__file__))
    srcs = [os.path.join(here, "mac_requests_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                   ("host_mac.cpp", "host_batch.cpp", "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "verify ok" and len(lines) == 22
    seen = set()
    for line in lines[:-1]:
        i, r, k, n, mac = line.split()
        i, r, k, n = int(i), int(r), int(k), int(n)
        seen.add(n)
        payload = bytes((j * 131 + n * 7 + i) & 0xFF for j in range(n))
        hdr = mu.header(1000 + r, 10 * r + i, i - 1, n)
        assert mac == mu.mac_of(hdr + payload, mu.mac_key(b"pw%d" % k)).hex(), (i, r, k, n)
    assert {0, 1, 31, 32, 33, 63, 64, 65} <= seen
