"""CPU: the MAC reframe (reframe_requests_mac_host) through the CPU route, against Python's hmac: whole
buffers compared, so a frame that is not OK must come back byte for byte; argument checks; a process without
a device; and the host walker and sha1::compress2 under AddressSanitizer in a stand-alone program. No GPU
compute here."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mac_reframe_util as mr
import mac_requests_util as mq
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd.build import CSRC

INVALID_ARG = -1
TRUSTED = 1
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def run(b, table, lacs, frames=None, trusted=False):
    """Reframes writable copies of the frames: (status, prefix int64, the buffers after the call)."""
    bufs = [bytearray(f) for f in (b.frames if frames is None else frames)]
    status, prefix = dg.reframe_requests_mac_host(table, b.req_keys, bufs, b.first, b.lids, b.firsts, lacs, b.flags,
                                                  trusted=trusted)
    return status, prefix.astype(np.int64), [bytes(x) for x in bufs]


@pytest.mark.parametrize("trusted", [False, True])
def test_length_sweep(trusted):
    """Every payload length of SWEEP: block 0 carries its padding up to 23 and spills at 24; 31/32 and 87/88
    are block edges."""
    sizes = [len(mu.SWEEP) // 2, len(mu.SWEEP) - len(mu.SWEEP) // 2]
    b = mq.Requests(sizes, lengths=mu.SWEEP, seed=41)
    lacs = [mr.lac_of(i) for i in range(b.n)]
    status, prefix, got = run(b, dg.mac_key_table(b.passwords()), lacs, trusted=trusted)
    assert (status == 0).all() and prefix.tolist() == sizes
    want = [mr.reframed(f, lacs[i], mq.key(b.req_of(i))) for i, f in enumerate(b.frames)]
    assert [i for i in range(b.n) if got[i] != want[i]] == []


@pytest.mark.parametrize("skip", [0, 1])
def test_failure_kinds_default(skip):
    """Statuses and prefixes are verify_requests_mac_host's own; only status-0 frames change."""
    b, passwords, keys, lo, nbad = mr.failures(skip)
    table = dg.mac_key_table(passwords)
    v_status, v_prefix = dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids, b.firsts, b.flags)
    assert set(v_status[lo:lo + nbad].tolist()) == ({0, 1, 2, 3, 4} if not skip else {0, 1, 2, 3})
    lacs = [mr.lac_of(i) for i in range(b.n)]
    status, prefix, got = run(b, table, lacs)
    assert status.tolist() == v_status.tolist() and prefix.tolist() == v_prefix.astype(np.int64).tolist()
    for i, f in enumerate(b.frames):
        want = mr.reframed(f, lacs[i], keys[i]) if status[i] == 0 else bytes(f)
        assert got[i] == want, i


@pytest.mark.parametrize("skip", [0, 1])
def test_failure_kinds_trusted(skip):
    """Trusted: 1 if shorter than 52 bytes, else what the ids decide; never 2. A frame whose bytes were
    damaged comes back with a MAC that verifies."""
    b, passwords, keys, lo, nbad = mr.failures(skip)
    table = dg.mac_key_table(passwords)
    lacs = [mr.lac_of(i) for i in range(b.n)]
    status, prefix, got = run(b, table, lacs, trusted=True)
    want_status = mr.header_status(b, b.frames).tolist()
    assert status.tolist() == want_status and 2 not in want_status
    flipped_and_foreign, damaged = mr.damaged_frames()
    assert status[lo + flipped_and_foreign] == 3
    assert prefix.tolist() == [6, 0, mu.first_bad(want_status[lo:lo + nbad]), 7]
    for i, f in enumerate(b.frames):
        want = mr.reframed(f, lacs[i], keys[i]) if status[i] == 0 else bytes(f)
        assert got[i] == want, i
    # frames of the right ledger with a flipped header, MAC or payload byte: trusted gives each a MAC that verifies
    for i in damaged:
        assert status[lo + i] == 0
        assert mq.ref_status(got[lo + i], mu.mac_key(), mu.LEDGER, mu.FIRST_ENTRY + i, False) == 0, i


@pytest.mark.parametrize("trusted", [False, True])
def test_wide_lacs_and_equal_lac(trusted):
    ps = mu.payloads([0, 5, 23, 24, 100, 64, 31, 32], seed=42)
    b = mq.Requests([3, 5], lengths=[len(p) for p in ps], seed=42)
    table = dg.mac_key_table(b.passwords())
    for lac in mu.WIDE_LACS:
        status, _, got = run(b, table, [lac] * b.n, trusted=trusted)
        assert (status == 0).all()
        assert got == [mr.reframed(f, lac, mq.key(b.req_of(i))) for i, f in enumerate(b.frames)], lac
    # a new LAC equal to the old one (frame() writes entry id - 1): the frame comes back identical
    old = [int.from_bytes(f[16:24], "big", signed=True) for f in b.frames]
    status, _, got = run(b, table, old, trusted=trusted)
    assert (status == 0).all() and got == [bytes(f) for f in b.frames]


@pytest.mark.parametrize("ledger", mu.WIDE_LEDGERS)
def test_wide_ids(ledger):
    cases = mu.wide_verify_cases(ledger)
    frames = [f for _, fr, _, _ in cases for f in fr]
    sizes = [len(fr) for _, fr, _, _ in cases]
    table = dg.mac_key_table([b"unused", mu.PASSWD])
    lacs = [mr.lac_of(i) for i in range(len(frames))]
    bufs = [bytearray(f) for f in frames]
    status, prefix = dg.reframe_requests_mac_host(table, [1] * len(cases), bufs, np.concatenate(([0], np.cumsum(sizes))),
                                                  [ledger] * len(cases), [c[2] for c in cases], lacs)
    want = [s for c in cases for s in c[3]]
    assert status.tolist() == want and prefix.tolist() == [mu.first_bad(c[3]) for c in cases]
    for i, f in enumerate(frames):
        assert bytes(bufs[i]) == (mr.reframed(f, lacs[i], mu.mac_key()) if want[i] == 0 else f), i


@pytest.mark.parametrize("trusted", [False, True])
def test_key_is_per_request(trusted):
    b = mq.Requests([5, 5], lengths=[0, 1, 63, 64, 200] * 2, seed=5)
    table = dg.mac_key_table(b.passwords())
    lacs = [mr.lac_of(i) for i in range(b.n)]
    status, prefix, got = run(b, table, lacs, trusted=trusted)
    assert (status == 0).all() and prefix.tolist() == [5, 5]
    assert got == [mr.reframed(f, lacs[i], mq.key(i // 5)) for i, f in enumerate(b.frames)]
    if trusted:
        return
    b.req_keys[:] = [1, 0]  # the rows swapped: every status is 2 and no byte changes
    status, prefix, got = run(b, table, lacs)
    assert (status == 2).all() and prefix.tolist() == [0, 0] and got == [bytes(f) for f in b.frames]


@pytest.mark.parametrize("shape", list(mq.CSR_SHAPES))
def test_csr_shapes(shape):
    b = mq.Requests(mq.CSR_SHAPES[shape], seed=3)
    table = dg.mac_key_table(b.passwords())
    lacs = [mr.lac_of(i) for i in range(b.n)]
    status, prefix, got = run(b, table, lacs)
    assert status.shape == (b.n,) and (status == 0).all() and prefix.tolist() == b.sizes
    assert got == [mr.reframed(f, lacs[i], mq.key(b.req_of(i))) for i, f in enumerate(b.frames)]
    if b.n == 0:
        return
    r = max(range(b.nreq), key=lambda q: b.sizes[q])
    b.lids[r] += 1 << 32
    want, want_prefix = b.expected()
    status, prefix, got = run(b, table, lacs)
    assert (status == want).all() and (prefix == want_prefix).all()
    for i, f in enumerate(b.frames):
        assert got[i] == (mr.reframed(f, lacs[i], mq.key(b.req_of(i))) if want[i] == 0 else bytes(f)), i


# ---- argument checks: the raw C call ----

def _raw(b, table, req_keys=None, flags=0, nkeys=None, first=None, nreq=None, null=()):
    """bkd_digest_reframe_requests_mac_host over copies of b's frames: (rc, status, req_first_bad, whether any
    frame changed), the outputs prefilled."""
    bufs = [bytearray(f) for f in b.frames]
    views, ptrs, lens = mu.host_pointers(bufs)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    req_keys = np.ascontiguousarray(b.req_keys if req_keys is None else req_keys, dtype=np.uint32)
    first = np.ascontiguousarray(b.first if first is None else first, dtype=np.uint64)
    lids, firsts, rflags = b.lids.astype(np.int64), b.firsts.astype(np.int64), b.flags.astype(np.uint32)
    lacs = np.arange(max(b.n, 1), dtype=np.int64) + 77
    status = np.full(max(b.n, 1), -7, dtype=np.int32)
    fb = np.full(max(b.nreq, 1), 0xA5A5, dtype=np.uint64)
    arg = lambda name, a: None if name in null else vp(a.ctypes.data)
    rc = _native.lib().bkd_digest_reframe_requests_mac_host(
        arg("table", table), table.size // 10 if nkeys is None else nkeys, arg("req_keys", req_keys), flags,
        arg("frames", ptrs), arg("lengths", lens), b.n, arg("first", first), b.nreq if nreq is None else nreq,
        arg("ledgers", lids), arg("firsts", firsts), arg("flags", rflags), arg("lacs", lacs), arg("status", status),
        arg("first_bad", fb))
    del views
    return rc, status, fb, [bytes(x) for x in bufs] != [bytes(f) for f in b.frames]


def test_argument_checks():
    b = mq.Requests([4, 0, 6], seed=8)
    table = dg.mac_key_table(b.passwords())
    rc, st, fb, changed = _raw(b, table)
    assert rc == 0 and (st == 0).all() and fb.tolist() == [4, 0, 6] and changed
    assert _raw(b, table, flags=TRUSTED)[0] == 0

    def refused(**kw):
        rc, st, fb, changed = _raw(b, table, **kw)
        return rc == INVALID_ARG and (st == -7).all() and (fb == 0xA5A5).all() and not changed

    for flags in (2, 3, 0x80000000):
        assert refused(flags=flags), flags
    for name in ("table", "req_keys", "frames", "lengths", "first", "ledgers", "firsts", "flags", "lacs", "status",
                 "first_bad"):
        assert refused(null=(name,)), name
    assert refused(nreq=0) and refused(nreq=2**31)
    for keys in ([0, 1, 3], [0, 3, 2], [0xFFFFFFFF, 1, 2]):
        assert refused(req_keys=keys), keys
    assert refused(nkeys=2)
    for first in ([1, 4, 4, 10], [0, 5, 4, 10], [0, 4, 4, 9], [0, 4, 4, 11], [0, 4, 12, 10]):
        assert refused(first=first), first
    # no entries: every request's prefix is zero; no requests and no entries: nothing to do
    e = mq.Requests([0, 0], seed=8)
    rc, st, fb, _ = _raw(e, table, req_keys=[0, 1], null=("frames", "lengths", "status", "lacs"))
    assert rc == 0 and fb.tolist() == [0, 0]
    assert _raw(mq.Requests([], seed=8), table, req_keys=[], null=("req_keys", "ledgers", "firsts", "flags"))[0] == 0
    # the device form's refusals come before it looks for a device
    L, p = _native.lib(), 1 << 20
    dev = lambda flags=0, lacs=p, out=None, stride=0, status=p: L.bkd_digest_reframe_requests_mac(
        p, 1, p, flags, p, 64, p, p, 1, p, 1, p, p, p, lacs, out, stride, status, p, None)
    assert dev(flags=2) == INVALID_ARG and dev(lacs=None) == INVALID_ARG and dev(status=None) == INVALID_ARG
    assert dev(out=p + 4096, stride=51) == INVALID_ARG and dev(out=None, stride=52) == INVALID_ARG
    assert dev(out=p + 32, stride=52) == INVALID_ARG  # out-frames overlap the framed buffer


def test_wrapper_refuses_frames_it_cannot_write():
    b = mq.Requests([2], seed=9)
    table = dg.mac_key_table(b.passwords())
    args = (b.first, b.lids, b.firsts, [1, 2])
    with pytest.raises(TypeError):
        dg.reframe_requests_mac_host(table, b.req_keys, [bytes(f) for f in b.frames], *args)
    strided = [np.frombuffer(bytearray(f) * 2, dtype=np.uint8)[::2] for f in b.frames]
    with pytest.raises(TypeError):
        dg.reframe_requests_mac_host(table, b.req_keys, strided, *args)
    with pytest.raises(ValueError):
        dg.reframe_requests_mac_host(table, b.req_keys, [bytearray(f) for f in b.frames], b.first, b.lids, b.firsts, [1])
    m = dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)
    with pytest.raises(NotImplementedError, match="MAC.*reframe_requests_mac"):
        m.reframe_batch()


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
bufs = [bytearray(f) for f in b.frames]
lacs = [50 + i for i in range(b.n)]
st, fb = dg.reframe_requests_mac_host(table, b.req_keys, bufs, b.first, b.lids, b.firsts, lacs)  # automatic: the CPU route
assert st.tolist() == [0, 0, 0, 0, 0, 2, 0] and fb.tolist() == [3, 0, 2]
for i, f in enumerate(b.frames):
    want = bytes(f) if i == 5 else mu.frame(mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]), f[52:],
                                            ledger=mq.ledger(b.req_of(i)), lac=lacs[i], key=mq.key(b.req_of(i)))
    assert bytes(bufs[i]) == want, i
with ck.host_batch_route(ck.HOST_ROUTE_GPU):
    try:
        dg.reframe_requests_mac_host(table, b.req_keys, bufs, b.first, b.lids, b.firsts, lacs)
        raise SystemExit("the forced GPU route succeeded without a device")
    except _native.BkdError as e:
        assert e.code == -2, e  # BKD_ERR_NO_DEVICE
L, p = _native.lib(), 1 << 20  # the device-resident call is GPU work only
assert L.bkd_digest_reframe_requests_mac(p, 1, p, 0, p, 64, p, p, 1, p, 1, p, p, p, p, None, 0, p, p, None) == -2
print("mac reframe without a device")
"""


def test_mac_reframe_without_a_device():
    """A fresh process with the devices hidden: the automatic route is the CPU route, the forced GPU route and
    the device-resident call say BKD_ERR_NO_DEVICE."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "mac reframe without a device" in r.stdout, r.stderr[-2000:]


# ---- the host walker and compress2 under a sanitizer: a stand-alone program, nothing loaded into Python ----

def test_host_mac_reframe_under_address_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = str(tmp_path / "mac_reframe_sanitize")
    here = os.path.dirname(os.path.abspath(__file__))
    srcs = [os.path.join(here, "mac_reframe_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                  ("host_mac.cpp", "host_batch.cpp", "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert "reframe ok" in lines and lines[-1] == "compress2 ok"
    lengths = [0, 51, 52, 53, 75, 76, 4148]
    seen = set()
    for line in (x for x in lines if x[0] in "01"):
        trusted, off, n, lac, head = line.split()
        off, n, lac = int(off), int(n), int(lac)
        i = lengths.index(n) * 4 + off
        seen.add((int(trusted), off, n))
        payload = bytes((j * 131 + n * 7 + i) & 0xFF for j in range(n - 52))
        want = mu.frame(100 + i, payload, ledger=7000 + (i & 1), lac=lac, key=mu.mac_key(b"pw%d" % (1 - (i & 1))))[:52]
        assert head == want.hex(), line[:20]
    assert seen == {(t, o, n) for t in (0, 1) for o in range(4) for n in lengths[2:]}
