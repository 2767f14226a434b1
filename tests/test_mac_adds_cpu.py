"""MAC adds on the CPU: the host forms of package_batch_segments_mac and package_batch_v2_mac on the CPU
route against Python's hmac, their argument checks, the capped segment sum, and the segment walker the
device kernel shares with the host under a sanitizer. No device needed."""
import ctypes
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mac_adds_util as ma
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bookkeeper_amd", "csrc")
INVALID = -1  # BKD_ERR_INVALID_ARG


@functools.lru_cache(maxsize=None)
def table():
    """The key table of ma.PASSWORDS. Made on first use, not at import: collecting this module must not
    load the library (the GPU suite imports torch before it does)."""
    return dg.mac_key_table(ma.PASSWORDS)


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def package(b: ma.Batch, stride=None, rows=True, ledgers=True, ledger_id=0):
    return dg.package_batch_segments_mac_host(table(), np.array(b.rows, dtype=np.uint32) if rows else None,
                                              b.lids if ledgers else None, b.eids, b.lacs, b.lfs, b.host_payloads(),
                                              frame_stride=stride, ledger_id=ledger_id)


# ---- composite payloads ----

@pytest.mark.parametrize("make", [ma.cut_sweep, ma.three_segments, ma.tiny_segments, ma.shared_and_edges,
                                  ma.long_entries], ids=lambda f: f.__name__)
def test_segments_match_hmac(make):
    b = make()
    frames, macs = package(b)
    assert frames.shape == (b.n, 52) and mu.wrong_rows(frames, b.expected()) == []
    assert (macs == frames[:, 32:]).all()


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_batch_sizes_and_strides(n):
    b = ma.mixed(n)
    frames, _ = package(b, stride=64)
    assert frames.shape == (n, 64) and mu.wrong_rows(frames[:, :52], b.expected()) == []
    assert not frames[:, 52:].any()


def test_equals_the_contiguous_call_and_null_indices():
    b = ma.mixed(40, seed=41)
    frames, _ = package(b)
    joined = [np.concatenate(p) if p else np.zeros(0, dtype=np.uint8) for p in b.host_payloads()]
    flat, _ = dg.package_batch_ledgers_mac_host(table(), np.array(b.rows, dtype=np.uint32), b.lids, b.eids, b.lacs, b.lfs,
                                                joined)
    assert (frames == flat).all()
    # a null key_of is row 0 for all, null ledger_ids is ledger_id for all
    b.rows = [0] * b.n
    b.lids = [mu.LEDGER] * b.n
    frames, _ = package(b, rows=False, ledgers=False, ledger_id=mu.LEDGER)
    assert mu.wrong_rows(frames, b.expected()) == []


def test_empty_batches():
    frames, macs = dg.package_batch_segments_mac_host(table(), [], [], [], [], [], [])
    assert frames.shape == (0, 52) and macs.shape == (0, 20)
    b = ma.Batch()
    for _ in range(3):
        b.entry([])  # nseg == 0 with n > 0
    frames, _ = package(b)
    assert mu.wrong_rows(frames, b.expected()) == []


def test_wide_ids_and_two_passwords():
    w = mu.wide_ids()
    for led in mu.WIDE_LEDGERS:
        b = ma.Batch()
        for r, p in enumerate(w["payloads"]):
            b.pieces(p, [len(p) // 3], row=r % 2, ids=(led, int(w["ids"][r]), int(w["lacs"][r]), int(w["lfs"][r])))
        frames, _ = package(b)
        assert mu.wrong_rows(frames, b.expected()) == []
    # byte-identical payloads under two passwords
    b = ma.Batch()
    seg = b.put(ma.payload_bytes(100, 3))
    i, j = b.entry([seg], row=0, ids=(1, 2, 3, 4)), b.entry([seg], row=1, ids=(1, 2, 3, 4))
    frames, macs = package(b)
    assert mu.wrong_rows(frames, b.expected()) == [] and (macs[i] != macs[j]).any()


def test_over_the_cap_takes_the_cpu_route():
    """8 MiB + 1 and 8 MiB: over BKD_MAC_MAX_ENTRY, which only bounds a GPU lane; the CPU route hashes it."""
    b = ma.Batch()
    big = b.put(bytes(8 << 20) + b"\x01")
    b.entry([big, (big[0], 8 << 20)])
    frames, _ = package(b)
    assert mu.wrong_rows(frames, b.expected()) == []


# ---- the capped sum ----

def capped(lengths, cap=ma.CAP):
    arr = np.array(lengths, dtype=np.uint32)
    out = ctypes.c_uint64(0)
    over = _native.lib().bkd_host_segments_length_capped(ctypes.c_void_p(arr.ctypes.data), arr.size, cap, ctypes.byref(out))
    return over, out.value


def test_capped_segment_sum():
    cap = ma.CAP
    assert capped([]) == (0, 0)
    assert capped([cap - 1]) == (0, cap - 1) and capped([cap // 2, cap // 2 - 1]) == (0, cap - 1)
    assert capped([cap]) == (0, cap) and capped([cap // 2, 0, cap // 2]) == (0, cap)
    assert capped([cap + 1])[0] == 1 and capped([cap // 2, cap // 2, 1]) == (1, cap + 1)
    # 257 listings of one 16 MiB segment: 2^32 + 2^24 bytes, which a 32-bit sum would call 16 MiB; the sum
    # stops at the second listing
    assert capped([cap] * 257) == (1, 2 * cap)
    assert capped([2**31, 2**31]) == (1, 2**31)  # two segments of 2^31: a 32-bit sum would call it empty
    assert capped([2**32 - 1] * 5, cap=2**40) == (0, 5 * (2**32 - 1))  # 64-bit


# ---- argument checks: nothing is written ----

def raw_segments_call(first, key_of, nkeys=3, stride=52, nseg=None, frames=None):
    L = _native.lib()
    vp = ctypes.c_void_p
    segs = [np.frombuffer(b"abcdefgh", dtype=np.uint8), np.frombuffer(b"xyz", dtype=np.uint8)]
    ptrs = np.array([s.ctypes.data for s in segs], dtype=np.uint64)
    lens = np.array([8, 3], dtype=np.uint32)
    first = np.array(first, dtype=np.uint64)
    n = first.size - 1
    ids = np.arange(n, dtype=np.int64)
    key_of = np.array(key_of, dtype=np.uint32)
    frames = np.full(n * 4200, 0xEE, dtype=np.uint8) if frames is None else frames
    rc = L.bkd_digest_package_batch_segments_mac_host(
        vp(table().ctypes.data), nkeys, vp(key_of.ctypes.data), 5, None, vp(ids.ctypes.data), vp(ids.ctypes.data),
        vp(ids.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), 2 if nseg is None else nseg,
        vp(first.ctypes.data), n, vp(frames.ctypes.data), stride)
    return rc, frames


def test_segments_argument_checks_write_nothing():
    rc, frames = raw_segments_call([0, 1, 2], [0, 1])
    assert rc == 0 and (frames[:104] != 0xEE).any()
    bad_csrs = {"first not zero": [1, 1, 2], "decreasing": [0, 2, 1, 2], "ends short of nseg": [0, 1, 1],
                "ends past nseg": [0, 1, 3]}
    for name, first in bad_csrs.items():
        rc, frames = raw_segments_call(first, [0] * (len(first) - 1))
        assert rc == INVALID and (frames == 0xEE).all(), name
    for rows in ([0, 3], [0xFFFFFFFF, 0]):
        rc, frames = raw_segments_call([0, 1, 2], rows)
        assert rc == INVALID and (frames == 0xEE).all()
    for stride in (51, 4097):
        rc, frames = raw_segments_call([0, 1, 2], [0, 1], stride=stride)
        assert rc == INVALID and (frames == 0xEE).all()


def raw_v2_call(key_of=(0, 1), key_stride=20, flags=0):
    L = _native.lib()
    vp = ctypes.c_void_p
    ps = [np.frombuffer(b"abcdefgh", dtype=np.uint8), np.frombuffer(b"xyz", dtype=np.uint8)]
    ptrs = np.array([s.ctypes.data for s in ps], dtype=np.uint64)
    lens = np.array([8, 3], dtype=np.uint32)
    ids = np.arange(2, dtype=np.int64)
    key_of = np.array(key_of, dtype=np.uint32)
    master = np.zeros(64, dtype=np.uint8)
    out = np.full(2 * 128, 0xEE, dtype=np.uint8)
    rptr = np.array([out.ctypes.data, out.ctypes.data + 128], dtype=np.uint64)
    rc = L.bkd_digest_package_batch_v2_mac_host(
        vp(table().ctypes.data), 3, vp(key_of.ctypes.data), 5, None, vp(ids.ctypes.data), vp(ids.ctypes.data),
        vp(ids.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), 2, vp(master.ctypes.data), key_stride, flags,
        16384, vp(rptr.ctypes.data))
    return rc, out


def test_v2_argument_checks_write_nothing():
    rc, out = raw_v2_call()
    assert rc == 0 and (out[:88] != 0xEE).any() and (out[88:128] == 0xEE).all()
    for kw in (dict(key_stride=1), dict(key_stride=19), dict(flags=1 << 16), dict(key_of=(0, 3)),
               dict(key_of=(0xFFFFFFFF, 0))):
        rc, out = raw_v2_call(**kw)
        assert rc == INVALID and (out == 0xEE).all(), kw


# ---- V2 add requests ----

V2_LENGTHS = list(range(0, 201)) + [4096]


@pytest.mark.parametrize("small,key_stride,flags", [(dg.SMALL_ENTRY_SIZE_THRESHOLD, None, 0), (100, 24, 0xFFFF),
                                                    (0, 20, 0)])
def test_v2_requests_match_hmac(small, key_stride, flags):
    lens = V2_LENGTHS + ([99, 100, 101] if small == 100 else [16383, 16384, 16385])
    ps = mu.payloads(lens, seed=60)
    n = len(ps)
    rows, lids, eids, lacs, lfs = ma.ids_for(n)
    if key_stride is None:
        master, masters = ma.MASTER, [ma.MASTER] * n
    else:
        master = np.random.default_rng(61).integers(0, 256, (n, key_stride), dtype=np.uint8)
        masters = [master[i, :20].tobytes() for i in range(n)]
    reqs, macs = dg.package_batch_v2_mac_host(table(), rows, lids, eids, lacs, lfs, ps, master, flags=flags,
                                              small_threshold=small)
    want = ma.v2_expected(ps, rows, lids, eids, lacs, lfs, masters, flags, small)
    assert [r.tobytes() for r in reqs] == want
    assert all(macs[i].tobytes() == want[i][60:80] for i in range(n))
    assert len(want[99]) == (80 + 99 if small else 80)


def test_v2_request_sizes():
    lens = np.array([0, 99, 100, 16383, 16384], dtype=np.uint32)
    assert dg.request_sizes_v2_mac(lens).tolist() == [80, 179, 180, 80 + 16383, 80]
    assert dg.request_sizes_v2_mac(lens, 100).tolist() == [80, 179, 80, 80, 80]


# ---- the manager's methods stay unbuilt; _algo_of has no MAC ----

def test_manager_methods_still_raise():
    m = dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)
    for name in ("package_batch_segments", "package_batch_segments_host", "package_batch_v2", "package_batch_v2_host"):
        with pytest.raises(NotImplementedError, match="MAC.*package_batch_segments_mac"):
            getattr(m, name)()
    with pytest.raises(ValueError):
        dg._algo_of(dg.DigestType.HMAC)


# ---- a process without a device ----

CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import mac_adds_util as ma, mac_util as mu
from bookkeeper_amd import _native, digest as dg
assert _native.device_count() == 0
table = dg.mac_key_table(ma.PASSWORDS)
b = ma.mixed(20)
frames, _ = dg.package_batch_segments_mac_host(table, np.array(b.rows, dtype=np.uint32), b.lids, b.eids, b.lacs, b.lfs,
                                               b.host_payloads())
assert mu.wrong_rows(frames, b.expected()) == []
ps = mu.payloads([0, 5, 300], seed=1)
rows, lids, eids, lacs, lfs = ma.ids_for(3)
reqs, _ = dg.package_batch_v2_mac_host(table, rows, lids, eids, lacs, lfs, ps, ma.MASTER)
assert [r.tobytes() for r in reqs] == ma.v2_expected(ps, rows, lids, eids, lacs, lfs, [ma.MASTER] * 3, 0, 16384)
print("served")
"""


def test_host_forms_serve_without_a_device():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, "-c", CHILD % (os.path.dirname(here), here)], capture_output=True, text=True,
                         env=env)
    assert run.returncode == 0 and run.stdout.strip() == "served", run.stderr[-2000:]


# ---- the shared walker under a sanitizer: a stand-alone program, nothing loaded into Python ----

def test_segment_walker_under_address_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = str(tmp_path / "mac_adds_sanitize")
    here = os.path.dirname(os.path.abspath(__file__))
    srcs = [os.path.join(here, "mac_adds_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                               ("host_mac.cpp", "host_batch.cpp", "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-300:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert lines[-1] == "batch ok" and len(lines) == 141 * 142 // 2 + 2
    key = mu.mac_key(b"testPasswd")
    for line in lines[:-2]:
        tag, length, cut, mac = line.split()
        length, cut = int(length), int(cut)
        data = bytes((k * 131 + length * 7) & 0xFF for k in range(length))
        assert tag == "cut" and mac == mu.mac_of(mu.header(length, cut, -1, length) + data, key).hex(), (length, cut)
    data = bytes((k * 131 + 70 * 7) & 0xFF for k in range(70))
    assert lines[-2] == "leaves " + mu.mac_of(mu.header(7, 8, 9, 70) + data, key).hex()
