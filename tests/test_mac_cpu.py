"""CPU: MAC ledgers (HMAC-SHA1, MacDigestManager) on the host — key setup, the per-call MAC, the CPU
route of the host-resident batches and MacDigestManager's per-entry methods, against Python's hmac /
hashlib; and host_mac.cpp under AddressSanitizer in a stand-alone program. No GPU compute here."""
import hashlib
import hmac
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd.build import CSRC

KEY = mu.mac_key()


@pytest.fixture(scope="module")
def ks():
    return ck.mac_key_init(mu.PASSWD)


@pytest.fixture(scope="module")
def mgr():
    return dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)


@pytest.fixture()
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


# ---- known answers ----

RFC2202 = [  # (key, data, HMAC-SHA1): RFC 2202 section 3
    (b"\x0b" * 20, b"Hi There", "b617318655057264e28bc0b6fb378c8ef146be00"),
    (b"Jefe", b"what do ya want for nothing?", "effcdf6ae5eb2fa2d27416d5f184df9c259a7c79"),
    (b"\xaa" * 20, b"\xdd" * 50, "125d7342b9ac11cd91a39af48aa17b4f63f175d3"),
    (bytes(range(1, 26)), b"\xcd" * 50, "4c9007f4026250c6bc8414f9bf50c86c2d7235da"),
    (b"\x0c" * 20, b"Test With Truncation", "4c1a03424b55e07fe7f27be1d58bb9324a9a5a04"),
]


@pytest.mark.parametrize("key,data,want", RFC2202, ids=["case1", "case2", "case3", "case4", "case5"])
def test_rfc2202_vectors(key, data, want):
    assert hmac.new(key, data, "sha1").hexdigest() == want  # the reference agrees with the RFC
    state = ck.mac_key_state(key)
    assert (state == mu.key_state_of(key)).all()
    assert ck.mac_cpu(state, data).hex() == want


def test_sha1_known_answers():
    assert ck.mac_gen_digest(b"", b"").hex() == "da39a3ee5e6b4b0d3255bfef95601890afd80709"
    assert ck.mac_gen_digest(b"", b"abc").hex() == "a9993e364706816aba3e25717850c26c9cd0d89d"
    assert ck.mac_gen_digest(b"ledger", b"") == hashlib.sha1(b"ledger").digest()  # EMPTY_LEDGER_KEY
    assert dg.MacDigestManager.genDigest("ledger", b"pw") == hashlib.sha1(b"ledgerpw").digest()
    for n in (55, 56, 63, 64, 119, 120, 1000):  # pad and password across block boundaries
        pw = bytes(range(256)) * 4
        assert ck.mac_gen_digest(b"mac", pw[:n]) == hashlib.sha1(b"mac" + pw[:n]).digest(), n


@pytest.mark.parametrize("n", [0, 1, 63, 64, 200])
def test_key_init_states(n):
    pw = bytes((7 * k + 1) & 0xFF for k in range(n))
    assert (ck.mac_key_init(pw) == mu.key_state_of(hashlib.sha1(b"mac" + pw).digest())).all()


def test_key_state_rejects_long_keys():
    L = _native.lib()
    out = np.zeros(10, dtype=np.uint32)
    assert L.bkd_mac_key_state(bytes(65), 65, out.ctypes.data) == -1
    assert L.bkd_mac_key_state(bytes(64), 64, out.ctypes.data) == 0
    assert (out == mu.key_state_of(bytes(64))).all()


# ---- padding boundaries: every length 0..200 and 4090..4100 through three paths ----

def test_sweep_mac_cpu(ks):
    for p in mu.payloads(mu.SWEEP):
        assert ck.mac_cpu(ks, p) == mu.mac_of(p), len(p)


def test_sweep_batch_host_cpu_route(ks, cpu_route):
    ps = mu.payloads(mu.SWEEP)
    got = ck.mac_batch_host(ks, ps)
    assert got.shape == (len(ps), 20)
    for i, p in enumerate(ps):
        assert got[i].tobytes() == mu.mac_of(p), len(p)


def test_sweep_package_verify_host_cpu_route(mgr, cpu_route):
    ps = mu.payloads(mu.SWEEP)
    n = len(ps)
    ids = np.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n)
    heads, macs = mgr.package_batch_host(ids, ids - 1, [len(p) for p in ps], ps)
    assert heads.shape == (n, 52) and macs.shape == (n, 20)
    frames = []
    for i, p in enumerate(ps):
        want = mu.frame(mu.FIRST_ENTRY + i, p)
        assert heads[i].tobytes() == want[:52], len(p)
        assert macs[i].tobytes() == want[32:52]
        frames.append(want)
    status, fb = mgr.verify_batch_host(frames, mu.FIRST_ENTRY)
    assert (status == 0).all() and fb == n


def test_package_host_writes_only_52_bytes_of_a_stride(mgr, ks, cpu_route):
    L = _native.lib()
    ps = mu.payloads([0, 10, 100])
    n = len(ps)
    frames = np.full((n, 64), 0xA5, dtype=np.uint8)
    views = [np.frombuffer(p, dtype=np.uint8) for p in ps]
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    lens = np.array([v.size for v in views], dtype=np.uint32)
    ids = np.arange(n, dtype=np.int64)
    rc = L.bkd_digest_package_batch_mac_host(ks.ctypes.data, mu.LEDGER, ids.ctypes.data, ids.ctypes.data,
                                             ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data, n, frames.ctypes.data, 64)
    assert rc == 0
    assert (frames[:, 52:] == 0xA5).all()
    for i, p in enumerate(ps):
        hdr = mu.header(mu.LEDGER, i, i, i)  # the length field is the caller's value, not the payload's size
        assert frames[i, :52].tobytes() == hdr + mu.mac_of(hdr + p)
    for stride in (51, 4097):
        assert L.bkd_digest_package_batch_mac_host(ks.ctypes.data, mu.LEDGER, ids.ctypes.data, ids.ctypes.data,
                                                   ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data, n,
                                                   frames.ctypes.data, stride) == -1


def test_bit_length_crosses_2_pow_32(ks):
    """One entry of 2^29 bytes: its message bit length, 8 * (64 + 2^29), needs more than 32 bits."""
    data = np.tile(np.arange(251, dtype=np.uint8), (1 << 29) // 251 + 1)[:1 << 29]
    assert ck.mac_cpu(ks, data) == hmac.new(KEY, data.data, "sha1").digest()


# ---- verify failure kinds ----

@pytest.mark.parametrize("skip", [False, True])
def test_verify_failure_kinds(mgr, cpu_route, skip):
    frames, want, want_skip = mu.failure_frames()
    status, fb = mgr.verify_batch_host(frames, mu.FIRST_ENTRY, skip_entry_check=skip)
    exp = want_skip if skip else want
    assert status.tolist() == exp.tolist()
    assert fb == mu.first_bad(exp) == 1
    # the first failure further back, and none at all
    status, fb = mgr.verify_batch_host([frames[0], frames[3], frames[2]], mu.FIRST_ENTRY, skip_entry_check=True)
    assert status.tolist() == [0, 0, 1] and fb == 2
    status, fb = mgr.verify_batch_host([frames[0]], mu.FIRST_ENTRY)
    assert status.tolist() == [0] and fb == 1


def test_empty_batches(mgr, ks, cpu_route):
    status, fb = mgr.verify_batch_host([], 0)
    assert status.size == 0 and fb == 0
    heads, macs = mgr.package_batch_host([], [], [], [])
    assert heads.shape == (0, 52) and macs.shape == (0, 20)
    assert ck.mac_batch_host(ks, []).shape == (0, 20)


# ---- the fixtures of the GPU edge suite (test_gpu_mac_edges.py) through the CPU route ----

@pytest.fixture(scope="module")
def seg():
    return mu.segment_batch()


@pytest.fixture(scope="module")
def seg_pk(seg):
    return mu.segment_package(seg)


def test_segment_batch_is_what_the_gpu_suite_assumes(seg):
    assert len(seg["payloads"]) == 4551 and int(seg["lens"].max()) <= mu.SEGMENT
    assert 181 * mu.MIB < int(seg["lens"].sum()) < 182 * mu.MIB
    assert (seg["prefix"] > 2 * mu.SEGMENT).sum() >= 10  # entries that a third segment or a later one holds


def test_segment_batch_mac_cpu_route(ks, cpu_route, seg):
    mu.check_segment_mac(ck, ks, seg)


@pytest.mark.parametrize("stride", [52, 60])
def test_segment_batch_package_cpu_route(mgr, cpu_route, seg, seg_pk, stride):
    mu.check_segment_package(mgr, seg, seg_pk, stride)


def test_segment_batch_verify_cpu_route(mgr, cpu_route, seg):
    for case in mu.segment_verify(seg)["cases"]:
        mu.check_segment_verify(mgr, case)


@pytest.mark.parametrize("ledger", mu.WIDE_LEDGERS)
def test_wide_ids_cpu_route(cpu_route, ledger):
    m = dg.DigestManager.instantiate(ledger, mu.PASSWD, dg.DigestType.HMAC)
    w = mu.wide_ids()
    heads, macs = m.package_batch_host(w["ids"], w["lacs"], w["lfs"], w["payloads"])
    assert mu.wrong_rows(heads, w["heads"][ledger]) == []
    assert (macs == heads[:, 32:]).all()
    for name, frames, first, want in mu.wide_verify_cases(ledger):
        status, fb = m.verify_batch_host(frames, first)
        assert status.tolist() == want and fb == mu.first_bad(want), name


# ---- MacDigestManager's per-entry methods ----

def test_instantiate_hmac():
    m = dg.DigestManager.instantiate(5, b"pw", dg.DigestType.HMAC, True)
    assert isinstance(m, dg.MacDigestManager) and m.useV2Protocol and m.ledgerId == 5
    assert m.macCodeLength == 20 and m.isInt32Digest() is False


@pytest.mark.parametrize("size", [16383, 16384])  # BookieWriteLedgersWithDifferentDigestsTest's two sizes
def test_package_v3_and_v2(size):
    payload = mu.payloads([size], seed=size)[0]
    hdr = mu.header(mu.LEDGER, 9, 8, size)
    mac = mu.mac_of(hdr + payload)
    v3 = dg.MacDigestManager(mu.LEDGER, mu.PASSWD, False)
    assert v3.computeDigestAndPackageForSending(9, 8, size, payload) == hdr + mac + payload
    v2 = dg.MacDigestManager(mu.LEDGER, mu.PASSWD, True)
    master = dg.MacDigestManager.genDigest("ledger", mu.PASSWD)
    prefix = struct.pack(">ii", 4 + 20 + 32 + 20 + size, (2 << 24) | (1 << 16)) + master
    assert v2.computeDigestAndPackageForSending(9, 8, size, payload, masterKey=master) == prefix + hdr + mac + payload
    assert v3.verifyDigestAndReturnData(9, hdr + mac + payload) == payload


def test_composite_payload_is_joined(mgr):
    from bookkeeper_amd.bytebuf import CompositeBuffer
    a, b = mu.payloads([100, 37])
    hdr = mu.header(mu.LEDGER, 1, 0, 137)
    comp = CompositeBuffer([a, b])
    assert mgr.computeDigestAndPackageForSending(1, 0, 137, comp) == hdr + mu.mac_of(hdr + a + b) + a + b


def test_lac_pair(mgr):
    hdr = struct.pack(">qq", mu.LEDGER, 77)
    packed = mgr.computeDigestAndPackageForSendingLac(77)
    assert packed == hdr + mu.mac_of(hdr)
    assert mgr.verifyDigestAndReturnLac(packed) == 77
    bad = bytearray(packed)
    bad[20] ^= 1
    with pytest.raises(dg.BKDigestMatchException) as e:
        mgr.verifyDigestAndReturnLac(bytes(bad))
    assert e.value.reason == dg.VERIFY_DIGEST_MISMATCH
    with pytest.raises(dg.BKDigestMatchException) as e:
        mgr.verifyDigestAndReturnLac(packed[:35])
    assert e.value.reason == dg.VERIFY_TOO_SHORT
    other = dg.MacDigestManager(mu.LEDGER + 1, mu.PASSWD)
    with pytest.raises(dg.BKDigestMatchException) as e:
        other.verifyDigestAndReturnLac(packed)
    assert e.value.reason == dg.VERIFY_LEDGER_MISMATCH


def test_verify_and_return_data_reasons(mgr):
    frames, want, _ = mu.failure_frames()
    for i, (f, st) in enumerate(zip(frames, want.tolist())):
        if st == 0:
            assert mgr.verifyDigestAndReturnData(mu.FIRST_ENTRY + i, f) == f[52:]
        else:
            with pytest.raises(dg.BKDigestMatchException) as e:
                mgr.verifyDigestAndReturnData(mu.FIRST_ENTRY + i, f)
            assert e.value.reason == st, i


def test_unbuilt_batches_say_so(mgr):
    for name in ("reframe_batch", "reframe_batch_host", "package_batch_segments", "package_batch_segments_host",
                 "package_batch_v2", "package_batch_v2_host"):
        with pytest.raises(NotImplementedError, match="MAC"):
            getattr(mgr, name)()


# ---- no device ----

def test_no_device_routes(mgr, ks):
    if _native.device_count() > 0:
        pytest.skip("a device is visible")
    L = _native.lib()
    ps = mu.payloads([5, 70])
    assert ck.mac_batch_host(ks, ps)[1].tobytes() == mu.mac_of(ps[1])  # automatic: the CPU route
    frames = [mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)]
    assert mgr.verify_batch_host(frames, mu.FIRST_ENTRY)[1] == 2
    assert mgr.package_batch_host([1, 2], [0, 1], [5, 70], ps)[0][0].tobytes() == mu.frame(1, ps[0])[:52]
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        for call in (lambda: ck.mac_batch_host(ks, ps), lambda: mgr.verify_batch_host(frames, mu.FIRST_ENTRY),
                     lambda: mgr.package_batch_host([1, 2], [0, 1], [5, 70], ps)):
            with pytest.raises(_native.BkdError) as e:
                call()
            assert e.value.code == -2  # BKD_ERR_NO_DEVICE
    # device-resident calls are GPU work only
    k, p = ks.ctypes.data, 1 << 20
    assert L.bkd_mac_batch(k, p, 64, p, p, 1, p, None) == -2
    assert L.bkd_digest_package_batch_mac(k, 1, p, p, p, p, 64, p, p, 1, p, 52, None) == -2
    assert L.bkd_digest_verify_batch_mac(k, 1, 0, 0, p, 64, p, p, 1, p, p, None) == -2
    assert L.bkd_digest_package_batch_mac(k, 1, p, p, p, p, 64, p, p, 1, p, 51, None) == -1  # stride < 52


def test_oversize_entry_takes_cpu_route_or_fails_when_gpu_forced(ks):
    """An entry over BKD_MAC_MAX_ENTRY: the CPU route serves it whatever the automatic choice is."""
    big = np.zeros(_native.MAC_MAX_ENTRY + 1, dtype=np.uint8)
    got = ck.mac_batch_host(ks, [b"abc", big])
    assert got[0].tobytes() == mu.mac_of(b"abc")
    assert got[1].tobytes() == hmac.new(KEY, big.data, "sha1").digest()


# ---- host SHA-1 under a sanitizer: a stand-alone program, nothing loaded into Python ----

def test_host_mac_under_address_sanitizer(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    exe = str(tmp_path / "mac_sanitize")
    here = os.path.dirname(os.path.abspath(__file__))
    srcs = [os.path.join(here, "mac_sanitize_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                          ("host_mac.cpp", "host_batch.cpp", "host_crc.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-o", exe] + srcs, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "batch ok" and len(lines) == 4 * 201 + 1
    for line in lines[:-1]:
        off, n, raw, framed = line.split()
        off, n = int(off), int(n)
        data = bytes((k * 131 + n * 7 + off) & 0xFF for k in range(off + n))[off:]
        assert raw == mu.mac_of(data).hex(), (off, n)
        assert framed == mu.mac_of(bytes([n]) * 32 + data).hex(), (off, n)
