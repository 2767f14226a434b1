"""CPU: re-framing verified entries with a new LAC (bkd_digest_reframe_batch_host on the CPU route,
host_batch.cpp reframe_frames) — LedgerFragmentReplicator's second computeDigestAndPackageForSending of
an entry it has just verified (LedgerFragmentReplicator.java:436-442), without a second pass over the
payload. CRC is affine over GF(2):

    crc(H' || P) = crc(H || P) ^ R(H ^ H') * x^(8 |P|)   (mod P)

Every expected byte is the oracle's DigestManager framing of the same payload with the new LAC. Needs no
GPU: the route is forced to the CPU (the automatic one without a device). The device call and the GPU
route of the host call are tested in test_gpu_reframe.py."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle
import reframe_util as ru
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

ALGOS = [(ck.CRC32C, dg.DigestType.CRC32C), (ck.CRC32, dg.DigestType.CRC32)]
LAC_PAIRS = [(7, 7), (-1, 0), (0, 2**63 - 1), (41, 42), (2**40 + 3, 5), (-1, 2**63 - 1)]


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def _delta(algo, old_lac, new_lac, payload_len):
    """R(D) * x^(8 L) with the library's host GF(2) helpers; R(D), the register after folding the
    32-byte header difference from a zero register, is ~resume(~0, D)."""
    L = _native.lib()
    diff = bytes(16) + struct.pack(">Q", (old_lac ^ new_lac) & (2**64 - 1)) + bytes(8)
    r = ~oracle.resume(algo, 0xFFFFFFFF, diff) & 0xFFFFFFFF
    return L.bkd_host_gf_mul(algo, r, L.bkd_host_xpow8n(algo, payload_len))


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_affine_identity_against_oracle(algo, dtype):
    """old ^ gf_mul(R(D), xpow8n(L)) is the oracle's digest of the entry framed with the new LAC."""
    rng = np.random.default_rng(3 + algo)
    for L in (0, 1, 3, 4, 15, 16, 17, 255, 4096, 70000):
        payload = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        for old_lac, new_lac in LAC_PAIRS:
            old, _ = oracle.digest_entry(algo, 9, 77, old_lac, 5000 + L, payload)
            want, _ = oracle.digest_entry(algo, 9, 77, new_lac, 5000 + L, payload)
            d = _delta(algo, old_lac, new_lac, L)
            assert (old_lac != new_lac) or d == 0
            assert old ^ d == want, (L, old_lac, new_lac)


@pytest.mark.parametrize("threads", [1, 0], ids=["1-thread", "all-threads"])
@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_batch_host_cpu_matches_oracle(algo, dtype, threads):
    """600 frames of 32 + mac .. 2 600 bytes and one of 70 000, in place: every frame equals the
    oracle's frame with the new LAC byte for byte, the digests the oracle's."""
    rng = np.random.default_rng(11 + algo)
    hl = 32 + ru.MAC[algo]
    flens = [hl + (i * (2600 - hl)) // 599 for i in range(600)] + [70000]
    n = len(flens)
    lacs = rng.integers(-1, 2**62, n)
    lacs[:4] = [-1, 0, 2**63 - 1, 499]  # 499: entry 3's old LAC (equal LACs)
    b = ru.Batch(algo, 21, 500, [f - hl for f in flens], lacs, seed=5)
    dm = dg.DigestManager.instantiate(21, b"", dtype)
    frames = [bytearray(f) for f in b.old]
    ck.set_host_threads(threads)
    try:
        st, fb, digests = dm.reframe_batch_host(frames, 500, lacs)
    finally:
        ck.set_host_threads(0)
    assert (st == 0).all() and fb == n
    for i in range(n):
        assert bytes(frames[i]) == b.new_frame(i), i
    assert (digests == b.new_digests).all()
    # numpy buffers are rewritten in place too
    arrs = [np.frombuffer(f, dtype=np.uint8).copy() for f in b.old[:50]]
    st, fb, _ = dm.reframe_batch_host(arrs, 500, lacs[:50])
    assert fb == 50 and all(a.tobytes() == b.new_frame(i) for i, a in enumerate(arrs))
    st, fb, digests = dm.reframe_batch_host([], 500, [])
    assert fb == 0 and st.size == 0 and digests.size == 0


def _corrupt_batch(algo):
    rng = np.random.default_rng(17 + algo)
    n = 64
    plens = rng.integers(40, 3000, n)
    lacs = rng.integers(0, 2**40, n)
    b = ru.Batch(algo, 33, 2000, plens, lacs, seed=9)
    where = {"payload": 9, "digest": 17, "high": 23, "ledger": 31, "entry": 40, "short": 52}
    return b, where, ru.corrupt(b, where), lacs


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_batch_host_leaves_bad_frames_alone(algo, dtype):
    """One frame of each failure kind: statuses and first_bad are verify_batch_host's, the bad frames'
    bytes unchanged and their digests 0; every other frame is the oracle's new frame."""
    b, where, frames, lacs = _corrupt_batch(algo)
    dm = dg.DigestManager.instantiate(33, b"", dtype)
    before = [bytes(f) for f in frames]
    want_st, want_fb = dm.verify_batch_host([bytearray(f) for f in frames], 2000)
    oracle_st = np.array([oracle.verify_entry(algo, f, 33, 2000 + i) for i, f in enumerate(before)])
    assert (want_st == oracle_st).all()
    assert set(np.unique(want_st).tolist()) == {0, 1, 2, 3, 4}
    st, fb, digests = dm.reframe_batch_host(frames, 2000, lacs)
    assert (st == want_st).all() and fb == want_fb == 9
    for i in range(b.n):
        if want_st[i]:
            assert bytes(frames[i]) == before[i] and digests[i] == 0, i
        else:
            assert bytes(frames[i]) == b.new_frame(i) and digests[i] == b.new_digests[i], i
    assert sum(1 for s in want_st if s) == (6 if algo == ck.CRC32 else 5)
    # skip_entry_check: the entry-id frame passes and is re-framed with its own ids
    frames = [bytearray(f) for f in before]
    st, fb, digests = dm.reframe_batch_host(frames, 2000, lacs, skip_entry_check=True)
    assert (st == np.where(want_st == 4, 0, want_st)).all()
    i = where["entry"]
    pay = before[i][32 + b.mac:]
    assert bytes(frames[i]) == ru.frame(algo, 33, 2000 + i + 5, lacs[i], b.lenf[i], pay)[0]


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_batch_host_trusted(algo, dtype):
    """BKD_REFRAME_TRUSTED recomputes no digest: a frame with a flipped payload byte is re-framed with
    status 0 and digest old ^ delta, which does not verify (the documented contract); what the header
    alone decides (too short, CRC32's high digest word, ids) is still caught. Clean frames come out as
    in the default mode."""
    b, where, frames, lacs = _corrupt_batch(algo)
    dm = dg.DigestManager.instantiate(33, b"", dtype)
    before = [bytes(f) for f in frames]
    st, fb, digests = dm.reframe_batch_host(frames, 2000, lacs, trusted=True)
    want = np.zeros(b.n, dtype=np.int32)
    want[where["short"]], want[where["ledger"]], want[where["entry"]] = 1, 3, 4
    if algo == ck.CRC32:
        want[where["high"]] = 2
    assert (st == want).all() and fb == int(np.nonzero(want)[0][0])
    hl = 32 + b.mac
    for i in range(b.n):
        if want[i]:
            assert bytes(frames[i]) == before[i] and digests[i] == 0, i
        elif i in (where["payload"], where["digest"]):
            old = struct.unpack(">I", before[i][hl - 4:hl])[0]
            new = old ^ _delta(algo, 2000 + i - 1, int(lacs[i]), len(before[i]) - hl)
            assert digests[i] == new
            assert bytes(frames[i]) == before[i][:16] + struct.pack(">q", int(lacs[i])) + before[i][24:hl - 4] + \
                struct.pack(">I", new) + before[i][hl:]
            assert oracle.verify_entry(algo, bytes(frames[i]), 33, 2000 + i) == 2
        else:
            assert bytes(frames[i]) == b.new_frame(i) and digests[i] == b.new_digests[i], i


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_batch_host_long_frame_over_the_pool(algo, dtype):
    """A frame of more than 4 MiB is verified in pieces over the host pool (host_batch.cpp fold) and
    re-framed like any other; corrupted in its last piece it is left alone."""
    b = ru.Batch(algo, 8, 70, [5 * (1 << 20) + 13, 100], [2**40, 68], seed=13)
    dm = dg.DigestManager.instantiate(8, b"", dtype)
    for trusted in (False, True):
        frames = [bytearray(f) for f in b.old]
        st, fb, digests = dm.reframe_batch_host(frames, 70, b.new_lacs, trusted=trusted)
        assert fb == 2 and not st.any() and (digests == b.new_digests).all()
        assert bytes(frames[0]) == b.new_frame(0) and bytes(frames[1]) == b.new_frame(1)
    frames = [bytearray(f) for f in b.old]
    frames[0][-2] ^= 0x10
    before = bytes(frames[0])
    st, fb, digests = dm.reframe_batch_host(frames, 70, b.new_lacs)
    assert st.tolist() == [2, 0] and fb == 0 and digests[0] == 0
    assert bytes(frames[0]) == before and bytes(frames[1]) == b.new_frame(1)


def test_reframe_argument_errors_and_dummy_refusal():
    L = _native.lib()
    dm = dg.DigestManager.instantiate(1, b"", dg.DigestType.CRC32C)
    f, _ = ru.frame(ck.CRC32C, 1, 0, -1, 3, b"abc")
    with pytest.raises(TypeError):
        dm.reframe_batch_host([f], 0, [5])  # bytes: not writable
    with pytest.raises(ValueError):
        dm.reframe_batch_host([bytearray(f)], 0, [5, 6])
    buf = bytearray(f)
    ptrs = np.array([np.frombuffer(buf, dtype=np.uint8).ctypes.data], dtype=np.uint64)
    lens = np.array([len(buf)], dtype=np.uint32)
    lacs = np.array([5], dtype=np.int64)
    st = np.zeros(1, dtype=np.int32)
    fb = ctypes.c_uint64(0)
    vp = ctypes.c_void_p
    host = lambda algo, flags, lac, fbp: L.bkd_digest_reframe_batch_host(
        algo, 1, 0, 0, flags, vp(ptrs.ctypes.data), vp(lens.ctypes.data), 1, lac, None, vp(st.ctypes.data), fbp)
    assert host(0, 2, vp(lacs.ctypes.data), ctypes.byref(fb)) == -1  # unknown flag bits
    assert host(0, 0, None, ctypes.byref(fb)) == -1  # NULL new_lacs
    assert host(7, 0, vp(lacs.ctypes.data), ctypes.byref(fb)) == -1  # unknown algorithm
    assert host(0, 0, vp(lacs.ctypes.data), None) == -1  # NULL first_bad
    assert bytes(buf) == f
    assert host(0, 0, vp(lacs.ctypes.data), ctypes.byref(fb)) == 0 and fb.value == 1  # h_digests may be NULL
    assert bytes(buf) == ru.frame(ck.CRC32C, 1, 0, 5, 3, b"abc")[0]
    # the device call checks its arguments before it touches a device (the pointers are never read)
    P = 1 << 30
    dev = lambda flags, lac, out, stride: L.bkd_digest_reframe_batch(
        0, 1, 0, 0, flags, vp(P), 1 << 20, vp(P), vp(P), 4, lac, out, stride, None, vp(P), vp(P), None)
    assert dev(4, vp(P), None, 0) == -1  # unknown flag bits
    assert dev(0, None, None, 0) == -1  # NULL new_lacs
    assert dev(0, vp(P), vp(P << 1), 35) == -1  # frame_stride < 32 + mac
    assert dev(0, vp(P), vp(P + (1 << 20) - 1), 36) == -1  # out-frames start inside the framed buffer
    assert dev(0, vp(P), vp(P - 3 * 36 - 1), 36) == -1  # out-frames end inside it
    for name in ("reframe_batch", "reframe_batch_host"):
        with pytest.raises(NotImplementedError):
            getattr(dg.DigestManager.instantiate(1, b"", dg.DigestType.DUMMY), name)([], 0, [])


_NO_DEVICE_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import reframe_util as ru
from bookkeeper_amd import _native, digest as dg
assert _native.device_count() == 0
assert _native.lib().bkd_get_host_batch_route() == 1  # automatic: the CPU route
for algo, dtype in ((0, dg.DigestType.CRC32C), (1, dg.DigestType.CRC32)):
    b = ru.Batch(algo, 4, 10, [0, 1, 100, 5000], [3, -1, 2**63 - 1, 9], seed=2)
    frames = [bytearray(f) for f in b.old]
    for trusted in (False, True):
        st, fb, digests = dg.DigestManager.instantiate(4, b"", dtype).reframe_batch_host(
            frames, 10, b.new_lacs, trusted=trusted)
        assert fb == 4 and (st == 0).all() and (digests == b.new_digests).all()
        assert [bytes(f) for f in frames] == [b.new_frame(i) for i in range(4)]
print("reframed without a device")
"""


def test_reframe_batch_host_without_a_device():
    """With no device visible the automatic route is the CPU route and the call succeeds (a fresh
    process with the devices hidden, so the check also runs on a host that has one)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "reframed without a device" in r.stdout, r.stderr[-2000:]
