"""GPU: bkd_digest_reframe_batch — verified frames re-framed with a new LAC from the old header, the
stored digest and the payload length (reframe_frame_kernel), after the verify sequence or, trusted,
without reading a payload byte. Every expected byte is the oracle's DigestManager framing of the same
payload with the new LAC; statuses are compared with verify_batch's on the same input and with the
oracle's verify_entry."""
import contextlib
import functools
import threading

import numpy as np
import pytest

import oracle
import reframe_util as ru
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

ALGOS = [(ck.CRC32C, dg.DigestType.CRC32C), (ck.CRC32, dg.DigestType.CRC32)]
SENTINEL = 0xA5
LEDGER, FIRST = 61, 7000


@pytest.fixture(autouse=True)
def _auto_routes():
    ck.set_group_lanes(0)
    ck.set_plan_mode(0)
    yield
    ck.set_group_lanes(0)
    ck.set_plan_mode(0)


class Case:
    """A batch with some frames corrupted, packed into one buffer: what verify must say about every
    frame (the oracle's verify_entry; 1 for a frame whose offset lies outside the buffer) and the bytes
    a reframe must leave, apart and in place."""

    def __init__(self, b, where, misalign, oob=()):
        self.b, self.hl = b, 32 + b.mac
        frames = ru.corrupt(b, where)
        self.blob, self.offs, self.lens = ru.pack(frames, misalign=misalign, lead=3)
        self.want = np.array([oracle.verify_entry(b.algo, bytes(f), b.ledger, b.first + i)
                              for i, f in enumerate(frames)], dtype=np.int32)
        self.header_only = np.array([0 if s == 2 and k not in ("high",) else s for s, k in
                                     zip(self.want, self._kinds(where))], dtype=np.int32)
        for i in oob:
            self.offs[i] = self.blob.size - 10
            self.want[i] = self.header_only[i] = 1
        self.first_bad = int(np.nonzero(self.want)[0][0]) if self.want.any() else b.n
        self.heads = np.frombuffer(b"".join(b.new_head), dtype=np.uint8).reshape(b.n, self.hl)

    def _kinds(self, where):
        kinds = [None] * self.b.n
        for kind, i in (where.items() if isinstance(where, dict) else where):
            kinds[i] = kind if not (kind == "high" and self.b.algo == ck.CRC32C) else None
        return kinds

    def in_place(self, status):
        """The whole buffer after an in-place reframe: the OK frames' first 32 + mac bytes replaced
        (their payloads, the other frames and the gaps between frames as they were)."""
        blob = self.blob.copy()
        for i in np.nonzero(status == 0)[0]:
            blob[self.offs[i]:self.offs[i] + self.hl] = self.heads[i]
        return blob

    def trusted_heads(self, status):
        """Heads a trusted reframe gives: for a frame whose digest did not verify, the stored digest
        moved by the same correction as a good one's (old ^ new of the good digests)."""
        heads = self.heads.copy()
        for i in np.nonzero((status == 0) & (self.want != 0))[0]:
            f = self.blob[self.offs[i]:self.offs[i] + self.hl]
            delta = self.b.old_digests[i] ^ int(self.b.new_digests[i])
            stored = int.from_bytes(f[self.hl - 4:].tobytes(), "big")
            heads[i, :32] = np.frombuffer(self.b.new_head[i][:32], dtype=np.uint8)
            heads[i, 32:self.hl - 4] = f[32:self.hl - 4]
            heads[i, self.hl - 4:] = np.frombuffer((stored ^ delta).to_bytes(4, "big"), dtype=np.uint8)
        return heads


@functools.lru_cache(maxsize=None)
def _ragged(algo):
    """3 000 frames: every payload length 0 .. 2 599 once, then 400 random ones up to 70 000; frame
    offsets at byte misalignments 0, 1 and 7; one frame of each failure kind and one outside the buffer."""
    rng = np.random.default_rng(100 + algo)
    plens = np.concatenate([np.arange(2600), rng.integers(0, 70001, 400)])
    lacs = rng.integers(-1, 2**62, plens.size)
    lacs[:3] = [-1, 2**63 - 1, FIRST - 1 + 2]  # entry 2 keeps its LAC
    b = ru.Batch(algo, LEDGER, FIRST, plens, lacs, seed=41)
    where = {"payload": 700, "digest": 1400, "high": 1800, "ledger": 2100, "entry": 2400, "short": 2800}
    return Case(b, where, misalign=(0, 1, 7), oob=(2950,))


@functools.lru_cache(maxsize=None)
def _clean(algo):
    rng = np.random.default_rng(200 + algo)
    plens = np.concatenate([np.arange(0, 1200, 3), rng.integers(0, 70001, 100)])
    b = ru.Batch(algo, LEDGER, FIRST, plens, rng.integers(0, 2**50, plens.size), seed=43)
    return Case(b, {}, misalign=(0, 1, 7))


def _upload(torch, gpu, c):
    return (torch.from_numpy(c.blob).to(gpu), torch.from_numpy(c.offs).to(gpu),
            torch.from_numpy(c.lens.astype(np.int32)).to(gpu), torch.from_numpy(c.b.new_lacs).to(gpu))


def _check_apart(torch, gpu, dm, c, dev, stride, want_status, heads=None, stream=None, **kw):
    d_blob, d_off, d_len, d_lac = dev
    n, hl = c.b.n, c.hl
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        out = torch.full((n * stride,), SENTINEL, dtype=torch.uint8, device=gpu)
        st, fb, dig = dm.reframe_batch(d_blob, d_off, d_len, FIRST, d_lac, out_frames=out, frame_stride=stride,
                                       stream=stream, **kw)
        st, fb, dig = st.cpu().numpy(), int(fb.item()), dig.cpu().numpy()
        got, blob = out.cpu().numpy(), d_blob.cpu().numpy()
    assert (st == want_status).all(), np.nonzero(st != want_status)[0][:5]
    nz = np.nonzero(want_status)[0]
    assert fb == (int(nz[0]) if nz.size else n)
    want = np.full((n, stride), SENTINEL, dtype=np.uint8)
    ok = st == 0
    want[ok, :hl] = (c.heads if heads is None else heads)[ok]
    got = got.reshape(n, stride)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], st[bad[:5]])
    want_dig = np.where(ok, want[:, hl - 4:hl].copy().view(">u4").reshape(-1), 0).astype(np.uint32)
    assert (dig.view(np.uint32) == want_dig).all()
    assert (blob == c.blob).all()  # apart: the framed buffer is only read
    return st


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["auto", "direct", "plan"])
@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_ragged_every_route(gpu, algo, dtype, mode):
    """The header / payload / finish verify route with the payloads through the direct kernel and the
    chunk plan: apart at the packed stride and at stride 64, then in place. OK frames equal the oracle's,
    the others (and a sentinel in their out-frames) are untouched; status and first_bad are
    verify_batch's."""
    import torch
    c = _ragged(algo)
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    dev = _upload(torch, gpu, c)
    d_blob, d_off, d_len, d_lac = dev
    ck.set_plan_mode(mode)
    try:
        vst, vfb = dm.verify_batch(d_blob, d_off, d_len, first_entry_id=FIRST)
        vst = vst.cpu().numpy()
        assert (vst == c.want).all() and int(vfb.item()) == c.first_bad
        assert set(np.unique(vst).tolist()) == {0, 1, 2, 3, 4}
        for stride in (c.hl, 64):
            _check_apart(torch, gpu, dm, c, dev, stride, vst)
        st, fb, dig = dm.reframe_batch(d_blob, d_off, d_len, FIRST, d_lac)
    finally:
        ck.set_plan_mode(0)
    st = st.cpu().numpy()
    assert (st == vst).all() and int(fb.item()) == c.first_bad
    got, want = d_blob.cpu().numpy(), c.in_place(vst)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    assert (dig.cpu().numpy().view(np.uint32) == np.where(vst == 0, c.b.new_digests, 0)).all()


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_fused_verify_route(gpu, algo, dtype):
    """Near-uniform frames (4 096 +- 64 B payloads), one per 8-lane group over at least the chip's lane
    slots: verify takes the fused kernel (the condition of verify_framed, checked here as
    test_gpu_parity.py checks it). Frames of every failure kind before and after index 8 * 8 * 64; the
    bad ones are untouched apart (sentinel) and in place."""
    import torch
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = cus * 128 + 40
    rng = np.random.default_rng(300 + algo)
    plens = rng.integers(4096 - 64, 4096 + 65, n)
    b = ru.Batch(algo, LEDGER, FIRST, plens, rng.integers(-1, 2**62, n), seed=47)
    edge = 8 * 8 * 64
    where = [(k, edge - 900 + 150 * j) for j, k in enumerate(("payload", "digest", "high", "ledger", "entry"))]
    where += [(k, edge + 100 + 150 * j) for j, k in enumerate(("payload", "digest", "high", "ledger", "entry"))]
    c = Case(b, where, misalign=(0, 1, 7, 4), oob=(edge - 1000, edge + 1000))
    # the fused route's condition: the plan route, in-band lengths, the automatic lane choice for one
    # frame per group equal to the plan's 8 lanes (bkdigest.hip auto_lanes)
    assert c.blob.size > 256 << 10
    assert (np.abs(c.lens - c.lens[0]) <= c.lens[0] // 16 + 64).all()
    mean = c.blob.size // n
    g = 4 if mean < 512 else (8 if mean < 32768 else 32)
    while g < 64 and n * g < cus * 1024:
        g *= 2
    assert g == 8, g
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    dev = _upload(torch, gpu, c)
    d_blob, d_off, d_len, d_lac = dev
    vst, vfb = dm.verify_batch(d_blob, d_off, d_len, first_entry_id=FIRST)
    vst = vst.cpu().numpy()
    assert (vst == c.want).all() and int(vfb.item()) == c.first_bad
    assert np.count_nonzero(vst) == (12 if algo == ck.CRC32 else 10)
    _check_apart(torch, gpu, dm, c, dev, c.hl, vst)
    st, fb, dig = dm.reframe_batch(d_blob, d_off, d_len, FIRST, d_lac)
    assert (st.cpu().numpy() == vst).all() and int(fb.item()) == c.first_bad
    got, want = d_blob.cpu().numpy(), c.in_place(vst)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    assert (dig.cpu().numpy().view(np.uint32) == np.where(vst == 0, b.new_digests, 0)).all()


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_equals_verify_then_package(gpu, algo, dtype):
    """Today's two-call route: verify_batch, then package_batch of the same payloads with the new LACs.
    reframe_batch's apart frames are the same bytes."""
    import torch
    c = _clean(algo)
    b = c.b
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    d_blob, d_off, d_len, d_lac = _upload(torch, gpu, c)
    vst, _ = dm.verify_batch(d_blob, d_off, d_len, first_entry_id=FIRST)
    assert not vst.any()
    ids = torch.from_numpy(np.arange(FIRST, FIRST + b.n, dtype=np.int64)).to(gpu)
    frames, digests = dm.package_batch(ids, d_lac, torch.from_numpy(b.lenf.astype(np.int64)).to(gpu), d_blob,
                                       d_off + c.hl, (d_len - c.hl).to(torch.int32), sync_check=True)
    out = torch.empty(b.n * c.hl, dtype=torch.uint8, device=gpu)
    st, fb, dig = dm.reframe_batch(d_blob, d_off, d_len, FIRST, d_lac, out_frames=out)
    assert not st.any() and int(fb.item()) == b.n
    assert torch.equal(out.reshape(b.n, c.hl), frames) and torch.equal(dig, digests)
    assert (frames.cpu().numpy() == c.heads).all()


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_trusted(gpu, algo, dtype):
    """BKD_REFRAME_TRUSTED: clean frames come out as in the default mode; a frame with a flipped payload
    or digest byte is re-framed with status 0 (its digest moved by the same correction: the documented
    contract); too short, outside the buffer, CRC32's high digest word and the ids are still caught."""
    import torch
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    c = _clean(algo)
    dev = _upload(torch, gpu, c)
    _check_apart(torch, gpu, dm, c, dev, c.hl, np.zeros(c.b.n, dtype=np.int32), trusted=True)
    st, fb, dig = dm.reframe_batch(*dev[:3], FIRST, dev[3], trusted=True)
    assert not st.any() and int(fb.item()) == c.b.n
    assert (dev[0].cpu().numpy() == c.in_place(np.zeros(c.b.n))).all()
    c = _ragged(algo)
    dev = _upload(torch, gpu, c)
    assert c.header_only[700] == 0 and c.header_only[1400] == 0 and c.want[700] == 2
    heads = c.trusted_heads(c.header_only)
    for stride in (c.hl, 45):
        _check_apart(torch, gpu, dm, c, dev, stride, c.header_only, heads=heads, trusted=True)
    st, fb, dig = dm.reframe_batch(*dev[:3], FIRST, dev[3], trusted=True)
    assert (st.cpu().numpy() == c.header_only).all()
    want = c.blob.copy()
    for i in np.nonzero(c.header_only == 0)[0]:
        want[c.offs[i]:c.offs[i] + c.hl] = heads[i]
    assert (dev[0].cpu().numpy() == want).all()
    # skip_entry_check: the entry-id frame is OK too
    st, _, _ = dm.reframe_batch(*_upload(torch, gpu, c)[:3], FIRST, dev[3], trusted=True, skip_entry_check=True)
    assert (st.cpu().numpy() == np.where(c.header_only == 4, 0, c.header_only)).all()


@pytest.mark.parametrize("trusted", [False, True])
@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_small_batches(gpu, algo, dtype, trusted):
    """n = 0 and n = 1, a frame of exactly 32 + mac bytes (empty payload) and a frame whose offset lies
    outside the buffer."""
    import torch
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    b = ru.Batch(algo, LEDGER, FIRST, [0, 33], [12345, -1], seed=3)
    c = Case(b, {}, misalign=(5,))
    assert c.lens[0] == c.hl
    d_blob, d_off, d_len, d_lac = _upload(torch, gpu, c)
    st, fb, dig = dm.reframe_batch(d_blob, d_off[:0], d_len[:0], FIRST, d_lac[:0], trusted=trusted)
    assert st.numel() == 0 and dig.numel() == 0 and int(fb.item()) == 0
    assert (d_blob.cpu().numpy() == c.blob).all()
    out = torch.full((c.hl,), SENTINEL, dtype=torch.uint8, device=gpu)
    st, fb, dig = dm.reframe_batch(d_blob, d_off[:1], d_len[:1], FIRST, d_lac[:1], out_frames=out, trusted=trusted)
    assert st.tolist() == [0] and int(fb.item()) == 1
    assert out.cpu().numpy().tobytes() == b.new_head[0] and dig.cpu().numpy().view(np.uint32)[0] == b.new_digests[0]
    offs = c.offs.copy()
    offs[1] = c.blob.size - 5  # outside the buffer
    st, fb, dig = dm.reframe_batch(d_blob, torch.from_numpy(offs).to(gpu), d_len, FIRST, d_lac, trusted=trusted)
    assert st.tolist() == [0, 1] and int(fb.item()) == 1 and dig.cpu().numpy().view(np.uint32)[1] == 0
    want = c.blob.copy()
    want[c.offs[0]:c.offs[0] + c.hl] = c.heads[0]
    assert (d_blob.cpu().numpy() == want).all()


def test_reframe_two_streams(gpu):
    """Two batches re-framed concurrently from two threads, each on its own stream: each batch's
    results equal its single-stream results (the oracle's), apart and in place."""
    import torch
    cases = [_ragged(ck.CRC32C), _ragged(ck.CRC32)]
    dms = [dg.DigestManager.instantiate(LEDGER, b"", t) for _, t in ALGOS]
    streams = [torch.cuda.Stream(device=gpu) for _ in cases]
    devs = [_upload(torch, gpu, c) for c in cases]
    torch.cuda.synchronize()
    errors, barrier = [], threading.Barrier(2)

    def work(k):
        try:
            torch.cuda.set_device(gpu)
            c, dm, s = cases[k], dms[k], streams[k]
            barrier.wait()
            for _ in range(3):
                _check_apart(torch, gpu, dm, c, devs[k], c.hl, c.want, stream=s)
            with torch.cuda.stream(s):
                st, fb, _ = dm.reframe_batch(*devs[k][:3], FIRST, devs[k][3], stream=s)
                assert (st.cpu().numpy() == c.want).all() and int(fb.item()) == c.first_bad
                assert (devs[k][0].cpu().numpy() == c.in_place(c.want)).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("algo,dtype", ALGOS)
def test_reframe_batch_host_gpu_route(gpu, algo, dtype):
    """The host call through the GPU (pinned staging, the device sequence, status and digests back, the
    host writing each OK frame's 12 bytes): 2 000 frames with one of each failure kind, as the CPU-route
    test checks them."""
    rng = np.random.default_rng(400 + algo)
    n = 2000
    plens = rng.integers(0, 2600, n)
    plens[-1] = 70000
    plens[[300, 700]] += 8  # (the corrupted payload needs a byte)
    lacs = rng.integers(-1, 2**62, n)
    b = ru.Batch(algo, LEDGER, FIRST, plens, lacs, seed=53)
    where = {"payload": 300, "digest": 500, "high": 900, "ledger": 1100, "entry": 1300, "short": 1700}
    frames = ru.corrupt(b, where)
    before = [bytes(f) for f in frames]
    want = np.array([oracle.verify_entry(algo, f, LEDGER, FIRST + i) for i, f in enumerate(before)])
    dm = dg.DigestManager.instantiate(LEDGER, b"", dtype)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        vst, vfb = dm.verify_batch_host(frames, FIRST)
        st, fb, digests = dm.reframe_batch_host(frames, FIRST, lacs)
    assert (vst == want).all() and (st == want).all() and fb == vfb == 300
    for i in range(n):
        if want[i]:
            assert bytes(frames[i]) == before[i] and digests[i] == 0, i
        else:
            assert bytes(frames[i]) == b.new_frame(i) and digests[i] == b.new_digests[i], i
    frames = [bytearray(f) for f in b.old]
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        st, fb, digests = dm.reframe_batch_host(frames, FIRST, lacs, trusted=True)
    assert not st.any() and fb == n and (digests == b.new_digests).all()
    assert all(bytes(f) == b.new_frame(i) for i, f in enumerate(frames))
    # three copies of the batch in one call (ids unchecked): the host's write-back runs on its thread pool
    frames = [bytearray(f) for f in b.old * 3]
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        st, fb, digests = dm.reframe_batch_host(frames, FIRST, np.tile(lacs, 3), skip_entry_check=True)
    assert not st.any() and fb == 3 * n and (digests == np.tile(b.new_digests, 3)).all()
    assert all(bytes(f) == b.new_frame(i % n) for i, f in enumerate(frames))
