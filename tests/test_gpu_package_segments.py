"""GPU: packaging batches whose payloads are composite buffers (bkd_digest_package_batch_segments and
the host forms through the GPU route).

Expected digests and frames are oracle.digest_entry over each entry's concatenated segments; every
entry of every batch is compared, byte for byte, with sentinels around the frames. The malformed
inputs (tests/segments_util.py) are the ones tests/test_package_segments_cpu.py drives the clamp with
on the CPU; here they check that the call flags them and returns.
"""
import ctypes
import threading

import numpy as np
import pytest

import oracle
import segments_util as su
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd._native import BkdError

pytestmark = pytest.mark.gpu

BOUNDS, INVALID_ARG = -4, -1
DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}


@pytest.fixture
def gpu_route(gpu):
    """The host forms through the GPU, whatever route an earlier module left selected (one of them ends
    on the automatic choice). Afterwards the route that was in effect is put back: the GPU route if it
    was selected, else the automatic choice, so later modules run as they would without this one."""
    L = _native.lib()
    before = L.bkd_get_host_batch_route()  # what the next batch would have taken: 1 CPU, 2 GPU
    assert L.bkd_set_host_batch_route(ck.HOST_ROUTE_GPU) == 0
    try:
        yield
    finally:
        L.bkd_set_host_batch_route(ck.HOST_ROUTE_GPU if before == ck.HOST_ROUTE_GPU else ck.HOST_ROUTE_AUTO)


def _dev(torch, a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _package(algo, per_entry, b, payload, offs, lens, first, **kw):
    """The device call with one ledger (DigestManager) or ledger ids (module level); b: id tensors."""
    if per_entry:
        return dg.package_batch_segments(DTYPE[algo], b["ledgers"], b["ids"], b["lacs"], b["lenf"], payload, offs, lens,
                                         first, **kw)
    dm = dg.DigestManager.instantiate(su.ONE_LEDGER[algo], b"", DTYPE[algo])
    return dm.package_batch_segments(b["ids"], b["lacs"], b["lenf"], payload, offs, lens, first, **kw)


@pytest.fixture(scope="module")
def dev_batch(gpu):
    import torch
    b = su.batch()
    return {"ids": _dev(torch, b.ids, gpu), "lacs": _dev(torch, b.lacs, gpu), "lenf": _dev(torch, b.lenf, gpu),
            "ledgers": _dev(torch, b.ledgers, gpu), "offs": _dev(torch, b.offs, gpu),
            "lens": _dev(torch, b.lens.astype(np.int32), gpu), "first": _dev(torch, b.first, gpu)}


@pytest.mark.parametrize("mis", [1, 3])
@pytest.mark.parametrize("mode", [1, 2], ids=["direct", "plan"])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_fixture_batch_on_device(gpu, dev_batch, algo, mode, mis):
    """The fixture batch with its base 1 and 3 bytes off a dword, the segment registers through the
    direct kernel and through the chunked plan: frames in their own buffer (stride 64, one ledger) and
    inside the payload buffer in a region no segment touches (packed, ledger ids)."""
    import torch
    b = su.batch()
    mac = su.MAC[algo]
    hl = 32 + mac
    room = 64 + b.n * 64
    buf = torch.full((mis + su.SIZE + room + 64,), su.SENTINEL, dtype=torch.uint8, device=gpu)
    buf[mis:mis + su.SIZE] = _dev(torch, b.data, gpu)
    payload = buf[mis:mis + su.SIZE + room]  # the frame region is part of the payload buffer
    d = dev_batch
    with ck.plan_mode(mode):  # the mode that was set comes back afterwards
        own = torch.full((b.n, 64), su.SENTINEL, dtype=torch.uint8, device=gpu)
        frames, digests = _package(algo, False, d, payload, d["offs"], d["lens"], d["first"], frame_stride=64,
                                   out_frames=own, sync_check=True)
        assert frames is own
        su.check_frames(own.cpu().numpy(), digests.cpu().numpy(), *b.expected(algo, False), 64)
        inside = payload[su.SIZE + 13:]  # unaligned frames: the byte path of the frame writer
        frames, digests = _package(algo, True, d, payload, d["offs"], d["lens"], d["first"], out_frames=inside,
                                   sync_check=True)
        got = inside.cpu().numpy()
        su.check_frames(got[:b.n * hl], digests.cpu().numpy(), *b.expected(algo, True), hl)
        assert (got[b.n * hl:] == su.SENTINEL).all()
        host = buf.cpu().numpy()
        assert (host[mis:mis + su.SIZE] == b.data).all()  # no payload byte was written
        assert (host[:mis] == su.SENTINEL).all() and (host[mis + su.SIZE:mis + su.SIZE + 13] == su.SENTINEL).all()
        # the default: a new packed [n, 32 + mac] tensor
        frames, digests = _package(algo, True, d, payload, d["offs"], d["lens"], d["first"], sync_check=True)
        assert tuple(frames.shape) == (b.n, hl)
        su.check_frames(frames.cpu().numpy(), digests.cpu().numpy(), *b.expected(algo, True), hl)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_power_table_lengths(gpu, algo):
    """One entry per length at which the power table's index changes bytes: as the last segment after a
    40-byte one, and as the middle segment of three. All segments are cut from one 17 MiB buffer."""
    import torch
    size = 17 << 20
    data = oracle.fill_splitmix64(size, 91)
    assert max(su.POWER_LENGTHS) + 4096 <= size
    offs, lens, first = [], [], [0]
    for j, L in enumerate(su.POWER_LENGTHS):
        offs += [1000 + j, 3 + 5 * j]
        lens += [40, L]
        first.append(len(offs))
        offs += [77 + j, 9 + 3 * j, size - 200 - j]
        lens += [100, L, 77]
        first.append(len(offs))
    n = len(first) - 1
    cats = [b"".join(data[offs[k]:offs[k] + lens[k]].tobytes() for k in range(first[i], first[i + 1])) for i in range(n)]
    ids = np.arange(n, dtype=np.int64) + 2**32 - 3
    lacs = ids - 1
    lenf = np.full(n, 2**40, dtype=np.int64)
    want_d, want_h = su.expected_frames(algo, [-1] * n, ids, lacs, lenf, cats)
    dm = dg.DigestManager.instantiate(-1, b"", DTYPE[algo])
    frames, digests = dm.package_batch_segments(
        _dev(torch, ids, gpu), _dev(torch, lacs, gpu), _dev(torch, lenf, gpu), _dev(torch, data, gpu),
        _dev(torch, np.array(offs, dtype=np.int64), gpu), _dev(torch, np.array(lens, dtype=np.int32), gpu),
        _dev(torch, np.array(first, dtype=np.int64), gpu), sync_check=True)
    assert (digests.cpu().numpy().view(np.uint32) == want_d).all()
    assert (frames.cpu().numpy() == want_h).all()


def _cut_case(kind, algo):
    """4096 packed entries (near-uniform 3900..4300 B: the plan's near-uniform gate; or Zipf-like
    64 B..64 KiB), each cut at 0..4 random points (equal points give empty segments)."""
    rng = np.random.default_rng(300 + 10 * algo + (kind == "zipf"))
    n = 4096
    if kind == "uniform":
        lens = rng.integers(3900, 4301, n)
    else:
        lens = np.clip(64 * rng.zipf(1.3, n) - rng.integers(0, 64, n), 64, 65536)
    offs = np.cumsum(lens) - lens + 3
    data = oracle.fill_splitmix64(int(offs[-1] + lens[-1]) + 69, 17 + algo)
    so, sl, first = [], [], [0]
    for o, l in zip(offs.tolist(), lens.tolist()):
        cuts = [0] + sorted(rng.integers(0, l + 1, int(rng.integers(0, 5))).tolist()) + [l]
        so += [o + c for c in cuts[:-1]]
        sl += [c1 - c0 for c0, c1 in zip(cuts[:-1], cuts[1:])]
        first.append(len(so))
    ids = np.arange(n, dtype=np.int64) + 2**32 - 2000
    lacs = ids - 1
    lenf = 2**40 + np.cumsum(lens)
    return data, offs, lens, np.array(so, dtype=np.int64), np.array(sl, dtype=np.int32), np.array(first, dtype=np.int64), \
        ids, lacs, lenf


@pytest.mark.parametrize("kind", ["uniform", "zipf"])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_cutting_does_not_change_the_result(gpu, algo, kind):
    """Frames and digests of the cut entries equal package_batch on the uncut entries byte for byte,
    and the oracle."""
    import torch
    data, offs, lens, so, sl, first, ids, lacs, lenf = _cut_case(kind, algo)
    n = offs.size
    payloads = [data[o:o + l] for o, l in zip(offs.tolist(), lens.tolist())]
    want_d, want_h = su.expected_frames(algo, [2**32] * n, ids, lacs, lenf, payloads)
    dm = dg.DigestManager.instantiate(2**32, b"", DTYPE[algo])
    base = _dev(torch, data, gpu)
    d_ids, d_lacs, d_lenf = (_dev(torch, a, gpu) for a in (ids, lacs, lenf))
    whole_f, whole_d = dm.package_batch(d_ids, d_lacs, d_lenf, base, _dev(torch, offs, gpu),
                                        _dev(torch, lens.astype(np.int32), gpu), sync_check=True)
    cut_f, cut_d = dm.package_batch_segments(d_ids, d_lacs, d_lenf, base, _dev(torch, so, gpu), _dev(torch, sl, gpu),
                                             _dev(torch, first, gpu), sync_check=True)
    assert torch.equal(cut_f, whole_f) and torch.equal(cut_d, whole_d)
    assert (cut_d.cpu().numpy().view(np.uint32) == want_d).all()
    assert (cut_f.cpu().numpy() == want_h).all()


@pytest.mark.parametrize("mode", [1, 2], ids=["direct", "plan"])
def test_out_of_range_segments(gpu, dev_batch, mode):
    """Three out-of-range segments (first, a middle and the last entry with segments): the stream's
    sync reports BKD_ERR_BOUNDS, every other entry is exact and all headers are written."""
    import torch
    b = su.batch()
    offs, lens, ents = su.out_of_range_segments(b)
    d = dev_batch
    payload = _dev(torch, b.data, gpu)
    with ck.plan_mode(mode):  # the mode that was set comes back afterwards
        for algo in (ck.CRC32C, ck.CRC32):
            own = torch.full((b.n, 64), su.SENTINEL, dtype=torch.uint8, device=gpu)
            _, digests = _package(algo, True, d, payload, _dev(torch, offs, gpu), _dev(torch, lens.astype(np.int32), gpu),
                                  d["first"], frame_stride=64, out_frames=own)
            with pytest.raises(BkdError) as e:
                ck.stream_sync(torch.cuda.current_stream(gpu))
            assert e.value.code == BOUNDS
            su.check_frames(own.cpu().numpy(), digests.cpu().numpy(), *b.expected(algo, True), 64, skip=ents)
            ck.stream_sync(torch.cuda.current_stream(gpu))  # the flag was cleared by the sync that read it


def test_malformed_seg_first(gpu, dev_batch):
    """Each malformed seg_first raises the stream's bounds flag and the call returns; a clean call
    afterwards is exact and unflagged."""
    import torch
    b = su.batch()
    d = dev_batch
    payload = _dev(torch, b.data, gpu)
    cur = torch.cuda.current_stream(gpu)
    for name, first in su.malformed_firsts(b.first, b.nseg).items():
        _package(ck.CRC32C, False, d, payload, d["offs"], d["lens"], _dev(torch, first, gpu))
        with pytest.raises(BkdError) as e:
            ck.stream_sync(cur)
        assert e.value.code == BOUNDS, name
    frames, digests = _package(ck.CRC32C, False, d, payload, d["offs"], d["lens"], d["first"], sync_check=True)
    su.check_frames(frames.cpu().numpy(), digests.cpu().numpy(), *b.expected(ck.CRC32C, False), 36)


def test_degenerate_and_argument_checks(gpu, dev_batch):
    import torch
    b = su.batch()
    d = dev_batch
    payload = _dev(torch, b.data, gpu)
    n = 5
    zero = torch.zeros(n + 1, dtype=torch.int64, device=gpu)
    none64, none32 = torch.zeros(0, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu)
    for algo in (ck.CRC32C, ck.CRC32):  # nseg == 0 with n > 0: every payload is empty
        frames, digests = _package(algo, False, d, payload, none64, none32, zero, sync_check=True)
        want_d, want_h = su.expected_frames(algo, [su.ONE_LEDGER[algo]] * n, b.ids, b.lacs, b.lenf, [b""] * n)
        su.check_frames(frames.cpu().numpy(), digests.cpu().numpy(), want_d, want_h, 32 + su.MAC[algo])
    # a payload shorter than one 16-byte block, an empty segment at its end: the direct kernel whatever the mode
    tiny = _dev(torch, b.data[:10].copy(), gpu)
    t_off = _dev(torch, np.array([0, 10, 3, 9], dtype=np.int64), gpu)
    t_len = _dev(torch, np.array([10, 0, 4, 1], dtype=np.int32), gpu)
    t_first = _dev(torch, np.array([0, 2, 2, 4], dtype=np.int64), gpu)
    cats = [b.data[:10].tobytes(), b"", b.data[3:7].tobytes() + b.data[9:10].tobytes()]
    for mode in (0, 2):
        with ck.plan_mode(mode):
            frames, digests = _package(ck.CRC32C, False, d, tiny, t_off, t_len, t_first, sync_check=True)
        want_d, want_h = su.expected_frames(ck.CRC32C, [su.ONE_LEDGER[ck.CRC32C]] * 3, b.ids, b.lacs, b.lenf, cats)
        su.check_frames(frames.cpu().numpy(), digests.cpu().numpy(), want_d, want_h, 36)
    frames, digests = _package(ck.CRC32C, False, d, payload, none64, none32, zero[:1], sync_check=True)  # n == 0
    assert frames.numel() == 0 and digests.numel() == 0
    with pytest.raises(BkdError) as e:
        _package(ck.CRC32, False, d, payload, d["offs"], d["lens"], d["first"], frame_stride=39)
    assert e.value.code == INVALID_ARG
    with pytest.raises(ValueError):
        _package(ck.CRC32C, False, d, payload, d["offs"], d["lens"][:7], d["first"])
    with pytest.raises(ValueError):  # out_frames too small for n frames
        _package(ck.CRC32C, False, d, payload, d["offs"], d["lens"], d["first"],
                 out_frames=torch.zeros(100, dtype=torch.uint8, device=gpu))
    with pytest.raises(TypeError):
        _package(ck.CRC32C, False, d, payload, d["offs"].to(torch.int32), d["lens"], d["first"])


def test_two_streams_at_once(gpu, dev_batch):
    """Two threads on two streams package different batches concurrently: both results exact, only the
    stream with a bad segment reports."""
    import torch
    b = su.batch()
    d = dev_batch
    payload = _dev(torch, b.data, gpu)
    offs, lens, ents = su.out_of_range_segments(b)
    bad = (_dev(torch, offs, gpu), _dev(torch, lens.astype(np.int32), gpu))
    torch.cuda.synchronize()  # inputs were made on the current stream; the batches run on others
    results = {}
    barrier = threading.Barrier(2)

    def worker(name, algo, per_entry, o, l):
        s = torch.cuda.Stream(device=gpu)
        barrier.wait()
        try:
            with torch.cuda.stream(s):  # the outputs are allocated for the stream that writes them
                for _ in range(10):
                    frames, digests = _package(algo, per_entry, d, payload, o, l, d["first"], stream=s)
            code = 0
            try:
                ck.stream_sync(s)
            except BkdError as e:
                code = e.code
            ck.release_stream(s)  # (the sync above read and cleared the flag)
            results[name] = (code, frames.cpu().numpy(), digests.cpu().numpy())
        except Exception as e:  # noqa: BLE001 - reported by the assertions below
            results[name] = (repr(e), None, None)

    ts = [threading.Thread(target=worker, args=("good", ck.CRC32C, True, d["offs"], d["lens"])),
          threading.Thread(target=worker, args=("bad", ck.CRC32, False, *bad))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert results["good"][0] == 0 and results["bad"][0] == BOUNDS
    su.check_frames(results["good"][1], results["good"][2], *b.expected(ck.CRC32C, True), 36)
    su.check_frames(results["bad"][1], results["bad"][2], *b.expected(ck.CRC32, False), 40, skip=ents)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_host_forms_through_the_gpu_fixture(gpu, algo, gpu_route):
    """The fixture batch through both host forms on the GPU route."""
    b = su.batch()
    views = b.segment_views()
    for per_entry, stride in ((False, 64), (True, 32 + su.MAC[algo])):
        rc, frames, digests = su.package_host_raw(algo, su.ONE_LEDGER[algo], b.ledgers if per_entry else None, b.ids,
                                                  b.lacs, b.lenf, views, b.first, stride)
        assert rc == 0
        su.check_frames(frames, digests, *b.expected(algo, per_entry), stride)
    got = ck.crc_batch_segments_host(algo, views, b.first, seeds=b.seeds)
    assert (got == np.array([oracle.resume(algo, int(b.seeds[i]), b.cat[i]) for i in range(b.n)], np.uint32)).all()
    got = ck.crc_batch_segments_host(algo, views, b.first, seed_all=7)
    assert (got == np.array([oracle.resume(algo, 7, c) for c in b.cat], np.uint32)).all()


def test_host_forms_gather_across_staging_segments(gpu, gpu_route):
    """20 entries of 8 MiB, each of three segments: three staging segments of <= 64 MiB (8, 8 and 4
    entries), so entries are gathered on both sides of a staging boundary."""
    M = 1 << 20
    src = oracle.fill_splitmix64(24 * M, 5)
    n = 20
    views, first, cats = [], [0], []
    for i in range(n):
        a, c = 3 * M + 17 * i, M + 5 + i
        parts = [src[7 + i:7 + i + a], src[12 * M - i:12 * M - i + c], src[9 * M + 3 * i:9 * M + 3 * i + 8 * M - a - c]]
        assert sum(p.size for p in parts) == 8 * M
        views += parts
        first.append(len(views))
        cats.append(np.concatenate(parts))
    ids = np.arange(n, dtype=np.int64) + 2**32 - 10
    lacs, lenf = ids - 1, np.full(n, 2**40, dtype=np.int64)
    want_d, want_h = su.expected_frames(ck.CRC32C, [-2**63] * n, ids, lacs, lenf, cats)
    rc, frames, digests = su.package_host_raw(ck.CRC32C, -2**63, None, ids, lacs, lenf, views, first, 36)
    assert rc == 0
    su.check_frames(frames, digests, want_d, want_h, 36)
    got = ck.crc_batch_segments_host(ck.CRC32, views, first, seed_all=3)
    assert got.tolist() == [oracle.resume(ck.CRC32, 3, c) for c in cats]


def test_forced_gpu_route_refuses_an_oversize_entry(gpu, gpu_route):
    """An entry whose segments sum to more than a staging segment, the GPU route forced: refused with
    BKD_ERR_INVALID_ARG before any work — the lengths claim 3 x 32 MiB over pointers to one small
    buffer, which is never read, and nothing is written."""
    small = np.zeros(4096, dtype=np.uint8)
    vp = ctypes.c_void_p
    ptrs = np.full(4, small.ctypes.data, dtype=np.uint64)
    lens = np.array([100, 32 << 20, 32 << 20, 32 << 20], dtype=np.uint32)
    first = np.array([0, 1, 4], dtype=np.uint64)
    ids = np.array([1, 2], dtype=np.int64)
    frames = np.full(2 * 36, su.SENTINEL, dtype=np.uint8)
    digests = np.full(2, 0xDEADBEEF, dtype=np.uint32)
    rc = _native.lib().bkd_digest_package_batch_segments_host(
        ck.CRC32C, 1, None, vp(ids.ctypes.data), vp(ids.ctypes.data), vp(ids.ctypes.data), vp(ptrs.ctypes.data),
        vp(lens.ctypes.data), 4, vp(first.ctypes.data), 2, vp(frames.ctypes.data), 36, vp(digests.ctypes.data))
    assert rc == INVALID_ARG
    assert (frames == su.SENTINEL).all() and (digests == 0xDEADBEEF).all()
    out = np.full(2, 0xDEADBEEF, dtype=np.uint32)
    rc = _native.lib().bkd_crc_batch_segments_host(ck.CRC32C, vp(ptrs.ctypes.data), vp(lens.ctypes.data), 4,
                                                   vp(first.ctypes.data), 2, None, 0, vp(out.ctypes.data))
    assert rc == INVALID_ARG and (out == 0xDEADBEEF).all()
