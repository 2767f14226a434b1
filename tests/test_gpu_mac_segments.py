"""GPU: package_batch_segments_mac — composite payloads of MAC ledgers, one lane hashing its entry's
segments as one byte stream — bit for bit against Python's hmac, and the host form's GPU route against its
CPU route."""
import ctypes

import numpy as np
import pytest

import mac_adds_util as ma
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

BOUNDS = -4  # BKD_ERR_BOUNDS


def to_dev(gpu, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu) for a in arrays]
    assert out[0].data_ptr() % 16 == 0  # the alignments of Batch.put are the device addresses'
    return out


def dev_table(gpu):
    import torch
    t = torch.from_numpy(dg.mac_key_table(ma.PASSWORDS).view(np.int32).copy()).to(gpu)
    assert t.numel() == 10 * len(ma.PASSWORDS)  # exactly nkeys rows: nothing behind them to depend on
    return t


def sync(stream=None):
    import torch
    ck.stream_sync(torch.cuda.current_stream() if stream is None else stream)


def sync_raises_bounds_once(stream=None):
    with pytest.raises(_native.BkdError) as e:
        sync(stream)
    assert e.value.code == BOUNDS
    sync(stream)


def package(gpu, b: ma.Batch, stride=52, first=None, rows=True, ledgers=True, ledger_id=0, frame_shift=0, stream=None,
            payload=None):
    """(the whole output buffer, 0xEE where nothing was written, with frame i at frame_shift + i * stride; the
    macs tensor); the caller syncs."""
    import torch
    buf, offs, lens, good_first, rws, lids, eids, lacs, lfs = b.arrays()
    d_buf, d_offs, d_lens, d_first, d_rows, d_lids, d_eids, d_lacs, d_lfs = to_dev(
        gpu, buf if payload is None else payload, offs, lens, good_first if first is None else first, rws, lids, eids,
        lacs, lfs)
    n = len(good_first) - 1
    out = torch.full((n * stride + frame_shift + 8,), 0xEE, dtype=torch.uint8, device=gpu)
    assert out.data_ptr() % 4 == 0
    if stream is not None:
        torch.cuda.synchronize()  # the fill above ran on the current stream
    frames, macs = dg.package_batch_segments_mac(dev_table(gpu), d_rows if rows else None, d_lids if ledgers else None,
                                                 d_eids, d_lacs, d_lfs, d_buf, d_offs, d_lens, d_first,
                                                 frame_stride=stride, out_frames=out[frame_shift:], stream=stream,
                                                 ledger_id=ledger_id)
    return out, macs


def frames_of(out, n, stride=52, shift=0):
    return out.cpu().numpy()[shift:shift + n * stride].reshape(n, stride)


def check(gpu, b: ma.Batch, bounds=False, **kw):
    out, macs = package(gpu, b, **kw)
    sync_raises_bounds_once() if bounds else sync()
    got = frames_of(out, b.n)
    assert mu.wrong_rows(got, b.expected()) == []
    assert (macs.cpu().numpy() == got[:, 32:]).all()
    assert (out.cpu().numpy()[b.n * 52:] == 0xEE).all()
    return got


@pytest.mark.parametrize("make", [ma.cut_sweep, ma.three_segments, ma.tiny_segments, ma.shared_and_edges,
                                  ma.long_entries], ids=lambda f: f.__name__)
def test_segments_match_hmac(gpu, make):
    check(gpu, make())


def test_capped_entries(gpu):
    """Two listings of one 8 MiB segment are exactly the cap and are hashed; 8 MiB + 1 and 8 MiB are over it:
    header, zero MAC, the bounds flag, and the neighbours are untouched."""
    b = ma.Batch()
    half = 8 << 20
    big = b.put(ma.payload_bytes(half + 1, 70), 3)
    b.pieces(ma.payload_bytes(50, 71), [20])
    b.entry([(big[0], half), (big[0], half)])
    b.entry([big, (big[0], half)], readable=False)
    b.entry([(big[0], 100), (big[0] + 7, 5)])
    # 257 listings of a 16 MiB range: out of range here too, but the sum must stop long before it wraps
    b.entry([(0, ma.CAP)] * 257, readable=False)
    check(gpu, b, bounds=True)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_batch_sizes_strides_and_frame_alignment(gpu, n):
    b = ma.mixed(n)
    shift = (n + 2) % 4  # frames at addresses 1, 2, 3 modulo 4; every other test has them at 0
    for stride in (52, 64):
        out, _ = package(gpu, b, stride=stride, frame_shift=shift)
        sync()
        host = out.cpu().numpy()
        got = host[shift:shift + n * stride].reshape(n, stride)
        assert mu.wrong_rows(got[:, :52], b.expected()) == []
        assert (got[:, 52:] == 0xEE).all() and (host[:shift] == 0xEE).all() and (host[shift + n * stride:] == 0xEE).all()


def test_empty_batches(gpu):
    b = ma.Batch()
    out, macs = package(gpu, b, payload=np.zeros(16, dtype=np.uint8))  # n == 0
    sync()
    assert macs.shape == (0, 20) and (out.cpu().numpy() == 0xEE).all()
    for _ in range(3):
        b.entry([])  # nseg == 0 with n > 0
    check(gpu, b, payload=np.zeros(16, dtype=np.uint8))


@pytest.mark.parametrize("kind", ma.MALFORMED)
def test_malformed_csr_only_raises_the_flag(gpu, kind):
    """The clamp (segments_range; the CPU suite drives it with these arrays before any GPU test runs) keeps
    every access inside the caller's arrays: the call completes and only the bounds flag says so."""
    b = ma.mixed(8, seed=44)
    first = ma.malformed_first(b.first, len(b.offs), kind)
    n, nseg = b.n, len(b.offs)
    for i in range(n):  # what the device will read stays inside the arrays
        k0, k1 = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.lib().bkd_host_segments_range(int(first[i]), int(first[i + 1]), i, n, nseg, ctypes.byref(k0),
                                              ctypes.byref(k1))
        assert k0.value <= k1.value <= nseg
    out, _ = package(gpu, b, first=first)
    sync_raises_bounds_once()
    got = frames_of(out, n)
    assert all(got[i, :32].tobytes() == b.header(i) for i in range(n))  # every header is still written


def test_keys_and_ids(gpu):
    # two passwords over byte-identical payloads
    b = ma.Batch()
    seg = b.put(ma.payload_bytes(100, 3), 1)
    tail = b.put(ma.payload_bytes(9, 4), 2)
    b.entry([seg, tail], row=0, ids=(1, 2, 3, 4))
    b.entry([seg, tail], row=1, ids=(1, 2, 3, 4))
    got = check(gpu, b)
    assert (got[0, 32:] != got[1, 32:]).any() and (got[0, :32] == got[1, :32]).all()
    # a row index of nkeys and of 0xFFFFFFFF: header, zero MAC, the flag
    b.entry([seg], row=len(ma.KEYS))
    b.entry([tail, seg], row=0xFFFFFFFF)
    b.entry([tail], row=2)
    check(gpu, b, bounds=True)
    # null key_of: row 0 for all; null ledger_ids: ledger_id for all
    b = ma.mixed(10, seed=45)
    b.rows = [0] * b.n
    b.lids = [mu.LEDGER] * b.n
    check(gpu, b, rows=False, ledgers=False, ledger_id=mu.LEDGER)
    # header fields over the whole 64-bit range
    w = mu.wide_ids()
    for led in mu.WIDE_LEDGERS:
        b = ma.Batch()
        for r, p in enumerate(w["payloads"]):
            b.pieces(p, [len(p) // 3], row=r % 3, ids=(led, int(w["ids"][r]), int(w["lacs"][r]), int(w["lfs"][r])))
        check(gpu, b)


def test_out_of_range_segment_makes_its_entry_unreadable(gpu):
    b = ma.mixed(6, seed=46)
    size = len(b.buf)
    b.entry([(0, 10), (size - 3, 4)], readable=False)  # ends one byte past the payload
    b.entry([(size + 1, 1)], readable=False)
    b.entry([(2**63 - 4, 8), (0, 4)], readable=False)  # offset + length past 2^63
    b.entry([(size - 4, 4), (size + 100, 0)])  # an empty segment is skipped wherever it says it lies
    check(gpu, b, bounds=True)


def test_equals_the_contiguous_call(gpu):
    b = ma.mixed(300, seed=47)
    out, _ = package(gpu, b)
    joined = [b.data[i] for i in range(b.n)]
    buf, off, ln = mu.lay_out(joined, [i % 16 for i in range(b.n)], tail=3)
    _, _, _, _, rws, lids, eids, lacs, lfs = b.arrays()
    d_buf, d_off, d_ln, d_rows, d_lids, d_eids, d_lacs, d_lfs = to_dev(gpu, buf, off, ln, rws, lids, eids, lacs, lfs)
    flat, _ = dg.package_batch_ledgers_mac(dev_table(gpu), d_rows, d_lids, d_eids, d_lacs, d_lfs, d_buf, d_off, d_ln)
    sync()
    assert (frames_of(out, b.n) == flat.cpu().numpy()).all()


def test_a_second_stream_keeps_its_own_flag(gpu):
    import torch
    side = torch.cuda.Stream(device=gpu)
    good, bad = ma.mixed(5, seed=48), ma.mixed(5, seed=49)
    bad.entry([(len(bad.buf), 1)], readable=False)
    torch.cuda.synchronize()
    out_bad, _ = package(gpu, bad, stream=side)
    out_good, _ = package(gpu, good)
    sync()  # the current stream is clean
    sync_raises_bounds_once(side)
    assert mu.wrong_rows(frames_of(out_good, good.n), good.expected()) == []
    assert mu.wrong_rows(frames_of(out_bad, bad.n), bad.expected()) == []
    ck.release_stream(side)


def test_host_form_over_the_cap(gpu):
    """8 MiB + 1 and 8 MiB in host memory: INVALID_ARG when the GPU route is forced, the CPU route when the
    choice is automatic."""
    b = ma.Batch()
    big = b.put(bytes(8 << 20) + b"\x01")
    b.entry([big, (big[0], 8 << 20)])
    table = dg.mac_key_table(ma.PASSWORDS)
    args = (table, np.array(b.rows, dtype=np.uint32), b.lids, b.eids, b.lacs, b.lfs, b.host_payloads())
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        with pytest.raises(_native.BkdError) as e:
            dg.package_batch_segments_mac_host(*args)
        assert e.value.code == -1  # BKD_ERR_INVALID_ARG
    with ck.host_batch_route(ck.HOST_ROUTE_AUTO):
        frames, _ = dg.package_batch_segments_mac_host(*args)
    assert mu.wrong_rows(frames, b.expected()) == []


def test_host_form_gpu_route_equals_cpu_route(gpu):
    """mu.segment_batch()'s 181 MiB, three staged segments, every entry cut into two or three leaves; one
    entry's leaves are listed across the 64 MiB cut."""
    seg = mu.segment_batch()
    pk = mu.segment_package(seg)
    n = len(seg["payloads"])
    payloads = []
    for i, p in enumerate(seg["payloads"]):
        a, c = len(p) // 3, (2 * len(p)) // 3 + (i % 2)
        payloads.append([p[:a], p[a:c], p[c:]] if i % 3 else [p[:a], p[a:]])
    across = int(np.flatnonzero((seg["prefix"] < mu.SEGMENT) & (seg["prefix"] + seg["lens"] > mu.SEGMENT))[0])
    assert len(payloads[across]) >= 2
    table = dg.mac_key_table([mu.PASSWD, b"other"])
    rows = np.zeros(n, dtype=np.uint32)
    lids = np.full(n, mu.LEDGER, dtype=np.int64)
    args = (table, rows, lids, pk["ids"], pk["lacs"], pk["lfs"], payloads)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        gpu_frames, gpu_macs = dg.package_batch_segments_mac_host(*args, frame_stride=64)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cpu_frames, cpu_macs = dg.package_batch_segments_mac_host(*args, frame_stride=64)
    assert (gpu_frames == cpu_frames).all() and (gpu_macs == cpu_macs).all()
    assert mu.wrong_rows(gpu_frames[:, :52], pk["heads"]) == [] and not gpu_frames[:, 52:].any()
