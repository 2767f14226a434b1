"""GPU: package_batch_v2_mac — V2 add requests of MAC ledgers, the 80-byte head written by the lane that
hashed the entry and the small payloads copied in behind it — byte for byte against Python's hmac, and the
host form's GPU route against its CPU route."""
import numpy as np
import pytest

import mac_adds_util as ma
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

BOUNDS = -4  # BKD_ERR_BOUNDS
DEFAULT = dg.SMALL_ENTRY_SIZE_THRESHOLD


def to_dev(gpu, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu) for a in arrays]
    assert out[0].data_ptr() % 16 == 0
    return out


def dev_table(gpu):
    import torch
    return torch.from_numpy(dg.mac_key_table(ma.PASSWORDS).view(np.int32).copy()).to(gpu)


def sync():
    import torch
    ck.stream_sync(torch.cuda.current_stream())


def sync_raises_bounds_once():
    with pytest.raises(_native.BkdError) as e:
        sync()
    assert e.value.code == BOUNDS
    sync()


def run(gpu, ps, small=DEFAULT, flags=0, key_stride=None, req_align=None, pay_align=None, rows=None, offsets=None,
        lengths=None, requests_size=None, readable=None, bounds=False, gaps=3):
    """Packages `ps` and compares the whole request buffer: request i at an address that is req_align(i)
    modulo 16, `gaps` sentinel bytes between and behind the requests."""
    import torch
    n = len(ps)
    r, lids, eids, lacs, lfs = ma.ids_for(n)
    rows = r if rows is None else np.array(rows, dtype=np.uint32).view(np.int32)
    buf, off, ln = mu.lay_out(ps, [None if pay_align is None else pay_align(i) for i in range(n)], tail=5)
    off = off if offsets is None else np.array(offsets, dtype=np.int64)
    ln = ln if lengths is None else np.array(lengths, dtype=np.uint32).view(np.int32)
    if not key_stride:  # one key for all: the C call's key_stride 0
        key_stride, master, masters = None, ma.MASTER, [ma.MASTER] * n
    else:
        keys = np.random.default_rng(62).integers(0, 256, (n, key_stride), dtype=np.uint8)
        masters = [keys[i, :20].tobytes() for i in range(n)]
        master = torch.from_numpy(keys.copy()).to(gpu)
    want = ma.v2_expected(ps, [int(x) & 0xFFFFFFFF for x in rows], lids, eids, lacs, lfs, masters, flags, small, readable)
    # where the requests go
    at, roffs = 0, []
    for i, w in enumerate(want):
        at += gaps
        if req_align is not None:
            at += (req_align(i) - at) % 16
        roffs.append(at)
        at += len(w)
    total = at + gaps if requests_size is None else requests_size
    image = np.full(total, 0xEE, dtype=np.uint8)
    for o, w in zip(roffs, want):
        if o + len(w) <= total:
            image[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
    d_buf, d_off, d_ln, d_rows, d_lids, d_eids, d_lacs, d_lfs, d_roffs = to_dev(
        gpu, buf, off, ln, rows, lids, eids, lacs, lfs, np.array(roffs, dtype=np.int64))
    requests = torch.full((total,), 0xEE, dtype=torch.uint8, device=gpu)
    assert requests.data_ptr() % 16 == 0
    _, _, macs = dg.package_batch_v2_mac(dev_table(gpu), d_rows, d_lids, d_eids, d_lacs, d_lfs, d_buf, d_off, d_ln,
                                         master, key_stride=key_stride, flags=flags, small_threshold=small,
                                         requests=requests, request_offsets=d_roffs)
    sync_raises_bounds_once() if bounds else sync()
    got = requests.cpu().numpy()
    bad = np.flatnonzero(got != image)
    assert bad.size == 0, (bad[:5].tolist(), [i for i, o in enumerate(roffs) if o <= bad[0]][-1:])
    macs = macs.cpu().numpy()
    for i, (o, w) in enumerate(zip(roffs, want)):
        if o + len(w) <= total:
            assert macs[i].tobytes() == w[60:80]
    return got, roffs, want


def test_lengths_0_to_200_at_every_alignment(gpu):
    """Request offsets at every alignment modulo 16, payloads at every alignment modulo 4 (and 16)."""
    ps = mu.payloads(range(201), seed=80)
    run(gpu, ps, req_align=lambda i: (i * 7) % 16, pay_align=lambda i: (i * 5) % 16)
    run(gpu, ps, req_align=lambda i: (i + 3) % 16, pay_align=lambda i: i % 4)


@pytest.mark.parametrize("small,lens", [(100, [99, 100, 101]), (DEFAULT, [16383, 16384, 16385]), (0, [0, 1, 50])])
def test_thresholds(gpu, small, lens):
    ps = mu.payloads(lens + [0, 7], seed=81)
    got, roffs, want = run(gpu, ps, small=small, req_align=lambda i: (5 * i + 1) % 16)
    assert [len(w) for w in want[:3]] == [80 + (l if l < small else 0) for l in lens]


@pytest.mark.parametrize("key_stride,flags", [(0, 0), (20, 0xFFFF), (24, 0)])
def test_key_strides_and_flags(gpu, key_stride, flags):
    ps = mu.payloads([0, 1, 63, 64, 65, 300, 4096], seed=82)
    run(gpu, ps, key_stride=key_stride, flags=flags, req_align=lambda i: (3 * i) % 16)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_batch_sizes(gpu, n):
    lens = np.random.default_rng(83).integers(0, 300, n)
    run(gpu, mu.payloads(lens, seed=84), req_align=lambda i: i % 16, gaps=1)


def test_a_request_that_does_not_fit_is_left_alone(gpu):
    ps = mu.payloads([10, 20, 30], seed=85)
    # the buffer ends one byte short of the last request's payload: the request is not written at all
    probe = ma.v2_expected(ps, [0, 1, 2], *ma.ids_for(3)[1:], [ma.MASTER] * 3, 0, DEFAULT)
    total = sum(3 + len(w) for w in probe) - 1
    got, roffs, _ = run(gpu, ps, requests_size=total, bounds=True)
    assert (got[roffs[2]:] == 0xEE).all()


def test_unreadable_entries_get_a_head_and_no_copy(gpu):
    """A payload out of range, a row of nkeys and one of 0xFFFFFFFF: the 80-byte head with a zero MAC, nothing
    copied (the bytes behind the head stay as they were), the bounds flag."""
    ps = mu.payloads([40, 50, 60, 70, 0], seed=86)
    size = sum(len(p) for p in ps) + 5
    offs = [0, size - 10, 90, 150, 0]  # entry 1 ends past the payload
    got, roffs, want = run(gpu, ps, rows=[0, 1, len(ma.KEYS), 0xFFFFFFFF, 2], offsets=offs, lengths=[40, 50, 60, 70, 0],
                           readable=[True, False, True, True, True], bounds=True, gaps=100)
    assert [len(w) for w in want] == [120, 80, 80, 80, 80]
    for i in (1, 2, 3):
        assert not got[roffs[i] + 60:roffs[i] + 80].any() and (got[roffs[i] + 80:roffs[i] + 100] == 0xEE).all()


def test_host_form_gpu_route_equals_cpu_route(gpu):
    """mu.segment_batch()'s 181 MiB through three staged segments: requests byte for byte on both routes."""
    seg = mu.segment_batch()
    pk = mu.segment_package(seg)
    n = len(seg["payloads"])
    table = dg.mac_key_table([mu.PASSWD, b"other"])
    rows = np.zeros(n, dtype=np.uint32)
    lids = np.full(n, mu.LEDGER, dtype=np.int64)
    args = (table, rows, lids, pk["ids"], pk["lacs"], pk["lfs"], seg["payloads"], ma.MASTER)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        gpu_reqs, gpu_macs = dg.package_batch_v2_mac_host(*args, flags=5)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cpu_reqs, cpu_macs = dg.package_batch_v2_mac_host(*args, flags=5)
    assert (gpu_macs == cpu_macs).all()
    assert all(a.size == b.size and (a == b).all() for a, b in zip(gpu_reqs, cpu_reqs))
    for i in (0, 1, n // 2, n - 2, n - 1):
        p = seg["payloads"][i]
        assert gpu_reqs[i].tobytes() == ma.v2_request(pk["heads"][i][:32], pk["heads"][i][32:], p.tobytes(), ma.MASTER, 5,
                                                      DEFAULT)
    assert mu.wrong_rows(np.stack([r[28:80] for r in gpu_reqs]), pk["heads"]) == []
