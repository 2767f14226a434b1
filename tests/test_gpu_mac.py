"""GPU: the MAC (HMAC-SHA1) batch kernels — raw, package and verify, device-resident and through the
host forms' GPU route — bit for bit against Python's hmac / hashlib."""
import hmac

import numpy as np
import pytest

import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

CAP = _native.MAC_MAX_ENTRY


@pytest.fixture(scope="module")
def ks():
    return ck.mac_key_init(mu.PASSWD)


@pytest.fixture(scope="module")
def mgr():
    return dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)


def sync():
    """bkd_stream_sync on the stream the calls above ran on: raises BKD_ERR_BOUNDS for an unread entry."""
    import torch
    ck.stream_sync(torch.cuda.current_stream())


lay_out = mu.lay_out


def to_dev(gpu, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu) for a in arrays]
    assert out[0].data_ptr() % 16 == 0  # alignments in lay_out are the device addresses'
    return out


# every length 0..200 at every start alignment 0..15: 16 x 201 entries in one batch; references once
@pytest.fixture(scope="module")
def sweep():
    lengths = [n for _ in range(16) for n in range(201)]
    aligns = [a for a in range(16) for _ in range(201)]
    ps = mu.payloads(lengths, seed=21)
    ids = np.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + len(ps), dtype=np.int64)
    frames = [mu.frame(int(i), p) for i, p in zip(ids, ps)]
    return dict(ps=ps, aligns=aligns, ids=ids, frames=frames, macs=[mu.mac_of(p) for p in ps])


@pytest.fixture(scope="module")
def long_sweep():
    ps = mu.payloads(range(4090, 4101), seed=22)
    ids = np.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + len(ps), dtype=np.int64)
    aligns = [(5 * i + 1) % 16 for i in range(len(ps))]
    return dict(ps=ps, aligns=aligns, ids=ids, frames=[mu.frame(int(i), p) for i, p in zip(ids, ps)],
                macs=[mu.mac_of(p) for p in ps])


def check_raw_package_verify(gpu, ks, mgr, case):
    ps, ids = case["ps"], case["ids"]
    n = len(ps)
    buf, off, ln = lay_out(ps, case["aligns"])
    d_buf, d_off, d_ln, d_ids = to_dev(gpu, buf, off, ln, ids)
    macs = ck.mac_batch(ks, d_buf, d_off, d_ln, sync_check=True).cpu().numpy()
    for i in range(n):
        assert macs[i].tobytes() == case["macs"][i], (i, len(ps[i]), case["aligns"][i])
    frames, fmacs = mgr.package_batch(d_ids, d_ids - 1, d_ln.to(d_ids.dtype), d_buf, d_off, d_ln, sync_check=True)
    frames, fmacs = frames.cpu().numpy(), fmacs.cpu().numpy()
    for i in range(n):
        assert frames[i].tobytes() == case["frames"][i][:52], (i, len(ps[i]), case["aligns"][i])
        assert fmacs[i].tobytes() == case["frames"][i][32:52]
    fbuf, foff, fln = lay_out(case["frames"], case["aligns"])
    d_fbuf, d_foff, d_fln = to_dev(gpu, fbuf, foff, fln)
    status, fb = mgr.verify_batch(d_fbuf, d_foff, d_fln, mu.FIRST_ENTRY)
    sync()
    assert status.cpu().numpy().tolist() == [0] * n and int(fb.item()) == n


def test_sweep_every_length_and_alignment(gpu, ks, mgr, sweep):
    check_raw_package_verify(gpu, ks, mgr, sweep)


def test_sweep_4090_to_4100(gpu, ks, mgr, long_sweep):
    check_raw_package_verify(gpu, ks, mgr, long_sweep)


def test_ragged_batch_and_tiny_batches(gpu, ks, mgr):
    """257 entries whose lengths cycle through 0, 1, 5000, 63, 64, 65, 65536: neighbouring lanes of a
    wave diverge and the last wave is partial. Then n = 1 and n = 0."""
    import torch
    cyc = [0, 1, 5000, 63, 64, 65, 65536]
    ps = mu.payloads([cyc[i % 7] for i in range(257)], seed=23)
    buf, off, ln = lay_out(ps, [None] * 257)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    macs = ck.mac_batch(ks, d_buf, d_off, d_ln, sync_check=True).cpu().numpy()
    for i, p in enumerate(ps):
        assert macs[i].tobytes() == mu.mac_of(p), (i, len(p))
    one = ck.mac_batch(ks, d_buf, d_off[2:3], d_ln[2:3], sync_check=True).cpu().numpy()
    assert one[0].tobytes() == mu.mac_of(ps[2])
    assert ck.mac_batch(ks, d_buf, d_off[:0], d_ln[:0], sync_check=True).shape == (0, 20)
    frames, fmacs = mgr.package_batch(d_off[:0], d_off[:0], d_off[:0], d_buf, d_off[:0], d_ln[:0])
    assert frames.shape == (0, 52) and fmacs.shape == (0, 20)
    status, fb = mgr.verify_batch(d_buf, d_off[:0], d_ln[:0], 0)
    torch.cuda.synchronize()
    assert status.numel() == 0 and int(fb.item()) == 0


@pytest.mark.parametrize("n_last", [1, 4, 63, 64, 130])
def test_first_entry_at_byte_one_last_ends_on_last_byte(gpu, ks, mgr, n_last):
    ps = mu.payloads([77, 3, n_last], seed=24 + n_last)
    buf, off, ln = lay_out(ps, [1, None, None])
    assert off[0] == 1 and off[-1] + ln[-1] == buf.size
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    macs = ck.mac_batch(ks, d_buf, d_off, d_ln, sync_check=True).cpu().numpy()
    assert [m.tobytes() for m in macs] == [mu.mac_of(p) for p in ps]
    fr = [mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)]
    fbuf, foff, fln = lay_out(fr, [1, None, None])
    d_fbuf, d_foff, d_fln = to_dev(gpu, fbuf, foff, fln)
    status, fb = mgr.verify_batch(d_fbuf, d_foff, d_fln, mu.FIRST_ENTRY)
    assert status.cpu().numpy().tolist() == [0, 0, 0] and int(fb.item()) == 3


def test_entry_of_exactly_the_cap(gpu, ks):
    import torch
    data = torch.empty(CAP, dtype=torch.uint8, device=gpu)
    ck.fill_splitmix64(data, 99)
    off = torch.zeros(1, dtype=torch.int64, device=gpu)
    ln = torch.full((1,), CAP, dtype=torch.int32, device=gpu)
    mac = ck.mac_batch(ks, data, off, ln, sync_check=True).cpu().numpy()
    assert mac[0].tobytes() == hmac.new(mu.mac_key(), data.cpu().numpy().data, "sha1").digest()


def test_over_the_cap_and_out_of_range_are_not_read(gpu, ks, mgr):
    """One entry of cap + 1 bytes and one with offset + length > size: zero MACs, BKD_ERR_BOUNDS from the
    stream's sync, and the neighbours in the same batch exact."""
    import torch
    size = CAP + 1 + 300
    data = torch.empty(size, dtype=torch.uint8, device=gpu)
    ck.fill_splitmix64(data, 98)
    off = torch.tensor([0, 100, CAP + 1, size - 50, CAP + 101], dtype=torch.int64, device=gpu)
    ln = torch.tensor([100, CAP + 1, 100, 51, 199], dtype=torch.int32, device=gpu)
    host = data.cpu().numpy()
    want = [mu.mac_of(host[o:o + l].tobytes()) for o, l in ((0, 100), (CAP + 1, 100), (CAP + 101, 199))]
    macs = ck.mac_batch(ks, data, off, ln)
    with pytest.raises(_native.BkdError) as e:
        sync()
    assert e.value.code == -4  # BKD_ERR_BOUNDS
    sync()  # the flag is cleared by the sync that reported it
    macs = macs.cpu().numpy()
    assert [macs[i].tobytes() for i in (0, 2, 4)] == want
    assert not macs[1].any() and not macs[3].any()
    ids = torch.arange(5, dtype=torch.int64, device=gpu)
    frames, fmacs = mgr.package_batch(ids, ids, ids, data, off, ln)
    with pytest.raises(_native.BkdError):
        sync()
    frames = frames.cpu().numpy()
    for i in range(5):
        assert frames[i, :32].tobytes() == mu.header(mu.LEDGER, i, i, i)  # the header is still written
    assert not frames[1, 32:].any() and not frames[3, 32:].any()
    hdr = mu.header(mu.LEDGER, 2, 2, 2)
    assert frames[2, 32:].tobytes() == mu.mac_of(hdr + host[CAP + 1:CAP + 101].tobytes())
    # verify: an unreadable frame gets the status the CRC verify gives an out-of-range one, 1
    status, fb = mgr.verify_batch(data, off, ln, 0)
    with pytest.raises(_native.BkdError):
        sync()
    status = status.cpu().numpy()
    assert status[1] == 1 and status[3] == 1 and int(fb.item()) == 0
    assert (status[[0, 2, 4]] == 2).all()  # random bytes are read and do not verify


def test_package_writes_only_52_bytes_of_a_stride(gpu, mgr):
    import torch
    ps = mu.payloads([0, 1, 64, 300, 4096], seed=26)
    buf, off, ln = lay_out(ps, [None] * 5)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = torch.arange(5, dtype=torch.int64, device=gpu)
    out = torch.full((5, 64), 0xA5, dtype=torch.uint8, device=gpu)
    frames, _ = mgr.package_batch(ids, ids - 1, d_ln.to(torch.int64), d_buf, d_off, d_ln, frame_stride=64,
                                  sync_check=True, out_frames=out)
    got = out.cpu().numpy()
    assert (got[:, 52:] == 0xA5).all()
    for i, p in enumerate(ps):
        assert got[i, :52].tobytes() == mu.frame(i, p)[:52]


def test_verify_failure_kinds_on_device(gpu, mgr):
    frames, want, want_skip = mu.failure_frames()
    buf, off, ln = lay_out(frames, [(3 * i) % 16 for i in range(len(frames))], tail=7)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    for skip, exp in ((False, want), (True, want_skip)):
        status, fb = mgr.verify_batch(d_buf, d_off, d_ln, mu.FIRST_ENTRY, skip_entry_check=skip)
        sync()
        assert status.cpu().numpy().tolist() == exp.tolist()
        assert int(fb.item()) == mu.first_bad(exp)


def test_verify_thousand_frames_three_bad(gpu, mgr):
    ps = mu.payloads([100 + (i % 90) for i in range(1000)], seed=27)
    frames = [bytearray(mu.frame(mu.FIRST_ENTRY + i, p)) for i, p in enumerate(ps)]
    frames[3][60] ^= 1                    # a payload byte: digest mismatch
    frames[500] = bytearray(mu.frame(mu.FIRST_ENTRY + 500, ps[500], ledger=mu.LEDGER + 1))
    frames[999] = bytearray(mu.frame(mu.FIRST_ENTRY + 998, ps[999]))
    want = np.zeros(1000, dtype=np.int32)
    want[[3, 500, 999]] = [2, 3, 4]
    buf, off, ln = lay_out([bytes(f) for f in frames], [None] * 1000)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    status, fb = mgr.verify_batch(d_buf, d_off, d_ln, mu.FIRST_ENTRY)
    sync()
    assert (status.cpu().numpy() == want).all() and int(fb.item()) == 3


def test_host_forms_on_the_gpu_route(gpu, ks, mgr):
    """The 0..200 sweep and the failure kinds through the staged pipeline (the GPU route, selected here: the
    session's setting may have been changed by an earlier test), equal to hmac and to the CPU route's
    results for the same inputs."""
    ps = mu.payloads(mu.SWEEP, seed=28)
    n = len(ps)
    ids = np.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n)
    lens = [len(p) for p in ps]
    bad, want, want_skip = mu.failure_frames()
    good = [mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)]

    def run():
        return (ck.mac_batch_host(ks, ps), mgr.package_batch_host(ids, ids - 1, lens, ps),
                [mgr.verify_batch_host(good, mu.FIRST_ENTRY), mgr.verify_batch_host(bad, mu.FIRST_ENTRY),
                 mgr.verify_batch_host(bad, mu.FIRST_ENTRY, skip_entry_check=True)])

    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        assert ck.get_host_batch_route() == ck.HOST_ROUTE_GPU
        macs, (heads, hm), res = run()
        wide, _ = mgr.package_batch_host(ids, ids - 1, lens, ps, frame_stride=64)
        # an entry over the cap: refused on the forced GPU route
        with pytest.raises(_native.BkdError) as e:
            ck.mac_batch_host(ks, [b"abc", np.zeros(CAP + 1, dtype=np.uint8)])
        assert e.value.code == -1
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cmacs, (cheads, _), cpu = run()
    assert (cmacs == macs).all() and (cheads == heads).all()
    for (s, fb), (cs, cfb) in zip(res, cpu):
        assert s.tolist() == cs.tolist() and fb == cfb
    for i, p in enumerate(ps):
        assert macs[i].tobytes() == mu.mac_of(p), len(p)
        assert heads[i].tobytes() == good[i][:52] and hm[i].tobytes() == good[i][32:52]
    assert (wide[:, :52] == heads).all() and not wide[:, 52:].any()  # bytes 52.. are the wrapper's zeros
    assert res[0][1] == n and res[1][0].tolist() == want.tolist() and res[2][0].tolist() == want_skip.tolist()


def test_round_trip(gpu, mgr):
    """Frames from package_batch joined with their payloads verify with verify_batch, and equal
    computeDigestAndPackageForSending's first 52 bytes for the same ids."""
    import torch
    lens = [0, 1, 55, 56, 1000, 4096, 5000]
    ps = mu.payloads(lens, seed=29)
    n = len(ps)
    buf, off, ln = lay_out(ps, [None] * n)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = torch.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n, dtype=torch.int64, device=gpu)
    frames, _ = mgr.package_batch(ids, ids - 1, d_ln.to(torch.int64), d_buf, d_off, d_ln, sync_check=True)
    heads = frames.cpu().numpy()
    for i, p in enumerate(ps):
        assert heads[i].tobytes() == mgr.computeDigestAndPackageForSending(mu.FIRST_ENTRY + i, mu.FIRST_ENTRY + i - 1,
                                                                          len(p), p)[:52]
    fbuf, foff, fln = lay_out([heads[i].tobytes() + p for i, p in enumerate(ps)], [None] * n)
    d_fbuf, d_foff, d_fln = to_dev(gpu, fbuf, foff, fln)
    status, fb = mgr.verify_batch(d_fbuf, d_foff, d_fln, mu.FIRST_ENTRY)
    sync()
    assert status.cpu().numpy().tolist() == [0] * n and int(fb.item()) == n
