"""GPU: the MAC (HMAC-SHA1) calls where test_gpu_mac.py does not reach — host forms cut into several
staging segments (by bytes and by entry count), destinations that are not 4-byte aligned, non-default
streams and concurrent callers with keys of their own, header fields that use all 64 bits, ragged package
and verify batches, and addresses past 4 GiB. Every expectation is Python's hmac / hashlib / struct
through mac_util; every comparison is for equality."""
import ctypes
import threading

import numpy as np
import pytest

import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
CYCLE = [0, 1, 55, 56, 63, 64, 65, 119, 120, 300]  # SHA-1 padding edges with and without the 32-byte header


@pytest.fixture(scope="module")
def ks():
    return ck.mac_key_init(mu.PASSWD)


@pytest.fixture(scope="module")
def mgr():
    return dg.DigestManager.instantiate(mu.LEDGER, mu.PASSWD, dg.DigestType.HMAC)


def to_dev(gpu, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu) for a in arrays]
    assert out[0].data_ptr() % 16 == 0  # alignments in lay_out are the device addresses'
    return out


def sync(stream=None):
    import torch
    ck.stream_sync(torch.cuda.current_stream() if stream is None else stream)


def verify(m, gpu, frames, first, aligns=None, skip=False):
    """verify_batch over the frames laid out in one device buffer: (status list, first_bad)."""
    buf, off, ln = mu.lay_out(frames, aligns or [None] * len(frames), tail=5)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    status, fb = m.verify_batch(d_buf, d_off, d_ln, first, skip_entry_check=skip)
    sync()
    return status.cpu().numpy().tolist(), int(fb.item())


# ---- A. host forms across staging segments ----

@pytest.fixture(scope="module")
def seg():
    return mu.segment_batch()


def test_segment_fixture_spans_three_segments(seg):
    """What the tests below rely on, from byte counts alone: an entry with more than k * 64 MiB in front of
    it is not in the first k segments."""
    assert len(seg["payloads"]) == 4551 and int(seg["lens"].max()) <= mu.SEGMENT
    assert (seg["prefix"] > 2 * mu.SEGMENT).any()


def test_segments_mac_batch_host(gpu, ks, seg):
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        got = mu.check_segment_mac(ck, ks, seg)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        assert (ck.mac_batch_host(ks, seg["payloads"]) == got).all()


@pytest.fixture(scope="module")
def seg_pk(seg):
    return mu.segment_package(seg)


@pytest.mark.parametrize("stride", [52, 60])
def test_segments_package_batch_host(gpu, mgr, seg, seg_pk, stride):
    assert (seg_pk["lacs"] == -1).any() and int(seg_pk["ids"].max()) > 2**62 and int(seg_pk["lfs"].max()) > 2**62
    late = seg["prefix"] > 2 * mu.SEGMENT
    assert (seg_pk["lacs"][late] == -1).any() and (seg_pk["lacs"][late] > 2**32).any()
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        got = mu.check_segment_package(mgr, seg, seg_pk, stride)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cpu, _ = mgr.package_batch_host(seg_pk["ids"], seg_pk["lacs"], seg_pk["lfs"], seg["payloads"], frame_stride=stride)
    assert (cpu == got).all()


def test_segments_verify_batch_host(gpu, mgr, seg):
    """All good (fails if a segment's first index is not added to the first entry id); one failure of each
    kind past 128 MiB; one more past 64 MiB and one among the first hundred; entry ids not checked."""
    sv = mu.segment_verify(seg)
    for name, frames, first, skip, want in sv["cases"]:
        prefix = mu.prefix_bytes([len(f) for f in frames])
        assert max(len(f) for f in frames) <= mu.SEGMENT
        assert all(prefix[i] > 2 * mu.SEGMENT for i in sv["late"]), name
        assert mu.SEGMENT < prefix[sv["mid"]] and sv["early"] < 100
        big = [len(frames[i]) > 4 * mu.MIB for i in sv["late"]]
        assert any(big) and not all(big)
    names = [c[0] for c in sv["cases"]]
    assert sorted(sv["cases"][1][4][list(sv["late"])].tolist()) == [1, 2, 3, 4]
    assert mu.first_bad(sv["cases"][1][4]) == min(sv["late"]) and mu.first_bad(sv["cases"][2][4]) == sv["early"]
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        got = [mu.check_segment_verify(mgr, case) for case in sv["cases"]]
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        for name, (status, fb), (_, frames, first, skip, _w) in zip(names, got, sv["cases"]):
            cstatus, cfb = mgr.verify_batch_host(frames, first, skip_entry_check=skip)
            assert (cstatus == status).all() and cfb == fb, name


@pytest.fixture(scope="module")
def count():
    return mu.count_batch()


def test_entry_count_cut_mac_batch_host(gpu, ks, count):
    """2^20 + 300 entries under 64 MiB in all: only the entry-count rule cuts them, and the MACs of the
    entries behind the cut land behind the first 2^20 rows."""
    n, idx = count["n"], count["idx"]
    views, ptrs, lens = mu.host_pointers(count["payloads"])
    ptrs, lens = ptrs[idx], lens[idx]
    assert n > 1 << 20 and int(lens.sum()) <= mu.SEGMENT
    out = np.zeros((n, 20), dtype=np.uint8)
    vp = ctypes.c_void_p
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        _native.check(_native.lib().bkd_mac_batch_host(vp(ks.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), n,
                                                       vp(out.ctypes.data)))
    want = np.frombuffer(b"".join(count["macs"]), dtype=np.uint8).reshape(256, 20)[idx]
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, (bad[:5].tolist(), idx[bad[:5]].tolist())


def test_entry_count_cut_verify_batch_host(gpu, mgr, ks, count):
    """The same index as frames, entry ids not checked: status 0 everywhere but at the one planted frame
    past entry 2^20, which is first_bad."""
    n, idx, at = count["n"], count["idx"].copy(), count["bad_at"]
    idx[at] = 256  # the frame with a flipped payload byte
    views, ptrs, lens = mu.host_pointers(count["frames"])
    ptrs, lens = ptrs[idx], lens[idx]
    assert at > 1 << 20 and int(lens[:1 << 20].sum()) <= mu.SEGMENT
    status = np.full(n, -1, dtype=np.int32)
    fb = ctypes.c_uint64(0)
    vp = ctypes.c_void_p
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        _native.check(_native.lib().bkd_digest_verify_batch_mac_host(
            vp(ks.ctypes.data), mu.LEDGER, 0, 1, vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(status.ctypes.data),
            ctypes.byref(fb)))
    want = np.zeros(n, dtype=np.int32)
    want[at] = 2
    bad = np.flatnonzero(status != want)
    assert bad.size == 0, (bad[:5].tolist(), status[bad[:5]].tolist())
    assert fb.value == at


# ---- B. destinations that are not 4-byte aligned ----

@pytest.fixture(scope="module")
def cyc():
    ps = mu.payloads([CYCLE[i % len(CYCLE)] for i in range(130)], seed=41)
    return dict(ps=ps, frames=[mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)], macs=[mu.mac_of(p) for p in ps])


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("stride", [53, 54, 55, 57])
def test_package_into_unaligned_rows(gpu, mgr, cyc, stride, k):
    """out_frames starts k bytes into a buffer and its rows are `stride` apart, so rows start at every
    address modulo 4 (at strides 53 and 55 neighbouring lanes differ): 52 bytes per row are exact and every
    other byte of the buffer, in front, between and behind, keeps its sentinel."""
    import torch
    n = len(cyc["ps"])
    buf, off, ln = mu.lay_out(cyc["ps"], [None] * n)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = torch.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n, dtype=torch.int64, device=gpu)
    flat = torch.full((k + n * stride + 9,), SENTINEL, dtype=torch.uint8, device=gpu)
    assert flat.data_ptr() % 4 == 0
    view = flat[k:k + n * stride].view(n, stride)
    assert {(view.data_ptr() + i * stride) % 4 for i in range(n)} >= ({0, 1, 2, 3} if stride % 2 else {k % 2, k % 2 + 2})
    _, macs = mgr.package_batch(ids, ids - 1, d_ln.to(torch.int64), d_buf, d_off, d_ln, frame_stride=stride,
                                sync_check=True, out_frames=view)
    want = np.full(flat.numel(), SENTINEL, dtype=np.uint8)
    for i in range(n):
        want[k + i * stride:k + i * stride + 52] = np.frombuffer(cyc["frames"][i][:52], dtype=np.uint8)
    got = flat.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (stride, k, bad[:8].tolist())
    assert mu.wrong_rows(macs.cpu().numpy(), [f[32:52] for f in cyc["frames"]]) == []


@pytest.mark.parametrize("k", [1, 2, 3])
def test_mac_batch_into_unaligned_out(gpu, ks, cyc, k):
    import torch
    n = len(cyc["ps"])
    buf, off, ln = mu.lay_out(cyc["ps"], [None] * n)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    flat = torch.full((k + 20 * n + 9,), SENTINEL, dtype=torch.uint8, device=gpu)
    assert flat.data_ptr() % 4 == 0
    ck.mac_batch(ks, d_buf, d_off, d_ln, out=flat[k:k + 20 * n], sync_check=True)
    want = bytes([SENTINEL]) * k + b"".join(cyc["macs"]) + bytes([SENTINEL]) * 9
    got = flat.cpu().numpy()
    bad = np.flatnonzero(got != np.frombuffer(want, dtype=np.uint8))
    assert bad.size == 0, (k, bad[:8].tolist())


# ---- C. streams and threads ----

@pytest.mark.parametrize("call", ["mac_batch", "package_batch", "verify_batch"])
def test_bounds_flag_is_on_the_calls_stream(gpu, ks, mgr, call):
    """One entry with offset + length > size, on stream s1: s2's sync is clean, s1's raises BKD_ERR_BOUNDS
    once, and the entries around it are exact."""
    import torch
    ps = mu.payloads([100, 64, 300, 0, 77], seed=42)
    frames = [mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)]
    buf, off, ln = mu.lay_out(frames if call == "verify_batch" else ps, [None] * 5)
    ln[2] = buf.size - off[2] + 1  # one byte past the buffer
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = torch.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + 5, dtype=torch.int64, device=gpu)
    lf = torch.tensor([len(p) for p in ps], dtype=torch.int64, device=gpu)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    if call == "mac_batch":
        out = ck.mac_batch(ks, d_buf, d_off, d_ln, stream=s1)
    elif call == "package_batch":
        out, _ = mgr.package_batch(ids, ids - 1, lf, d_buf, d_off, d_ln, stream=s1)
    else:
        out, fb = mgr.verify_batch(d_buf, d_off, d_ln, mu.FIRST_ENTRY, stream=s1)
    ck.stream_sync(s2)  # another stream: no flag
    with pytest.raises(_native.BkdError) as e:
        ck.stream_sync(s1)
    assert e.value.code == -4  # BKD_ERR_BOUNDS
    ck.stream_sync(s1)  # reported once
    got = out.cpu().numpy()
    near = (0, 1, 3, 4)
    if call == "mac_batch":
        assert [got[i].tobytes() for i in near] == [mu.mac_of(ps[i]) for i in near] and not got[2].any()
    elif call == "package_batch":
        assert [got[i].tobytes() for i in near] == [frames[i][:52] for i in near]
        assert got[2].tobytes() == frames[2][:32] + bytes(20)  # the header is written, the MAC is not
    else:
        assert got.tolist() == [0, 0, 1, 0, 0] and int(fb.item()) == 2
    ck.release_stream(s1)
    ck.release_stream(s2)


def test_four_threads_four_keys(gpu):
    """Four host threads at once, each with its own stream, ledger key and manager: device package + verify,
    raw MACs, and the host forms (which share the staging sets), six rounds each, every result exact against
    that thread's key. Then thread 0's frames under thread 1's key: every MAC differs."""
    import torch
    passwords = [b"", b"a" * 20, bytes(range(100)), mu.PASSWD]
    ledgers = [77, 77, (1 << 40) + 3, mu.LEDGER]  # threads 0 and 1: the same ledger id, so only the key differs
    cyc = [0, 1, 700, 63, 64, 65, 3000]
    ps = mu.payloads([cyc[i % 7] for i in range(300)], seed=43)
    n = len(ps)
    buf, off, ln = mu.lay_out(ps, [(3 * i) % 16 for i in range(n)])
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = np.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n, dtype=np.int64)
    d_ids, = to_dev(gpu, ids)
    d_lf = d_ln.to(torch.int64)
    mgrs = [dg.DigestManager.instantiate(led, pw, dg.DigestType.HMAC) for led, pw in zip(ledgers, passwords)]
    keys = [mu.mac_key(pw) for pw in passwords]
    frames = [[mu.frame(int(ids[i]), p, ledger=led, key=key) for i, p in enumerate(ps)] for led, key in zip(ledgers, keys)]
    macs = [[mu.mac_of(p, key) for p in ps] for key in keys]
    fbuf, foff, fln = zip(*(mu.lay_out(f, [(5 * i) % 16 for i in range(n)]) for f in frames))
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            st = torch.cuda.Stream(device=gpu)
            m, mine = mgrs[k], frames[k]
            for r in range(6):
                kind = (k + r) % 3
                if kind == 0:
                    with torch.cuda.stream(st):
                        heads, hm = m.package_batch(d_ids, d_ids - 1, d_lf, d_buf, d_off, d_ln, stream=st)
                        d_f = [torch.from_numpy(a.copy()).to(gpu, non_blocking=False) for a in (fbuf[k], foff[k], fln[k])]
                        status, fb = m.verify_batch(*d_f, mu.FIRST_ENTRY, stream=st)
                        ck.stream_sync(st)
                        heads, hm = heads.cpu().numpy(), hm.cpu().numpy()
                        status, fb = status.cpu().numpy(), int(fb.item())
                    assert mu.wrong_rows(heads, [f[:52] for f in mine]) == [], ("package", k, r)
                    assert mu.wrong_rows(hm, [f[32:52] for f in mine]) == [], ("package macs", k, r)
                    assert not status.any() and fb == n, ("verify", k, r)
                elif kind == 1:
                    with torch.cuda.stream(st):
                        got = ck.mac_batch(m.key_state, d_buf, d_off, d_ln, stream=st)
                        ck.stream_sync(st)
                        got = got.cpu().numpy()
                    assert mu.wrong_rows(got, macs[k]) == [], ("mac_batch", k, r)
                else:
                    heads, hm = m.package_batch_host(ids, ids - 1, [len(p) for p in ps], ps)
                    assert mu.wrong_rows(heads, [f[:52] for f in mine]) == [], ("package host", k, r)
                    status, fb = m.verify_batch_host(mine, mu.FIRST_ENTRY)
                    assert not status.any() and fb == n, ("verify host", k, r)
            ck.release_stream(st)
        except BaseException as e:  # surfaced below
            errors.append((k, repr(e)))

    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        alive = [k for k, t in enumerate(threads) if t.is_alive()]
    assert not alive and not errors, (alive, errors)
    status, fb = verify(mgrs[1], gpu, frames[0], mu.FIRST_ENTRY)
    assert status == [2] * n and fb == 0


# ---- D. 64-bit header fields ----

@pytest.mark.parametrize("ledger", mu.WIDE_LEDGERS)
def test_wide_ids_package_and_verify(gpu, ledger):
    """Ledger ids, entry ids, LACs (-1 among them) and length fields with every high word: each packaged row
    is struct.pack(">qqqq", ...) + MAC; verify tells ids that differ in the high word only."""
    import torch
    m = dg.DigestManager.instantiate(ledger, mu.PASSWD, dg.DigestType.HMAC)
    w = mu.wide_ids()
    buf, off, ln = mu.lay_out(w["payloads"], [(7 * i) % 16 for i in range(len(w["payloads"]))])
    d_buf, d_off, d_ln, d_ids, d_lacs, d_lfs = to_dev(gpu, buf, off, ln, w["ids"], w["lacs"], w["lfs"])
    heads, macs = m.package_batch(d_ids, d_lacs, d_lfs, d_buf, d_off, d_ln, sync_check=True)
    assert mu.wrong_rows(heads.cpu().numpy(), w["heads"][ledger]) == []
    assert mu.wrong_rows(macs.cpu().numpy(), [h[32:] for h in w["heads"][ledger]]) == []
    for name, frames, first, want in mu.wide_verify_cases(ledger):
        status, fb = verify(m, gpu, frames, first, aligns=[(3 * i + 1) % 16 for i in range(len(frames))])
        assert status == want and fb == mu.first_bad(want), name


# ---- E. ragged package and verify ----

def test_ragged_package_and_verify(gpu, mgr):
    """The lengths 0, 1, 5000, 63, 64, 65, 65536 cycling over 257 lanes, through the kernels that hash the
    header in front of the payload: heads exact, frames verify, three planted failures found."""
    import torch
    cyc = [0, 1, 5000, 63, 64, 65, 65536]
    n = 257
    ps = mu.payloads([cyc[i % 7] for i in range(n)], seed=44)
    aligns = [(3 * i) % 16 for i in range(n)]
    frames = [mu.frame(mu.FIRST_ENTRY + i, p) for i, p in enumerate(ps)]
    buf, off, ln = mu.lay_out(ps, aligns)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    ids = torch.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n, dtype=torch.int64, device=gpu)
    heads, _ = mgr.package_batch(ids, ids - 1, d_ln.to(torch.int64), d_buf, d_off, d_ln, sync_check=True)
    assert mu.wrong_rows(heads.cpu().numpy(), [f[:52] for f in frames]) == []
    status, fb = verify(mgr, gpu, frames, mu.FIRST_ENTRY, aligns=aligns)
    assert status == [0] * n and fb == n
    i_long, i_one, i_empty = 6 + 7 * 20, 1 + 7 * 5, 7 * 30
    assert (len(ps[i_long]), len(ps[i_one]), len(ps[i_empty])) == (65536, 1, 0)
    bad = list(frames)
    for i in (i_long, i_one):  # the last payload byte of the long one, the only (= first) byte of the short one
        f = bytearray(frames[i])
        f[-1 if i == i_long else 52] ^= 0x80
        bad[i] = bytes(f)
    bad[i_empty] = mu.frame(mu.FIRST_ENTRY + i_empty, b"", ledger=mu.LEDGER + 1)
    want = [0] * n
    want[i_long], want[i_one], want[i_empty] = 2, 2, 3
    status, fb = verify(mgr, gpu, bad, mu.FIRST_ENTRY, aligns=aligns)
    assert status == want and fb == i_one


# ---- F. addresses past 4 GiB ----

def test_entries_around_and_past_4gib(gpu, ks, mgr):
    """Entries that end at byte 2^32, straddle it, start past it and end on the last byte of a buffer of
    4 GiB + 1 MiB: raw MACs and packaged heads against hmac over host copies, and frames at those
    offsets verify until a payload byte past 2^32 is flipped."""
    import torch
    four = 1 << 32
    size = four + (1 << 20)
    base = torch.empty(size, dtype=torch.uint8, device=gpu)
    w0, w1 = four - 4096, four + 8192  # every entry but the last lies in [w0, w1)
    t0 = size - 1024
    rng = np.random.default_rng(45)
    win, tail = rng.integers(0, 256, w1 - w0, dtype=np.uint8), rng.integers(0, 256, 1024, dtype=np.uint8)
    base[w0:w1].copy_(torch.from_numpy(win))
    base[t0:].copy_(torch.from_numpy(tail))
    offs = np.array([four - 1000, four - 7, four - 7, four + 5, size - 333], dtype=np.int64)
    lens = np.array([1000, 300, 5000, 777, 333], dtype=np.int32)
    assert offs[0] + lens[0] == four and offs[4] + lens[4] == size
    n = len(offs)

    def host(i):
        o, l = int(offs[i]), int(lens[i])
        return (tail[o - t0:o - t0 + l] if o >= t0 else win[o - w0:o - w0 + l]).tobytes()

    ps = [host(i) for i in range(n)]
    d_off, d_ln = to_dev(gpu, offs, lens)
    macs = ck.mac_batch(ks, base, d_off, d_ln, sync_check=True).cpu().numpy()
    assert mu.wrong_rows(macs, [mu.mac_of(p) for p in ps]) == []
    ids = torch.arange(mu.FIRST_ENTRY, mu.FIRST_ENTRY + n, dtype=torch.int64, device=gpu)
    heads, _ = mgr.package_batch(ids, ids - 1, d_ln.to(torch.int64), base, d_off, d_ln, sync_check=True)
    assert mu.wrong_rows(heads.cpu().numpy(), [mu.frame(mu.FIRST_ENTRY + i, p)[:52] for i, p in enumerate(ps)]) == []
    # frames of the same sizes at the same offsets; those that overlap take turns. `flip`: a payload byte past 2^32
    for group, flip in (((0, 3, 4), four + 5 + 60), ((1, 4), four + 100), ((2, 4), four + 4000)):
        frames = [mu.frame(mu.FIRST_ENTRY + j, ps[i][:len(ps[i]) - 52]) for j, i in enumerate(group)]
        for f, i in zip(frames, group):
            o = int(offs[i])
            base[o:o + len(f)].copy_(torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()))
        g_off, g_ln = to_dev(gpu, offs[list(group)], lens[list(group)])
        hit = [j for j, i in enumerate(group) if offs[i] + 52 <= flip < offs[i] + lens[i]]
        assert len(hit) == 1 and flip >= four
        for want in ([0] * len(group), [2 if j == hit[0] else 0 for j in range(len(group))]):
            status, fb = mgr.verify_batch(base, g_off, g_ln, mu.FIRST_ENTRY)
            sync()
            assert status.cpu().numpy().tolist() == want and int(fb.item()) == mu.first_bad(want), (group, want)
            base[flip] ^= 0x04
