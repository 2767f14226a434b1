"""GPU: the MAC calls that span ledgers — verify_requests_mac and package_batch_ledgers_mac, device-resident
and through the host forms' GPU route — bit for bit against Python's hmac."""
import numpy as np
import pytest

import mac_requests_util as mq
import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

BOUNDS = -4  # BKD_ERR_BOUNDS


def to_dev(gpu, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu) for a in arrays]
    assert out[0].data_ptr() % 16 == 0  # alignments in lay_out are the device addresses'
    return out


def dev_table(gpu, passwords):
    """The key table on the device: exactly nkeys rows, nothing behind them that a test could depend on."""
    import torch
    table = dg.mac_key_table(passwords)
    t = torch.from_numpy(table.view(np.int32).copy()).to(gpu)
    assert t.numel() == 10 * len(passwords)
    return t


def sync(stream=None):
    import torch
    ck.stream_sync(torch.cuda.current_stream() if stream is None else stream)


def sync_raises_bounds_once(stream=None):
    with pytest.raises(_native.BkdError) as e:
        sync(stream)
    assert e.value.code == BOUNDS
    sync(stream)


def verify(gpu, b, frames=None, aligns=None, table=None, first=None, stream=None, check=True):
    """verify_requests_mac over b's frames laid out in one device buffer: (status, prefix) as numpy arrays
    once the stream's sync came back clean (`check`)."""
    frames = b.frames if frames is None else frames
    buf, off, ln = mu.lay_out(frames, aligns or [None] * len(frames), tail=5)
    d_buf, d_off, d_ln = to_dev(gpu, buf, off, ln)
    d_first, d_lids, d_firsts, d_keys, d_flags = to_dev(gpu, b.first if first is None else first, b.lids, b.firsts,
                                                        b.req_keys, b.flags)
    table = dev_table(gpu, b.passwords()) if table is None else table
    status, prefix = dg.verify_requests_mac(table, d_keys, d_buf, d_off, d_ln, d_first, d_lids, d_firsts, d_flags,
                                            stream=stream)
    if not check:
        return status, prefix  # device tensors: the caller syncs the stream, then reads them
    sync(stream)
    return status.cpu().numpy(), prefix.cpu().numpy()


# ---- CSR shapes ----

@pytest.mark.parametrize("shape", list(mq.CSR_SHAPES))
def test_csr_shapes(gpu, shape):
    b = mq.Requests(mq.CSR_SHAPES[shape], seed=3)
    status, prefix = verify(gpu, b)
    assert (status == 0).all() and prefix.tolist() == b.sizes
    if b.n == 0:
        return
    # one failure of each id kind and a flipped byte, spread over the requests
    b.lids[b.req_of(0)] ^= 1 << 32
    b.firsts[b.req_of(b.n - 1)] += 1 << 32
    mid = b.n // 2
    b.frames[mid] = b.frames[mid][:40] + bytes([b.frames[mid][40] ^ 4]) + b.frames[mid][41:]
    want, want_prefix = b.expected()
    assert want.any()
    status, prefix = verify(gpu, b)
    assert (status == want).all() and (prefix == want_prefix).all()


def test_request_boundaries_at_wave_and_block_edges(gpu):
    """600 frames of 52..400 bytes; requests end at entries 63, 64, 65, 255, 256, 257 (wave and block
    edges): each request has its own key, ledger and first entry id, so an entry that took its
    neighbour's request fails on all three."""
    cuts = [0, 63, 64, 65, 255, 256, 257, 600]
    sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    b = mq.Requests(sizes, seed=12)
    assert min(len(f) for f in b.frames) >= 52 and max(len(f) for f in b.frames) <= 400
    status, prefix = verify(gpu, b)
    assert np.flatnonzero(status).tolist() == [] and prefix.tolist() == sizes
    # a failure in the last entry of each request and in the first of the next: per-request prefixes
    for r in range(1, b.nreq, 2):
        last = int(b.first[r + 1]) - 1
        b.frames[last] = b.frames[last][:-1] + bytes([b.frames[last][-1] ^ 0x80]) if len(b.frames[last]) > 52 \
            else b.frames[last][:51]
    want, want_prefix = b.expected()
    status, prefix = verify(gpu, b)
    assert (status == want).all() and (prefix == want_prefix).all()
    assert [int(p) for p in want_prefix[1::2]] == [s - 1 for s in sizes[1::2]]


# ---- the key is the request's ----

def test_key_is_per_request(gpu):
    lens = [0, 1, 63, 64, 200] * 2
    b = mq.Requests([5, 5], lengths=lens, seed=5)
    b.payloads[5:] = b.payloads[:5]
    b.lids[1], b.firsts[1] = b.lids[0], b.firsts[0]
    b.frames[5:] = [mu.frame(mq.first_entry(0) + j, b.payloads[j], ledger=mq.ledger(0), key=mq.key(1)) for j in range(5)]
    assert all(x[:32] == y[:32] and x[52:] == y[52:] and x[32:52] != y[32:52] for x, y in zip(b.frames[:5], b.frames[5:]))
    status, prefix = verify(gpu, b)
    assert (status == 0).all() and prefix.tolist() == [5, 5]
    b.req_keys[:] = [1, 0]  # swapped: every entry of both requests fails on its MAC
    status, prefix = verify(gpu, b)
    assert (status == 2).all() and prefix.tolist() == [0, 0]
    b.req_keys[:] = [0, 0]  # two requests share one row
    status, prefix = verify(gpu, b, frames=b.frames[:5] * 2)
    assert (status == 0).all() and prefix.tolist() == [5, 5]


# ---- failure kinds and precedence inside a request ----

@pytest.mark.parametrize("skip", [0, 1])
def test_failure_kinds_inside_a_request(gpu, skip):
    bad, want, want_skip = mu.failure_frames()
    b = mq.Requests([70, 0, len(bad), 7], seed=6, keys=[1, 2, 0, 3])
    lo = int(b.first[2])
    table = dev_table(gpu, [mu.PASSWD] + b.passwords()[1:])  # failure_frames() are keyed with mac_util's password
    b.frames[lo:lo + len(bad)] = bad
    b.lids[2], b.firsts[2], b.flags[2] = mu.LEDGER, mu.FIRST_ENTRY, skip
    exp = want_skip if skip else want
    status, prefix = verify(gpu, b, table=table)
    assert status[lo:lo + len(bad)].tolist() == exp.tolist()
    assert not status[:lo].any() and not status[lo + len(bad):].any()  # untouched neighbours
    assert prefix.tolist() == [70, 0, mu.first_bad(exp), 7] and mu.first_bad(exp) == 1
    # the skip flag is the request's own: the neighbour with entry ids off by one fails without it
    b.firsts[3] += 1
    for flag, code, pre in ((0, 4, 0), (1, 0, 7)):
        b.flags[3] = flag
        status, prefix = verify(gpu, b, table=table)
        assert (status[int(b.first[3]):] == code).all() and prefix.tolist() == [70, 0, 1, pre]
        assert status[lo:lo + len(bad)].tolist() == exp.tolist()


@pytest.mark.parametrize("ledger", mu.WIDE_LEDGERS)
def test_wide_ids(gpu, ledger):
    cases = mu.wide_verify_cases(ledger)
    b = mq.Requests([len(c[1]) for c in cases], seed=1, keys=[1] * len(cases), nkeys=2)
    b.frames = [f for c in cases for f in c[1]]
    b.lids[:] = ledger
    b.firsts[:] = [c[2] for c in cases]
    status, prefix = verify(gpu, b, table=dev_table(gpu, [b"unused", mu.PASSWD]))
    assert status.tolist() == [s for c in cases for s in c[3]]
    assert prefix.tolist() == [mu.first_bad(c[3]) for c in cases]


# ---- alignment ----

def test_frame_starts_at_every_address_modulo_four(gpu):
    """Payload lengths 0..130 at frame starts 0..3 modulo 4 (and modulo 16 through lay_out), requests of
    irregular sizes; 0xEE between the frames."""
    lens = [n for _ in range(4) for n in range(131)]
    aligns = [(4 * (i % 3) + a) % 16 for a in range(4) for i in range(131)]
    assert {a % 4 for a in aligns} == {0, 1, 2, 3}
    sizes = []
    while sum(sizes) < len(lens):
        sizes.append(min(len(lens) - sum(sizes), (7 * len(sizes)) % 23))
    b = mq.Requests(sizes, lengths=lens, seed=13)
    status, prefix = verify(gpu, b, aligns=aligns)
    assert np.flatnonzero(status).tolist() == [] and prefix.tolist() == b.sizes
    flipped = [f[:-1] + bytes([f[-1] ^ 1]) for f in b.frames]  # every last byte counts, at every alignment
    status, _ = verify(gpu, b, frames=flipped, aligns=aligns)
    assert (status == 2).all()


# ---- key indices outside the table ----

@pytest.mark.parametrize("bad_key", ["nkeys", "0xFFFFFFFF"])
def test_key_index_outside_the_table(gpu, bad_key):
    b = mq.Requests([9, 6, 80, 5], seed=14)
    bad = b.nkeys if bad_key == "nkeys" else -1  # int32 -1 is uint32 0xFFFFFFFF
    b.req_keys[1] = bad
    lo, hi = int(b.first[1]), int(b.first[2])
    want = np.zeros(b.n, dtype=np.int32)
    want[lo:hi] = 1
    status, prefix = verify(gpu, b, check=False)
    sync_raises_bounds_once()
    assert (status.cpu().numpy() == want).all() and prefix.cpu().tolist() == [9, 0, 80, 5]
    # package: the header and a zero MAC for those entries, everything else exact
    f = mq.package_fields(b.n, b.nkeys, seed=15)
    f["key_of"][lo:hi] = bad
    heads = mq.package_heads(dict(f, key_of=np.where(f["key_of"] == bad, 0, f["key_of"])), b.payloads)
    buf, off, ln = mu.lay_out(b.payloads, [None] * b.n)
    d_buf, d_off, d_ln, d_key_of, d_lids, d_ids, d_lacs, d_lfs = to_dev(
        gpu, buf, off, ln, f["key_of"], f["lids"], f["ids"], f["lacs"], f["lfs"])
    frames, macs = dg.package_batch_ledgers_mac(dev_table(gpu, b.passwords()), d_key_of, d_lids, d_ids, d_lacs, d_lfs,
                                                d_buf, d_off, d_ln)
    sync_raises_bounds_once()
    frames = frames.cpu().numpy()
    for i in range(b.n):
        want_i = heads[i][:32] + bytes(20) if lo <= i < hi else heads[i]
        assert frames[i].tobytes() == want_i, i


# ---- malformed CSR: only the bounds flag is asserted ----

@pytest.mark.parametrize("first", [[0, 10, 8, 30, 40], [1, 10, 20, 30, 40], [0, 10, 20, 30, 39]],
                         ids=["decreases in the middle", "first is not 0", "last is not n"])
def test_malformed_csr_raises_the_bounds_flag(gpu, first):
    b = mq.Requests([10, 10, 10, 10], seed=16)
    assert all(0 <= v <= b.n for v in first)
    verify(gpu, b, first=np.array(first, dtype=np.int64), check=False)
    sync_raises_bounds_once()
    status, prefix = verify(gpu, b)  # the stream and the scratch are fine afterwards
    assert not status.any() and prefix.tolist() == b.sizes


# ---- package ----

@pytest.mark.parametrize("stride", [52, 64])
def test_package_ledgers(gpu, stride):
    import torch
    n, nkeys = 300, 11
    ps = mu.payloads([(37 * r) % 211 for r in range(n)], seed=33)
    ps[5] = ps[4]  # the same payload and header fields under two rows below
    f = mq.package_fields(n, nkeys)
    for name in ("lids", "ids", "lacs", "lfs"):
        f[name][5] = f[name][4]
    f["key_of"][4:6] = [2, 3]
    heads = mq.package_heads(f, ps)
    assert heads[4][:32] == heads[5][:32] and heads[4][32:] != heads[5][32:]
    buf, off, ln = mu.lay_out(ps, [(3 * i) % 16 for i in range(n)])
    d_buf, d_off, d_ln, d_key_of, d_lids, d_ids, d_lacs, d_lfs = to_dev(
        gpu, buf, off, ln, f["key_of"], f["lids"], f["ids"], f["lacs"], f["lfs"])
    table = dev_table(gpu, [mq.password(k) for k in range(nkeys)])
    frames, macs = dg.package_batch_ledgers_mac(table, d_key_of, d_lids, d_ids, d_lacs, d_lfs, d_buf, d_off, d_ln,
                                                frame_stride=stride, sync_check=True)
    assert frames.shape == (n, stride) and macs.shape == (n, 20)
    assert mu.wrong_rows(frames.cpu().numpy()[:, :52], heads) == []
    assert (macs.cpu() == frames.cpu()[:, 32:52]).all()
    # only 52 bytes of a stride are written: the same call into a prefilled frame array through the C call
    out = torch.full((n, stride), 0xA5, dtype=torch.uint8, device=gpu)
    st = torch.cuda.current_stream()
    _native.check(_native.lib().bkd_digest_package_batch_ledgers_mac(
        table.data_ptr(), nkeys, d_key_of.data_ptr(), d_lids.data_ptr(), d_ids.data_ptr(), d_lacs.data_ptr(),
        d_lfs.data_ptr(), d_buf.data_ptr(), d_buf.numel(), d_off.data_ptr(), d_ln.data_ptr(), n, out.data_ptr(), stride,
        st.cuda_stream))
    sync()
    out = out.cpu().numpy()
    assert mu.wrong_rows(out[:, :52], heads) == [] and (out[:, 52:] == 0xA5).all()


def test_package_unreadable_payloads_still_get_their_header(gpu):
    """One payload past the end of the buffer and one over the cap: header written, MAC zero, the flag raised."""
    ps = mu.payloads([100, 64, 300, 0, 77], seed=42)
    f = mq.package_fields(5, 3, seed=17)
    heads = mq.package_heads(f, ps)
    buf, off, ln = mu.lay_out(ps, [None] * 5)
    ln[2] = buf.size - off[2] + 1
    ln[4] = _native.MAC_MAX_ENTRY + 1
    d_buf, d_off, d_ln, d_key_of, d_lids, d_ids, d_lacs, d_lfs = to_dev(
        gpu, buf, off, ln, f["key_of"], f["lids"], f["ids"], f["lacs"], f["lfs"])
    frames, _ = dg.package_batch_ledgers_mac(dev_table(gpu, [mq.password(k) for k in range(3)]), d_key_of, d_lids,
                                             d_ids, d_lacs, d_lfs, d_buf, d_off, d_ln)
    sync_raises_bounds_once()
    got = frames.cpu().numpy()
    assert [got[i].tobytes() for i in (0, 1, 3)] == [heads[i] for i in (0, 1, 3)]
    assert [got[i].tobytes() for i in (2, 4)] == [heads[i][:32] + bytes(20) for i in (2, 4)]


def test_round_trip_across_37_ledgers(gpu):
    """Package 37 requests' entries, lay the frames out with their payloads, verify them as requests."""
    sizes = [(5 * r) % 13 for r in range(37)]
    b = mq.Requests(sizes, seed=18)
    key_of, lids = np.repeat(b.req_keys, b.sizes), np.repeat(b.lids, b.sizes)
    ids = np.array([mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]) for i in range(b.n)], dtype=np.int64)
    buf, off, ln = mu.lay_out(b.payloads, [None] * b.n)
    d_buf, d_off, d_ln, d_key_of, d_lids, d_ids = to_dev(gpu, buf, off, ln, key_of, lids, ids)
    table = dev_table(gpu, b.passwords())
    heads, _ = dg.package_batch_ledgers_mac(table, d_key_of, d_lids, d_ids, d_ids - 1, d_ln.to(d_ids.dtype), d_buf,
                                            d_off, d_ln, sync_check=True)
    heads = heads.cpu().numpy()
    frames = [heads[i].tobytes() + b.payloads[i] for i in range(b.n)]
    assert frames == b.frames  # what hmac makes of the same entries
    status, prefix = verify(gpu, b, frames=frames, table=table)
    assert not status.any() and prefix.tolist() == sizes


# ---- host forms with the GPU route forced ----

def host_both_routes(call):
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        got = call()
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cpu = call()
    for g, c in zip(got, cpu):
        assert g.tobytes() == c.tobytes()  # byte-equal outputs on both routes
    return got


@pytest.mark.parametrize("shape", list(mq.CSR_SHAPES))
def test_host_forms_csr_shapes(gpu, shape):
    b = mq.Requests(mq.CSR_SHAPES[shape], seed=19)
    if b.n:
        b.frames[b.n // 2] = b.frames[b.n // 2][:51]
        b.lids[b.req_of(0)] += 1
    want, want_prefix = b.expected()
    table = dg.mac_key_table(b.passwords())
    status, prefix = host_both_routes(lambda: dg.verify_requests_mac_host(table, b.req_keys, b.frames, b.first, b.lids,
                                                                          b.firsts, b.flags))
    assert (status == want).all() and (prefix.astype(np.int64) == want_prefix).all()
    key_of, lids = np.repeat(b.req_keys, b.sizes), np.repeat(mq.Requests(b.sizes).lids, b.sizes)
    ids = np.array([mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]) for i in range(b.n)], dtype=np.int64)
    for stride in (52, 64):
        frames, macs = host_both_routes(lambda: dg.package_batch_ledgers_mac_host(
            table, key_of, lids, ids, ids - 1, [len(p) for p in b.payloads], b.payloads, frame_stride=stride))
        good = mq.Requests(b.sizes, seed=19).frames
        assert frames.shape == (b.n, stride) and not frames[:, 52:].any()
        assert b.n == 0 or mu.wrong_rows(frames[:, :52], [f[:52] for f in good]) == []


@pytest.fixture(scope="module")
def straddle():
    """mac_util.segment_batch() (views into one blob, 181.5 MiB, three staged segments) cut into requests of
    197 entries with a key each, as frames; the requests that straddle 64 MiB by prefix_bytes alone."""
    seg = mu.segment_batch()
    n = len(seg["payloads"])
    sizes = [197] * (n // 197) + [n % 197]
    b = mq.Requests(sizes, lengths=[0] * n, seed=20)
    b.payloads = seg["payloads"]
    b.frames = [mu.frame(mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]), p, ledger=mq.ledger(b.req_of(i)),
                         key=mq.key(b.req_of(i))) for i, p in enumerate(seg["payloads"])]
    prefix = mu.prefix_bytes([len(f) for f in b.frames])
    assert int(prefix[-1]) > 2 * mu.SEGMENT and max(len(f) for f in b.frames) <= mu.SEGMENT
    across = [r for r in range(b.nreq) if b.sizes[r] and prefix[b.first[r]] < mu.SEGMENT < prefix[b.first[r + 1] - 1]]
    assert len(across) == 1
    return b, prefix, across[0]


def test_host_verify_request_straddles_a_staging_cut(gpu, straddle):
    b, prefix, r = straddle
    lo, hi = int(b.first[r]), int(b.first[r + 1])
    # on the CPU, before the call: the request has entries on both sides of 64 MiB, and the failure is
    # planted in one that cannot lie in the first segment
    later = [i for i in range(lo, hi) if prefix[i] > mu.SEGMENT and len(b.frames[i]) > 52]
    assert prefix[lo] < mu.SEGMENT and later and later[0] > lo
    at = later[len(later) // 2]
    frames = list(b.frames)
    frames[at] = frames[at][:-1] + bytes([frames[at][-1] ^ 2])
    late = next(i for i in range(b.n - 1, 0, -1) if prefix[i] > 2 * mu.SEGMENT and len(frames[i]) > 100)
    frames[late] = frames[late][:60]  # and one more in a third segment or later: a digest mismatch
    want = np.zeros(b.n, dtype=np.int32)
    want[[at, late]] = 2
    want_prefix = np.array(b.sizes, dtype=np.int64)
    want_prefix[r] = at - lo
    want_prefix[b.req_of(late)] = late - int(b.first[b.req_of(late)])
    assert 0 < want_prefix[r] < b.sizes[r]
    table = dg.mac_key_table(b.passwords())
    status, got_prefix = host_both_routes(lambda: dg.verify_requests_mac_host(table, b.req_keys, frames, b.first, b.lids,
                                                                              b.firsts))
    assert np.flatnonzero(status != want).tolist() == []
    assert got_prefix.astype(np.int64).tolist() == want_prefix.tolist()  # the later index, not the entry count


def test_host_package_across_staging_cuts(gpu, straddle):
    b, prefix, _ = straddle
    key_of, lids = np.repeat(b.req_keys, b.sizes), np.repeat(b.lids, b.sizes)
    ids = np.array([mq.first_entry(b.req_of(i)) + i - int(b.first[b.req_of(i)]) for i in range(b.n)], dtype=np.int64)
    table = dg.mac_key_table(b.passwords())
    frames, macs = host_both_routes(lambda: dg.package_batch_ledgers_mac_host(
        table, key_of, lids, ids, ids - 1, [len(p) for p in b.payloads], b.payloads, frame_stride=60))
    assert mu.wrong_rows(frames[:, :52], [f[:52] for f in b.frames]) == [] and not frames[:, 52:].any()
    assert (macs == frames[:, 32:52]).all()


# ---- streams ----

def test_two_streams_and_the_flag_is_the_calls_streams(gpu):
    import torch
    b1, b2 = mq.Requests([30, 40, 3], seed=21), mq.Requests([5, 66], seed=22)
    b1.req_keys[1] = b1.nkeys  # outside the table, on stream s1 only
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    st1, pre1 = verify(gpu, b1, stream=s1, check=False)
    st2, pre2 = verify(gpu, b2, stream=s2, check=False)
    ck.stream_sync(s2)  # clean
    sync_raises_bounds_once(s1)
    st1, pre1, st2, pre2 = (t.cpu().numpy() for t in (st1, pre1, st2, pre2))
    assert st1[:30].tolist() == [0] * 30 and (st1[30:70] == 1).all() and not st1[70:].any()
    assert pre1.tolist() == [30, 0, 3] and not st2.any() and pre2.tolist() == [5, 66]
    ck.release_stream(s1)
    ck.release_stream(s2)
