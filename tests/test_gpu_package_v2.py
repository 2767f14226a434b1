"""GPU: V2 add requests packaged whole on the device (bkd_digest_package_batch_v2) and through the host
form's GPU route.

Every byte of the request buffer is compared: the requests with v2_util.expected_requests (struct.pack
prefix, key, the oracle's header and digest, the payload), everything else — the 1 .. 19 bytes between
requests, the room behind the digest of an entry at or over the threshold, the buffer's ends — with the
0xA5 it was filled with. The device sequence is the digests as package_batch computes them, then
package_v2_head_kernel and package_v2_copy_kernel<G>; a forced lane width is the copy kernel's too.
"""
import contextlib

import numpy as np
import pytest

import oracle
import v2_util as vu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}
LANES = (4, 8, 16, 32, 64)
LEAD = 64  # sentinel bytes in front of the first request and behind the last


@contextlib.contextmanager
def _forced(lanes):
    try:
        ck.set_group_lanes(lanes)
        yield
    finally:
        ck.set_group_lanes(0)


def _dev(torch, a, gpu):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    assert t.data_ptr() % 256 == 0  # the placement's residues are the addresses' residues
    return t


def _same(got, want, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def sweep_lengths(G):
    """0 .. 2 S + 19 at G = 4 and 8; 0 .. 40 and m S - 19 .. m S + 19 for m = 1 .. 3 above (S = 16 G)."""
    S = 16 * G
    if G <= 8:
        return np.arange(0, 2 * S + 20, dtype=np.int64)
    return np.concatenate([np.arange(0, 41)] + [np.arange(m * S - 19, m * S + 20) for m in (1, 2, 3)]).astype(np.int64)


def place_payloads(plens, a):
    """Payload i starts at a byte = (5 i + a) mod 16, in a slot of whole 16-byte blocks."""
    n = len(plens)
    r = (5 * np.arange(n, dtype=np.int64) + a) % 16
    slot = (r + plens + 15) // 16 * 16
    return np.cumsum(slot) - slot + r, int(slot.sum())


def place_requests(rlens, b, room=None):
    """Request i starts at a byte = (7 i + b) mod 16, the first LEAD bytes into the buffer, each 1 .. 16
    bytes behind the room of the one before (`room`: the bytes kept for request i, its length unless a
    payload that must not be copied gets room too); (offsets, buffer size)."""
    room = rlens if room is None else room
    offs = np.empty(len(rlens), dtype=np.int64)
    end = LEAD - 1
    for i in range(len(rlens)):
        want = (7 * i + b) % 16
        offs[i] = end + 1 + (want - (end + 1)) % 16
        end = int(offs[i] + room[i])
    gaps = offs[1:] - (offs[:-1] + room[:-1])
    assert ((gaps >= 1) & (gaps <= 19)).all()
    return offs, end + LEAD


def want_buffer(size, roffs, want):
    buf = np.full(size, vu.SENTINEL, dtype=np.uint8)
    for o, w in zip(roffs.tolist(), want):
        buf[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
    return buf


def run_device(torch, gpu, algo, ledgers, ids, lacs, lenf, d_blob, poffs, plens, keys, key_stride, flags, small, roffs,
               rsize, stream=None, sync=True):
    """package_batch_v2 (one ledger: the DigestManager method; per-entry ids: the module form) into a
    buffer of rsize sentinel bytes: (the buffer, digests uint32[n]) on the host."""
    req = torch.full((rsize,), vu.SENTINEL, dtype=torch.uint8, device=gpu)
    d_key = bytes(keys) if key_stride == 0 else _dev(torch, keys, gpu)
    args = [_dev(torch, x, gpu) for x in (ids, lacs, lenf)] + [d_blob, _dev(torch, poffs, gpu),
                                                               _dev(torch, plens.astype(np.int32), gpu), d_key]
    kw = dict(key_stride=key_stride or None, flags=flags, small_threshold=small, requests=req,
              request_offsets=_dev(torch, roffs, gpu), stream=stream, sync_check=sync)
    if np.ndim(ledgers):
        got_req, _, digests = dg.package_batch_v2(DTYPE[algo], _dev(torch, ledgers, gpu), *args, **kw)
    else:
        dm = dg.DigestManager.instantiate(int(ledgers), b"", DTYPE[algo], True)
        got_req, _, digests = dm.package_batch_v2(*args, **kw)
    assert got_req is req
    return req, digests


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
@pytest.mark.parametrize("lanes", LANES)
def test_alignment_sweep(gpu, lanes, algo):
    """Every payload length class at every (source, destination) residue pair mod 16."""
    import torch
    plens = sweep_lengths(lanes)
    n = plens.size
    small = int(plens.max()) + 1  # every entry is copied
    ledgers, ids, lacs, lenf = vu.ids_for(n, lanes + algo, lanes % 3 == 1)
    key_stride = 20 if np.ndim(ledgers) else 0
    keys = vu.keys_for(n, key_stride, lanes)
    rlens = vu.head_len(algo) + plens
    pairs = set()
    with _forced(lanes):
        for b in range(16):
            a = (2 * b) % 16
            poffs, psize = place_payloads(plens, a)
            blob = oracle.fill_splitmix64(psize, 31 * lanes + algo)  # the same stream: other bytes per placement
            want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, key_stride, 0,
                                                small)
            roffs, rsize = place_requests(rlens, b)
            req, digests = run_device(torch, gpu, algo, ledgers, ids, lacs, lenf, _dev(torch, blob, gpu), poffs, plens,
                                      keys, key_stride, 0, small, roffs, rsize)
            _same(digests.cpu().numpy().view(np.uint32), want_d, ("digests", b))
            _same(req.cpu().numpy(), want_buffer(rsize, roffs, want), ("request buffer", b))
            long = plens >= 33
            pairs |= set(zip((poffs[long] % 16).tolist(), ((roffs[long] + vu.head_len(algo)) % 16).tolist()))
    assert len(pairs) == 256  # every source residue met every destination residue at a length >= 33


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_threshold(gpu, algo):
    """Entries one under, at and one over the threshold mixed in one batch, at a small threshold and at
    the reference's 16 384: those at or over it get their 60 + mac bytes only. Automatic lanes."""
    import torch
    for small, plens in ((256, np.array([255, 256, 257, 0, 255, 300, 257, 256, 255, 1, 4000], dtype=np.int64)),
                         (dg.SMALL_ENTRY_SIZE_THRESHOLD, np.array([16383, 16384, 16383, 16384, 5], dtype=np.int64))):
        n = plens.size
        ledgers, ids, lacs, lenf = vu.ids_for(n, small + algo, False)
        keys = vu.keys_for(n, 0, 3)
        poffs, psize = place_payloads(plens, 3)
        blob = oracle.fill_splitmix64(psize, small)
        want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, 0, 0, small)
        assert [len(w) - vu.head_len(algo) for w in want] == [l if l < small else 0 for l in plens.tolist()]
        roffs, rsize = place_requests(vu.head_len(algo) + np.where(plens < small, plens, 0), 5,
                                      room=vu.head_len(algo) + plens)
        req, digests = run_device(torch, gpu, algo, ledgers, ids, lacs, lenf, _dev(torch, blob, gpu), poffs, plens,
                                  keys, 0, 0, small, roffs, rsize)
        _same(digests.cpu().numpy().view(np.uint32), want_d, ("digests", small))
        _same(req.cpu().numpy(), want_buffer(rsize, roffs, want), ("request buffer", small))


def test_ragged_batch_plan_and_direct_modes(gpu):
    """A ragged batch (lengths 0 .. 70 000) with the indexed strategy forced to the chunked plan and to
    one entry per group, the payload buffer's base 0 and 7 bytes off a 256-byte boundary: the same
    requests whatever the strategy (package_framed, whose digests these are, folds every batch one entry
    per group: the mode does not reach it)."""
    import torch
    algo, small = ck.CRC32C, dg.SMALL_ENTRY_SIZE_THRESHOLD
    rng = np.random.default_rng(17)
    n = 2048
    plens = np.where(rng.random(n) < 0.8, rng.integers(0, 2000, n), rng.integers(0, 70001, n)).astype(np.int64)
    plens[:4] = [0, 70000, small - 1, small]
    ledgers, ids, lacs, lenf = vu.ids_for(n, 5, True)
    keys = vu.keys_for(n, 24, 5)
    poffs, psize = place_payloads(plens, 9)
    blob = oracle.fill_splitmix64(psize, 23)
    want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, 24, 0x00FF, small)
    roffs, rsize = place_requests(vu.head_len(algo) + np.where(plens < small, plens, 0), 11)
    wantbuf = want_buffer(rsize, roffs, want)
    for mis in (0, 7):
        d_blob = torch.empty(psize + mis, dtype=torch.uint8, device=gpu)
        d_blob[mis:] = torch.from_numpy(blob).to(gpu)
        for mode in (2, 1):
            with ck.plan_mode(mode):
                req, digests = run_device(torch, gpu, algo, ledgers, ids, lacs, lenf, d_blob[mis:], poffs, plens, keys,
                                          24, 0x00FF, small, roffs, rsize)
            _same(digests.cpu().numpy().view(np.uint32), want_d, ("digests", mis, mode))
            _same(req.cpu().numpy(), wantbuf, ("request buffer", mis, mode))


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_ids_keys_and_flags(gpu, algo):
    """Per-entry 64-bit ledger ids with per-entry keys (key_stride 20 and 24) against one ledger with one
    key (key_stride 0); flags 0xFFFF and 0; a forced one-lane geometry (the header-first package route,
    its frames in the stream's scratch)."""
    import torch
    plens = np.concatenate([np.arange(0, 70), [500, 1000]]).astype(np.int64)
    n = plens.size
    poffs, psize = place_payloads(plens, 1)
    blob = oracle.fill_splitmix64(psize, 41)
    d_blob = _dev(torch, blob, gpu)
    for per_entry, key_stride, flags, lanes in ((True, 20, 0xFFFF, 0), (True, 24, 0, 0), (False, 0, 0xFFFF, 0),
                                                (False, 0, 0, 1), (True, 20, 1, 1)):
        ledgers, ids, lacs, lenf = vu.ids_for(n, 7 + key_stride, per_entry)
        keys = vu.keys_for(n, key_stride, 9)
        want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, key_stride, flags,
                                            600)
        roffs, rsize = place_requests(vu.head_len(algo) + np.where(plens < 600, plens, 0), 2)
        with _forced(lanes):
            req, digests = run_device(torch, gpu, algo, ledgers, ids, lacs, lenf, d_blob, poffs, plens, keys,
                                      key_stride, flags, 600, roffs, rsize)
        _same(digests.cpu().numpy().view(np.uint32), want_d, ("digests", key_stride, flags, lanes))
        _same(req.cpu().numpy(), want_buffer(rsize, roffs, want), ("buffer", key_stride, flags, lanes))
    # the default layouts of the Python form: packed, and on a 64-byte grid
    ledgers, ids, lacs, lenf = vu.ids_for(n, 3, False)
    dm = dg.DigestManager.instantiate(int(ledgers), b"", DTYPE[algo], True)
    want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, bytes(range(20)), 0, 0, 600)
    for align in (1, 64):
        req, roffs, digests = dm.package_batch_v2(*[_dev(torch, x, gpu) for x in (ids, lacs, lenf)], d_blob,
                                                  _dev(torch, poffs, gpu), _dev(torch, plens.astype(np.int32), gpu),
                                                  bytes(range(20)), small_threshold=600, align=align, sync_check=True)
        ro, got = roffs.cpu().numpy(), req.cpu().numpy()
        assert (ro % align == 0).all() and ro[0] == 0
        if align == 1:
            assert got.tobytes() == b"".join(want)
        for i in range(n):
            assert got[ro[i]:ro[i] + len(want[i])].tobytes() == want[i], (align, i)
        _same(digests.cpu().numpy().view(np.uint32), want_d, ("digests", align))


def test_bounds(gpu):
    """One payload past payload_size: digest 0, its head written, nothing copied. One request past
    requests_size: no byte of it written. Both raise the stream's flag, reported once by its next sync
    and not seen by another stream; every other entry is exact."""
    import torch
    algo, small = ck.CRC32C, 600
    plens = np.concatenate([np.arange(20, 60), [300, 300]]).astype(np.int64)
    n = plens.size
    ledgers, ids, lacs, lenf = vu.ids_for(n, 13, False)
    keys = vu.keys_for(n, 0, 13)
    poffs, psize = place_payloads(plens, 4)
    blob = oracle.fill_splitmix64(psize, 43)
    bad_p, bad_r = 7, n - 1
    want, want_d = vu.expected_requests(algo, ledgers, ids, lacs, lenf, blob, poffs, plens, keys, 0, 0, small)
    roffs, rsize = place_requests(vu.head_len(algo) + plens, 6)
    cut = int(roffs[bad_r] + len(want[bad_r]) - 1)  # requests_size: one byte short of the last request
    # the payload that starts inside and ends one byte past the buffer
    poffs2 = poffs.copy()
    poffs2[bad_p] = psize - plens[bad_p] + 1
    hl = vu.head_len(algo)
    want[bad_p] = want[bad_p][:hl - 4] + bytes(4)  # the head with digest 0, no payload
    want[bad_r] = b""
    want_d = want_d.copy()
    want_d[bad_p] = 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    full = torch.full((rsize,), vu.SENTINEL, dtype=torch.uint8, device=gpu)
    d_blob = _dev(torch, blob, gpu)
    args = [_dev(torch, x, gpu) for x in (ids, lacs, lenf)] + [d_blob, _dev(torch, poffs2, gpu),
                                                               _dev(torch, plens.astype(np.int32), gpu), bytes(keys)]
    d_roffs = _dev(torch, roffs, gpu)
    torch.cuda.synchronize()
    dm = dg.DigestManager.instantiate(int(ledgers), b"", DTYPE[algo], True)
    _, _, digests = dm.package_batch_v2(*args, small_threshold=small, requests=full[:cut], request_offsets=d_roffs,
                                        stream=s1)
    ck.stream_sync(s2)  # another stream: no flag
    with pytest.raises(_native.BkdError) as e:
        ck.stream_sync(s1)
    assert e.value.code == -4
    ck.stream_sync(s1)  # reported once
    _same(digests.cpu().numpy().view(np.uint32), want_d, "digests")
    _same(full.cpu().numpy(), want_buffer(rsize, roffs, want), "request buffer")
    ck.release_stream(s1)
    ck.release_stream(s2)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_host_form_gpu_route_equals_cpu_route(gpu, algo):
    """The host form through pinned staging, a batch of more than one 64 MiB staging segment with small
    and large entries on both sides of the cut: byte-equal to the CPU route, digests the oracle's."""
    small = dg.SMALL_ENTRY_SIZE_THRESHOLD
    rng = np.random.default_rng(3 + algo)
    mib = 1 << 20
    part = np.concatenate([rng.integers(0, 700, 1500), [small - 1, small, 2 * mib], np.full(16, 2 * mib + 5)])
    plens = np.concatenate([part, part]).astype(np.int64)  # 2 x ~35 MiB
    assert plens.sum() > 64 * mib
    n = plens.size
    poffs = np.cumsum(plens) - plens
    blob = oracle.fill_splitmix64(int(plens.sum()), 51 + algo)
    views = [blob[o:o + l] for o, l in zip(poffs.tolist(), plens.tolist())]
    ledgers, ids, lacs, lenf = vu.ids_for(n, 19, True)
    keys = vu.keys_for(n, 24, 19)
    want_d, _ = vu.digests_for(algo, ledgers, ids, lacs, lenf, blob, poffs, plens)
    out = {}
    for name, route in (("gpu", ck.HOST_ROUTE_GPU), ("cpu", ck.HOST_ROUTE_CPU)):
        bufs = vu.sentinel_buffers(algo, np.where(plens < small, plens, 64))
        with ck.host_batch_route(route):
            rc, digests = vu.package_v2_host_raw(algo, 0, ledgers, ids, lacs, lenf, views, keys, 24, 0x8001, small, bufs)
        assert rc == 0, _native.last_error()
        _same(digests, want_d, ("digests", name))
        out[name] = bufs
    for i in range(n):
        assert (out["gpu"][i] == out["cpu"][i]).all(), i
        assert (out["gpu"][i][-16:] == vu.SENTINEL).all(), i
