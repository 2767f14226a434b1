"""GPU: batches that span many ledgers — bkd_digest_verify_requests, bkd_digest_package_batch_ledgers
and their host-resident forms through the GPU route.

requests_util.py's batch (18 requests, empty ones first, last and adjacent; 64-bit ledger ids; an
entry-id carry inside a request; two skip flags; every corruption kind placed by request) on every
route of the verify sequence, with the geometry forced as test_gpu_framed_sweep.py forces it:

* fused (plan mode 2, lengths within the gate's band: request_expand_kernel, then
  crc_verify_fused_kernel<G, .., RequestIds>) for G = 4 .. 64, both algorithms, both fold schedules;
* header / plan / finish (plan mode 2, payloads 0 .. 2600 bytes: out of band) and header / direct /
  finish (plan mode 1): verify_header_kernel<RequestIds>, verify_finish_kernel<RequestIds>;
* failures in different rounds of the fused kernel's grid stride than the prefix word they lower;
* one request (bit for bit bkd_digest_verify_batch), one entry per request, 3 n requests, no entries;
* a malformed CSR: BKD_ERR_BOUNDS from the stream's sync, nothing written outside the outputs, the
  stream usable afterwards; two streams at once, one of them with a malformed CSR;
* package with per-entry ledger ids on the fused and the header-first route,
  package_frame_kernel<LedgerPerEntry>'s LDS and per-thread paths, equality with
  bkd_digest_package_batch for one ledger id, a round trip;
* the host forms through the GPU with a request cut across staged segments;
* the two id sources of each kernel against each other: one ledger id per call against the same id per
  entry, one read against one request, on the same frames.

Every status, prefix, frame byte and digest equals the oracle's.
"""
import contextlib
import ctypes
import threading

import numpy as np
import pytest

import framed_util as fu
import oracle
import requests_util as rq
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg
from bookkeeper_amd._native import BkdError, check, lib

pytestmark = pytest.mark.gpu

DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}
ALGOS = [ck.CRC32C, ck.CRC32]
BOUNDS = -4


@contextlib.contextmanager
def _forced(lanes, schedule, plan_mode):
    """Lane width `lanes` for every one-entry-per-group kernel and for the plan (so the fused verify's
    lane count equals the plan's), the fold schedule and the indexed route; all restored."""
    try:
        ck.set_group_lanes(lanes)
        ck.set_plan_geometry(lanes, min(32, 32768 // (16 * lanes)), 16)
        ck.set_fold_schedule(schedule)
        ck.set_plan_mode(plan_mode)
        yield
    finally:
        ck.set_group_lanes(0)
        ck.set_plan_geometry()
        ck.set_fold_schedule(0)
        ck.set_plan_mode(0)


def _dev(torch, a, gpu):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    assert t.data_ptr() % 256 == 0  # the placement's residues are the addresses' residues
    return t


def _same(got, want, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))
    assert bad[0].size == 0, (what, bad[0].size, [b[:5].tolist() for b in bad])


class _Dev:
    """A requests_util.Batch on the device."""

    def __init__(self, torch, gpu, b):
        self.b = b
        self.blob = _dev(torch, b.blob, gpu)
        self.off, self.len = _dev(torch, b.foffs, gpu), _dev(torch, b.flens.astype(np.int32), gpu)
        self.first, self.ledgers = _dev(torch, b.first, gpu), _dev(torch, b.ledgers, gpu)
        self.firsts, self.flags = _dev(torch, b.firsts, gpu), _dev(torch, b.flags, gpu)

    def verify(self, stream=None):
        st, fb = dg.verify_requests(DTYPE[self.b.algo], self.blob, self.off, self.len, self.first, self.ledgers,
                                    self.firsts, self.flags, stream=stream)
        return st, fb

    def check(self, what, stream=None):
        st, fb = self.verify(stream)
        ck.stream_sync(stream)  # a well-formed CSR raises nothing
        _same(st.cpu().numpy(), self.b.want, (what, "status"))
        _same(fb.cpu().numpy(), self.b.want_prefix, (what, "prefix"))


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_verify_requests_fused_route(gpu, lanes, algo, schedule):
    import torch
    d = _Dev(torch, gpu, rq.fused_batch(algo, lanes))
    # plan mode 2 gives route == 1, the forced width is both fused_lanes and g_plan_lanes, and every
    # length lies in the band of the first (requests_util.fused_batch asserts it)
    with _forced(lanes, schedule, 2):
        d.check(("fused", lanes, algo, schedule))


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_verify_requests_plan_and_direct_routes(gpu, lanes, algo):
    import torch
    b = rq.ragged_batch(algo)
    d = _Dev(torch, gpu, b)
    with _forced(lanes, 1, 2):  # out of band: the gate sends it to the header / plan / finish sequence
        d.check(("plan", lanes, algo))
    with _forced(lanes, 1, 1):  # route == 0: header, the direct kernel at the forced width, finish
        d.check(("direct", lanes, algo))
    # the same statuses and prefixes the fused route gives for the same requests and corruptions
    f = rq.fused_batch(algo, lanes)
    live = np.arange(rq.N) != rq.N - 1  # (the short frame: a 20-byte frame here, a cut buffer there)
    assert (f.want == b.want)[live].all() and (f.want_prefix == b.want_prefix).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_requests_failures_across_grid_rounds(gpu, algo):
    """2 ngroups + 77 short frames at G = 8 in requests of 1000: failures at entries ngroups - 1 (the
    last group's first round), ngroups (the first group's second round) and the last entry, so a
    request's failing entry and the group that stores its prefix word meet in different rounds."""
    import torch
    ng = torch.cuda.get_device_properties(gpu).multi_processor_count * (1024 // 8)
    n, plen = 2 * ng + 77, 64
    hl = 32 + fu.MAC[algo]
    fl = hl + plen
    nreq = (n + 999) // 1000
    first = np.minimum(np.arange(nreq + 1, dtype=np.int64) * 1000, n)
    req = np.repeat(np.arange(nreq), np.diff(first))
    ledgers = (np.arange(nreq, dtype=np.int64) * 0x100000001) - 5
    firsts = 2**32 - 500 + 7 * np.arange(nreq, dtype=np.int64)
    ids = firsts[req] + (np.arange(n) - first[req])
    lacs, lenf = ids - 1, fu.LENGTH_FIELD_BASE + np.arange(n, dtype=np.int64) * plen
    blob = oracle.fill_splitmix64(n * fl, 5 + algo)
    hdr = fu.headers(ledgers[req], ids, lacs, lenf)
    foffs = np.arange(n, dtype=np.int64) * fl
    hcrc = oracle.batch(algo, hdr.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
    digests = oracle.batch(algo, blob, (foffs + hl).astype(np.uint64), np.full(n, plen, np.uint32), seeds=hcrc)
    blob.reshape(n, fl)[:, :hl] = np.concatenate([hdr, fu.digest_bytes(algo, digests)], axis=1)
    bad = [ng - 1, ng, n - 1]
    for i in bad:
        blob[i * fl + hl + 3] ^= 0x40
    frames = blob.reshape(n, fl)
    want = np.array([oracle.verify_entry(algo, frames[i], int(ledgers[req[i]]), int(ids[i])) for i in range(n)],
                    dtype=np.int32)
    assert np.nonzero(want)[0].tolist() == bad
    with _forced(8, 1, 2):
        st, fb = dg.verify_requests(DTYPE[algo], _dev(torch, blob, gpu), _dev(torch, foffs, gpu),
                                    _dev(torch, np.full(n, fl, np.int32), gpu), _dev(torch, first, gpu),
                                    _dev(torch, ledgers, gpu), _dev(torch, firsts, gpu))
        ck.stream_sync(None)
    _same(st.cpu().numpy(), want, "status")
    _same(fb.cpu().numpy(), rq.prefixes(want, first), "prefix")


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_requests_degenerate_groupings(gpu, algo):
    import torch
    dt = DTYPE[algo]
    for route, b in (("fused", rq.fused_batch(algo, 8)), ("plan", rq.ragged_batch(algo))):
        d = _Dev(torch, gpu, b)
        with _forced(8, 1, 2):
            # one request: request 7's frames (two corrupted) against bkd_digest_verify_batch, bit for bit
            i0, i1 = int(b.first[7]), int(b.first[8])
            dm = dg.DigestManager.instantiate(rq.LEDGERS[7], b"", dt, False)
            for skip in (False, True):
                st1, fb1 = dm.verify_batch(d.blob, d.off[i0:i1], d.len[i0:i1], rq.FIRSTS[7], skip_entry_check=skip)
                st, fb = dg.verify_requests(dt, d.blob, d.off[i0:i1], d.len[i0:i1],
                                            _dev(torch, np.array([0, i1 - i0]), gpu),
                                            _dev(torch, np.array([rq.LEDGERS[7]]), gpu),
                                            _dev(torch, np.array([rq.FIRSTS[7]]), gpu),
                                            _dev(torch, np.array([int(skip)], dtype=np.int32), gpu))
                assert torch.equal(st, st1) and int(fb[0].item()) == int(fb1.item()) == 100, (route, skip)
            # one entry per request, and 3 n requests of sizes 0, 1, 0
            flags_e = b.flags[b.req]
            for what, sizes, pick in (("nreq = n", np.ones(rq.N, dtype=np.int64), np.arange(rq.N)),
                                      ("nreq = 3n", np.tile([0, 1, 0], rq.N), np.repeat(np.arange(rq.N), 3))):
                first = rq.csr(sizes)
                st, fb = dg.verify_requests(dt, d.blob, d.off, d.len, _dev(torch, first, gpu),
                                            _dev(torch, b.lid[pick], gpu), _dev(torch, b.ids[pick], gpu),
                                            _dev(torch, flags_e[pick], gpu))
                ck.stream_sync(None)
                _same(st.cpu().numpy(), b.want, (route, what, "status"))
                _same(fb.cpu().numpy(), rq.prefixes(b.want, first), (route, what, "prefix"))
    # no entries: every request's prefix is zero
    e64 = torch.empty(0, dtype=torch.int64, device=gpu)
    st, fb = dg.verify_requests(dt, torch.empty(0, dtype=torch.uint8, device=gpu), e64,
                                torch.empty(0, dtype=torch.int32, device=gpu),
                                torch.zeros(6, dtype=torch.int64, device=gpu),
                                torch.arange(5, dtype=torch.int64, device=gpu), torch.arange(5, dtype=torch.int64, device=gpu))
    ck.stream_sync(None)
    assert st.numel() == 0 and fb.cpu().tolist() == [0] * 5


def _raw_verify(torch, gpu, d, first, stream, pad=64):
    """bkd_digest_verify_requests with the outputs between sentinels: (status, prefixes, intact)."""
    n, nreq = rq.N, len(first) - 1
    st = torch.full((pad + n + pad,), -7, dtype=torch.int32, device=gpu)
    fb = torch.full((pad + nreq + pad,), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
    d_first = _dev(torch, np.asarray(first, dtype=np.int64), gpu)
    torch.cuda.synchronize()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    check(lib().bkd_digest_verify_requests(d.b.algo, p(d.blob), d.blob.numel(), p(d.off), p(d.len), n, p(d_first), nreq,
                                           p(d.ledgers), p(d.firsts), p(d.flags), p(st, 4 * pad), p(fb, 8 * pad),
                                           ck._stream_ptr(stream)))

    def intact():
        s, f = st.cpu().numpy(), fb.cpu().numpy()
        return bool((s[:pad] == -7).all() and (s[pad + n:] == -7).all() and (f[:pad] == 0x5A5A5A5A).all() and
                    (f[pad + nreq:] == 0x5A5A5A5A).all())

    return st[pad:pad + n], fb[pad:pad + nreq], intact


def _malformed(b):
    dec, above, below = b.first.copy(), b.first.copy(), b.first.copy()
    dec[6], dec[7] = dec[7], dec[6]  # requests 5 .. 7: a decreasing pair in the middle
    above[-2:] = rq.N + 9            # the last requests end past n
    below[-3:] = rq.N - 9            # the CSR ends below n
    assert (np.diff(dec) < 0).any() and above[-1] > rq.N > below[-1]
    return {"decreasing": dec, "ends above n": above, "ends below n": below}


@pytest.mark.parametrize("algo", ALGOS)
def test_verify_requests_malformed_csr_on_the_device(gpu, algo):
    """The reporting path: the kernels clamp, nothing faults; the stream's next sync returns
    BKD_ERR_BOUNDS, no byte around the outputs is written, and the stream then serves a correct call."""
    import torch
    s = torch.cuda.Stream(device=gpu)
    for route, b in (("fused", rq.fused_batch(algo, 8)), ("plan", rq.ragged_batch(algo))):
        d = _Dev(torch, gpu, b)
        with _forced(8, 1, 2):
            for what, first in _malformed(b).items():
                _, _, intact = _raw_verify(torch, gpu, d, first, s)
                with pytest.raises(BkdError) as e:
                    ck.stream_sync(s)
                assert e.value.code == BOUNDS, (route, what)
                assert intact(), (route, what)
                st, fb, intact = _raw_verify(torch, gpu, d, b.first, s)
                ck.stream_sync(s)  # the flag was cleared; a well-formed call raises nothing
                _same(st.cpu().numpy(), b.want, (route, what, "status after"))
                _same(fb.cpu().numpy(), b.want_prefix, (route, what, "prefix after"))
                assert intact()
    ck.release_stream(s)


def test_verify_requests_two_streams(gpu):
    """Two threads on their own streams with different request layouts, one of them malformed: the
    bounds flag reaches that stream's sync alone and neither sees the other's prefixes."""
    import torch
    b = rq.ragged_batch(ck.CRC32C)
    d = _Dev(torch, gpu, b)
    bad_first = _malformed(b)["decreasing"]
    sizes1 = np.ones(rq.N, dtype=np.int64)
    one = (_dev(torch, rq.csr(sizes1), gpu), _dev(torch, b.lid, gpu), _dev(torch, b.ids, gpu),
           _dev(torch, b.flags[b.req], gpu))
    results, barrier = {}, threading.Barrier(2)

    def worker(name):
        s = torch.cuda.Stream(device=gpu)
        torch.cuda.synchronize()
        barrier.wait()
        try:
            for _ in range(10):
                if name == "requests":
                    st, fb = d.verify(stream=s)
                else:
                    _raw_verify(torch, gpu, d, bad_first, s)
                    st, fb = dg.verify_requests(dg.DigestType.CRC32C, d.blob, d.off, d.len, *one, stream=s)
            ck.stream_sync(s)
            results[name] = ("ok", st.cpu().numpy(), fb.cpu().numpy())
        except BkdError as e:
            with torch.cuda.stream(s):
                results[name] = ("err", e.code, st.cpu().numpy(), fb.cpu().numpy())
        finally:
            ck.release_stream(s)

    ts = [threading.Thread(target=worker, args=(k,)) for k in ("requests", "malformed then per entry")]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert results["requests"][0] == "ok"
    _same(results["requests"][1], b.want, "status")
    _same(results["requests"][2], b.want_prefix, "prefix")
    assert results["malformed then per entry"][:2] == ("err", BOUNDS)
    _same(results["malformed then per entry"][2], b.want, "status, one entry per request")
    _same(results["malformed then per entry"][3], (b.want == 0).astype(np.int64), "prefix, one entry per request")


def _package_want(b, poffs, plens, blob):
    """Every entry's [32 B header][digest] and digest for payloads at poffs of `blob`, from the oracle."""
    n = len(poffs)
    hdr = fu.headers(b.lid[:n], b.ids[:n], b.lacs[:n], b.lenf[:n])
    hcrc = oracle.batch(b.algo, hdr.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
    want = oracle.batch(b.algo, blob, np.asarray(poffs, dtype=np.uint64), np.asarray(plens, dtype=np.uint32), seeds=hcrc)
    return np.concatenate([hdr, fu.digest_bytes(b.algo, want)], axis=1), want


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_package_batch_ledgers_routes(gpu, lanes, algo, schedule):
    import torch
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    b = rq.ragged_batch(algo)
    n, hl, dt = rq.N, b.hl, DTYPE[algo]
    poffs = np.minimum(b.poffs, b.size)  # (the 20-byte frame has no payload)
    head, want_d = _package_want(b, poffs, b.plens, b.blob)
    d_lid, d_ids, d_lacs, d_lenf = (_dev(torch, a, gpu) for a in (b.lid, b.ids, b.lacs, b.lenf))
    d_plen, d_blob = _dev(torch, b.plens.astype(np.int32), gpu), _dev(torch, b.blob, gpu)
    with _forced(lanes, schedule, 0):
        # fused: the frames are a tensor of their own (frames_apart), the forced width >= 4
        for stride in (None, 64):
            frames, digests = dg.package_batch_ledgers(dt, d_lid, d_ids, d_lacs, d_lenf, d_blob, _dev(torch, poffs, gpu),
                                                       d_plen, frame_stride=stride, sync_check=True)
            _same(digests.cpu().numpy().view(np.uint32), want_d, ("fused digests", stride))
            _same(frames.cpu().numpy()[:, :hl], head, ("fused frames", stride))
        # header-first: each frame in front of its payload, inside the payload buffer
        stride = int(hl + b.plens.max())
        stride += (5 - stride) % 16
        f0 = 3
        at = f0 + hl + stride * np.arange(n, dtype=np.int64)
        buf = oracle.fill_splitmix64(int(at[-1] + b.plens[-1]) + 1, 9 + algo)
        run = np.arange(int(b.plens.sum()), dtype=np.int64) - np.repeat(np.cumsum(b.plens) - b.plens, b.plens)
        buf[np.repeat(at, b.plens) + run] = b.blob[np.repeat(poffs, b.plens) + run]
        d_buf = _dev(torch, buf, gpu)
        dig = torch.empty(n, dtype=torch.int32, device=gpu)
        check(lib().bkd_digest_package_batch_ledgers(algo, p(d_lid), p(d_ids), p(d_lacs), p(d_lenf), p(d_buf),
                                                     d_buf.numel(), p(_dev(torch, at, gpu)), p(d_plen), n, p(d_buf, f0),
                                                     stride, p(dig), None))
        ck.stream_sync(None)
    _same(dig.cpu().numpy().view(np.uint32), want_d, "in-place digests")
    want = buf.copy()
    want[(f0 + stride * np.arange(n)[:, None] + np.arange(hl)).reshape(-1)] = head.reshape(-1)
    _same(d_buf.cpu().numpy(), want, "in-place buffer: frames written, payloads untouched")


@pytest.mark.parametrize("algo", ALGOS)
def test_package_frame_ledgers_kernel_packed_and_misaligned(gpu, algo):
    """package_frame_kernel<LedgerPerEntry> at the packed stride: the LDS path with n = 1, 255, 256, 257 and the
    per-thread path with the frame buffer 1, 2 and 3 bytes off a dword, between sentinel bytes."""
    import torch
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    b = rq.ragged_batch(algo)
    hl, pad = b.hl, 256
    poffs = np.minimum(b.poffs, b.size)
    d_blob = _dev(torch, b.blob, gpu)
    for n, mis in [(1, 0), (255, 0), (256, 0), (257, 0), (257, 1), (256, 2), (255, 3), (1, 3)]:
        i0 = 60  # (from request 5 on: ledger ids -1, -2^63, 2^63 - 1 and the entry-id carry of request 7)
        sl = slice(i0, i0 + n)
        sub = type("S", (), dict(algo=algo, lid=b.lid[sl], ids=b.ids[sl], lacs=b.lacs[sl], lenf=b.lenf[sl]))
        head, want_d = _package_want(sub, poffs[sl], b.plens[sl], b.blob)
        out = torch.full((pad + mis + n * hl + pad,), 0xA5, dtype=torch.uint8, device=gpu)
        assert out.data_ptr() % 4 == 0
        dig = torch.empty(n, dtype=torch.int32, device=gpu)
        args = [_dev(torch, a, gpu) for a in (sub.lid, sub.ids, sub.lacs, sub.lenf, poffs[sl], b.plens[sl].astype(np.int32))]
        check(lib().bkd_digest_package_batch_ledgers(algo, p(args[0]), p(args[1]), p(args[2]), p(args[3]), p(d_blob),
                                                     d_blob.numel(), p(args[4]), p(args[5]), n, p(out, pad + mis), hl,
                                                     p(dig), None))
        ck.stream_sync(None)
        _same(dig.cpu().numpy().view(np.uint32), want_d, ("digests", n, mis))
        want = np.full(out.numel(), 0xA5, dtype=np.uint8)
        want[pad + mis:pad + mis + n * hl] = head.reshape(-1)
        _same(out.cpu().numpy(), want, ("frames and sentinels", n, mis))


@pytest.mark.parametrize("algo", ALGOS)
def test_package_batch_ledgers_one_ledger_and_round_trip(gpu, algo):
    import torch
    dt = DTYPE[algo]
    n, L = rq.N, 200
    payload = torch.empty(n * L, dtype=torch.uint8, device=gpu)
    ck.fill_splitmix64(payload, 77 + algo)
    first = rq.csr(rq.SIZES)
    req = np.repeat(np.arange(rq.NREQ), rq.SIZES)
    ledgers, firsts = np.array(rq.LEDGERS, dtype=np.int64), np.array(rq.FIRSTS, dtype=np.int64)
    ids = _dev(torch, firsts[req] + (np.arange(n) - first[req]), gpu)
    lacs, lenf = ids - 1, torch.full((n,), L, dtype=torch.int64, device=gpu)
    offs = torch.arange(n, dtype=torch.int64, device=gpu) * L
    lens = torch.full((n,), L, dtype=torch.int32, device=gpu)
    # one ledger id for every entry: bkd_digest_package_batch's output, bit for bit
    dm = dg.DigestManager.instantiate(2**32 + 5, b"", dt, False)
    for stride in (None, 64):
        f1, d1 = dm.package_batch(ids, lacs, lenf, payload, offs, lens, frame_stride=stride, sync_check=True)
        same = torch.full((n,), 2**32 + 5, dtype=torch.int64, device=gpu)
        f, d = dg.package_batch_ledgers(dt, same, ids, lacs, lenf, payload, offs, lens, frame_stride=stride, sync_check=True)
        hl = 32 + dm.macCodeLength
        assert torch.equal(f[:, :hl], f1[:, :hl]) and torch.equal(d, d1)
    # round trip: frames of 18 requests' ledgers, the payloads copied behind them, verified by request
    frames, _ = dg.package_batch_ledgers(dt, _dev(torch, ledgers[req], gpu), ids, lacs, lenf, payload, offs, lens)
    framed = torch.cat([frames, payload.view(n, L)], dim=1).contiguous()
    fl = framed.shape[1]
    for mode in (0, 2):
        with _forced(8, 1, mode):
            st, fb = dg.verify_requests(dt, framed.view(-1), torch.arange(n, dtype=torch.int64, device=gpu) * fl,
                                        torch.full((n,), fl, dtype=torch.int32, device=gpu), _dev(torch, first, gpu),
                                        _dev(torch, ledgers, gpu), _dev(torch, firsts, gpu))
            ck.stream_sync(None)
        assert not st.any().item() and fb.cpu().tolist() == rq.SIZES, mode


def test_host_forms_through_the_gpu_cut_a_request_across_segments(gpu):
    """20 frames of 8 MiB: three staged segments of <= 64 MiB (8, 8 and 4 frames); request 2 owns
    entries 3 .. 14 and so lies in both of the first two. Results equal the CPU route's and the oracle's."""
    algo, dt = ck.CRC32C, dg.DigestType.CRC32C
    n, fl, hl = 20, 8 << 20, 36
    sizes = [0, 3, 12, 5, 0]
    first = rq.csr(sizes)
    req = np.repeat(np.arange(len(sizes)), sizes)
    ledgers = np.array([3, -1, 2**32 + 5, 5, 9], dtype=np.int64)
    firsts = np.array([0, 2**32 - 2, 100, 7, 0], dtype=np.int64)
    lid, ids = ledgers[req], firsts[req] + (np.arange(n) - first[req])
    lacs, lenf = ids - 1, np.cumsum(np.full(n, fl - hl, dtype=np.int64))
    big = oracle.fill_splitmix64(n * fl, 21).reshape(n, fl)
    payloads = [big[i, hl:] for i in range(n)]
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        cpu_frames, cpu_dig = dg.package_batch_ledgers_host(dt, lid, ids, lacs, lenf, payloads)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        frames, dig = dg.package_batch_ledgers_host(dt, lid, ids, lacs, lenf, payloads)
    assert (frames == cpu_frames).all() and (dig == cpu_dig).all()
    for i in range(n):
        d, hdr = oracle.digest_entry(algo, int(lid[i]), int(ids[i]), int(lacs[i]), int(lenf[i]), payloads[i])
        assert bytes(frames[i]) == hdr + oracle.digest_bytes(algo, d), i
    big[:, :hl] = frames
    big[9, 5000] ^= 1   # request 2, position 6: in the second segment
    big[12, fl - 1] ^= 1
    big[16, 33] ^= 1    # request 3, position 1: in the third
    views = [big[i] for i in range(n)]
    want = np.array([oracle.verify_entry(algo, views[i], int(lid[i]), int(ids[i])) for i in range(n)], dtype=np.int32)
    assert np.nonzero(want)[0].tolist() == [9, 12, 16]
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        st_c, fb_c = dg.verify_requests_host(dt, views, first, ledgers, firsts)
    with ck.host_batch_route(ck.HOST_ROUTE_GPU):
        st, fb = dg.verify_requests_host(dt, views, first, ledgers, firsts)
    assert (st == want).all() and (st_c == want).all()
    assert fb.tolist() == fb_c.tolist() == [0, 3, 6, 1, 0]


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_id_sources_agree(gpu, lanes, algo):
    """Every package and verify kernel is one template on where the ids come from; here both
    instantiations get the same work. 257 frames of ledger L: package_batch and package_batch_ledgers
    with L for every entry write the same bytes; verify_batch and verify_requests with one request give
    the same statuses and the same verified prefix, on the intact frames and on frames with one
    corrupted digest (2), one frame of another ledger (3) and one of another entry id (4), the last two
    valid for the ids they carry. Frames of 48 .. 4096 bytes take header / direct / finish (plan mode 1)
    and header / plan / finish (mode 2: out of the gate's band); frames within 64 bytes of the first,
    mode 2, take the fused kernel. Equalities only."""
    import torch
    dt, n, hl = DTYPE[algo], 257, 32 + fu.MAC[algo]
    L, first_id = 2**32 + 5, 2**32 - 100  # the entry ids carry into the high word
    dm = dg.DigestManager.instantiate(L, b"", dt, False)
    i64 = lambda a: _dev(torch, np.asarray(a, dtype=np.int64), gpu)
    ids = first_id + np.arange(n, dtype=np.int64)
    bad_digest, bad_ledger, bad_entry = 200, 131, 77
    lids2, ids2 = np.full(n, L, dtype=np.int64), ids.copy()
    lids2[bad_ledger] ^= 1 << 32
    ids2[bad_entry] ^= 1 << 32
    ragged = 48 + (np.arange(n, dtype=np.int64) * 1009) % (4096 - 48 + 1)
    ragged[0], ragged[1] = 48, 4096
    banded = 4096 - (np.arange(n, dtype=np.int64) * 7) % 65
    for flens, modes in ((ragged, (1, 2)), (banded, (2,))):
        assert rq.in_band(flens) == (flens is banded) and flens.min() >= 48 and flens.max() == 4096
        plens = flens - hl
        foffs, size = fu._place(flens, 7)
        blob = oracle.fill_splitmix64(size, 3 + algo)
        lenf = fu.LENGTH_FIELD_BASE + np.cumsum(plens)
        d_blob, d_poff, d_plen = _dev(torch, blob, gpu), i64(foffs + hl), _dev(torch, plens.astype(np.int32), gpu)
        d_off, d_len = i64(foffs), _dev(torch, flens.astype(np.int32), gpu)
        rows = (foffs[:, None] + np.arange(hl)).reshape(-1)
        one = (i64([0, n]), i64([L]), i64([first_id]))
        for mode in modes:
            with _forced(lanes, 1, mode):
                for stride in (None, 64):
                    f1, d1 = dm.package_batch(i64(ids), i64(ids - 1), i64(lenf), d_blob, d_poff, d_plen,
                                              frame_stride=stride, sync_check=True)
                    f2, d2 = dg.package_batch_ledgers(dt, i64(np.full(n, L)), i64(ids), i64(ids - 1), i64(lenf), d_blob,
                                                      d_poff, d_plen, frame_stride=stride, sync_check=True)
                    assert torch.equal(f1[:, :hl], f2[:, :hl]) and torch.equal(d1, d2), (mode, stride)
                # frames valid for another ledger id and another entry id, from the per-entry form
                f3, _ = dg.package_batch_ledgers(dt, i64(lids2), i64(ids2), i64(ids - 1), i64(lenf), d_blob, d_poff,
                                                 d_plen, sync_check=True)
                intact, broken = blob.copy(), blob.copy()
                intact[rows] = f2.cpu().numpy()[:, :hl].reshape(-1)
                broken[rows] = f3.cpu().numpy()[:, :hl].reshape(-1)
                broken[foffs[bad_digest] + hl - 1] ^= 0x01
                for what, framed, want in (("intact", intact, {}),
                                           ("broken", broken, {bad_digest: 2, bad_ledger: 3, bad_entry: 4})):
                    d_framed = _dev(torch, framed, gpu)
                    st1, fb1 = dm.verify_batch(d_framed, d_off, d_len, first_id)
                    st2, fb2 = dg.verify_requests(dt, d_framed, d_off, d_len, *one)
                    ck.stream_sync(None)
                    assert torch.equal(st1, st2), (what, mode)
                    got = st1.cpu().numpy()
                    assert {int(i): int(got[i]) for i in np.nonzero(got)[0]} == want, (what, mode)
                    assert int(fb1.item()) == int(fb2[0].item()) == min(want, default=n), (what, mode)
