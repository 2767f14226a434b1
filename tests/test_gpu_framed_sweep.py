"""GPU: every payload length class through the framed package / verify kernels at every lane width.

framed_util.py's batches (every length 0 .. 3 S + 19 and m S +- 19 for m = 4 .. 11 at S = 16 G bytes
per step, all 16 start residues in every step count, 64-bit ledger ids, an entry-id carry, wide LACs,
a length field that is not the payload's length) with the lane width forced to G = 4 .. 64, CRC32C and
CRC32, both fold schedules (1: never fold4_main, 2: always), on every route of bkd_digest_package_batch
and bkd_digest_verify_batch:

* package: the fused route (frames in a buffer of their own: crc_package_fused_kernel<G> with the
  header CRC as a late seed, then package_frame_kernel) and the header-first route (each frame in
  front of its payload);
* verify: the fused route (plan mode 2, one call per band of frame lengths the gate accepts:
  crc_verify_fused_kernel<G>), the header / plan / finish sequence (plan mode 2, the whole list: out
  of band), and the direct kernel (plan mode 1); clean, with framed_util's corruptions (two faults
  in one frame among them), and with skip_entry_check.

Every digest, frame byte, status and verified prefix equals the oracle's. Nothing observes the route
from outside: the conditions in bkdigest.hip (package_framed, verify_framed) that the settings meet
are named at each call.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import framed_util as fu
import oracle
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

pytestmark = pytest.mark.gpu

DTYPE = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}


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


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
@pytest.mark.parametrize("lanes", fu.LANES)
def test_package_framed_sweep(gpu, lanes, algo, schedule):
    import torch
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    for shift in fu.SHIFTS:
        c = fu.package_case(lanes, algo, shift)
        dm = dg.DigestManager.instantiate(c.ledger, b"", DTYPE[algo], False)
        n, hl = c.n, c.hl
        d_ids, d_lacs, d_lenf = _dev(torch, c.ids, gpu), _dev(torch, c.lacs, gpu), _dev(torch, c.lenf, gpu)
        d_plen = _dev(torch, c.plens.astype(np.int32), gpu)
        with _forced(lanes, schedule, 0):
            # fused: package_batch's frames are a tensor of their own (frames_apart) and auto_lanes
            # returns the forced width (lanes >= 4): crc_package_fused_kernel<lanes>
            frames, digests = dm.package_batch(d_ids, d_lacs, d_lenf, _dev(torch, c.blob, gpu), _dev(torch, c.poffs, gpu),
                                               d_plen, sync_check=True)
            _same(digests.cpu().numpy().view(np.uint32), c.digests, ("fused digests", shift))
            _same(frames.cpu().numpy(), c.head, ("fused frames", shift))
            # header-first: the frames lie inside the payload buffer (not frames_apart)
            blob, f0, stride, poffs = fu.in_place_case(lanes, algo, shift)
            buf = _dev(torch, blob, gpu)
            dig = torch.empty(n, dtype=torch.int32, device=gpu)
            ck._native.check(ck.lib().bkd_digest_package_batch(algo, c.ledger, p(d_ids), p(d_lacs), p(d_lenf), p(buf),
                                                               buf.numel(), p(_dev(torch, poffs, gpu)), p(d_plen), n,
                                                               p(buf, f0), stride, p(dig), None))
            ck.stream_sync(None)
        _same(dig.cpu().numpy().view(np.uint32), c.digests, ("in-place digests", shift))
        got = buf.cpu().numpy()
        want = blob.copy()
        want[(f0 + stride * np.arange(n)[:, None] + np.arange(hl)).reshape(-1)] = c.head.reshape(-1)
        _same(got, want, ("in-place buffer: frames, payloads untouched", shift))  # every byte of the buffer


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
@pytest.mark.parametrize("lanes", fu.LANES)
def test_verify_framed_sweep(gpu, lanes, algo, schedule):
    import torch
    for shift in fu.SHIFTS:
        c, bd, picks, bad, clean, want, want_skip = fu.verify_case(lanes, algo, shift)
        assert (want_skip == np.where(want == 4, 0, want)).all() and (want == 4).any()
        dm = dg.DigestManager.instantiate(c.ledger, b"", DTYPE[algo], False)
        d_off, d_len = _dev(torch, c.foffs, gpu), _dev(torch, c.flens.astype(np.int32), gpu)
        d_clean, d_bad = _dev(torch, c.blob, gpu), _dev(torch, bad, gpu)

        def run(blob, i0, i1, w, what, skip=False):
            st, fb = dm.verify_batch(blob, d_off[i0:i1], d_len[i0:i1], first_entry_id=c.first + i0,
                                     skip_entry_check=skip)
            _same(st.cpu().numpy(), w[i0:i1], (what, shift, i0, i1))
            nz = np.nonzero(w[i0:i1])[0]
            assert int(fb.item()) == (int(nz[0]) if nz.size else i1 - i0), (what, shift, i0, i1)

        # fused: plan mode 2 gives route == 1, the forced width is both fused_lanes and g_plan_lanes,
        # and every length of a call lies in the band of its first (framed_util.bands asserts it)
        with _forced(lanes, schedule, 2):
            for i0, i1 in bd:
                run(d_clean, i0, i1, clean, "fused clean")
                run(d_bad, i0, i1, want, "fused corrupted")
            with4 = [b for b in bd if (want[b[0]:b[1]] == 4).any()]
            run(d_bad, *with4[len(with4) // 2], want_skip, "fused skip", True)
            # the whole list is out of band: the gate sends it to the header / plan / finish sequence
            assert len(bd) > 1
            run(d_clean, 0, c.n, clean, "plan clean")
            run(d_bad, 0, c.n, want, "plan corrupted")
            run(d_bad, 0, c.n, want_skip, "plan skip", True)
        with _forced(lanes, schedule, 1):  # route == 0: header, the direct kernel at the forced width, finish
            run(d_clean, 0, c.n, clean, "direct clean")
            run(d_bad, 0, c.n, want, "direct corrupted")
            run(d_bad, 0, c.n, want_skip, "direct skip", True)


@pytest.mark.parametrize("algo", [ck.CRC32C, ck.CRC32])
def test_package_frame_kernel_packed_and_misaligned(gpu, algo):
    """package_frame_kernel at the packed stride (32 + mac): the LDS path with n = 1, 255, 256, 257 (one
    partial block, one full, one full + one frame), and the per-thread path at the same stride with
    the frame buffer's base 1, 2 and 3 bytes off a dword; frames equal the oracle's and the sentinel
    bytes on both sides of them are untouched."""
    import torch
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    mac = fu.MAC[algo]
    hl = 32 + mac
    ledger = fu.LEDGER[8]
    rng = np.random.default_rng(5 + algo)
    pad = 256
    for n, mis in [(1, 0), (255, 0), (256, 0), (257, 0), (257, 1), (256, 2), (255, 3), (1, 3)]:
        plens = rng.integers(0, 200, n).astype(np.int64)
        poffs = np.cumsum(plens) - plens
        payload = oracle.fill_splitmix64(int(plens.sum()) + 16, 3 + n + mis)
        ids = fu.FIRST_ENTRY_ID + 100 + np.arange(n, dtype=np.int64)
        lacs = rng.integers(-1, 2**63, n, dtype=np.int64)
        lenf = fu.LENGTH_FIELD_BASE + np.cumsum(plens)
        hdr = fu.headers(ledger, ids, lacs, lenf)
        hcrc = oracle.batch(algo, hdr.reshape(-1), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint32))
        want_d = oracle.batch(algo, payload, poffs.astype(np.uint64), plens.astype(np.uint32), seeds=hcrc)
        head = np.concatenate([hdr, fu.digest_bytes(algo, want_d)], axis=1)
        out = torch.full((pad + mis + n * hl + pad,), 0xA5, dtype=torch.uint8, device=gpu)
        assert out.data_ptr() % 4 == 0
        dig = torch.empty(n, dtype=torch.int32, device=gpu)
        d_pay = _dev(torch, payload, gpu)
        args = [_dev(torch, a, gpu) for a in (ids, lacs, lenf, poffs, plens.astype(np.int32))]
        # frames apart from the payload, automatic lanes >= 4: the fused route, whose second kernel this is
        ck._native.check(ck.lib().bkd_digest_package_batch(algo, ledger, p(args[0]), p(args[1]), p(args[2]), p(d_pay),
                                                           d_pay.numel(), p(args[3]), p(args[4]), n,
                                                           p(out, pad + mis), hl, p(dig), None))
        ck.stream_sync(None)
        _same(dig.cpu().numpy().view(np.uint32), want_d, ("digests", n, mis))
        want = np.full(out.numel(), 0xA5, dtype=np.uint8)
        want[pad + mis:pad + mis + n * hl] = head.reshape(-1)
        _same(out.cpu().numpy(), want, ("frames and sentinels", n, mis))
