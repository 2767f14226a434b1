"""CPU: the framed length sweep (framed_util.py) through the CPU route of the host-resident batches.

The same frames, payloads, wide header fields and corruptions that test_gpu_framed_sweep.py puts
through the fused package / verify kernels, here through bkd_digest_verify_batch_host and
bkd_digest_package_batch_host on the CPU route (host_batch.cpp): a second implementation agrees with
the oracle on every fixture before a GPU sees them, and the host route gets the same sweep of every
length class at every start alignment. Needs no GPU.
"""
import numpy as np
import pytest

import framed_util as fu
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

ALGOS = [(ck.CRC32C, dg.DigestType.CRC32C), (ck.CRC32, dg.DigestType.CRC32)]


@pytest.fixture(autouse=True, params=[1, 0], ids=["1-thread", "all-threads"])
def cpu_route(request):
    ck.set_host_threads(request.param)
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        assert ck.get_host_batch_route() == ck.HOST_ROUTE_CPU
        yield
    ck.set_host_threads(0)


def test_lengths_and_bands():
    """The generator's own shape: 524 lengths at 4 lanes, 3 404 at 64; the band partition covers
    every frame once, in order."""
    assert fu.lengths_for(4).size == 524 and fu.lengths_for(64).size == 3404
    for G in fu.LANES:
        S = 16 * G
        ls = fu.lengths_for(G)
        assert ls[0] == 0 and ls[-1] == 11 * S + 19 and set(range(3 * S + 20)) <= set(ls.tolist())
        for hl in (36, 40):
            fl = np.concatenate([[0, 1, 31, 32, hl - 1], ls + hl])
            bd = fu.bands(fl)
            assert bd[0][0] == 0 and bd[-1][1] == fl.size
            assert all(a[1] == b[0] for a, b in zip(bd, bd[1:]))


@pytest.mark.parametrize("algo,dtype", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_verify_host_cpu_framed_sweep(lanes, algo, dtype):
    for shift in fu.SHIFTS:
        c, bd, picks, bad, clean, want, want_skip = fu.verify_case(lanes, algo, shift)
        dm = dg.DigestManager.instantiate(c.ledger, b"", dtype)
        st, fb = dm.verify_batch_host(c.frame_views(c.blob), c.first)
        assert (st == clean).all() and (st[5:] == 0).all() and (st[:5] == 1).all()
        # without the too-short frames: all 0 and the whole batch the verified prefix
        st, fb = dm.verify_batch_host(c.frame_views(c.blob)[5:], c.first + 5)
        assert (st == 0).all() and fb == c.n - 5
        st, fb = dm.verify_batch_host(c.frame_views(bad)[5:], c.first + 5)
        assert (st == want[5:]).all(), np.nonzero(st != want[5:])[0][:5]
        assert fb == min(i for _, i in picks) - 5
        for i0, i1 in bd[1:3] + bd[-1:]:  # per band, as the GPU's fused route is called
            st, fb = dm.verify_batch_host(c.frame_views(bad)[i0:i1], c.first + i0)
            assert (st == want[i0:i1]).all() and fb == int(np.nonzero(want[i0:i1])[0][0])
        st, _ = dm.verify_batch_host(c.frame_views(bad), c.first, skip_entry_check=True)
        assert (st == want_skip).all() and (want_skip == np.where(want == 4, 0, want)).all()
        assert {1, 2, 3, 4} <= set(want.tolist())


@pytest.mark.parametrize("algo,dtype", ALGOS)
@pytest.mark.parametrize("lanes", fu.LANES)
def test_package_host_cpu_framed_sweep(lanes, algo, dtype):
    for shift in fu.SHIFTS:
        c = fu.package_case(lanes, algo, shift)
        dm = dg.DigestManager.instantiate(c.ledger, b"", dtype)
        frames, digests = dm.package_batch_host(c.ids, c.lacs, c.lenf, c.payload_views())
        assert (digests == c.digests).all(), np.nonzero(digests != c.digests)[0][:5]
        assert frames.shape == c.head.shape and (frames == c.head).all()
        # the in-place layout holds the same payloads: the same digests again
        blob, f0, stride, poffs = fu.in_place_case(lanes, algo, shift)
        views = [blob[o:o + l] for o, l in zip(poffs.tolist(), c.plens.tolist())]
        _, digests = dm.package_batch_host(c.ids, c.lacs, c.lenf, views)
        assert (digests == c.digests).all()
