"""The edge logs of test_gpu_scrub_edges.py through the host form's CPU route (host_scrub.cpp): each fixture of
scrub_util agrees with its reference (hmac, oracle.verify_entry, the DUMMY length rule) without a device, and
the CPU route sees the same alignments, tail bytes, first-failure positions, long bins and index shapes."""
import time

import numpy as np
import pytest

import scrub_util as su
from bookkeeper_amd import checksum as ck


@pytest.fixture(autouse=True)
def cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def check(log, types=su.ALL, rc_want=0):
    buf, offs, lens, table, want = log
    rc, status, fb = su.run_host(buf, offs, lens, table, types=types)
    assert rc == rc_want
    assert (status == want).all(), np.nonzero(status != want)[0][:10]
    assert fb == su.want_first_bad(want)
    return status


# ---- B.2: alignment x length ----

@pytest.mark.parametrize("end_mod", [None, 1, 2, 3])
def test_alignment_length_sweep(end_mod):
    a, b = su.sweep_log(0x00, end_mod), su.sweep_log(0xFF, end_mod)
    want = a[4]
    assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[4] == b[4]).all()
    assert (a[0] != b[0]).sum() >= len(want)  # only the filler differs, at least a byte per entry
    n_each = {name: 4 * (hi - lo + 1) for name, (lo, hi) in su.SWEEP_RANGES.items()}
    assert n_each["HMAC"] == 528 and len(want) == sum(n_each.values()) + (end_mod is not None)
    for name in ("HMAC", "CRC32C", "CRC32"):  # a third intact, two thirds fail, for every type with a digest
        mine = np.array([su.type_name(su.SWEEP_SPECS[su.ledger_of(a[0], int(o))]) == name for o in a[1]])
        got = want[mine]
        assert set(got.tolist()) == {0, 2} and mine.sum() == n_each[name] + (name == "HMAC" and end_mod is not None)
        assert (got == 0).sum() >= n_each[name] // 3 and (got == 2).sum() >= 2 * (n_each[name] // 3), name
    if end_mod is not None:
        assert want[-1] == (2 if end_mod == 2 else 0)
    assert (check(a) == check(b)).all()


# ---- B.3: where the first failure is ----

@pytest.mark.parametrize("kind", su.FB_KINDS)
@pytest.mark.parametrize("p", su.FB_POSITIONS)
def test_first_bad_placement(p, kind):
    log = su.first_bad_log(p, kind)
    want = log[4]
    assert su.want_first_bad(want) == p and want[p] == su.FB_KIND_STATUS[kind]
    assert (want > 0).sum() == 1 + (p + 1 < su.FB_N) + (p // 256 < 3)
    check(log)


def test_first_bad_none():
    log = su.first_bad_log()
    assert not log[4].any() and len(log[4]) == su.FB_N == 775
    check(log)


# ---- B.4: long bins ----

def test_long_bins_and_one_cap_frame():
    """The e <= 14 frames and one frame of exactly the cap (16 MiB; bin 72): 41 frames, 28 MB. Measured: the
    CPU route's call 0.08 s, the whole test with the log and its reference statuses 0.31 s."""
    log = su.long_bins_log(cap=("good",))
    buf, offs, lens, table, want = log
    assert su.bin_of(su.MAC_MAX_ENTRY) == 72 and (lens == su.MAC_MAX_ENTRY).sum() == 1
    assert len({su.bin_of(int(n)) for n in lens}) >= 30
    assert (want == 0).sum() >= 20 and (want == 2).sum() >= 20
    t = time.perf_counter()
    check(log)
    print(f"CPU route, long bins: {time.perf_counter() - t:.3f} s")


# ---- B.5: the calls of the one-stream test ----

def test_changing_shapes():
    for log, types, _, rc_want in su.shape_steps():
        check(log, types, rc_want)
    sizes = [len(s[0][4]) for s in su.shape_steps()]
    assert sizes == [2000, 5, 700, 3, 2000]


# ---- B.7: index shapes ----

def test_index_shapes():
    down, thrice, nested = su.index_shapes()
    assert (np.diff(down[1].astype(np.int64)) < 0).all()
    assert len(thrice[4]) == len(down[4]) + 2 * ((len(down[4]) + 9) // 10)
    for log in (down, thrice, nested):
        check(log)
