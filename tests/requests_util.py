"""Shared by test_requests_cpu.py and test_gpu_requests.py: one batch of framed entries that spans
many ledgers, grouped into read requests (bkd_digest_verify_requests), and the per-entry package
inputs that go with it (bkd_digest_package_batch_ledgers).

700 frames in 18 requests of sizes SIZES (empty requests first, last and adjacent), ledger ids that
use their 64 bits (a pair that differs in the high word only, -1, -2^63, 2^63 - 1, ledger ids shared
by two requests), first entry ids that carry into the high word inside a request, two requests with
the skip flag, and corruptions placed by request (PICKS and the extras in Batch). Headers and digests
come from oracle.batch / oracle.digest_entry, expected statuses from oracle.verify_entry called per
entry with its request's ledger id and expected entry id; nothing comes from the library under test.
"""
import functools
import types

import numpy as np

import framed_util as fu
import oracle

SIZES = [0, 1, 0, 0, 3, 64, 1, 257, 0, 40, 100, 31, 7, 1, 64, 50, 81, 0]
NREQ = len(SIZES)
N = sum(SIZES)
LEDGERS = [9, 5, 77, 78, 2**32 + 5, -1, -2**63, 2**63 - 1, 1, 61, 61, 1000, 2**40 + 3, 5, 123456789, -2, 7, 8]
FIRSTS = [0, 10, 20, 30, 2**32 - 2, 0, 2**63 - 1, 2**32 - 200, 40, 9000, 10**12, 11000, 12000, 13000, 14000, 2**62,
          16000, 17000]
SKIP = (11, 14)
# (request, position in the request, framed_util kind): every kind in another request; request 9's is
# its last entry; request 7 holds a second corruption behind the first (Batch)
PICKS = [(4, 1, "payload_first"), (5, 10, "payload_last"), (7, 100, "digest"), (9, 39, "lac"), (10, 50, "high"),
         (11, 3, "ledger"), (12, 2, "entry"), (14, 60, "digest_ledger"), (15, 20, "ledger_entry")]
assert N == 700 and len(LEDGERS) == len(FIRSTS) == NREQ
assert sorted(k for _, _, k in PICKS) == sorted(fu.KINDS) and len({r for r, _, _ in PICKS}) == len(PICKS)
assert all(p < SIZES[r] for r, p, _ in PICKS) and SIZES[9] - 1 == 39


def csr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def prefixes(status, first):
    """Per request: the position of its first non-zero status, or its entry count."""
    out = np.diff(first).astype(np.int64)
    for r in range(out.size):
        nz = np.nonzero(status[first[r]:first[r + 1]])[0]
        if nz.size:
            out[r] = nz[0]
    return out


class Batch:
    """blob: the frames (corrupted), frame i of flens[i] bytes at foffs[i], starting at byte
    (5 i + 7) mod 16. plens: payload lengths wanted (a pick's payload is at least one byte).
    short: how the frame that is shorter than a header + digest comes about (the last entry):
    "frame" = its length is 20; "cut" = its length is a whole frame's but the buffer ends 20 bytes
    into it (what a batch whose lengths must all pass the verify gate can hold).
    want / want_prefix: the oracle's statuses and per-request verified prefixes.
    clean_head: the [32 B header][digest] of every entry before the corruptions (package's output)."""

    def __init__(self, algo, plens, short="frame"):
        self.algo, self.mac = algo, fu.MAC[algo]
        self.hl = hl = 32 + self.mac
        self.first = csr(SIZES)
        self.req = np.repeat(np.arange(NREQ), SIZES)
        self.flags = np.array([1 if r in SKIP else 0 for r in range(NREQ)], dtype=np.int32)
        self.ledgers = np.array(LEDGERS, dtype=np.int64)
        self.firsts = np.array(FIRSTS, dtype=np.int64)
        pos = np.arange(N) - self.first[self.req]
        self.lid = self.ledgers[self.req]
        self.ids = self.firsts[self.req] + pos
        assert (self.ids[self.req == 4] == [2**32 - 2, 2**32 - 1, 2**32]).all()
        at = lambda r, p: int(self.first[r]) + p
        plens = np.asarray(plens, dtype=np.int64).copy()
        assert plens.size == N
        extras = [at(7, 200), at(16, 5), at(10, 70), at(11, 20)]
        touched = [at(r, p) for r, p, _ in PICKS] + extras
        plens[touched] = np.maximum(plens[touched], 1)
        self.plens = plens
        self.flens = plens + hl
        if short == "frame":
            self.flens[-1], self.plens[-1] = 20, 0
        rng = np.random.default_rng(77 + algo)
        self.lacs = rng.integers(-1, 2**63, N, dtype=np.int64)
        self.lenf = fu.LENGTH_FIELD_BASE + np.cumsum(self.plens)
        self.foffs, size = fu._place(self.flens, 7)
        if short == "cut":
            size = int(self.foffs[-1]) + 20
        self.poffs = self.foffs + hl
        blob = oracle.fill_splitmix64(int(self.foffs[-1] + self.flens[-1]), 31 + algo)
        hdr = fu.headers(self.lid, self.ids, self.lacs, self.lenf)
        hcrc = oracle.batch(algo, hdr.reshape(-1), np.arange(N, dtype=np.uint64) * 32, np.full(N, 32, np.uint32))
        ok = self.flens >= hl
        self.digests = np.zeros(N, dtype=np.uint32)
        self.digests[ok] = oracle.batch(algo, blob, self.poffs[ok].astype(np.uint64), self.plens[ok].astype(np.uint32),
                                        seeds=hcrc[ok])
        self.clean_head = np.concatenate([hdr, fu.digest_bytes(algo, self.digests)], axis=1)
        blob[(self.foffs[ok, None] + np.arange(hl)).reshape(-1)] = self.clean_head[ok].reshape(-1)
        # framed_util's corruptions, each against its own request's ledger id
        for r, p, kind in PICKS + [(7, 200, "payload_first")]:
            blob = self._corrupt(blob, kind, at(r, p))
        # a frame of request 15's ledger, whole and valid, delivered in request 16 (status 3)
        self._reframe(blob, at(16, 5), LEDGERS[15], FIRSTS[15] + 5)
        # an entry id off by one: status 4 in request 10 (behind its first failure), 0 under request 11's skip flag
        self._reframe(blob, at(10, 70), LEDGERS[10], int(self.ids[at(10, 70)]) + 1)
        self._reframe(blob, at(11, 20), LEDGERS[11], int(self.ids[at(11, 20)]) + 1)
        self.blob = blob[:size]
        self.size = size
        self.want = np.array([oracle.verify_entry(algo, self.frame(i), int(self.lid[i]), int(self.ids[i]),
                                                  bool(self.flags[self.req[i]])) for i in range(N)], dtype=np.int32)
        self.want_prefix = prefixes(self.want, self.first)
        counts = np.diff(self.first)
        assert set(self.want.tolist()) == {0, 1, 2, 3, 4}
        assert ((self.want_prefix == counts) & (counts > 0)).any()  # a request that verified whole
        assert self.want[at(16, 5)] == 3 and self.want[at(10, 70)] == 4 and self.want[at(11, 20)] == 0
        assert self.want[-1] == 1 and self.want_prefix[7] == 100 and self.want_prefix[9] == 39

    def frame(self, i):
        """The bytes of frame i that exist in the buffer."""
        return self.blob[self.foffs[i]:min(self.size, self.foffs[i] + self.flens[i])]

    def frame_views(self):
        return [self.frame(i) for i in range(N)]

    def _corrupt(self, blob, kind, i):
        shim = types.SimpleNamespace(blob=blob, hl=self.hl, algo=self.algo, ledger=int(self.lid[i]), ids=self.ids,
                                     lacs=self.lacs, lenf=self.lenf,
                                     frame=lambda b, j: b[self.foffs[j]:self.foffs[j] + self.flens[j]])
        return fu.corrupt(shim, [(kind, i)])

    def _reframe(self, blob, i, ledger, entry_id):
        f = blob[self.foffs[i]:self.foffs[i] + self.flens[i]]
        d, hdr = oracle.digest_entry(self.algo, ledger, entry_id, int(self.lacs[i]), int(self.lenf[i]), f[self.hl:])
        f[:self.hl] = np.frombuffer(hdr + oracle.digest_bytes(self.algo, d), dtype=np.uint8)


def fused_plens(G):
    """Payload lengths l0 + (7 i mod 97) - 48 around l0 = 3 * 16 G + 5, the sequence started where its
    first term is l0 itself (i + 90: 7 * 90 = 48 mod 97): the verify gate compares every frame with the
    call's FIRST frame (PlanRun::in_band: within ref / 16 + 64 bytes), and from l0 - 48 the far end,
    96 bytes away, is out of band at G = 4 and 8. The same 97 lengths, every one within 48 of the first."""
    l0 = 3 * 16 * G + 5
    plens = l0 + (7 * (np.arange(N) + 90)) % 97 - 48
    assert plens[0] == l0 and plens.min() == l0 - 48 and plens.max() == l0 + 48 and plens.min() >= 1
    return plens


def in_band(flens):
    """PlanRun::in_band (crc_kernels.hpp) of every frame length against the first."""
    fl = np.asarray(flens, dtype=np.int64)
    return bool((np.abs(fl - fl[0]) <= fl[0] // 16 + 64).all())


@functools.lru_cache(maxsize=4)
def fused_batch(algo, G):
    b = Batch(algo, fused_plens(G), short="cut")
    assert in_band(b.flens)  # the gate passes: crc_verify_fused_kernel<.., RequestIds> verifies it
    return b


@functools.lru_cache(maxsize=2)
def ragged_batch(algo):
    """Payload lengths spread over 0 .. 2600: out of band, the header / plan / finish route."""
    plens = (np.arange(N) * 37 + 11) % 2601
    plens[0], plens[at_free()] = 2600, 0
    b = Batch(algo, plens, short="frame")
    assert not in_band(b.flens) and b.plens.min() == 0 and b.plens.max() == 2600
    return b


def at_free():
    """An entry no corruption touches (request 5, position 0)."""
    return int(csr(SIZES)[5])
