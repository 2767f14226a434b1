"""A/B of verifying and packaging a batch that spans many ledgers, in ONE process on the same device
buffers: 1M framed 4 KiB entries (CRC32C), events on the stream, interleaved rounds in both orders
(cdna_hip_programming.md §5.4 rule 24: cross-process and first-run noise is larger than the effects
measured).

  a   verify_batch, one ledger (the single-ledger route: the yardstick)
  b   verify_requests, 1 request
  c   verify_requests, 1 024 requests of 1 024 entries, each its own ledger
  d   verify_requests, 1M requests of one entry
  e   what a caller does without verify_requests for c: 1 024 verify_batch calls on one stream
  fa  package_batch, one ledger          fb  package_batch_ledgers, 1 024 distinct ledger ids

Before timing, every route must verify every frame (the frames are packaged per ledger for c / d / e
and for one ledger for a / b) and fa's and fb's frames must equal the frames packaged in place.

Usage (GPU box): python3 tools/requests_ab.py     Environment: AB_ROUNDS (default 6), AB_N (entries,
a multiple of 1 024).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = int(os.environ.get("AB_ROUNDS", "6"))
REPS = 10
FRAME, HL = 4096, 36
NLEDGERS = 1024


def main():
    import torch
    from bookkeeper_amd import _native

    L = _native.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    n = int(os.environ.get("AB_N", str(1 << 20)))
    assert n % NLEDGERS == 0
    per = n // NLEDGERS
    i64 = dict(dtype=torch.int64, device=dev)
    # two copies of the frames: F1 framed for one ledger (a, b), FM for 1 024 ledgers (c, d, e)
    F1 = torch.empty(n * FRAME, dtype=torch.uint8, device=dev)
    assert L.bkd_fill_splitmix64(ptr(F1), F1.numel(), 7, 0, None) == 0
    FM = F1.clone()
    idx = torch.arange(n, **i64)
    lenf = torch.full((n,), FRAME - HL, **i64)
    poff, plen = idx * FRAME + HL, torch.full((n,), FRAME - HL, dtype=torch.int32, device=dev)
    foff, flen = idx * FRAME, torch.full((n,), FRAME, dtype=torch.int32, device=dev)
    ledger_of = 1000 + (idx // per) * 0x100000001  # distinct in both words
    ids_m = idx % per                                # entry ids restart in every ledger
    dig = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    fb = torch.empty(1, **i64)
    sep = torch.empty(n * HL, dtype=torch.uint8, device=dev)
    sep2 = torch.empty(n * HL, dtype=torch.uint8, device=dev)

    def requests(nreq):
        size = n // nreq
        r = torch.arange(nreq, **i64)
        return dict(first=torch.arange(nreq + 1, **i64) * size, ledgers=1000 + (r * size // per) * 0x100000001,
                    firsts=(r * size) % per, flags=torch.zeros(nreq, dtype=torch.int32, device=dev),
                    prefix=torch.empty(nreq, **i64), nreq=nreq, size=size)

    rq1 = dict(first=torch.tensor([0, n], **i64), ledgers=torch.tensor([7], **i64), firsts=torch.tensor([0], **i64),
               flags=torch.zeros(1, dtype=torch.int32, device=dev), prefix=torch.empty(1, **i64), nreq=1, size=n)
    rq1k, rq1m = requests(NLEDGERS), requests(n)

    def package(frames, stride, lacs=idx - 1):
        return L.bkd_digest_package_batch(0, 7, ptr(idx), ptr(lacs), ptr(lenf), ptr(F1), F1.numel(), ptr(poff), ptr(plen),
                                          n, ptr(frames), stride, ptr(dig), sp)

    def package_ledgers(buf, frames, stride):
        return L.bkd_digest_package_batch_ledgers(0, ptr(ledger_of), ptr(ids_m), ptr(ids_m), ptr(lenf), ptr(buf),
                                                  buf.numel(), ptr(poff), ptr(plen), n, ptr(frames), stride, ptr(dig), sp)

    def verify(buf=F1, ledger=7, first=0, lo=0, cnt=n):
        return L.bkd_digest_verify_batch(0, ledger, first, 0, ptr(buf), buf.numel(), ptr(foff, 8 * lo), ptr(flen, 4 * lo),
                                         cnt, ptr(status, 4 * lo), ptr(fb), sp)

    def verify_requests(buf, r):
        return L.bkd_digest_verify_requests(0, ptr(buf), buf.numel(), ptr(foff), ptr(flen), n, ptr(r["first"]), r["nreq"],
                                            ptr(r["ledgers"]), ptr(r["firsts"]), ptr(r["flags"]), ptr(status),
                                            ptr(r["prefix"]), sp)

    ledgers_host = rq1k["ledgers"].cpu().tolist()

    def per_ledger_calls():
        for k, lid in enumerate(ledgers_host):
            rc = verify(FM, lid, 0, k * per, per)
            if rc:
                return rc
        return 0

    variants = {
        "a verify_batch": lambda: verify(),
        "b requests x1": lambda: verify_requests(F1, rq1),
        "c requests x1024": lambda: verify_requests(FM, rq1k),
        "d requests x1M": lambda: verify_requests(FM, rq1m),
        "e 1024 verify_batch": per_ledger_calls,
        "fa package_batch": lambda: package(sep, HL),
        "fb package_ledgers": lambda: package_ledgers(F1, sep2, HL),
    }
    # the frames, packaged in place (stride 4 KiB) in front of their payloads; then every route verifies them
    assert package(F1, FRAME) == 0 and package_ledgers(FM, FM, FRAME) == 0
    for name, r in (("b requests x1", rq1), ("c requests x1024", rq1k), ("d requests x1M", rq1m)):
        status.fill_(-1)
        assert variants[name]() == 0
        torch.cuda.synchronize()
        assert not status.any() and bool((r["prefix"] == r["size"]).all()), name
    for name in ("a verify_batch", "e 1024 verify_batch"):
        status.fill_(-1)
        assert variants[name]() == 0
        torch.cuda.synchronize()
        assert not status.any(), name
    assert variants["fa package_batch"]() == 0 and variants["fb package_ledgers"]() == 0
    torch.cuda.synchronize()
    assert torch.equal(sep.view(n, HL), F1.view(n, FRAME)[:, :HL]), "package_batch apart != in place"
    assert torch.equal(sep2.view(n, HL), FM.view(n, FRAME)[:, :HL]), "package_ledgers apart != in place"
    print(f"parity ok: {n} frames verify on every route; package_ledgers apart == in place", flush=True)
    for v in variants.values():  # warm-up
        for _ in range(3):
            v()
    torch.cuda.synchronize()
    res = {}
    for r in range(ROUNDS):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 2 if name.startswith("e ") else REPS  # (1 024 calls each)
            e0.record(st)
            for _ in range(reps):
                assert variants[name]() == 0
            e1.record(st)
            torch.cuda.synchronize()
            res.setdefault((name, r % 2), []).append(e0.elapsed_time(e1) / reps)
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"{'variant':22s} {'forward ms':>11s} {'reverse ms':>11s}   (median of {ROUNDS // 2} rounds x {REPS} calls; min)")
    for name in variants:
        f, b = res[(name, 0)], res.get((name, 1), [float('nan')])
        print(f"{name:22s} {med(f):11.4f} {med(b):11.4f}   min {min(f):.4f} / {min(b):.4f}", flush=True)
    for k in (0, 1):
        m = {x.split()[0]: med(res[(x, k)]) for x in variants}
        print(f"order {k}: b / a = {m['b'] / m['a']:.4f}   c / a = {m['c'] / m['a']:.4f}   d / a = {m['d'] / m['a']:.4f}   "
              f"e / c = {m['e'] / m['c']:.2f}   fb / fa = {m['fb'] / m['fa']:.4f}")


if __name__ == "__main__":
    main()
