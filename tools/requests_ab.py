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
  ga / gb  fa / fb with each frame written in place in front of its payload (the header-first route)
  ha / hc  a / c with frame 5 cut to 2 KiB: out of the gate's band, so the header / plan / finish
           sequence runs (and frame 5, cut short, is the one digest mismatch)

Before timing, every route must verify every frame (the frames are packaged per ledger for c / d / e
and for one ledger for a / b) and fa's and fb's frames must equal the frames packaged in place.

Usage (GPU box): python3 tools/requests_ab.py [lib.so ...]
Default library: bookkeeper_amd/libbkdigest.so. Several libraries (as tools/ab_libs.py takes them) are
timed row by row in the same rounds on the same buffers; the first is the yardstick, and every other
library's row is printed as its difference from the first's. Giving a second copy of the first
library (under another file name, so that it is loaded again) shows the spread between two loads of
the same code, the margin for the others.
Environment: AB_ROUNDS (default 6), AB_N (entries, a multiple of 1 024), AB_ROWS (row letters to
run, default all).
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


def main(paths):
    import torch
    from bookkeeper_amd import _native

    libs = {}
    for p in paths:
        lib = ctypes.CDLL(os.path.abspath(p))
        for fn, (res, args) in _native.PROTOTYPES.items():
            if hasattr(lib, fn):
                getattr(lib, fn).restype = res
                getattr(lib, fn).argtypes = args
        libs[os.path.basename(p)] = lib
    L = next(iter(libs.values()))  # fills the buffers and packages the frames every library verifies
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
    flen_cut = flen.clone()
    flen_cut[5] = FRAME // 2
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

    def package(L, frames, stride, lacs=idx - 1):
        return L.bkd_digest_package_batch(0, 7, ptr(idx), ptr(lacs), ptr(lenf), ptr(F1), F1.numel(), ptr(poff), ptr(plen),
                                          n, ptr(frames), stride, ptr(dig), sp)

    def package_ledgers(L, buf, frames, stride):
        return L.bkd_digest_package_batch_ledgers(0, ptr(ledger_of), ptr(ids_m), ptr(ids_m), ptr(lenf), ptr(buf),
                                                  buf.numel(), ptr(poff), ptr(plen), n, ptr(frames), stride, ptr(dig), sp)

    def verify(L, buf=F1, ledger=7, first=0, lo=0, cnt=n, flen=flen):
        return L.bkd_digest_verify_batch(0, ledger, first, 0, ptr(buf), buf.numel(), ptr(foff, 8 * lo), ptr(flen, 4 * lo),
                                         cnt, ptr(status, 4 * lo), ptr(fb), sp)

    def verify_requests(L, buf, r, flen=flen):
        return L.bkd_digest_verify_requests(0, ptr(buf), buf.numel(), ptr(foff), ptr(flen), n, ptr(r["first"]), r["nreq"],
                                            ptr(r["ledgers"]), ptr(r["firsts"]), ptr(r["flags"]), ptr(status),
                                            ptr(r["prefix"]), sp)

    ledgers_host = rq1k["ledgers"].cpu().tolist()

    def per_ledger_calls(L):
        for k, lid in enumerate(ledgers_host):
            rc = verify(L, FM, lid, 0, k * per, per)
            if rc:
                return rc
        return 0

    variants = {
        "a verify_batch": lambda L: verify(L),
        "b requests x1": lambda L: verify_requests(L, F1, rq1),
        "c requests x1024": lambda L: verify_requests(L, FM, rq1k),
        "d requests x1M": lambda L: verify_requests(L, FM, rq1m),
        "e 1024 verify_batch": per_ledger_calls,
        "fa package_batch": lambda L: package(L, sep, HL),
        "fb package_ledgers": lambda L: package_ledgers(L, F1, sep2, HL),
        # in place: the frames and digests already there are written again with the same bytes
        "ga package in place": lambda L: package(L, F1, FRAME),
        "gb ledgers in place": lambda L: package_ledgers(L, FM, FM, FRAME),
        "ha verify, one cut": lambda L: verify(L, flen=flen_cut),
        "hc x1024, one cut": lambda L: verify_requests(L, FM, rq1k, flen=flen_cut),
    }
    rows = os.environ.get("AB_ROWS", "").split()
    if rows:
        variants = {k: v for k, v in variants.items() if k.split()[0] in rows}
    # the frames, packaged in place (stride 4 KiB) in front of their payloads; then every route of
    # every library verifies them
    assert package(L, F1, FRAME) == 0 and package_ledgers(L, FM, FM, FRAME) == 0
    for lname, lib in libs.items():
        for name, r in (("b requests x1", rq1), ("c requests x1024", rq1k), ("d requests x1M", rq1m)):
            if name in variants:
                status.fill_(-1)
                assert variants[name](lib) == 0
                torch.cuda.synchronize()
                assert not status.any() and bool((r["prefix"] == r["size"]).all()), (lname, name)
        for name in ("a verify_batch", "e 1024 verify_batch"):
            if name in variants:
                status.fill_(-1)
                fb.fill_(-1)
                assert variants[name](lib) == 0
                torch.cuda.synchronize()
                assert not status.any() and int(fb.item()) in (n, per), (lname, name)
        for name, prefix in (("ha verify, one cut", fb), ("hc x1024, one cut", rq1k["prefix"])):
            if name in variants:
                status.fill_(-1)
                assert variants[name](lib) == 0
                torch.cuda.synchronize()
                assert status.nonzero().flatten().tolist() == [5] and int(status[5]) == 2, (lname, name)
                assert int(prefix[0]) == 5 and (name[1] == "a" or bool((prefix[1:] == per).all())), (lname, name)
        for name, out, want in (("fa package_batch", sep, F1), ("fb package_ledgers", sep2, FM)):
            if name in variants:
                out.fill_(0)
                assert variants[name](lib) == 0
                torch.cuda.synchronize()
                assert torch.equal(out.view(n, HL), want.view(n, FRAME)[:, :HL]), (lname, name, "apart != in place")
        for name, buf in (("ga package in place", F1), ("gb ledgers in place", FM)):
            if name in variants:
                before = buf.view(n, FRAME)[:, :HL].clone()
                buf.view(n, FRAME)[:, :HL] = 0
                assert variants[name](lib) == 0
                torch.cuda.synchronize()
                assert torch.equal(buf.view(n, FRAME)[:, :HL], before), (lname, name, "in place differs")
    print(f"parity ok: {n} frames verify on every route of {len(libs)} libraries; packaged apart == in place", flush=True)
    for v in variants.values():  # warm-up
        for lib in libs.values():
            for _ in range(3):
                v(lib)
    torch.cuda.synchronize()
    res = {}
    for r in range(ROUNDS):
        order = [(name, lname) for name in variants for lname in libs]
        for name, lname in (order if r % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 2 if name.startswith("e ") else REPS  # (1 024 calls each)
            e0.record(st)
            for _ in range(reps):
                assert variants[name](libs[lname]) == 0
            e1.record(st)
            torch.cuda.synchronize()
            res.setdefault((name, lname, r % 2), []).append(e0.elapsed_time(e1) / reps)
    med = lambda v: sorted(v)[len(v) // 2]
    yard = next(iter(libs))
    print(f"{'variant':22s} {'library':26s} {'forward ms':>11s} {'reverse ms':>11s}   (median of {ROUNDS // 2} rounds x "
          f"{REPS} calls; min; median - {yard}'s in us)")
    for name in variants:
        for lname in libs:
            f, b = res[(name, lname, 0)], res.get((name, lname, 1), [float('nan')])
            line = f"{name:22s} {lname:26s} {med(f):11.4f} {med(b):11.4f}   min {min(f):.4f} / {min(b):.4f}"
            if lname != yard:
                y0, y1 = res[(name, yard, 0)], res.get((name, yard, 1), [float('nan')])
                line += f"   {1e3 * (med(f) - med(y0)):+7.1f} / {1e3 * (med(b) - med(y1)):+7.1f}"
            print(line, flush=True)
    for lname in libs:
        for k in (0, 1):
            m = {x.split()[0]: med(res[(x, lname, k)]) for x in variants if (x, lname, k) in res}
            ratio = lambda p, q: f"{p} / {q} = {m[p] / m[q]:.4f}" if p in m and q in m else ""
            print(f"{lname} order {k}: " + "   ".join(filter(None, (ratio("b", "a"), ratio("c", "a"), ratio("d", "a"),
                                                                   ratio("e", "c"), ratio("fb", "fa"), ratio("gb", "ga")))))


if __name__ == "__main__":
    main(sys.argv[1:] or [os.path.join(ROOT, "bookkeeper_amd", "libbkdigest.so")])
