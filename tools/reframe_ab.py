"""A/B of the re-replication digest work in ONE process on the same device buffers: 1M framed 4 KiB
entries (CRC32C), events on the stream, interleaved rounds in both orders (cdna_hip_programming.md §5.4
rule 24: cross-process and first-run noise is larger than the effects measured).

  a  verify_batch
  b  verify_batch, then package_batch of the same payloads with the new LACs into packed frames
     (the route before bkd_digest_reframe_batch)
  c  reframe_batch, out-frames apart and packed          ci  the same in place
  d  reframe_batch trusted, apart and packed             di  the same in place

Before timing, c's frames and digests must equal b's bit for bit. Every call re-frames with LACs that
differ from the stored ones (the in-place variants alternate between two sets), so the per-entry
product by x^(8 * payload length) is never skipped.

Usage (GPU box): python3 tools/reframe_ab.py        Environment: AB_ROUNDS (default 6), AB_N (entries),
AB_EQUAL_LACS=1 (diagnostic: c and d re-frame with the LACs the frames already hold, which skips the
per-entry product; the difference to a normal run is the product's cost; ci and di are left out).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = int(os.environ.get("AB_ROUNDS", "6"))
REPS = 10
FRAME, HL = 4096, 36


def main():
    import torch
    from bookkeeper_amd import _native

    L = _native.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n = int(os.environ.get("AB_N", str(1 << 20)))
    F = torch.empty(n * FRAME, dtype=torch.uint8, device=dev)
    assert L.bkd_fill_splitmix64(ptr(F), F.numel(), 7, 0, None) == 0
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    lenf = torch.full((n,), FRAME - HL, dtype=torch.int64, device=dev)
    poff, plen = ids * FRAME + HL, torch.full((n,), FRAME - HL, dtype=torch.int32, device=dev)
    foff, flen = ids * FRAME, torch.full((n,), FRAME, dtype=torch.int32, device=dev)
    lac_new = ids + 5  # apart: always different from the stored LAC
    lac_alt = [ids + 1, ids + 2]  # in place: alternating, so each call changes every LAC
    dig = torch.empty(n, dtype=torch.int32, device=dev)
    dig2 = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    fb = torch.empty(1, dtype=torch.int64, device=dev)
    sep = torch.empty(n * HL, dtype=torch.uint8, device=dev)
    sep2 = torch.empty(n * HL, dtype=torch.uint8, device=dev)
    flip = [0]

    def package(lacs, frames, stride, out_dig):
        return L.bkd_digest_package_batch(0, 7, ptr(ids), ptr(lacs), ptr(lenf), ptr(F), F.numel(), ptr(poff), ptr(plen),
                                          n, ptr(frames), stride, ptr(out_dig), sp)

    def verify():
        return L.bkd_digest_verify_batch(0, 7, 0, 0, ptr(F), F.numel(), ptr(foff), ptr(flen), n, ptr(status), ptr(fb), sp)

    def reframe(flags, out, lacs):
        return L.bkd_digest_reframe_batch(0, 7, 0, 0, flags, ptr(F), F.numel(), ptr(foff), ptr(flen), n, ptr(lacs),
                                          ptr(out) if out is not None else None, HL if out is not None else 0,
                                          ptr(dig2), ptr(status), ptr(fb), sp)

    def alt():
        flip[0] ^= 1
        return lac_alt[flip[0]]

    variants = {
        "a verify": lambda: verify(),
        "b verify+package": lambda: verify() or package(lac_new, sep, HL, dig),
        "c reframe apart": lambda: reframe(0, sep2, lac_new),
        "d trusted apart": lambda: reframe(1, sep2, lac_new),
        "ci reframe in place": lambda: reframe(0, None, alt()),
        "di trusted in place": lambda: reframe(1, None, alt()),
    }
    # the frames: packaged in place (stride 4 KiB) with LAC = id - 1; then parity of c against b
    assert package(ids - 1, F, FRAME, dig) == 0
    assert variants["b verify+package"]() == 0
    torch.cuda.synchronize()
    assert int(fb.item()) == n and not status.any()
    for name in ("c reframe apart", "d trusted apart"):
        sep2.zero_()
        assert variants[name]() == 0
        torch.cuda.synchronize()
        assert int(fb.item()) == n and not status.any(), name
        assert torch.equal(sep2, sep) and torch.equal(dig2, dig), name
    for name in ("ci reframe in place", "di trusted in place"):
        assert variants[name]() == 0
        assert verify() == 0
        torch.cuda.synchronize()
        assert int(fb.item()) == n, name  # the re-framed frames verify
    print(f"parity ok: reframe == verify + package on {n} frames; in-place frames verify", flush=True)
    if os.environ.get("AB_EQUAL_LACS"):
        lac_new.copy_(lac_alt[flip[0]])  # what the last in-place call stored
        del variants["ci reframe in place"], variants["di trusted in place"]
        print("AB_EQUAL_LACS: c and d skip the per-entry product", flush=True)
    for v in variants.values():  # warm-up
        for _ in range(3):
            v()
    torch.cuda.synchronize()
    res = {}
    for r in range(ROUNDS):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(REPS):
                assert variants[name]() == 0
            e1.record(st)
            torch.cuda.synchronize()
            res.setdefault((name, r % 2), []).append(e0.elapsed_time(e1) / REPS)
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"{'variant':22s} {'forward ms':>11s} {'reverse ms':>11s}   (median of {ROUNDS // 2} rounds x {REPS} calls; min)")
    for name in variants:
        f, b = res[(name, 0)], res.get((name, 1), [float('nan')])
        print(f"{name:22s} {med(f):11.4f} {med(b):11.4f}   min {min(f):.4f} / {min(b):.4f}", flush=True)
    for k in (0, 1):
        a, b, c = (med(res[(x, k)]) for x in ("a verify", "b verify+package", "c reframe apart"))
        print(f"order {k}: c / b = {c / b:.4f}   c - a = {1000 * (c - a):.1f} us   b - a = {1000 * (b - a):.1f} us")


if __name__ == "__main__":
    main()
