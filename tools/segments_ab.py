"""A/B of packaging a batch of composite adds, in ONE process on the same device buffers: 1M entries of
two segments (96 B of metadata from one region, 4 000 B of payload from another region of the same
allocation), CRC32C, events on the stream, interleaved rounds in both orders (cdna_hip_programming.md
§5.4 rule 24: cross-process and first-run noise is larger than the effects measured).

  a   package_batch on a contiguous copy of the same bytes, prepared outside the timed region: the floor
  b   package_batch_segments on the two regions as they lie
  c   what a caller does without b: a device copy of each entry's two pieces into a contiguous buffer
      (two strided copies), then package_batch

Before timing, the frames of b and c must equal a's byte for byte.

Usage (GPU box): python3 tools/segments_ab.py     Environment: AB_ROUNDS (default 6), AB_N (entries).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = int(os.environ.get("AB_ROUNDS", "6"))
REPS = 10
META, PAY, HL = 96, 4000, 36
ENTRY = META + PAY


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
    i64 = dict(dtype=torch.int64, device=dev)
    # one allocation: [n x 96 B of metadata][n x 4 000 B of payload]
    A = torch.empty(n * ENTRY, dtype=torch.uint8, device=dev)
    assert L.bkd_fill_splitmix64(ptr(A), A.numel(), 11, 0, None) == 0
    meta, pay = A[:n * META].view(n, META), A[n * META:].view(n, PAY)
    idx = torch.arange(n, **i64)
    lacs = idx - 1
    lenf = torch.full((n,), ENTRY, **i64)
    seg_off = torch.stack([idx * META, n * META + idx * PAY], dim=1).reshape(-1).contiguous()
    seg_len = torch.tensor([META, PAY], dtype=torch.int32, device=dev).repeat(n)
    seg_first = torch.arange(n + 1, **i64) * 2
    # the contiguous copy of (a), made here; (c) rebuilds the same bytes in C2 inside its timed region
    C = torch.empty(n * ENTRY, dtype=torch.uint8, device=dev)
    C2 = torch.empty(n * ENTRY, dtype=torch.uint8, device=dev)
    off, ln = idx * ENTRY, torch.full((n,), ENTRY, dtype=torch.int32, device=dev)
    frames = {k: torch.empty(n * HL, dtype=torch.uint8, device=dev) for k in "abc"}
    dig = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in "abc"}

    def gather(dst):
        v = dst.view(n, ENTRY)
        v[:, :META] = meta
        v[:, META:] = pay

    def package(buf, k):
        return L.bkd_digest_package_batch(0, 7, ptr(idx), ptr(lacs), ptr(lenf), ptr(buf), buf.numel(), ptr(off), ptr(ln), n,
                                          ptr(frames[k]), HL, ptr(dig[k]), sp)

    def package_segments():
        return L.bkd_digest_package_batch_segments(0, 7, None, ptr(idx), ptr(lacs), ptr(lenf), ptr(A), A.numel(),
                                                   ptr(seg_off), ptr(seg_len), 2 * n, ptr(seg_first), n, ptr(frames["b"]),
                                                   HL, ptr(dig["b"]), sp)

    def copy_then_package():
        gather(C2)
        return package(C2, "c")

    gather(C)
    variants = {
        "a package_batch (contiguous)": lambda: package(C, "a"),
        "b package_batch_segments": package_segments,
        "c copy + package_batch": copy_then_package,
    }
    for v in variants.values():
        assert v() == 0
    assert L.bkd_stream_sync(sp) == 0
    assert torch.equal(frames["b"], frames["a"]) and torch.equal(dig["b"], dig["a"]), "segments != contiguous"
    assert torch.equal(frames["c"], frames["a"]) and torch.equal(dig["c"], dig["a"]), "copy + package != contiguous"
    print(f"parity ok: {n} entries of {META} + {PAY} B; frames of b and c equal a's", flush=True)
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
    print(f"{'variant':30s} {'forward ms':>11s} {'reverse ms':>11s}   (median of {ROUNDS // 2} rounds x {REPS} calls; min)")
    for name in variants:
        f, b = res[(name, 0)], res.get((name, 1), [float('nan')])
        print(f"{name:30s} {med(f):11.4f} {med(b):11.4f}   min {min(f):.4f} / {min(b):.4f}", flush=True)
    for k in (0, 1):
        m = {x.split()[0]: med(res[(x, k)]) for x in variants if (x, k) in res}
        if len(m) == 3:
            print(f"order {k}: b / a = {m['b'] / m['a']:.4f}   b / c = {m['b'] / m['c']:.4f}   c / a = {m['c'] / m['a']:.4f}")


if __name__ == "__main__":
    main()
