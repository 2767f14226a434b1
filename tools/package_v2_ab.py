"""A/B of packaging V2 add requests whole, in ONE process on the same device buffers: 1M entries of
4 KiB, CRC32C, every entry under the 16 KiB threshold, requests packed (4 160 B apart), events on the
stream, interleaved rounds in both orders (cdna_hip_programming.md §5.4 rule 24: cross-process and
first-run noise is larger than the effects measured).

  a   package_batch alone: the floor (no request is assembled)
  b   what a caller does without the new call: package_batch, then the requests assembled with torch
      (the 28-byte prefixes built from the lengths, prefix / frame / payload scattered with strided copies;
      the uniform length is what lets torch do that without a kernel of the caller's own)
  c   package_batch_v2: digests, head kernel, copy kernel
  d   a fused route (fold and copy in one kernel, then the head kernel), timed only on a build that has
      one behind bkd_set_package_v2_route(2); the library does not (it lost: DESIGN.md §3, §5e)

Before timing, the request buffers of b, c and d must be equal byte for byte, and their digests a's.

Usage (GPU box): python3 tools/package_v2_ab.py     Environment: AB_ROUNDS (default 6), AB_N (entries).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = int(os.environ.get("AB_ROUNDS", "6"))
REPS = 10
PAY, HL, PREFIX = 4096, 36, 28
REQ = PREFIX + HL + PAY
SMALL = 16384
FLAGS = 0x0002


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
    u8 = dict(dtype=torch.uint8, device=dev)
    P = torch.empty(n * PAY, **u8)
    assert L.bkd_fill_splitmix64(ptr(P), P.numel(), 11, 0, None) == 0
    idx = torch.arange(n, **i64)
    lacs = idx - 1
    lenf = (idx + 1) * PAY
    off = idx * PAY
    ln = torch.full((n,), PAY, dtype=torch.int32, device=dev)
    key = torch.arange(20, **u8) * 7 + 1
    roff = idx * REQ
    has_fused = hasattr(L, "bkd_set_package_v2_route")
    names = "bcd" if has_fused else "bc"
    req = {k: torch.zeros(n * REQ, **u8) for k in names}
    dig = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in "a" + names}
    frames = torch.empty(n * HL, **u8)
    shifts = torch.tensor([24, 16, 8, 0], **i64)
    pkt = torch.tensor([2, 1, FLAGS >> 8, FLAGS & 255], **u8)  # PacketHeader.toInt(2, ADDENTRY, flags), BE

    def package(k):
        return L.bkd_digest_package_batch(0, 7, ptr(idx), ptr(lacs), ptr(lenf), ptr(P), P.numel(), ptr(off), ptr(ln), n,
                                          ptr(frames), HL, ptr(dig[k]), sp)

    def assemble():
        rc = package("b")
        R = req["b"].view(n, REQ)
        size = ln.to(torch.int64) + (PREFIX - 4 + HL)  # headersSize + payloadSize
        R[:, 0:4] = ((size.unsqueeze(1) >> shifts) & 255).to(torch.uint8)
        R[:, 4:8] = pkt
        R[:, 8:PREFIX] = key
        R[:, PREFIX:PREFIX + HL] = frames.view(n, HL)
        R[:, PREFIX + HL:] = P.view(n, PAY)
        return rc

    def v2(k, route):
        if has_fused:
            assert L.bkd_set_package_v2_route(route) == 0
        return L.bkd_digest_package_batch_v2(0, 7, None, ptr(idx), ptr(lacs), ptr(lenf), ptr(P), P.numel(), ptr(off),
                                             ptr(ln), n, ptr(key), 0, FLAGS, SMALL, ptr(req[k]), req[k].numel(),
                                             ptr(roff), ptr(dig[k]), sp)

    variants = {
        "a package_batch alone": lambda: package("a"),
        "b package_batch + torch assembly": assemble,
        "c package_batch_v2 two-pass": lambda: v2("c", 1),
    }
    if has_fused:
        variants["d package_batch_v2 fused"] = lambda: v2("d", 2)
    for v in variants.values():
        assert v() == 0
    assert L.bkd_stream_sync(sp) == 0
    for k in names:
        assert torch.equal(dig[k], dig["a"]), f"digests of {k} != a"
    for k in names[1:]:
        assert torch.equal(req[k], req["b"]), f"requests of {k} != b"
    print(f"parity ok: {n} entries of {PAY} B; requests of {', '.join(names)} equal byte for byte", flush=True)
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
    if has_fused:
        assert L.bkd_set_package_v2_route(0) == 0
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"{'variant':34s} {'forward ms':>11s} {'reverse ms':>11s}   (median of {ROUNDS // 2} rounds x {REPS} calls; min)")
    for name in variants:
        f, b = res[(name, 0)], res.get((name, 1), [float('nan')])
        print(f"{name:34s} {med(f):11.4f} {med(b):11.4f}   min {min(f):.4f} / {min(b):.4f}", flush=True)
    for k in (0, 1):
        m = {x.split()[0]: med(res[(x, k)]) for x in variants if (x, k) in res}
        line = f"order {k}: c / a = {m['c'] / m['a']:.4f}   c / b = {m['c'] / m['b']:.4f}   b / a = {m['b'] / m['a']:.4f}"
        if "d" in m:
            line += f"   d / c = {m['d'] / m['c']:.4f}   d / a = {m['d'] / m['a']:.4f}"
        print(line)


if __name__ == "__main__":
    main()
