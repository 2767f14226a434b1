"""A/B several builds of libbkdigest.so in ONE process on the GPU route of the framed host entry points
(bkd_digest_verify_batch_host / bkd_digest_package_batch_host, 1M separate 4 KiB host frames):
interleaved rounds on the same host buffers, as tools/ab_libs.py does for the device batches.

Usage (GPU box): python3 tools/ab_host_route.py lib.so [lib.so ...]     (ROUNDS: rounds, default 8)
Every library stages through pinned buffers of its own, and where those land moves a library's time
by 10-20 % between processes and between copies of one file (profiles/glue_fold_ab_host_gpu_route_probe*):
pass two or three copies of each build and compare the groups, not single libraries.
"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(paths):
    import torch
    from bookkeeper_amd import _native
    libs = {}
    for p in paths:
        L = ctypes.CDLL(os.path.abspath(p))
        for fn, (res, args) in _native.PROTOTYPES.items():
            if hasattr(L, fn):
                getattr(L, fn).restype = res
                getattr(L, fn).argtypes = args
        libs[os.path.basename(p) + "#" + str(len(libs))] = L
    n, Lf, mac = 1 << 20, 4096, 4
    plen = Lf - 32 - mac
    dev = torch.empty(n * Lf, dtype=torch.uint8, device="cuda")
    first = next(iter(libs.values()))
    first.bkd_fill_splitmix64(ctypes.c_void_p(dev.data_ptr()), dev.numel(), 42, 0, None)
    torch.cuda.synchronize()
    host = np.ascontiguousarray(dev.cpu().numpy())
    del dev
    ids = np.arange(n, dtype=np.int64)
    lacs = ids - 1
    lf = np.full(n, plen, dtype=np.int64)
    base = host.ctypes.data
    pay_ptrs = (base + ids.astype(np.uint64) * Lf + 32 + mac).astype(np.uint64)
    pay_lens = np.full(n, plen, dtype=np.uint32)
    hdrs = np.zeros((n, 32 + mac), dtype=np.uint8)
    digests = np.zeros(n, dtype=np.uint32)
    frame_ptrs = (base + ids.astype(np.uint64) * Lf).astype(np.uint64)
    frame_lens = np.full(n, Lf, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    fb = ctypes.c_uint64(0)
    vp = ctypes.c_void_p

    def package(L):
        assert L.bkd_digest_package_batch_host(0, 7, vp(ids.ctypes.data), vp(lacs.ctypes.data), vp(lf.ctypes.data),
                                               vp(pay_ptrs.ctypes.data), vp(pay_lens.ctypes.data), n,
                                               vp(hdrs.ctypes.data), 32 + mac, vp(digests.ctypes.data)) == 0

    def verify(L):
        assert L.bkd_digest_verify_batch_host(0, 7, 0, 0, vp(frame_ptrs.ctypes.data), vp(frame_lens.ctypes.data), n,
                                              vp(status.ctypes.data), ctypes.byref(fb)) == 0

    first.bkd_set_host_batch_route(1)
    package(first)
    host.reshape(n, Lf)[:, :32 + mac] = hdrs
    want = digests.copy()
    for L in libs.values():
        assert L.bkd_set_host_batch_route(2) == 0
        for _ in range(2):
            verify(L)
            assert fb.value == n and (status == 0).all()
            package(L)
            assert (digests == want).all()
    res = {}
    for _ in range(int(os.environ.get("ROUNDS", "8"))):
        for name, L in libs.items():
            for what, fn in (("verify", verify), ("package", package)):
                t0 = time.perf_counter()
                for _ in range(2):
                    fn(L)
                res.setdefault((what, name), []).append((time.perf_counter() - t0) / 2 * 1e3)
    for (what, name), v in sorted(res.items()):
        s = sorted(v)
        print(f"{what:8s} {name:16s} mean {sum(v) / len(v):7.2f} ms  median {s[len(s) // 2]:7.2f}  min {s[0]:7.2f}  "
              f"max {s[-1]:7.2f}  all {' '.join(f'{x:.1f}' for x in v)}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
