"""A/B of re-framing a MAC (HMAC-SHA1) batch that spans many ledgers with a new LAC, in ONE process on the
same device bytes: 1M framed 4 KiB entries as 1 024 requests of 1 024 ledgers with a key each, HIP events on
the stream, every leg through the C call with preallocated outputs.

  a    today's two-call way at its floor: bkd_digest_verify_requests_mac, then
       bkd_digest_package_batch_ledgers_mac over the same payloads where they lie, nothing on the host in between
  p    bkd_digest_package_batch_ledgers_mac alone (the yardstick of the trusted reframe)
  b    bkd_digest_reframe_requests_mac, default: verify and re-frame in one pass, out-frames apart
  c    the same, BKD_REFRAME_TRUSTED
  b'   b in place (timed last: it rewrites the frames, which verify again afterwards)

Before timing, b's and c's out-frames must equal the package call's for the new LACs, sampled frames must
equal hmac's, and every status must be 0. Each leg is timed REPS times in each of ROUNDS rounds (the legs
interleaved round by round); all samples are printed, then median, minimum and maximum per leg: the spread
is what a ratio has to beat.

Usage (GPU box): python3 tools/mac_reframe_ab.py   Environment: MAC_RF_N (entries, a multiple of 1 024,
default 1M), MAC_RF_REPS (5), MAC_RF_ROUNDS (3), MAC_RF_LOG (default profiles/mac_reframe_ab_1m4k.log).
"""
import ctypes
import hmac
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("MAC_RF_N", str(1 << 20)))
REPS = int(os.environ.get("MAC_RF_REPS", "5"))
ROUNDS = int(os.environ.get("MAC_RF_ROUNDS", "3"))
LOG = os.environ.get("MAC_RF_LOG", os.path.join(ROOT, "profiles", "mac_reframe_ab_1m4k.log"))
L4K, FL, NLEDGERS = 4096, 52 + 4096, 1024


def main():
    import hashlib

    import numpy as np
    import torch

    from bookkeeper_amd import _native
    from bookkeeper_amd import checksum as ck
    from bookkeeper_amd import digest as dg

    assert N % NLEDGERS == 0
    per = N // NLEDGERS
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log = open(LOG, "w")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    L = _native.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = dict(dtype=torch.int64, device=dev)
    say(f"mac_reframe_ab: {torch.cuda.get_device_name(0)}, {N} entries of {L4K} B, {NLEDGERS} requests / ledgers, "
        f"reps {REPS}, rounds {ROUNDS}")

    passwords = [b"ledger-%d" % k for k in range(NLEDGERS)]
    table = torch.from_numpy(dg.mac_key_table(passwords).view(np.int32).copy()).to(dev)
    payload = torch.empty(N * L4K, dtype=torch.uint8, device=dev)
    ck.fill_splitmix64(payload, 2025)
    idx = torch.arange(N, **i64)
    lenf = torch.full((N,), L4K, **i64)
    off, ln = idx * L4K, torch.full((N,), L4K, dtype=torch.int32, device=dev)
    ledger_of = 1000 + (idx // per) * 0x100000001  # distinct in both words
    key_of = (idx // per).to(torch.int32)
    ids = idx % per                                 # entry ids restart in every ledger
    ledgers_h = (1000 + np.arange(NLEDGERS, dtype=np.int64) * 0x100000001).tolist()
    new_lacs = ids + 12345

    heads, _ = dg.package_batch_ledgers_mac(table, key_of, ledger_of, ids, ids - 1, lenf, payload, off, ln, sync_check=True)
    FM = torch.cat([heads, payload.view(N, L4K)], dim=1).contiguous().view(-1)
    del payload, heads
    foff, fln = idx * FL, torch.full((N,), FL, dtype=torch.int32, device=dev)
    poff = foff + 52  # the payloads where they lie, behind their frames' heads
    first, ledgers = torch.arange(NLEDGERS + 1, **i64) * per, torch.tensor(ledgers_h, **i64)
    firsts, rflags = torch.zeros(NLEDGERS, **i64), torch.zeros(NLEDGERS, dtype=torch.int32, device=dev)
    rkeys = torch.arange(NLEDGERS, dtype=torch.int32, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    prefix = torch.empty(NLEDGERS, **i64)
    out = torch.empty((N, 52), dtype=torch.uint8, device=dev)

    def verify():
        assert L.bkd_digest_verify_requests_mac(ptr(table), NLEDGERS, ptr(rkeys), ptr(FM), FM.numel(), ptr(foff), ptr(fln), N,
                                                ptr(first), NLEDGERS, ptr(ledgers), ptr(firsts), ptr(rflags), ptr(status),
                                                ptr(prefix), sp) == 0

    def package():
        assert L.bkd_digest_package_batch_ledgers_mac(ptr(table), NLEDGERS, ptr(key_of), ptr(ledger_of), ptr(ids),
                                                      ptr(new_lacs), ptr(lenf), ptr(FM), FM.numel(), ptr(poff), ptr(ln), N,
                                                      ptr(out), 52, sp) == 0

    def reframe(flags, apart=True):
        assert L.bkd_digest_reframe_requests_mac(ptr(table), NLEDGERS, ptr(rkeys), flags, ptr(FM), FM.numel(), ptr(foff),
                                                 ptr(fln), N, ptr(first), NLEDGERS, ptr(ledgers), ptr(firsts), ptr(rflags),
                                                 ptr(new_lacs), ptr(out) if apart else None, 52 if apart else 0,
                                                 ptr(status), ptr(prefix), sp) == 0

    def leg_a():
        verify()
        package()

    legs = [("a   verify, then package", leg_a), ("p   package alone", package),
            ("b   reframe, default", lambda: reframe(0)), ("c   reframe, trusted", lambda: reframe(_native.REFRAME_TRUSTED))]

    # ---- parity ----
    def clean():
        ck.stream_sync(st)
        return not status.any().item() and bool((prefix == per).all())

    status.fill_(-1)
    leg_a()
    assert clean(), "leg a"
    want = out.clone()
    for i in (0, 1, per - 1, per, N // 3, N - 1):
        k = i // per
        body = FM[i * FL + 52:(i + 1) * FL].cpu().numpy().tobytes()
        hdr = struct.pack(">qqqq", ledgers_h[k], i % per, i % per + 12345, L4K)
        keyk = hashlib.sha1(b"mac" + passwords[k]).digest()
        assert want[i].cpu().numpy().tobytes() == hdr + hmac.digest(keyk, hdr + body, "sha1"), f"frame {i}"
    for name, flags in (("b", 0), ("c", _native.REFRAME_TRUSTED)):
        out.fill_(0)
        status.fill_(-1)
        reframe(flags)
        assert clean() and torch.equal(out, want), f"leg {name}"
    say(f"parity ok: sampled frames equal hmac's, all {N} statuses 0 on every leg, b and c write a's out-frames")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    samples = {name: [] for name, _ in legs}
    for rnd in range(ROUNDS):
        for name, fn in legs:
            ms = timed(fn)
            samples[name] += ms
            say(f"round {rnd}  {name:28s} " + " ".join(f"{x:.3f}" for x in ms))
    inplace = "b'  reframe, default, in place"
    samples[inplace] = timed(lambda: reframe(0, apart=False)) + timed(lambda: reframe(0, apart=False))
    assert clean(), "leg b'"
    say(f"         {inplace:28s} " + " ".join(f"{x:.3f}" for x in samples[inplace]))
    verify()
    assert clean(), "the frames re-framed in place verify"

    gb = N * L4K / 1e9
    med = {}
    for name, ms in samples.items():
        ms = sorted(ms)
        med[name[0:2].strip()] = m = ms[len(ms) // 2]
        say(f"{name:32s} median {m:8.3f} ms  min {ms[0]:8.3f}  max {ms[-1]:8.3f}  spread {(ms[-1] - ms[0]) / m * 100:5.1f} %"
            f"  {gb / (m / 1e3):8.1f} GB/s of payload")
    a, p, b, c, b_in_place = (med[k] for k in ("a", "p", "b", "c", "b'"))
    say(f"b / a = {b / a:.4f}   c / p = {c / p:.4f}   b' / b = {b_in_place / b:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
