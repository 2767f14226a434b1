"""A/B of the MAC add paths, in ONE process on the same device bytes: 1M entries of 96 + 4 000 B (the entries
of tools/segments_ab.py: a metadata piece and a message piece), 1 024 ledgers with a key each, HIP events on
the stream, median of 5.

  a   package_batch_ledgers_mac on the bytes already contiguous (the yardstick)
  b   package_batch_segments_mac on the two pieces as they lie
  c   what a caller does without b: copy the pieces together, then a
  d   package_batch_v2_mac for the 4 KiB payloads under the default threshold: heads and payloads in one call
  e   what a caller does without d: a, then a separate pass that writes the prefixes, moves the frames in
      and copies the payloads

The claims to confirm or withdraw: b is under c, d is under e. Before timing, b's frames must equal a's,
d's requests must equal e's, and sampled frames must equal hmac's.

Usage (GPU box): python3 tools/mac_adds_ab.py   Environment: MAC_ADDS_N (entries, a multiple of 1 024,
default 1M), MAC_ADDS_REPS (5), MAC_ADDS_LOG (default profiles/mac_adds_ab_1m.log).
"""
import hashlib
import hmac
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = int(os.environ.get("MAC_ADDS_N", str(1 << 20)))
REPS = int(os.environ.get("MAC_ADDS_REPS", "5"))
LOG = os.environ.get("MAC_ADDS_LOG", os.path.join(ROOT, "profiles", "mac_adds_ab_1m.log"))
META, MSG, NLEDGERS = 96, 4000, 1024
LEN = META + MSG
MASTER = bytes(range(20))


def main():
    import numpy as np
    import torch

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

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    i64 = dict(dtype=torch.int64, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    say(f"mac_adds_ab: {torch.cuda.get_device_name(0)}, {N} entries of {META} + {MSG} B, {NLEDGERS} ledgers, "
        f"reps {REPS}")

    passwords = [b"ledger-%d" % k for k in range(NLEDGERS)]
    table = torch.from_numpy(dg.mac_key_table(passwords).view(np.int32).copy()).to(dev)
    # the pieces as they lie: all metadata pieces, then all message pieces
    pieces = torch.empty(N * LEN, **u8)
    ck.fill_splitmix64(pieces, 2025)
    metas, msgs = pieces[:N * META].view(N, META), pieces[N * META:].view(N, MSG)
    joined = torch.empty((N, LEN), **u8)

    def join():
        joined[:, :META] = metas
        joined[:, META:] = msgs

    join()
    idx = torch.arange(N, **i64)
    lenf = torch.full((N,), LEN, **i64)
    ledger_of = 1000 + (idx // per) * 0x100000001
    key_of = (idx // per).to(torch.int32)
    ids, lacs = idx % per, idx % per - 1
    off, ln = idx * LEN, torch.full((N,), LEN, dtype=torch.int32, device=dev)
    seg_off = torch.stack([idx * META, N * META + idx * MSG], dim=1).contiguous().view(-1)
    seg_len = torch.tensor([META, MSG], dtype=torch.int32, device=dev).repeat(N)
    seg_first = torch.arange(N + 1, **i64) * 2
    flat = joined.view(-1)
    frames_a = torch.empty((N, 52), **u8)
    frames_b = torch.empty((N, 52), **u8)
    RQ = 80 + LEN
    req_off = idx * RQ
    req_d = torch.empty(N * RQ, **u8)
    req_e = torch.empty((N, RQ), **u8)
    prefix = torch.tensor(list(struct.pack(">II", 76 + LEN, (2 << 24) | (1 << 16)) + MASTER), **u8).repeat(N, 1)

    def a():
        return dg.package_batch_ledgers_mac(table, key_of, ledger_of, ids, lacs, lenf, flat, off, ln)

    def a_into():
        frames, _ = a()
        frames_a.copy_(frames)

    def b():
        dg.package_batch_segments_mac(table, key_of, ledger_of, ids, lacs, lenf, pieces, seg_off, seg_len, seg_first,
                                      out_frames=frames_b)

    def c():
        join()
        a()

    def d():
        dg.package_batch_v2_mac(table, key_of, ledger_of, ids, lacs, lenf, flat, off, ln, MASTER, requests=req_d,
                                request_offsets=req_off, with_macs=False)

    def e():
        frames, _ = a()
        req_e[:, :28] = prefix
        req_e[:, 28:80] = frames
        req_e[:, 80:] = joined

    a_into()
    b()
    d()
    e()
    ck.stream_sync(st)
    assert torch.equal(frames_a, frames_b), "b's frames differ from a's"
    assert torch.equal(req_d.view(N, RQ), req_e), "d's requests differ from e's"
    for i in (0, 1, per - 1, per, N // 3, N - 1):
        body = joined[i].cpu().numpy().tobytes()
        k = i // per
        hdr = struct.pack(">qqqq", 1000 + k * 0x100000001, i % per, i % per - 1, LEN)
        key = hashlib.sha1(b"mac" + passwords[k]).digest()
        assert frames_b[i].cpu().numpy().tobytes() == hdr + hmac.digest(key, hdr + body, "sha1"), f"frame {i}"
    say(f"parity ok: b's {N} frames equal a's, d's requests equal e's, sampled frames equal hmac's")

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
        return sorted(ms)[len(ms) // 2], min(ms), max(ms)

    gb = N * LEN / 1e9
    med = {}
    # two rounds in alternating order: the second shows the spread of the first
    for rnd in (1, 2):
        for name, fn in (("a  contiguous, ledgers_mac", a), ("b  segments_mac on the pieces", b),
                         ("c  join the pieces, then a", c), ("d  v2_mac, heads and payloads", d),
                         ("e  a, then a head-and-copy pass", e)):
            m, lo, hi = timed(fn)
            med.setdefault(name[0], []).append(m)
            say(f"round {rnd}  {name:34s} median {m:9.3f} ms (min {lo:.3f}, max {hi:.3f})  "
                f"{gb / (m / 1e3):8.1f} GB/s of payload")
    mean = {k: sum(v) / len(v) for k, v in med.items()}
    say(f"b / a = {mean['b'] / mean['a']:.4f}   b / c = {mean['b'] / mean['c']:.4f}   "
        f"d / a = {mean['d'] / mean['a']:.4f}   d / e = {mean['d'] / mean['e']:.4f}")
    say(f"claim b under c: {'confirmed' if mean['b'] < mean['c'] else 'NOT confirmed'};  "
        f"claim d under e: {'confirmed' if mean['d'] < mean['e'] else 'NOT confirmed'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
