"""CPU: what every host-resident binding does with its arguments, form by form, on the library's CPU route.

The values the forms compute are other suites' business. Pinned here, for batches of five entries of 0 to
100 bytes: (a) the ValueError text when the id arrays and the payloads disagree in size, (b) the return
code and bkd_last_error when entry 3 of 5 is a null pointer with a length (through the C-ABI directly; a
null pointer with length 0 is legal), (c) the frame_stride range of the forms that return a frame array,
(d) what an empty batch returns, (e) each result's dtype and shape, (f) for the many-ledger, composite, V2 and
read-request forms, which error is reported when two faults are present at once, and the exact texts of the CSR
and key-index errors, (g) the size texts of the MAC forms' key index.
"""
import ctypes
import functools

import numpy as np
import pytest

import mac_util as mu
from bookkeeper_amd import _native
from bookkeeper_amd import checksum as ck
from bookkeeper_amd import digest as dg

INVALID_ARG = -1
LENS = [0, 17, 100, 33, 64]
N = len(LENS)
LEDGER, FIRST, PASSWD = 7, 10, b"host forms"
PAYLOADS = mu.payloads(LENS, seed=9)
IDS = np.arange(FIRST, FIRST + N, dtype=np.int64)
LACS, LENF, LIDS = IDS - 1, np.array(LENS, dtype=np.int64), np.arange(100, 100 + N, dtype=np.int64)
KEY = bytes(range(20))
REQ_FIRST, REQ_LEDGERS, REQ_ENTRIES = [0, 2, N], [LEDGER, LEDGER], [FIRST, FIRST + 2]
CRC = {ck.CRC32C: dg.DigestType.CRC32C, ck.CRC32: dg.DigestType.CRC32}
MAC = {ck.CRC32C: 4, ck.CRC32: 8}
T = dg.DigestType.CRC32C

NO_LEDGERS = "entry_ids, lacs, length_fields and payloads must have one element per entry"
WITH_LEDGERS = "ledger_ids, entry_ids, lacs, length_fields and payloads must have one element per entry"
REQUESTS = "ledger_ids, first_entry_ids and skip_flags must have one element per request (req_first one more)"
STRIDE = "BKD_ERR_INVALID_ARG: frame_stride must be in [32 + digest length, 4096]"


@pytest.fixture(autouse=True)
def _cpu_route():
    with ck.host_batch_route(ck.HOST_ROUTE_CPU):
        yield


def _dm(algo=ck.CRC32C):
    return dg.DigestManager.instantiate(LEDGER, b"", CRC[algo])


@functools.lru_cache(None)
def _mm():
    return dg.MacDigestManager(LEDGER, PASSWD)


@functools.lru_cache(None)
def _table():
    """Two key rows; row 0 is the key of _mm() and of the "mac" frames."""
    return dg.mac_key_table([PASSWD, b"another"])


KEY_OF = np.array([0, 1, 1, 0, 1], dtype=np.uint32)


@functools.lru_cache(None)
def _frames(kind):
    """PAYLOADS as good frames of ledger LEDGER, entry ids FIRST + i: CRC32C frames or MAC frames."""
    if kind == "mac":
        return [mu.frame(FIRST + i, p, ledger=LEDGER, key=mu.mac_key(PASSWD)) for i, p in enumerate(PAYLOADS)]
    heads, _ = _dm().package_batch_host(IDS, LACS, LENF, PAYLOADS)
    return [heads[i].tobytes() + p for i, p in enumerate(PAYLOADS)]


def _entries(kind, n=N):
    return list(PAYLOADS[:n]) if kind == "payloads" else _frames(kind)[:n]


# ---- the Python bindings: name -> (what its entries are, the call, what it returns for n entries) ----
# The call takes (entries, entry ids, LACs, length fields, ledger ids, frame stride); a form uses what it has.
# A result is (dtype, shape), int for a Python int, ("requests", head) for a list of n uint8 arrays.

def _crc_batch_host(b, ids, lacs, lenf, lids, stride, seeds=None):
    lens = np.array([len(x) for x in b], dtype=np.uint32)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    return ck.crc_batch_host(ck.CRC32C, b"".join(b), offs, lens[:len(lenf)], seeds=seeds)


def _crc_segments_host(b, ids, lacs, lenf, lids, stride, seeds=None):
    return ck.crc_batch_segments_host(ck.CRC32C, b, np.arange(len(b) + 1), seeds=seeds)


def _requests(form):
    """form(frames, req_first, ledger ids, first entry ids) over the two requests, or over none for no frames."""
    def call(b, ids, lacs, lenf, lids, stride):
        if not len(b):
            return form(b, [0], [], [])
        return form(b, REQ_FIRST, REQ_LEDGERS[:2 if len(lids) == len(b) else 1], REQ_ENTRIES)
    return call


_requests_host = _requests(lambda b, *rq: dg.verify_requests_host(T, b, *rq))
_requests_mac_host = _requests(lambda b, *rq: dg.verify_requests_mac_host(_table(), [0] * (len(rq[0]) - 1), b, *rq))
_MAC_FRAMED = lambda n, stride: [(np.uint8, (n, stride or 52)), (np.uint8, (n, 20))]


def _framed(mac):
    return lambda n, stride: [(np.uint8, (n, stride or 32 + mac)), (np.uint32, (n,))]


PY = {
    "dm.verify_batch_host": ("crc", lambda b, ids, lacs, lenf, lids, stride: _dm().verify_batch_host(b, FIRST),
                             lambda n, stride: [(np.int32, (n,)), int]),
    "dm.package_batch_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                              _dm().package_batch_host(ids, lacs, lenf, b, stride), _framed(4)),
    "dm.reframe_batch_host": ("crc", lambda b, ids, lacs, lenf, lids, stride:
                              _dm().reframe_batch_host([bytearray(x) for x in b], FIRST, lacs),
                              lambda n, stride: [(np.int32, (n,)), int, (np.uint32, (n,))]),
    "dm.package_batch_segments_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                       _dm().package_batch_segments_host(ids, lacs, lenf, b, stride), _framed(4)),
    "dm.package_batch_v2_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                 _dm().package_batch_v2_host(ids, lacs, lenf, b, KEY),
                                 lambda n, stride: [("requests", 64), (np.uint32, (n,))]),
    "dg.verify_requests_host": ("crc", _requests_host,
                                lambda n, stride: [(np.int32, (n,)), (np.uint64, (2 if n else 0,))]),
    "dg.package_batch_ledgers_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                      dg.package_batch_ledgers_host(T, lids, ids, lacs, lenf, b, stride), _framed(4)),
    "dg.package_batch_segments_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                       dg.package_batch_segments_host(T, lids, ids, lacs, lenf, b, stride), _framed(4)),
    "dg.package_batch_v2_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                 dg.package_batch_v2_host(T, lids, ids, lacs, lenf, b, KEY),
                                 lambda n, stride: [("requests", 64), (np.uint32, (n,))]),
    "mac.verify_batch_host": ("mac", lambda b, ids, lacs, lenf, lids, stride: _mm().verify_batch_host(b, FIRST),
                              lambda n, stride: [(np.int32, (n,)), int]),
    "mac.package_batch_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                               _mm().package_batch_host(ids, lacs, lenf, b, stride), _MAC_FRAMED),
    "dg.verify_requests_mac_host": ("mac", _requests_mac_host,
                                    lambda n, stride: [(np.int32, (n,)), (np.uint64, (2 if n else 0,))]),
    "dg.package_batch_ledgers_mac_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                          dg.package_batch_ledgers_mac_host(_table(), KEY_OF[:len(b)], lids, ids, lacs,
                                                                            lenf, b, stride), _MAC_FRAMED),
    "dg.package_batch_segments_mac_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                           dg.package_batch_segments_mac_host(_table(), KEY_OF[:len(b)], lids, ids, lacs,
                                                                              lenf, b, stride), _MAC_FRAMED),
    "dg.package_batch_v2_mac_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride:
                                     dg.package_batch_v2_mac_host(_table(), KEY_OF[:len(b)], lids, ids, lacs, lenf, b, KEY),
                                     lambda n, stride: [("requests", 80), (np.uint8, (n, 20))]),
    "ck.mac_batch_host": ("payloads", lambda b, ids, lacs, lenf, lids, stride: ck.mac_batch_host(_mm().key_state, b),
                          lambda n, stride: [(np.uint8, (n, 20))]),
    "ck.crc_batch_host": ("payloads", _crc_batch_host, lambda n, stride: [(np.uint32, (n,))]),
    "ck.crc_batch_segments_host": ("payloads", _crc_segments_host, lambda n, stride: [(np.uint32, (n,))]),
}


def _call(name, n=N, stride=None, **short):
    """The form on the first n entries; short={"ids": 4} passes only four entry ids, "entries" four entries."""
    kind, fn, _ = PY[name]
    ids, lacs, lenf, lids = (a[:short.get(k, n)] for k, a in (("ids", IDS), ("lacs", LACS), ("lenf", LENF), ("lids", LIDS)))
    return fn(_entries(kind, short.get("entries", n)), ids, lacs, lenf, lids, stride)


def _check_results(name, out, n, stride=None):
    out = out if isinstance(out, tuple) else (out,)
    spec = PY[name][2](n, stride)
    assert len(out) == len(spec), name
    for got, want in zip(out, spec):
        if want is int:
            assert type(got) is int, (name, type(got))
        elif want[0] == "requests":  # ("requests", the bytes of a request's head: 60 + the digest)
            assert isinstance(got, list) and len(got) == n, name
            assert all(isinstance(r, np.ndarray) and r.dtype == np.uint8 and r.ndim == 1 for r in got), name
            assert [r.size for r in got] == [want[1] + l for l in LENS[:n]], name
        else:
            assert isinstance(got, np.ndarray) and got.dtype == want[0] and got.shape == want[1], \
                (name, got.dtype, got.shape, want)


# ---- (e) result dtypes and shapes, (d) empty batches ----

@pytest.mark.parametrize("name", list(PY))
def test_result_dtypes_and_shapes(name):
    out = _call(name)
    _check_results(name, out, N)
    if "verify" in name or "reframe" in name:  # the frames are good ones
        assert not out[0].any()
        assert out[1] == N if isinstance(out[1], int) else out[1].tolist() == [2, 3]


@pytest.mark.parametrize("name", list(PY))
def test_empty_batch(name):
    out = _call(name, n=0)
    _check_results(name, out, 0)
    if "verify_batch" in name or "reframe" in name:
        assert out[1] == 0  # first_bad


# ---- (a) size mismatches between the id arrays and the entries ----

FIELDS = ("ids", "lacs", "lenf")
MISMATCH = [(name, field, text)
            for name, fields, text in (
                ("dm.package_batch_host", FIELDS, NO_LEDGERS),
                ("mac.package_batch_host", FIELDS, NO_LEDGERS),
                ("dm.package_batch_segments_host", FIELDS, WITH_LEDGERS),
                ("dm.package_batch_v2_host", FIELDS, WITH_LEDGERS),
                ("dg.package_batch_ledgers_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.package_batch_segments_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.package_batch_v2_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.package_batch_ledgers_mac_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.package_batch_segments_mac_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.package_batch_v2_mac_host", FIELDS + ("lids",), WITH_LEDGERS),
                ("dg.verify_requests_mac_host", ("lids",), REQUESTS),
                ("dm.reframe_batch_host", ("lacs",), "new_lacs must have one element per frame"),
                ("dg.verify_requests_host", ("lids",), REQUESTS),
                ("ck.crc_batch_host", ("lenf",), "offsets/lengths size mismatch"))
            for field in fields + (("entries",) if fields[0] == "ids" or name == "dm.reframe_batch_host" else ())]


@pytest.mark.parametrize("name,field,text", MISMATCH, ids=[f"{n}-{f}" for n, f, _ in MISMATCH])
def test_size_mismatch_text(name, field, text):
    with pytest.raises(ValueError) as e:
        _call(name, **{field: N - 1})
    assert str(e.value) == text


@pytest.mark.parametrize("form", [_crc_batch_host, _crc_segments_host], ids=["crc_batch_host", "crc_batch_segments_host"])
def test_short_seeds_text(form):
    with pytest.raises(ValueError) as e:
        form(list(PAYLOADS), IDS, LACS, LENF, LIDS, None, seeds=np.zeros(N - 1, dtype=np.uint32))
    assert str(e.value) == f"seeds has {N - 1} elements, needs {N}"
    assert form(list(PAYLOADS), IDS, LACS, LENF, LIDS, None, seeds=np.zeros(N + 1, dtype=np.uint32)).shape == (N,)


# ---- (c) the frame_stride range ----

STRIDED = [("dm.package_batch_host", ck.CRC32C), ("dm.package_batch_host", ck.CRC32),
           ("dm.package_batch_segments_host", ck.CRC32C), ("dm.package_batch_segments_host", ck.CRC32),
           ("dg.package_batch_ledgers_host", ck.CRC32C), ("dg.package_batch_ledgers_host", ck.CRC32),
           ("dg.package_batch_segments_host", ck.CRC32C), ("dg.package_batch_segments_host", ck.CRC32),
           ("mac.package_batch_host", None), ("dg.package_batch_ledgers_mac_host", None),
           ("dg.package_batch_segments_mac_host", None)]


@pytest.mark.parametrize("name,algo", STRIDED, ids=[f"{n}-{a}" for n, a in STRIDED])
def test_frame_stride_range(name, algo):
    mac = 20 if algo is None else MAC[algo]
    if name.startswith("dm."):
        mgr = _dm(algo)
        call = lambda s: getattr(mgr, name[3:])(IDS, LACS, LENF, PAYLOADS, s)
    elif name.startswith("dg."):
        first = (_table(), KEY_OF) if algo is None else (CRC[algo],)
        call = lambda s: getattr(dg, name[3:])(*first, LIDS, IDS, LACS, LENF, PAYLOADS, s)
    else:
        call = lambda s: _mm().package_batch_host(IDS, LACS, LENF, PAYLOADS, s)
    for stride in (31 + mac, 4097):
        with pytest.raises(_native.BkdError) as e:
            call(stride)
        assert e.value.code == INVALID_ARG and str(e.value) == STRIDE, stride
    for stride in (32 + mac, 4096):
        frames, _ = call(stride)
        assert frames.shape == (N, stride) and not frames[:, 32 + mac:].any()


# ---- (b) a null entry with a length, through the C-ABI ----

def _raw_forms():
    """name -> (the noun of its error, call(ptrs uint64[N], lens uint32[N]) -> rc): every host form of the
    C-ABI that takes separate entry buffers, everything but the entry pointers valid."""
    L, vp = _native.lib(), ctypes.c_void_p
    p = lambda a: vp(a.ctypes.data)
    status, dig = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.uint32)
    fb, frames = ctypes.c_uint64(0), np.zeros((N, 64), dtype=np.uint8)
    macs, ks = np.zeros((N, 20), dtype=np.uint8), _mm().key_state
    seg_first = np.arange(N + 1, dtype=np.uint64)
    req_first, req_fb = np.array(REQ_FIRST, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    req_lid, req_eid = np.array(REQ_LEDGERS, dtype=np.int64), np.array(REQ_ENTRIES, dtype=np.int64)
    req_flags = np.zeros(2, dtype=np.uint32)
    requests = [np.zeros(60 + 20 + l, dtype=np.uint8) for l in LENS]  # (room for the longest digest, the MAC)
    rptr = np.array([r.ctypes.data for r in requests], dtype=np.uint64)
    table, req_keys = _table(), np.zeros(2, dtype=np.uint32)
    keep = (status, dig, frames, macs, ks, seg_first, req_first, req_fb, req_lid, req_eid, req_flags, requests, rptr,
            table, req_keys)
    key = np.frombuffer(KEY, dtype=np.uint8)
    ids, lacs, lenf, lids = p(IDS), p(LACS), p(LENF), p(LIDS)
    return keep, rptr, {
        "bkd_digest_verify_batch_host": ("frame", lambda q, l: L.bkd_digest_verify_batch_host(
            ck.CRC32C, LEDGER, FIRST, 0, p(q), p(l), N, p(status), ctypes.byref(fb))),
        "bkd_digest_package_batch_host": ("payload", lambda q, l: L.bkd_digest_package_batch_host(
            ck.CRC32C, LEDGER, ids, lacs, lenf, p(q), p(l), N, p(frames), 64, p(dig))),
        "bkd_digest_package_batch_ledgers_host": ("payload", lambda q, l: L.bkd_digest_package_batch_ledgers_host(
            ck.CRC32C, lids, ids, lacs, lenf, p(q), p(l), N, p(frames), 64, p(dig))),
        "bkd_digest_reframe_batch_host": ("frame", lambda q, l: L.bkd_digest_reframe_batch_host(
            ck.CRC32C, LEDGER, FIRST, 0, 0, p(q), p(l), N, lacs, p(dig), p(status), ctypes.byref(fb))),
        "bkd_digest_verify_requests_host": ("frame", lambda q, l: L.bkd_digest_verify_requests_host(
            ck.CRC32C, p(q), p(l), N, p(req_first), 2, p(req_lid), p(req_eid), p(req_flags), p(status), p(req_fb))),
        "bkd_digest_package_batch_v2_host": ("payload", lambda q, l: L.bkd_digest_package_batch_v2_host(
            ck.CRC32C, LEDGER, vp(0), ids, lacs, lenf, p(q), p(l), N, p(key), 0, 0, 16384, p(rptr), p(dig))),
        "bkd_digest_package_batch_segments_host": ("segment", lambda q, l: L.bkd_digest_package_batch_segments_host(
            ck.CRC32C, LEDGER, vp(0), ids, lacs, lenf, p(q), p(l), N, p(seg_first), N, p(frames), 64, p(dig))),
        "bkd_crc_batch_segments_host": ("segment", lambda q, l: L.bkd_crc_batch_segments_host(
            ck.CRC32C, p(q), p(l), N, p(seg_first), N, vp(0), 0, p(dig))),
        "bkd_mac_batch_host": ("entry", lambda q, l: L.bkd_mac_batch_host(p(ks), p(q), p(l), N, p(macs))),
        "bkd_digest_package_batch_mac_host": ("entry", lambda q, l: L.bkd_digest_package_batch_mac_host(
            p(ks), LEDGER, ids, lacs, lenf, p(q), p(l), N, p(frames), 64)),
        "bkd_digest_verify_batch_mac_host": ("entry", lambda q, l: L.bkd_digest_verify_batch_mac_host(
            p(ks), LEDGER, FIRST, 0, p(q), p(l), N, p(status), ctypes.byref(fb))),
        "bkd_digest_verify_requests_mac_host": ("frame", lambda q, l: L.bkd_digest_verify_requests_mac_host(
            p(table), 2, p(req_keys), p(q), p(l), N, p(req_first), 2, p(req_lid), p(req_eid), p(req_flags), p(status),
            p(req_fb))),
        "bkd_digest_package_batch_ledgers_mac_host": ("entry", lambda q, l: L.bkd_digest_package_batch_ledgers_mac_host(
            p(table), 2, p(KEY_OF), lids, ids, lacs, lenf, p(q), p(l), N, p(frames), 64)),
        "bkd_digest_package_batch_segments_mac_host": ("segment", lambda q, l: L.bkd_digest_package_batch_segments_mac_host(
            p(table), 2, p(KEY_OF), LEDGER, vp(0), ids, lacs, lenf, p(q), p(l), N, p(seg_first), N, p(frames), 64)),
        "bkd_digest_package_batch_v2_mac_host": ("payload", lambda q, l: L.bkd_digest_package_batch_v2_mac_host(
            p(table), 2, p(KEY_OF), LEDGER, vp(0), ids, lacs, lenf, p(q), p(l), N, p(key), 0, 0, 16384, p(rptr))),
    }


RAW_NAMES = ["bkd_digest_verify_batch_host", "bkd_digest_package_batch_host", "bkd_digest_package_batch_ledgers_host",
             "bkd_digest_reframe_batch_host", "bkd_digest_verify_requests_host", "bkd_digest_package_batch_v2_host",
             "bkd_digest_package_batch_segments_host", "bkd_crc_batch_segments_host", "bkd_mac_batch_host",
             "bkd_digest_package_batch_mac_host", "bkd_digest_verify_batch_mac_host",
             "bkd_digest_verify_requests_mac_host", "bkd_digest_package_batch_ledgers_mac_host",
             "bkd_digest_package_batch_segments_mac_host", "bkd_digest_package_batch_v2_mac_host"]


@pytest.mark.parametrize("name", RAW_NAMES)
def test_null_entry(name):
    keep, rptr, forms = _raw_forms()
    assert sorted(forms) == sorted(RAW_NAMES)
    noun, call = forms[name]
    bufs = [np.array(np.frombuffer(b, dtype=np.uint8)) for b in PAYLOADS]  # (writable: reframe's frames)
    ptrs = np.array([b.ctypes.data if b.size else 0 for b in bufs], dtype=np.uint64)
    lens = np.array(LENS, dtype=np.uint32)
    assert ptrs[0] == 0 and call(ptrs, lens) == 0, _native.last_error()  # null with length 0 is an empty entry
    ptrs[3] = 0
    assert call(ptrs, lens) == INVALID_ARG
    assert _native.last_error() == f"null {noun} 3"
    ptrs[1] = 0  # the first null entry is the one named
    assert call(ptrs, lens) == INVALID_ARG
    assert _native.last_error() == f"null {noun} 1"
    if name in ("bkd_digest_package_batch_v2_host", "bkd_digest_package_batch_v2_mac_host"):
        ptrs[1], rptr[1] = bufs[1].ctypes.data, 0
        assert call(ptrs, lens) == INVALID_ARG
        assert _native.last_error() == "null request 1"  # entry 1's request before entry 3's payload
        ptrs[3] = bufs[3].ctypes.data
        assert call(ptrs, lens) == INVALID_ARG
        assert _native.last_error() == "null request 1"
    del keep


# ---- (f) two faults at once: which one is reported, and the exact texts of the CSR and key-index errors ----

def _folded_forms():
    """name -> the C arguments of a folded host form in order, by name and all valid: an array is passed as its
    pointer, anything else as it is. _raw() overrides some of them; None is a null pointer."""
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in PAYLOADS]
    entries = dict(ptrs=np.array([b.ctypes.data for b in bufs], dtype=np.uint64), lengths=np.array(LENS, dtype=np.uint32))
    keyed = lambda index: dict(table=_table(), nkeys=2, **index)
    fields = lambda **first: dict(**first, lids=LIDS, ids=IDS, lacs=LACS, lenf=LENF)
    requests = lambda: dict(**entries, n=N, req_first=np.array(REQ_FIRST, dtype=np.uint64), nreq=2,
                            req_lids=np.array(REQ_LEDGERS, dtype=np.int64), req_eids=np.array(REQ_ENTRIES, dtype=np.int64),
                            req_flags=np.zeros(2, dtype=np.uint32), status=np.zeros(N, dtype=np.int32),
                            req_first_bad=np.zeros(2, dtype=np.uint64))
    segments = lambda: dict(**entries, nseg=N, seg_first=np.arange(N + 1, dtype=np.uint64), n=N,
                            frames=np.zeros((N, 64), dtype=np.uint8), stride=64)
    outs = [np.zeros(80 + l, dtype=np.uint8) for l in LENS]
    v2 = lambda: dict(**entries, n=N, master=np.frombuffer(KEY, dtype=np.uint8), key_stride=0, flags=0, small=16384,
                      requests=np.array([r.ctypes.data for r in outs], dtype=np.uint64))
    digests = lambda: dict(digests=np.zeros(N, dtype=np.uint32))
    return (bufs, outs), {
        "bkd_digest_verify_requests_host": dict(algo=ck.CRC32C, **requests()),
        "bkd_digest_verify_requests_mac_host": dict(**keyed(dict(req_keys=np.array([0, 1], dtype=np.uint32))), **requests()),
        "bkd_digest_package_batch_ledgers_mac_host": dict(**keyed(dict(key_of=KEY_OF)), **fields(), **entries, n=N,
                                                          frames=np.zeros((N, 64), dtype=np.uint8), stride=64),
        "bkd_digest_package_batch_segments_host": dict(algo=ck.CRC32C, **fields(ledger_id=LEDGER), **segments(), **digests()),
        "bkd_digest_package_batch_segments_mac_host": dict(**keyed(dict(key_of=KEY_OF)), **fields(ledger_id=LEDGER),
                                                           **segments()),
        "bkd_digest_package_batch_v2_host": dict(algo=ck.CRC32C, **fields(ledger_id=LEDGER), **v2(), **digests()),
        "bkd_digest_package_batch_v2_mac_host": dict(**keyed(dict(key_of=KEY_OF)), **fields(ledger_id=LEDGER), **v2()),
    }


def _raw(name, **faults):
    """(rc, bkd_last_error) of the form with `faults` in place of its valid arguments."""
    keep, forms = _folded_forms()
    args = forms[name]
    assert set(faults) <= set(args), (name, sorted(args))
    if faults.get("ptrs") is NULL_3:
        faults = dict(faults, ptrs=[0 if i == 3 else int(q) for i, q in enumerate(args["ptrs"])])
    args.update({k: np.array(v, dtype=args[k].dtype) if isinstance(v, list) else v for k, v in faults.items()})
    rc = getattr(_native.lib(), name)(*(ctypes.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a
                                        for a in args.values()))
    del keep
    return rc, _native.last_error()


NULL_3 = "entry 3 of 5, 33 bytes, is a null pointer"
RQ, RQM = "bkd_digest_verify_requests_host", "bkd_digest_verify_requests_mac_host"
LM, SC, SM = ("bkd_digest_package_batch_ledgers_mac_host", "bkd_digest_package_batch_segments_host",
              "bkd_digest_package_batch_segments_mac_host")
V2, V2M = "bkd_digest_package_batch_v2_host", "bkd_digest_package_batch_v2_mac_host"
KEY_STRIDE, FLAGS = "key_stride must be 0 or at least 20", "flags must fit 16 bits"
BAD_STRIDE = "frame_stride must be in [32 + digest length, 4096]"

# (form, the faulty arguments, the one error reported); the checks run in the order the forms document:
# scalars, null arrays, the key table, the key indices, the CSR, the entry buffers, each entry
FAULTS = [
    # the exact texts, one fault each
    (RQ, dict(req_first=[1, 2, N]), "req_first[0] is not 0"),
    (RQ, dict(req_first=[0, N, N - 1]), "req_first decreases at request 1"),
    (RQ, dict(req_first=[0, 2, N - 1]), "req_first[nreq] is not n"),
    (RQ, dict(req_first=[0, 2, N + 1]), "req_first[nreq] is not n"),
    (RQM, dict(req_first=[1, 2, N]), "req_first[0] is not 0"),
    (RQM, dict(req_first=[0, N, N - 1]), "req_first decreases at request 1"),
    (RQM, dict(req_first=[0, 2, N + 1]), "req_first[nreq] is not n"),
    (RQM, dict(req_keys=[0, 2]), "request 1 names a key outside the table"),
    (RQM, dict(req_keys=[0xFFFFFFFF, 2]), "request 0 names a key outside the table"),
    (LM, dict(key_of=[0, 1, 1, 2, 7]), "entry 3 names a key outside the table"),
    (SM, dict(key_of=[0, 1, 2, 0, 1]), "entry 2 names a key outside the table"),
    (V2M, dict(key_of=[2, 1, 1, 0, 1]), "entry 0 names a key outside the table"),
    (SM, dict(key_of=None, nkeys=0, table=None), "an empty key table"),
    (V2M, dict(key_of=None, nkeys=0, table=None), "an empty key table"),
    (SC, dict(seg_first=[1, 1, 2, 3, 4, N]), "seg_first[0] is not 0"),
    (SC, dict(seg_first=[0, 1, 3, 2, 4, N]), "seg_first decreases at entry 2"),
    (SC, dict(seg_first=[0, 1, 2, 3, 4, N - 1]), "seg_first[n] is not nseg"),
    (SM, dict(seg_first=[1, 1, 2, 3, 4, N]), "seg_first[0] is not 0"),
    (SM, dict(seg_first=[0, 1, 3, 2, 4, N]), "seg_first decreases at entry 2"),
    (SM, dict(seg_first=[0, 1, 2, 3, 4, N + 1]), "seg_first[n] is not nseg"),
    (V2, dict(key_stride=19), KEY_STRIDE), (V2, dict(flags=1 << 16), FLAGS),
    (V2M, dict(key_stride=1), KEY_STRIDE), (V2M, dict(flags=1 << 16), FLAGS),
    # verify requests, CRC: algorithm, request count, request arrays, CSR, buffers, frames
    (RQ, dict(algo=99, nreq=1 << 31), "unknown algorithm"),
    (RQ, dict(nreq=1 << 31, req_flags=None), "a call holds fewer than 2^31 requests"),
    (RQ, dict(nreq=0, req_first=None), "entries without a request"),
    (RQ, dict(req_flags=None, req_first=[1, 2, N]), "null request array"),
    (RQ, dict(req_first_bad=None, status=None), "null request array"),
    (RQ, dict(req_first=[1, 0, N], status=None), "req_first[0] is not 0"),
    (RQ, dict(req_first=[0, N, 0]), "req_first decreases at request 1"),
    (RQ, dict(req_first=[0, 2, N - 1], lengths=None), "req_first[nreq] is not n"),
    (RQ, dict(status=None, ptrs=NULL_3), "null buffer"),
    # verify requests, MAC: the key table and the key indices between the request arrays and the CSR
    (RQM, dict(nreq=1 << 31, req_keys=None), "a call holds fewer than 2^31 requests"),
    (RQM, dict(nreq=0, req_keys=[5, 5]), "entries without a request"),
    (RQM, dict(req_keys=None, table=None), "null request array"),
    (RQM, dict(req_flags=None, req_keys=[0, 2]), "null request array"),
    (RQM, dict(table=None, req_keys=[0, 2]), "null key table"),
    (RQM, dict(req_keys=[0, 2], req_first=[1, 2, N]), "request 1 names a key outside the table"),
    (RQM, dict(nkeys=1, req_first=[0, N, 0]), "request 1 names a key outside the table"),
    (RQM, dict(req_first=[0, N, 0], status=None), "req_first decreases at request 1"),
    (RQM, dict(status=None, ptrs=NULL_3), "null buffer"),
    # many-ledger MAC package: buffers, key table, stride, key indices, entries
    (LM, dict(lids=None, table=None), "null buffer"),
    (LM, dict(key_of=None, stride=51), "null buffer"),
    (LM, dict(table=None, stride=51), "null key table"),
    (LM, dict(stride=4097, key_of=[2, 0, 0, 0, 0]), BAD_STRIDE),
    (LM, dict(key_of=[0, 0, 0, 0, 2], ptrs=NULL_3), "entry 4 names a key outside the table"),
    # composite payloads: buffers, key table, stride, key indices, the CSR, segments
    (SC, dict(algo=99, frames=None), "unknown algorithm"),
    (SC, dict(frames=None, stride=35), "null buffer"),
    (SC, dict(stride=35, seg_first=[1, 1, 2, 3, 4, N]), BAD_STRIDE),
    (SC, dict(seg_first=None, stride=64), "null buffer"),
    (SC, dict(seg_first=[0, 1, 2, 3, 4, N - 1], ptrs=NULL_3), "seg_first[n] is not nseg"),
    (SC, dict(seg_first=[1, 0, 2, 3, 4, N - 1]), "seg_first[0] is not 0"),
    (SC, dict(seg_first=[0, 2, 1, 3, 4, N - 1]), "seg_first decreases at entry 1"),
    (SM, dict(ids=None, table=None), "null buffer"),
    (SM, dict(table=None, stride=51), "null key table"),
    (SM, dict(stride=51, key_of=[2, 0, 0, 0, 0]), BAD_STRIDE),
    (SM, dict(key_of=[0, 0, 0, 2, 0], seg_first=[1, 1, 2, 3, 4, N]), "entry 3 names a key outside the table"),
    (SM, dict(key_of=[0, 0, 0, 2, 0], seg_first=None), "entry 3 names a key outside the table"),
    (SM, dict(seg_first=[0, 1, 3, 2, 4, N], ptrs=NULL_3), "seg_first decreases at entry 2"),
    (SM, dict(seg_first=[0, 1, 2, 3, 4, N + 1], lengths=None), "null buffer"),
    # V2 add requests: algorithm, key_stride, flags, buffers, key table, payloads and requests, key indices
    (V2, dict(algo=99, key_stride=19), "unknown algorithm"),
    (V2, dict(key_stride=19, flags=1 << 16), KEY_STRIDE),
    (V2, dict(key_stride=19, master=None), KEY_STRIDE),
    (V2, dict(key_stride=19, n=0), KEY_STRIDE),
    (V2, dict(flags=1 << 16, requests=None), FLAGS),
    (V2, dict(flags=1 << 16, n=0), FLAGS),
    (V2, dict(digests=None, ptrs=NULL_3), "null buffer"),
    (V2M, dict(key_stride=19, flags=1 << 16), KEY_STRIDE),
    (V2M, dict(key_stride=19, requests=None), KEY_STRIDE),
    (V2M, dict(key_stride=19, n=0), KEY_STRIDE),
    (V2M, dict(flags=1 << 16, table=None), FLAGS),
    (V2M, dict(master=None, table=None), "null buffer"),
    (V2M, dict(table=None, ptrs=NULL_3), "null key table"),
    (V2M, dict(ptrs=NULL_3, key_of=[2, 0, 0, 0, 0]), "null payload 3"),
    (V2M, dict(requests=[1, 1, 0, 1, 1], key_of=[2, 0, 0, 0, 0]), "null request 2"),
]


@pytest.mark.parametrize("name,faults,text", FAULTS, ids=[f"{n[11:]}-{'+'.join(f)}-{i}" for i, (n, f, _) in enumerate(FAULTS)])
def test_first_fault_wins(name, faults, text):
    assert _raw(name)[0] == 0, _native.last_error()
    rc, err = _raw(name, **faults)
    assert rc == INVALID_ARG and err == text


def test_v2_device_forms_check_key_stride_and_flags_first():
    """bkd_digest_package_batch_v2 and its MAC form refuse a bad key_stride or flags before they look at n, at a
    pointer or for a device."""
    L = _native.lib()
    for key_stride, flags, text in ((19, 1 << 16, KEY_STRIDE), (20, 1 << 16, FLAGS), (1, 0, KEY_STRIDE)):
        for n in (0, N):
            assert L.bkd_digest_package_batch_v2(ck.CRC32C, LEDGER, *[None] * 5, 0, None, None, n, None, key_stride, flags,
                                                 16384, None, 0, None, None, None) == INVALID_ARG
            assert _native.last_error() == text
            assert L.bkd_digest_package_batch_v2_mac(None, 2, None, LEDGER, *[None] * 5, 0, None, None, n, None, key_stride,
                                                     flags, 16384, None, 0, None, None) == INVALID_ARG
            assert _native.last_error() == text
    assert L.bkd_digest_package_batch_v2(99, LEDGER, *[None] * 5, 0, None, None, 0, None, 19, 0, 16384, None, 0, None,
                                         None, None) == INVALID_ARG
    assert _native.last_error() == "unknown algorithm"


# ---- (g) the key index of the Python MAC forms: its size text, and which size mismatch is reported ----

def test_key_index_size_texts():
    t, short = _table(), KEY_OF[:N - 1]
    for form in (dg.package_batch_ledgers_mac_host, dg.package_batch_segments_mac_host):
        with pytest.raises(ValueError) as e:
            form(t, short, LIDS, IDS, LACS, LENF, PAYLOADS)
        assert str(e.value) == f"key_of has {N - 1} elements, needs {N}"
    with pytest.raises(ValueError) as e:
        dg.package_batch_v2_mac_host(t, short, LIDS, IDS, LACS, LENF, PAYLOADS, KEY)
    assert str(e.value) == f"key_of has {N - 1} elements, needs {N}"
    with pytest.raises(ValueError) as e:
        dg.verify_requests_mac_host(t, [0], _frames("mac"), REQ_FIRST, REQ_LEDGERS, REQ_ENTRIES)
    assert str(e.value) == "req_keys has 1 elements, needs 2"
    with pytest.raises(ValueError) as e:
        dg.package_batch_segments_mac_host(t.reshape(-1)[:-1], None, LIDS, IDS, LACS, LENF, PAYLOADS)
    assert str(e.value) == "key_states holds ten words per key (mac_key_table)"
    # with the entry fields short as well: the many-ledger form reports the key index, the other three the fields
    with pytest.raises(ValueError) as e:
        dg.package_batch_ledgers_mac_host(t, short, LIDS, IDS[:N - 1], LACS, LENF, PAYLOADS)
    assert str(e.value) == f"key_of has {N - 1} elements, needs {N}"
    for form, tail in ((dg.package_batch_segments_mac_host, ()), (dg.package_batch_v2_mac_host, (KEY,))):
        with pytest.raises(ValueError) as e:
            form(t, short, LIDS, IDS[:N - 1], LACS, LENF, PAYLOADS, *tail)
        assert str(e.value) == WITH_LEDGERS
    with pytest.raises(ValueError) as e:
        dg.verify_requests_mac_host(t, [0], _frames("mac"), REQ_FIRST, REQ_LEDGERS[:1], REQ_ENTRIES)
    assert str(e.value) == REQUESTS
