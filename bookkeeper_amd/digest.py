"""Host-side mirror of BookKeeper's DigestManager family over the GPU engine.

Reference: bookkeeper-server/src/main/java/org/apache/bookkeeper/proto/checksum/
  DigestManager.java:46-401      framing, instantiate, package V2/V3, verify, LAC
  CRC32CDigestManager.java:27-62 4-byte big-endian int digest via Crc32cIntChecksum
  CRC32DigestManager.java:28-87  8-byte big-endian long digest (zero-extended CRC32)
  DummyDigestManager.java:30-62  no digest
  MacDigestManager.java:46-107   20-byte HMAC-SHA1 keyed with SHA1("mac" || passwd)

Per-entry methods keep the reference's two ``update`` calls (header, then payload). The batch
methods (``package_batch`` / ``verify_batch``) are the new device path: one launch sequence
frames or verifies thousands of device-resident entries.
"""
from __future__ import annotations

import contextlib
import ctypes
import enum
import struct

import numpy as np

from . import checksum as _ck
from .bytebuf import CompositeBuffer
from ._native import (CRC32, CRC32C, MAC_LENGTH, VERIFY_DIGEST_MISMATCH, VERIFY_ENTRY_MISMATCH, VERIFY_LEDGER_MISMATCH,
                      VERIFY_OK, VERIFY_TOO_SHORT, REFRAME_TRUSTED, check, lib)

METADATA_LENGTH = 32          # DigestManager.java:48
LAC_METADATA_LENGTH = 16      # DigestManager.java:49
MASTER_KEY_LENGTH = 20        # BookieProtocol.java:65
CURRENT_PROTOCOL_VERSION = 2  # BookieProtocol.java:47
ADDENTRY = 1                  # BookieProtocol.java:114
FLAG_NONE = 0                 # BookieProtocol.java:188
SMALL_ENTRY_SIZE_THRESHOLD = 16 * 1024  # BookieProtoEncoding.java:48
INVALID_ENTRY_ID = -1         # LedgerHandle.INVALID_ENTRY_ID


class DigestType(enum.Enum):  # DataFormats.proto:45-51
    HMAC = 0
    CRC32 = 1
    CRC32C = 2
    DUMMY = 3


class BKDigestMatchException(Exception):
    """BKException.BKDigestMatchException (DigestManager.java:234, 248, 260, 272, 280)."""

    def __init__(self, reason: int = VERIFY_DIGEST_MISMATCH):
        super().__init__({VERIFY_TOO_SHORT: "too short", VERIFY_DIGEST_MISMATCH: "digest mismatch",
                          VERIFY_LEDGER_MISMATCH: "ledger id mismatch",
                          VERIFY_ENTRY_MISMATCH: "entry id mismatch"}.get(reason, str(reason)))
        self.reason = reason


def packet_header_to_int(version: int, opcode: int, flags: int) -> int:
    """BookieProtocol.PacketHeader.toInt (BookieProtocol.java:75-83)."""
    if version == 0:
        return opcode
    return ((version & 0xFF) << 24) | ((opcode & 0xFF) << 16) | (flags & 0xFFFF)


def _header(ledger_id: int, entry_id: int, lac: int, length: int) -> bytes:
    # buf.writeLong x4, big-endian (DigestManager.java:146-149 / :172-175)
    return struct.pack(">qqqq", ledger_id, entry_id, lac, length)


def _entry_fields(n, entry_ids, lacs, length_fields, ledger_ids=None, optional_ledgers: bool = False):
    """The per-entry header fields of a host batch of n entries as contiguous int64 arrays: (entry ids,
    LACs, length fields, ledger ids or None). The ValueError for a size mismatch names ledger_ids when
    they are given, or when the form takes them optionally (`optional_ledgers`: the composite and V2 forms)."""
    ids = np.ascontiguousarray(entry_ids, dtype=np.int64)
    lac = np.ascontiguousarray(lacs, dtype=np.int64)
    lf = np.ascontiguousarray(length_fields, dtype=np.int64)
    lids = None if ledger_ids is None else np.ascontiguousarray(ledger_ids, dtype=np.int64)
    if not (ids.size == lac.size == lf.size == n) or (lids is not None and lids.size != n):
        raise ValueError(("ledger_ids, " if lids is not None or optional_ledgers else "") +
                         "entry_ids, lacs, length_fields and payloads must have one element per entry")
    return ids, lac, lf, lids


def _package_frames(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride,
                    out_frames, stream, sync_check, with_digests: bool = True):
    """The device forms that frame one payload range per entry: the library's `fn`(*first, *ledger ids,
    entry ids, ..., frames, stride, [digests,] stream); `ledger_ids` is () for a form of one ledger, the
    (tensor,) for the many-ledger form. Returns (frames, digests int32[n] or None)."""
    import torch
    n = offsets.numel()
    stride = frame_stride or (METADATA_LENGTH + mac)
    dev = payload.device
    if out_frames is None:
        out_frames = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    elif out_frames.dim() != 2 or out_frames.shape[0] < n or out_frames.shape[1] != stride:
        raise ValueError("out_frames must be a [n, frame_stride] tensor")
    digests = torch.empty(n, dtype=torch.int32, device=dev) if with_digests else None
    i64, u32 = torch.int64, _ck._u32_dtypes()
    with _ck._on_device(payload):
        st = _ck._stream_ptr(stream, payload)
        check(getattr(lib(), fn)(
            *first, *(_ck._dev_ptr(t, "ledger_ids", i64, dev, n) for t in ledger_ids),
            _ck._dev_ptr(entry_ids, "entry_ids", i64, dev, n), _ck._dev_ptr(lacs, "lacs", i64, dev, n),
            _ck._dev_ptr(length_fields, "length_fields", i64, dev, n), _ck._dev_ptr(payload, "payload"),
            payload.numel() * payload.element_size(), _ck._dev_ptr(offsets, "offsets", i64, dev),
            _ck._dev_ptr(lengths, "lengths", u32, dev, n), n, _ck._dev_ptr(out_frames, "frames", torch.uint8, dev), stride,
            *((_ck._dev_ptr(digests, "digests"),) if with_digests else ()), st))
        if sync_check:
            check(lib().bkd_stream_sync(st))
    return out_frames, digests


def _package_frames_host(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payloads, frame_stride,
                         with_digests: bool = True):
    """The host forms that frame one buffer per entry: the library's `fn`(*first, [ledger ids,] entry ids,
    ..., frames, stride[, digests]). Returns (frames uint8[n, frame_stride], digests uint32[n] or None)."""
    views, ptrs, lens = _ck._host_entries(payloads)
    n = len(views)
    stride = frame_stride or (METADATA_LENGTH + mac)
    ids, lac, lf, lids = _entry_fields(n, entry_ids, lacs, length_fields, ledger_ids)
    frames = np.zeros((n, stride), dtype=np.uint8)
    digests = np.zeros(n, dtype=np.uint32) if with_digests else None
    vp = ctypes.c_void_p
    check(getattr(lib(), fn)(
        *first, *(() if lids is None else (vp(lids.ctypes.data),)), vp(ids.ctypes.data), vp(lac.ctypes.data),
        vp(lf.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(frames.ctypes.data), stride,
        *((vp(digests.ctypes.data),) if with_digests else ())))
    del views
    return frames, digests


class DigestManager:
    algo: int | None = None
    macCodeLength: int = 0

    def __init__(self, ledgerId: int, useV2Protocol: bool = False):
        self.ledgerId = int(ledgerId)
        self.useV2Protocol = bool(useV2Protocol)
        self._hash = _ck.GpuIntHash(self.algo) if self.algo is not None else None

    # DigestManager.instantiate (DigestManager.java:88-102)
    @staticmethod
    def instantiate(ledgerId: int, passwd: bytes, digestType: DigestType, useV2Protocol: bool = False):
        if digestType == DigestType.CRC32:
            return CRC32DigestManager(ledgerId, useV2Protocol)
        if digestType == DigestType.CRC32C:
            return CRC32CDigestManager(ledgerId, useV2Protocol)
        if digestType == DigestType.DUMMY:
            return DummyDigestManager(ledgerId, useV2Protocol)
        if digestType == DigestType.HMAC:
            return MacDigestManager(ledgerId, passwd, useV2Protocol)
        raise ValueError(f"Unknown checksum type: {digestType}")

    # ---- the two hooks subclasses define (DigestManager.java:56-76) ----
    def update(self, digest: int, buf, offset: int, length: int) -> int:
        """DigestManager.update (:62-72): a composite buffer is visited leaf by leaf and the digest
        chained over the leaves (ByteBufVisitor, :380-392); anything else is one resume."""
        if isinstance(buf, CompositeBuffer):
            for leaf, off, n in buf.visit(offset, length):
                digest = self.internalUpdate(digest, leaf, off, n)
            return digest
        return self.internalUpdate(digest, buf, offset, length)

    def internalUpdate(self, digest: int, buf, offset: int, length: int) -> int:
        return self._hash.resume(digest, buf, offset, length)

    def digest_bytes(self, digest: int) -> bytes:
        raise NotImplementedError

    def isInt32Digest(self) -> bool:
        raise NotImplementedError

    # ---- packaging (DigestManager.java:117-181) ----
    def computeDigestAndPackageForSending(self, entryId: int, lastAddConfirmed: int, length: int, data: bytes,
                                          masterKey: bytes = b"\0" * MASTER_KEY_LENGTH,
                                          flags: int = FLAG_NONE) -> bytes:
        hdr = _header(self.ledgerId, entryId, lastAddConfirmed, length)
        digest = self.update(0, hdr, 0, METADATA_LENGTH)
        if isinstance(data, CompositeBuffer):  # the readable bytes, digested leaf by leaf (:152-153)
            digest = self.update(digest, data, data.reader_index, data.readable_bytes())
            data = data.readable()
        else:
            data = bytes(data)
            digest = self.update(digest, data, 0, len(data))
        dbytes = self.digest_bytes(digest)
        if not self.useV2Protocol:  # V3: ByteBufList(header+digest, data)  (:169-181)
            return hdr + dbytes + data
        headers_size = 4 + MASTER_KEY_LENGTH + METADATA_LENGTH + self.macCodeLength  # :130-133
        prefix = struct.pack(">ii", headers_size + len(data),
                             packet_header_to_int(CURRENT_PROTOCOL_VERSION, ADDENTRY, flags))
        return prefix + bytes(masterKey[:MASTER_KEY_LENGTH]) + hdr + dbytes + data  # :138-166

    def computeDigestAndPackageForSendingLac(self, lac: int) -> bytes:  # :190-204
        hdr = struct.pack(">qq", self.ledgerId, lac)
        return hdr + self.digest_bytes(self.update(0, hdr, 0, LAC_METADATA_LENGTH))

    # ---- verification (DigestManager.java:206-370) ----
    def _verify(self, entryId: int, data: bytes, skipEntryIdCheck: bool) -> None:
        data = bytes(data)
        if METADATA_LENGTH + self.macCodeLength > len(data):
            raise BKDigestMatchException(VERIFY_TOO_SHORT)
        digest = self.update(0, data, 0, METADATA_LENGTH)
        off = METADATA_LENGTH + self.macCodeLength
        digest = self.update(digest, data, off, len(data) - off)
        if self.digest_bytes(digest) != data[METADATA_LENGTH:METADATA_LENGTH + self.macCodeLength]:
            raise BKDigestMatchException(VERIFY_DIGEST_MISMATCH)
        actual_ledger, actual_entry = struct.unpack(">qq", data[:16])
        if actual_ledger != self.ledgerId:
            raise BKDigestMatchException(VERIFY_LEDGER_MISMATCH)
        if not skipEntryIdCheck and actual_entry != entryId:
            raise BKDigestMatchException(VERIFY_ENTRY_MISMATCH)

    def verifyDigestAndReturnData(self, entryId: int, dataReceived: bytes) -> bytes:  # :333-338
        self._verify(entryId, dataReceived, False)
        return bytes(dataReceived)[METADATA_LENGTH + self.macCodeLength:]

    def verifyDigestAndReturnLac(self, dataReceived: bytes) -> int:  # :285-323
        data = bytes(dataReceived)
        if LAC_METADATA_LENGTH + self.macCodeLength > len(data):
            raise BKDigestMatchException(VERIFY_TOO_SHORT)
        digest = self.update(0, data, 0, LAC_METADATA_LENGTH)
        if self.digest_bytes(digest) != data[LAC_METADATA_LENGTH:LAC_METADATA_LENGTH + self.macCodeLength]:
            raise BKDigestMatchException(VERIFY_DIGEST_MISMATCH)
        ledger, lac = struct.unpack(">qq", data[:16])
        if ledger != self.ledgerId:
            raise BKDigestMatchException(VERIFY_LEDGER_MISMATCH)
        return lac

    # ---- what a digest type's batch methods pass to the library ----
    _c_suffix = ""  # bkd_digest_verify_batch<suffix>[_host], bkd_digest_package_batch<suffix>[_host]

    def _c_first(self):
        """(the first C argument of those functions, what must stay alive while it is used)."""
        return self.algo, None

    def _c_add_first(self):
        """(algo, ledger id): what the composite and V2 package functions take in front."""
        if self.algo is None:
            raise NotImplementedError("DUMMY digests need no device work")
        return self.algo, self.ledgerId

    # ---- batch device path (new) ----
    def package_batch(self, entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride=None,
                      stream=None, sync_check: bool = False):
        """Frames n device-resident entries: returns (frames[n, frame_stride] uint8, digests int32[n]).
        frames[i] = [32 B header][digest]; payload bytes stay where they are (ByteBufList(header, data)).
        An entry outside `payload` gets digest 0 and raises BKD_ERR_BOUNDS from the stream's next
        bkd_stream_sync (here, when ``sync_check``)."""
        return _package_frames("bkd_digest_package_batch", (self.algo, self.ledgerId), self.macCodeLength, (),
                               entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride, None, stream,
                               sync_check)

    def verify_batch(self, framed, offsets, lengths, first_entry_id: int, skip_entry_check: bool = False,
                     stream=None):
        """Verifies n framed entries on the device; returns (status int32[n], first_bad int64[1])
        with BatchedReadOp's verified-prefix rule: entries [0, first_bad) verified."""
        import torch
        n = offsets.numel()
        dev = framed.device
        status = torch.empty(n, dtype=torch.int32, device=dev)
        first_bad = torch.empty(1, dtype=torch.int64, device=dev)
        first, _keep = self._c_first()
        with _ck._on_device(framed):
            check(getattr(lib(), "bkd_digest_verify_batch" + self._c_suffix)(
                first, self.ledgerId, first_entry_id, int(skip_entry_check), _ck._dev_ptr(framed, "framed"),
                framed.numel() * framed.element_size(), _ck._dev_ptr(offsets, "offsets", torch.int64, dev),
                _ck._dev_ptr(lengths, "lengths", _ck._u32_dtypes(), dev, n), n, _ck._dev_ptr(status, "status"),
                _ck._dev_ptr(first_bad, "first_bad"), _ck._stream_ptr(stream, framed)))
        return status, first_bad

    def reframe_batch(self, framed, offsets, lengths, first_entry_id: int, new_lacs, *, out_frames=None,
                      frame_stride=None, trusted: bool = False, skip_entry_check: bool = False, stream=None):
        """LedgerFragmentReplicator's second framing (LedgerFragmentReplicator.java:436-442): verifies n
        framed entries as ``verify_batch`` does and gives every entry that verified the LAC new_lacs[i]
        and the digest that goes with it, computed from the old digest and the payload length alone
        (CRC is affine over GF(2)): the payloads are read once, by the verify. ``trusted``: the caller
        has verified these frames; no payload byte is read and the status covers only what the header
        decides (too short, CRC32's high digest word, ids) — a frame whose stored digest was wrong gets
        a digest that is wrong again. ``out_frames`` (uint8 tensor): the new [32 B header][digest] of
        entry i at byte i * frame_stride (default 32 + mac); None: `framed` is rewritten in place
        (bytes 16..23 and the digest of each frame; frames must not overlap). Entries that are not OK
        are left untouched in either. Returns (status int32[n], first_bad int64[1], digests int32[n],
        0 for entries that are not OK)."""
        import torch
        n = offsets.numel()
        dev = framed.device
        hl = METADATA_LENGTH + self.macCodeLength
        stride = 0
        if out_frames is not None:
            stride = frame_stride or hl
            if stride >= hl and n and out_frames.numel() * out_frames.element_size() < (n - 1) * stride + hl:
                raise ValueError("out_frames is too small for n frames at this stride")
        elif frame_stride is not None:
            raise ValueError("frame_stride given without out_frames")
        status = torch.empty(n, dtype=torch.int32, device=dev)
        first_bad = torch.empty(1, dtype=torch.int64, device=dev)
        digests = torch.empty(n, dtype=torch.int32, device=dev)
        with _ck._on_device(framed):
            check(lib().bkd_digest_reframe_batch(
                self.algo, self.ledgerId, first_entry_id, int(skip_entry_check), REFRAME_TRUSTED if trusted else 0,
                _ck._dev_ptr(framed, "framed"), framed.numel() * framed.element_size(),
                _ck._dev_ptr(offsets, "offsets", torch.int64, dev),
                _ck._dev_ptr(lengths, "lengths", _ck._u32_dtypes(), dev, n), n,
                _ck._dev_ptr(new_lacs, "new_lacs", torch.int64, dev, n),
                _ck._dev_ptr(out_frames, "out_frames", None, dev), stride, _ck._dev_ptr(digests, "digests"),
                _ck._dev_ptr(status, "status"), _ck._dev_ptr(first_bad, "first_bad"),
                _ck._stream_ptr(stream, framed)))
        return status, first_bad, digests

    def package_batch_segments(self, entry_ids, lacs, length_fields, payload, seg_offsets, seg_lengths, seg_first,
                               frame_stride=None, out_frames=None, stream=None, sync_check: bool = False):
        """``package_batch`` for composite payloads (a CompositeByteBuf add, digested leaf by leaf:
        DigestManager.java:62-72, 126-181): entry i's payload is the concatenation of segments
        seg_first[i] .. seg_first[i+1]-1, segment k = payload[seg_offsets[k] : + seg_lengths[k]] (int64,
        int32 and int64[n + 1] device tensors); empty segments are skipped and no bytes are copied
        together. ``out_frames`` (uint8 device tensor): frame i is written at byte i * frame_stride of it
        — it may lie inside `payload`, in bytes no segment touches; None: a new [n, frame_stride] tensor.
        Returns (frames, digests int32[n]). An out-of-range segment or a malformed seg_first raises
        BKD_ERR_BOUNDS from the stream's next ``stream_sync`` (here, when ``sync_check``).
        Short and empty segments are legal anywhere, the payload's last byte and offset == size included:
        the device reads no byte outside a segment shorter than 16 bytes."""
        return _package_segments("bkd_digest_package_batch_segments", self._c_add_first(), self.macCodeLength, None,
                                 entry_ids, lacs, length_fields, payload, seg_offsets, seg_lengths, seg_first, frame_stride,
                                 out_frames, stream, sync_check)

    def package_batch_v2(self, entry_ids, lacs, length_fields, payload, offsets, lengths, master_key, *,
                         key_stride=None, flags: int = FLAG_NONE, small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD,
                         requests=None, request_offsets=None, align: int = 1, stream=None, sync_check: bool = False):
        """The V2 add requests of n device-resident entries, whole (computeDigestAndPackageForSendingV2,
        DigestManager.java:126-167): request i = [int32 56 + mac + length][int32 packet header][20 B master
        key][32 B header][digest], and the payload copied in behind it when it is shorter than
        ``small_threshold`` (SMALL_ENTRY_SIZE_THRESHOLD; a larger entry's payload stays where it is, the
        second buffer of the reference's ByteBufList). ``master_key``: 20 bytes for all entries, or a
        uint8 device tensor of per-entry keys ``key_stride`` (default: its row length) bytes apart.
        ``request_offsets`` (int64 device tensor) with ``requests`` (uint8 device tensor) place request i
        at requests[request_offsets[i]:], any alignment, not overlapping; without them the requests are
        laid out in order, each on a multiple of ``align`` bytes (1: packed; sizing the new tensor is
        this path's one host sync — pass ``requests`` as well to avoid it). Bytes between requests are
        not written. Returns (requests, request_offsets, digests int32[n]). An out-of-range payload
        (digest 0, nothing copied) or a request outside ``requests`` (not written) raises BKD_ERR_BOUNDS
        from the stream's next ``stream_sync`` (here, when ``sync_check``)."""
        return _package_v2("bkd_digest_package_batch_v2", self._c_add_first(), self.macCodeLength, None, entry_ids, lacs,
                           length_fields, payload, offsets, lengths, master_key, key_stride, flags, small_threshold,
                           requests, request_offsets, align, stream, sync_check)

    # ---- batch host path (new; entries in host memory, SURVEY §8f rows 1-2 / BASELINE config 5) ----
    def package_batch_v2_host(self, entry_ids, lacs, length_fields, payloads, master_key, *, key_stride=None,
                              flags: int = FLAG_NONE, small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD):
        """``package_batch_v2`` for payloads in host memory (a sequence of buffers): returns (requests, a
        list of uint8 arrays, request i whole — the bytes computeDigestAndPackageForSending returns with
        useV2Protocol for a small entry, its first 60 + mac bytes for a large one; digests uint32[n]).
        ``master_key``: 20 bytes for all, or n rows of uint8 keys."""
        return _package_v2_host("bkd_digest_package_batch_v2_host", self._c_add_first(), self.macCodeLength, None,
                                entry_ids, lacs, length_fields, payloads, master_key, key_stride, flags, small_threshold)

    def verify_batch_host(self, frames, first_entry_id: int, skip_entry_check: bool = False):
        """BatchedReadOp.complete over a ByteBufList (BatchedReadOp.java:164-190): `frames` is a
        sequence of host buffers, each one framed entry. Returns (status int32[n], first_bad) with
        first_bad = n when every entry verified, else the verified prefix's length."""
        views, ptrs, lens = _ck._host_entries(frames)
        n = len(views)
        status = np.zeros(n, dtype=np.int32)
        first_bad = ctypes.c_uint64(0)
        first, _keep = self._c_first()
        check(getattr(lib(), f"bkd_digest_verify_batch{self._c_suffix}_host")(
            first, self.ledgerId, first_entry_id, int(skip_entry_check), ctypes.c_void_p(ptrs.ctypes.data),
            ctypes.c_void_p(lens.ctypes.data), n, ctypes.c_void_p(status.ctypes.data), ctypes.byref(first_bad)))
        del views
        return status, int(first_bad.value)

    def package_batch_host(self, entry_ids, lacs, length_fields, payloads, frame_stride=None):
        """PendingAddOp / LedgerFragmentReplicator packaging of host payloads (DigestManager.java:117-181)
        in one call: returns (headers uint8[n, frame_stride] = [32 B header][digest], digests uint32[n])."""
        return _package_frames_host("bkd_digest_package_batch_host", (self.algo, self.ledgerId), self.macCodeLength,
                                    None, entry_ids, lacs, length_fields, payloads, frame_stride)

    def package_batch_segments_host(self, entry_ids, lacs, length_fields, payloads, frame_stride=None):
        """``package_batch_host`` for composite payloads: each payload is a bytes-like object, a sequence
        of buffers, or a ``bytebuf.CompositeBuffer`` (its readable bytes, leaf by leaf as ``visit`` yields
        them: nested composites, reader and writer indices honoured). The digest is chained over the
        leaves as DigestManager.update chains it (DigestManager.java:62-72, 380-392); nothing is joined
        in Python; empty leaves may be passed anywhere.
        Returns (headers uint8[n, frame_stride] = [32 B header][digest], digests uint32[n])."""
        return _package_segments_host("bkd_digest_package_batch_segments_host", self._c_add_first(), self.macCodeLength,
                                      None, entry_ids, lacs, length_fields, payloads, frame_stride)

    def reframe_batch_host(self, frames, first_entry_id: int, new_lacs, trusted: bool = False,
                           skip_entry_check: bool = False):
        """``reframe_batch`` for entries in host memory: `frames` is a sequence of writable host buffers
        (bytearray, writable numpy arrays), each one framed entry, rewritten in place. Returns
        (status int32[n], first_bad, digests uint32[n])."""
        if any(isinstance(f, np.ndarray) and not f.flags.c_contiguous for f in frames):
            raise TypeError("frames must be contiguous: they are re-framed in place")
        views, ptrs, lens = _ck._host_entries(frames)
        if any(not v.flags.writeable for v in views):
            raise TypeError("frames must be writable buffers: they are re-framed in place")
        n = len(views)
        lacs = np.ascontiguousarray(new_lacs, dtype=np.int64)
        if lacs.size != n:
            raise ValueError("new_lacs must have one element per frame")
        status = np.zeros(n, dtype=np.int32)
        digests = np.zeros(n, dtype=np.uint32)
        first_bad = ctypes.c_uint64(0)
        vp = ctypes.c_void_p
        check(lib().bkd_digest_reframe_batch_host(
            self.algo, self.ledgerId, first_entry_id, int(skip_entry_check), REFRAME_TRUSTED if trusted else 0,
            vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(lacs.ctypes.data), vp(digests.ctypes.data),
            vp(status.ctypes.data), ctypes.byref(first_bad)))
        del views
        return status, int(first_bad.value), digests


# ---- batches that span many ledgers (module level: a DigestManager is bound to one ledger) ----
# An aggregation queue across pending reads and adds forms its batches across
# ledgers: a few entries from each of thousands. One digest type per call, as everywhere else.

def _algo_of(digest_type) -> int:
    if digest_type in (DigestType.CRC32C, DigestType.CRC32):
        return CRC32C if digest_type == DigestType.CRC32C else CRC32
    if isinstance(digest_type, int) and not isinstance(digest_type, enum.Enum) and digest_type in (CRC32C, CRC32):
        return digest_type
    raise ValueError(f"the batch engine computes CRC32C and CRC32 digests, not {digest_type}")


def _mac_of(algo: int) -> int:
    return 4 if algo == CRC32C else 8


def _check_csr_sizes(nreq: int, *arrays) -> None:
    if any(a is not None and a != nreq for a in arrays):
        raise ValueError("ledger_ids, first_entry_ids and skip_flags must have one element per request "
                         "(req_first one more)")


# The bodies below serve both digest families. `fn` is the library function, `first` its C arguments in front
# of the per-entry arrays ((algo[, ledger id]) for CRC, ([ledger id]) for MAC), and `keys` the MAC forms' key
# table, marshalled in front of those: (key_states, the index array, its name), None for CRC.

def _verify_requests(fn, first, keys, framed, offsets, lengths, req_first, ledger_ids, first_entry_ids, skip_flags, stream,
                     reframe=None):
    """`reframe`: (new_lacs, out_frames or None, frame stride) of the reframe forms, marshalled behind the skip
    flags."""
    import torch
    n = offsets.numel()
    dev = framed.device
    i64, u32 = torch.int64, _ck._u32_dtypes()
    if req_first.numel() < 1:
        raise ValueError("req_first holds nreq + 1 values")
    nreq = req_first.numel() - 1
    _check_csr_sizes(nreq, ledger_ids.numel(), first_entry_ids.numel(),
                     None if skip_flags is None else skip_flags.numel())
    if skip_flags is None:
        skip_flags = torch.zeros(nreq, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    req_first_bad = torch.empty(nreq, dtype=torch.int64, device=dev)
    with _ck._on_device(framed):
        check(getattr(lib(), fn)(
            *(_dev_key_table(*keys, dev, nreq) if keys else ()), *first, _ck._dev_ptr(framed, "framed"),
            framed.numel() * framed.element_size(), _ck._dev_ptr(offsets, "offsets", i64, dev),
            _ck._dev_ptr(lengths, "lengths", u32, dev, n), n, _ck._dev_ptr(req_first, "req_first", i64, dev), nreq,
            _ck._dev_ptr(ledger_ids, "ledger_ids", i64, dev), _ck._dev_ptr(first_entry_ids, "first_entry_ids", i64, dev),
            _ck._dev_ptr(skip_flags, "skip_flags", u32, dev),
            *((_ck._dev_ptr(reframe[0], "new_lacs", i64, dev, n),
               None if reframe[1] is None else _ck._dev_ptr(reframe[1], "out_frames", torch.uint8, dev), reframe[2])
              if reframe else ()),
            _ck._dev_ptr(status, "status"), _ck._dev_ptr(req_first_bad, "req_first_bad"), _ck._stream_ptr(stream, framed)))
    return status, req_first_bad


def verify_requests(digest_type, framed, offsets, lengths, req_first, ledger_ids, first_entry_ids, skip_flags=None,
                    stream=None):
    """Verifies n framed device-resident entries grouped into read requests of different ledgers in one
    launch sequence (bkd_digest_verify_requests). Request r owns entries [req_first[r], req_first[r+1])
    (int64[nreq + 1], non-decreasing, from 0 to n; empty requests are legal), is read from ledger
    ledger_ids[r] and expects entry ids first_entry_ids[r], first_entry_ids[r] + 1, ...; skip_flags[r]
    bit 0 skips its entry-id check. Returns (status int32[n], req_first_bad int64[nreq]): request r's
    entries [0, req_first_bad[r]) verified — BatchedReadOp's verified prefix per request. A malformed
    req_first raises BKD_ERR_BOUNDS from the stream's next ``stream_sync``."""
    return _verify_requests("bkd_digest_verify_requests", (_algo_of(digest_type),), None, framed, offsets, lengths,
                            req_first, ledger_ids, first_entry_ids, skip_flags, stream)


def package_batch_ledgers(digest_type, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths,
                          frame_stride=None, stream=None, sync_check: bool = False):
    """``DigestManager.package_batch`` with ledger_ids[i] (int64[n]) framing entry i: returns
    (frames[n, frame_stride] uint8, digests int32[n])."""
    algo = _algo_of(digest_type)
    return _package_frames("bkd_digest_package_batch_ledgers", (algo,), _mac_of(algo), (ledger_ids,), entry_ids, lacs,
                           length_fields, payload, offsets, lengths, frame_stride, None, stream, sync_check)


def _verify_requests_host(fn, first, keys, frames, req_first, ledger_ids, first_entry_ids, skip_flags, new_lacs=None):
    """`new_lacs`: the reframe forms' LACs, one per frame, marshalled behind the skip flags; the frames are then
    written and must be writable contiguous buffers."""
    if new_lacs is not None and any(isinstance(f, np.ndarray) and not f.flags.c_contiguous for f in frames):
        raise TypeError("frames must be contiguous: they are re-framed in place")
    views, ptrs, lens = _ck._host_entries(frames)
    if new_lacs is not None and any(not v.flags.writeable for v in views):
        raise TypeError("frames must be writable buffers: they are re-framed in place")
    n = len(views)
    lacs = None if new_lacs is None else np.ascontiguousarray(new_lacs, dtype=np.int64)
    if lacs is not None and lacs.size != n:
        raise ValueError("new_lacs must have one element per frame")
    first_of = np.ascontiguousarray(req_first, dtype=np.uint64)
    if first_of.size < 1:
        raise ValueError("req_first holds nreq + 1 values")
    nreq = first_of.size - 1
    lids = np.ascontiguousarray(ledger_ids, dtype=np.int64)
    eids = np.ascontiguousarray(first_entry_ids, dtype=np.int64)
    flags = np.zeros(nreq, dtype=np.uint32) if skip_flags is None else np.ascontiguousarray(skip_flags, dtype=np.uint32)
    _check_csr_sizes(nreq, lids.size, eids.size, flags.size)
    _keep, table = _host_key_table(*keys, nreq) if keys else (None, ())
    status = np.zeros(n, dtype=np.int32)
    first_bad = np.zeros(nreq, dtype=np.uint64)
    vp = ctypes.c_void_p
    check(getattr(lib(), fn)(
        *table, *first, vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(first_of.ctypes.data), nreq, vp(lids.ctypes.data),
        vp(eids.ctypes.data), vp(flags.ctypes.data), *(() if lacs is None else (vp(lacs.ctypes.data),)),
        vp(status.ctypes.data), vp(first_bad.ctypes.data)))
    del views
    return status, first_bad


def verify_requests_host(digest_type, frames, req_first, ledger_ids, first_entry_ids, skip_flags=None):
    """``verify_requests`` for entries in host memory: `frames` is a sequence of host buffers, each one
    framed entry; the request arrays are host sequences. A malformed req_first raises
    BKD_ERR_INVALID_ARG before any work. Returns (status int32[n], req_first_bad uint64[nreq])."""
    return _verify_requests_host("bkd_digest_verify_requests_host", (_algo_of(digest_type),), None, frames, req_first,
                                 ledger_ids, first_entry_ids, skip_flags)


def package_batch_ledgers_host(digest_type, ledger_ids, entry_ids, lacs, length_fields, payloads, frame_stride=None):
    """``DigestManager.package_batch_host`` with ledger_ids[i] framing entry i: returns
    (headers uint8[n, frame_stride] = [32 B header][digest], digests uint32[n])."""
    algo = _algo_of(digest_type)
    return _package_frames_host("bkd_digest_package_batch_ledgers_host", (algo,), _mac_of(algo),
                                np.ascontiguousarray(ledger_ids, dtype=np.int64), entry_ids, lacs, length_fields,
                                payloads, frame_stride)


# ---- MAC ledgers across ledgers: a table of key states and an index per request or per entry ----
# One GPU lane hashes one MAC entry, so only a batch across thousands of ledgers fills the device, and every
# MAC ledger has its own password: these calls take uint32[nkeys, 10] key states (``mac_key_table``) where
# MacDigestManager's batch methods take the one key of their ledger.

def mac_key_table(passwords) -> np.ndarray:
    """uint32[nkeys, 10]: row k is the key state of a MAC ledger with passwords[k] (``checksum.mac_key_init``).
    The host forms take it as it is; the device forms take it as a tensor on the device, e.g.
    ``torch.from_numpy(table.view(np.int32)).to(device)``."""
    table = np.zeros((len(passwords), 10), dtype=np.uint32)
    for k, passwd in enumerate(passwords):
        table[k] = _ck.mac_key_init(passwd)
    return table


def _dev_key_table(key_states, index, name: str, dev, min_numel: int):
    """(pointer of the device key table, its rows, pointer of the uint32 index tensor)."""
    u32 = _ck._u32_dtypes()
    if key_states.numel() % 10:
        raise ValueError("key_states holds ten words per key (mac_key_table)")
    return (_ck._dev_ptr(key_states, "key_states", u32, dev), key_states.numel() // 10,
            _ck._dev_ptr(index, name, u32, dev, min_numel))


def _host_key_table(key_states, index, name: str, count: int):
    """(the table uint32[nkeys, 10] and the index uint32[count] to keep alive, then their C arguments); an
    index of None is a null pointer (row 0 for everything)."""
    table = np.ascontiguousarray(key_states, dtype=np.uint32)
    if table.size % 10:
        raise ValueError("key_states holds ten words per key (mac_key_table)")
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
    if idx is not None and idx.size != count:
        raise ValueError(f"{name} has {idx.size} elements, needs {count}")
    return (table, idx), (ctypes.c_void_p(table.ctypes.data), table.size // 10,
                          ctypes.c_void_p(0 if idx is None else idx.ctypes.data))


def verify_requests_mac(key_states, req_keys, framed, offsets, lengths, req_first, ledger_ids, first_entry_ids,
                        skip_flags=None, stream=None):
    """``verify_requests`` for MAC ledgers (bkd_digest_verify_requests_mac): request r is keyed with row
    req_keys[r] (int32 / uint32 [nreq]) of key_states (a device tensor of ``mac_key_table``'s words). A key
    index outside the table gives its entries VERIFY_TOO_SHORT and, like a malformed req_first, raises
    BKD_ERR_BOUNDS from the stream's next ``stream_sync``. Returns (status int32[n], req_first_bad int64[nreq])."""
    return _verify_requests("bkd_digest_verify_requests_mac", (), (key_states, req_keys, "req_keys"), framed, offsets,
                            lengths, req_first, ledger_ids, first_entry_ids, skip_flags, stream)


def package_batch_ledgers_mac(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths,
                              frame_stride=None, stream=None, sync_check: bool = False):
    """``MacDigestManager.package_batch`` with ledger_ids[i] framing entry i and row key_of[i] of key_states
    keying it (bkd_digest_package_batch_ledgers_mac): returns (frames[n, frame_stride] uint8, macs uint8[n, 20]).
    A key index outside the table: the header is written, the MAC bytes are zero, BKD_ERR_BOUNDS from the
    stream's next sync (here, when ``sync_check``)."""
    import torch
    n = offsets.numel()
    frames, _ = _package_frames("bkd_digest_package_batch_ledgers_mac",
                                _dev_key_table(key_states, key_of, "key_of", payload.device, n), MAC_LENGTH,
                                (ledger_ids,), entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride,
                                None, stream, sync_check, with_digests=False)
    with _ck._on_device(payload):
        with torch.cuda.stream(stream) if hasattr(stream, "cuda_stream") else contextlib.nullcontext():
            macs = frames[:, METADATA_LENGTH:METADATA_LENGTH + MAC_LENGTH].contiguous()
    return frames, macs


def verify_requests_mac_host(key_states, req_keys, frames, req_first, ledger_ids, first_entry_ids, skip_flags=None):
    """``verify_requests_host`` for MAC ledgers: key_states uint32[nkeys, 10] and req_keys[nreq] in host
    memory. A key index outside the table or a malformed req_first raises BKD_ERR_INVALID_ARG before any
    work. Returns (status int32[n], req_first_bad uint64[nreq])."""
    return _verify_requests_host("bkd_digest_verify_requests_mac_host", (), (key_states, req_keys, "req_keys"), frames,
                                 req_first, ledger_ids, first_entry_ids, skip_flags)


def reframe_requests_mac(key_states, req_keys, framed, offsets, lengths, req_first, ledger_ids, first_entry_ids, new_lacs,
                         skip_flags=None, *, out_frames=None, frame_stride=None, trusted: bool = False, stream=None):
    """Re-replication of MAC ledgers in one pass (bkd_digest_reframe_requests_mac): the requests, keys, statuses
    and prefixes of ``verify_requests_mac``, and every frame whose status is 0 re-framed with new_lacs[i]
    (int64[n]) — in place (header bytes 16..23 and the MAC at 32..51 of `framed`), or, with `out_frames` (a
    uint8 device tensor of n strides of `frame_stride` >= 52 bytes, default 52), as [32 B header][20 B MAC] at
    out_frames + i * frame_stride, `framed` left alone. No byte of a frame that is not OK is written.
    ``trusted``: the caller has verified the frames; only the new MAC is computed and the status is what the
    header alone decides (never 2) — the MAC written is valid for the bytes as they lie.
    Returns (status int32[n], req_first_bad int64[nreq])."""
    n = offsets.numel()
    if out_frames is not None and frame_stride is None:
        frame_stride = METADATA_LENGTH + MAC_LENGTH
    stride = frame_stride or 0
    if (out_frames is not None and n and stride >= METADATA_LENGTH + MAC_LENGTH and
            out_frames.numel() * out_frames.element_size() < (n - 1) * stride + METADATA_LENGTH + MAC_LENGTH):
        raise ValueError("out_frames is too small for n frames at this stride")
    return _verify_requests("bkd_digest_reframe_requests_mac", (REFRAME_TRUSTED if trusted else 0,),
                            (key_states, req_keys, "req_keys"), framed, offsets, lengths, req_first, ledger_ids,
                            first_entry_ids, skip_flags, stream, reframe=(new_lacs, out_frames, stride))


def reframe_requests_mac_host(key_states, req_keys, frames, req_first, ledger_ids, first_entry_ids, new_lacs,
                              skip_flags=None, *, trusted: bool = False):
    """``reframe_requests_mac`` for entries in host memory: `frames` is a sequence of writable contiguous host
    buffers (bytearray, writable numpy arrays), each one framed entry, re-framed in place where its status is
    0. Returns (status int32[n], req_first_bad uint64[nreq])."""
    return _verify_requests_host("bkd_digest_reframe_requests_mac_host", (REFRAME_TRUSTED if trusted else 0,),
                                 (key_states, req_keys, "req_keys"), frames, req_first, ledger_ids, first_entry_ids,
                                 skip_flags, new_lacs=new_lacs)


def package_batch_ledgers_mac_host(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payloads,
                                   frame_stride=None):
    """``MacDigestManager.package_batch_host`` with ledger_ids[i] framing entry i and row key_of[i] keying it:
    returns (headers uint8[n, frame_stride] = [32 B header][20 B MAC], macs uint8[n, 20])."""
    _keep, keys = _host_key_table(key_states, key_of, "key_of", len(payloads))
    frames, _ = _package_frames_host("bkd_digest_package_batch_ledgers_mac_host", keys, MAC_LENGTH,
                                     np.ascontiguousarray(ledger_ids, dtype=np.int64), entry_ids, lacs, length_fields,
                                     payloads, frame_stride, with_digests=False)
    return frames, frames[:, METADATA_LENGTH:METADATA_LENGTH + MAC_LENGTH].copy()


# ---- composite payloads (a CompositeByteBuf add: DigestManager.java:62-72, 126-181, 380-392) ----

def _package_segments(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payload, seg_offsets, seg_lengths,
                      seg_first, frame_stride, out_frames, stream, sync_check, keys=None, with_digests: bool = True):
    """The device forms over composite payloads (`fn`, `first`, `keys`: above). Returns (frames, digests int32[n]
    or None)."""
    import torch
    if seg_first.numel() < 1:
        raise ValueError("seg_first holds n + 1 values")
    n = seg_first.numel() - 1
    nseg = seg_offsets.numel()
    if seg_lengths.numel() != nseg:
        raise ValueError("seg_offsets/seg_lengths size mismatch")
    hl = METADATA_LENGTH + mac
    stride = frame_stride or hl
    dev = payload.device
    if out_frames is None:
        out_frames = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    elif stride >= hl and n and out_frames.numel() * out_frames.element_size() < (n - 1) * stride + hl:
        raise ValueError("out_frames is too small for n frames at this stride")
    digests = torch.empty(n, dtype=torch.int32, device=dev) if with_digests else None
    i64, u32 = torch.int64, _ck._u32_dtypes()
    with _ck._on_device(payload):
        st = _ck._stream_ptr(stream, payload)
        check(getattr(lib(), fn)(
            *(_dev_key_table(*keys, dev, n) if keys else ()), *first, _ck._dev_ptr(ledger_ids, "ledger_ids", i64, dev, n),
            _ck._dev_ptr(entry_ids, "entry_ids", i64, dev, n), _ck._dev_ptr(lacs, "lacs", i64, dev, n),
            _ck._dev_ptr(length_fields, "length_fields", i64, dev, n), _ck._dev_ptr(payload, "payload"),
            payload.numel() * payload.element_size(), _ck._dev_ptr(seg_offsets, "seg_offsets", i64, dev),
            _ck._dev_ptr(seg_lengths, "seg_lengths", u32, dev), nseg, _ck._dev_ptr(seg_first, "seg_first", i64, dev), n,
            _ck._dev_ptr(out_frames, "out_frames", torch.uint8, dev), stride,
            *((_ck._dev_ptr(digests, "digests"),) if with_digests else ()), st))
        if sync_check:
            check(lib().bkd_stream_sync(st))
    return out_frames, digests


def package_batch_segments(digest_type, ledger_ids, entry_ids, lacs, length_fields, payload, seg_offsets, seg_lengths,
                           seg_first, frame_stride=None, out_frames=None, stream=None, sync_check: bool = False):
    """``DigestManager.package_batch_segments`` with ledger_ids[i] (int64[n]) framing entry i: an
    aggregation queue's composite adds across ledgers in one launch sequence."""
    if ledger_ids is None:
        raise ValueError("ledger_ids holds one ledger id per entry")
    algo = _algo_of(digest_type)
    return _package_segments("bkd_digest_package_batch_segments", (algo, 0), _mac_of(algo), ledger_ids, entry_ids, lacs,
                             length_fields, payload, seg_offsets, seg_lengths, seg_first, frame_stride, out_frames, stream,
                             sync_check)


def _leaves(payload) -> list:
    """The host buffers a payload is made of, in order: the readable leaves of a CompositeBuffer
    (ByteBufVisitor's walk, bytebuf.CompositeBuffer.visit), one buffer for a bytes-like object, the
    leaves of each element for a sequence of buffers."""
    if isinstance(payload, CompositeBuffer):
        return [_ck._host_view(leaf)[off:off + cnt]
                for leaf, off, cnt in payload.visit(payload.reader_index, payload.readable_bytes())]
    if isinstance(payload, (list, tuple)):
        return [v for part in payload for v in _leaves(part)]
    return [_ck._host_view(payload)]


def _package_segments_host(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payloads, frame_stride, keys=None,
                           with_digests: bool = True):
    """The host forms over composite payloads (`fn`, `first`, `keys`: above). Returns (frames uint8[n,
    frame_stride], digests uint32[n] or None)."""
    leaves = [_leaves(p) for p in payloads]
    n = len(leaves)
    seg_first = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(l) for l in leaves], out=seg_first[1:])
    views, ptrs, lens, seg_first, _ = _ck._host_segments([v for l in leaves for v in l], seg_first)
    stride = frame_stride or (METADATA_LENGTH + mac)
    ids, lac, lf, lids = _entry_fields(n, entry_ids, lacs, length_fields, ledger_ids, optional_ledgers=True)
    _keep, table = _host_key_table(*keys, n) if keys else (None, ())
    frames = np.zeros((n, stride), dtype=np.uint8)
    digests = np.zeros(n, dtype=np.uint32) if with_digests else None
    vp = ctypes.c_void_p
    check(getattr(lib(), fn)(
        *table, *first, vp(0 if lids is None else lids.ctypes.data), vp(ids.ctypes.data), vp(lac.ctypes.data),
        vp(lf.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), len(views), vp(seg_first.ctypes.data), n,
        vp(frames.ctypes.data), stride, *((vp(digests.ctypes.data),) if with_digests else ())))
    del views
    return frames, digests


def package_batch_segments_host(digest_type, ledger_ids, entry_ids, lacs, length_fields, payloads, frame_stride=None):
    """``DigestManager.package_batch_segments_host`` with ledger_ids[i] framing entry i."""
    if ledger_ids is None:
        raise ValueError("ledger_ids holds one ledger id per entry")
    algo = _algo_of(digest_type)
    return _package_segments_host("bkd_digest_package_batch_segments_host", (algo, 0), _mac_of(algo), ledger_ids,
                                  entry_ids, lacs, length_fields, payloads, frame_stride)


# ---- V2 add requests, packaged whole (DigestManager.java:126-167) ----

V2_PREFIX_LENGTH = 4 + 4 + MASTER_KEY_LENGTH  # the two ints and the master key in front of the header


def request_sizes_v2(algo: int, lengths, small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD):
    """Bytes of each V2 request buffer (bufferSize, DigestManager.java:135): 60 + mac, and the payload
    when it is shorter than `small_threshold`. `lengths`: a numpy array or a torch tensor."""
    return _request_sizes(V2_PREFIX_LENGTH + METADATA_LENGTH + _mac_of(algo), lengths, small_threshold)


def request_sizes_v2_mac(lengths, small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD):
    """``request_sizes_v2`` for MAC ledgers: an 80-byte head (28 + 32 + the 20-byte MAC), and the payload
    when it is shorter than `small_threshold`."""
    return _request_sizes(V2_PREFIX_LENGTH + METADATA_LENGTH + MAC_LENGTH, lengths, small_threshold)


def _request_sizes(head: int, lengths, small_threshold: int):
    if isinstance(lengths, np.ndarray):
        l = lengths.astype(np.int64)
        return head + np.where(l < small_threshold, l, 0)
    import torch
    l = lengths.to(torch.int64) & 0xFFFFFFFF  # (an int32 tensor holds the u32 lengths' bit patterns)
    return head + torch.where(l < small_threshold, l, torch.zeros_like(l))


def request_offsets_v2(sizes, align: int = 1):
    """Requests laid out in order, each starting on a multiple of `align` bytes (1: packed):
    (offsets int64[n], total bytes as a 0-d array / tensor)."""
    if align < 1:
        raise ValueError("align must be at least 1")
    slots = (sizes + (align - 1)) // align * align
    ends = slots.cumsum(0)
    return ends - slots, (ends[-1] if len(ends) else ends.sum())


def _master_keys(master_key, n: int, key_stride, to_device=None):
    """(keys, key_stride): one 20-byte key for all (bytes-like: stride 0), or per-entry keys, a uint8
    array / tensor of n rows of `key_stride` >= 20 bytes (default: its row length)."""
    if isinstance(master_key, (bytes, bytearray, memoryview)):
        key = bytes(master_key)
        if len(key) < MASTER_KEY_LENGTH:
            raise ValueError("a master key holds 20 bytes")
        if key_stride not in (None, 0):
            raise ValueError("one key for all entries has key_stride 0")
        keys = np.frombuffer(key[:MASTER_KEY_LENGTH], dtype=np.uint8)
        return (to_device(keys) if to_device else keys), 0
    rows = master_key.shape[-1] if master_key.ndim > 1 else MASTER_KEY_LENGTH
    stride = rows if key_stride is None else int(key_stride)
    size = master_key.numel() if to_device else master_key.size
    if stride < MASTER_KEY_LENGTH or (n and size < (n - 1) * stride + MASTER_KEY_LENGTH):
        raise ValueError("master keys: n keys of 20 bytes, key_stride >= 20 bytes apart")
    return master_key, stride


def _package_v2(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths, master_key,
                key_stride, flags, small_threshold, requests, request_offsets, align, stream, sync_check, keys=None,
                with_digests: bool = True):
    """The device forms that write V2 add requests (`fn`, `first`, `keys`: above). Returns (requests,
    request_offsets, digests int32[n] or None)."""
    import torch
    n = offsets.numel()
    dev = payload.device
    i64, u32 = torch.int64, _ck._u32_dtypes()
    mkeys, stride = _master_keys(master_key, n, key_stride, lambda a: torch.from_numpy(a.copy()).to(dev))
    if request_offsets is None:
        sizes = _request_sizes(V2_PREFIX_LENGTH + METADATA_LENGTH + mac, lengths, small_threshold)
        request_offsets, total = request_offsets_v2(sizes, align)
        if requests is None:  # (the one host sync of this path: pass `requests` or offsets to avoid it)
            requests = torch.empty(int(total) if n else 0, dtype=torch.uint8, device=dev)
    elif requests is None:
        raise ValueError("request_offsets given without the requests buffer they index")
    digests = torch.empty(n, dtype=torch.int32, device=dev) if with_digests else None
    with _ck._on_device(payload):
        st = _ck._stream_ptr(stream, payload)
        check(getattr(lib(), fn)(
            *(_dev_key_table(*keys, dev, n) if keys else ()), *first, _ck._dev_ptr(ledger_ids, "ledger_ids", i64, dev, n),
            _ck._dev_ptr(entry_ids, "entry_ids", i64, dev, n), _ck._dev_ptr(lacs, "lacs", i64, dev, n),
            _ck._dev_ptr(length_fields, "length_fields", i64, dev, n), _ck._dev_ptr(payload, "payload"),
            payload.numel() * payload.element_size(), _ck._dev_ptr(offsets, "offsets", i64, dev),
            _ck._dev_ptr(lengths, "lengths", u32, dev, n), n, _ck._dev_ptr(mkeys, "master_key", torch.uint8, dev),
            stride, flags, small_threshold, _ck._dev_ptr(requests, "requests", torch.uint8, dev), requests.numel(),
            _ck._dev_ptr(request_offsets, "request_offsets", i64, dev, n),
            *((_ck._dev_ptr(digests, "digests"),) if with_digests else ()), st))
        if sync_check:
            check(lib().bkd_stream_sync(st))
    return requests, request_offsets, digests


def package_batch_v2(digest_type, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths, master_key,
                     *, key_stride=None, flags: int = FLAG_NONE, small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD,
                     requests=None, request_offsets=None, align: int = 1, stream=None, sync_check: bool = False):
    """``DigestManager.package_batch_v2`` with ledger_ids[i] (int64[n]) framing entry i."""
    if ledger_ids is None:
        raise ValueError("ledger_ids holds one ledger id per entry")
    algo = _algo_of(digest_type)
    return _package_v2("bkd_digest_package_batch_v2", (algo, 0), _mac_of(algo), ledger_ids, entry_ids, lacs, length_fields,
                       payload, offsets, lengths, master_key, key_stride, flags, small_threshold, requests,
                       request_offsets, align, stream, sync_check)


def _package_v2_host(fn, first, mac, ledger_ids, entry_ids, lacs, length_fields, payloads, master_key, key_stride, flags,
                     small_threshold, keys=None, with_digests: bool = True):
    """The host forms that write V2 add requests (`fn`, `first`, `keys`: above). Returns (the requests, views of
    one allocation, digests uint32[n] or None)."""
    views, ptrs, lens = _ck._host_entries(payloads)
    n = len(views)
    ids, lac, lf, lids = _entry_fields(n, entry_ids, lacs, length_fields, ledger_ids, optional_ledgers=True)
    if not isinstance(master_key, (bytes, bytearray, memoryview)):
        master_key = np.ascontiguousarray(master_key, dtype=np.uint8)
    mkeys, stride = _master_keys(master_key, n, key_stride)
    _keep, table = _host_key_table(*keys, n) if keys else (None, ())
    offs, total = request_offsets_v2(_request_sizes(V2_PREFIX_LENGTH + METADATA_LENGTH + mac, lens, small_threshold))
    buf = np.zeros(int(total) if n else 0, dtype=np.uint8)
    rptr = (buf.ctypes.data + offs).astype(np.uint64)
    digests = np.zeros(n, dtype=np.uint32) if with_digests else None
    vp = ctypes.c_void_p
    check(getattr(lib(), fn)(
        *table, *first, vp(0 if lids is None else lids.ctypes.data), vp(ids.ctypes.data), vp(lac.ctypes.data),
        vp(lf.ctypes.data), vp(ptrs.ctypes.data), vp(lens.ctypes.data), n, vp(mkeys.ctypes.data), stride, flags,
        small_threshold, vp(rptr.ctypes.data), *((vp(digests.ctypes.data),) if with_digests else ())))
    del views
    ends = np.append(offs[1:], total) if n else offs
    return [buf[a:b] for a, b in zip(offs.tolist(), ends.tolist())], digests


def package_batch_v2_host(digest_type, ledger_ids, entry_ids, lacs, length_fields, payloads, master_key, *,
                          key_stride=None, flags: int = FLAG_NONE,
                          small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD):
    """``DigestManager.package_batch_v2_host`` with ledger_ids[i] framing entry i."""
    if ledger_ids is None:
        raise ValueError("ledger_ids holds one ledger id per entry")
    algo = _algo_of(digest_type)
    return _package_v2_host("bkd_digest_package_batch_v2_host", (algo, 0), _mac_of(algo), ledger_ids, entry_ids, lacs,
                            length_fields, payloads, master_key, key_stride, flags, small_threshold)


# ---- MAC adds: composite payloads and V2 add requests across ledgers ----
# The parameters of their CRC namesakes with the key table and the per-entry key rows in front.
# key_of None: row 0 keys every entry; ledger_ids None: `ledger_id` frames every entry.

def package_batch_segments_mac(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payload, seg_offsets,
                               seg_lengths, seg_first, frame_stride=None, out_frames=None, stream=None,
                               sync_check: bool = False, ledger_id: int = 0):
    """``package_batch_segments`` for MAC ledgers (bkd_digest_package_batch_segments_mac): entry i is the
    segments seg_first[i] .. seg_first[i + 1] - 1 of `payload`, hashed as one byte stream by one lane, keyed
    with row key_of[i] of key_states and framed for ledger_ids[i]. Returns (frames[n, frame_stride] uint8,
    macs uint8[n, 20]). An entry with a key index outside the table, a segment out of range or more than
    MAC_MAX_ENTRY bytes is not read: its header is written, its MAC bytes are zero, BKD_ERR_BOUNDS from the
    stream's next sync (here, when ``sync_check``)."""
    import torch
    out_frames, _ = _package_segments("bkd_digest_package_batch_segments_mac", (ledger_id,), MAC_LENGTH, ledger_ids,
                                      entry_ids, lacs, length_fields, payload, seg_offsets, seg_lengths, seg_first,
                                      frame_stride, out_frames, stream, sync_check, (key_states, key_of, "key_of"), False)
    hl = METADATA_LENGTH + MAC_LENGTH
    with _ck._on_device(payload):
        with torch.cuda.stream(stream) if hasattr(stream, "cuda_stream") else contextlib.nullcontext():
            macs = torch.as_strided(out_frames.reshape(-1), (seg_first.numel() - 1, hl),
                                    (frame_stride or hl, 1))[:, METADATA_LENGTH:].contiguous()
    return out_frames, macs


def package_batch_segments_mac_host(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payloads,
                                    frame_stride=None, ledger_id: int = 0):
    """``package_batch_segments_host`` for MAC ledgers (bkd_digest_package_batch_segments_mac_host):
    payloads[i] is a CompositeBuffer, a sequence of host buffers or one buffer; its leaves are hashed in
    order without being joined on the CPU route and laid end to end in pinned staging on the GPU route.
    Returns (headers uint8[n, frame_stride] = [32 B header][20 B MAC], macs uint8[n, 20])."""
    frames, _ = _package_segments_host("bkd_digest_package_batch_segments_mac_host", (ledger_id,), MAC_LENGTH, ledger_ids,
                                       entry_ids, lacs, length_fields, payloads, frame_stride,
                                       (key_states, key_of, "key_of"), False)
    return frames, frames[:, METADATA_LENGTH:METADATA_LENGTH + MAC_LENGTH].copy()


def package_batch_v2_mac(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payload, offsets, lengths,
                         master_key, *, key_stride=None, flags: int = FLAG_NONE,
                         small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD, requests=None, request_offsets=None,
                         align: int = 1, stream=None, sync_check: bool = False, ledger_id: int = 0,
                         with_macs: bool = True):
    """``package_batch_v2`` for MAC ledgers (bkd_digest_package_batch_v2_mac): request i is [int32 BE 76 + len]
    [int32 BE packet header][20 B master key][32 B header][20 B MAC] and the payload behind it when it is
    shorter than `small_threshold`, at request_offsets[i] of `requests` (``request_sizes_v2_mac``). The lane
    that hashed an entry writes its 80-byte head; the copy pass is the CRC call's. Returns (requests,
    request_offsets, macs uint8[n, 20], gathered from the requests that lie inside the buffer; None when
    ``with_macs`` is false, which saves the gather)."""
    import torch
    requests, request_offsets, _ = _package_v2(
        "bkd_digest_package_batch_v2_mac", (ledger_id,), MAC_LENGTH, ledger_ids, entry_ids, lacs, length_fields, payload,
        offsets, lengths, master_key, key_stride, flags, small_threshold, requests, request_offsets, align, stream,
        sync_check, (key_states, key_of, "key_of"), False)
    if not with_macs:
        return requests, request_offsets, None
    n, dev = offsets.numel(), payload.device
    with _ck._on_device(payload):
        with torch.cuda.stream(stream) if hasattr(stream, "cuda_stream") else contextlib.nullcontext():
            # the MAC bytes of every request whose head lies inside the buffer; zeros for the others
            at = request_offsets.to(torch.int64) + (V2_PREFIX_LENGTH + METADATA_LENGTH)
            inside = (at >= 0) & (at + MAC_LENGTH <= requests.numel())
            idx = torch.where(inside, at, torch.zeros_like(at))[:, None] + torch.arange(MAC_LENGTH, device=dev)[None, :]
            flat = requests.reshape(-1)
            macs = flat[idx] * inside[:, None].to(torch.uint8) if flat.numel() >= MAC_LENGTH else \
                torch.zeros((n, MAC_LENGTH), dtype=torch.uint8, device=dev)
    return requests, request_offsets, macs


def package_batch_v2_mac_host(key_states, key_of, ledger_ids, entry_ids, lacs, length_fields, payloads, master_key, *,
                              key_stride=None, flags: int = FLAG_NONE,
                              small_threshold: int = SMALL_ENTRY_SIZE_THRESHOLD, ledger_id: int = 0):
    """``package_batch_v2_host`` for MAC ledgers (bkd_digest_package_batch_v2_mac_host): returns (the list of
    request buffers, views of one allocation, macs uint8[n, 20])."""
    reqs, _ = _package_v2_host("bkd_digest_package_batch_v2_mac_host", (ledger_id,), MAC_LENGTH, ledger_ids, entry_ids,
                               lacs, length_fields, payloads, master_key, key_stride, flags, small_threshold,
                               (key_states, key_of, "key_of"), False)
    head = V2_PREFIX_LENGTH + METADATA_LENGTH
    macs = np.array([r[head:head + MAC_LENGTH] for r in reqs], dtype=np.uint8).reshape(len(reqs), MAC_LENGTH)
    return reqs, macs


class CRC32CDigestManager(DigestManager):
    """CRC32CDigestManager.java:27-62."""
    algo = CRC32C
    macCodeLength = 4

    def digest_bytes(self, digest: int) -> bytes:  # buf.writeInt(digest)  (:44-46)
        return struct.pack(">i", _ck.to_java_int(digest))

    def isInt32Digest(self) -> bool:
        return True


class CRC32DigestManager(DigestManager):
    """CRC32DigestManager.java:28-87: the CRC is carried as an int through update() and written as
    writeLong(crcValue & 0xffffffffL) (:60-63, DirectMemoryCRC32Digest.java:39-43)."""
    algo = CRC32
    macCodeLength = 8

    def digest_bytes(self, digest: int) -> bytes:
        return struct.pack(">Q", digest & 0xFFFFFFFF)

    def isInt32Digest(self) -> bool:
        return False


class DummyDigestManager(DigestManager):
    """DummyDigestManager.java:30-62: no digest bytes, update is a no-op."""
    algo = None
    macCodeLength = 0

    def internalUpdate(self, digest, buf, offset, length):
        return 0

    def digest_bytes(self, digest: int) -> bytes:
        return b""

    def isInt32Digest(self) -> bool:
        return True

    def package_batch(self, *a, **k):
        raise NotImplementedError("DUMMY digests need no device work")

    verify_batch = package_batch_host = verify_batch_host = reframe_batch = reframe_batch_host = package_batch
    package_batch_segments = package_batch_segments_host = package_batch
    package_batch_v2 = package_batch_v2_host = package_batch


class MacDigestManager(DigestManager):
    """MacDigestManager.java:46-107: HmacSHA1 keyed with SHA1("mac" || passwd), a 20-byte digest.

    The reference's stateful ``Mac`` (update per buffer, doFinal in populateValueAndReset, :86-101) maps
    onto collecting the pieces of one entry: ``update`` returns the pieces seen so far and
    ``digest_bytes`` finishes them through the library's CPU HMAC (bkd_mac_cpu); composite buffers are
    joined. That is the latency-bound per-call path. The batch methods run one entry per GPU lane
    (bkd_mac_batch and the two framed calls) or one entry per host task."""
    algo = None
    macCodeLength = 20

    def __init__(self, ledgerId: int, passwd: bytes, useV2Protocol: bool = False):
        super().__init__(ledgerId, useV2Protocol)
        self.passwd = bytes(passwd)
        self.key_state = _ck.mac_key_init(self.passwd)

    @staticmethod
    def genDigest(pad: str, passwd: bytes) -> bytes:  # :79-84
        return _ck.mac_gen_digest(pad.encode(), passwd)

    def internalUpdate(self, digest, buf, offset: int, length: int):
        piece = bytes(memoryview(buf).cast("B")[offset:offset + length])
        return (digest or ()) + (piece,)

    def digest_bytes(self, digest) -> bytes:
        return _ck.mac_cpu(self.key_state, b"".join(digest or ()))

    def isInt32Digest(self) -> bool:
        return False

    # ---- batches: verify_batch and verify_batch_host are the base class's, through these two ----
    _c_suffix = "_mac"

    def _c_first(self):
        ks, kp = _ck._key_ptr(self.key_state)
        return kp, ks

    def package_batch(self, entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride=None,
                      stream=None, sync_check: bool = False, out_frames=None):
        """As ``DigestManager.package_batch`` with frames of [32 B header][20 B MAC] (``out_frames``: a
        uint8 [n, frame_stride] device tensor to write them into, only 52 bytes of each row); returns
        (frames[n, frame_stride] uint8, macs uint8[n, 20], a copy of the frames' MAC bytes). A payload
        out of range or longer than MAC_MAX_ENTRY is not read: zero MAC, BKD_ERR_BOUNDS from the stream's
        next sync (here, when ``sync_check``)."""
        import torch
        first, _keep = self._c_first()
        frames, _ = _package_frames("bkd_digest_package_batch_mac", (first, self.ledgerId), self.macCodeLength, (),
                                    entry_ids, lacs, length_fields, payload, offsets, lengths, frame_stride, out_frames,
                                    stream, sync_check, with_digests=False)
        with _ck._on_device(payload):
            with torch.cuda.stream(stream) if hasattr(stream, "cuda_stream") else contextlib.nullcontext():
                macs = frames[:, METADATA_LENGTH:METADATA_LENGTH + self.macCodeLength].contiguous()
        return frames, macs

    def package_batch_host(self, entry_ids, lacs, length_fields, payloads, frame_stride=None):
        """As ``DigestManager.package_batch_host``: (headers uint8[n, frame_stride] = [32 B header]
        [20 B MAC], macs uint8[n, 20])."""
        first, _keep = self._c_first()
        frames, _ = _package_frames_host("bkd_digest_package_batch_mac_host", (first, self.ledgerId),
                                         self.macCodeLength, None, entry_ids, lacs, length_fields, payloads,
                                         frame_stride, with_digests=False)
        return frames, frames[:, METADATA_LENGTH:METADATA_LENGTH + self.macCodeLength].copy()

    def _no_batch(self, *a, **k):
        raise NotImplementedError(
            "MAC ledgers have package_batch / verify_batch and their _host forms only: reframes, composite "
            "and V2 batches of MAC ledgers are the module-level reframe_requests_mac, "
            "package_batch_segments_mac / package_batch_v2_mac and their _host forms, which take a key table")

    reframe_batch = reframe_batch_host = _no_batch
    package_batch_segments = package_batch_segments_host = _no_batch
    package_batch_v2 = package_batch_v2_host = _no_batch
