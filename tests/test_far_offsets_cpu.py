"""The entry points that take a capacity, asked for bytes they must refuse
before any device call: an offset and a length whose sum wraps 2^64 (offset
2^64 - 10, length 20), and one whose sum passes a capacity above 2^32 by a
single byte.  cdc_assemble_device, cdc_object_digests_device,
cdc_line_table_device, cdc_line_ids_device, cdc_diff_emit_device and
cdc_zip_pieces_device, each on every offset it takes; the pointers are made up
and never dereferenced.  The same arguments one byte shorter are valid: where no
device can run them they get as far as the library's state (CDC_E_NOT_INIT),
which shows that the refusals above are the bound's and nothing else's.
tests/test_far_offsets.py runs the valid side of these bounds on the device."""
import ctypes

import numpy as np

from plakar_amd import _lib, diff

CAP = 2 ** 32 + 1000          # a capacity past 32 bits
FAR = 2 ** 32 + 900           # FAR + 100 == CAP: the last byte that fits
WRAP_OFF, WRAP_LEN = 2 ** 64 - 10, 20
E = _lib.CDC_E_INVALID
SRC, DST, AUX = 1 << 40, 3 << 40, 5 << 40  # made-up device addresses, more than CAP apart


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


def _u64(*v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def _valid(status):
    """A call with valid arguments and made-up pointers: made only where no
    device can run it, and then it stops at the library's state."""
    assert status == _lib.CDC_E_NOT_INIT


def test_assemble_refuses_far_segments_past_either_capacity():
    L = _lib.lib()

    def call(src_off, ln, dst_off, src_cap=CAP, dst_cap=CAP):
        return L.cdc_assemble_device(0, ctypes.c_void_p(SRC), src_cap, _u64(0, src_off), _u64(50, ln), _u64(0, dst_off), 2,
                                     ctypes.c_void_p(DST), dst_cap, None)

    assert call(WRAP_OFF, WRAP_LEN, 100) == E, "src_off + len wraps"
    assert call(100, WRAP_LEN, WRAP_OFF) == E, "dst_off + len wraps"
    assert call(WRAP_OFF, WRAP_LEN, WRAP_OFF) == E
    assert call(WRAP_OFF, WRAP_LEN, 100, src_cap=2 ** 64 - 1, dst_cap=2 ** 64 - 1) == E, "whatever the capacity"
    assert call(FAR, 101, 100) == E, "one byte past src_cap"
    assert call(100, 101, FAR) == E, "one byte past dst_cap"
    assert call(FAR + 1, 100, 100) == E and call(100, 100, FAR + 1) == E
    assert call(CAP + 1, 0, 100) == E and call(100, 0, CAP + 1) == E, "an empty segment past the end"
    assert call(100, 2 ** 32 + 1, 100, src_cap=2 ** 32, dst_cap=2 ** 33) == E, "a length past src_cap alone"
    assert call(100, 2 ** 32 + 1, 100, src_cap=2 ** 33, dst_cap=2 ** 32) == E, "a length past dst_cap alone"
    if not _has_gpu():
        _valid(call(FAR, 100, FAR))
        _valid(call(0, CAP - 50, 50))  # one segment longer than 2^32


def test_object_digests_refuses_far_segments_past_the_data():
    L = _lib.lib()

    def call(off, ln, cap=CAP):
        return L.cdc_object_digests_device(0, ctypes.c_void_p(SRC), cap, _u64(0, off, 200), _u64(50, ln, 7), 3, _u64(0, 2, 3), 2,
                                           ctypes.c_void_p(DST), None)

    assert call(WRAP_OFF, WRAP_LEN) == E, "offset + length wraps"
    assert call(WRAP_OFF, WRAP_LEN, cap=2 ** 64 - 1) == E
    assert call(FAR, 101) == E, "one byte past the data"
    assert call(FAR + 1, 100) == E
    assert call(CAP + 1, 0) == E, "an empty segment past the end"
    if not _has_gpu():
        _valid(call(FAR, 100))


def test_line_table_refuses_far_texts_past_the_data():
    L = _lib.lib()
    counts, total = _u64(0, 0), ctypes.c_uint64()

    def call(off, ln, cap=CAP):
        return L.cdc_line_table_device(0, ctypes.c_void_p(SRC), cap, _u64(0, off), _u64(50, ln), 2, ctypes.c_void_p(DST), 1000,
                                       counts, ctypes.byref(total), None)

    assert call(WRAP_OFF, WRAP_LEN) == E, "offset + length wraps"
    assert call(WRAP_OFF, WRAP_LEN, cap=2 ** 64 - 1) == E
    assert call(FAR, 101) == E, "one byte past the data"
    assert call(FAR + 1, 100) == E
    assert call(CAP + 1, 0) == E, "an empty text past the end"
    if not _has_gpu():
        _valid(call(FAR, 100))


def test_line_ids_refuses_far_records_past_the_data():
    L = _lib.lib()
    ids, rounds = (ctypes.c_uint32 * 3)(), ctypes.c_uint32()

    def call(off, ln, cap=CAP):
        lines = np.zeros(3, dtype=diff.LINE_DTYPE)
        lines["off"], lines["len"] = [0, off, 20], [5, ln, 5]
        return L.cdc_line_ids_device(0, ctypes.c_void_p(SRC), cap, ctypes.c_void_p(lines.ctypes.data), 3, _u64(0, 2, 3), 2, 0,
                                     ids, ctypes.byref(rounds), None)

    assert call(WRAP_OFF, WRAP_LEN) == E, "offset + length wraps"
    assert call(WRAP_OFF, WRAP_LEN, cap=2 ** 64 - 1) == E
    assert call(FAR, 101) == E, "one byte past the data"
    assert call(FAR + 1, 100) == E
    assert call(CAP + 1, 0) == E, "an empty line past the end"
    if not _has_gpu():
        _valid(call(FAR, 100))


P, LIT, N = 0x100, 0x200, 0x400


def test_diff_emit_refuses_far_records_past_any_of_its_three_capacities():
    L = _lib.lib()

    def call(src_off, ln, dst_off, flags=0, plain_cap=CAP, lit_cap=CAP, dst_cap=CAP):
        er = np.zeros(2, dtype=diff.EMIT_DTYPE)
        er["src_off"], er["dst_off"], er["len"], er["flags"] = [0, src_off], [0, dst_off], [10, ln], [P | N | 43, flags]
        return L.cdc_diff_emit_device(0, ctypes.c_void_p(SRC), plain_cap, ctypes.c_void_p(AUX), lit_cap,
                                      ctypes.cast(er.ctypes.data, ctypes.POINTER(_lib.cdc_emit_rec)), 2, ctypes.c_void_p(DST),
                                      dst_cap, None)

    for flags in (0, LIT):
        assert call(WRAP_OFF, WRAP_LEN, 100, flags) == E, "src_off + len wraps"
        assert call(WRAP_OFF, WRAP_LEN, 100, flags, plain_cap=2 ** 64 - 1, lit_cap=2 ** 64 - 1) == E
        assert call(FAR, 101, 100, flags) == E, "one byte past the source"
        assert call(FAR + 1, 100, 100, flags) == E
        assert call(CAP + 1, 0, 100, flags | N) == E, "no bytes, from past the end"
        assert call(100, WRAP_LEN, WRAP_OFF, flags) == E, "dst_off + bytes wraps"
        assert call(100, 100, FAR + 1, flags) == E, "one byte past dst_cap"
        assert call(100, 99, FAR, flags | P | N) == E, "the prefix and the newline count: 101 bytes"
        assert call(100, 100, FAR, flags | N) == E
    assert call(FAR, 100, 100, 0, plain_cap=FAR + 99) == E and call(FAR, 100, 100, LIT, lit_cap=FAR + 99) == E
    assert call(100, 20, 2 ** 64 - 21, N, dst_cap=2 ** 64 - 1) == E, "dst_off + 21 is 2^64"
    if not _has_gpu():
        _valid(call(FAR, 100, FAR, 0, lit_cap=50))
        _valid(call(FAR, 100, FAR, LIT, plain_cap=50))
        _valid(call(FAR, 98, FAR, P | N | 45))


def test_zip_pieces_refuses_far_pieces_past_the_source():
    L = _lib.lib()
    outs = (_lib.cdc_zip_piece_out * 2)()
    total = ctypes.c_uint64()

    def call(off, ln, cap=CAP, level=0):
        pc = (_lib.cdc_zip_piece * 2)()
        for p, (o, n) in zip(pc, ((0, 50), (off, ln))):
            p.src_off, p.len, p.first, p.last, p.hdr_off, p.hdr_len, p.crc_reg = o, n, 1, 1, 0, 30, 0xFFFFFFFF
        args = (0, ctypes.c_void_p(SRC), cap, pc, 2, bytes(64), 64, ctypes.c_void_p(DST), 1 << 20, outs, ctypes.byref(total))
        if level:
            return L.cdc_zip_pieces_device_level(*args, level, None)
        return L.cdc_zip_pieces_device(*args, None)

    for level in (0, 1):
        assert call(WRAP_OFF, WRAP_LEN, level=level) == E, "offset + length wraps"
        assert call(WRAP_OFF, WRAP_LEN, cap=2 ** 64 - 1, level=level) == E
        assert call(FAR, 101, level=level) == E, "one byte past the source"
        assert call(FAR + 1, 100, level=level) == E
    if not _has_gpu():
        assert call(FAR, 100) == _lib.CDC_E_DEVICE  # valid: as far as the device there is not
