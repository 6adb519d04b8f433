"""Compression level 9 (CDC_LEVEL_BEST: k_lz_seq_deep, four candidates per hash
bucket and a lazy parse), the checks that need no GPU: the two new entry
points (cdc_transcode_device_level, cdc_backup_run_level) are exported and
declared, every entry point that takes a level takes 9 and still refuses the
levels that do not exist, before any device is touched; the Python keywords;
and the compiler's resource report of the new kernel."""
import ctypes
import inspect
import os
import re

import pytest

from plakar_amd import _lib, archive, encode, snapshot, sync
from test_wide_cpu import LDS_MAX, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cdc_transcode_device_level", "cdc_backup_run_level"]
LEVEL_SYMBOLS = ["cdc_encode_device_level", "cdc_gzip_stream_set_level", "cdc_zip_pieces_device_level",
                 "cdc_archive_set_level", "cdc_backup_set_level"] + NEW_SYMBOLS
REFUSED = (2, -1, 6)


def _header():
    with open(os.path.join(ROOT, "include", "plakar_cdc.h")) as f:
        return f.read()


def test_new_entry_points_are_exported_and_declared():
    L, h = _lib.lib(), _header()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
        assert re.search(rf"\bint {name}\(", h), name
    assert re.search(r"#define CDC_LEVEL_BEST 9\b", h)
    assert re.search(r"#define CDC_LEVEL_FAST 0\b", h) and re.search(r"#define CDC_LEVEL_WIDE 1\b", h)
    assert _lib.CDC_LEVEL_BEST == 9
    assert h.count("compression/compression.go:12-51") >= len(LEVEL_SYMBOLS)
    assert L.cdc_abi_version() == 1


def _encode_args(level):
    offs, lens, oo = (ctypes.c_uint64 * 1)(), (ctypes.c_uint64 * 1)(1 << 31), (ctypes.c_uint64 * 2)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: the blob is too long, which is found after the level
    return [0, buf, offs, lens, 1, _lib.CDC_COMPRESS_GZIP, None, None, buf, 1 << 20, oo, level, None]


def test_level_9_passes_encode_and_zip_argument_checks():
    L = _lib.lib()
    # past the level check and on to the next one: a blob of 2 GiB is CDC_E_UNSUPPORTED, not CDC_E_INVALID
    for level in (0, 1, 9):
        assert L.cdc_encode_device_level(*_encode_args(level)) == _lib.CDC_E_UNSUPPORTED, level
    for level in REFUSED + (3, 8, 10):
        assert L.cdc_encode_device_level(*_encode_args(level)) == _lib.CDC_E_INVALID, level
    total = ctypes.c_uint64(7)
    assert L.cdc_zip_pieces_device_level(0, None, 0, None, 0, None, 0, None, 0, None, ctypes.byref(total), 9,
                                         None) == _lib.CDC_OK   # no pieces: nothing to do
    assert total.value == 0
    for level in REFUSED:
        assert L.cdc_zip_pieces_device_level(0, None, 0, None, 0, None, 0, None, 0, None, ctypes.byref(total), level,
                                             None) == _lib.CDC_E_INVALID


def test_level_9_is_set_on_a_gzip_stream():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_gzip_stream_new(0, ctypes.byref(h)) == _lib.CDC_OK   # touches no device
    try:
        assert L.cdc_gzip_stream_set_level(h, 9) == _lib.CDC_OK
        for level in REFUSED:
            assert L.cdc_gzip_stream_set_level(h, level) == _lib.CDC_E_INVALID
        assert L.cdc_gzip_stream_set_level(h, 1) == _lib.CDC_OK and L.cdc_gzip_stream_set_level(h, 9) == _lib.CDC_OK
    finally:
        L.cdc_gzip_stream_free(h)
    # the two session setters check the handle and the level together, before anything else
    assert L.cdc_archive_set_level(None, 9) == _lib.CDC_E_INVALID
    assert L.cdc_backup_set_level(None, 9) == _lib.CDC_E_INVALID


def test_sessions_take_level_9():
    """Without a device the native contexts cannot come up, and say so; with
    one they do, and 9 is set on them while 2, -1 and 6 are refused."""
    try:
        with snapshot.BackupSession(compression="GZIP", level=9) as s:
            for level in REFUSED:
                assert _lib.lib().cdc_backup_set_level(s._h, level) == _lib.CDC_E_INVALID
            assert _lib.lib().cdc_backup_set_level(s._h, 9) == _lib.CDC_OK
        with archive.ArchiveSession(level=9) as a:
            for level in REFUSED:
                assert _lib.lib().cdc_archive_set_level(a._h, level) == _lib.CDC_E_INVALID
            assert _lib.lib().cdc_archive_set_level(a._h, 9) == _lib.CDC_OK
    except _lib.CdcError as e:
        assert e.status in (_lib.CDC_E_NO_DEVICE, _lib.CDC_E_DEVICE, _lib.CDC_E_NOT_INIT)


def _transcode(level, **over):
    L = _lib.lib()
    one, oo, st = (ctypes.c_uint64 * 1)(16), (ctypes.c_uint64 * 2)(7, 7), (ctypes.c_int32 * 1)()
    zero = (ctypes.c_uint64 * 1)(0)
    src, dst = _lib.cdc_codec(_lib.CDC_COMPRESS_LZ4, None), _lib.cdc_codec(_lib.CDC_COMPRESS_GZIP, None)
    a = dict(device=0, d_in=ctypes.c_void_p(4096), offsets=zero, lens=one, n=0, src=ctypes.byref(src), dst=ctypes.byref(dst),
             checksums=None, random=None, d_out=ctypes.c_void_p(4096), out_cap=64, out_offsets=oo, status=st, level=level,
             stream=None)
    a.update(over)
    return L.cdc_transcode_device_level(*a.values()), oo


def test_transcode_level_is_checked_before_the_device():
    for level in REFUSED:
        assert _transcode(level)[0] == _lib.CDC_E_INVALID, level
        assert _transcode(level, n=1)[0] == _lib.CDC_E_INVALID, level
    for level in (0, 1, 9):
        # the level is fine: the next argument check speaks (a device outside 0..63, a NULL codec)
        assert _transcode(level, device=64)[0] == _lib.CDC_E_INVALID
        assert _transcode(level, src=None)[0] == _lib.CDC_E_INVALID
        rc, oo = _transcode(level)   # no blobs: CDC_OK with a library that is initialised, CDC_E_NOT_INIT before
        assert rc in (_lib.CDC_OK, _lib.CDC_E_NOT_INIT), level
        if rc == _lib.CDC_OK:
            assert oo[0] == 0


def test_backup_run_level_is_checked_before_anything_is_opened():
    L = _lib.lib()
    o = _lib.cdc_backup_opts()
    for level in REFUSED:
        # valid options and no files: only the level is wrong
        o.chunking = _lib.cdc_opts(4096, 16384, 65536, 0)
        assert L.cdc_backup_run_level(0, None, 0, ctypes.byref(o), _lib.BACKUP_FILE_FN(), _lib.BACKUP_PACK_FN(), None,
                                      None, level) == _lib.CDC_E_INVALID, level
    for level in (0, 1, 9):
        # the level is fine: the missing options are what is refused (cdc_backup_new's own check)
        assert L.cdc_backup_run_level(0, None, 0, None, _lib.BACKUP_FILE_FN(), _lib.BACKUP_PACK_FN(), None, None,
                                      level) == L.cdc_backup_run(0, None, 0, None, _lib.BACKUP_FILE_FN(),
                                                                 _lib.BACKUP_PACK_FN(), None, None) != _lib.CDC_OK


def test_python_layers_take_level_9():
    for fn in (sync.transcode_device, sync.transcode_blobs, sync.SyncSession.__init__, encode.encode_device,
               encode.encode_blobs, snapshot.BackupSession.__init__, snapshot.backup_files, archive.GzipStream.__init__,
               archive.ArchiveSession.__init__, archive.ZipSession.__init__):
        assert inspect.signature(fn).parameters["level"].default == 0, fn.__qualname__
    assert [_lib.level_code(v) for v in (0, 1, 9)] == [0, 1, 9]
    assert _lib.level_code(9) == 9
    assert encode.DeviceEncoder(compression="GZIP", level=9).level == 9
    assert sync.SyncSession(dst_compression="GZIP", level=9).level == 9 and sync.SyncSession().level == 0
    for bad in (2, -1, "9", None, True, 9.0, 6, 3):
        with pytest.raises(ValueError):
            _lib.level_code(bad)
        with pytest.raises(ValueError):
            sync.SyncSession(level=bad)
        with pytest.raises(ValueError):
            sync.transcode_blobs([b"x"], level=bad)
        with pytest.raises(ValueError):
            snapshot.backup_files([], level=bad)


def test_deep_kernel_resources():
    """no scratch, no spills, and an LDS size that lets two
    workgroups share a CU's 160 KiB, the window (40,960 + 16 bytes) and a
    table of 32 KiB."""
    name = "k_lz_seq_deep"
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3enc{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) == 0
    lds = int(k["LDS Size [bytes/block]"])
    assert 40960 + 16 + 32768 <= lds and 2 * lds <= LDS_MAX, "two workgroups per CU"
    assert int(k["VGPRs"]) <= 128, "the registers allow more waves than the LDS does"
