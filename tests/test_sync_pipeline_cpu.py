"""The sync pipeline's checks that need no GPU: the host planner under the
sanitizers (tests/c/sync_plan_check.cpp), the argument checks cdc_sync_new and
cdc_sync_run make before they touch a device, and the Python layer's.  A run
needs a context and a context needs cdc_init, so an unsorted `wanted` and a run
with no packfile registered are in tests/test_sync_pipeline.py."""
import ctypes
import os
import re
import subprocess

import pytest

from plakar_amd import _lib, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(64, 96))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("splan") / "sync_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "sync_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_planner_under_sanitizers(plan_check_exe):
    """The 33-byte search at the first, last and absent keys, 400 seeded row
    lists against the brute-force filter and cut, 300 splits: no sanitizer
    report and no wrong plan."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) row lists, (\d+) splits, ok", r.stdout)
    assert m and int(m.group(1)) == 400 and int(m.group(2)) == 300, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _opts():
    o = _lib.cdc_sync_opts()
    _lib.lib().cdc_sync_default_opts(ctypes.byref(o))
    return o


def test_default_opts():
    o = _opts()
    assert o.struct_size == ctypes.sizeof(_lib.cdc_sync_opts) and o.verify == 1
    assert (o.src.compress, o.src.key, o.dst.compress, o.dst.key) == (0, None, 0, None)
    assert (o.level, o.packfile_max, o.batch_bytes, o.readers, o.packers, o.timestamp, o.known, o.nknown) == \
        (0, 0, 0, 0, 0, 0, None, 0)
    _lib.lib().cdc_sync_default_opts(None)  # nothing to fill: no fault


def _rec(t, fill):
    return bytes([t]) + bytes([fill]) * 32


def test_new_checks_its_arguments_before_the_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    o = _opts()
    assert L.cdc_sync_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_sync_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    for device in (-1, 64):
        assert L.cdc_sync_new(device, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID and not h.value
    for field, bad in [("struct_size", 0), ("struct_size", o.struct_size - 8), ("struct_size", o.struct_size + 8),
                       ("level", 2), ("level", -1), ("level", 6), ("readers", -1), ("readers", 257), ("packers", -1),
                       ("packers", 257), ("nknown", 1)]:  # nknown without known
        keep = getattr(o, field)
        setattr(o, field, bad)
        assert L.cdc_sync_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID, (field, bad)
        assert not h.value
        setattr(o, field, keep)
    for side in ("src", "dst"):
        for bad in (3, -1, 7):
            getattr(o, side).compress = bad
            assert L.cdc_sync_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID, (side, bad)
            getattr(o, side).compress = 0
    # known: descending records, and records that differ in the type byte only
    for recs in (_rec(1, 9) + _rec(1, 8), _rec(2, 5) + _rec(1, 5), _rec(1, 1) + _rec(1, 3) + _rec(1, 2)):
        buf = ctypes.create_string_buffer(recs, len(recs))
        o.known, o.nknown = ctypes.cast(buf, ctypes.c_void_p), len(recs) // 33
        assert L.cdc_sync_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID and not h.value
    # sorted known (equal neighbours too) passes the checks: what comes next is the library's state
    recs = _rec(1, 5) + _rec(1, 5) + _rec(2, 5) + _rec(3, 0)
    buf = ctypes.create_string_buffer(recs, len(recs))
    o.known, o.nknown = ctypes.cast(buf, ctypes.c_void_p), 4
    st = L.cdc_sync_new(0, ctypes.byref(o), ctypes.byref(h))
    if _has_gpu():  # an earlier test of the run may have initialised the library
        assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
        L.cdc_sync_free(h)
    else:
        assert st == _lib.CDC_E_NOT_INIT and not h.value


def test_calls_on_no_context():
    L = _lib.lib()
    cb = _lib.BACKUP_PACK_FN(lambda ctx, data, n: 0)
    fb = _lib.SYNC_BLOB_FN(lambda ctx, t, c, s: None)
    st = _lib.cdc_sync_stats()
    st.struct_size = ctypes.sizeof(st)
    assert L.cdc_sync_run(None, None, 0, cb, fb, None, ctypes.byref(st)) == _lib.CDC_E_INVALID
    assert L.cdc_sync_add_packfile(None, b"x" * 52, 52) == _lib.CDC_E_INVALID
    assert L.cdc_sync_add_packfile_path(None, b"/nonexistent") == _lib.CDC_E_INVALID
    L.cdc_sync_free(None)


def test_python_layer_checks_keys_and_compression():
    with pytest.raises(ValueError):
        sync.SyncPipeline(src_compression="ZSTD")
    with pytest.raises(ValueError):
        sync.SyncPipeline(dst_compression="ZSTD")
    with pytest.raises(ValueError):
        sync.SyncPipeline(src_key=b"short")
    with pytest.raises(ValueError):
        sync.SyncPipeline(dst_key=KEY + b"x")
    with pytest.raises(ValueError):
        sync.SyncPipeline(level=2)
    with pytest.raises(ValueError):
        sync.SyncPipeline(known={(1, b"short")})
    with pytest.raises(ValueError):
        sync.sync_packfiles([], dst_compression="ZSTD")
    from plakar_amd import snapshot
    assert snapshot.SyncPipeline is sync.SyncPipeline and snapshot.sync_packfiles is sync.sync_packfiles
