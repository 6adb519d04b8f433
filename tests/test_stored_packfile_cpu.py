"""The stored packfile form's checks that need no GPU: the layout planner
(plakar_amd/csrc/stored_plan.h) against a brute-force restatement under the
sanitizers (tests/c/stored_plan_check.cpp), the argument checks the new entry
points make before they touch a device, the ctypes table, and the reference
writer and reader of tests/stored_ref.py against each other."""
import ctypes
import os
import re
import subprocess

import pytest

import packfile_ref as pf
import stored_ref as sr
from plakar_amd import _lib, packer, restore, snapshot, stored, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cdc_packfile_index_stored", "cdc_packer_stored_bound", "cdc_packer_serialize_stored",
               "cdc_backup_set_packfile_form", "cdc_sync_set_packfile_form"] + \
              [f"cdc_{c}_add_packfiles" for c in ("restore", "check", "diff", "archive", "sync")]


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stplan") / "stored_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "stored_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_planner_under_sanitizers(plan_check_exe):
    """Every file length 0..300 with every last byte, 10,000 random trailers,
    the index ranges around every expansion bound, the writer's trailer read
    back: the planner agrees with the brute-force restatement and reads nothing
    it was not given."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) accepted, (\d+) rejected, (\d+) ranges, ok", r.stdout)
    assert m, r.stdout
    accepted, rejected, ranges = (int(g) for g in m.groups())
    assert accepted + rejected == 301 * 256 * 3 * 2 + 10000 and accepted > 50000 and ranges > 30000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_lib_exports_the_new_symbols():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "plakar_cdc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
        assert re.search(r"\b%s\(" % name, header), name
    assert (_lib.PACKFILE_PLAIN, _lib.PACKFILE_STORED, _lib.PACKFILE_ROWS) == (0, 1, 2)
    for name, value in (("PLAIN", 0), ("STORED", 1), ("ROWS", 2)):
        assert re.search(r"#define CDC_PACKFILE_%s\s+%d\b" % (name, value), header)
    assert "#define CDC_ABI_VERSION 1\n" in header and L.cdc_abi_version() == 1
    # the struct is the header's: two pointers, a length, a form, the rows and their count
    assert ctypes.sizeof(_lib.cdc_packfile_src) == 48
    assert [(n, getattr(_lib.cdc_packfile_src, n).offset) for n, _ in _lib.cdc_packfile_src._fields_] == \
           [("bytes", 0), ("len", 8), ("path", 16), ("form", 24), ("rows", 32), ("nrows", 40)]


def test_calls_on_no_context_are_invalid():
    L = _lib.lib()
    src = (_lib.cdc_packfile_src * 1)()
    buf = ctypes.create_string_buffer(b"x" * 64, 64)
    src[0].bytes, src[0].len, src[0].form = ctypes.cast(buf, ctypes.c_void_p), 64, _lib.PACKFILE_STORED
    status = (ctypes.c_int32 * 1)(7)
    for c in ("restore", "check", "diff", "archive", "sync"):
        assert getattr(L, f"cdc_{c}_add_packfiles")(None, src, 1, status) == _lib.CDC_E_INVALID, c
    assert status[0] == 7
    assert L.cdc_backup_set_packfile_form(None, _lib.PACKFILE_STORED) == _lib.CDC_E_INVALID
    assert L.cdc_sync_set_packfile_form(None, _lib.PACKFILE_STORED) == _lib.CDC_E_INVALID
    f, need = _lib.cdc_packfile_footer(), ctypes.c_uint64(5)
    data = b"y" * 100
    rows = (_lib.cdc_packfile_row * 1)()
    # cdc_packfile_index_stored: no footer, rows missing for a capacity, bytes missing for a length, devices outside 0..63
    assert L.cdc_packfile_index_stored(0, data, len(data), 0, None, None, rows, 1, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_packfile_index_stored(0, data, len(data), 0, None, ctypes.byref(f), None, 1, None) == _lib.CDC_E_INVALID
    assert L.cdc_packfile_index_stored(0, None, 10, 0, None, ctypes.byref(f), None, 0, None) == _lib.CDC_E_INVALID
    for device in (-1, 64):
        assert L.cdc_packfile_index_stored(device, data, len(data), 0, None, ctypes.byref(f), None, 0,
                                           None) == _lib.CDC_E_INVALID
    # cdc_packer_serialize_stored: no packer, no length, devices outside 0..63
    pk = packer.Packer(timestamp=1)
    ln = ctypes.c_uint64()
    out = (ctypes.c_uint8 * 256)()
    assert L.cdc_packer_serialize_stored(None, 1, 0, 0, None, None, out, 256, ctypes.byref(ln)) == _lib.CDC_E_INVALID
    assert L.cdc_packer_serialize_stored(pk._h, 1, 0, 0, None, None, out, 256, None) == _lib.CDC_E_INVALID
    for device in (-1, 64):
        assert L.cdc_packer_serialize_stored(pk._h, 1, device, 0, None, None, out, 256,
                                             ctypes.byref(ln)) == _lib.CDC_E_INVALID
    assert L.cdc_packer_stored_bound(None, 0, 0) == 0
    # the bound: the data, both encodings' bounds, five bytes
    pk.AddBlob(1, b"\1" * 32, b"abc")
    for comp in (0, 1, 2):
        for enc in (0, 1):
            assert L.cdc_packer_stored_bound(pk._h, comp, enc) == \
                3 + L.cdc_encode_bound(41, comp, enc) + L.cdc_encode_bound(52, comp, enc) + 5
    pk.close()


def test_python_layer_checks_its_arguments():
    with pytest.raises(ValueError):
        _lib.packfile_form_code("rows")
    with pytest.raises(ValueError):
        _lib.packfile_form_code(None)
    assert _lib.packfile_form_code("plain") == 0 and _lib.packfile_form_code("stored") == 1
    with pytest.raises(ValueError):
        stored.packfile_index_stored(b"x" * 100, key=b"short")
    with pytest.raises(ValueError):
        stored.packfile_index_stored(b"x" * 100, compression="ZSTD")
    with pytest.raises(ValueError):
        stored.sources([b"a", b"b"], rows=[[]])  # one list of rows per packfile
    with pytest.raises(ValueError):
        stored.sources([b"a"], form="rows")
    with pytest.raises(ValueError):
        stored.sources([b"a"], rows=[[(1, b"short", 0, 0)]])
    arr, n, keep, temp = stored.sources([b"abc", "/some/path"], rows=[[(1, b"\7" * 32, 0, 3)], []])
    assert n == 2 and arr[0].len == 3 and arr[0].form == arr[1].form == _lib.PACKFILE_ROWS
    assert arr[0].nrows == 1 and arr[0].rows[0].length == 3 and bytes(arr[0].rows[0].checksum) == b"\7" * 32
    assert arr[1].path == b"/some/path" and not arr[1].bytes and arr[1].nrows == 0 and len(keep) == 1
    pk = packer.Packer(timestamp=1)
    with pytest.raises(ValueError):
        pk.PutPackfileBytes(device=0, key=b"short")
    with pytest.raises(ValueError):
        pk.PutPackfileBytes(device=0, random=b"r" * 56)
    with pytest.raises(ValueError):
        pk.PutPackfileBytes(device=0, compression="ZSTD")
    pk.close()
    assert restore.packfile_index_stored is stored.packfile_index_stored
    for fn in (snapshot.restore_files, snapshot.read_ranges, snapshot.check_files, snapshot.diff_files,
               sync.sync_packfiles, snapshot.backup_files):
        assert "packfile_form" in fn.__code__.co_varnames[:fn.__code__.co_argcount], fn.__name__


@pytest.mark.parametrize("cfg", sr.CONFIGS, ids=sr.config_id)
def test_reference_writer_and_reader_agree(cfg):
    """tests/stored_ref.py on its own: what its writer makes, its reader (and
    packfile_ref's packer) gets back, and the trailer is the layout's."""
    comp, key = cfg[0], (sr.KEY if cfg[1] else None)
    for p in (sr.small_packfile(), sr.wide_packfile()):
        s = sr.write(p, comp, key)
        q, enc_index, enc_footer = sr.read(s, comp, key)
        assert q.index == p.index and bytes(q.blobs) == bytes(p.blobs) and q.timestamp == p.timestamp
        assert s[-1] == len(enc_footer) and s[-5:-1] == b"\x64\0\0\0"
        assert len(s) == len(p.blobs) + len(enc_index) + len(enc_footer) + 5
        assert sr.decode(enc_footer, comp, key) == p.serialize_footer()
        if key:
            with pytest.raises(Exception):
                sr.read(s, comp, sr.KEY_B)
        # the plain reader takes the plain form only
        assert pf.parse(p.serialize()).index == p.index
