"""Restore's checks that need no GPU: the packfile index reader against the
packfile.go restatement (tests/packfile_ref.py) and the native packer, the
argument checks that every restore entry point makes before it touches the
device, and the stand-alone sanitizer program over the index reader and the
batch planner (tests/c/restore_plan_check.cpp)."""
import ctypes
import os
import random
import re
import struct
import subprocess

import pytest

import packfile_ref as pf
from plakar_amd import _lib, packer, restore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


def _random_packfile(rng, count, timestamp):
    p = pf.PackFile(timestamp)
    for _ in range(count):
        n = 0 if rng.random() < 0.25 else rng.randrange(1, 300)
        p.add_blob(rng.choice([1, 1, 2, 3]), rng.randbytes(32), rng.randbytes(n))
    return p


@pytest.mark.parametrize("count", [0, 1, 5, 300])
def test_index_reader_matches_packfile_ref(count):
    rng = random.Random(1000 + count)
    p = _random_packfile(rng, count, timestamp=rng.randrange(-2 ** 40, 2 ** 40))
    raw = p.serialize()
    footer, rows = restore.packfile_index(raw)
    want = pf.parse(raw)
    assert rows == want.index == p.index and len(rows) == count
    assert footer == dict(version=100, timestamp=p.timestamp, count=count, index_offset=len(p.blobs),
                          index_checksum=want.index_checksum)
    if count:
        assert any(n == 0 for _, _, _, n in rows) or count == 1  # zero-length blobs are in the mix


def test_index_reader_nospace_reports_the_count_and_the_first_rows():
    p = _random_packfile(random.Random(5), 9, 3)
    raw = p.serialize()
    f, need = _lib.cdc_packfile_footer(), ctypes.c_uint64()
    rows = (_lib.cdc_packfile_row * 4)()
    L = _lib.lib()
    assert L.cdc_packfile_index(raw, len(raw), ctypes.byref(f), rows, 4, ctypes.byref(need)) == _lib.CDC_E_NOSPACE
    assert need.value == 9 and f.count == 9
    assert [(r.type, bytes(r.checksum), r.offset, r.length) for r in rows] == p.index[:4]
    assert L.cdc_packfile_index(raw, len(raw), ctypes.byref(f), None, 0, None) == _lib.CDC_E_NOSPACE
    assert L.cdc_packfile_index(raw, len(raw), None, None, 0, None) == _lib.CDC_E_INVALID
    assert L.cdc_packfile_index(None, 10, ctypes.byref(f), None, 0, None) == _lib.CDC_E_INVALID
    assert L.cdc_packfile_index(raw, len(raw), ctypes.byref(f), None, 4, None) == _lib.CDC_E_INVALID


def _status(raw):
    f = _lib.cdc_packfile_footer()
    rows = (_lib.cdc_packfile_row * 16)()
    return _lib.lib().cdc_packfile_index(bytes(raw), len(raw), ctypes.byref(f), rows, 16, None)


def test_index_reader_rejects_every_malformed_form():
    p = _random_packfile(random.Random(7), 6, 42)
    raw = p.serialize()
    data_len = len(p.blobs)
    assert _status(raw) == 0
    for n in (0, 1, 51):                                    # shorter than a footer
        assert _status(raw[len(raw) - n:]) == _lib.CDC_E_CORRUPT, n
    assert _status(raw[:data_len] + b"\0" + raw[data_len:]) == _lib.CDC_E_CORRUPT   # index not 41 * count
    assert _status(raw[:data_len] + raw[data_len + 41:]) == _lib.CDC_E_CORRUPT      # a row short of count
    bad = bytearray(raw)
    struct.pack_into("<I", bad, len(raw) - 52, 101)          # version
    assert _status(bad) == _lib.CDC_E_CORRUPT
    q = pf.PackFile(42)                                      # an entry one byte past the index offset
    q.blobs, q.index, q.count, q.index_offset = p.blobs, list(p.index), p.count, p.index_offset
    t, c, o, n = q.index[-1]
    q.index[-1] = (t, c, o, n + 1)
    assert _status(q.serialize()) == _lib.CDC_E_CORRUPT
    q.index[-1] = (t, c, 0xFFFFFFFF, 2)                      # offset + length wraps 32 bits
    assert _status(q.serialize()) == _lib.CDC_E_CORRUPT
    bad = bytearray(raw)
    bad[data_len + 5] ^= 1                                   # the index no longer hashes to the footer's checksum
    assert _status(bad) == _lib.CDC_E_CORRUPT
    bad = bytearray(raw)
    bad[-1] ^= 1
    assert _status(bad) == _lib.CDC_E_CORRUPT
    with pytest.raises(_lib.CdcError) as e:
        restore.packfile_index(bytes(bad))
    assert e.value.status == _lib.CDC_E_CORRUPT


def test_native_packer_output_parses_to_the_rows_added():
    rng = random.Random(11)
    added = []
    pk = packer.Packer(1 << 20, 77)
    for i in range(40):
        data = rng.randbytes(0 if i % 7 == 0 else rng.randrange(1, 5000))
        csum = rng.randbytes(32)
        added.append((packer.TYPE_CHUNK, csum, data))
        pk.AddBlob(packer.TYPE_CHUNK, csum, data)
    raw = pk.Serialize()
    pk.close()
    footer, rows = restore.packfile_index(raw)
    assert footer["version"] == 100 and footer["timestamp"] == 77 and footer["count"] == 40
    assert [(t, c) for t, c, _, _ in rows] == [(t, c) for t, c, _ in added]
    for (_, _, o, n), (_, _, data) in zip(rows, added):
        assert raw[o:o + n] == data
    assert footer["index_offset"] == sum(len(d) for _, _, d in added)


def _u64(*v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def test_assemble_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    src, dst = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)  # never dereferenced
    good = dict(device=0, d_src=src, src_cap=4096, src_off=_u64(0, 100), len=_u64(100, 50), dst_off=_u64(10, 110),
                n=2, d_dst=dst, dst_cap=4096, stream=None)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return L.cdc_assemble_device(*[a[k] for k in order])

    for name, bad in [("src_off", None), ("len", None), ("dst_off", None), ("d_src", None), ("d_dst", None),
                      ("device", -1), ("device", 64)]:
        assert call(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert call(dst_off=_u64(10, 109)) == _lib.CDC_E_INVALID          # overlapping destinations
    assert call(dst_off=_u64(200, 10)) == _lib.CDC_E_INVALID          # unsorted
    assert call(dst_off=_u64(10, 4047)) == _lib.CDC_E_INVALID         # a segment past dst_cap
    assert call(dst_off=_u64(10, 2 ** 64 - 20)) == _lib.CDC_E_INVALID  # ... whose end wraps
    assert call(src_off=_u64(0, 4047)) == _lib.CDC_E_INVALID          # a segment past src_cap
    assert call(d_dst=ctypes.c_void_p((1 << 20) + 4095)) == _lib.CDC_E_INVALID  # source and destination alias
    # Valid arguments get as far as the library's state.  Segments without
    # bytes never reach the device, so that call is safe wherever it runs;
    # the one with bytes and made-up pointers only where no device can run it.
    assert call(len=_u64(0, 0)) in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
    if not _has_gpu():
        assert call(len=_u64(0, 0)) == _lib.CDC_E_NOT_INIT
        assert call() == _lib.CDC_E_NOT_INIT
    assert L.cdc_debug_set_assemble_policy(4) == _lib.CDC_E_INVALID
    assert L.cdc_debug_set_assemble_policy(2) == 0


def test_restore_context_argument_checks_without_a_device():
    L = _lib.lib()
    o = _lib.cdc_restore_opts()
    L.cdc_restore_default_opts(ctypes.byref(o))
    assert (o.verify, o.compress, o.writers, o.batch_bytes, o.key) == (1, 0, 0, 0, None)
    h = ctypes.c_void_p()
    assert L.cdc_restore_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_restore_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    assert L.cdc_restore_new(-1, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    o.writers = -1
    assert L.cdc_restore_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    o.writers = 0
    st = L.cdc_restore_new(0, ctypes.byref(o), ctypes.byref(h))
    if _has_gpu():  # an earlier test of the run may have initialised the library
        assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
        L.cdc_restore_free(h)
    else:
        assert st == _lib.CDC_E_NOT_INIT and not h.value
    f =(_lib.cdc_restore_file * 1)()
    cb = _lib.RESTORE_FILE_FN(lambda ctx, r: None)
    assert L.cdc_restore_files(None, f, 1, cb, None, None) == _lib.CDC_E_INVALID
    assert L.cdc_restore_add_packfile(None, b"x", 1) == _lib.CDC_E_INVALID
    assert L.cdc_restore_add_packfile_path(None, b"/nonexistent") == _lib.CDC_E_INVALID
    L.cdc_restore_free(None)
    assert _lib.CDC_E_NOTFOUND == -15 and L.cdc_strerror(-15).decode() != "unknown status"


def test_python_layer_checks_key_and_compression():
    with pytest.raises(ValueError):
        restore.RestoreSession(key=b"short")
    with pytest.raises(ValueError):
        restore.RestoreSession(compression="ZSTD")


def test_assemble_kernel_resources():
    """The compiler's report of k_assemble (every cache-policy instance): no
    spills and no private memory, so the Job descriptor stays in scalar
    registers and the copy loop in vector registers."""
    from plakar_amd import build
    path = build.resources_path()
    assert os.path.exists(path), f"{path} is absent: build the library with plakar_amd.build"
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
            if not m:
                continue
            k, _, v = m.group(1).partition(":")
            if k.strip() == "Function Name":
                cur = out.setdefault(v.strip(), {})
            elif cur is not None:
                cur[k.strip()] = v.strip()
    ks = {k: v for k, v in out.items() if k.startswith("_ZN4asmb10k_assembleILi")}
    assert len(ks) == 4, sorted(ks)
    for name, k in ks.items():
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, name
        assert int(k["ScratchSize [bytes/lane]"]) == 0, name
        assert int(k["VGPRs"]) <= 64, name


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rplan") / "restore_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "restore_plan_check.cpp"),
           os.path.join(ROOT, "plakar_amd", "csrc", "cdc_sha256.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_index_reader_and_planner_under_sanitizers(plan_check_exe):
    """The stand-alone program: valid packfiles parse back, every reject case,
    20,000 mutations in exactly-sized heap buffers, 3,000 random plans; no
    sanitizer report and no broken promise."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) accepted, (\d+) rejected, (\d+) plans, ok", r.stdout)
    assert m and int(m.group(1)) > 500 and int(m.group(2)) > 5000 and int(m.group(3)) == 3000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
