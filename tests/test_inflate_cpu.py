"""GZIP Decode's checks that need no GPU: the shared gzip / DEFLATE walker
passes the sanitizer program (its own fixtures, 20,000 single-bit mutations
judged by zlib, and every stream the GPU tests use, each held against
inflate_ref), the entry points take the selector and still reject bad
arguments before touching the device, the Python layers accept "GZIP", and
the compiler's resource report of the two new kernels stays within bounds."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import pytest

import inflate_ref as ir
from plakar_amd import _lib, build, decode, restore, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIVATE_MAX = 256       # bytes per lane
LDS_MAX = 163_840       # one CU's LDS


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate") / "inflate_host_fuzz")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "c", "inflate_host_fuzz.cpp"),
           "-l:libz.so.1"]
    subprocess.run(cmd, check=True)
    return exe


def test_walker_under_sanitizers(fuzz_exe, tmp_path):
    """The stand-alone program: no sanitizer report, no acceptance that zlib
    refuses, equal bytes where both accept; and for every stream of the GPU
    tests the status and the bytes that inflate_ref gives."""
    streams = ir.all_streams()
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
    r = subprocess.run([fuzz_exe, "--streams", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) accepted, (\d+) rejected, ok", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = re.findall(r"^S (\d+) (-?\d+) (\d+) ([0-9a-f]{8})$", r.stdout, re.M)
    assert len(rows) == len(streams)
    for (i, st, size, crc), s in zip(rows, streams):
        want_st, want = ir.status_of(s)
        want = want or b""
        assert (int(st), int(size), int(crc, 16)) == (want_st, len(want), zlib.crc32(want)), f"stream {i}"


def _args(n=1):
    return (ctypes.c_uint64 * max(n, 1))()


def test_selector_constants():
    assert (_lib.CDC_COMPRESS_NONE, _lib.CDC_COMPRESS_LZ4, _lib.CDC_COMPRESS_GZIP) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "plakar_cdc.h")) as f:
        h = f.read()
    for name, v in (("NONE", 0), ("LZ4", 1), ("GZIP", 2)):
        assert re.search(rf"#define\s+CDC_COMPRESS_{name}\s+{v}\b", h), name
    assert _lib.compress_code("GZIP") == 2 and _lib.compress_code("LZ4") == 1 and _lib.compress_code(None) == 0


def test_gzip_decode_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, oo, st = _args(), _args(), _args(2), (ctypes.c_int32 * 1)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: every call below fails on its arguments
    good = dict(device=0, d_in=buf, offsets=offs, lens=lens, n=1, compressed=_lib.CDC_COMPRESS_GZIP, key=None,
                d_out=buf, out_cap=16, out_offsets=oo, status=st, stream=None)
    order = list(good)
    for name, bad in [("d_in", None), ("offsets", None), ("lens", None), ("status", None), ("out_offsets", None),
                      ("d_out", None), ("device", -1), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_decode_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name


def test_gzip_check_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, st = _args(), _args(), (ctypes.c_int32 * 1)()
    buf = ctypes.c_void_p(4096)
    good = dict(device=0, d_in=buf, offsets=offs, lens=lens, n=1, compressed=_lib.CDC_COMPRESS_GZIP, key=None,
                checksums=bytes(32), d_scratch=buf, scratch_cap=16, needed=None, status=st, stream=None)
    order = list(good)
    for name, bad in [("d_in", None), ("offsets", None), ("lens", None), ("status", None), ("checksums", None),
                      ("d_scratch", None), ("device", -1), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_check_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name


def test_python_layers_take_gzip_and_refuse_other_names():
    d = decode.DeviceDecoder(compression="GZIP")
    assert d.compressed == "GZIP" and decode._sel(d.compressed) == _lib.CDC_COMPRESS_GZIP
    assert decode.DeviceDecoder(compression="LZ4").compressed is True
    assert decode.DeviceDecoder(compression=None).compressed is False
    assert (decode._sel(True), decode._sel(False), decode._sel("GZIP")) == (1, 0, 2)
    with pytest.raises(ValueError):
        decode.DeviceDecoder(compression="ZSTD")
    with pytest.raises(ValueError):
        decode._sel("ZSTD")
    with pytest.raises(ValueError):
        restore.RestoreSession(compression="ZSTD")
    with pytest.raises(ValueError):
        snapshot.restore_files([], [], compression="ZSTD")


def test_restore_session_constructs_for_gzip():
    """The name passes the configuration check (it was a ValueError before);
    without a device the native context then cannot come up, and says so."""
    try:
        with restore.RestoreSession(compression="GZIP", key=bytes(32)) as s:
            assert s._h
    except _lib.CdcError as e:
        assert e.status in (_lib.CDC_E_NO_DEVICE, _lib.CDC_E_DEVICE, _lib.CDC_E_NOT_INIT)


def _report():
    path = build.resources_path()
    assert os.path.exists(path), f"{path} is absent: build the library with plakar_amd.build"
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
            if not m:
                continue
            key, _, val = m.group(1).partition(":")
            if key.strip() == "Function Name":
                cur = out.setdefault(val.strip(), {})
            elif cur is not None:
                cur[key.strip()] = val.strip()
    return out


@pytest.mark.parametrize("name", ["k_gz_size", "k_gz_emit"])
def test_gzip_kernel_resources(name):
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3dec{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["VGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) < PRIVATE_MAX
    assert int(k["LDS Size [bytes/block]"]) <= LDS_MAX
