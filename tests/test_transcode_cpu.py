"""Transcode's checks that need no GPU: the host planner under the sanitizers
(tests/c/transcode_plan_check.cpp), cdc_transcode_size against streams sealed
by libcrypto (decode_ref.seal_stream), the argument checks cdc_transcode_device
makes before it touches a device, and the compiler's resource report of
k_rekey."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import decode_ref as dr
from plakar_amd import _lib, build, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(64, 96))

# k_rekey's occupancy: eight waves per workgroup and one workgroup per CU, so
# two waves per SIMD.  Its LDS sets that: the 64-KiB T-table and two key sets
# and a stage per wave come to 65,536 + 8 x 11,712 = 159,232 bytes of the CU's
# 163,840; twelve waves (k_gcm's three per SIMD) would need 206,080.
REKEY_WAVES_PER_SIMD = 2
REKEY_LDS_BYTES = 65536 + 8 * 11712
CU_LDS_BYTES = 160 * 1024


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tplan") / "transcode_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "transcode_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_planner_under_sanitizers(plan_check_exe):
    """Every length around a record edge, the four key combinations, a mixed
    batch, the record-count refusal and 3,000 random batches: no sanitizer
    report and no wrong plan."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) lengths, (\d+) batches, ok", r.stdout)
    assert m and int(m.group(1)) == 17 and int(m.group(2)) == 3000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.parametrize("size", [0, 1, 65535, 65536, 65537, 131073])
def test_transcode_size_against_sealed_streams(size):
    stream = dr.seal_stream(KEY, dr.rnd(size, 300 + size % 7), 310)
    assert sync.transcode_size(len(stream), True, True) == len(stream)
    assert sync.transcode_size(len(stream), True, False) == size
    assert sync.transcode_size(size, False, True) == len(stream)
    assert sync.transcode_size(size, False, False) == size


def test_transcode_size_refuses_lengths_no_writer_produces():
    L = _lib.lib()
    for n in (0, 59, 61, 60 + 12, 60 + 27, 60 + 65564 + 12, 60 + 65564 + 27, 60 + 65580):
        assert L.cdc_transcode_size(n, 1, 1) == _lib.CDC_E_CORRUPT, n
        assert L.cdc_transcode_size(n, 1, 0) == _lib.CDC_E_CORRUPT, n
        with pytest.raises(_lib.CdcError):
            sync.transcode_size(n, True, False)
    assert L.cdc_transcode_size(60 + 28, 1, 1) == 88 and L.cdc_transcode_size(60 + 28, 1, 0) == 0
    assert L.cdc_transcode_size(60 + 65564 + 28, 1, 0) == 65536
    assert L.cdc_transcode_size(60 + 65580 + 12, 1, 0) == 65536 and L.cdc_transcode_size(60 + 65580 + 28, 1, 0) == 65552


def _call(L, **kw):
    one = (ctypes.c_uint64 * 1)(60)
    zero = (ctypes.c_uint64 * 1)(0)
    a = dict(device=0, d_in=ctypes.c_void_p(4096), offsets=zero, lens=one, n=1,
             src=ctypes.byref(_lib.cdc_codec(1, KEY)), dst=ctypes.byref(_lib.cdc_codec(1, KEY)), checksums=None,
             random=bytes(56), d_out=ctypes.c_void_p(8192), out_cap=60, oo=(ctypes.c_uint64 * 2)(),
             status=(ctypes.c_int32 * 1)(), stream=None)
    a.update(kw)
    return L.cdc_transcode_device(a["device"], a["d_in"], a["offsets"], a["lens"], a["n"], a["src"], a["dst"],
                                  a["checksums"], a["random"], a["d_out"], a["out_cap"], a["oo"], a["status"],
                                  a["stream"])


def test_argument_checks_come_before_the_device():
    L = _lib.lib()
    for bad in (dict(device=-1), dict(device=64), dict(d_in=None), dict(offsets=None), dict(lens=None),
                dict(src=None), dict(dst=None), dict(oo=None), dict(status=None), dict(d_out=None),
                dict(random=None)):
        assert _call(L, **bad) == _lib.CDC_E_INVALID, bad
    # random is only needed with a destination key; d_out may be NULL for out_cap = 0
    # (empty batches: nothing here may reach a device with these made-up pointers)
    plain = ctypes.byref(_lib.cdc_codec(1, None))
    ok = (_lib.CDC_OK, _lib.CDC_E_NOT_INIT)
    assert _call(L, n=0, dst=plain, random=None) in ok
    assert _call(L, n=0, d_out=None, out_cap=0) in ok
    assert _call(L, n=0, d_in=None, offsets=None, lens=None, status=None) in ok


def test_without_cdc_init_it_fails_loudly():
    L = _lib.lib()
    st = _call(L, n=0)
    if _has_gpu():  # an earlier test of the run may have initialised the library
        assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
    else:
        assert st == _lib.CDC_E_NOT_INIT
        assert _call(L) == _lib.CDC_E_NOT_INIT
        assert L.cdc_strerror(st).decode() == "cdc_init() has not been called"


def test_python_layer_checks_keys_compression_and_shapes():
    with pytest.raises(ValueError):
        sync.SyncSession(src_key=b"short")
    with pytest.raises(ValueError):
        sync.SyncSession(dst_compression="ZSTD")
    assert sync.path_of((KEY, "LZ4"), (KEY, "LZ4")) == "rekey"
    assert sync.path_of((KEY, "GZIP"), (None, "GZIP")) == "open"
    assert sync.path_of((None, None), (KEY, None)) == "seal"
    assert sync.path_of((None, "LZ4"), (None, "LZ4")) == "copy"
    assert sync.path_of((KEY, "LZ4"), (KEY, "GZIP")) == "reencode"
    assert sync.SyncSession(src_key=KEY, dst_key=KEY).path == "rekey"
    with pytest.raises(_lib.CdcError):
        sync.SyncSession().add_packfile(b"not a packfile")
    assert np.dtype(np.uint8).itemsize == ctypes.sizeof(ctypes.c_uint8)
    assert ctypes.sizeof(_lib.cdc_codec) == 16


def _kernels():
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


def test_rekey_kernel_resources():
    """No spills and no private memory (both keystreams and both GHASH sums
    stay in vector registers), and an LDS footprint that fits one CU at the
    occupancy chosen above."""
    ks = _kernels()
    name = "_ZN2tc7k_rekeyENS_6RBatchE"
    assert name in ks, sorted(k for k in ks if "tc" in k)
    k = ks[name]
    assert int(k["VGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) == 0
    assert int(k["LDS Size [bytes/block]"]) <= CU_LDS_BYTES
    assert int(k["LDS Size [bytes/block]"]) == REKEY_LDS_BYTES
    assert int(k["Occupancy [waves/SIMD]"]) == REKEY_WAVES_PER_SIMD
    # the registers two waves per SIMD leave a wave: 512 / 2
    assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 256
