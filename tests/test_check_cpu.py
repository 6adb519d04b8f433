"""Check's tests that need no GPU: the argument checks every new entry point
makes before it touches the device, the defaults, the Python layer's
ValueErrors, k_object_digest's line in the compiler's resource report, and the
stand-alone sanitizer program over the run and seam planner, the SHA-256 block
arithmetic and the split rule (tests/c/check_plan_check.cpp)."""
import ctypes
import os
import re
import subprocess

import pytest

from plakar_amd import _lib, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


def _u64(*v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def test_object_digests_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    data, dig = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)  # never dereferenced
    good = dict(device=0, d_data=data, len=4096, seg_off=_u64(0, 100, 4000), seg_len=_u64(100, 50, 96), nsegs=3,
                obj_seg0=_u64(0, 2, 3), n=2, d_digests=dig, stream=None)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return L.cdc_object_digests_device(*[a[k] for k in order])

    for name, bad in [("seg_off", None), ("seg_len", None), ("obj_seg0", None), ("d_data", None), ("d_digests", None),
                      ("device", -1), ("device", 64)]:
        assert call(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert call(seg_len=_u64(100, 50, 97)) == _lib.CDC_E_INVALID            # a segment one byte past the end
    assert call(seg_off=_u64(0, 4097, 4000)) == _lib.CDC_E_INVALID          # an offset past the end
    assert call(seg_len=_u64(100, 2 ** 64 - 50, 96)) == _lib.CDC_E_INVALID  # offset + length wraps
    assert call(obj_seg0=_u64(0, 2, 2)) == _lib.CDC_E_INVALID               # does not reach nsegs
    assert call(obj_seg0=_u64(0, 2, 4)) == _lib.CDC_E_INVALID               # passes nsegs
    assert call(obj_seg0=_u64(2, 1, 3)) == _lib.CDC_E_INVALID               # descends
    assert call(d_digests=ctypes.c_void_p((2 << 20) + 8)) == _lib.CDC_E_INVALID  # not 16-byte aligned
    # Valid arguments get as far as the library's state.  Without objects
    # nothing is launched, so that call is safe wherever it runs; the one with
    # objects and made-up pointers only where no device can run it.
    assert call(n=0, obj_seg0=_u64(3)) in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
    if not _has_gpu():
        assert call(n=0, obj_seg0=_u64(3)) == _lib.CDC_E_NOT_INIT
        assert call() == _lib.CDC_E_NOT_INIT


def test_check_context_argument_checks_and_defaults_without_a_device():
    L = _lib.lib()
    o = _lib.cdc_check_opts()
    o.fast = 5
    L.cdc_check_default_opts(ctypes.byref(o))
    assert o.struct_size == ctypes.sizeof(_lib.cdc_check_opts)
    assert (o.compress, o.key, o.fast, o.threads, o.batch_bytes, o.host_min_len) == (0, None, 0, 0, 0, 0)
    L.cdc_check_default_opts(None)
    h = ctypes.c_void_p()
    assert L.cdc_check_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_check_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    assert L.cdc_check_new(-1, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_check_new(64, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    for field, bad in [("struct_size", 0), ("struct_size", o.struct_size + 8), ("threads", -1), ("threads", 257),
                       ("batch_bytes", (1 << 30) + 1), ("compress", 7)]:
        keep = getattr(o, field)
        setattr(o, field, bad)
        assert L.cdc_check_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID, field
        assert not h.value
        setattr(o, field, keep)
    for fast in (0, 1):
        o.fast = fast
        st = L.cdc_check_new(0, ctypes.byref(o), ctypes.byref(h))
        if _has_gpu():  # an earlier test of the run may have initialised the library
            assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
            L.cdc_check_free(h)
            h = ctypes.c_void_p()
        else:
            assert st == _lib.CDC_E_NOT_INIT and not h.value
    f = (_lib.cdc_check_file * 1)()
    cb = _lib.CHECK_FILE_FN(lambda ctx, r: None)
    assert L.cdc_check_files(None, f, 1, cb, None, None) == _lib.CDC_E_INVALID
    assert L.cdc_check_add_packfile(None, b"x", 1) == _lib.CDC_E_INVALID
    assert L.cdc_check_add_packfile_path(None, b"/nonexistent") == _lib.CDC_E_INVALID
    L.cdc_check_free(None)


def test_python_layer_checks_key_and_compression():
    with pytest.raises(ValueError):
        check.CheckSession(key=b"short")
    with pytest.raises(ValueError):
        check.CheckSession(compression="ZSTD")
    with pytest.raises(ValueError):
        check.check_files([], [], key=bytes(31))


def _resources():
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
    return out


def test_object_digest_kernel_resources():
    """k_object_digest keeps k_chunk_digest's structure: no more private
    memory and no more spilled vector registers than k_chunk_digest's own
    lines in the same report, the same LDS (two workgroups per CU), and the
    same occupancy."""
    out = _resources()
    obj = [v for k, v in out.items() if "k_object_digest" in k]
    chunk = [v for k, v in out.items() if "k_chunk_digest" in k]
    assert len(obj) == 1 and len(chunk) == 2, sorted(out)
    k = obj[0]
    assert int(k["ScratchSize [bytes/lane]"]) <= min(int(c["ScratchSize [bytes/lane]"]) for c in chunk)
    assert int(k["VGPRs Spill"]) <= min(int(c["VGPRs Spill"]) for c in chunk)
    assert int(k["LDS Size [bytes/block]"]) <= max(int(c["LDS Size [bytes/block]"]) for c in chunk)
    assert int(k["Occupancy [waves/SIMD]"]) >= min(int(c["Occupancy [waves/SIMD]"]) for c in chunk)


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cplan") / "check_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "check_plan_check.cpp"),
           os.path.join(ROOT, "plakar_amd", "csrc", "cdc_sha256.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_planner_block_arithmetic_and_split_under_sanitizers(plan_check_exe):
    """The stand-alone program: 4,000 random segment lists in exactly sized
    heap buffers replayed and hashed the way the kernel walks them, the block
    arithmetic against a byte-wise padding for totals up to 300 and around
    2^29, 2^32, 2^35 and 2^61, the split rule's edge cases; no sanitizer
    report and no broken promise."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) plans, (\d+) objects, (\d+) totals, ok", r.stdout)
    assert m and int(m.group(1)) == 4000 and int(m.group(2)) > 15000 and int(m.group(3)) > 1000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
