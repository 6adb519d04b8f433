"""Ranged reads' checks that need no GPU: the argument checks that
cdc_decode_prefix_device and cdc_restore_ranges make before they touch the
device, the Python layer's ValueErrors, the prefix kernels' lines in the
compiler's resource report, and two stand-alone sanitizer programs: the range
planner against a brute-force byte map (tests/c/read_plan_check.cpp) and the
walkers' stop mode at every cut (tests/c/prefix_host_fuzz.cpp)."""
import ctypes
import os
import re
import struct
import subprocess
import types

import pytest

import decode_ref as dr
from plakar_amd import _lib, build, decode, restore, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _u64(n=1):
    return (ctypes.c_uint64 * max(n, 1))()


def test_decode_prefix_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, upto, oo, st = _u64(), _u64(), _u64(), _u64(2), (ctypes.c_int32 * 1)()
    upto[0] = 8
    buf = ctypes.c_void_p(4096)  # never dereferenced: every call below fails on its arguments
    good = dict(device=0, d_in=buf, offsets=offs, lens=lens, upto=upto, n=1, compressed=1, key=None, d_out=buf,
                out_cap=16, out_offsets=oo, status=st, stream=None)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return L.cdc_decode_prefix_device(*[a[k] for k in order])

    for name, bad in [("d_in", None), ("offsets", None), ("lens", None), ("upto", None), ("status", None),
                      ("out_offsets", None), ("d_out", None), ("device", -1), ("device", 64)]:
        assert call(**{name: bad}) == _lib.CDC_E_INVALID, name
    for sel in (_lib.CDC_COMPRESS_NONE, _lib.CDC_COMPRESS_GZIP):
        assert call(compressed=sel, lens=None) == _lib.CDC_E_INVALID  # upto without lens
    # the capacity is held against the sum of upto on the host: nothing is launched
    oo[1] = 0
    assert call(out_cap=7) == _lib.CDC_E_NOSPACE and (oo[0], oo[1]) == (0, 8)
    two = _u64(2)
    two[0], two[1] = 2 ** 64 - 1, 2
    assert call(n=2, upto=two, offsets=_u64(2), lens=_u64(2), out_offsets=_u64(3),
                status=(ctypes.c_int32 * 2)()) == _lib.CDC_E_INVALID  # the sum wraps
    # nothing wanted: CDC_OK with nothing read, wherever it runs
    upto[0] = 0
    st[0] = 77
    assert call() == _lib.CDC_OK and st[0] == 0 and oo[1] == 0
    assert call(n=0) == _lib.CDC_OK


def test_restore_ranges_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)  # stands for a context: every call below fails before it is looked at
    files = (_lib.cdc_restore_file * 1)()
    ranges = (_lib.cdc_read_range * 1)()
    cb = _lib.READ_RANGE_FN(lambda ctx, r: None)
    stats = _lib.cdc_read_stats()
    stats.struct_size = ctypes.sizeof(stats)
    E = _lib.CDC_E_INVALID
    assert L.cdc_restore_ranges(None, files, 1, ranges, 1, cb, None, ctypes.byref(stats)) == E  # no (or a closed) context
    assert L.cdc_restore_ranges(fake, None, 1, ranges, 1, cb, None, None) == E
    assert L.cdc_restore_ranges(fake, files, 1, None, 1, cb, None, None) == E
    assert L.cdc_restore_ranges(fake, files, -1, ranges, 1, cb, None, None) == E
    assert L.cdc_restore_ranges(fake, files, 1, ranges, -1, cb, None, None) == E
    files[0].nchunks = 3                        # chunks without their arrays
    assert L.cdc_restore_ranges(fake, files, 1, ranges, 1, cb, None, None) == E
    files[0].nchunks = 0
    stats.struct_size = 4                       # too small to carry its own size back
    assert L.cdc_restore_ranges(fake, files, 1, ranges, 1, cb, None, ctypes.byref(stats)) == E
    assert ctypes.sizeof(_lib.cdc_read_range) == 24 and ctypes.sizeof(_lib.cdc_read_stats) == 8 + 12 * 8 + 7 * 8
    assert L.cdc_abi_version() == 1


def test_header_declares_what_the_bindings_bind():
    with open(os.path.join(ROOT, "include", "plakar_cdc.h")) as f:
        h = f.read()
    assert re.search(r"int cdc_decode_prefix_device\(int device, const void \*d_in, const uint64_t \*offsets, "
                     r"const uint64_t \*lens,\s+const uint64_t \*upto, uint32_t n, int compressed", h)
    assert re.search(r"int cdc_restore_ranges\(cdc_restore \*r, const cdc_restore_file \*files, int nfiles, "
                     r"const cdc_read_range \*ranges,\s+int nranges, cdc_read_range_fn on_range, void \*ctx, "
                     r"cdc_read_stats \*stats\);", h)
    body = re.search(r"typedef struct cdc_read_stats \{(.*?)\} cdc_read_stats;", h, re.S).group(1)
    names = re.findall(r"\b([a-z_0-9]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.cdc_read_stats._fields_]


def test_python_layer_value_errors():
    with pytest.raises(ValueError):
        decode.decode_prefix([b"x"], [1, 2])            # one upto per blob
    with pytest.raises(ValueError):
        decode.decode_prefix([b"x"], [-1])
    with pytest.raises(ValueError):
        decode.decode_prefix([b"x"], [1], key=b"short")
    with pytest.raises(ValueError):
        decode.decode_prefix([b"x"], [1], compression="ZSTD")
    assert decode.decode_prefix([], []) == []
    with pytest.raises(ValueError):
        snapshot.read_ranges([], [], [], compression="ZSTD")
    with pytest.raises(ValueError):
        restore.read_ranges([], [], [], key=b"short")
    s = restore.RestoreSession.__new__(restore.RestoreSession)  # a session that is closed
    s._h, s._keep = None, []
    with pytest.raises(ValueError):
        s.read_ranges([], [])
    obj = types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=bytes(32), Length=10)])
    with pytest.raises(ValueError):
        restore.SnapshotFile(s, obj, readahead=-1)
    f = restore.SnapshotFile(s, obj)
    assert f.size == 10 and f.seek(10) == 10 and f.read() == b"" and f.seek(-10, 2) == 0
    for bad in ((11,), (-1,), (1, 2), (-11, 2)):
        with pytest.raises(OSError):
            f.seek(*bad)
    with pytest.raises(ValueError):
        f.seek(0, 9)
    with pytest.raises(ValueError):
        f.read(1)                                       # the session is closed: said before any device call


def test_range_tuples_are_checked():
    class Open(restore.RestoreSession):
        def __init__(self):
            self._h, self._keep = ctypes.c_void_p(1), []

        def close(self):
            self._h = None

    s = Open()
    for bad in ([(0, -1, 5)], [(-1, 0, 5)], [(0, 0, -5)], [(0, 0)]):
        with pytest.raises(ValueError):
            s.read_ranges([], bad)
    s.close()


def _report():
    out, cur = {}, None
    with open(build.resources_path()) as f:
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


@pytest.mark.parametrize("name,beside", [("k_lz4_prefix", "k_lz4_emit"), ("k_gz_prefix", "k_gz_emit")])
def test_prefix_kernels_keep_the_budget_of_the_ones_they_sit_beside(name, beside):
    rep = _report()

    def one(k):
        ks = [v for n, v in rep.items() if n.startswith(f"_ZN3dec{len(k)}{k}E")]
        assert len(ks) == 1, f"{k} is not in the resource report"
        return ks[0]

    new, old = one(name), one(beside)
    assert int(new["VGPRs Spill"]) == 0 and int(new["SGPRs Spill"]) == 0 and int(new["ScratchSize [bytes/lane]"]) == 0
    assert int(new["LDS Size [bytes/block]"]) == int(old["LDS Size [bytes/block]"])
    assert int(new["Occupancy [waves/SIMD]"]) >= int(old["Occupancy [waves/SIMD]"])


def test_range_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "read_plan_check")
    subprocess.run(SAN + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
                          os.path.join(ROOT, "tests", "c", "read_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) cases, (\d+) ranges, (\d+) bytes, ok", r.stdout)
    assert m and int(m.group(1)) > 300 and int(m.group(2)) > 100_000 and int(m.group(3)) > 1_000_000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _blocks():
    """The distinct good blocks the GPU tests decode (hand-made sequences with
    extension bytes, liblz4's 64-KiB blocks, offset 65,535), the smaller first."""
    seen = {b for b, _ in dr.ext_blocks()}
    for name in ("lz4f-0x7c", "mixed", "many-blocks"):
        seen |= set(dr.lenient_blocks(dr.fixture_frames()[name][0]))
    return sorted(seen, key=len)[-12:] + sorted(seen, key=len)[:12]


def test_stop_mode_under_sanitizers(tmp_path):
    exe = str(tmp_path / "prefix_host_fuzz")
    subprocess.run(SAN + ["-o", exe, os.path.join(ROOT, "tests", "c", "prefix_host_fuzz.cpp"), "-l:libz.so.1"], check=True)
    path = tmp_path / "blocks.bin"
    with open(path, "wb") as f:
        for b in _blocks():
            f.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([exe, "--blocks", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) cuts, (\d+) short ok, (\d+) short refused, ok", r.stdout)
    assert m and int(m.group(1)) > 150_000 and int(m.group(2)) > 1000 and int(m.group(3)) > 1000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
