"""GZIP Encode's checks that need no GPU: the shared DEFLATE writer
(plakar_amd/csrc/deflate_enc.h) passes the sanitizer program (code lengths
from seeded histograms, whole members from hand-made record lists, each judged
by zlib there and by inflate_ref here, and the CRC-32 assembled from stretches
and spans as the device does it, against zlib's), the bound, the entry point's argument
checks before the device, the Python layers, and the compiler's resource
report of the new kernels."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import pytest

import inflate_ref as ir
from plakar_amd import _lib, build, encode, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIVATE_MAX = 256       # bytes per lane
LDS_MAX = 163_840       # one CU's LDS
SPAN = 32768


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The stand-alone program, built with the sanitizers and run once:
    (stdout, [(member, content)])."""
    d = tmp_path_factory.mktemp("deflate")
    exe, out = str(d / "deflate_host_fuzz"), str(d / "members.bin")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "c", "deflate_host_fuzz.cpp"),
           "-l:libz.so.1"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe, "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok")
    pairs = []
    with open(out, "rb") as f:
        data = f.read()
    p = 0
    while p < len(data):
        (n,) = struct.unpack_from("<I", data, p)
        m = data[p + 4:p + 4 + n]
        p += 4 + n
        (k,) = struct.unpack_from("<I", data, p)
        pairs.append((m, data[p + 4:p + 4 + k]))
        p += 4 + k
    return r.stdout, pairs


def test_code_lengths_are_limited_and_complete(run):
    stdout, _ = run
    rows = re.findall(r"^H (\S+) (\d+) (\d+)((?: \d+)+)$", stdout, re.M)
    names = {r[0] for r in rows}
    assert {"fib-lit", "fib-dist", "one-used-lit", "none-used-dist", "one-used-dist-17", "two-used-dist",
            "eob-and-one-literal", "all-286-equal", "all-286-powers", "all-30-equal", "all-30-powers", "fib-cl",
            "powers-cl", "one-used-cl"} <= names and len(rows) > 200
    deep = 0
    for name, limit, n, lens in rows:
        limit, lens = int(limit), [int(x) for x in lens.split()]
        assert len(lens) == int(n), name
        assert max(lens) <= limit, name
        # inflate_ref counts in units of 2^-15: a set limited to 7 bits is complete at the same sum
        assert ir.kraft(lens) == 1 << 15 and ir.set_ok(lens), name
        assert sum(1 for x in lens if x) >= 2, name
        deep += max(lens) == limit
    assert deep >= 5, "the limit was reached"
    by = {r[0]: [int(x) for x in r[3].split()] for r in rows}
    assert [x for x in by["none-used-dist"] if x] == [1, 1]
    assert by["one-used-dist-17"][17] == 1 and by["one-used-dist-17"][0] == 1
    assert by["eob-and-one-literal"][256] == 1 and by["eob-and-one-literal"][ord("x")] == 1


def test_members_written_on_the_host_inflate(run):
    stdout, pairs = run
    rows = re.findall(r"^M (\S+) (\d+) (\d+) (\d+) (\d+) (\d+)$", stdout, re.M)
    assert len(rows) == len(pairs) > 60
    kinds = [0, 0, 0]
    walked = 0
    for (name, msize, csize, st, fx, dy), (m, c) in zip(rows, pairs):
        assert (len(m), len(c)) == (int(msize), int(csize)), name
        assert zlib.decompress(m, 31) == c, name
        assert len(m) <= encode.encode_bound(len(c), "GZIP", False), name
        for i, k in enumerate((st, fx, dy)):
            kinds[i] += int(k)
        if walked + len(c) <= 2 << 20:   # the Python walker's budget; zlib has judged every member above
            assert ir.status_of(m) == (0, c), name
            walked += len(c)
    assert all(kinds), f"stored, fixed and dynamic blocks all occur: {kinds}"
    # every record length 4..1100: its pairs are 3..258 bytes long and the content is whole
    m, c = pairs[0]
    out, end, walk = ir.inflate(m, 10)
    assert out == c and end + 8 == len(m)
    lengths = [ln for b in walk for _, ln, _ in b["matches"]]
    assert min(lengths) >= 3 and max(lengths) == 258 and {255 + 1, 255 + 2} <= set(lengths)
    # a stored block that starts mid-byte, after a coded one
    name_to = {r[0]: p for r, p in zip(rows, pairs)}
    m, c = name_to["alternating"]
    _, _, walk = ir.inflate(m, 10)
    assert [b["btype"] for b in walk[:4]] == [2, 0, 2, 0]


def test_crc32_assembly_equals_zlib(run):
    """The program restated the device's CRC-32 assembly (stretches, spans,
    the moved start) with the shared functions and compared it with zlib's
    crc32 itself; here: it printed every size, and the shift past 2^29 + 3
    zero bytes, where the exponent is reduced mod 2^32 - 1."""
    stdout, _ = run
    rows = re.findall(r"^C (\d+) ([0-9a-f]{8})$", stdout, re.M)
    assert [int(n) for n, _ in rows] == [1, 127, 128, 129, 32767, 32768, 32769, (2 << 20) + 1, (4 << 20) + 5,
                                         (8 << 20) + 3]
    assert len({c for _, c in rows}) == len(rows)
    (shift,) = re.findall(r"^S (\d+) ([0-9a-f]{8})$", stdout, re.M)
    n = (1 << 29) + 3
    assert int(shift[0]) == n and 8 * n > 1 << 32
    z, piece = zlib.crc32(b"shift"), bytes(1 << 20)
    for _ in range(n >> 20):
        z = zlib.crc32(piece, z)
    assert int(shift[1], 16) == zlib.crc32(bytes(n & 0xFFFFF), z)


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, (4 << 20) + 5])
def test_bound(n):
    z = zlib.compressobj(0, wbits=31)
    stored = len(z.compress(bytes(n)) + z.flush())
    b = encode.encode_bound(n, "GZIP", False)
    assert stored <= b <= n + 18 + 5 * (-(-n // SPAN) + 1)
    f = b  # sealed: the 60-byte header and 28 bytes per 64-KiB piece
    assert encode.encode_bound(n, "GZIP", True) == 60 + f + 28 * (-(-f // 65536))
    assert _lib.lib().cdc_encode_bound(n, _lib.CDC_COMPRESS_GZIP, 0) == b
    # the other selectors are what they were: every other non-zero value means LZ4
    lz4 = 7 + 4 * (-(-n // (4 << 20))) + n + 8
    assert [encode.encode_bound(n, c, False) for c in (True, "LZ4", False, None)] == [lz4, lz4, n, n]
    assert _lib.lib().cdc_encode_bound(n, 7, 0) == lz4


def test_gzip_encode_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, oo = (ctypes.c_uint64 * 1)(), (ctypes.c_uint64 * 1)(100), (ctypes.c_uint64 * 2)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: every call below fails on its arguments
    good = dict(device=0, d_base=buf, offsets=offs, lens=lens, n=1, compress=_lib.CDC_COMPRESS_GZIP, key=None,
                random=None, d_out=buf, out_cap=1 << 20, out_offsets=oo, stream=None)
    order = list(good)
    for name, bad in [("d_base", None), ("offsets", None), ("lens", None), ("out_offsets", None), ("d_out", None),
                      ("device", -1), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_encode_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name
    assert L.cdc_encode_device(*[dict(good, key=bytes(32))[k] for k in order]) == _lib.CDC_E_INVALID  # a key, no random
    for n in (1 << 31, (1 << 32) + 5):
        big = (ctypes.c_uint64 * 1)(n)
        assert L.cdc_encode_device(*[dict(good, lens=big)[k] for k in order]) == _lib.CDC_E_UNSUPPORTED, n


def test_python_layers_take_gzip_and_refuse_other_names():
    e = encode.DeviceEncoder(compression="GZIP")
    assert e.compress == "GZIP" and encode._sel(e.compress) == _lib.CDC_COMPRESS_GZIP
    assert encode.DeviceEncoder(compression="LZ4").compress is True
    assert encode.DeviceEncoder(compression=None).compress is False
    assert (encode._sel(True), encode._sel(False), encode._sel("GZIP")) == (1, 0, 2)
    for bad in ("ZSTD", "gzip"):
        with pytest.raises(ValueError):
            encode.DeviceEncoder(compression=bad)
        with pytest.raises(ValueError):
            encode.encode_bound(10, bad)
        with pytest.raises(ValueError):
            snapshot.BackupSession(compression=bad)
        with pytest.raises(ValueError):
            snapshot.backup_files([], compression=bad)


def test_backup_session_constructs_for_gzip():
    """The name passes the configuration check (it was a ValueError before);
    without a device the native context then cannot come up, and says so."""
    try:
        with snapshot.BackupSession(compression="GZIP", key=bytes(32)) as s:
            assert s._h
    except _lib.CdcError as e:
        assert e.status in (_lib.CDC_E_NO_DEVICE, _lib.CDC_E_DEVICE, _lib.CDC_E_NOT_INIT)


def test_header_no_longer_says_gzip_is_not_written():
    with open(os.path.join(ROOT, "include", "plakar_cdc.h")) as f:
        h = f.read()
    assert "GZIP is not written" not in h and "writing GZIP is not built" not in h


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


@pytest.mark.parametrize("name", ["k_dfl_size", "k_dfl_emit", "k_gz_fin"])
def test_gzip_encode_kernel_resources(name):
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3enc{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["VGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) < PRIVATE_MAX
    assert int(k["LDS Size [bytes/block]"]) <= LDS_MAX
