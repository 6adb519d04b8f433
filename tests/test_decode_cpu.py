"""Decode's checks that need no GPU: the fixtures hold the structures the GPU
tests rely on, the shared LZ4 walker passes the sanitizer program (its valid
fixtures, 20,000 mutations and every block the GPU tests use), the entry
points reject bad arguments before touching the device, and the compiler's
resource report of the decode kernels stays within bounds."""
import ctypes
import ctypes.util
import os
import re
import struct
import subprocess

import pytest

import decode_ref as dr
import lz4_ref
from plakar_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECODE_KERNELS = ("k_dec_keys", "k_dec_pows", "k_rec_open", "k_lz4_size", "k_dec_plan", "k_lz4_emit",
                  "k_dec_compact", "k_dec_copy", "k_check_cmp")
PRIVATE_MAX = 256       # bytes per lane: no by-value copy of the launch descriptor
LDS_MAX = 163_840       # one CU's LDS


def test_block_fixture_keeps_its_structures():
    blk = lz4_ref.lz4_block_compress(dr.block_fixture())
    data, seqs = lz4_ref.walk_block(blk)
    assert data == dr.block_fixture()
    assert len(seqs) == 4 and seqs[-1][1:] == (0, 0)
    assert seqs[0] == (40960, 40960, 20480)        # the long literal run, the far long match
    assert seqs[1][1:] == (1, 4999) and seqs[2][1:] == (3, 2097)  # overlapping matches
    assert max(s[1] for s in seqs) == 40960


def test_offset_65535_fixture():
    data, seqs = lz4_ref.walk_block(lz4_ref.lz4_block_compress(dr.offset_65535_content()))
    assert data == dr.offset_65535_content()
    assert max(s[1] for s in seqs) == 65535


def test_extension_terminator_fixtures():
    lits, matches = set(), set()
    for blk, content in dr.ext_blocks():
        data, seqs = lz4_ref.walk_block(blk)
        assert data == content
        lits |= {s[0] for s in seqs}
        matches |= {s[2] for s in seqs}
    assert {15, 270} <= lits and {19, 274} <= matches


def test_fixture_frames_decode_with_liblz4():
    import crypto_ref
    for name, (frame, content) in dr.fixture_frames().items():
        if content is not None:
            assert crypto_ref.lz4f_decompress(frame) == content, name
    assert len(dr.lenient_blocks(dr.fixture_frames()["two-blocks"][0])) == 2
    assert len(dr.lenient_blocks(dr.fixture_frames()["lz4f-0x7c"][0])) >= 4  # 64-KiB blocks: multi-block


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lz4d") / "lz4d_host_fuzz")
    lz4 = ctypes.util.find_library("lz4") or "liblz4.so.1"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "c", "lz4d_host_fuzz.cpp"),
           f"-l:{lz4}"]
    subprocess.run(cmd, check=True)
    return exe


def test_walker_under_sanitizers(fuzz_exe, tmp_path):
    """The stand-alone program: fixtures against liblz4, 20,000 mutations, and
    every block the GPU tests decode; no sanitizer report, no wrong acceptance."""
    path = tmp_path / "blocks.bin"
    with open(path, "wb") as f:
        for b in dr.all_blocks():
            f.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([fuzz_exe, "--blocks", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) accepted, (\d+) rejected, ok", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _args(n=1):
    a = (ctypes.c_uint64 * max(n, 1))()
    return a


def test_decode_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, oo, st = _args(), _args(), _args(2), (ctypes.c_int32 * 1)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: every call below fails on its arguments
    good = dict(device=0, d_in=buf, offsets=offs, lens=lens, n=1, compressed=1, key=None, d_out=buf, out_cap=16,
                out_offsets=oo, status=st, stream=None)
    order = list(good)
    for name, bad in [("d_in", None), ("offsets", None), ("lens", None), ("status", None), ("out_offsets", None),
                      ("d_out", None), ("device", -1), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_decode_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name
    a = dict(good, n=0, out_offsets=None)
    assert L.cdc_decode_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID


def test_check_rejects_bad_arguments_before_the_device():
    L = _lib.lib()
    offs, lens, st = _args(), _args(), (ctypes.c_int32 * 1)()
    buf = ctypes.c_void_p(4096)
    sums = bytes(32)
    good = dict(device=0, d_in=buf, offsets=offs, lens=lens, n=1, compressed=1, key=None, checksums=sums,
                d_scratch=buf, scratch_cap=16, needed=None, status=st, stream=None)
    order = list(good)
    for name, bad in [("d_in", None), ("offsets", None), ("lens", None), ("status", None), ("checksums", None),
                      ("d_scratch", None), ("device", -1), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_check_device(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name


def test_new_status_codes_have_messages():
    L = _lib.lib()
    assert (_lib.CDC_E_AUTH, _lib.CDC_E_CORRUPT, _lib.CDC_E_MISMATCH) == (-12, -13, -14)
    for code in (-12, -13, -14):
        assert L.cdc_strerror(code).decode() != "unknown status"


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


@pytest.mark.parametrize("name", DECODE_KERNELS)
def test_decode_kernel_resources(name):
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3dec{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["VGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) < PRIVATE_MAX
    assert int(k["LDS Size [bytes/block]"]) <= LDS_MAX
