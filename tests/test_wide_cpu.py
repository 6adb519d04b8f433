"""The compression level's checks that need no GPU: the DEFLATE writer
(plakar_amd/csrc/deflate_enc.h) takes records that reach before their segment
(tests/c/wide_records_check.cpp under the sanitizers, each member judged by
zlib there and walked by inflate_ref here), the new entry points' argument
checks before the device, the Python keywords, the exported symbols and the
compiler's resource report of k_lz_seq_wide, and the generator of contents
with planted repeats (tests/planted.py) that the device tests feed it."""
import ctypes
import inspect
import os
import re
import struct
import subprocess
import zlib

import pytest

import inflate_ref as ir
import planted
from plakar_amd import _lib, archive, build, encode, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIVATE_MAX = 256       # bytes per lane
LDS_MAX = 163_840       # one CU's LDS
SEG = 8192
WINDOW = 32768
NEW_SYMBOLS = ["cdc_encode_device_level", "cdc_backup_set_level", "cdc_gzip_stream_set_level", "cdc_archive_set_level",
               "cdc_zip_pieces_device_level"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The stand-alone program, built with the sanitizers and run once:
    (stdout, {case: [(member, content) with dynamic blocks, with fixed blocks]})."""
    d = tmp_path_factory.mktemp("wide")
    exe, out = str(d / "wide_records_check"), str(d / "members.bin")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "c", "wide_records_check.cpp"),
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
    rows = re.findall(r"^M (\S+) (\d+) (\d+) (\d+) (\d+)$", r.stdout, re.M)
    assert len(pairs) == 2 * len(rows)
    return r.stdout, {row[0]: (row, pairs[2 * i:2 * i + 2]) for i, row in enumerate(rows)}


def _matches(member):
    out, end, walk = ir.inflate(member, 10)
    assert end + 8 == len(member)
    return out, [m for b in walk for m in b["matches"]], {b["btype"] for b in walk}


def test_members_with_records_before_their_segment_inflate(run):
    _, cases = run
    assert set(cases) == {"six-segments", "six-segments-two-refused", "level-0-rule-all-records",
                          "level-0-rule-kept-records", "two-segments"}
    for name, (row, pairs) in cases.items():
        for (m, c), btype in zip(pairs, (2, 1)):
            assert zlib.decompress(m, 31) == c, name
            assert ir.status_of(m) == (0, c), name
            out, ms, kinds = _matches(m)
            assert out == c and kinds == {btype}, name
            assert sum(ln for _, ln, _ in ms) > 0
            assert max(d for _, _, d in ms) == int(row[4]), name


def test_the_edges_of_the_window_are_taken(run):
    _, cases = run
    m, c = cases["six-segments"][1][0]
    _, ms, _ = _matches(m)
    by_pos = {}
    for pos, ln, d in ms:
        by_pos.setdefault(pos, []).append((ln, d))
    # offset p + hist exactly: the copy starts at the blob's first byte
    for pos in (300, SEG + 350, 2 * SEG + 5, 3 * SEG + 100, 4 * SEG):
        assert by_pos[pos][0][1] == pos, pos
    assert {0, SEG, 2 * SEG, 3 * SEG, WINDOW} == {min(WINDOW, (pos // SEG) * SEG) for pos in by_pos}, "every hist occurs"
    # 32,768 exactly, in pairs that add up to a record longer than 258
    assert by_pos[4 * SEG] == [(258, WINDOW)] and by_pos[4 * SEG + 258] == [(258, WINDOW)]
    assert by_pos[4 * SEG + 516] == [(184, WINDOW)]
    # an overlapping copy at offset 1 from a segment's first byte
    assert by_pos[SEG][0] == (258, 1) and c[SEG - 1:SEG + 300] == c[SEG - 1:SEG] * 301
    # a last piece of 2 bytes borrows from the pair before it
    assert [by_pos[5 * SEG + 4000 + k][0][0] for k in (0, 258, 515)] == [258, 257, 3]
    m, c = cases["two-segments"][1][0]
    _, ms, _ = _matches(m)
    assert ms[0] == (SEG, 4, SEG)


def test_records_one_byte_too_far_come_out_as_literals(run):
    _, cases = run
    for m, c in cases["six-segments-two-refused"][1]:
        _, ms, _ = _matches(m)
        dists = {d for _, _, d in ms}
        assert WINDOW + 1 not in dists and SEG + 372 + 1 not in dists and max(dists) == WINDOW
        assert len({pos for pos, _, _ in ms if pos in (SEG + 372, 5 * SEG + 100)}) == 0, "no token starts where they stood"
    assert int(cases["six-segments-two-refused"][0][3]) == int(cases["six-segments"][0][3]) == 11


def test_hist_0_is_the_level_0_rule(run):
    _, cases = run
    a, b = cases["level-0-rule-all-records"][1], cases["level-0-rule-kept-records"][1]
    assert a == b, "records that reach before their segment are literals when hist is 0"
    _, ms, _ = _matches(a[0][0])
    assert all(d <= pos % SEG for pos, _, d in ms) and len(ms) == 2 + 1  # the 500-byte run is two pairs


def test_new_entry_points_are_exported_and_declared():
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "plakar_cdc.h")) as f:
        h = f.read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
        assert re.search(rf"\bint {name}\(", h), name
    assert re.search(r"#define CDC_LEVEL_FAST 0\b", h) and re.search(r"#define CDC_LEVEL_WIDE 1\b", h)
    assert (_lib.CDC_LEVEL_FAST, _lib.CDC_LEVEL_WIDE) == (0, 1)
    assert h.count("compression/compression.go:12-51") >= len(NEW_SYMBOLS)
    assert L.cdc_abi_version() == 1


def test_encode_level_is_checked_before_the_device():
    L = _lib.lib()
    offs, lens, oo = (ctypes.c_uint64 * 1)(), (ctypes.c_uint64 * 1)(100), (ctypes.c_uint64 * 2)()
    buf = ctypes.c_void_p(4096)  # never dereferenced: every call below fails on its arguments
    good = dict(device=0, d_base=buf, offsets=offs, lens=lens, n=1, compress=_lib.CDC_COMPRESS_GZIP, key=None,
                random=None, d_out=buf, out_cap=1 << 20, out_offsets=oo, level=1, stream=None)
    order = list(good)
    for level in (2, -1, 6):
        for comp in (_lib.CDC_COMPRESS_NONE, _lib.CDC_COMPRESS_LZ4, _lib.CDC_COMPRESS_GZIP, 7):
            a = dict(good, level=level, compress=comp)
            assert L.cdc_encode_device_level(*[a[k] for k in order]) == _lib.CDC_E_INVALID, (level, comp)
    for name, bad in [("d_base", None), ("out_offsets", None), ("d_out", None), ("device", 64)]:
        a = dict(good, **{name: bad})
        assert L.cdc_encode_device_level(*[a[k] for k in order]) == _lib.CDC_E_INVALID, name
    big = (ctypes.c_uint64 * 1)(1 << 31)
    assert L.cdc_encode_device_level(*[dict(good, lens=big)[k] for k in order]) == _lib.CDC_E_UNSUPPORTED


def test_zip_pieces_level_is_checked_before_the_device():
    L = _lib.lib()
    total = ctypes.c_uint64(7)
    for level in (2, -1):
        assert L.cdc_zip_pieces_device_level(0, None, 0, None, 0, None, 0, None, 0, None, ctypes.byref(total), level,
                                             None) == _lib.CDC_E_INVALID
    for level in (0, 1):   # no pieces: nothing to do, at either level
        assert L.cdc_zip_pieces_device_level(0, None, 0, None, 0, None, 0, None, 0, None, ctypes.byref(total), level,
                                             None) == _lib.CDC_OK
        assert total.value == 0


def test_gzip_stream_set_level_before_and_after_a_piece():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_gzip_stream_new(0, ctypes.byref(h)) == _lib.CDC_OK   # touches no device
    try:
        assert L.cdc_gzip_stream_set_level(None, 1) == _lib.CDC_E_INVALID
        for level in (2, -1):
            assert L.cdc_gzip_stream_set_level(h, level) == _lib.CDC_E_INVALID
        assert L.cdc_gzip_stream_set_level(h, 1) == _lib.CDC_OK
        assert L.cdc_gzip_stream_set_level(h, 0) == _lib.CDC_OK
        n = ctypes.c_uint64()
        if L.cdc_gzip_stream_piece(h, None, 0, 1, ctypes.c_void_p(4096), 0, ctypes.byref(n), None) == _lib.CDC_E_NOSPACE:
            # the empty last piece needs 23 bytes and got none: the writer is as it was
            assert n.value == 23 and L.cdc_gzip_stream_set_level(h, 1) == _lib.CDC_OK
    finally:
        L.cdc_gzip_stream_free(h)
    assert L.cdc_backup_set_level(None, 0) == _lib.CDC_E_INVALID
    assert L.cdc_archive_set_level(None, 0) == _lib.CDC_E_INVALID


def test_python_layers_take_the_level():
    for fn in (encode.encode_device, encode.encode_blobs, encode.DeviceEncoder.__init__, snapshot.BackupSession.__init__,
               snapshot.backup_files, archive.GzipStream.__init__, archive.ArchiveSession.__init__,
               archive.ZipSession.__init__, archive.archive_files, archive.zip_files, archive.zip_pieces_device):
        assert inspect.signature(fn).parameters["level"].default == 0, fn.__qualname__
    assert encode.DeviceEncoder(compression="GZIP", level=1).level == 1 and encode.DeviceEncoder().level == 0
    assert [_lib.level_code(v) for v in (0, 1)] == [0, 1]
    for bad in (2, -1, "1", None, True, 1.5):
        with pytest.raises(ValueError):
            _lib.level_code(bad)
        with pytest.raises(ValueError):
            encode.DeviceEncoder(level=bad)
        with pytest.raises(ValueError):
            snapshot.BackupSession(level=bad)
        with pytest.raises(ValueError):
            snapshot.backup_files([], level=bad)
        with pytest.raises(ValueError):
            archive.ArchiveSession(level=bad)
        with pytest.raises(ValueError):
            archive.ZipSession(level=bad)
        with pytest.raises(ValueError):
            archive.GzipStream(level=bad)


def test_backup_session_takes_the_level():
    """Without a device the native context cannot come up, and says so; with
    one it does, and the level is set on it."""
    try:
        with snapshot.BackupSession(compression="GZIP", level=1) as s:
            assert s._h
            assert _lib.lib().cdc_backup_set_level(s._h, 2) == _lib.CDC_E_INVALID
            assert _lib.lib().cdc_backup_set_level(s._h, 0) == _lib.CDC_OK
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


def test_wide_kernel_resources():
    name = "k_lz_seq_wide"
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3enc{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0
    assert int(k["ScratchSize [bytes/lane]"]) < PRIVATE_MAX
    assert 40960 + 2 * 8192 <= int(k["LDS Size [bytes/block]"]) <= LDS_MAX, "the window and a table of at least 8,192 u16"


# ---- the planted generator (tests/planted.py) that tests/test_encode_wide_planted.py feeds the device ----
def test_planted_is_deterministic_and_replays():
    for mode in ("free", "edges", "far"):
        for n, seed in ((0, 1), (1, 2), (5, 3), (8193, 4), (70_001, 5), (300_000, 6)):
            content, plants = planted.planted(n, seed, mode)
            assert (content, plants) == planted.planted(n, seed, mode) and len(content) == n
            assert planted.replay(content, plants) == content, (mode, n, seed)
            assert all(1 <= d <= min(pos, planted.DIST_MAX) and 1 <= ln <= planted.RUN_MAX for pos, ln, d in plants)
            assert all(a[0] + a[1] <= b[0] for a, b in zip(plants, plants[1:])), "ascending, no copy inside another"
            if mode == "edges":
                assert all(d in planted.EDGES or d == pos for pos, _, d in plants)
            if mode == "far":
                assert all(d > planted.FAR for _, _, d in plants)
    assert planted.planted(70_001, 5)[0] != planted.planted(70_001, 6)[0]
    with pytest.raises(ValueError):
        planted.planted(10, 1, "near")


def test_planted_has_what_the_search_is_to_meet():
    content, plants = planted.planted(1 << 20, 11, "edges")
    assert {d for _, _, d in plants} >= set(planted.EDGES)
    assert any(d < ln for _, ln, d in plants), "a copy that overlaps itself"
    content, plants = planted.planted(1 << 20, 12)
    touching = sum(a[0] + a[1] == b[0] for a, b in zip(plants, plants[1:]))
    literal_runs = len(plants) - touching + 1
    assert 0.15 < touching / (len(plants) + literal_runs) < 0.35, "about one run in four is a copy right behind a copy"
    lens = [ln for _, ln, _ in plants]
    assert min(lens) <= 8 and max(lens) > 6000 and max(d for _, _, d in plants) > WINDOW
    gaps = [b[0] - a[0] - a[1] for a, b in zip(plants, plants[1:])]
    assert max(gaps) > SEG, "a repeat that begins deep inside a literal run of more than a segment"


def test_planted_batches_reach_past_8192():
    for content, plants in planted.window_blobs():
        assert planted.replay(content, plants) == content
        if len(content) > 2 * SEG:
            assert planted.far_share(plants, len(content)) > 0
    lens = [len(c) for c, _ in planted.window_blobs()]
    assert {n // SEG for n in lens} == {1, 2, 3, 4, 5} and {n % SEG for n in lens} == set(planted.WINDOW_TAILS)
    for _, n, seed, mode in planted.SIZE_CASES:
        content, plants = planted.planted(n, seed, mode)
        assert planted.far_share(plants, n) > 0.05
    for seed in planted.BATCH_SEEDS:
        batch = planted.seeded_batch(seed)
        assert batch == planted.seeded_batch(seed) and 1 <= len(batch) <= 120
        assert sum(len(c) >= planted.BLOCK for c, _ in batch) == 1
        assert sum(planted.far_share(p, 1) for _, p in batch) > 0, seed
    tile = planted.tile_blobs()
    assert len(tile) == 1500 and all(9000 <= len(c) <= 20000 for c, _ in tile)
    assert sum(planted.far_share(p, 1) for _, p in tile) > 0
