"""Archive's checks that need no GPU.  The streamed gzip member: the joiner and
the final block after a block that ends at each of the eight bits, the running
CRC-32 as the writer combines it, the piece bound (the stand-alone program
tests/c/gzip_stream_check.cpp, built from the library's headers under the
address and undefined-behaviour sanitizers; zlib judges what it wrote), the
entry points' argument checks before the device, and the compiler's resource
report of the new kernels.  The tar layout and the batch planner
(tests/c/archive_plan_check.cpp over archive_plan.h, the same way): every
header case read back by hand and by tarfile, and the plan against a
byte-level restatement of the stream."""
import ctypes
import io
import os
import re
import struct
import subprocess
import tarfile
import zlib

import pytest

from plakar_amd import _lib, archive, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = 32768


_built = {}


def _sanitized(tmp_path_factory, name, args_of):
    """Build tests/c/<name>.cpp with the sanitizers (once) and run it: (stdout, the output file)."""
    d = tmp_path_factory.mktemp(name)
    out = str(d / "out.bin")
    if name not in _built:
        exe = str(d / name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
               os.path.join(ROOT, "tests", "c", name + ".cpp")]
        subprocess.run(cmd, check=True)
        _built[name] = exe
    exe = _built[name]
    r = subprocess.run([exe] + args_of(out), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok")
    return r.stdout, out


def _records(path):
    with open(path, "rb") as f:
        data = f.read()
    pairs, p = [], 0
    while p < len(data):
        (n,) = struct.unpack_from("<I", data, p)
        a = data[p + 4:p + 4 + n]
        p += 4 + n
        (k,) = struct.unpack_from("<I", data, p)
        pairs.append((a, data[p + 4:p + 4 + k]))
        p += 4 + k
    return pairs


@pytest.fixture(scope="module")
def stream_run(tmp_path_factory):
    stdout, out = _sanitized(tmp_path_factory, "gzip_stream_check", lambda o: ["--out", o])
    return stdout, _records(out)


def test_joiner_and_final_block_at_every_end_bit(stream_run):
    stdout, pairs = stream_run
    rows = [(int(b), int(s), int(t)) for b, s, t in re.findall(r"^J (\d) (\d+) (\d+)$", stdout, re.M)]
    assert sorted(b for b, _, _ in rows) == list(range(8)) and len(pairs) == 16
    for b, s, t in rows:
        # the block's 74..81 bits end at bit b of byte E // 8; the joiner's 000 fits that byte up to bit 5 and
        # spills into one more from bit 6 on; then LEN and NLEN
        E = 74 + (b - 2) % 8
        assert E % 8 == b and s == E // 8 + (2 if b >= 6 else 1) + 4, (b, s)
        assert t == 6 + 1 + 4 + 5, "the second piece: 52 bits end at bit 4 of byte 6, the joiner, the final block"
    for stream, content in pairs:
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == content and d.eof and d.unused_data == b""
        assert stream.endswith(b"\x01\x00\x00\xff\xff")
        assert stream[-9:-5] == b"\x00\x00\xff\xff", "the joiner stands before the final block"


def test_running_crc_equals_zlib(stream_run):
    stdout, _ = stream_run
    rows = re.findall(r"^K (\w+) (\d+) ([0-9a-f]{8})$", stdout, re.M)
    assert [(k, int(n)) for k, n, _ in rows] == [("zeros", 0), ("zeros", 1), ("zeros", 65537),
                                                 ("zeros", (1 << 32) + 5), ("pattern", 65537)]
    head = zlib.crc32(b"archive")
    block = bytes(1 << 24)
    for kind, n, got in rows:
        n = int(n)
        if kind == "zeros":
            z = head
            for _ in range(n >> 24):
                z = zlib.crc32(block, z)
            z = zlib.crc32(bytes(n & 0xFFFFFF), z)
        else:
            z = zlib.crc32(bytes((i * 131 + (i >> 8)) & 255 for i in range(n)), head)
        assert int(got, 16) == z, (kind, n)


def test_piece_bound(stream_run):
    stdout, _ = stream_run
    rows = [tuple(map(int, r)) for r in re.findall(r"^B (\d+) (\d+) (\d+)$", stdout, re.M)]
    assert {n for n, _, _ in rows} >= {1, SPAN - 1, SPAN, SPAN + 1, (2 << 20) + SPAN + 1, (1 << 31) - 1}
    for n, worst, bound in rows:
        assert worst <= bound == archive.gzip_stream_bound(n) == n + 5 * (-(-n // SPAN)) + 29
    assert archive.gzip_stream_bound(0) == 29   # header, final block, trailer and the joiner's room


def test_stream_entry_points_check_their_arguments_before_the_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_gzip_stream_new(0, None) == _lib.CDC_E_INVALID
    for dev in (-1, 64):
        assert L.cdc_gzip_stream_new(dev, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_gzip_stream_new(0, ctypes.byref(h)) == _lib.CDC_OK and h
    buf, got = ctypes.c_void_p(4096), ctypes.c_uint64(7)   # never dereferenced: every call below ends on its arguments
    try:
        assert L.cdc_gzip_stream_piece(None, buf, 1, 0, buf, 100, ctypes.byref(got), None) == _lib.CDC_E_INVALID
        assert L.cdc_gzip_stream_piece(h, buf, 1, 0, buf, 100, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_gzip_stream_piece(h, None, 1, 0, buf, 100, ctypes.byref(got), None) == _lib.CDC_E_INVALID
        for n in (1 << 31, (1 << 32) + 5):
            assert L.cdc_gzip_stream_piece(h, buf, n, 0, buf, 1 << 40, ctypes.byref(got), None) == _lib.CDC_E_UNSUPPORTED
        # an empty piece that is not the last writes nothing and needs no output
        got.value = 7
        assert L.cdc_gzip_stream_piece(h, None, 0, 0, None, 0, ctypes.byref(got), None) == _lib.CDC_OK
        assert got.value == 0
        assert L.cdc_gzip_stream_piece(h, buf, 1, 0, None, 100, ctypes.byref(got), None) == _lib.CDC_E_INVALID
    finally:
        L.cdc_gzip_stream_free(h)
    L.cdc_gzip_stream_free(None)
    assert L.cdc_abi_version() == 1


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


@pytest.mark.parametrize("name", ["k_gzs_plan", "k_gzs_fin"])
def test_stream_kernel_resources(name):
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3enc{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["ScratchSize [bytes/lane]"]) == 0
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0


# ---- the tar layout and the planner (plakar_amd/csrc/archive_plan.h) ------------------------
GIB8 = 8 << 30
NAME255 = "p" * 150 + "/" + "n" * 104            # no valid split: the part after the slash is over 100
SPLIT255 = "d" * 154 + "/" + "f" * 100           # 255 bytes, prefix 154 and name 100
HEADER_CASES = [  # (label, type, mode, mtime, size, name, pax keys)
    ("name-100", 0, 0o644, 1_700_000_000, 5, "a" * 100, set()),
    ("name-101", 0, 0o600, 1_700_000_001, 5, "dir/" + "b" * 97, set()),
    ("name-255-split", 0, 0o644, 12, 0, SPLIT255, set()),
    ("name-255-no-split", 0, 0o644, 12, 0, NAME255, {"path"}),
    ("name-256-split", 0, 0o755, 12, 7, "e" * 155 + "/" + "g" * 100, set()),   # archive/tar's longest ustar name
    ("name-256", 0, 0o755, 12, 7, "e" * 150 + "/" + "g" * 105, {"path"}),
    ("name-257", 0, 0o755, 12, 7, "e" * 155 + "/" + "g" * 101, {"path"}),
    ("name-101-no-slash", 0, 0o644, 12, 7, "h" * 101, {"path"}),
    ("non-ascii", 0, 0o644, 12, 7, "café/naïve.txt", {"path"}),
    ("size-8g-1", 0, 0o644, 12, GIB8 - 1, "big", set()),
    ("size-8g", 0, 0o644, 12, GIB8, "bigger", {"size"}),
    ("mtime--1", 0, 0o644, -1, 3, "old", {"mtime"}),
    ("mtime-over", 0, 0o644, 1 << 33, 3, "far", {"mtime"}),
    ("all-three", 0, 0o7777, -5, GIB8 + 511, "ü" * 130, {"path", "size", "mtime"}),
    ("directory", 1, 0o755, 99, 0, "some/dir", set()),
    ("directory-size-ignored", 1, 0o700, 99, 12345, "other/dir/", set()),
]
REFUSED = [(0, 0o644, 1, 1, b"nul\0inside"), (0, 0o644, 1, 1, b""), (0, 0o10644, 1, 1, b"mode-with-type-bits"),
           (2, 0o644, 1, 1, b"symlink")]


def _hex(name):
    b = name.encode() if isinstance(name, str) else name
    return b.hex() if b else "-"


def _plan_program(tmp_path_factory, spec):
    d = tmp_path_factory.mktemp("archive_spec")
    path = d / "spec.txt"
    path.write_text(spec)
    stdout, out = _sanitized(tmp_path_factory, "archive_plan_check", lambda o: [str(path), o])
    with open(out, "rb") as f:
        return stdout, f.read()


def _octal(field):
    return int(field.rstrip(b"\0 ") or b"0", 8)


def _check_block(blk):
    """The fields every block has, read back by hand; the checksum recomputed."""
    assert len(blk) == 512
    assert blk[257:263] == b"ustar\0" and blk[263:265] == b"00"
    assert _octal(blk[108:116]) == 0 and _octal(blk[116:124]) == 0          # uid, gid
    assert blk[265:297] == bytes(32) and blk[297:329] == bytes(32)           # uname, gname
    assert blk[157:257] == bytes(100)                                        # linkname
    want = sum(blk[:148]) + 8 * 32 + sum(blk[156:])
    assert blk[148:156] == b"%06o\0 " % want


@pytest.fixture(scope="module")
def header_run(tmp_path_factory):
    spec = "".join(f"H {t} {m:o} {mt} {sz} {_hex(n)}\n" for _, t, m, mt, sz, n, _ in HEADER_CASES)
    spec += "".join(f"H {t} {m:o} {mt} {sz} {_hex(n)}\n" for t, m, mt, sz, n in REFUSED)
    stdout, _ = _plan_program(tmp_path_factory, spec)
    rows = re.findall(r"^H (\d+) (-?\d+) ([0-9a-f]*)$", stdout, re.M)
    assert len(rows) == len(HEADER_CASES) + len(REFUSED)
    return [(int(st), bytes.fromhex(h)) for _, st, h in rows]


@pytest.mark.parametrize("i", range(len(HEADER_CASES)), ids=[c[0] for c in HEADER_CASES])
def test_header_fields(header_run, i):
    label, typ, mode, mtime, size, name, pax = HEADER_CASES[i]
    st, hdr = header_run[i]
    assert st == 0 and len(hdr) % 512 == 0
    raw = name.encode()
    size = 0 if typ == 1 else size
    main = hdr[-512:]
    _check_block(main)
    assert main[156:157] == (b"5" if typ == 1 else b"0")
    assert _octal(main[100:108]) == mode
    if pax:
        x = hdr[:512]
        _check_block(x)
        assert x[156:157] == b"x" and len(hdr) == 512 + 512 * (-(-_octal(x[124:136]) // 512)) + 512
        recs = hdr[512:512 + _octal(x[124:136])]
        got, p = {}, 0
        while p < len(recs):      # "%d %s=%s\n", the length counting itself
            n = int(recs[p:recs.index(b" ", p)])
            body = recs[recs.index(b" ", p) + 1:p + n]
            assert body.endswith(b"\n")
            k, _, v = body[:-1].partition(b"=")
            got[k.decode()] = v
            p += n
        assert p == len(recs) and set(got) == pax and list(got) == sorted(got)
        assert hdr[512 + len(recs):-512] == bytes(len(hdr) - 1024 - len(recs))
        if "path" in pax:
            assert got["path"] == raw
        if "size" in pax:
            assert int(got["size"]) == size and _octal(main[124:136]) == 0
        if "mtime" in pax:
            assert int(got["mtime"]) == mtime and _octal(main[136:148]) == 0
        # its own name, as archive/tar makes it: dir/PaxHeaders.0/file, ASCII bytes only, 100 at most
        d, _, f = raw.rpartition(b"/")
        xn = (d + b"/" if d else b"") + b"PaxHeaders.0" + (b"/" + f if f else b"")
        assert x[:100].rstrip(b"\0") == bytes(c for c in xn if c < 0x80)[:100].rstrip(b"/")
    else:
        assert len(hdr) == 512
        prefix, short = main[345:500].rstrip(b"\0"), main[:100].rstrip(b"\0")
        assert (prefix + b"/" + short if prefix else short) == raw
        assert len(raw) <= 100 and not prefix or (len(prefix) <= 155 and len(short) <= 100)
    if "size" not in pax:
        assert _octal(main[124:136]) == size
    if "mtime" not in pax:
        assert _octal(main[136:148]) == mtime
    # Python's tarfile is the judge of the whole
    t = tarfile.open(fileobj=io.BytesIO(hdr + bytes(1024)), mode="r:")
    m = t.next()
    assert m.name == name.rstrip("/") and m.size == size and m.mtime == mtime and m.mode == mode
    assert m.isdir() == (typ == 1) and m.isfile() == (typ == 0) and (m.uid, m.gid, m.uname, m.gname) == (0, 0, "", "")
    assert bool(m.pax_headers) == bool(pax)


def test_names_and_modes_no_header_can_carry_are_refused(header_run):
    for st, hdr in header_run[len(HEADER_CASES):]:
        assert st == _lib.CDC_E_INVALID and hdr == b""


def _blob(i, n):
    return bytes((i * 131 + j * 7 + (j >> 8)) & 255 for j in range(n))


def _plan_case(tmp_path_factory, budget, entries):
    """entries: (type, name, [(blob id, length)]).  The program's plan, and the
    stream restated here byte by byte from its header blocks."""
    spec = "".join(f"H {t} 644 7 {sum(n for _, n in ch)} {_hex(name)}\n" for t, name, ch in entries)
    spec += f"B {budget}\n"
    spec += "".join(f"E {t} 644 7 {_hex(name)} {len(ch)} " + " ".join(f"{b} {n}" for b, n in ch) + "\n"
                    for t, name, ch in entries)
    stdout, image = _plan_program(tmp_path_factory, spec)
    hdrs = [bytes.fromhex(h) for _, _, h in re.findall(r"^H (\d+) (-?\d+) ([0-9a-f]*)$", stdout, re.M)]
    want = bytearray()
    spans = []       # (kind, entry, start, end) in the stream
    for e, ((t, name, ch), h) in enumerate(zip(entries, hdrs)):
        spans.append(("hdr", e, len(want), len(want) + len(h)))
        want += h
        size = 0
        for b, n in ch:
            if n:
                spans.append(("chunk", e, len(want), len(want) + n))
            want += _blob(b, n)
            size += n
        if size % 512:
            spans.append(("pad", e, len(want), len(want) + 512 - size % 512))
            want += bytes(512 - size % 512)
    want += bytes(1024)
    batches = [tuple(map(int, r)) for r in re.findall(r"^P (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)$", stdout, re.M)]
    segs = [tuple(map(int, r)) for r in re.findall(r"^S (\d+) (\d) (\d+) (\d+) (\d+) (\d+) (-?\d+)$", stdout, re.M)]
    return bytes(want), image, spans, batches, segs


def _check_plan(budget, entries, want, image, spans, batches, segs):
    assert image == want and len(want) % 512 == 0 and want.endswith(bytes(1024))
    at = 0
    for k, off, out_bytes, plain, nblobs, arena in batches:
        mine = [s for s in segs if s[0] == k]
        assert off == at and out_bytes == sum(s[3] for s in mine)
        assert out_bytes <= budget or len(mine) == 1, "only a single item may take a batch past the budget"
        ids = {}
        for _, ar, src, ln, dst, ent, blob in mine:
            if not ar:
                ids.setdefault((blob, ln), src)
                assert ids[(blob, ln)] == src, "a blob that occurs twice in a batch is decoded once"
        assert nblobs == len(ids) and plain == sum(ln for _, ln in ids)
        # the arena: the batch's header blocks, then one zero block
        assert arena == sum(s[3] for s in mine if s[1] and s[2] < arena - 512) + 512
        assert all(s[2] == arena - 512 and s[3] <= 512 for s in mine if s[1] and s[2] >= arena - 512)
        at += out_bytes
    assert at == len(want)
    # every item of the stream is one segment, whole in one batch: a header never straddles
    starts = {}
    for k, off, *_ in batches:
        for s in segs:
            if s[0] == k:
                starts[off + s[4]] = (k, s[3])
    items = [(a, b - a) for _, _, a, b in spans] + [(len(want) - 1024, 512), (len(want) - 512, 512)]
    assert sorted((a, starts[a][1]) for a in starts) == sorted(items)


def test_planner_against_a_byte_level_restatement(tmp_path_factory):
    ch = [(1, 700), (2, 300), (1, 700)]                       # 1,700 bytes, blob 1 twice
    small = [(0, "a.txt", ch), (1, "d", []), (0, "empty", []), (0, "b.txt", [(3, 512)]), (0, "c.txt", [(1, 700)])]
    # one batch, and budgets down to a single block
    for budget in (1 << 20, 4096 + 512, 2048, 512, 1):
        r = _plan_case(tmp_path_factory, budget, small)
        _check_plan(budget, small, *r)

    # a header in a batch's last 512 bytes: 512 header + 1,024 of file, then the next header ends the batch
    e = [(0, "x", [(1, 1024)]), (0, "y", [(2, 100)])]
    want, image, spans, batches, segs = r = _plan_case(tmp_path_factory, 2048, e)
    _check_plan(2048, e, *r)
    assert batches[0][2] == 2048 and [s[1] for s in segs if s[0] == 0][-1] == 1, "the second header closes batch 0"
    assert [s[3] for s in segs if s[0] == 0][-1] == 512

    # a padding run at a batch's start: header 512 + 1,000 of file fill the budget but for 24 bytes
    e = [(0, "x", [(1, 1000)]), (0, "y", [(2, 10)])]
    want, image, spans, batches, segs = r = _plan_case(tmp_path_factory, 1512 + 23, e)
    _check_plan(1512 + 23, e, *r)
    first = [s for s in segs if s[0] == 1][0]
    assert first[1] == 1 and first[3] == 24 and first[4] == 0 and first[5] == 0, "entry 0's padding opens batch 1"

    # a file cut into three pieces on chunk boundaries, its padding after the last
    e = [(0, "big", [(i, 900) for i in range(1, 8)]), (0, "after", [(9, 5)])]
    want, image, spans, batches, segs = r = _plan_case(tmp_path_factory, 2800, e)
    _check_plan(2800, e, *r)
    with_big = sorted({s[0] for s in segs if s[5] == 0 and not s[1]})
    assert with_big == [0, 1, 2]
    pad = [s for s in segs if s[5] == 0 and s[1] and s[3] == 512 - 6300 % 512]
    assert len(pad) == 1 and pad[0][0] == 2

    # PAX entries travel whole too
    e = [(0, "café", [(1, 100)]), (0, NAME255, [(2, 600)])]
    r = _plan_case(tmp_path_factory, 1536, e)
    _check_plan(1536, e, *r)
    t = tarfile.open(fileobj=io.BytesIO(r[0]), mode="r:")
    assert [(m.name, m.size) for m in t.getmembers()] == [("café", 100), (NAME255, 600)]
    assert t.extractfile(NAME255).read() == _blob(2, 600)


def test_archive_entry_points_check_their_arguments_before_the_device():
    L = _lib.lib()
    o = _lib.cdc_archive_opts()
    L.cdc_archive_default_opts(ctypes.byref(o))
    assert (o.struct_size, o.verify, o.format, o.compress) == (ctypes.sizeof(o), 1, _lib.CDC_ARCHIVE_TARGZ, 0)
    h = ctypes.c_void_p()
    assert L.cdc_archive_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_archive_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    for field, bad in (("struct_size", 4), ("format", 2), ("writers", -1), ("writers", 257)):
        b = _lib.cdc_archive_opts()
        L.cdc_archive_default_opts(ctypes.byref(b))
        setattr(b, field, bad)
        assert L.cdc_archive_new(0, ctypes.byref(b), ctypes.byref(h)) == _lib.CDC_E_INVALID, field
    for dev in (-1, 64):
        assert L.cdc_archive_new(dev, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_archive_run(None, None, 0, b"x", _lib.ARCHIVE_DATA_FN(), _lib.ARCHIVE_ENTRY_FN(), None, None) == \
        _lib.CDC_E_INVALID
    L.cdc_archive_free(None)
    with pytest.raises(ValueError):
        archive.ArchiveSession(format="zip")
    with pytest.raises(ValueError):
        archive.ArchiveSession(compression="ZSTD")
    with pytest.raises(ValueError):
        archive.ArchiveSession(key=b"short")
    assert archive.ArchiveEntry("d", directory=True).mode == 0o755 and archive.ArchiveEntry("f").mode == 0o644
    with pytest.raises(ValueError):
        archive.ArchiveEntry("d", obj=object(), directory=True)
