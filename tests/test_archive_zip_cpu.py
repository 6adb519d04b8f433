"""Zip's checks that need no GPU.  The container and the batch planner
(tests/c/zip_plan_check.cpp over plakar_amd/csrc/zip_plan.h, built under the
address and undefined-behaviour sanitizers and run as a program): every local
header case read back by hand, the planner against a byte-level restatement,
the central directory and the end records of synthetic records (sizes, an
offset and entry counts past the 32- and 16-bit fields) read with struct and
by zipfile over a sparse file that holds only the tail at its true offset.
Then the entry points' argument checks before the device and the compiler's
resource report of the new kernels."""
import ctypes
import os
import re
import struct
import subprocess
import time
import zipfile

import pytest

from plakar_amd import _lib, archive, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX32, MAX16 = 0xFFFFFFFF, 0xFFFF
KMAXBLOB = 0x7FFFFFFF

_built = {}


def _program(tmp_path_factory, spec):
    """Build tests/c/zip_plan_check.cpp with the sanitizers (once) and run it over the spec: (stdout, OUT's bytes)."""
    d = tmp_path_factory.mktemp("zip_plan")
    name = "zip_plan_check"
    if name not in _built:
        exe = str(d / name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
               os.path.join(ROOT, "tests", "c", name + ".cpp")]
        subprocess.run(cmd, check=True)
        _built[name] = exe
    path, out = d / "spec.txt", str(d / "out.bin")
    path.write_text(spec)
    r = subprocess.run([_built[name], str(path), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok")
    with open(out, "rb") as f:
        return r.stdout, f.read()


def _hex(name):
    b = name.encode() if isinstance(name, str) else name
    return b.hex() if b else "-"


# ---- local headers ------------------------------------------------------------------------------
LONGEST = "n" * 65535
HEADER_CASES = [  # (label, mode, mtime, name, trimmed name, wants the UTF-8 flag)
    ("plain", 0o644, 1_700_000_000, "a.txt", "a.txt", False),
    ("leading-slashes", 0o600, 1_700_000_000, "//abs/path", "abs/path", False),
    ("non-ascii", 0o644, 1_700_000_000, "café/naïve.txt", "café/naïve.txt", True),
    ("tilde", 0o644, 12, "a~b", "a~b", True),                    # above 0x7d
    ("closing-brace", 0o644, 12, "a}b", "a}b", False),           # 0x7d itself needs no flag
    ("backslash", 0o644, 12, "a\\b", "a\\b", True),
    ("control", 0o644, 12, "a\x01b", "a\x01b", True),
    ("not-utf8", 0o644, 12, b"\xff\xfe.bin", b"\xff\xfe.bin", False),
    ("overlong", 0o644, 12, b"\xc0\xaf", b"\xc0\xaf", False),
    ("surrogate", 0o644, 12, b"\xed\xa0\x80", b"\xed\xa0\x80", False),
    ("cut-short", 0o644, 12, b"ab\xe2\x82", b"ab\xe2\x82", False),
    ("four-bytes", 0o644, 12, "\U0001F600", "\U0001F600", True),
    ("odd-second", 0o644, 1_700_000_001, "odd", "odd", False),
    ("dos-epoch", 0o644, 315_532_800, "epoch", "epoch", False),
    ("before-1980", 0o644, 100, "old", "old", False),
    ("negative", 0o644, -5, "older", "older", False),
    ("past-2107", 0o644, 5_000_000_000, "far", "far", False),
    ("end-of-2107", 0o644, 4_354_819_199, "edge", "edge", False),
    ("all-mode-bits", 0o7777, 12, "m", "m", False),
    ("no-owner-write", 0o444, 12, "ro", "ro", False),
    ("name-65535", 0o644, 12, LONGEST, LONGEST, False),
    ("name-65535-after-trimming", 0o644, 12, "/" + LONGEST, LONGEST, False),
]
REFUSED = [(0o644, 1, b""), (0o644, 1, b"///"), (0o644, 1, b"nul\0inside"), (0o10644, 1, b"mode-with-type-bits"),
           (0o644, 1, b"n" * 65536)]


def _dos(mtime):
    t = time.gmtime(mtime)
    if t.tm_year < 1980:
        return (1 << 5) | 1, 0
    if t.tm_year > 2107:
        return (127 << 9) | (12 << 5) | 31, (23 << 11) | (59 << 5) | 29
    return ((t.tm_year - 1980) << 9) | (t.tm_mon << 5) | t.tm_mday, (t.tm_hour << 11) | (t.tm_min << 5) | (t.tm_sec // 2)


@pytest.fixture(scope="module")
def header_run(tmp_path_factory):
    spec = "".join(f"H {m:o} {mt} {_hex(n)}\n" for _, m, mt, n, _, _ in HEADER_CASES)
    spec += "".join(f"H {m:o} {mt} {_hex(n)}\n" for m, mt, n in REFUSED)
    stdout, _ = _program(tmp_path_factory, spec)
    rows = re.findall(r"^H (\d+) (-?\d+) (\d+) (\d+) (\d+) ([0-9a-f]*)$", stdout, re.M)
    assert len(rows) == len(HEADER_CASES) + len(REFUSED)
    return [(int(st), int(fl), int(d), int(t), bytes.fromhex(h)) for _, st, fl, d, t, h in rows]


@pytest.mark.parametrize("i", range(len(HEADER_CASES)), ids=[c[0] for c in HEADER_CASES])
def test_local_header_fields(header_run, i):
    label, mode, mtime, name, trimmed, utf8 = HEADER_CASES[i]
    st, flags, date, tm, hdr = header_run[i]
    raw = trimmed.encode() if isinstance(trimmed, str) else trimmed
    assert st == 0 and len(hdr) == 30 + len(raw) + 9
    sig, ver, fl, method, t, d, crc, cs, us, nlen, xlen = struct.unpack("<IHHHHHIIIHH", hdr[:30])
    assert (sig, ver, method) == (0x04034B50, 20, 8)
    assert fl == flags == (0x0808 if utf8 else 0x0008)
    assert (crc, cs, us) == (0, 0, 0), "the descriptor carries them"
    assert (nlen, xlen) == (len(raw), 9) and hdr[30:30 + nlen] == raw
    assert hdr[30 + nlen:] == b"UT\x05\x00\x01" + struct.pack("<I", mtime & MAX32)
    assert (d, t) == (date, tm) == _dos(mtime)
    if label == "before-1980" or label == "negative":
        assert (d, t) == (0x0021, 0)                       # 1980-01-01 00:00:00
    if label == "odd-second":
        assert t & 31 == (1_700_000_001 % 60) // 2          # two-second resolution: the odd second is dropped


def test_names_and_modes_no_header_can_carry_are_refused(header_run):
    for st, _, _, _, hdr in header_run[len(HEADER_CASES):]:
        assert st == _lib.CDC_E_INVALID and hdr == b""


# ---- the planner ----------------------------------------------------------------------------------
def _blob(i, n):
    return bytes((i * 131 + j * 7 + (j >> 8)) & 255 for j in range(n))


def _plan_case(tmp_path_factory, budget, entries):
    """entries: (name, [(blob id, length)]).  The program's plan and each batch's (header arena, image)."""
    spec = "".join(f"H 644 7 {_hex(name)}\n" for name, _ in entries) + f"B {budget}\n"
    spec += "".join(f"E 644 7 {_hex(name)} {len(ch)} " + " ".join(f"{b} {n}" for b, n in ch) + "\n" for name, ch in entries)
    stdout, out = _program(tmp_path_factory, spec)
    hdrs = [bytes.fromhex(r[-1]) for r in re.findall(r"^H (\d+) (-?\d+) (\d+) (\d+) (\d+) ([0-9a-f]*)$", stdout, re.M)]
    batches = [tuple(map(int, r)) for r in re.findall(r"^P (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)$", stdout, re.M)]
    segs = [tuple(map(int, r)) for r in re.findall(r"^S (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)$", stdout, re.M)]
    pieces = [tuple(map(int, r)) for r in re.findall(r"^Q (\d+) (\d+) (\d) (\d) (\d+) (\d+) (\d+) (\d+)$", stdout, re.M)]
    blobs, p = [], 0
    for _ in batches:
        pair = []
        for _ in range(2):
            (n,) = struct.unpack_from("<Q", out, p)
            pair.append(out[p + 8:p + 8 + n])
            p += 8 + n
        blobs.append(tuple(pair))
    assert p == len(out)
    return hdrs, batches, segs, pieces, blobs


def _check_plan(budget, entries, hdrs, batches, segs, pieces, blobs):
    # the items in archive order: (entry, "hdr" or chunk index, bytes)
    items = []
    for e, (name, ch) in enumerate(entries):
        items.append((e, "hdr", hdrs[e]))
        items += [(e, c, _blob(b, n)) for c, (b, n) in enumerate(ch) if n]
    at = 0                    # the next item
    open_entry = None         # the entry a batch's first piece continues
    for k, used, img_bytes, plain, nblobs, hdr_bytes in batches:
        arena, image = blobs[k]
        assert len(arena) == hdr_bytes and len(image) == img_bytes
        mine = [q for q in pieces if q[0] == k]
        assert mine, "no empty batch"
        n_items, img_at = 0, 0
        for j, (_, e, first, last, img_off, ln, hoff, hlen) in enumerate(mine):
            assert img_off == img_at, "the image is file bytes back to back: no headers, no padding"
            if first:
                assert items[at] == (e, "hdr", arena[hoff:hoff + hlen]), "a header is whole in its batch's arena"
                at += 1
                n_items += 1
            else:
                assert j == 0 and e == open_entry and ln > 0, "only a batch's first piece continues an entry"
            got = b""
            while len(got) < ln:              # whole chunks only
                ie, c, data = items[at]
                assert ie == e and c != "hdr"
                got += data
                at += 1
                n_items += 1
            assert got == image[img_off:img_off + ln], "a piece is whole chunks of its entry, in order"
            more = at < len(items) and items[at][0] == e
            assert bool(last) == (not more), "the last chunk is in the last piece, and only there"
            if not last:
                assert j == len(mine) - 1, "an entry goes on only in the next batch"
            open_entry = None if last else e
            img_at += ln
        assert img_at == img_bytes
        assert used == sum(q[7] for q in mine if q[2]) + img_bytes
        assert used <= budget or n_items == 1, "only a single item may take a batch past the budget"
        if at < len(items):
            assert used + len(items[at][2]) > budget, "a batch ends only when the next item does not fit"
        ids = {}
        for _, src, ln, dst, ent, blob in (s for s in segs if s[0] == k):
            ids.setdefault((blob, ln), src)
            assert ids[(blob, ln)] == src, "a blob that occurs twice in a batch is decoded once"
        assert nblobs == len(ids) and plain == sum(ln for _, ln in ids)
        off = 0
        for (_, ln), src in ids.items():      # in order of first use
            assert src == off, "distinct blobs back to back in order of first use"
            off += ln
    assert at == len(items) and open_entry is None


def test_planner_against_a_byte_level_restatement(tmp_path_factory):
    ch = [(1, 700), (2, 300), (1, 700)]                       # 1,700 bytes, blob 1 twice
    small = [("a.txt", ch), ("empty", []), ("b.txt", [(3, 512)]), ("c.txt", [(1, 700)]), ("zero-chunks", [(4, 0), (5, 9), (6, 0)])]
    hl = 30 + 9
    for budget in (1 << 20, 2048, 1700 + hl + 5, 700 + hl + 5, 700, 512, 1):
        r = _plan_case(tmp_path_factory, budget, small)
        _check_plan(budget, small, *r)
    one = _plan_case(tmp_path_factory, 1 << 20, small)
    assert len(one[1]) == 1 and all(q[2] and q[3] for q in one[3]), "one batch: every entry is one piece, first and last"
    assert [q[5] for q in one[3]] == [1700, 0, 512, 700, 9]

    # a file cut into three pieces on chunk boundaries
    e = [("big", [(i, 900) for i in range(1, 8)]), ("after", [(9, 5)])]
    hdrs, batches, segs, pieces, blobs = r = _plan_case(tmp_path_factory, 2800, e)
    _check_plan(2800, e, *r)
    big = [q for q in pieces if q[1] == 0]
    assert [(q[2], q[3], q[5]) for q in big] == [(1, 0, 2700), (0, 0, 2700), (0, 1, 900)]

    # a header that fits where its first chunk does not: a piece that is only the header
    e = [("x", [(1, 1000)]), ("y", [(2, 500)])]
    hx = 30 + 1 + 9
    hdrs, batches, segs, pieces, blobs = r = _plan_case(tmp_path_factory, 1000 + 2 * hx + 10, e)
    _check_plan(1000 + 2 * hx + 10, e, *r)
    assert [(q[0], q[1], q[2], q[3], q[5]) for q in pieces] == [(0, 0, 1, 1, 1000), (0, 1, 1, 0, 0), (1, 1, 0, 1, 500)]

    # a header that does not fit closes the batch whole
    hdrs, batches, segs, pieces, blobs = r = _plan_case(tmp_path_factory, 1000 + hx + 10, e)
    _check_plan(1000 + hx + 10, e, *r)
    assert [(q[0], q[1], q[2], q[3]) for q in pieces] == [(0, 0, 1, 1), (1, 1, 1, 1)]


def test_detect_utf8_alone(tmp_path_factory):
    cases = [(b"plain", (1, 0)), ("é".encode(), (1, 1)), (b"\x80", (0, 0)), (b"\xf4\x90\x80\x80", (0, 0)),
             (b"\xf4\x8f\xbf\xbf", (1, 1)), (b"\xe0\x9f\xbf", (0, 0)), (b"\xef\xbf\xbd", (1, 1)), (b"~", (1, 1)), (b"}", (1, 0))]
    stdout, _ = _program(tmp_path_factory, "".join(f"U {_hex(n)}\n" for n, _ in cases))
    assert [tuple(map(int, r)) for r in re.findall(r"^U (\d) (\d)$", stdout, re.M)] == [w for _, w in cases]


# ---- the central directory and the end records ------------------------------------------------------
def _read_tail(tail, offset):
    """The tail by hand: (central records, end fields)."""
    recs, p = [], 0
    while tail[p:p + 4] == b"PK\x01\x02":
        (_, creator, reader, flags, method, t, d, crc, cs, us, nlen, xlen, clen, disk, iattr, xattr,
         off) = struct.unpack_from("<IHHHHHHIIIHHHHHII", tail, p)
        name = tail[p + 46:p + 46 + nlen]
        extra = tail[p + 46 + nlen:p + 46 + nlen + xlen]
        recs.append(dict(creator=creator, reader=reader, flags=flags, method=method, time=t, date=d, crc=crc, cs=cs, us=us,
                         name=name, extra=extra, xattr=xattr, off=off))
        assert (clen, disk, iattr) == (0, 0, 0)
        p += 46 + nlen + xlen
    end = dict(dir_size=p, z64=None)
    if tail[p:p + 4] == b"PK\x06\x06":
        sig, sz, made, need, d0, d1, n0, n1, size, off = struct.unpack_from("<IQHHIIQQQQ", tail, p)
        assert (sz, made, need, d0, d1) == (44, 45, 45, 0, 0) and n0 == n1
        end["z64"] = (n0, size, off)
        p += 56
        sig, d0, where, disks = struct.unpack_from("<IIQI", tail, p)
        assert (sig, d0, disks) == (0x07064B50, 0, 1) and where == offset + end["dir_size"], "the locator points at the zip64 record"
        p += 20
    sig, d0, d1, n0, n1, size, off, clen = struct.unpack_from("<IHHHHIIH", tail, p)
    assert (sig, d0, d1, clen) == (0x06054B50, 0, 0, 0) and n0 == n1 and p + 22 == len(tail)
    end["plain"] = (n0, size, off)
    return recs, end


def _zipfile_over_tail(tmp_path, tail, offset):
    path = tmp_path / f"tail{offset}.zip"
    with open(path, "wb") as f:       # sparse: only the tail is written, at its true offset
        f.seek(offset)
        f.write(tail)
    with zipfile.ZipFile(path) as z:
        infos = z.infolist()
    os.unlink(path)
    return infos


def _tail(tmp_path_factory, records, generated, offset):
    spec = "".join(f"R {m:o} {mt} {_hex(n)} {crc} {cs} {us} {off}\n" for n, m, mt, crc, cs, us, off in records)
    spec += (f"N {generated}\n" if generated else "") + f"D {offset}\n"
    return _program(tmp_path_factory, spec)[1]


def test_a_small_directory_is_all_32_bit(tmp_path_factory, tmp_path):
    records = [("a.txt", 0o644, 1_700_000_001, 0xDEADBEEF, 10, 20, 0), ("café", 0o400, 100, 7, MAX32 - 1, MAX32 - 1, 90)]
    offset = MAX32 - 1
    tail = _tail(tmp_path_factory, records, 0, offset)
    recs, end = _read_tail(tail, offset)
    assert end["z64"] is None and end["plain"] == (2, end["dir_size"], offset)
    for r, (n, m, mt, crc, cs, us, off) in zip(recs, records):
        assert (r["creator"], r["reader"], r["method"]) == (0x0314, 20, 8)
        assert (r["crc"], r["cs"], r["us"], r["off"], r["name"]) == (crc, cs, us, off, n.encode())
        assert r["extra"] == b"UT\x05\x00\x01" + struct.pack("<I", mt)
        assert r["xattr"] == ((0o100000 | m) << 16) | (0 if m & 0o200 else 1)
        assert (r["date"], r["time"]) == _dos(mt)
    assert recs[0]["flags"] == 0x0008 and recs[1]["flags"] == 0x0808
    infos = _zipfile_over_tail(tmp_path, tail, offset)
    assert [(i.filename, i.CRC, i.compress_size, i.file_size, i.header_offset) for i in infos] == \
        [(n, crc, cs, us, off) for n, _, _, crc, cs, us, off in records]
    assert [i.external_attr for i in infos] == [0o100644 << 16, (0o100400 << 16) | 1]
    assert all(i.create_system == 3 and i.create_version == 20 and i.extract_version == 20 for i in infos)
    assert infos[0].date_time == (2023, 11, 14, 22, 13, 20) and infos[1].date_time == (1980, 1, 1, 0, 0, 0)


def test_sizes_and_offsets_past_32_bits_take_the_zip64_forms(tmp_path_factory, tmp_path):
    big = 5 << 30
    records = [("csize-edge", 0o644, 12, 1, MAX32, 77, 0),                 # exactly 0xFFFFFFFF is already zip64
               ("usize-big", 0o644, 12, 2, 1000, big, MAX32 + 100),
               ("offset-only", 0o600, 12, 3, 10, 20, MAX32 + 2000),
               ("offset-edge", 0o600, 12, 4, 10, 20, MAX32)]
    offset = MAX32 + 5000
    tail = _tail(tmp_path_factory, records, 0, offset)
    recs, end = _read_tail(tail, offset)
    for r, (n, m, mt, crc, cs, us, off) in zip(recs, records):
        assert (r["cs"], r["us"], r["off"]) == (MAX32, MAX32, MAX32), "all three fields saturate together"
        assert r["extra"] == struct.pack("<HHQQQ", 1, 24, us, cs, off) + b"UT\x05\x00\x01" + struct.pack("<I", mt), \
            "the zip64 extra stands in front of the timestamp"
        assert r["reader"] == (45 if cs >= MAX32 or us >= MAX32 else 20) and r["creator"] == 0x0314
    assert end["z64"] == (4, end["dir_size"], offset) and end["plain"] == (MAX16, MAX32, MAX32), \
        "the plain record holds the saturated values"
    infos = _zipfile_over_tail(tmp_path, tail, offset)
    assert [(i.filename, i.CRC, i.compress_size, i.file_size, i.header_offset) for i in infos] == \
        [(n, crc, cs, us, off) for n, _, _, crc, cs, us, off in records]


@pytest.mark.parametrize("count", [65534, 65535, 65536])
def test_entry_counts_around_the_16_bit_field(tmp_path_factory, tmp_path, count):
    offset = count * 64
    tail = _tail(tmp_path_factory, [], count, offset)
    recs, end = _read_tail(tail, offset)
    assert len(recs) == count and end["dir_size"] == count * (46 + 8 + 9)
    if count >= MAX16:
        assert end["z64"] == (count, end["dir_size"], offset) and end["plain"] == (MAX16, MAX32, MAX32)
    else:
        assert end["z64"] is None and end["plain"] == (count, end["dir_size"], offset)
    assert [r["off"] for r in recs[:3]] == [0, 64, 128] and recs[-1]["name"] == b"e%07d" % (count - 1)
    infos = _zipfile_over_tail(tmp_path, tail, offset)
    assert len(infos) == count and infos[-1].filename == "e%07d" % (count - 1) and infos[-1].header_offset == (count - 1) * 64


def test_no_records_is_the_22_byte_end_record(tmp_path_factory, tmp_path):
    tail = _tail(tmp_path_factory, [], 0, 0)
    assert tail == b"PK\x05\x06" + bytes(18)
    assert _zipfile_over_tail(tmp_path, tail, 0) == []


# ---- the entry points' argument checks, before the device --------------------------------------------
def test_zip_constructor_checks_its_arguments_before_the_device():
    L = _lib.lib()
    o = _lib.cdc_archive_opts()
    L.cdc_archive_default_opts(ctypes.byref(o))
    h = ctypes.c_void_p()
    assert L.cdc_archive_new_zip(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_archive_new_zip(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    for field, bad in (("struct_size", 4), ("writers", -1), ("writers", 257)):
        b = _lib.cdc_archive_opts()
        L.cdc_archive_default_opts(ctypes.byref(b))
        setattr(b, field, bad)
        assert L.cdc_archive_new_zip(0, ctypes.byref(b), ctypes.byref(h)) == _lib.CDC_E_INVALID, field
    for dev in (-1, 64):
        assert L.cdc_archive_new_zip(dev, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    # format is not read: a value cdc_archive_new refuses is not an argument error here
    b = _lib.cdc_archive_opts()
    L.cdc_archive_default_opts(ctypes.byref(b))
    b.format = 2
    assert L.cdc_archive_new(0, ctypes.byref(b), ctypes.byref(h)) == _lib.CDC_E_INVALID
    st = L.cdc_archive_new_zip(0, ctypes.byref(b), ctypes.byref(h))
    assert st != _lib.CDC_E_INVALID
    if st == _lib.CDC_OK:
        L.cdc_archive_free(h)
    with pytest.raises(ValueError):
        archive.ZipSession(compression="ZSTD")
    with pytest.raises(ValueError):
        archive.ZipSession(key=b"short")
    assert L.cdc_abi_version() == 1
    assert {"ZipSession", "zip_files", "zip_pieces_device"} <= set(archive.__all__)


def test_zip_pieces_checks_its_arguments_before_the_device():
    L = _lib.lib()
    buf = ctypes.c_void_p(4096)                # never dereferenced: every call below ends on its arguments
    hdr = bytes(64)
    pc = (_lib.cdc_zip_piece * 2)()
    outs = (_lib.cdc_zip_piece_out * 2)()
    total = ctypes.c_uint64(7)

    def call(pieces=pc, n=1, src=buf, src_cap=1 << 40, hdrs=hdr, hdr_len=64, out=buf, o=outs, tot=None, device=0):
        return L.cdc_zip_pieces_device(device, src, src_cap, pieces, n, hdrs, hdr_len, out, 1 << 40, o,
                                       ctypes.byref(total) if tot is None else tot, None)

    def piece(i, **kw):
        ctypes.memset(ctypes.byref(pc[i]), 0, ctypes.sizeof(pc[i]))
        for k, v in dict(dict(len=1, first=1, last=1, hdr_len=30, crc_reg=MAX32), **kw).items():
            setattr(pc[i], k, v)

    piece(0)
    assert call(tot=ctypes.POINTER(ctypes.c_uint64)()) == _lib.CDC_E_INVALID
    assert call(pieces=ctypes.POINTER(_lib.cdc_zip_piece)()) == _lib.CDC_E_INVALID
    assert call(o=ctypes.POINTER(_lib.cdc_zip_piece_out)()) == _lib.CDC_E_INVALID
    assert call(src=None) == _lib.CDC_E_INVALID
    assert call(hdrs=None) == _lib.CDC_E_INVALID
    assert call(out=None) == _lib.CDC_E_INVALID
    for dev in (-1, 64):
        assert call(device=dev) == _lib.CDC_E_INVALID
    # no pieces: nothing to do, nothing needed
    total.value = 7
    assert L.cdc_zip_pieces_device(0, None, 0, None, 0, None, 0, None, 0, None, ctypes.byref(total), None) == _lib.CDC_OK
    assert total.value == 0
    piece(0, len=KMAXBLOB + 1)
    assert call() == _lib.CDC_E_UNSUPPORTED, "a piece's bit positions and spans are planned like a blob's"
    piece(0)
    piece(1, len=(1 << 32) + 5, first=0, hdr_len=0)
    assert call(n=2) == _lib.CDC_E_UNSUPPORTED
    piece(0, hdr_len=0)
    assert call() == _lib.CDC_E_INVALID, "a first piece has its header"
    piece(0, hdr_off=40, hdr_len=30)
    assert call() == _lib.CDC_E_INVALID, "a header inside the arena"
    piece(0, src_off=100, len=50)
    assert call(src_cap=149) == _lib.CDC_E_INVALID, "a piece inside the source"


# ---- the compiler's resource report -------------------------------------------------------------------
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


@pytest.mark.parametrize("name", ["k_zip_plan", "k_zip_place", "k_zip_fin"])
def test_zip_kernel_resources(name):
    ks = {k: v for k, v in _report().items() if k.startswith(f"_ZN3enc{len(name)}{name}E")}
    assert len(ks) == 1, f"{name} is not in the resource report"
    (k,) = ks.values()
    assert int(k["ScratchSize [bytes/lane]"]) == 0
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0
