"""Grep's checks that need no GPU: the host-only pieces of
plakar_amd/csrc/grep_plan.h (the query compiler, the scalar matcher, the emit
records) under the sanitizers (tests/c/grep_plan_check.cpp), the judge of
tests/grep_ref.py against `re` and hand-worked cases, the ctypes table and the
struct layouts, the argument checks the entry points make before they touch a
device, the compiler's resource report of the new kernels, and the tile and
grid constants tests/test_grep_device.py mirrors."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import grep_ref as gref
import test_grep_device as gd
from plakar_amd import _lib, build, grep, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cdc_grep_device", "cdc_debug_set_grep_blocks", "cdc_grep_default_opts", "cdc_grep_new",
               "cdc_grep_add_packfile", "cdc_grep_add_packfile_path", "cdc_grep_add_packfiles", "cdc_grep_files",
               "cdc_grep_free"]
KERNELS = ["k_grep_scan", "k_grep_count", "k_grep_block_scan", "k_grep_rank", "k_grep_text", "k_grep_compact"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grplan") / "grep_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "grep_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_host_pieces_under_sanitizers(plan_check_exe):
    """Every bit of the first-byte set, the one-byte set, the start masks and
    the prefix bitmap of six pattern sets against a brute force, with and
    without ignore-case (12 x 65,536 prefix bits and 12 x 768 others); a
    newline, 0 and 33 patterns, lengths 0 and 257, NULL arrays and an unknown
    flag refused; the scalar matcher against a naive one on 10,000 seeded
    cases; the emit records."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) bits, (\d+) refusals, (\d+) matcher cases, (\d+) emit checks, ok", r.stdout)
    assert m, r.stdout
    bits, refusals, cases, emits = (int(g) for g in m.groups())
    assert bits == 12 * (65536 + 768) and refusals == 8 and cases == 10000 and emits == 6
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _lookahead(pattern, ignore_case):
    parts = []
    for c in pattern:
        ch = bytes([c])
        if ignore_case and ch.isalpha() and c < 0x80:
            parts.append(b"[" + ch.lower() + ch.upper() + b"]")
        else:
            parts.append(re.escape(ch))
    return re.compile(b"(?=" + b"".join(parts) + b")", re.S)


def _by_re(text, patterns, ignore_case):
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # the text is empty or ends in a newline
    hits, off = [], 0
    for no, line in enumerate(lines, 1):
        mask, nocc, col = 0, 0, None
        for k, p in enumerate(patterns):
            cols = [m.start() for m in _lookahead(p, ignore_case).finditer(line)]
            if cols:
                mask |= 1 << k
                nocc += len(cols)
                col = min(cols) if col is None else min(col, min(cols))
        if mask:
            hits.append((0, no, off, len(line), col, mask, nocc))
        off += len(line) + 1
    return hits, len(lines)


def test_judge_against_re():
    alphabet = b"abAB \r\n\n\xc9\xe9\x00@`[{.*"
    total = 0
    for seed in range(80):
        rng = random.Random(seed)
        text = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 400)))
        pats = []
        for _ in range(rng.randrange(1, 6)):
            m = rng.randrange(1, 5)
            at = rng.randrange(0, max(len(text) - m, 1))
            p = text[at:at + m].replace(b"\n", b"a") or b"a"
            pats.append(p.swapcase() if rng.random() < 0.3 else p)
        ic = bool(seed & 1)
        hits, lines, binary = gref.grep_text(text, pats, ic)
        want, nlines = _by_re(text, pats, ic)
        assert hits == want and lines == nlines and binary == (b"\0" in text), seed
        total += len(hits)
    assert total > 400


def test_judge_on_hand_worked_cases():
    assert gref.grep_text(b"aaaa", [b"aa"]) == ([(0, 1, 0, 4, 0, 1, 3)], 1, False)
    hits, lines, binary = gref.grep_text(b"x\nab\n", [b"b", b"ab"])
    assert hits == [(0, 2, 2, 2, 0, 3, 2)] and lines == 2 and not binary
    assert gref.grep_text(b"\xc9 @[{", [b"\xe9", b"`"], ignore_case=True)[0] == []  # 0xC9 | 0x20 and '@' | 0x20: no letters
    assert gref.grep_text(b"\xc9 @[", [b"\xe9", b"`", b"{"], ignore_case=True)[0] == []
    assert gref.grep_text(b"\xc9 @[`{", [b"\xe9", b"`"], ignore_case=True)[0] == [(0, 1, 0, 6, 4, 2, 1)]
    assert gref.grep_text(b"HeLLo", [b"hEllO"], ignore_case=True)[0] == [(0, 1, 0, 5, 0, 1, 1)]
    assert gref.grep_text(b"HeLLo", [b"hEllO"])[0] == []
    # lines: grep's count
    for text, n in ((b"", 0), (b"\n", 1), (b"a", 1), (b"a\n", 1), (b"a\nb", 2), (b"\n\n", 2), (b"a\r\n", 1)):
        assert gref.grep_text(text, [b"zz"])[1] == n, text
    assert gref.grep_text(b"a\r\nb", [b"\r"])[0] == [(0, 1, 0, 2, 1, 1, 1)]  # the \r belongs to the line
    # a seam: nothing of the next text or of a gap completes a match
    buf = b"xabc"
    assert gref.grep_buffer(buf, [(0, 3), (3, 1)], [b"abc"])[0] == []
    assert gref.grep_buffer(buf, [(0, 3), (3, 1)], [b"ab", b"c"])[0] == [(0, 1, 0, 3, 1, 1, 1), (1, 1, 3, 1, 0, 2, 1)]
    hits, lines, matched, binary = gref.grep_buffer(b"a\na\na\n\0", [(0, 6), (6, 1)], [b"a"], limit=2)
    assert [h[1] for h in hits] == [1, 2] and matched == [3, 0] and lines == [3, 1] and binary == [False, True]
    assert gref.text_of(b"hello\nworld\n", gref.grep_text(b"hello\nworld\n", [b"o"])[0], 4) == b"hell\nworl\n"
    with pytest.raises(ValueError):
        gref.grep_text(b"a", [b"a\nb"])
    with pytest.raises(ValueError):
        gref.grep_text(b"a", [])
    with pytest.raises(ValueError):
        gref.grep_text(b"a", [b"a"] * 33)
    with pytest.raises(ValueError):
        gref.grep_text(b"a", [b"a" * 257])


def test_lib_exports_the_new_symbols_and_layouts():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "plakar_cdc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define CDC_GREP_IGNORE_CASE\s+1u\b", header) and _lib.GREP_IGNORE_CASE == 1
    hit = _lib.cdc_grep_hit
    assert ctypes.sizeof(hit) == 32 == grep.HIT_DTYPE.itemsize
    offsets = [("text", 0), ("line", 4), ("off", 8), ("len", 16), ("col", 20), ("mask", 24), ("nocc", 28)]
    assert [(n, getattr(hit, n).offset) for n, _ in hit._fields_] == offsets
    assert [(n, grep.HIT_DTYPE.fields[n][1]) for n in grep.HIT_DTYPE.names] == offsets
    assert ctypes.sizeof(_lib.cdc_grep_opts) == 40 and ctypes.sizeof(_lib.cdc_grep_query) == 48
    assert ctypes.sizeof(_lib.cdc_grep_result) == 80 and ctypes.sizeof(_lib.cdc_grep_stats) == 8 + 14 * 8 + 11 * 8
    res = _lib.cdc_grep_result
    assert [getattr(res, n).offset for n, _ in res._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    o = _lib.cdc_grep_opts()
    o.threads = 5
    L.cdc_grep_default_opts(ctypes.byref(o))
    assert (o.struct_size, o.compress, o.key, o.threads, o.batch_bytes, o.max_lines) == (40, 0, None, 0, 0, 0)
    L.cdc_grep_default_opts(None)
    for name in ("GrepSession", "grep_files"):
        assert hasattr(grep, name) and name in snapshot.__all__ and getattr(snapshot, name) is getattr(grep, name)
    assert callable(grep.grep_device)
    import plakar_amd
    assert "grep" in plakar_amd.__all__


def _u64(*v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def _pats(*ps):
    bufs = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in ps]
    ptrs = (ctypes.c_void_p * max(len(ps), 1))(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_uint32 * max(len(ps), 1))(*[len(p) for p in ps])
    return bufs, ptrs, lens


def test_device_call_rejects_bad_arguments_before_the_device():
    """Run without a GPU, a call that reached for a device would be
    CDC_E_DEVICE or CDC_E_NOT_INIT, not CDC_E_INVALID."""
    L = _lib.lib()
    data, hits = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)  # never dereferenced
    keep, ptrs, lens = _pats(b"ab", b"c")
    lines, matched, total = _u64(0, 0), _u64(0, 0), ctypes.c_uint64()
    binary = (ctypes.c_uint8 * 2)()
    good = dict(device=0, d_data=data, len=4096, text_off=_u64(0, 100), text_len=_u64(100, 3996), n=2, patterns=ptrs,
                pattern_len=lens, npatterns=2, flags=0, limit=0, d_hits=hits, cap=10, lines=lines, matched=matched,
                binary=binary, total=ctypes.byref(total), stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.cdc_grep_device(*[a[k] for k in good])

    for name, bad in [("device", -1), ("device", 64), ("text_off", None), ("text_len", None), ("d_data", None),
                      ("d_hits", None), ("d_hits", ctypes.c_void_p((2 << 20) + 8)), ("text_len", _u64(100, 3997)),
                      ("text_off", _u64(0, 4097)), ("text_len", _u64(100, 2 ** 64 - 50)),
                      ("text_off", _u64(0, 99)),      # the texts overlap
                      ("text_off", _u64(200, 100)),   # they do not ascend
                      ("patterns", None), ("pattern_len", None), ("npatterns", 0), ("npatterns", 33), ("flags", 2),
                      ("flags", 0x80000001)]:
        assert call(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert call(len=2 ** 33, text_len=_u64(100, 2 ** 32)) == _lib.CDC_E_INVALID  # a text of 4 GiB
    assert call(len=2 ** 33, text_off=_u64(0, 2 ** 31), text_len=_u64(2 ** 31, 2 ** 31)) == _lib.CDC_E_INVALID  # too many lines possible
    for bad in (b"", b"x" * 257, b"a\nb", b"\n"):
        k2, p2, l2 = _pats(b"ab", bad)
        assert call(patterns=p2, pattern_len=l2) == _lib.CDC_E_INVALID, bad
    k3, p3, l3 = _pats(b"ab", b"x" * 256, b"\0")
    st = call(patterns=p3, pattern_len=l3, npatterns=3, n=0)
    assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
    k33, p33, l33 = _pats(*[b"p"] * 33)
    assert call(patterns=p33, pattern_len=l33, npatterns=33) == _lib.CDC_E_INVALID
    if not _has_gpu():
        assert call() == _lib.CDC_E_NOT_INIT and call(n=0) == _lib.CDC_E_NOT_INIT
        assert call(flags=1, limit=3, cap=0, d_hits=None, lines=None, matched=None, binary=None, total=None) == _lib.CDC_E_NOT_INIT
    assert L.cdc_debug_set_grep_blocks(3) == _lib.CDC_OK and L.cdc_debug_set_grep_blocks(0) == _lib.CDC_OK


def test_grep_context_argument_checks_without_a_device():
    L = _lib.lib()
    o = _lib.cdc_grep_opts()
    L.cdc_grep_default_opts(ctypes.byref(o))
    h = ctypes.c_void_p()
    assert L.cdc_grep_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_grep_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    assert L.cdc_grep_new(-1, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_grep_new(64, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    for field, bad in [("struct_size", 0), ("struct_size", o.struct_size + 8), ("threads", -1), ("threads", 257),
                       ("batch_bytes", (1 << 30) + 1), ("max_lines", (1 << 31) + 1), ("compress", 7)]:
        keep = getattr(o, field)
        setattr(o, field, bad)
        assert L.cdc_grep_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID, field
        assert not h.value
        setattr(o, field, keep)
    st = L.cdc_grep_new(0, ctypes.byref(o), ctypes.byref(h))
    if _has_gpu():  # an earlier test of the run may have initialised the library
        assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
        L.cdc_grep_free(h)
    else:
        assert st == _lib.CDC_E_NOT_INIT and not h.value
    f = (_lib.cdc_check_file * 1)()
    q = _lib.cdc_grep_query()
    cb = _lib.GREP_FILE_FN(lambda ctx, r: None)
    assert L.cdc_grep_files(None, ctypes.byref(q), f, 1, cb, None, None) == _lib.CDC_E_INVALID
    assert L.cdc_grep_add_packfile(None, b"x", 1) == _lib.CDC_E_INVALID
    assert L.cdc_grep_add_packfile_path(None, b"/nonexistent") == _lib.CDC_E_INVALID
    assert L.cdc_grep_add_packfiles(None, None, 0, None) == _lib.CDC_E_INVALID
    L.cdc_grep_free(None)
    with pytest.raises(ValueError):
        grep.GrepSession(key=b"short")


def test_new_kernels_use_no_private_segment():
    path = build.resources_path()
    assert os.path.exists(path), f"{path}: the library is built by plakar_amd.build, which keeps the compiler's report"
    text = open(path).read()
    for k in KERNELS:
        m = re.search(r"Function Name: \S*%s\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)" % k, text, re.S)
        assert m, k
        assert (int(m.group(1)), int(m.group(2))) == (0, 0), (k, m.groups())
    # the scan's LDS: the query block, the tile with its halo, the wave sums; four workgroups fit a CU's 160 KiB
    m = re.search(r"Function Name: \S*k_grep_scan\S*.*?LDS Size \[bytes/block\]: (\d+)", text, re.S)
    assert m and int(m.group(1)) == 34432 and 4 * int(m.group(1)) <= 160 * 1024
    assert "34,432" in open(os.path.join(ROOT, "DESIGN.md")).read()


def _constant(text, name):
    """The value of `constexpr <type> ... name = <integer expression>`."""
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
    assert m, f"no constexpr {name}"
    expr = re.sub(r"(\d)[uUlL]+\b", r"\1", m.group(1)).strip()
    for known, value in (("kThreads", "256"),):
        expr = re.sub(r"\b%s\b" % known, value, expr)
    assert re.fullmatch(r"[\d\s<>*+()xXa-fA-F-]+", expr), f"{name} = {m.group(1)!r} is not an integer expression"
    return int(eval(expr, {"__builtins__": {}}))  # digits, shifts, products and sums only


def test_the_constants_the_device_tests_mirror():
    src = open(os.path.join(ROOT, "plakar_amd", "csrc", "cdc_grep.hip")).read()
    for name, want in gd.MIRRORED.items():
        assert _constant(src, name) == want, f"cdc_grep.hip: {name} changed: set it in tests/test_grep_device.py and resize its cases"
    assert re.search(r"device_cus\(device\)\)\s*\*\s*uint64_t\(per_cu\)", src)
    assert re.search(r"grid_for\(device, ntiles, kScanBlocksPerCU\)", src)
    plan = open(os.path.join(ROOT, "plakar_amd", "csrc", "grep_plan.h")).read()
    assert _constant(plan, "kMaxPatternLen") == gd.MIRRORED["kHalo"] + 1


def test_python_layer_is_importable_without_a_device():
    assert np.dtype(grep.HIT_DTYPE).names == ("text", "line", "off", "len", "col", "mask", "nocc")
    P = grep._Patterns([b"ab", b"\0"])
    assert P.n == 2 and list(P.lens) == [2, 1]
    assert grep._Patterns(b"solo").raw == [b"solo"]
