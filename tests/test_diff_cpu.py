"""Diff's tests that need no GPU: cdc_diff_script against difflib's grouped
opcodes and the emit plan's text against difflib's unified diff over the same
cases (diff_ref.id_cases), the argument checks every new entry point makes
before it touches the device, the defaults, the Python layer's ValueErrors,
the new kernels' lines in the compiler's resource report, and the stand-alone
sanitizer program over the matcher, the emit planner and the id re-leading
(tests/c/diff_plan_check.cpp)."""
import ctypes
import difflib
import os
import re
import subprocess

import numpy as np
import pytest

import diff_ref
from plakar_amd import _lib, diff, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = diff_ref.id_cases()
CONTEXTS = (0, 1, 3)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - no torch, no device
        return False


def _grouped(a, b, n):
    return [list(g) for g in difflib.SequenceMatcher(None, a, b).get_grouped_opcodes(n)]


def test_case_list_is_what_it_says():
    names = [c[0] for c in CASES]
    assert len(CASES) >= 225 and sum(n.startswith("random") for n in names) == 200
    for nb, junk in ((199, False), (200, True), (201, True)):
        (_, a, b), = [c for c in CASES if c[0] == f"popular id, len(b)={nb}"]
        assert len(b) == nb and (1 not in difflib.SequenceMatcher(None, a, b).b2j) == junk
    # the popular rule shows in the opcodes of these cases: without autojunk they differ
    (_, a, b), = [c for c in CASES if c[0] == "every third line is }"]
    assert len(a) == 3000 and 0 in difflib.SequenceMatcher(None, a, b).bpopular


@pytest.mark.parametrize("n", CONTEXTS)
def test_script_is_difflibs_grouped_opcodes(n):
    bad = [name for name, a, b in CASES if diff.diff_script(a, b, n) != _grouped(a, b, n)]
    assert not bad, bad[:5]


def test_two_changes_merge_at_2n_and_split_at_2n_plus_1():
    for n in CONTEXTS:
        for gap, groups in ((2 * n, 1), (2 * n + 1, 2)):
            (_, a, b), = [c for c in CASES if c[0] == f"two changes {gap} apart (n={n})"]
            assert len(diff.diff_script(a, b, n)) == groups == len(_grouped(a, b, n))


def test_script_capacity_one_short_reports_the_need():
    _, a, b = [c for c in CASES if c[0] == "every third line is }"][0]
    ops = diff.diff_ops(a, b, 3)
    assert len(ops) > 3
    aa, bb = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    p32 = ctypes.POINTER(ctypes.c_uint32)
    buf = (_lib.cdc_diff_op * len(ops))()
    need = ctypes.c_uint64(0)
    rc = _lib.lib().cdc_diff_script(aa.ctypes.data_as(p32), aa.size, bb.ctypes.data_as(p32), bb.size, 3, buf, len(ops) - 1,
                                    ctypes.byref(need))
    assert rc == _lib.CDC_E_NOSPACE and need.value == len(ops)
    assert buf[0].i2 == 0 and buf[0].j2 == 0  # nothing written


@pytest.mark.parametrize("n", CONTEXTS)
def test_emit_plan_text_is_difflibs_unified_diff(n):
    """The records executed in Python, over the ids as lines of text (every
    text gets the Go split's phantom last line)."""
    bad = []
    for name, a, b in CASES:
        ta, tb = diff_ref.ids_to_text(a), diff_ref.ids_to_text(b)
        got, recs, _ = diff_ref.plan_text(ta, tb, n, b"old/name", b"new name")
        if got != diff_ref.expected_diff(ta, tb, b"old/name", b"new name", n):
            bad.append(name)
        ends = recs["dst_off"].astype(np.int64) + recs["len"] + ((recs["flags"] & 0x100) != 0) + ((recs["flags"] & 0x400) != 0)
        assert (recs["dst_off"][1:] == ends[:-1]).all(), name  # back to back
    assert not bad, bad[:5]


TEXTS = [(b"", b""), (b"", b"a"), (b"a", b""), (b"a", b"a\n"), (b"a\n", b"a"), (b"a\nb\n", b"a\r\nb\r\n"),
         (b"\n\n\n", b"\n\n"), (b"x\xff\x00y\nsame\n", b"x\xff\x01y\nsame\n"), (b"\xff" * 5000, b"\xff" * 4999 + b"\n"),
         (b"".join(b"l%d\n" % i for i in range(300)), b"".join(b"l%d\n" % (i if i != 150 else 9999) for i in range(300)))]


@pytest.mark.parametrize("n", CONTEXTS)
def test_emit_plan_over_byte_texts(n):
    """The split rule's consequences: the empty text is one empty line, a
    trailing newline is a line of its own, CR, NUL and 0xff are ordinary."""
    assert diff_ref.split_lines(b"") == [b"\n"] and diff_ref.split_lines(b"a\n") == [b"a\n", b"\n"]
    assert diff_ref.split_lines(b"a") == [b"a\n"]
    for a, b in TEXTS:
        assert diff_ref.plan_text(a, b, n)[0] == diff_ref.expected_diff(a, b, n=n), (a[:20], b[:20])
    assert diff_ref.plan_text(b"", b"", n)[0] == b"" and diff_ref.expected_diff(b"a", b"a\n", n=3).startswith(b"--- a\n+++ b\n@@ ")


def test_emit_plan_bases_and_capacity():
    a, b = TEXTS[-1]
    la, lb = diff_ref.split_lines(a), diff_ref.split_lines(b)
    ids = diff_ref.first_ids(la + lb)
    ops = diff.diff_ops(ids[:len(la)], ids[len(la):], 3)
    ra = np.zeros(len(la), dtype=diff.LINE_DTYPE)
    rb = np.zeros(len(lb), dtype=diff.LINE_DTYPE)
    for r, recs in ((ra, diff_ref.line_records(a)), (rb, diff_ref.line_records(b, len(a)))):
        for k, (off, ln) in enumerate(recs):
            r[k]["off"], r[k]["len"] = off, ln
    r0, lit0, size0 = diff.diff_emit_plan(ops, ra, rb, "a", "b")
    r1, lit1, size1 = diff.diff_emit_plan(ops, ra, rb, "a", "b", dst_base=1000, lit_base=77)
    assert lit0 == lit1 and size0 == size1 and (r1["dst_off"] == r0["dst_off"] + 1000).all()
    is_lit = (r0["flags"] & 0x200) != 0
    assert (r1["src_off"][is_lit] == r0["src_off"][is_lit] + 77).all() and (r1["src_off"][~is_lit] == r0["src_off"][~is_lit]).all()
    P = ctypes.POINTER
    args = [ctypes.cast(ops.ctypes.data, P(_lib.cdc_diff_op)), ops.size, ctypes.cast(ra.ctypes.data, P(_lib.cdc_line_rec)), ra.size,
            ctypes.cast(rb.ctypes.data, P(_lib.cdc_line_rec)), rb.size, b"a", b"b", 0, 0]
    nr, nl, no = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    recs = (_lib.cdc_emit_rec * len(r0))()
    lit = ctypes.create_string_buffer(len(lit0))
    tail = [ctypes.byref(nr), ctypes.byref(nl), ctypes.byref(no)]
    L = _lib.lib()
    assert L.cdc_diff_emit_plan(*args, recs, len(r0) - 1, lit, len(lit0), *tail) == _lib.CDC_E_NOSPACE
    assert (nr.value, nl.value, no.value) == (len(r0), len(lit0), size0)
    assert L.cdc_diff_emit_plan(*args, recs, len(r0), lit, len(lit0) - 1, *tail) == _lib.CDC_E_NOSPACE
    assert L.cdc_diff_emit_plan(*args, recs, len(r0), lit, len(lit0), *tail) == _lib.CDC_OK and lit.raw == lit0
    # an opcode outside the lines is refused
    bad = ops.copy()
    bad[0]["i2"] = len(la) + 1
    args[0] = ctypes.cast(bad.ctypes.data, P(_lib.cdc_diff_op))
    assert L.cdc_diff_emit_plan(*args, recs, len(r0), lit, len(lit0), *tail) == _lib.CDC_E_INVALID


def test_host_entry_points_reject_bad_arguments():
    L = _lib.lib()
    ids = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    need = ctypes.c_uint64()
    assert L.cdc_diff_script(None, 4, ids, 4, 3, None, 0, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_script(ids, 4, None, 4, 3, None, 0, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_script(ids, 4, ids, 4, -1, None, 0, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_script(ids, 4, ids, 4, 3, None, 5, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_script(ids, 2 ** 32, ids, 4, 3, None, 0, ctypes.byref(need)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_script(None, 0, None, 0, 3, None, 0, ctypes.byref(need)) == _lib.CDC_OK and need.value == 0
    assert L.cdc_diff_script(ids, 4, ids, 4, 3, None, 0, None) == _lib.CDC_OK  # equal: no opcode


def _u64(*v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def test_device_calls_reject_bad_arguments_before_the_device():
    L = _lib.lib()
    data, recs, dst = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)  # never dereferenced
    counts, total = _u64(0, 0), ctypes.c_uint64()
    good = dict(device=0, d_data=data, len=4096, text_off=_u64(0, 100), text_len=_u64(100, 3996), n=2, d_recs=recs, cap=10,
                counts=counts, total=ctypes.byref(total), stream=None)

    def table(**kw):
        a = dict(good, **kw)
        return L.cdc_line_table_device(*[a[k] for k in good])

    for name, bad in [("device", -1), ("device", 64), ("text_off", None), ("text_len", None), ("d_data", None), ("d_recs", None),
                      ("d_recs", ctypes.c_void_p((2 << 20) + 8)), ("text_len", _u64(100, 3997)), ("text_off", _u64(0, 4097)),
                      ("text_len", _u64(100, 2 ** 64 - 50))]:
        assert table(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert table(len=2 ** 33, text_len=_u64(100, 2 ** 32)) == _lib.CDC_E_INVALID  # a text of 4 GiB
    assert table(len=2 ** 33, text_off=_u64(0, 0), text_len=_u64(2 ** 31, 2 ** 31)) == _lib.CDC_E_INVALID  # too many lines possible
    assert table(n=0) in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)

    lines = np.zeros(3, dtype=diff.LINE_DTYPE)
    lines["off"], lines["len"] = [0, 10, 20], [5, 5, 5]
    ids = (ctypes.c_uint32 * 3)()
    rounds = ctypes.c_uint32()
    gid = dict(device=0, d_data=data, len=4096, recs=ctypes.c_void_p(lines.ctypes.data), nlines=3, group=_u64(0, 2, 3), ngroups=2,
               hash_bits=0, ids=ids, rounds=ctypes.byref(rounds), stream=None)

    def line_ids(**kw):
        a = dict(gid, **kw)
        return L.cdc_line_ids_device(*[a[k] for k in gid])

    for name, bad in [("device", 64), ("d_data", None), ("recs", None), ("group", None), ("ids", None), ("hash_bits", -1),
                      ("hash_bits", 129), ("group", _u64(0, 2, 2)), ("group", _u64(1, 2, 3)), ("group", _u64(0, 3, 2, 3)),
                      ("len", 24)]:
        assert line_ids(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert line_ids(nlines=0, group=_u64(0, 0, 0)) in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)

    er = np.zeros(3, dtype=diff.EMIT_DTYPE)
    er["src_off"], er["dst_off"], er["len"], er["flags"] = [0, 5, 50], [0, 12, 20], [10, 3, 7], [0x52B, 0x200, 0x400]
    ge = dict(device=0, d_plain=data, plain_cap=4096, d_lit=recs, lit_cap=8, recs=ctypes.cast(er.ctypes.data, ctypes.POINTER(_lib.cdc_emit_rec)),
              n=3, d_dst=dst, dst_cap=28, stream=None)

    def emit(**kw):
        a = dict(ge, **kw)
        return L.cdc_diff_emit_device(*[a[k] for k in ge])

    def with_rec(i, field, value):
        e = er.copy()
        e[i][field] = value
        emit.keep = e
        return emit(recs=ctypes.cast(e.ctypes.data, ctypes.POINTER(_lib.cdc_emit_rec)))

    for name, bad in [("device", -1), ("recs", None), ("d_plain", None), ("d_lit", None), ("d_dst", None), ("dst_cap", 27),
                      ("lit_cap", 7), ("plain_cap", 56), ("d_dst", ctypes.c_void_p((1 << 20) + 4000))]:
        assert emit(**{name: bad}) == _lib.CDC_E_INVALID, name
    assert with_rec(1, "dst_off", 11) == _lib.CDC_E_INVALID     # overlaps the record before (12 bytes: prefix, 10, newline)
    assert with_rec(2, "dst_off", 14) == _lib.CDC_E_INVALID     # overlaps the literal
    assert with_rec(0, "flags", 0x800) == _lib.CDC_E_INVALID    # an unknown flag
    assert with_rec(2, "src_off", 4090) == _lib.CDC_E_INVALID   # source past the plaintext
    assert with_rec(1, "src_off", 2 ** 64 - 1) == _lib.CDC_E_INVALID
    assert emit(n=0) in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
    if not _has_gpu():
        assert table() == _lib.CDC_E_NOT_INIT and line_ids() == _lib.CDC_E_NOT_INIT and emit() == _lib.CDC_E_NOT_INIT
    assert L.cdc_debug_set_line_threshold(0) == _lib.CDC_OK


def test_diff_context_argument_checks_and_defaults_without_a_device():
    L = _lib.lib()
    o = _lib.cdc_diff_opts()
    o.context = 5
    L.cdc_diff_default_opts(ctypes.byref(o))
    assert o.struct_size == ctypes.sizeof(_lib.cdc_diff_opts)
    assert (o.compress, o.key, o.context, o.threads, o.batch_bytes, o.max_lines, o.hash_bits) == (0, None, 0, 0, 0, 0, 0)
    L.cdc_diff_default_opts(None)
    h = ctypes.c_void_p()
    assert L.cdc_diff_new(0, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_new(0, ctypes.byref(o), None) == _lib.CDC_E_INVALID
    assert L.cdc_diff_new(-1, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_diff_new(64, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID
    for field, bad in [("struct_size", 0), ("struct_size", o.struct_size + 8), ("threads", -1), ("threads", 257), ("context", -1),
                       ("batch_bytes", (1 << 30) + 1), ("max_lines", (1 << 31) + 1), ("hash_bits", -1), ("hash_bits", 129),
                       ("compress", 7)]:
        keep = getattr(o, field)
        setattr(o, field, bad)
        assert L.cdc_diff_new(0, ctypes.byref(o), ctypes.byref(h)) == _lib.CDC_E_INVALID, field
        assert not h.value
        setattr(o, field, keep)
    st = L.cdc_diff_new(0, ctypes.byref(o), ctypes.byref(h))
    if _has_gpu():  # an earlier test of the run may have initialised the library
        assert st in (_lib.CDC_E_NOT_INIT, _lib.CDC_OK)
        L.cdc_diff_free(h)
    else:
        assert st == _lib.CDC_E_NOT_INIT and not h.value
    p = (_lib.cdc_diff_pair * 1)()
    cb = _lib.DIFF_PAIR_FN(lambda ctx, r: None)
    assert L.cdc_diff_files(None, p, 1, cb, None, None) == _lib.CDC_E_INVALID
    assert L.cdc_diff_add_packfile(None, b"x", 1) == _lib.CDC_E_INVALID
    assert L.cdc_diff_add_packfile_path(None, b"/nonexistent") == _lib.CDC_E_INVALID
    L.cdc_diff_free(None)
    # the stats struct ends as the header's does
    assert ctypes.sizeof(_lib.cdc_diff_stats) == 8 + 16 * 8 + 11 * 8 and ctypes.sizeof(_lib.cdc_line_rec) == 32
    assert ctypes.sizeof(_lib.cdc_emit_rec) == 24 and ctypes.sizeof(_lib.cdc_diff_op) == 24


def test_python_layer_checks_its_arguments():
    with pytest.raises(ValueError):
        diff.DiffSession(key=b"short")
    with pytest.raises(ValueError):
        diff.DiffSession(compression="ZSTD")
    with pytest.raises(ValueError):
        diff.DiffSession(context=0)
    with pytest.raises(ValueError):
        diff.DiffSession(hash_bits=129)
    with pytest.raises(ValueError):
        diff.diff_files([], [], key=bytes(31))
    with pytest.raises(ValueError):
        diff.diff_script([1], [2], context=-1)
    assert snapshot.DiffSession is diff.DiffSession and snapshot.diff_files is diff.diff_files
    assert diff.diff_script([1, 2, 3], [1, 5, 3], 1) == [[("equal", 0, 1, 0, 1), ("replace", 1, 2, 1, 2), ("equal", 2, 3, 2, 3)]]


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


def test_diff_kernels_use_no_private_memory():
    """The table, compare and emit kernels keep everything in registers: no
    private-segment bytes, no spilled registers, and room for eight waves per
    SIMD (they are latency-bound on short lines)."""
    out = _resources()
    for name in ("k_line_count", "k_tile_scan", "k_text_lines", "k_line_mark", "k_line_hash", "k_line_hash_long", "k_line_verify",
                 "k_line_verify_long", "k_diff_emit"):
        ks = [v for k, v in out.items() if re.search(r"\d" + name + r"E", k)]
        assert len(ks) == 1, (name, sorted(out))
        k = ks[0]
        assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["Occupancy [waves/SIMD]"]) == 8, (name, k)
    emit = [v for k, v in out.items() if "k_diff_emit" in k][0]
    assert int(emit["LDS Size [bytes/block]"]) <= 2048


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dplan") / "diff_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "diff_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_matcher_emit_planner_and_ids_under_sanitizers(plan_check_exe):
    """The stand-alone program over the same shapes of cases: every script a
    valid one, every plan executed in exactly sized heap buffers and equal to
    an independent rendering, exact ids from hashes cut to a few bits; no
    sanitizer report."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) cases, (\d+) ops, (\d+) records, (\d+) rounds, ok", r.stdout)
    assert m and int(m.group(1)) >= 225 and int(m.group(2)) > 10000 and int(m.group(3)) > 20000 and int(m.group(4)) > 300, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
