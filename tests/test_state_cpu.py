"""The state's checks that need no GPU: the layout code (plakar_amd/csrc/
state_plan.h) against a brute-force restatement under the sanitizers
(tests/c/state_plan_check.cpp), the reference of tests/state_ref.py against
itself and against cdc_state_serialize, the ctypes table and the struct
layout, the argument checks the entry points make before they touch a device,
and the compiler's resource report of the new kernels."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import state_ref as sref
from plakar_amd import _lib, build, repository, state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cdc_state_new", "cdc_state_free", "cdc_state_merge", "cdc_state_lookup", "cdc_state_lookup_device",
               "cdc_state_rows", "cdc_state_extends", "cdc_state_info", "cdc_state_serialize",
               "cdc_debug_set_state_blocks"]
KERNELS = ["k_state_plan", "k_state_index", "k_state_resolve", "k_state_insert", "k_state_count", "k_state_lookup",
           "k_state_rows"]


def csum(*parts):
    import hashlib
    return hashlib.sha256(repr(parts).encode()).digest()


def random_rows(rng, n, packs=3, tag=0):
    """n rows over every type, with some (type, blob) keys repeated at another location."""
    rows = []
    for i in range(n):
        typ = rng.randrange(9)
        blob = csum("blob", tag, rng.randrange(max(1, (3 * n) // 4)))
        rows.append((typ, blob, csum("pack", tag, rng.randrange(packs)), rng.randrange(1 << 32), rng.randrange(1 << 32)))
    return rows


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("splan") / "state_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "state_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_planner_under_sanitizers(plan_check_exe):
    """Every truncation of a 717-byte state with two records per section, each
    of the 12 counts at 2^61, 2^64 - 1 and around what fits, 10,000 random
    mutations, the writer's output read back: the planner agrees with the
    brute-force restatement and reads nothing it was not given."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) accepted, (\d+) rejected, (\d+) truncations, (\d+) counts, writer ok", r.stdout)
    assert m, r.stdout
    accepted, rejected, truncations, counts = (int(g) for g in m.groups())
    assert truncations == 718 and counts == 48
    # 718 truncations, 3 around the end, 48 counts, 10,000 mutations, 2 of the writer
    assert accepted + rejected == 718 + 3 + 48 + 10000 + 2, r.stdout
    # the whole state, its padded copy, the 109 zero bytes, the writer's two, and the mutations that stay well formed
    assert accepted > 1000 and rejected >= 717 + 1 + 36 + 1000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_reference_writer_and_reader_agree(order):
    rng = random.Random(5)
    st = sref.from_rows(random_rows(rng, 200), timestamp=-7, extends=[csum("e", 1), csum("e", 2)], aggregate=True)
    st.delete_snapshot(csum("gone"), 99)
    data = st.serialize(order, seed=3)
    assert len(data) == st.size() == 109 + 32 * 2 + 16 * 1 + 40 * len(st.id_to_checksum) + \
        24 * sum(len(m) for m in st.maps.values())
    back = sref.deserialize(data + b"trailing bytes are ignored")
    assert back.maps == st.maps and back.id_to_checksum == st.id_to_checksum and back.deleted == st.deleted
    assert (back.version, back.timestamp, back.aggregate, back.extends) == (100, -7, True, st.extends)
    for cut in (0, 12, 108, len(data) - 1):
        with pytest.raises(ValueError):
            sref.deserialize(data[:cut])
    assert len(sref.State().serialize()) == 109
    # first given wins, and the types do not share keys
    a = sref.from_rows([(1, csum("k"), csum("p1"), 1, 2), (2, csum("k"), csum("p1"), 3, 4)])
    b = sref.from_rows([(1, csum("k"), csum("p2"), 5, 6)])
    agg = sref.aggregate_of([(csum("a"), a), (csum("b"), b)])
    assert agg.get_subpart_for_blob(1, csum("k")) == (csum("p1"), 1, 2, True)
    assert agg.get_subpart_for_blob(2, csum("k")) == (csum("p1"), 3, 4, True)
    assert agg.get_subpart_for_blob(3, csum("k")) == (sref.ZERO, 0, 0, False)
    assert sref.aggregate_of([(csum("b"), b), (csum("a"), a)]).get_subpart_for_blob(1, csum("k")) == (csum("p2"), 5, 6, True)
    with pytest.raises(ValueError):
        agg.blob_exists(9, csum("k"))


def test_serialize_agrees_with_the_reference():
    """cdc_state_serialize's output deserialises, under state_ref, to the maps
    state_ref's own SetPackfileForBlob builds from the same rows: the same ids
    (packfile first, then blob), the repeated keys dropped, every section
    ascending; and the size is the formula's."""
    rng = random.Random(11)
    for n, ext in ((0, []), (1, [csum("x")]), (300, [csum("x"), csum("y"), csum("z")])):
        rows = random_rows(rng, n)
        want = sref.from_rows(rows, timestamp=1234567890123456789, extends=ext)
        data = state.serialize_rows(rows, 1234567890123456789, aggregate=False, extends=ext)
        assert len(data) == want.size()
        got = sref.deserialize(data)
        assert got.maps == want.maps and got.id_to_checksum == want.id_to_checksum and not got.deleted
        assert (got.version, got.timestamp, got.aggregate, got.extends) == (100, 1234567890123456789, False, ext)
        # ascending ids in every section: byte-equal to the reference's ascending form
        assert data == want.serialize("asc")
    assert sref.deserialize(state.serialize_rows([], 5, aggregate=True)).aggregate is True
    with pytest.raises(ValueError):
        state.serialize_rows([(9, csum("b"), csum("p"), 0, 0)], 0)
    with pytest.raises(ValueError):
        state.serialize_rows([(1, b"short", csum("p"), 0, 0)], 0)
    with pytest.raises(ValueError):
        state.serialize_rows([], 0, extends=[b"short"])


def test_lib_exports_the_new_symbols():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "plakar_cdc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
        assert re.search(r"\b%s\(" % name, header), name
    assert (_lib.STATE_PLAIN, _lib.STATE_STORED) == (0, 1)
    for name, value in (("PLAIN", 0), ("STORED", 1)):
        assert re.search(r"#define CDC_STATE_%s\s+%d\b" % (name, value), header)
    assert not [n for n in dir(_lib) if n.startswith("CDC_STATE")]
    assert "#define CDC_ABI_VERSION 1\n" in header and L.cdc_abi_version() == 1
    row = _lib.cdc_state_row
    assert ctypes.sizeof(row) == 80 == state.ROW_DTYPE.itemsize
    assert [(n, getattr(row, n).offset) for n, _ in row._fields_] == \
        [("checksum", 0), ("packfile", 32), ("offset", 64), ("length", 68), ("type", 72), ("found", 73), ("reserved", 74)]
    assert [state.ROW_DTYPE.fields[n][1] for n, _ in row._fields_] == [0, 32, 64, 68, 72, 73, 74]
    src = _lib.cdc_state_src
    assert ctypes.sizeof(src) == 56
    assert [(n, getattr(src, n).offset) for n, _ in src._fields_] == [("bytes", 0), ("len", 8), ("id", 16), ("form", 48)]
    assert [getattr(state, "TYPE_" + n) for n in ("SNAPSHOT", "CHUNK", "OBJECT", "FILE", "DIRECTORY", "CHILD", "DATA",
                                                  "SIGNATURE", "ERROR")] == list(range(9))


def test_invalid_arguments_return_before_a_device_is_touched():
    """Run without a GPU, a call that reached for a device would be CDC_E_DEVICE,
    not CDC_E_INVALID; and an aggregate nothing was merged into answers its
    listings without one."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    for device in (-1, 64):
        assert L.cdc_state_new(device, 1, None, ctypes.byref(h)) == _lib.CDC_E_INVALID
    assert L.cdc_state_new(0, 1, None, None) == _lib.CDC_E_INVALID
    assert L.cdc_state_new(0, 1, bytes(range(32)), ctypes.byref(h)) == _lib.CDC_OK and h
    try:
        buf = ctypes.create_string_buffer(b"\0" * 109, 109)
        src = (_lib.cdc_state_src * 1)()
        src[0].bytes, src[0].len, src[0].form = ctypes.cast(buf, ctypes.c_void_p), 109, _lib.STATE_PLAIN
        status = (ctypes.c_int32 * 1)(7)
        assert L.cdc_state_merge(None, src, 1, status) == _lib.CDC_E_INVALID
        assert L.cdc_state_merge(h, None, 1, status) == _lib.CDC_E_INVALID
        assert L.cdc_state_merge(h, src, 1, None) == _lib.CDC_E_INVALID
        for form in (-1, 2):
            src[0].form = form
            assert L.cdc_state_merge(h, src, 1, status) == _lib.CDC_E_INVALID
        src[0].form, src[0].bytes = _lib.STATE_STORED, None
        assert L.cdc_state_merge(h, src, 1, status) == _lib.CDC_E_INVALID  # a length without bytes
        assert status[0] == 7
        assert L.cdc_state_merge(h, None, 0, None) == _lib.CDC_OK  # nothing to do
        q = ctypes.create_string_buffer(64)
        out = (_lib.cdc_state_row * 2)()
        for fn, extra in ((L.cdc_state_lookup, ()), (L.cdc_state_lookup_device, (None,))):
            assert fn(None, 1, q, 2, out, *extra) == _lib.CDC_E_INVALID
            assert fn(h, 9, q, 2, out, *extra) == _lib.CDC_E_INVALID     # the reference panics
            assert fn(h, 255, q, 2, out, *extra) == _lib.CDC_E_INVALID
            assert fn(h, 1, None, 2, out, *extra) == _lib.CDC_E_INVALID
            assert fn(h, 1, q, 2, None, *extra) == _lib.CDC_E_INVALID
            assert fn(h, 1, None, 0, None, *extra) == _lib.CDC_OK
        need = ctypes.c_uint64(5)
        assert L.cdc_state_rows(None, 1, out, 2, ctypes.byref(need)) == _lib.CDC_E_INVALID
        assert L.cdc_state_rows(h, 9, out, 2, ctypes.byref(need)) == _lib.CDC_E_INVALID
        assert L.cdc_state_rows(h, 1, None, 2, ctypes.byref(need)) == _lib.CDC_E_INVALID
        assert need.value == 5
        # an aggregate nothing was merged into answers without a device
        assert L.cdc_state_rows(h, 1, out, 2, ctypes.byref(need)) == _lib.CDC_OK and need.value == 0
        assert L.cdc_state_extends(None, q, 2, ctypes.byref(need)) == _lib.CDC_E_INVALID
        assert L.cdc_state_extends(h, None, 2, ctypes.byref(need)) == _lib.CDC_E_INVALID
        assert L.cdc_state_extends(h, q, 2, ctypes.byref(need)) == _lib.CDC_OK and need.value == 0
        st = _lib.cdc_state_stats()
        assert L.cdc_state_info(h, None) == _lib.CDC_E_INVALID
        assert L.cdc_state_info(None, ctypes.byref(st)) == _lib.CDC_E_INVALID
        assert L.cdc_state_info(h, ctypes.byref(st)) == _lib.CDC_E_INVALID  # struct_size not set
        st.struct_size = ctypes.sizeof(st)
        assert L.cdc_state_info(h, ctypes.byref(st)) == _lib.CDC_OK
        assert (st.states, st.rejected, st.records, st.capacity, st.device_bytes) == (0, 0, 0, 1024, 0)
    finally:
        L.cdc_state_free(h)
    L.cdc_state_free(None)
    n = ctypes.c_uint64()
    rows = (_lib.cdc_state_row * 1)()
    assert L.cdc_state_serialize(None, 1, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert L.cdc_state_serialize(rows, 1, 0, 0, None, 1, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert L.cdc_state_serialize(rows, 1, 0, 0, None, 0, None, 0, None) == _lib.CDC_E_INVALID
    rows[0].type = 9
    assert L.cdc_state_serialize(rows, 1, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert L.cdc_debug_set_state_blocks(3) == _lib.CDC_OK and L.cdc_debug_set_state_blocks(0) == _lib.CDC_OK


def test_python_layer_checks_its_arguments():
    with pytest.raises(ValueError):
        state.State(key=b"short")
    with pytest.raises(ValueError):
        state.State(compression="ZSTD")
    with pytest.raises(ValueError):
        _lib.state_form_code("rows")
    with state.State(key=None, compression=None) as s:
        with pytest.raises(ValueError):
            s.merge([b"x"], ids=[b"short"])
        with pytest.raises(ValueError):
            s.merge([b"x"], form="rows")
        with pytest.raises(ValueError):
            s.blob_exists(9, [csum("a")])
        with pytest.raises(ValueError):
            s.blob_exists(1, [b"short"])
        assert s.list_blobs(state.TYPE_CHUNK) == [] and s.extends() == [] and s.list_snapshots() == []
        assert s.info()["rows"] == [0] * 9 and s.packfile_rows() == {}
    with pytest.raises(ValueError):
        s.info()  # closed
    with pytest.raises(ValueError):
        repository.Repository().BlobExists(1, [csum("a")])  # RebuildState has not run
    assert np.array_equal(state._sums(csum("a") + csum("b")), state._sums([csum("a"), csum("b")]))


def test_new_kernels_use_no_private_segment():
    path = build.resources_path()
    assert os.path.exists(path), f"{path}: the library is built by plakar_amd.build, which keeps the compiler's report"
    text = open(path).read()
    for k in KERNELS:
        m = re.search(r"Function Name: \S*%s\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)" % k, text, re.S)
        assert m, k
        assert (int(m.group(1)), int(m.group(2))) == (0, 0), (k, m.groups())
