"""cdc_grep_device on small buffers against the judge of tests/grep_ref.py:
the hit records, the lines, the matching lines, the binary flags and the total
are exactly the judge's.  T is the scan's tile."""
import ctypes
import random
import time

import numpy as np
import pytest

import grep_ref as gref
from plakar_amd import _lib, grep

# cdc_grep.hip's constants, held to the source by tests/test_grep_cpu.py
MIRRORED = {"kThreads": 256, "kTile": 16384, "kHalo": 255, "kStep": 4096, "kScanBlocksPerCU": 4, "kBlocksPerCU": 8}
T = MIRRORED["kTile"]
LANE, WAVE_STEP, STEP = 16, 64 * 16, MIRRORED["kStep"]
CUS = 256  # of an MI355X: the scan's grid is cut to CUS * kScanBlocksPerCU workgroups

gpu = pytest.mark.gpu


def _dev(buf):
    import torch
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    if a.size == 0:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.copy()).cuda()


def _want(buf, texts, patterns, ignore_case=False, limit=0):
    hits, lines, matched, binary = gref.grep_buffer(buf, texts, patterns, ignore_case, limit)
    return np.array(hits, dtype=grep.HIT_DTYPE), lines, matched, binary


def _same(got, want, what=""):
    hits, lines, matched, binary = got
    assert lines.tolist() == want[1], (what, "lines", lines.tolist()[:8], want[1][:8])
    assert matched.tolist() == want[2], (what, "matched", matched.tolist()[:8], want[2][:8])
    assert binary.tolist() == want[3], (what, "binary")
    assert len(hits) == len(want[0]), (what, "total", len(hits), len(want[0]))
    if not np.array_equal(hits, want[0]):
        bad = [i for i in range(len(hits)) if hits[i] != want[0][i]][:3]
        raise AssertionError((what, [(i, hits[i], want[0][i]) for i in bad]))


def check(buf, texts, patterns, ignore_case=False, limit=0, what=""):
    """One device call over an allocation of exactly len(buf) bytes, held to the judge; returns the hits."""
    want = _want(buf, texts, patterns, ignore_case, limit)
    got = grep.grep_device(_dev(buf), texts, patterns, ignore_case, limit)
    _same(got, want, what)
    return got[0]


def whole(buf):
    return [(0, len(buf))]


# ---- texts and lines ---------------------------------------------------------------------------------------
@gpu
def test_empty_and_tiny_texts():
    assert len(check(b"", [(0, 0)], [b"a"])) == 0
    assert len(check(b"a", whole(b"a"), [b"a"])) == 1
    assert len(check(b"a", whole(b"a"), [b"b"])) == 0
    assert len(check(b"\n", whole(b"\n"), [b"a"])) == 0
    # empty texts between others, and at both ends
    buf = b"ab\nab"
    check(buf, [(0, 0), (0, 2), (2, 0), (2, 1), (3, 2), (5, 0)], [b"ab", b"b"])


@gpu
@pytest.mark.parametrize("k", [1, 64, 65, T - 1, T, T + 1])
def test_only_newlines(k):
    buf = b"\n" * k
    hits, lines, matched, binary = grep.grep_device(_dev(buf), whole(buf), [b"a", b"\r"])
    assert len(hits) == 0 and lines.tolist() == [k] and matched.tolist() == [0] and binary.tolist() == [False]
    buf = b"\n" * k + b"a"
    hits = check(buf, whole(buf), [b"a"])
    assert hits["line"].tolist() == [k + 1] and hits["off"].tolist() == [k]


@gpu
def test_last_line_crlf_and_line_numbers_past_70000():
    check(b"one\ntwo", whole(b"one\ntwo"), [b"two", b"one"])
    check(b"one\ntwo\n", whole(b"one\ntwo\n"), [b"two", b"one"])
    hits = check(b"a\r\nb\r\n\r\n", whole(b"a\r\nb\r\n\r\n"), [b"\r", b"b\r"])
    assert hits["len"].tolist() == [2, 2, 1] and hits["col"].tolist() == [1, 0, 0]
    a = b"".join(b"%d\n" % i for i in range(300))
    b = b"".join((b"needle %d\n" % i) if i % 10007 == 0 else b"x\n" for i in range(70100))
    hits = check(a + b, [(0, len(a)), (len(a), len(b))], [b"needle", b"299"])
    assert hits["line"].tolist()[-1] == 70050 and hits["text"].tolist()[-1] == 1


# ---- pattern lengths ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [1, 2, 3, 16, 17, 255, 256])
def test_a_pattern_as_the_whole_text(m):
    pat = bytes((i * 7 + 3) % 200 + 32 for i in range(m))
    hits = check(pat, whole(pat), [pat])
    assert hits.tolist() == [(0, 1, 0, m, 0, 1, 1)]
    assert len(check(pat[:-1], whole(pat[:-1]), [pat])) == 0
    # the missing byte lies right behind the text, in the buffer and in the next text
    if m > 1:
        assert len(check(pat, [(0, m - 1), (m - 1, 1)], [pat])) == 0
        assert len(check(pat, [(0, m - 1)], [pat])) == 0


# ---- boundaries --------------------------------------------------------------------------------------------
@gpu
def test_patterns_across_every_boundary():
    """A 2-byte and a 256-byte pattern start at B - k for every k in 0..len, B
    each of a lane's 16 bytes, a wave's step, the workgroup's step, the tile and
    the halo's end; a text per placement, each pattern found exactly once."""
    short, long_ = b"qz", b"q" + b"y" * 254 + b"z"
    bounds = list(range(STEP + LANE, STEP + 2 * LANE)) + [WAVE_STEP, STEP, T, T + MIRRORED["kHalo"]]
    parts, texts, at = [], [], 0
    for B in bounds:
        for pat in (short, long_):
            for k in range(len(pat) + 1):
                body = bytearray((b"x" * 60 + b"\n") * ((B + 300) // 61 + 1))[:B + 300]
                body[B - k:B - k + len(pat)] = pat
                gap = b"\0" * (len(texts) % 5)
                parts += [gap, bytes(body)]
                texts.append((at + len(gap), len(body)))
                at += len(gap) + len(body)
    buf = b"".join(parts)
    want = _want(buf, texts, [short, long_])
    assert want[2] == [1] * len(texts) and want[0]["nocc"].tolist() == [1] * len(texts)  # the premise, by the judge
    _same(grep.grep_device(_dev(buf), texts, [short, long_]), want)


# ---- seams -------------------------------------------------------------------------------------------------
@gpu
def test_seams_between_texts_and_the_end_of_the_allocation():
    buf = b"xxab" + b"c\n"
    texts = [(0, 4), (4, 2)]
    assert len(check(buf, texts, [b"abc"])) == 0
    hits = check(buf, texts, [b"ab", b"c"])
    assert hits.tolist() == [(0, 1, 0, 4, 2, 1, 1), (1, 1, 4, 1, 0, 2, 1)]
    gap = b"xxab" + b"c--" + b"c\n"   # a gap of 3 bytes that holds the c
    texts = [(0, 4), (7, 2)]
    assert len(check(gap, texts, [b"abc"])) == 0
    hits = check(gap, texts, [b"ab", b"c"])
    assert hits.tolist() == [(0, 1, 0, 4, 2, 1, 1), (1, 1, 7, 1, 0, 2, 1)]
    # the seam at a tile's end, and the last text flush against the end of the allocation
    a = b"x" * (T - 2) + b"ab"
    buf = a + b"c" + b"y" * 300 + b"ab"
    texts = [(0, T), (T, 301), (T + 301, 2)]
    hits = check(buf, texts, [b"abc", b"ab", b"abcd"])
    assert hits["text"].tolist() == [0, 2] and hits["mask"].tolist() == [2, 2]


# ---- overlap and sets --------------------------------------------------------------------------------------
@gpu
def test_overlaps_shared_prefixes_and_32_patterns():
    assert check(b"aaaa", whole(b"aaaa"), [b"aa"]).tolist() == [(0, 1, 0, 4, 0, 1, 3)]
    assert check(b"x\nab\n", whole(b"x\nab\n"), [b"b", b"ab"]).tolist() == [(0, 2, 2, 2, 0, 3, 2)]
    text = b"abd abc\nzbc\nab\nabcabd ab\n\nxbcx"
    hits = check(text, whole(text), [b"ab", b"abc", b"abd", b"bc", b"ab"])
    assert hits["mask"].tolist() == [0b11111, 0b01000, 0b10001, 0b11111, 0b01000]
    pats = [bytes([97 + k % 26, 97 + (k * 7) % 26]) + (b"!" if k & 1 else b"") for k in range(32)]
    rng = random.Random(5)
    text = b"\n".join(b"".join(rng.choice(pats + [b" ", b"q"]) for _ in range(rng.randrange(0, 12))) for _ in range(400))
    hits = check(text, whole(text), pats)
    assert len(hits) > 100 and int(np.bitwise_or.reduce(hits["mask"])) == 0xFFFFFFFF


# ---- ignore-case -------------------------------------------------------------------------------------------
@gpu
def test_ignore_case_folds_ascii_letters_only():
    text = b"HeLLo\nhello\nHELLO\n@[\n`{\n\xc9\n\xe9\nhEllO @[ `{ \xc9\xe9\n"
    pats = [b"hEllO", b"@[", b"`{", b"\xc9", b"\xe9"]
    hits = check(text, whole(text), pats, ignore_case=True)
    assert hits["mask"].tolist() == [1, 1, 1, 2, 4, 8, 16, 31]
    hits = check(text, whole(text), pats)
    assert hits["mask"].tolist() == [2, 4, 8, 16, 31]
    for ic in (False, True):
        check(text, whole(text), [b"L", b"lo", b"E"], ignore_case=ic)


# ---- binary ------------------------------------------------------------------------------------------------
@gpu
def test_zero_bytes():
    for text in (b"\0abc\n", b"abc\n\0", b"a\0b\nab\n", b"ab\n"):
        check(text, whole(text), [b"a\0b", b"\0", b"ab"])
    buf = b"\0" + b"a" * 40 + b"\0" + b"b" * 40 + b"\0"
    got = grep.grep_device(_dev(buf), [(1, 40), (42, 40)], [b"a"])  # the zeros lie outside the texts
    assert got[3].tolist() == [False, False]
    got = grep.grep_device(_dev(buf), [(0, 41), (41, 41), (82, 1)], [b"a"])
    assert got[3].tolist() == [True, True, True]
    big = bytearray(b"z" * (3 * T))
    big[2 * T + 5] = 0  # in the third tile only
    check(bytes(big), whole(big), [b"zz\0"])


# ---- long lines --------------------------------------------------------------------------------------------
@gpu
def test_a_line_of_a_mebibyte():
    n = 1 << 20
    line = bytearray(b"." * n)
    line[0:3] = b"END"
    line[n // 2:n // 2 + 3] = b"END"
    line[n - 3:n] = b"END"
    for text in (bytes(line), b"head\n" + bytes(line) + b"\ntail END"):
        hits = check(text, whole(text), [b"END", b"D", b"E"])
        assert hits["nocc"].tolist()[0] == 9 and hits["len"].tolist()[0] == n and hits["col"].tolist()[0] == 0


@gpu
def test_the_worst_case_one_byte_value():
    text = b"a" * 65536
    hits = check(text, whole(text), [b"a" * 256])
    assert hits["nocc"].tolist() == [65281]
    hits = check(text, whole(text), [b"a" * 256] * 32)
    assert hits["nocc"].tolist() == [32 * 65281] and hits["mask"].tolist() == [0xFFFFFFFF]


# ---- compaction and limit ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 63, 64, 65, 1023, 1024, 1025])
def test_compaction_limit_and_nospace(k):
    lines = [b"hit %d" % i if i % 3 == 1 else b"no" for i in range(3 * k)]
    a = b"\n".join(lines) + b"\n"
    buf = a + b"--" + a
    texts = [(0, len(a)), (len(a) + 2, len(a))]
    src = _dev(buf)
    for limit in sorted({0, 1, max(k - 1, 1), k}):
        want = _want(buf, texts, [b"hit"], limit=limit)
        assert want[2] == [k, k] and len(want[0]) == 2 * (min(limit, k) if limit else k)
        _same(grep.grep_device(src, texts, [b"hit"], limit=limit), want, limit)
    total = 2 * k
    with pytest.raises(_lib.CdcError) as e:
        grep.grep_device(src, texts, [b"hit"], capacity=total - 1)
    assert e.value.status == _lib.CDC_E_NOSPACE and e.value.needed == total
    assert e.value.lines.tolist() == [3 * k, 3 * k] and e.value.matched.tolist() == [k, k]
    # nothing is written to d_hits then
    import torch
    hits = torch.full((total, 32), 0xA5, dtype=torch.uint8, device="cuda")
    t = np.asarray(texts, dtype=np.uint64)
    off, ln = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
    P = grep._Patterns([b"hit"])
    tot = ctypes.c_uint64()
    p64 = ctypes.POINTER(ctypes.c_uint64)
    rc = _lib.lib().cdc_grep_device(0, ctypes.c_void_p(src.data_ptr()), src.numel(), off.ctypes.data_as(p64), ln.ctypes.data_as(p64),
                                    2, P.ptrs, P.lens, 1, 0, 0, ctypes.c_void_p(hits.data_ptr()), total - 1, None, None, None,
                                    ctypes.byref(tot), None)
    assert rc == _lib.CDC_E_NOSPACE and tot.value == total and bool((hits == 0xA5).all())


# ---- seeded cases ------------------------------------------------------------------------------------------
def seeded_case(seed):
    rng = random.Random(seed)
    alphabet = b"abAB \r\xc9\xe9"
    lines = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 81))) for _ in range(rng.randrange(20, 120))]
    text = b"\n".join(lines) + (b"\n" if seed % 3 else b"")
    pats = []
    for _ in range(rng.randrange(1, 33)):
        m = rng.randrange(3, 9)
        at = rng.randrange(0, len(text) - m)
        pats.append(text[at:at + m].replace(b"\n", b"a"))
    return text, pats, bool(seed & 1)


SEEDS = [s for s in range(41) if s != 2]  # every line of seed 2 matches: the premise below does not hold for it


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded(seed):
    text, pats, ic = seeded_case(seed)
    want = _want(text, whole(text), pats, ic)
    assert 0 < want[2][0] < want[1][0], "the premise: a matching and a non-matching line, by the judge alone"
    _same(grep.grep_device(_dev(text), whole(text), pats, ic), want)


# ---- past the grid -----------------------------------------------------------------------------------------
@gpu
def test_more_tiles_than_the_scans_grid():
    """2 * cap + 70 tiles: the first, the second and a partial third trip of
    k_grep_scan's loop over tiles, a hit in every 97th tile and at every tile edge."""
    ntiles = 2 * CUS * MIRRORED["kScanBlocksPerCU"] + 70
    body = bytearray((b"." * 999 + b"\n") * (ntiles * T // 1000 + 1))[:ntiles * T - 5]
    for t in range(1, ntiles):
        body[t * T - 3:t * T + 3] = b"<edge>"
    for t in range(0, ntiles, 97):
        body[t * T + 5000:t * T + 5006] = b"planted"[:6]
    buf = bytes(body)
    hits = check(buf, whole(buf), [b"<edge>", b"plante", b"ge>."])
    assert len(hits) >= ntiles - 1 + ntiles // 97


@gpu
def test_every_pass_with_a_grid_of_two_workgroups():
    """cdc_debug_set_grep_blocks(2): the loops of the scan, the ranks, the
    per-text counts and the compaction all go round many times."""
    rng = random.Random(11)
    parts, texts, at = [], [], 0
    for i in range(700):  # more than 2 * 256 texts: k_grep_text's loop too
        n = rng.choice((0, 1, 50, 700, 3000)) if i % 50 else 2 * T + 100
        body = b"".join(rng.choice((b"ab", b"ABc", b"\n", b"xyz", b" ", b"\r\n")) for _ in range(n // 2))
        parts.append(body)
        texts.append((at, len(body)))
        at += len(body)
    buf = b"".join(parts)
    assert _lib.lib().cdc_debug_set_grep_blocks(2) == _lib.CDC_OK
    try:
        for ic, limit in ((False, 0), (True, 3)):
            hits = check(buf, texts, [b"abc", b"zab", b"\r"], ic, limit)
            assert len(hits) > 1000
    finally:
        _lib.lib().cdc_debug_set_grep_blocks(0)


# ---- offsets -----------------------------------------------------------------------------------------------
@gpu
def test_texts_past_2_31_and_2_32():
    """The hits' offsets are 64-bit exact, and the call lasts no longer than over
    a small buffer: the work follows the texts, not the buffer."""
    import torch
    text = (b"far away: needle one\n" + b"x" * 100 + b"\nneedle two and NEEDLE three\n" + b"y" * 150)[:300]
    assert len(text) == 300
    small = _dev(b"\0" * 4096 + text)
    want_small = _want(b"\0" * 4096 + text, [(4096, 300)], [b"needle", b"three"], True)
    grep.grep_device(small, [(4096, 300)], [b"needle", b"three"], True)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = grep.grep_device(small, [(4096, 300)], [b"needle", b"three"], True)
    t_small = time.perf_counter() - t0
    _same(got, want_small)
    n = (4 << 30) + (1 << 20)
    try:
        big = torch.zeros(n, dtype=torch.uint8, device="cuda")
    except (RuntimeError, MemoryError) as e:
        pytest.skip(f"no {n} bytes of device memory: {e}")
    texts = [((1 << 31) + 7, 300), ((1 << 32) + 13, 300)]
    piece = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for off, ln in texts:
        big[off:off + ln] = piece
    torch.cuda.synchronize()
    one = gref.grep_text(text, [b"needle", b"three"], True)
    want = [(i, h[1], texts[i][0] + h[2], h[3], h[4], h[5], h[6]) for i in range(2) for h in one[0]]
    grep.grep_device(big, texts, [b"needle", b"three"], True)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hits, lines, matched, binary = grep.grep_device(big, texts, [b"needle", b"three"], True)
    t_big = time.perf_counter() - t0
    assert hits.tolist() == want and hits["off"].dtype == np.uint64 and int(hits["off"][-1]) > 1 << 32
    assert lines.tolist() == [one[1]] * 2 and matched.tolist() == [len(one[0])] * 2 and binary.tolist() == [False, False]
    print(f"small {t_small * 1e3:.3f} ms, 4 GiB + 1 MiB {t_big * 1e3:.3f} ms")
    # a scan of the buffer would take 10 ms and more at 400 GB/s: the same handful of launches either way
    assert t_big < 3 * t_small + 2e-3, (t_small, t_big)
    del big


# ---- a busy non-default stream -----------------------------------------------------------------------------
@gpu
def test_on_a_busy_non_default_stream():
    """The real bytes are written behind a delay on the caller's stream, over a
    decoy of zeros: only work ordered after that stream finds the judge's hits,
    and the call returns with the stream drained."""
    import torch

    import stream_busy as sb
    text, pats, ic = seeded_case(3)
    buf = b"\xEE" * 5 + text + b"\xEE" * 3 + text[:1000]
    texts = [(5, len(text)), (5 + len(text) + 3, 1000)]
    want = _want(buf, texts, pats, ic)
    staged = _dev(buf)
    inp = torch.zeros_like(staged)
    cap = len(want[0])
    hits = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
    t = np.asarray(texts, dtype=np.uint64)
    off, ln = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
    P = grep._Patterns(pats)
    p64 = ctypes.POINTER(ctypes.c_uint64)

    def call(s):
        lines, matched = np.full(2, 99, dtype=np.uint64), np.full(2, 99, dtype=np.uint64)
        binary = np.full(2, 9, dtype=np.uint8)
        tot = ctypes.c_uint64(99)
        rc = _lib.lib().cdc_grep_device(0, ctypes.c_void_p(inp.data_ptr()), inp.numel(), off.ctypes.data_as(p64),
                                        ln.ctypes.data_as(p64), 2, P.ptrs, P.lens, P.n, 1 if ic else 0, 0,
                                        ctypes.c_void_p(hits.data_ptr()), cap, lines.ctypes.data_as(p64),
                                        matched.ctypes.data_as(p64), binary.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                        ctypes.byref(tot), ctypes.c_void_p(s.cuda_stream))
        return rc, lines, matched, binary, int(tot.value)

    s = torch.cuda.Stream()
    try:
        grep.grep_device(staged, texts, pats, ic, stream=s)  # warm: the caches grow now
        inp.copy_(staged)
        torch.cuda.synchronize()
        assert call(s)[0] == 0
        hits.zero_()
        inp.zero_()
        torch.cuda.synchronize()
        (rc, lines, matched, binary, tot), gate = sb.run_busy(call, s, [staged], [inp])
        drained = not gate.pending()
        assert rc == 0 and tot == cap and drained, (rc, tot, drained, sb.calibration())
        torch.cuda.synchronize()
        got = hits.cpu().numpy().reshape(-1).view(grep.HIT_DTYPE)
        _same((got, lines, matched, binary.astype(bool)), want)
    finally:
        torch.cuda.synchronize()
