"""The line table and the exact line ids on the device (cdc_line_table_device,
cdc_line_ids_device) against a Python split: line counts, (off, len) records,
equal hashes for equal lines, and ids with all 128 hash bits and with 4 (nearly
every line collides), at the smallest shapes where the kernels can go wrong.
The tile is 16 KiB, a wave step 1 KiB (64 lanes of 16 bytes), the long-line
threshold 4096 bytes, a hash block 256 bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import diff_ref  # noqa: E402
from plakar_amd import _lib, diff  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 16384
THRESHOLD = 4096
LANE, WAVE = 1, 0xFFFFFFFF  # thresholds that put every line on the wave path / the lane path


def _dev(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _run(buf, texts, groups=None, thresholds=(0,), bits=(0, 4)):
    """The table and ids of `texts` in `buf`, checked; returns the records."""
    buf = bytes(buf)
    t = _dev(buf)
    want, want_counts = [], []
    for off, ln in texts:
        recs = diff_ref.line_records(buf[off:off + ln], off)
        want.extend(recs)
        want_counts.append(len(recs))
    lines = [buf[o:o + n] for o, n in want]
    groups = [0, len(want)] if groups is None else groups
    want_ids = []
    for g0, g1 in zip(groups, groups[1:]):
        want_ids.extend(diff_ref.first_ids(lines[g0:g1]))
    first = None
    try:
        for thr in thresholds:
            assert _lib.lib().cdc_debug_set_line_threshold(thr) == 0
            recs, counts = diff.line_table_device(t, texts)
            r = recs.cpu().numpy().reshape(-1).view(diff.LINE_DTYPE).reshape(-1)
            assert counts.tolist() == want_counts
            assert r.size == len(want)
            assert r["off"].tolist() == [o for o, _ in want] and r["len"].tolist() == [n for _, n in want]
            assert not r["reserved"].any()
            by_line = {}
            for ln, h in zip(lines, r["hash"].tolist()):
                assert by_line.setdefault(ln, h) == h, "equal lines with different hashes"
            if first is None:
                first = r
            else:
                assert (r["hash"] == first["hash"]).all(), "the hash depends on the path"
            for b in bits:
                ids, rounds = diff.line_ids_device(t, r, groups, hash_bits=b)
                assert ids.tolist() == want_ids, (thr, b)
                if b == 0 and len(set(map(tuple, r["hash"].tolist()))) == len(set(lines)):
                    assert rounds <= 1  # no collision: one comparison launch, or none without repeats
    finally:
        _lib.lib().cdc_debug_set_line_threshold(0)
    return first


def test_empty_and_one_byte_texts():
    _run(b"", [(0, 0)])
    _run(b"x", [(0, 1)])
    _run(b"\n", [(0, 1)])
    _run(b"ab", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)])


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1])
def test_only_newlines(k):
    r = _run(b"\n" * k, [(0, k)], thresholds=(0, LANE))
    assert r.size == k + 1 and not r["len"].any()


def test_newlines_at_tile_boundaries():
    """A newline as the last byte of a tile, as the first of the next, both,
    and lines that span two and five tiles."""
    for at in ([TILE - 1], [TILE], [TILE - 1, TILE], [2 * TILE - 1, 2 * TILE, 3 * TILE]):
        b = bytearray(b"a" * (3 * TILE + 100))
        for p in at:
            b[p] = 10
        _run(b, [(0, len(b))])
    two = b"x" * 100 + b"\n" + b"y" * (TILE + 500) + b"\n" + b"z" * 30
    five = b"q\n" + bytes(np.random.default_rng(7).integers(11, 256, 4 * TILE + 700, dtype=np.uint8)) + b"\nend"
    _run(two, [(0, len(two))])
    _run(five, [(0, len(five))], thresholds=(0, LANE))


@pytest.mark.parametrize("n", [THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, 255, 256, 257])
def test_lines_around_the_threshold_on_both_paths(n):
    """Two equal and two different lines of n bytes (the second pair differs
    in the last byte only), hashed by a lane, by a wave, and by whichever the
    default threshold picks: the same hashes, the same ids."""
    rng = np.random.default_rng(n)
    x = bytes(rng.integers(11, 256, n, dtype=np.uint8))
    y = x[:-1] + bytes([11 if x[-1] != 11 else 12])
    buf = b"\n".join([x, y, b"short", x, y, x[:n - 1]])
    r = _run(buf, [(0, len(buf))], thresholds=(0, LANE, WAVE))
    assert r["len"].tolist() == [n, n, 5, n, n, n - 1]


def test_one_four_mib_line():
    """One line of 4 MiB without a newline, twice (two texts, one pair), then
    once more with its last byte changed: a wave per line, never a lane."""
    rng = np.random.default_rng(3)
    x = rng.integers(11, 256, 4 << 20, dtype=np.uint8).tobytes()
    y = x[:-1] + b"\x0b"
    buf = x + y + x
    n = len(x)
    r = _run(buf, [(0, n), (n, n), (2 * n, n)], bits=(0,))
    assert r["len"].tolist() == [n, n, n]


def test_texts_at_every_offset_and_overlapping():
    body = b"first line\nsecond\n\nfourth \xff\x00 line\nlast without newline"
    buf = b"#" * 18 + body
    _run(buf, [(k, len(buf) - k) for k in range(18)], groups=None)
    buf = b"ab\ncd\nef\ngh"
    _run(buf, [(0, 8), (4, 7), (0, len(buf)), (3, 3)])


def test_three_hundred_texts_with_empty_ones():
    rng = np.random.default_rng(11)
    buf = bytes(rng.choice(np.frombuffer(b"ab\n\n xyz", dtype=np.uint8), 50_000))
    texts = []
    for i in range(300):
        ln = 0 if i % 7 == 0 else int(rng.integers(1, 400))
        texts.append((int(rng.integers(0, len(buf) - ln)), ln))
    counts = [buf[o:o + n].count(b"\n") + 1 for o, n in texts]
    groups = [0]
    for i in range(0, 300, 2):
        groups.append(groups[-1] + counts[i] + counts[i + 1])  # pairs of texts
    _run(buf, texts, groups=groups)


def test_line_content_edge_cases():
    """Lines equal but for the last byte, for a trailing CR, for length, and
    the bytes 0x00 and 0xff."""
    lines = [b"ab", b"ab\0", b"ab\r", b"ac", b"ab", b"", b"\0", b"\xff", b"\0\0", b"\xff\xff", b"ab\0", b"", b"a" * 300,
             b"a" * 299 + b"b", b"a" * 300]
    buf = b"\n".join(lines)
    r = _run(buf, [(0, len(buf))], thresholds=(0, LANE, WAVE))
    assert r.size == len(lines)


def _variant_positions(n, rng):
    """Every position of a line of up to 600 bytes; of a longer one the first
    600, the first and last byte of each 8-byte word next to a 256-byte block
    edge, the last byte, and 200 seeded positions."""
    if n <= 600:
        return list(range(n))
    at = set(range(600))
    for edge in range(256, n + 1, 256):
        at.update(p for p in (edge - 8, edge - 1, edge, edge + 7) if p < n)
    at.add(n - 1)
    at.update(int(p) for p in rng.integers(600, n, 200))
    return sorted(at)


def test_every_byte_and_the_length_reach_the_hash():
    """A line and its single-byte variants, at every position a word, a block
    or a wave step can drop, and lines of 1-17 zero bytes (equal but for their
    length): all hashes differ, on both paths, so a hash that left a position
    out would show here and not only as slow diffs.  With 4 hash bits the byte
    comparison meets a difference at each of those positions."""
    rng = np.random.default_rng(41)
    lengths = list(range(1, 25)) + [255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 16383, 16384, 16385]
    lines = []
    for n in lengths:
        x = rng.integers(11, 256, n, dtype=np.uint8)  # neither a newline nor a zero
        lines.append(x.tobytes())
        for p in _variant_positions(n, rng):
            y = x.copy()
            y[p] = x[p] + 1 if x[p] < 255 else 11
            lines.append(y.tobytes())
    lines += [b"\0" * k for k in range(1, 18)]
    assert len(set(lines)) == len(lines) > 5000
    buf = b"\n".join(lines)
    r = _run(buf, [(0, len(buf))], thresholds=(0, LANE, WAVE))
    assert r["len"].tolist() == [len(ln) for ln in lines]
    hashes = set(map(tuple, r["hash"].tolist()))
    assert len(hashes) == len(lines), f"{len(lines) - len(hashes)} lines share a 128-bit hash with another"


def test_seventy_thousand_short_lines():
    """More tiles than one pass of the scan's workgroup takes (256), so the
    running sum is carried; lengths 0-130 from an alphabet of 3."""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 131, 70_000)
    parts = [bytes(rng.choice(np.frombuffer(b"abc", dtype=np.uint8), int(n))) for n in lens]
    buf = b"\n".join(parts)
    assert len(buf) > 257 * TILE
    _run(buf, [(0, len(buf))], bits=(0,))
    # and as 1,000 texts of 70 lines: 1,000 tiles
    texts, off = [], 0
    for i in range(0, 70_000, 70):
        n = sum(len(p) for p in parts[i:i + 70]) + 69
        texts.append((off, n))
        off += n + 1
    _run(buf, texts, bits=(0,))


def test_capacity_one_short_reports_the_need():
    buf = b"a\nb\nc\n" * 100
    t = _dev(buf)
    with pytest.raises(_lib.CdcError) as e:
        diff.line_table_device(t, [(0, len(buf)), (0, 10)], capacity=306)
    assert e.value.status == _lib.CDC_E_NOSPACE and e.value.needed == 301 + 6
    recs, counts = diff.line_table_device(t, [(0, len(buf)), (0, 10)], capacity=307)
    assert recs.shape[0] == 307 and counts.tolist() == [301, 6]
    with pytest.raises(_lib.CdcError) as e:
        diff.line_table_device(t, [(len(buf) - 3, 4)])
    assert e.value.status == _lib.CDC_E_INVALID
    recs, counts = diff.line_table_device(t, [])
    assert recs.shape[0] == 0 and counts.size == 0
