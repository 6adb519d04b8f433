"""inflate_ref, the Python restatement of the gzip / DEFLATE walker, against
zlib: equal on everything zlib writes, never more lenient on mutations, and
every hand-made fixture holds the structure it is named for."""
import zlib

import numpy as np
import pytest

import inflate_ref as ir


def test_equals_zlib_on_what_zlib_writes():
    for name, (stream, content) in ir.zlib_streams().items():
        assert zlib.decompress(stream, 31) == content, name
        assert ir.gunzip(stream) == content, name


def test_zlib_streams_hold_every_block_type():
    zs = ir.zlib_streams()

    def types(name):
        s = zs[name][0]
        return [b["btype"] for b in ir.inflate(s, ir.member_header(s))[2]]

    assert set(types("mix-fixed")) == {1}
    t = types("random-70000")
    assert set(t) == {0} and len(t) >= 2     # a stored block holds 65,535 bytes at the most
    assert 2 in types("text-level6") and 2 in types("mix-huffman")
    assert types("mix-sync-flush").count(0) >= 3       # the empty stored block of every sync flush
    assert len(types("mix-full-flush")) >= 5
    assert set(types("mix-level0")) == {0}


def test_never_accepts_a_mutation_that_zlib_rejects():
    rng = np.random.default_rng(5)
    zs = ir.zlib_streams()
    bodies = [zs[k][0][10:-8] for k in ("small-mix-level6", "small-mix-fixed", "text-300", "text-200", "small-mix-level0", "zeros-300")]
    bodies += [s[ir.member_header(s):-8] for s, _ in ir.handmade().values() if len(s) < 2000]
    accepted = rejected = 0
    for i in range(3000):
        b = bytearray(bodies[i % len(bodies)])
        at = int(rng.integers(0, min(len(b), 80))) if i % 2 else int(rng.integers(0, len(b)))
        b[at] ^= 1 << int(rng.integers(0, 8))
        b = bytes(b)
        try:
            out, end, _ = ir.inflate(b)
        except ir.Corrupt:
            rejected += 1
            continue
        accepted += 1
        d = zlib.decompressobj(-15)
        ref = d.decompress(b[:end])
        assert d.eof and not d.unused_data, i
        assert ref == out, i
    assert accepted > 300 and rejected > 300, (accepted, rejected)


def _walk(name):
    s, content = ir.handmade()[name]
    out, end, walk = ir.inflate(s, ir.member_header(s))
    assert out == content and end == len(s) - 8, name
    return content, walk


def test_handmade_fixtures_decode_with_zlib_too():
    for name, (s, content) in ir.handmade().items():
        assert ir.gunzip(s) == content, name
        assert zlib.decompress(s, 31) == content, name


def test_all_lengths_and_distance_codes():
    _, walk = _walk("all-lengths-all-distances")
    assert [b["btype"] for b in walk] == [0, 1]
    m = walk[1]["matches"]
    assert {x[1] for x in m} == set(range(3, 259))
    assert {ir.dist_sym(x[2])[0] for x in m} == set(range(30))
    assert {x[2] for x in m} >= {ir.DIST_BASE[d] + (1 << ir.DIST_EXTRA[d]) - 1 for d in range(30)}
    assert any(ir.dist_sym(x[2])[2] not in (0, (1 << ir.DIST_EXTRA[ir.dist_sym(x[2])[0]]) - 1) for x in m)


def test_long_overlapping_and_far_matches():
    _, walk = _walk("258-at-distance-1-from-byte-1")
    assert walk[0]["matches"] == [(1, 258, 1)]
    _, walk = _walk("distance-32768")
    assert (32768, 10, 32768) in walk[1]["matches"] and max(x[2] for x in walk[1]["matches"]) == 32768
    content, walk = _walk("fixed-match-into-stored")
    assert [b["btype"] for b in walk] == [0, 1]
    pos, ln, d = walk[1]["matches"][0]
    assert pos - d < walk[1]["first"], "the match starts in the stored block"
    content, walk = _walk("three-blocks-beyond-32k")
    assert [b["btype"] for b in walk] == [0, 1, 2] and len(content) > 32768
    assert walk[2]["first"] > 32768 and walk[2]["matches"][0][2] == 32768


def test_code_shapes():
    _, walk = _walk("15-bit-code")
    assert walk[0]["maxbits"] == 15 and max(walk[0]["litlens"]) == 15
    _, walk = _walk("repeat-codes-across-the-boundary")
    cl, nlit = walk[0]["cl"], walk[0]["nlit"]
    assert {s for s, _, _ in cl} >= {16, 17, 18}
    assert any(s == 18 and at < nlit < at + rep for s, rep, at in cl), "a run over the HLIT / HDIST boundary"
    _, walk = _walk("single-distance-code")
    assert walk[0]["distlens"] == [1] and walk[0]["matches"]
    _, walk = _walk("literal-only-hdist-1-length-0")
    assert walk[0]["distlens"] == [0] and not walk[0]["matches"] and walk[0]["btype"] == 2
    _, walk = _walk("empty-stored-blocks")
    assert [b["stored"] for b in walk] == [0, None, 0]


def test_member_fields():
    hm = ir.handmade()
    flags = {n: hm["member-" + n][0][3] for n in ("fextra", "fextra-empty", "fname", "fcomment", "fhcrc", "ftext",
                                                   "all-fields")}
    assert flags == {"fextra": 4, "fextra-empty": 4, "fname": 8, "fcomment": 16, "fhcrc": 2, "ftext": 1,
                     "all-fields": 31}
    assert ir.member_header(hm["member-ftext"][0]) == 10
    assert ir.member_header(hm["member-fextra"][0]) == 10 + 2 + 8
    assert ir.member_header(hm["member-all-fields"][0]) == 10 + 2 + 5 + 2 + 1 + 2


@pytest.mark.parametrize("name", sorted(ir.corruptions()))
def test_named_corruption(name):
    stream, status = ir.corruptions()[name]
    assert ir.status_of(stream) == (status, None)
    if name == "isize-1GiB-in-30-bytes":
        assert ir.claim(stream) == (ir.CORRUPT, 0), "refused while sizing"
    if status == ir.CORRUPT and name not in ("trailing-byte", "isize-minus-1"):
        # zlib's gzip reader refuses it as well (it tolerates bytes after the
        # trailer, and stops at its own count of the output)
        with pytest.raises(zlib.error):
            d = zlib.decompressobj(31)
            d.decompress(stream)
            if not d.eof:
                raise zlib.error("incomplete")


def test_the_faults_are_the_named_ones():
    """Each DEFLATE-level corruption fails for its own reason, not an earlier one."""
    want = {"btype-3": "BTYPE 3", "len-nlen": "LEN / NLEN", "distance-before-start": "before the first byte",
            "over-subscribed": "code set", "incomplete-literal-length-set": "code set",
            "code-16-first": "nothing before it", "run-past-hlit-hdist": "a run past", "symbol-286": "286",
            "distance-code-30": "30 or 31", "no-end-of-block-code": "no end-of-block"}
    for name, msg in want.items():
        s = ir.corruptions()[name][0]
        with pytest.raises(ir.Corrupt, match=msg):
            ir.inflate(s, ir.member_header(s), ir.claim(s)[1])
    over = ir.corruptions()["over-subscribed"][0]
    assert ir.kraft([1, 1, 1]) > 1 << 15 and ir.kraft([2, 2]) < 1 << 15 and over


def test_mutations_split_both_ways():
    st = [r[0] for r in ir.mutation_refs()]
    assert len(st) == 512 and st.count(0) > 50 and st.count(ir.CORRUPT) > 50, (st.count(0), st.count(ir.CORRUPT))
