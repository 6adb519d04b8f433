"""The streamed gzip member (cdc_gzip_stream_piece, plakar_amd.archive.GzipStream)
on the device against zlib and inflate_ref: the pieces of one writer
concatenate into one member whatever their lengths and contents, every piece
ends on a byte boundary at each of the eight bits a block can end on, where
the input is cut does not change what inflates, Encode's members are what they
were, and a short out_cap writes nothing."""
import functools
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import inflate_ref as ir  # noqa: E402
from plakar_amd import _lib, archive, encode  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
JOINER_TAIL = b"\x00\x00\xff\xff"
FINAL = b"\x01\x00\x00\xff\xff"
SPAN = 32768
SENTINEL = 0x5A
SLACK = 4096
BIG = (2 << 20) + SPAN + 1          # more than 64 spans in one piece
LENS = [1, SPAN - 1, SPAN, 0, SPAN + 1, BIG, 0]   # 0 in the middle and as the last
KINDS = ["text", "zeros", "random", "mixed"]


@functools.lru_cache(None)
def _content(kind, n=sum(LENS)):
    if kind == "text":
        return ir.text(n, 11)
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return ir.rnd(n, 12)
    parts, i = [], 0                  # mixed: text, random and zeros in turn, odd lengths
    while sum(map(len, parts)) < n:
        k = 20011 + 7919 * (i % 5)
        parts.append(ir.text(k, 30 + i) if i % 3 == 0 else ir.rnd(k, 30 + i) if i % 3 == 1 else bytes(k))
        i += 1
    return b"".join(parts)[:n]


def _cut(data, lens):
    assert sum(lens) == len(data)
    out, p = [], 0
    for n in lens:
        out.append(data[p:p + n])
        p += n
    return out


def _write(pieces, gs=None):
    """The pieces through one writer (the last one closes it), each into the
    middle of a sentinel-filled buffer of exactly its bound: the outputs."""
    own = gs is None
    gs = gs or archive.GzipStream()
    outs = []
    try:
        for i, p in enumerate(pieces):
            cap = archive.gzip_stream_bound(len(p))
            src = torch.from_numpy(np.frombuffer(b"\xEE" + p + b"\xEE", dtype=np.uint8).copy()).cuda()
            buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
            n = gs.piece_device(src[1:], len(p), buf[SLACK:SLACK + cap], last=i + 1 == len(pieces))
            host = buf.cpu().numpy()
            assert n <= cap
            assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
            assert (host[SLACK + n:] == SENTINEL).all(), "bytes past the piece's length were written"
            outs.append(host[SLACK:SLACK + n].tobytes())
    finally:
        if own:
            gs.close()
    return outs


def _one_member(member, content):
    """zlib reads exactly one member that ends with the input: a BFINAL before
    the last block, a wrong CRC-32 or ISIZE would each end it otherwise."""
    d = zlib.decompressobj(31)
    out = d.decompress(member)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    assert out == content
    assert struct.unpack("<II", member[-8:]) == (zlib.crc32(content), len(content) & 0xFFFFFFFF)


def _walk(member, content):
    """inflate_ref stops at the first block with BFINAL: it is the member's
    last, an empty stored one, with only the trailer after it."""
    out, end, walk = ir.inflate(member, 10)
    assert out == content and end + 8 == len(member)
    assert walk[-1]["btype"] == 0 and walk[-1]["stored"] == 0
    assert member[end - 5:end] == FINAL
    return walk


@pytest.mark.parametrize("kind", KINDS)
def test_many_pieces_are_one_member(kind):
    content = _content(kind)
    pieces = _cut(content, LENS)
    outs = _write(pieces)
    assert outs[0].startswith(HEADER) and not any(o.startswith(HEADER) for o in outs[1:])
    assert outs[3] == b"", "an empty piece that is not the last writes nothing"
    assert outs[-1] == FINAL + struct.pack("<II", zlib.crc32(content), len(content)), \
        "an empty last piece: the final block and the trailer"
    for p, o in zip(pieces, outs):
        if p:   # the joiner: every piece is whole bytes
            assert o.endswith(JOINER_TAIL)
        assert len(o) <= archive.gzip_stream_bound(len(p))
    member = b"".join(outs)
    _one_member(member, content)
    walk = _walk(member, content)
    # a block per span and a joiner per piece, then the final block
    spans = sum(-(-len(p) // SPAN) for p in pieces)
    assert len(walk) == spans + sum(1 for p in pieces if p) + 1
    kinds = {b["btype"] for b in walk if b["btype"] or b["stored"]}
    # (the one-byte piece is a fixed block whatever the content)
    assert {"text": {2}, "zeros": set(), "random": {0}, "mixed": {0, 2}}[kind] <= kinds, kinds
    if kind == "text":
        assert len(member) < len(content) // 2
    if kind == "zeros":
        assert len(member) < len(content) // 100


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, SPAN - 1, SPAN, SPAN + 1])
def test_one_piece(kind, n):
    content = _content(kind)[:n]
    (member,) = _write([content])
    assert member.startswith(HEADER)
    _one_member(member, content)
    walk = _walk(member, content)
    assert len(walk) == -(-n // SPAN) + 2


def test_a_stream_with_no_bytes_is_a_whole_member():
    for pieces in ([b""], [b"", b"", b""]):
        outs = _write(pieces)
        assert outs[:-1] == [b""] * (len(pieces) - 1)
        assert outs[-1] == HEADER + FINAL + bytes(8)
        _one_member(outs[-1], b"")


def _end_bit_piece(b, salt):
    """Eight distinct bytes, b of them >= 144: no match and no repeat, so the
    fixed code takes 3 + 8 (8 - b) + 9 b + 7 = 74 + b bits, against 104 or more
    stored and more than 100 for a dynamic header alone."""
    lo = [(17 * salt + 13 * i) % 144 for i in range(8 - b)]
    hi = [144 + (11 * salt + 7 * i) % 112 for i in range(b)]
    p = bytes(lo + hi)
    assert len(set(p)) == 8
    return p


def test_every_end_bit():
    # each b twice: as a piece that follows a joiner (bit 0) and, in a second
    # stream, as the first piece (bit 80)
    for first in range(8):
        order = [(first + i) % 8 for i in range(8)]
        pieces = [_end_bit_piece(b, first) for b in order]
        outs = _write(pieces + [b""])
        member = b"".join(outs)
        content = b"".join(pieces)
        _one_member(member, content)
        walk = _walk(member, content)
        assert [w["btype"] for w in walk] == [1, 0] * 8 + [0]
        ends = set()
        at = 80
        for i, b in enumerate(order):
            blk, joiner = walk[2 * i], walk[2 * i + 1]
            assert blk["bit0"] == at and at % 8 == 0, "a piece starts at bit 0 of a byte"
            assert blk["bit1"] - blk["bit0"] == 74 + b
            assert blk["bit1"] % 8 == (2 + b) % 8
            ends.add(blk["bit1"] % 8)
            assert joiner["bit0"] == blk["bit1"] and joiner["stored"] == 0
            # 000, zeros to the byte boundary, LEN, NLEN: from bit 6 on the header spills into the next byte
            assert joiner["bit1"] == (blk["bit1"] + 3 + 7) // 8 * 8 + 32
            at = joiner["bit1"]
            assert len(outs[i]) == (10 if i == 0 else 0) + (joiner["bit1"] - blk["bit0"]) // 8
        assert ends == set(range(8))


def test_where_the_pieces_are_cut_does_not_change_what_inflates():
    content = _content("mixed")[:5 * SPAN + 4321]
    n = len(content)
    ways = [[n],
            [SPAN, SPAN, SPAN, n - 3 * SPAN],
            [1, 4999, 0, SPAN + 77, 1, 2 * SPAN - 3, n - (1 + 4999 + SPAN + 77 + 1 + 2 * SPAN - 3)]]
    members = []
    for lens in ways:
        member = b"".join(_write(_cut(content, lens)))
        _one_member(member, content)
        _walk(member, content)
        members.append(member)
    assert members[0] != members[2], "the cuts differ, so do the compressed bytes; what inflates does not"


def test_encode_is_untouched():
    blobs = [_content("text")[:70001], _content("mixed")[:SPAN + 5], b"\x07" * 300]
    before = encode.encode_blobs(blobs, compress="GZIP")
    _write(_cut(_content("text")[:3 * SPAN + 9], [SPAN, 9, 2 * SPAN]))
    with archive.GzipStream() as gs:     # a writer left open across the call
        gs.piece(_content("random")[:1000])
        during = encode.encode_blobs(blobs, compress="GZIP")
        gs.piece(b"", last=True)
    after = encode.encode_blobs(blobs, compress="GZIP")
    assert before == during == after
    assert [zlib.decompress(m, 31) for m in after] == blobs


def test_host_bytes_interface():
    content = _content("text")[:100000]
    with archive.GzipStream() as gs:
        member = gs.piece(content[:40000]) + gs.piece(b"") + gs.piece(np.frombuffer(content[40000:], np.uint8),
                                                                       last=True)
    _one_member(member, content)


def test_short_out_cap_writes_nothing_and_keeps_the_writer():
    content = _content("mixed")[:2 * SPAN + 100]
    a, b = content[:SPAN + 1], content[SPAN + 1:]
    with archive.GzipStream() as gs:
        src =torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).cuda()
        cap = archive.gzip_stream_bound(len(a))
        buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        n1 = gs.piece_device(src, len(a), buf[SLACK:SLACK + cap])
        first = buf[SLACK:SLACK + n1].cpu().numpy().tobytes()
        # the second piece with room for all but its last byte, for half of it and for none
        src2 = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
        cap2 = archive.gzip_stream_bound(len(b))
        probe = torch.empty(cap2, dtype=torch.uint8, device="cuda")
        with archive.GzipStream() as twin:     # the same two pieces: the second one's true length
            twin.piece_device(src, len(a), probe)
            need = twin.piece_device(src2, len(b), probe, last=True)
        for short in (need - 1, need // 2, 0):
            buf = torch.full((SLACK + cap2 + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
            with pytest.raises(_lib.CdcError) as e:
                gs.piece_device(src2, len(b), buf[SLACK:], last=True, out_cap=short)
            assert e.value.status == _lib.CDC_E_NOSPACE
            assert (buf.cpu().numpy() == SENTINEL).all(), "nothing is written when the piece does not fit"
        buf = torch.full((SLACK + need + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        n2 = gs.piece_device(src2, len(b), buf[SLACK:], last=True, out_cap=need)   # exactly enough
        host = buf.cpu().numpy()
        assert n2 == need and (host[:SLACK] == SENTINEL).all() and (host[SLACK + n2:] == SENTINEL).all()
        _one_member(first + host[SLACK:SLACK + n2].tobytes(), content)
        with pytest.raises(_lib.CdcError) as e:   # the member is closed
            gs.piece_device(src2, 1, buf[SLACK:])
        assert e.value.status == _lib.CDC_E_INVALID
