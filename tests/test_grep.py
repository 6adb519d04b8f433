"""Grep end to end: backup_files, then grep_files over the objects and
packfiles, against the judge of tests/grep_ref.py on the original bytes, over
LZ4 + key, GZIP + key and plain.  A hit's `off` is the line's offset in the
file and its `text` the file's index."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import grep_ref as gref  # noqa: E402
import pack_loss  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, grep, restore, snapshot  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
MIB = 1 << 20
CODECS = [(KEY, "LZ4"), (KEY, "GZIP"), (None, None)]
TOKEN = b"needle-in-a-haystack-"
PATTERNS = [b"0012345 the quick", b"PLANTED-STRING", b"needle", TOKEN, b"split-needle", b"an inserted line", b"LAZY DOG again"]
BIG, RND, EMPTY, NO_NEWLINE, BIG_B, STRADDLE, LEFT, RIGHT = range(8)
DEFAULT_LIMIT = 65536


def _files():
    big = b"".join(b"%07d the quick brown fox jumps over the lazy dog again\n" % i for i in range(120_000))
    assert len(big) > 6 * MIB
    cut = big.index(b"\n", len(big) // 2) + 1
    big_b = big[:cut] + b"an inserted line\nand another needle\n" + big[big.index(b"\n", cut + 200) + 1:]
    rnd = bytearray(random_bytes(3 * MIB, 31).tobytes())
    for k in range(12):
        at = 50_000 + 250_000 * k
        rnd[at:at + 14] = b"PLANTED-STRING"
    # a mebibyte without a newline, a token every 28 bytes: some chunk cut falls inside one
    straddle = b"first line\n" + b"".join(TOKEN + b"%06d " % i for i in range(MIB // 28)) + b"\nlast line with a needle\n"
    return [big, bytes(rnd), b"", b"alpha\nbeta needle\ngamma needle", big_b, straddle,
            b"the left file ends in split-ne", b"edle: the right file starts with the rest\nsplit-needle whole\n"]


def _write(d, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = d / f"f{i:04d}"
        p.write_bytes(b)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    files = _files()
    return _write(tmp_path_factory.mktemp("grep"), files), files


@pytest.fixture(scope="module")
def backups(corpus):
    paths, _ = corpus
    made = {}

    def get(key, compression, form="plain"):
        if (key, compression, form) not in made:
            repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))  # about 100 chunks in the 6-MiB text
            objs, packs, _ = snapshot.backup_files(paths, repo=repo, key=key, compression=compression, max_size=2 << 20,
                                                   timestamp=5, packfile_form=form)
            made[(key, compression, form)] = (objs, packs)
        return made[(key, compression, form)]
    return get


@pytest.fixture(scope="module")
def judged(corpus):
    """The judge over the original bytes, once per flag setting: per file (hits, lines, binary)."""
    _, files = corpus
    return {ic: [gref.grep_text(f, PATTERNS, ic, index=i) for i, f in enumerate(files)] for ic in (False, True)}


def _hits(want, limit=DEFAULT_LIMIT):
    return np.array(want[0][:limit], dtype=grep.HIT_DTYPE)


def _holds(r, want, size, limit=DEFAULT_LIMIT, what=""):
    assert (r["status"], r["bad_chunk"]) == (0, -1), (what, r["status"])
    assert (r["size"], r["lines"], r["matched"], r["binary"]) == (size, want[1], len(want[0]), want[2]), what
    assert np.array_equal(r["hits"], _hits(want, limit)), what


@pytest.mark.parametrize("ignore_case", [False, True])
@pytest.mark.parametrize("key,compression", CODECS)
def test_every_file_is_the_judges(corpus, backups, judged, key, compression, ignore_case):
    _, files = corpus
    objs, packs = backups(key, compression)
    res, st = snapshot.grep_files(objs, packs, PATTERNS, key=key, compression=compression, ignore_case=ignore_case)
    want = judged[ignore_case]
    for i, (f, r) in enumerate(zip(files, res)):
        _holds(r, want[i], len(f), what=i)
        assert r["text"] == b""
    # what the cases are there for
    assert len(res[BIG]["hits"]) == (DEFAULT_LIMIT if ignore_case else 1) and res[BIG]["matched"] == (120_000 if ignore_case else 1)
    assert res[RND]["binary"] and len(res[RND]["hits"]) >= 12
    assert res[EMPTY]["lines"] == 0 and res[NO_NEWLINE]["hits"]["line"].tolist() == [2, 3]
    assert res[STRADDLE]["hits"]["nocc"].tolist() == [2 * (MIB // 28), 1]
    assert res[LEFT]["matched"] == 0 and res[RIGHT]["hits"]["line"].tolist() == [2]  # nothing across the two files
    assert st["files"] == len(files) and st["failed_files"] == 0 and st["batches"] == 1
    assert st["bytes"] == sum(len(f) for f in files) and st["lines"] == sum(w[1] for w in want)
    assert st["matched_lines"] == sum(len(w[0]) for w in want)
    assert st["hits"] == sum(min(len(w[0]), DEFAULT_LIMIT) for w in want)
    assert st["occurrences"] == sum(h[6] for w in want for h in w[0][:DEFAULT_LIMIT]) and st["out_bytes"] == 0


def test_a_planted_string_straddles_a_chunk_cut(corpus, backups):
    """The premise of the straddle file, from the object's chunk lengths."""
    _, files = corpus
    objs, _ = backups(KEY, "LZ4")
    cuts = np.cumsum([c.Length for c in objs[STRADDLE].Chunks])[:-1]
    first = len(b"first line\n")
    inside = [int(c) for c in cuts if first < c < first + 28 * (MIB // 28) and 0 < (int(c) - first) % 28 < len(TOKEN)]
    assert inside, cuts.tolist()
    c = inside[0]
    assert files[STRADDLE][c - (c - first) % 28:].startswith(TOKEN)


def test_shared_chunks_decode_once(corpus, backups, judged):
    objs, packs = backups(KEY, "LZ4")
    res, st = snapshot.grep_files([objs[BIG], objs[BIG_B]], packs, PATTERNS, key=KEY, compression="LZ4")
    distinct = {bytes(c.Checksum) for o in (objs[BIG], objs[BIG_B]) for c in o.Chunks}
    assert st["segments"] == len(objs[BIG].Chunks) + len(objs[BIG_B].Chunks) > 40
    assert st["decoded_blobs"] == st["distinct_blobs"] == len(distinct) < st["segments"] * 0.6
    # line 0012345, the inserted line and the one after it; `text` is the index in `files` of this call
    assert res[1]["hits"]["text"].tolist() == [1, 1, 1] and res[1]["matched"] == 3
    assert [h[1:] for h in res[1]["hits"].tolist()] == [h[1:] for h in judged[False][BIG_B][0]]


def test_text_limit_and_two_queries_on_one_session(corpus, backups, judged):
    _, files = corpus
    objs, packs = backups(KEY, "GZIP")
    with snapshot.GrepSession(KEY, "GZIP") as s:
        for p in packs:
            s.add_packfile(p)
        for width in (1, 16, 0):
            res, st = s.run(objs, PATTERNS, ignore_case=True, limit=5, want_text=True, max_line_bytes=width)
            for i, (f, r) in enumerate(zip(files, res)):
                _holds(r, judged[True][i], len(f), limit=5, what=(width, i))
                assert r["text"] == gref.text_of(f, judged[True][i][0][:5], width or 4096), (width, i)
            assert st["out_bytes"] == sum(len(r["text"]) for r in res) > 0 and st["hits"] == sum(len(r["hits"]) for r in res)
        res, st = s.run(objs[3:], [b"gamma", b"\r", b"whole"], want_text=True)
        want = [gref.grep_text(f, [b"gamma", b"\r", b"whole"], index=i) for i, f in enumerate(files[3:])]
        for i, (f, r) in enumerate(zip(files[3:], res)):
            _holds(r, want[i], len(f), what=i)
            assert r["text"] == gref.text_of(f, want[i][0], 4096)
        assert s.run([], PATTERNS)[0] == []
        for bad in ([], [b"a\nb"], [b""], [b"x"] * 33):
            with pytest.raises(_lib.CdcError) as e:
                s.run(objs[:1], bad)
            assert e.value.status == _lib.CDC_E_INVALID
    with pytest.raises(ValueError):
        s.run(objs[:1], PATTERNS)


def test_three_batches_give_the_same(corpus, backups, judged):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    res, st = snapshot.grep_files(objs, packs, PATTERNS, key=KEY, compression="LZ4", batch_bytes=8 * MIB, want_text=True,
                                  max_line_bytes=16, max_lines=200_000)
    assert st["batches"] == 3 and st["failed_files"] == 0
    for i, (f, r) in enumerate(zip(files, res)):
        _holds(r, judged[False][i], len(f), what=i)
        assert r["text"] == gref.text_of(f, judged[False][i][0], 16)
    # one batch, its files in groups of at most 125,000 lines: each big text alone
    res, st = snapshot.grep_files(objs, packs, PATTERNS, key=KEY, compression="LZ4", max_lines=125_000)
    assert st["batches"] == 1 and st["failed_files"] == 0
    for i, (f, r) in enumerate(zip(files, res)):
        _holds(r, judged[False][i], len(f), what=i)


def _damage(packs, checksum):
    out, hit = [], 0
    for p in packs:
        _, rows = restore.packfile_index(p)
        for _, c, o, n in rows:
            if c == checksum and n:
                b = bytearray(p)
                b[o + n // 2] ^= 0x10
                p = bytes(b)
                hit += 1
        out.append(p)
    assert hit == 1
    return out


@pytest.mark.parametrize("key,compression,status", [(KEY, "LZ4", _lib.CDC_E_AUTH), (None, None, _lib.CDC_E_MISMATCH)])
def test_a_damaged_blob_fails_exactly_its_files(corpus, backups, judged, key, compression, status):
    _, files = corpus
    objs, packs = backups(key, compression)
    a_sums = [bytes(c.Checksum) for c in objs[BIG].Chunks]
    b_sums = [bytes(c.Checksum) for c in objs[BIG_B].Chunks]
    victim = [s for s in b_sums if s not in a_sums][0]
    res, st = snapshot.grep_files(objs, _damage(packs, victim), PATTERNS, key=key, compression=compression)
    for i, (f, r) in enumerate(zip(files, res)):
        if i == BIG_B:
            assert (r["status"], r["bad_chunk"], r["matched"], len(r["hits"])) == (status, b_sums.index(victim), 0, 0)
        else:
            _holds(r, judged[False][i], len(f), what=i)
    assert st["failed_files"] == 1
    shared = [s for s in a_sums if s in b_sums][3]
    res, st = snapshot.grep_files(objs, _damage(packs, shared), PATTERNS, key=key, compression=compression)
    for i, (f, r) in enumerate(zip(files, res)):
        if i in (BIG, BIG_B):
            assert (r["status"], r["bad_chunk"]) == (status, (a_sums if i == BIG else b_sums).index(shared)), i
        else:
            _holds(r, judged[False][i], len(f), what=i)
    assert st["failed_files"] == 2


def _obj(chunks):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks], Checksum=None)


def test_missing_chunk_oversized_file_and_too_many_lines(corpus, backups, judged):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    chunks = [(bytes(c.Checksum), c.Length) for c in objs[NO_NEWLINE].Chunks]
    missing = _obj(chunks + [(bytes(range(32)), 77)])
    order = [NO_NEWLINE, None, RND, RIGHT]
    res, st = snapshot.grep_files([objs[i] if i is not None else missing for i in order], packs, PATTERNS, key=KEY, compression="LZ4")
    assert (res[1]["status"], res[1]["bad_chunk"], res[1]["matched"]) == (_lib.CDC_E_NOTFOUND, len(chunks), 0)
    for k in (0, 2, 3):
        want = gref.grep_text(files[order[k]], PATTERNS, index=k)
        _holds(res[k], want, len(files[order[k]]), what=k)
    assert st["failed_files"] == 1
    # the two big texts do not fit 4 MiB; the others do
    res, st = snapshot.grep_files(objs, packs, PATTERNS, key=KEY, compression="LZ4", batch_bytes=4 * MIB)
    for i, (f, r) in enumerate(zip(files, res)):
        if i in (BIG, BIG_B):
            assert (r["status"], r["bad_chunk"], len(r["hits"])) == (_lib.CDC_E_NOSPACE, -1, 0)
        else:
            _holds(r, judged[False][i], len(f), what=i)
    assert st["failed_files"] == 2
    # max_lines: the texts of 120,000 lines fail alone
    res, st = snapshot.grep_files(objs, packs, PATTERNS, key=KEY, compression="LZ4", max_lines=100_000)
    assert [r["status"] for r in res] == [_lib.CDC_E_NOSPACE if i in (BIG, BIG_B) else 0 for i in range(len(files))]
    _holds(res[RND], judged[False][RND], len(files[RND]))


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None)])
def test_stored_packfiles_and_rows_give_the_same_hits(corpus, backups, judged, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    objs_s, packs_s = backups(key, compression, "stored")
    res, _ = snapshot.grep_files(objs_s, packs_s, PATTERNS, key=key, compression=compression, packfile_form="stored")
    for i, (f, r) in enumerate(zip(files, res)):
        _holds(r, judged[False][i], len(f), what=i)
    rows = [restore.packfile_index(p)[1] for p in packs]
    with snapshot.GrepSession(key, compression) as s:
        assert s.add_packfiles(packs, rows=rows) == [0] * len(packs)
        res, _ = s.run(objs, PATTERNS)
    for i, (f, r) in enumerate(zip(files, res)):
        _holds(r, judged[False][i], len(f), what=i)


@pytest.mark.parametrize("how", ["removed", "truncated"])
def test_an_unreadable_packfile_fails_exactly_its_files(corpus, backups, judged, tmp_path, how):
    """Registered by path, then lost before the run: CDC_E_IO and the first
    lost chunk for the files with a blob there, every other file searched."""
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    paths = pack_loss.write_packs(tmp_path, packs)
    with snapshot.GrepSession(KEY, "LZ4", threads=3) as s:
        for q in paths:
            s.add_packfile(q)
        lost = pack_loss.lose(paths, packs, pack_loss.pick(objs, packs), how, objs)
        res, st = s.run(objs, PATTERNS)
    want = [pack_loss.first_lost(o, lost) for o in objs]
    assert any(w is not None for w in want) and any(w is None and f for w, f in zip(want, files))
    for i, (f, r, w) in enumerate(zip(files, res, want)):
        if w is None:
            _holds(r, judged[False][i], len(f), what=i)
        else:
            assert (r["status"], r["bad_chunk"], r["matched"], len(r["hits"])) == (_lib.CDC_E_IO, w, 0, 0), i
    assert st["failed_files"] == sum(w is not None for w in want) and st["batches"] == 1


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None)])
@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
def test_a_wrong_recorded_length_fails_its_file_alone(corpus, backups, judged, key, compression, delta):
    """The first chunk's recorded Length one byte off: that file is
    CDC_E_MISMATCH at chunk 0, the files of the same batch are searched."""
    _, files = corpus
    objs, packs = backups(key, compression)
    chunks = [(bytes(c.Checksum), c.Length) for c in objs[STRADDLE].Chunks]
    assert len(chunks) >= 2
    (c0, n0) = chunks[0]
    res, st = snapshot.grep_files(list(objs) + [_obj([(c0, n0 + delta)] + chunks[1:])], packs, PATTERNS, key=key,
                                  compression=compression)
    n = len(files)
    for i, (f, r) in enumerate(zip(files, res[:n])):
        _holds(r, judged[False][i], len(f), what=i)
    assert (res[n]["status"], res[n]["bad_chunk"], res[n]["matched"], len(res[n]["hits"])) == (_lib.CDC_E_MISMATCH, 0, 0, 0)
    assert st["failed_files"] == 1 and st["batches"] == 1
