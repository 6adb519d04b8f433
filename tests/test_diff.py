"""Diff end to end: backup_files, then DiffSession over the objects and
packfiles, against difflib's unified diff of the original bytes split by the
Go rule (diff_ref.expected_diff), over LZ4 + key, GZIP + key and plain."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import diff_ref  # noqa: E402
import pack_loss  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, restore, snapshot  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
MIB = 1 << 20
CODECS = [(KEY, "LZ4"), (KEY, "GZIP"), (None, None)]


def _text(n, seed, width=40):
    """n lines of words, some of them repeated."""
    rng = np.random.default_rng(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"{", b"}", b"return", b"x = x + 1;", b"\xc3\xa9t\xc3\xa9"]
    out = []
    for i in range(n):
        k = int(rng.integers(0, 6))
        out.append(b" ".join(words[int(j)] for j in rng.integers(0, len(words), k)) + (b" %d" % i if i % 3 else b""))
    return b"\n".join(out) + b"\n"


def _autojunk_text():
    """600 lines, every third one "}": popular in b, so matches never start on it."""
    return b"".join(b"}\n" if i % 3 == 2 else b"stmt %d;\n" % i for i in range(600))


def _pairs():
    """(name, a, b) of the text cases, the binary, and the big shared text."""
    t300 = _text(300, 1)
    l300 = t300.split(b"\n")
    changed = list(l300)
    changed[140] = b"changed \xff line"
    aj = _autojunk_text().split(b"\n")
    aj_b = aj[:200] + [b"new one", b"}"] + aj[206:400] + aj[420:]
    rnd = random_bytes(3 * MIB, 31).tobytes()
    rnd_b = bytearray(rnd)
    for k in range(10):
        rnd_b[100_000 + 290_000 * k] ^= 0x55
    big = b"".join(b"%07d the quick brown fox jumps over the lazy dog again\n" % i for i in range(120_000))
    assert len(big) > 6 * MIB
    mid = len(big) // 2
    cut = big.index(b"\n", mid) + 1
    big_b = big[:cut] + b"an inserted line\nand another\n" + big[big.index(b"\n", cut + 200) + 1:]
    return [("one line of 300", t300, b"\n".join(changed)),
            ("trailing newline", b"a\nb\nc\n", b"a\nb\nc"),
            ("empty against text", b"", b"one\ntwo\n"),
            ("text against empty", b"one\ntwo\n", b""),
            ("crlf against lf", t300[:2000].replace(b"\n", b"\r\n"), t300[:2000]),
            ("autojunk", b"\n".join(aj), b"\n".join(aj_b)),
            ("binary", rnd, bytes(rnd_b)),
            ("big text", big, big_b)]


def _write(d, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = d / f"f{i:04d}"
        p.write_bytes(b)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    pairs = _pairs()
    files = [x for _, a, b in pairs for x in (a, b)]
    return _write(tmp_path_factory.mktemp("diff"), files), pairs


@pytest.fixture(scope="module")
def backups(corpus):
    paths, _ = corpus
    made = {}

    def get(key, compression):
        if (key, compression) not in made:
            repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))  # about 100 chunks in the 6-MiB text
            objs, packs, _ = snapshot.backup_files(paths, repo=repo, key=key, compression=compression, max_size=2 << 20,
                                                   timestamp=5)
            made[(key, compression)] = (objs, packs)
        return made[(key, compression)]
    return get


@pytest.fixture(scope="module")
def expected(corpus):
    """difflib over the original bytes, once."""
    _, pairs = corpus
    return [diff_ref.expected_diff(a, b, b"old/" + name.encode(), b"new/" + name.encode()) for name, a, b in pairs]


def _jobs(objs, pairs):
    return [(objs[2 * i], objs[2 * i + 1], "old/" + name, "new/" + name) for i, (name, _, _) in enumerate(pairs)]


@pytest.mark.parametrize("key,compression", CODECS)
def test_every_case_is_difflibs_text(corpus, backups, expected, key, compression):
    _, pairs = corpus
    objs, packs = backups(key, compression)
    res, st = snapshot.diff_files(_jobs(objs, pairs), packs, key=key, compression=compression)
    for i, ((name, a, b), r, want) in enumerate(zip(pairs, res, expected)):
        assert r["status"] == 0 and r["bad_side"] == -1 and r["bad_chunk"] == -1, (name, r["status"])
        assert r["text"] == want, name
        assert r["a_lines"] == a.count(b"\n") + 1 and r["b_lines"] == b.count(b"\n") + 1, name
        assert r["hunks"] == want.count(b"\n@@ -") and not r["identical"], name
    assert st["pairs"] == len(pairs) and st["failed_pairs"] == 0 and st["skipped_pairs"] == 0 and st["batches"] == 1
    assert st["hunks"] == sum(r["hunks"] for r in res) and st["out_bytes"] == sum(len(w) for w in expected)
    assert st["lines"] == sum(r["a_lines"] + r["b_lines"] for r in res)
    assert 0 < st["distinct_lines"] < st["lines"] and st["verify_rounds"] == 1
    # the autojunk text shows the rule: without it difflib gives another text
    import difflib
    name, a, b = pairs[5]
    la, lb = diff_ref.split_lines(a), diff_ref.split_lines(b)
    assert 200 <= len(lb) and difflib.SequenceMatcher(None, la, lb).bpopular


def test_shared_chunks_decode_once(corpus, backups):
    """The 6-MiB text edited in the middle: the two versions share most of
    their chunks, and every distinct blob is decoded once."""
    _, pairs = corpus
    objs, packs = backups(KEY, "LZ4")
    i = [n for n, _, _ in pairs].index("big text")
    res, st = snapshot.diff_files([_jobs(objs, pairs)[i]], packs, key=KEY, compression="LZ4")
    distinct = {bytes(c.Checksum) for o in objs[2 * i:2 * i + 2] for c in o.Chunks}
    assert st["segments"] == len(objs[2 * i].Chunks) + len(objs[2 * i + 1].Chunks) > 40
    assert st["decoded_blobs"] == st["distinct_blobs"] == len(distinct) < st["segments"] * 0.6
    assert st["decoded_bytes"] < 0.6 * st["bytes"]
    assert res[0]["hunks"] == 1


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """200 small pairs; 7, 90 and 199 are identical (the same bytes on both sides)."""
    blobs, want = [], []
    for i in range(200):
        a = _text(20 + i % 50, 100 + i)
        la = a.split(b"\n")
        lb = list(la)
        if i not in (7, 90, 199):
            lb[i % len(la)] = b"pair %d" % i
            if i % 4 == 0:
                del lb[2:4]
        b = b"\n".join(lb)
        blobs += [a, b]
        want.append(diff_ref.expected_diff(a, b, b"a/%d" % i, b"b/%d" % i))
    paths = _write(tmp_path_factory.mktemp("small"), blobs)
    objs, packs, _ = snapshot.backup_files(paths, key=KEY, compression="LZ4", timestamp=6)
    jobs = [(objs[2 * i], objs[2 * i + 1], "a/%d" % i, "b/%d" % i) for i in range(200)]
    return jobs, packs, want, blobs


def test_a_batch_of_small_pairs_and_the_same_in_three_batches(small):
    jobs, packs, want, blobs = small
    res, st = snapshot.diff_files(jobs, packs, key=KEY, compression="LZ4")
    assert [r["text"] for r in res] == want
    for i in (7, 90, 199):
        assert res[i]["identical"] and res[i]["text"] == b"" and res[i]["a_lines"] == 0 and res[i]["hunks"] == 0
    assert st["skipped_pairs"] == 3 == st["identical_pairs"] and st["batches"] == 1 and st["failed_pairs"] == 0
    used = {bytes(c.Checksum) for i, j in enumerate(jobs) if i not in (7, 90, 199) for o in j[:2] for c in o.Chunks}
    assert st["distinct_blobs"] == st["decoded_blobs"] == len(used)  # the identical pairs' blobs are not read
    assert st["bytes"] == sum(len(blobs[2 * i]) + len(blobs[2 * i + 1]) for i in range(200) if i not in (7, 90, 199))
    total = st["bytes"]
    res3, st3 = snapshot.diff_files(jobs, packs, key=KEY, compression="LZ4", batch_bytes=total // 3 + 2000)
    assert st3["batches"] == 3 and [r["text"] for r in res3] == want
    assert st3["lines"] == st["lines"] and st3["hunks"] == st["hunks"] and st3["out_bytes"] == st["out_bytes"]
    # only identical pairs: no device work at all
    res0, st0 = snapshot.diff_files([jobs[7], jobs[90]], packs, key=KEY, compression="LZ4")
    assert st0["batches"] == 0 and st0["decoded_blobs"] == 0 and st0["lines"] == 0 and all(r["identical"] for r in res0)
    # object checksums that are equal settle a pair before its chunk lists are looked at
    a = jobs[0][0]
    fake = types.SimpleNamespace(Chunks=jobs[0][1].Chunks, Checksum=a.Checksum)
    res1, st1 = snapshot.diff_files([(a, fake, "x", "y")], packs, key=KEY, compression="LZ4")
    assert res1[0]["identical"] and st1["skipped_pairs"] == 1 and st1["batches"] == 0
    # and without object checksums the chunk lists decide
    nosum = [types.SimpleNamespace(Chunks=o.Chunks, Checksum=None) for o in jobs[7][:2]]
    res2, st2 = snapshot.diff_files([(nosum[0], nosum[1], "x", "y"), jobs[3]], packs, key=KEY, compression="LZ4")
    assert res2[0]["identical"] and st2["skipped_pairs"] == 1 and res2[1]["text"] == want[3]


def test_hash_collisions_do_not_change_the_output(small, corpus, backups, expected):
    jobs, packs, want, _ = small
    res, st = snapshot.diff_files(jobs[:40], packs, key=KEY, compression="LZ4", hash_bits=4)
    assert [r["text"] for r in res] == want[:40]
    assert st["verify_rounds"] > 1
    _, pairs = corpus
    objs, packs = backups(None, None)
    res, st = snapshot.diff_files(_jobs(objs, pairs)[:6], packs, key=None, compression=None, hash_bits=4)
    assert [r["text"] for r in res] == expected[:6] and st["verify_rounds"] > 1


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
def test_a_damaged_blob_fails_exactly_its_pairs(corpus, backups, expected, key, compression, status):
    _, pairs = corpus
    objs, packs = backups(key, compression)
    i = [n for n, _, _ in pairs].index("big text")
    b_sums = [bytes(c.Checksum) for c in objs[2 * i + 1].Chunks]
    a_sums = [bytes(c.Checksum) for c in objs[2 * i].Chunks]
    only_b = [s for s in b_sums if s not in a_sums]
    victim = only_b[0]
    jobs = _jobs(objs, pairs)
    # the big pair twice (both fail), and a pair of a's version with itself by other names (does not use the blob)
    third = (objs[2 * i], objs[0], "p", "q")
    res, st = snapshot.diff_files(jobs + [jobs[i], third], _damage(packs, victim), key=key, compression=compression)
    for k, r in enumerate(res):
        if k in (i, len(jobs)):
            assert (r["status"], r["bad_side"], r["bad_chunk"], r["text"]) == (status, 1, b_sums.index(victim), b""), (k, r["status"])
        else:
            assert r["status"] == 0, k
    assert res[:i] + res[i + 1:len(jobs)] and [r["text"] for r in res[:i]] == expected[:i]
    assert st["failed_pairs"] == 2
    shared = [s for s in a_sums if s in b_sums][3]
    res, _ = snapshot.diff_files(jobs, _damage(packs, shared), key=key, compression=compression)
    assert (res[i]["status"], res[i]["bad_side"], res[i]["bad_chunk"]) == (status, 0, a_sums.index(shared))
    assert all(r["status"] == 0 for k, r in enumerate(res) if k != i)


def _obj(chunks, checksum=None):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks], Checksum=checksum)


def test_missing_chunk_and_oversized_pair(corpus, backups, expected):
    _, pairs = corpus
    objs, packs = backups(KEY, "LZ4")
    jobs = _jobs(objs, pairs)
    chunks = [(bytes(c.Checksum), c.Length) for c in objs[1].Chunks]
    missing = _obj(chunks + [(bytes(range(32)), 77)])
    res, st = snapshot.diff_files([jobs[0], (objs[0], missing, "a", "b"), (missing, objs[0], "a", "b"), jobs[1]], packs, key=KEY,
                                  compression="LZ4")
    assert (res[1]["status"], res[1]["bad_side"], res[1]["bad_chunk"]) == (_lib.CDC_E_NOTFOUND, 1, len(chunks))
    assert (res[2]["status"], res[2]["bad_side"], res[2]["bad_chunk"]) == (_lib.CDC_E_NOTFOUND, 0, len(chunks))
    assert res[0]["text"] == expected[0] and res[3]["text"] == expected[1] and st["failed_pairs"] == 2
    # the binary pair (6 MiB) does not fit 4 MiB; the others do
    res, st = snapshot.diff_files(jobs[:7], packs, key=KEY, compression="LZ4", batch_bytes=4 * MIB)
    assert res[6]["status"] == _lib.CDC_E_NOSPACE and res[6]["bad_side"] == -1 and res[6]["text"] == b""
    assert [r["text"] for r in res[:6]] == expected[:6] and st["failed_pairs"] == 1
    # max_lines: the 300-line pair (602 lines) fails alone, the others go in groups of at most 600
    res, st = snapshot.diff_files(jobs[:6], packs, key=KEY, compression="LZ4", max_lines=600)
    assert res[0]["status"] == _lib.CDC_E_NOSPACE and [r["text"] for r in res[1:5]] == expected[1:5]
    assert res[5]["status"] == _lib.CDC_E_NOSPACE  # the autojunk pair has 1,200 lines


def test_reused_session_and_packfiles_by_path(corpus, backups, expected, tmp_path):
    _, pairs = corpus
    objs, packs = backups(KEY, "GZIP")
    jobs = _jobs(objs, pairs)
    with snapshot.DiffSession(KEY, "GZIP", context=3) as s:
        for k, p in enumerate(packs):
            if k % 2:
                s.add_packfile(p)
            else:
                f = tmp_path / f"pack{k}"
                f.write_bytes(p)
                s.add_packfile(f)
        r1, _ = s.run(jobs[:3])
        r2, st2 = s.run(jobs[2:7])
        r3, _ = s.run([])
        assert [r["text"] for r in r1] == expected[:3] and [r["text"] for r in r2] == expected[2:7] and r3 == []
        assert st2["pairs"] == 5
    with pytest.raises(ValueError):
        s.run(jobs[:1])
    with snapshot.DiffSession(KEY, "GZIP", context=1) as s:
        for p in packs:
            s.add_packfile(p)
        r, _ = s.run(jobs[:1])
        name, a, b = pairs[0]
        assert r[0]["text"] == diff_ref.expected_diff(a, b, b"old/" + name.encode(), b"new/" + name.encode(), n=1)


@pytest.mark.parametrize("how", ["removed", "truncated"])
def test_an_unreadable_packfile_fails_exactly_its_pairs(corpus, backups, expected, tmp_path, how):
    """Registered by path, then lost before the run: CDC_E_IO with the side and
    the first lost chunk (a's before b's) for the pairs with a blob there, the
    text of every other pair."""
    _, pairs = corpus
    objs, packs = backups(KEY, "LZ4")
    jobs = _jobs(objs, pairs)
    paths = pack_loss.write_packs(tmp_path, packs)
    with snapshot.DiffSession(KEY, "LZ4", threads=3) as s:
        for q in paths:
            s.add_packfile(q)
        lost = pack_loss.lose(paths, packs, pack_loss.pick(objs, packs), how, objs)
        res, st = s.run(jobs)
    want = []
    for a, b, _, _ in jobs:
        la, lb = pack_loss.first_lost(a, lost), pack_loss.first_lost(b, lost)
        want.append((0, la) if la is not None else (1, lb) if lb is not None else None)
    assert any(w is not None for w in want) and any(w is None for w in want)
    for k, (r, w) in enumerate(zip(res, want)):
        if w is None:
            assert r["status"] == 0 and r["text"] == expected[k], k
        else:
            assert (r["status"], r["bad_side"], r["bad_chunk"], r["text"]) == (_lib.CDC_E_IO, w[0], w[1], b""), (k, r["status"])
    assert st["failed_pairs"] == sum(w is not None for w in want) and st["batches"] == 1


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None)])
@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
def test_a_wrong_recorded_length_fails_its_pair_alone(corpus, backups, expected, key, compression, delta):
    """The first chunk's recorded Length one byte off, on side a and on side b:
    that pair is CDC_E_MISMATCH at that side's chunk 0, the pairs of the same
    batch get their text."""
    _, pairs = corpus
    objs, packs = backups(key, compression)
    jobs = _jobs(objs, pairs)
    i = [n for n, _, _ in pairs].index("binary")
    bad = []
    for side in (0, 1):
        chunks = [(bytes(c.Checksum), c.Length) for c in objs[2 * i + side].Chunks]
        assert len(chunks) >= 2
        (c0, n0) = chunks[0]
        bad.append(_obj([(c0, n0 + delta)] + chunks[1:]))
    more = [(bad[0], objs[2 * i + 1], "a", "b"), (objs[2 * i], bad[1], "a", "b")]
    res, st = snapshot.diff_files(jobs + more, packs, key=key, compression=compression)
    n = len(jobs)
    assert [r["status"] for r in res[:n]] == [0] * n and [r["text"] for r in res[:n]] == expected
    for side in (0, 1):
        r = res[n + side]
        assert (r["status"], r["bad_side"], r["bad_chunk"], r["text"]) == (_lib.CDC_E_MISMATCH, side, 0, b""), side
    assert st["failed_pairs"] == 2 and st["batches"] == 1
