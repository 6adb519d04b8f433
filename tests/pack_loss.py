"""Packfiles on disk that a run can no longer read, for the error-path tests of
the packfile readers: the packfiles are registered by path (footer and index
are read then), one of them is removed or cut short, and the run that follows
must fail exactly the blobs that lay in the lost bytes with CDC_E_IO."""
import os

from plakar_amd import restore


def write_packs(d, packs):
    paths = []
    for i, p in enumerate(packs):
        q = d / f"pack{i}"
        q.write_bytes(p)
        paths.append(str(q))
    return paths


def first_home(packs):
    """checksum -> (packfile, offset, length) of its first row: the locator's rule."""
    home = {}
    for k, p in enumerate(packs):
        for _, c, o, n in restore.packfile_index(p)[1]:
            home.setdefault(bytes(c), (k, o, n))
    return home


def pick(objs, packs):
    """A packfile that some of the objects need and some non-empty ones do not:
    the one the fewest objects need."""
    home = first_home(packs)
    users = {}
    for i, o in enumerate(objs):
        for c in o.Chunks:
            users.setdefault(home[bytes(c.Checksum)][0], set()).add(i)
    nonempty = sum(1 for o in objs if o.Chunks)
    ok = [k for k, u in users.items() if len(u) < nonempty]
    assert ok, "every packfile is needed by every object"
    return min(ok, key=lambda k: (len(users[k]), k))


def lose(paths, packs, k, how, objs):
    """Remove paths[k], or cut it inside the middle one of the blobs the objects
    use there.  Returns the checksums whose blobs cannot be read any more."""
    home = first_home(packs)
    here = sorted({(o, n, c) for c, (p, o, n) in home.items() if p == k} &
                  {home[bytes(c.Checksum)][1:] + (bytes(c.Checksum),) for obj in objs for c in obj.Chunks})
    assert here, "no object uses that packfile"
    if how == "removed":
        os.remove(paths[k])
        return {c for c, (p, _, _) in home.items() if p == k}
    assert how == "truncated"
    cut = here[len(here) // 2][0] + 1
    os.truncate(paths[k], cut)
    return {c for c, (p, o, n) in home.items() if p == k and n and o + n > cut}


def first_lost(obj, lost):
    """The index of the object's first chunk among the lost ones, or None."""
    return next((i for i, c in enumerate(obj.Chunks) if bytes(c.Checksum) in lost), None)
