"""Mirror of the plakar call sites around the chunker.

    (*Repository).Chunker(rd)   repository/repository.go:283-294
    chunkify routing            snapshot/backup.go:631-666

Only the parts on the chunking path: the repository's Chunking configuration
drives the chunker exactly as the Go code does (algorithm name lower-cased,
sizes widened to int).
"""
from . import chunkers
from .chunking import Configuration, DefaultConfiguration


class Repository:
    def __init__(self, chunking: Configuration = None):
        self._chunking = chunking or DefaultConfiguration()

    def Configuration(self):
        return self

    @property
    def Chunking(self):
        return self._chunking

    def Chunker(self, rd):
        """repository/repository.go:283-294."""
        c = self._chunking
        return chunkers.NewChunker(c.Algorithm.lower(), rd, chunkers.ChunkerOpts(
            MinSize=int(c.MinSize), NormalSize=int(c.NormalSize), MaxSize=int(c.MaxSize)))

    def RebuildState(self, states, ids=None, key=None, compression="LZ4", form="stored", device=0):
        """repository/repository.go:58-164: merge the repository's state files
        (bytes as stored, named by ids) into the aggregate the queries below
        answer from.  Called again, it adds states to the same aggregate, as
        the reference fetches only the states its cache lacks.  Returns the
        per-state statuses (state.State.merge)."""
        from . import state
        if getattr(self, "_state", None) is None:
            self._state = state.State(key=key, compression=compression, device=device)
        return self._state.merge(states, ids=ids, form=form)

    def State(self):
        """The aggregate (state.State) RebuildState built; ValueError before it ran."""
        if getattr(self, "_state", None) is None:
            raise ValueError("RebuildState has not run")
        return self._state

    def BlobExists(self, type, checksums):
        """repository.go:468-475 over state.BlobExists, for many checksums at once."""
        return self.State().blob_exists(type, checksums)

    def GetSubpartForBlob(self, type, checksums):
        """state.GetSubpartForBlob as repository.go:449-466 calls it, for many checksums."""
        return self.State().get_subpart_for_blob(type, checksums)

    def ListSnapshots(self):
        """repository.go:477-484 over state.ListSnapshots."""
        return self.State().list_snapshots()

    def DeleteSnapshot(self, checksum, when_ns=None):
        """State.DeleteSnapshot (state.go:628-647) on the aggregate: `plakar
        rm`.  KeyError("snapshot not found") as the reference's error.  The
        caller stores the deletion with state.serialize_rows(deleted=...)."""
        if self.State().delete_snapshots([bytes(checksum)], when_ns=when_ns)[0]:
            raise KeyError("snapshot not found")

    def Cleanup(self, live_refs, packfile_of, **opts):
        """`plakar cleanup` (cleanup.go:35-45): live_refs are the (type,
        checksum) pairs the remaining snapshots use; they replace whatever was
        marked before.  Returns maintenance.cleanup's CleanupResult (key,
        compression, packfile_form, ... in opts are the repository's)."""
        from . import maintenance
        S = self.State()
        S.clear_marks()
        S.mark(live_refs)
        return maintenance.cleanup(S, packfile_of, **opts)


def chunkify_lengths(repo: Repository, size: int, rd):
    """snapshot/backup.go:631-666: the chunk lengths plakar records for a file of
    `size` bytes read from `rd` (empty file -> one empty chunk; smaller than
    MinSize -> the whole file as one chunk, no CDC; otherwise the chunker)."""
    if size == 0:
        return [0]
    if size < repo.Chunking.MinSize:
        return [len(rd.read())]
    lens = []
    chk = repo.Chunker(rd)
    try:
        while True:
            chunk, err = chk.Next()
            if chunk is None:
                break
            lens.append(len(chunk))
            if err is chunkers.EOF:
                break
    finally:
        chk.close()
    return lens
