"""plakar_amd: MI355X-native content-defined chunker for plakar.

Drop-in for plakar's chunking path (chunking/ + the go-cdc-chunkers FastCDC
chunker it configures): HIP kernels for gfx950 behind the C ABI in
include/plakar_cdc.h (libplakar_cdc.so), with Python mirrors of the Go API:

    plakar_amd.chunking    Configuration / DefaultConfiguration
    plakar_amd.chunkers    ChunkerOpts / NewChunker / Chunker.Next / ChunkBuffers
    plakar_amd.repository  Repository.Chunker / chunkify routing
    plakar_amd.device      device-resident batches (torch tensors in HBM)
    plakar_amd.encode      Repository.Encode on the device (DeviceEncoder)
    plakar_amd.decode      Repository.Decode and the blob check on the device (DeviceDecoder)
    plakar_amd.restore     packfiles and object records back to files (RestoreSession, restore_files)
    plakar_amd.check       chunks and object checksums verified on the device (CheckSession, check_files,
                           object_digests_device)
    plakar_amd.diff        unified diffs of pairs of files (DiffSession, diff_files; line_table_device,
                           line_ids_device, diff_script, diff_emit_device)
    plakar_amd.grep        fixed strings in snapshot files, per matching line (GrepSession, grep_files; grep_device)
    plakar_amd.sync        blobs of one repository as blobs of another, on the device: re-key and
                           re-encode (transcode_device), synchronize()'s loop over packfiles (SyncSession)
    plakar_amd.stored      the form a repository keeps its packfiles in (snapshot.PutPackfile): many
                           packfiles registered in one call (add_packfiles on every session), packfile_index_stored
    plakar_amd.archive     a snapshot's entries as one tar or tar.gz stream (ArchiveSession, archive_files);
                           a gzip member written piece by piece on the device (GzipStream)
    plakar_amd.state       the repository's blob index on the device (State: merge, lookup, rows, mark, sweep)
    plakar_amd.maintenance rm and cleanup: the live set marked and swept on the device, the packfiles worth it
                           rewritten through the sync pipeline (cleanup, SweepPlan, CleanupResult)
"""
from . import chunking  # noqa: F401

__all__ = ["chunking", "chunkers", "repository", "device", "encode", "decode", "restore", "check", "diff", "grep", "sync", "stored", "archive", "state",
           "maintenance", "build"]
