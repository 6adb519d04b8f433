"""Maintenance: what makes a repository smaller.

    plakar rm        State.DeleteSnapshot, repository/state/state.go:628-647
    plakar cleanup   cmd/plakar/subcommands/cleanup/cleanup.go:35-45: in the
                     reference a comment of seven steps and a `return 0`

The hot path is on the device (cdc_state_mark, cdc_state_sweep; DESIGN.md
5.25): the references of the snapshots that stay are marked against the
aggregate's table, and a sweep decides per record and per packfile what is
live.  cleanup() is the thin composition around it: the packfiles worth
rewriting go through the native sync pipeline with the repository's codec on
both sides (its COPY path, or with a key REKEY, which reseals each blob: no
blob is decompressed on either), and the rows that stay plus the
rows of the new packfiles become the new aggregate state.  Nothing here
deletes anything: the result names what the caller may delete once the new
packfiles and the new state are stored."""
import hashlib
import os
import time

from . import _lib
from .state import (PACK_DTYPE, TYPE_SNAPSHOT, VERDICTS, State, SweepPlan, rows_as_tuples, serialize_rows)


class CleanupResult:
    """new_packfiles     [(checksum, bytes)], to PutPackfile
    new_state         the new aggregate state's plaintext, to Encode and
                      PutState; None when a blob failed
    delete_packfiles  checksums of the DROP and REPACK packfiles
    delete_states     the ids of the states the new one replaces
    failures          {(type, checksum): status} of the blobs that could not
                      be carried over, and {packfile checksum: status} of a
                      packfile that could not be registered
    plan              the SweepPlan
    stats             the plan's info, plus `sync`: the pipeline's statistics

    With failures, new_state is None and both delete lists are empty: a
    cleanup that lost a blob must not be committed."""

    def __init__(self, new_packfiles, new_state, delete_packfiles, delete_states, failures, plan, stats):
        self.new_packfiles, self.new_state = new_packfiles, new_state
        self.delete_packfiles, self.delete_states = delete_packfiles, delete_states
        self.failures, self.plan, self.stats = failures, plan, stats

    @property
    def ok(self):
        return self.new_state is not None


def _index(packfile, form, key, compression, device):
    from . import restore, stored
    if form == "stored":
        return stored.packfile_index_stored(packfile, key=key, compression=compression, device=device)[1]
    return restore.packfile_index(packfile)[1]


def cleanup(state, packfile_of, key=None, compression="LZ4", packfile_form="plain", repack_permille=500,
            keep_types=(TYPE_SNAPSHOT,), verify=True, max_size=None, timestamp=None, device=0):
    """Steps 2 to 7 of cleanup.go:35-45 for an aggregate whose live rows are
    marked (State.mark / mark_device; step 1 is the caller's walk of its
    snapshots).  packfile_of(checksum) returns a packfile's bytes or path and
    is asked for the REPACK packfiles only; key, compression and packfile_form
    are the repository's.  Returns a CleanupResult."""
    from . import sync
    _lib.packfile_form_code(packfile_form)
    stamp = time.time_ns() if timestamp is None else int(timestamp)
    plan = state.sweep(keep_types=keep_types, repack_permille=repack_permille)
    slices = plan.repack_slices()
    new_packs, failures, sync_stats = [], {}, None
    if slices:
        with sync.SyncPipeline(src_key=key, src_compression=compression, dst_key=key, dst_compression=compression,
                               verify=verify, max_size=max_size, timestamp=stamp, device=device,
                               dst_packfile_form=packfile_form) as pipe:
            given = []
            for pack, _ in slices:
                p = packfile_of(pack)
                given.append(p if isinstance(p, (str, os.PathLike)) else bytes(p))
            for (pack, _), st in zip(slices, pipe.add_packfiles(given, rows=[rows for _, rows in slices])):
                if st:
                    failures[pack] = st
            _, blob_failures, sync_stats = pipe.run(on_pack=new_packs.append)
            failures.update(blob_failures)
    stats = dict(plan.info, sync=sync_stats)
    new_packfiles = [(hashlib.sha256(p).digest(), p) for p in new_packs]
    if failures:
        return CleanupResult(new_packfiles, None, [], [], failures, plan, stats)
    rows = rows_as_tuples(plan.kept_rows)
    for pack, p in new_packfiles:
        rows.extend((typ, csum, pack, off, ln) for typ, csum, off, ln in _index(p, packfile_form, key, compression, device))
    new_state = serialize_rows(rows, stamp, aggregate=True, extends=())
    return CleanupResult(new_packfiles, new_state, plan.packfiles("drop") + plan.packfiles("repack"), state.extends(),
                         failures, plan, stats)


__all__ = ["cleanup", "CleanupResult", "SweepPlan", "State", "PACK_DTYPE", "VERDICTS"]
