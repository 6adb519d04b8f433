"""Mark and sweep over Python dicts (TEST INFRASTRUCTURE: the independent
reference for cdc_state_mark, cdc_state_delete_snapshots and cdc_state_sweep;
nothing here calls the library).  It restates the rule of DESIGN.md 5.25 on
top of state_ref.py, from the list of states in the order they were given.

Record numbers.  The library numbers the records of its store in this order
(plakar_amd/csrc/cdc_state.cpp, merge_locked, "the type sections in
SerializeStream's order, then the deleted snapshots"):

    merge call, in the order of the calls
      state, in the order given (a rejected state has no records here)
        section: Chunks, Objects, Files, Directories, Children, Datas,
                 Snapshots, Signatures, Errors (state_ref.SECTION_TYPES, which
                 is MERGE_TYPES' order too), then DeletedSnapshots
          record, by its position in the serialised section

and cdc_state_delete_snapshots appends one deletion record per checksum it
found, in the order given.  Aggregate keeps exactly that list; a record's
number is its index.  state_ref.deserialize fills its dicts in file order, so
the position of a record in its section is the dict's order.

The rule.  The winner of a key (type, checksum) is its lowest record number.
A location record is live iff it is the winner, and its key is marked or its
type is in keep_types, and, for a snapshot, no deletion record names its
checksum.  Per packfile: extent = max(offset + length) over all its records,
live_rows / live_bytes over the live ones; DROP when live_rows == 0, REPACK
when live_bytes * 1000 < extent * permille, else KEEP."""
import state_ref as sref

KEEP, DROP, REPACK = 0, 1, 2
TYPE_DELETED = 9


class Plan:
    def __init__(self):
        self.packs = []        # dicts, ascending in first_record
        self.kept_rows = []    # (type, checksum, packfile, offset, length), in record order
        self.repack_rows = []  # grouped by packfile in the list's order, ascending in offset
        self.stats = {}

    def pack(self, checksum):
        return next(p for p in self.packs if p["packfile"] == checksum)


class Aggregate:
    def __init__(self):
        self.records = []  # (type, checksum, packfile, offset, length); type 9: a deletion
        self.marks = set()  # keys (type, checksum) that were marked and present at the time

    def merge(self, states):
        """states: state_ref.State objects (serialised ascending) or serialised bytes."""
        for st in states:
            data = st if isinstance(st, (bytes, bytearray)) else st.serialize("asc")
            d = sref.deserialize(data)
            for typ in sref.SECTION_TYPES:
                for bid, (pid, off, length) in d.maps[typ].items():
                    self.records.append((typ, d.id_to_checksum[bid], d.id_to_checksum[pid], off, length))
            for sid in d.deleted:
                self.records.append((TYPE_DELETED, d.id_to_checksum[sid], sref.ZERO, 0, 0))
        return self

    def winners(self):
        win = {}
        for r, rec in enumerate(self.records):
            win.setdefault((rec[0], rec[1]), r)
        return win

    def delete_snapshots(self, checksums):
        """The statuses' truth values: True where the snapshot was found."""
        win = self.winners()
        found = [(sref.TYPE_SNAPSHOT, bytes(c)) in win for c in checksums]
        for c, f in zip(checksums, found):
            if f:
                self.records.append((TYPE_DELETED, bytes(c), sref.ZERO, 0, 0))
        return found

    def mark(self, refs):
        """(found list in the order given, missing count)."""
        win = self.winners()
        found = [(int(t), bytes(c)) in win and int(t) != TYPE_DELETED for t, c in refs]
        self.marks.update((int(t), bytes(c)) for (t, c), f in zip(refs, found) if f)
        return found, found.count(False)

    def clear_marks(self):
        self.marks.clear()

    def sweep(self, keep_types=1, permille=500):
        win = self.winners()
        packs, order = {}, []
        live = []
        seen = losers = 0
        for r, (typ, blob, pack, off, length) in enumerate(self.records):
            if typ == TYPE_DELETED:
                continue
            seen += 1
            if pack not in packs:
                packs[pack] = dict(packfile=pack, extent=0, live_rows=0, live_bytes=0, first_record=r, row_first=0, row_count=0)
                order.append(pack)
            p = packs[pack]
            p["extent"] = max(p["extent"], off + length)
            winner = win[(typ, blob)] == r
            losers += not winner
            ok = winner and ((typ, blob) in self.marks or keep_types >> typ & 1)
            if ok and typ == sref.TYPE_SNAPSHOT and (TYPE_DELETED, blob) in win:
                ok = False
            if ok:
                p["live_rows"] += 1
                p["live_bytes"] += length
                live.append(r)
        plan = Plan()
        for pack in order:
            p = packs[pack]
            if p["live_rows"] == 0:
                p["verdict"] = DROP
            elif p["live_bytes"] * 1000 < p["extent"] * permille:
                p["verdict"] = REPACK
            else:
                p["verdict"] = KEEP
            plan.packs.append(p)
        plan.kept_rows = [self.records[r] for r in live if packs[self.records[r][2]]["verdict"] == KEEP]
        live_of = {}
        for r in live:
            live_of.setdefault(self.records[r][2], []).append(self.records[r])
        for pack in order:
            p = packs[pack]
            if p["verdict"] != REPACK:
                continue
            rows = sorted(live_of[pack], key=lambda rec: rec[3])  # stable: ties keep record order
            p["row_first"], p["row_count"] = len(plan.repack_rows), len(rows)
            plan.repack_rows.extend(rows)
        gone = [p for p in plan.packs if p["verdict"] != KEEP]
        plan.stats = dict(records=seen, live=len(live), dead=seen - len(live), losers=losers, packs=len(order),
                          keep=len(order) - len(gone), drop=sum(p["verdict"] == DROP for p in gone),
                          repack=sum(p["verdict"] == REPACK for p in gone), kept_rows=len(plan.kept_rows),
                          repack_rows=len(plan.repack_rows), live_bytes=sum(p["live_bytes"] for p in plan.packs),
                          reclaimable_bytes=sum(p["extent"] - p["live_bytes"] for p in gone))
        return plan
