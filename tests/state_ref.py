"""The repository state over Python dicts (TEST INFRASTRUCTURE: the independent
reference for libplakar_cdc.so's cdc_state_* entry points; nothing here calls
the library).  Restated from repository/state/state.go:

  State.serialize            SerializeStream, :132-233 (with a choice of record order:
                             Go ranges over maps, so a real file has any order)
  deserialize                DeserializeStream, :235-378
  State.merge                Merge / mergeLocationMaps, :384-455
  State.set_packfile_for_blob, blob_exists, get_subpart_for_blob   :572-626, :512-562, :457-510
  State.list_blobs, list_snapshots                                 :649-719

Python dicts keep insertion order, so merging deltas in a given order makes the
first-given state win among duplicates; the reference's own order is Go's map
order, that is, arbitrary.
"""
import random
import struct

VERSION = 100
TYPE_SNAPSHOT, TYPE_CHUNK, TYPE_OBJECT, TYPE_FILE, TYPE_DIRECTORY, TYPE_CHILD, TYPE_DATA, TYPE_SIGNATURE, TYPE_ERROR = \
    range(9)
TYPES = tuple(range(9))
# the order SerializeStream writes the location maps in (:194-207)
SECTION_TYPES = (TYPE_CHUNK, TYPE_OBJECT, TYPE_FILE, TYPE_DIRECTORY, TYPE_CHILD, TYPE_DATA, TYPE_SNAPSHOT,
                 TYPE_SIGNATURE, TYPE_ERROR)
# the order Merge walks them in (:438-446)
MERGE_TYPES = (TYPE_CHUNK, TYPE_OBJECT, TYPE_FILE, TYPE_DIRECTORY, TYPE_CHILD, TYPE_DATA, TYPE_SNAPSHOT,
               TYPE_SIGNATURE, TYPE_ERROR)
ZERO = bytes(32)


def _ordered(items, order, rng):
    items = sorted(items)
    if order == "desc":
        items.reverse()
    elif order == "shuffle":
        rng.shuffle(items)
    elif order != "asc":
        raise ValueError(order)
    return items


class State:
    def __init__(self):
        self.checksum_to_id = {}
        self.id_to_checksum = {}
        self.maps = {t: {} for t in TYPES}   # type -> {blob id: (packfile id, offset, length)}
        self.deleted = {}                    # snapshot id -> time (ns)
        self.version = VERSION
        self.timestamp = 0
        self.aggregate = False
        self.extends = []

    def _map(self, typ):
        if typ not in self.maps:
            raise ValueError("invalid blob type")  # the reference panics
        return self.maps[typ]

    def get_or_create_id(self, checksum):
        checksum = bytes(checksum)
        if checksum in self.checksum_to_id:
            return self.checksum_to_id[checksum]
        new = len(self.id_to_checksum)
        self.checksum_to_id[checksum] = new
        self.id_to_checksum[new] = checksum
        return new

    def set_packfile_for_blob(self, typ, packfile, blob, offset, length):
        pid = self.get_or_create_id(packfile)
        bid = self.get_or_create_id(blob)
        m = self._map(typ)
        if bid not in m:
            m[bid] = (pid, offset, length)

    def delete_snapshot(self, checksum, when=1):
        """DeleteSnapshot (:628-647) as a delta records it: the id and the time."""
        self.deleted[self.get_or_create_id(checksum)] = when

    def blob_exists(self, typ, blob):
        return self.get_or_create_id(blob) in self._map(typ)

    def get_subpart_for_blob(self, typ, blob):
        loc = self._map(typ).get(self.get_or_create_id(blob))
        if loc is None:
            return ZERO, 0, 0, False
        return self.id_to_checksum.get(loc[0], ZERO), loc[1], loc[2], True

    def list_blobs(self, typ):
        return [self.id_to_checksum.get(k, ZERO) for k in self._map(typ)]

    def list_snapshots(self):
        return [self.id_to_checksum.get(k, ZERO) for k in self.maps[TYPE_SNAPSHOT] if k not in self.deleted]

    def rows(self, typ):
        """The type's entries as a set of (type, blob, packfile, offset, length)."""
        return {(typ, self.id_to_checksum.get(b, ZERO), self.id_to_checksum.get(p, ZERO), o, n)
                for b, (p, o, n) in self._map(typ).items()}

    def merge(self, state_id, delta):
        for typ in MERGE_TYPES:
            for bid, (pid, off, length) in delta.maps[typ].items():
                self.set_packfile_for_blob(typ, delta.id_to_checksum.get(pid, ZERO), delta.id_to_checksum.get(bid, ZERO),
                                           off, length)
        for sid, when in delta.deleted.items():
            self.deleted[self.get_or_create_id(delta.id_to_checksum.get(sid, ZERO))] = when

    def serialize(self, order="asc", seed=0):
        """SerializeStream; every section's records ascending, descending or shuffled by id."""
        rng = random.Random(seed)
        out = [struct.pack("<IqBQ", self.version, self.timestamp, 1 if self.aggregate else 0, len(self.extends))]
        out.extend(bytes(e) for e in self.extends)
        out.append(struct.pack("<Q", len(self.deleted)))
        out.extend(struct.pack("<Qq", k, v) for k, v in _ordered(self.deleted.items(), order, rng))
        out.append(struct.pack("<Q", len(self.id_to_checksum)))
        out.extend(struct.pack("<Q32s", k, v) for k, v in _ordered(self.id_to_checksum.items(), order, rng))
        for typ in SECTION_TYPES:
            m = self.maps[typ]
            out.append(struct.pack("<Q", len(m)))
            out.extend(struct.pack("<QQII", k, p, o, n) for k, (p, o, n) in _ordered(m.items(), order, rng))
        return b"".join(out)

    def size(self):
        """109 + 32 * extends + 16 * deleted + 40 * ids + 24 * rows."""
        return (109 + 32 * len(self.extends) + 16 * len(self.deleted) + 40 * len(self.id_to_checksum) +
                24 * sum(len(m) for m in self.maps.values()))


def deserialize(data):
    """DeserializeStream; ValueError where io.ReadFull would fail.  Bytes after the last section are ignored."""
    data = bytes(data)
    pos = [0]

    def take(fmt):
        n = struct.calcsize(fmt)
        if pos[0] + n > len(data):
            raise ValueError("unexpected EOF")
        v = struct.unpack_from(fmt, data, pos[0])
        pos[0] += n
        return v

    def count(rec):
        (n,) = take("<Q")
        if n > (len(data) - pos[0]) // rec:  # the reference would loop until ReadFull fails
            raise ValueError("unexpected EOF")
        return n

    st = State()
    st.version, st.timestamp, agg = take("<IqB")
    st.aggregate = agg == 1
    st.extends = [take("<32s")[0] for _ in range(count(32))]
    for _ in range(count(16)):
        k, v = take("<Qq")
        st.deleted[k] = v
    for _ in range(count(40)):
        k, v = take("<Q32s")
        st.id_to_checksum[k] = v
        st.checksum_to_id[v] = k
    for typ in SECTION_TYPES:
        for _ in range(count(24)):
            k, p, o, n = take("<QQII")
            st.maps[typ][k] = (p, o, n)
    return st


def from_rows(rows, timestamp=0, extends=(), aggregate=False):
    """A state that SetPackfileForBlob entered `rows` into, in order: (type, blob, packfile, offset, length)."""
    st = State()
    st.timestamp, st.extends, st.aggregate = timestamp, [bytes(e) for e in extends], aggregate
    for typ, blob, pack, off, length in rows:
        st.set_packfile_for_blob(typ, pack, blob, off, length)
    return st


def aggregate_of(deltas):
    """RebuildState's loop (repository.go:118-160) over (id, State) pairs in the given order."""
    agg = State()
    agg.aggregate = True
    for state_id, delta in deltas:
        agg.merge(state_id, delta)
        agg.extends.append(bytes(state_id))
    return agg
