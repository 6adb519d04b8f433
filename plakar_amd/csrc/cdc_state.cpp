// cdc_state_*: a repository's aggregate state in device memory (RebuildState,
// repository/repository.go:58-164; state.Merge, BlobExists, GetSubpartForBlob,
// ListBlobs, ListSnapshots, repository/state/state.go:384-719).  The kernels
// are cdc_state.hip, the layout arithmetic and the writer state_plan.h;
// DESIGN.md 5.24 has the design.  What lives here is the merge call's staging:
//
//   1. every stored source into one device buffer, one cdc_decode_device over
//      all of them (its sizing pass and the decode in one call when the output
//      guess holds, else one more call with the size it reported); the plain
//      sources uploaded beside the plaintexts;
//   2. k_state_plan over all plaintexts, the layouts downloaded (a few hundred
//      bytes per state), and from them the runs of records (cst::Seg) and each
//      record's number in the record store;
//   3. k_state_index, k_state_resolve; the states a kernel marked bad have
//      their records voided;
//   4. k_state_insert of the new records, or of every record into a larger
//      table when they pass half its slots; k_state_count for the statistics.
//
// The record store and the table are the only device memory kept between
// calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "cdc_state.h"
#include "sweep_plan.h"

using cdc::align_up;

struct cdc_state {
    std::mutex mu;
    int device = 0;
    int compress = CDC_COMPRESS_NONE;
    std::vector<uint8_t> key;  // 32 bytes, or empty
    hipStream_t stream = nullptr;
    cdc::DevBuf recs;          // cdc_state_row[rec_cap], the first nrecs in use
    uint64_t nrecs = 0, rec_cap = 0;
    cdc::DevBuf slots;         // uint64_t[capacity]
    uint64_t capacity = 0;
    cdc::DevBuf words;         // kTypes + 1 counters, the rows counter [16], mark's misses [17], a sweep's counters [20..]
    cdc::DevBuf qbuf;          // the host lookups', cdc_state_rows' and cdc_state_mark's staging
    cdc::DevBuf marks;         // uint32_t[mark_words]: bit r is record r's mark (cdc_state_mark)
    uint64_t mark_words = 0;
    std::vector<uint8_t> extends;
    cdc_state_stats stats{};

    ~cdc_state()
    {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (!key.empty()) std::memset(key.data(), 0, key.size());
    }
    const uint8_t *key_ptr() const { return key.empty() ? nullptr : key.data(); }
    cst::Table table() const { return cst::Table{slots.as<uint64_t>(), capacity - 1, recs.as<cdc_state_row>()}; }
    uint64_t *counters() const { return words.as<uint64_t>(); }
    uint64_t *row_counter() const { return words.as<uint64_t>() + 16; }
    uint64_t *miss_counter() const { return words.as<uint64_t>() + 17; }
    cst::SweepCounts *sweep_counters() const { return reinterpret_cast<cst::SweepCounts *>(words.as<uint64_t>() + 20); }
};
static_assert(20 * 8 + sizeof(cst::SweepCounts) <= 256, "the counters' allocation");

struct cdc_sweep {
    std::vector<cdc_sweep_pack> packs;
    std::vector<cdc_state_row> kept, repack;
    cdc_sweep_stats stats{};
};

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool sync(cdc_state *s) { return hipStreamSynchronize(s->stream) == hipSuccess; }

bool copy(cdc_state *s, void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    return n == 0 || hipMemcpyAsync(dst, src, n, kind, s->stream) == hipSuccess;
}

// The stream, the counters and the smallest table, at the first call that needs the device.
int ensure_device(cdc_state *s)
{
    if (hipSetDevice(s->device) != hipSuccess) return CDC_E_DEVICE;
    if (!s->stream && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        s->stream = nullptr;
        return CDC_E_DEVICE;
    }
    if (!s->words.reserve(256)) return CDC_E_NOMEM;
    if (!s->capacity) {
        if (!s->slots.reserve(size_t(cst::kMinSlots) * 8)) return CDC_E_NOMEM;
        if (hipMemsetAsync(s->slots.data(), 0xFF, size_t(cst::kMinSlots) * 8, s->stream) != hipSuccess || !sync(s))
            return CDC_E_DEVICE;
        s->capacity = cst::kMinSlots;
    }
    if (!s->recs.reserve(sizeof(cdc_state_row))) return CDC_E_NOMEM;
    return CDC_OK;
}

// Room for `need` records, the ones in use kept.
int reserve_recs(cdc_state *s, uint64_t need)
{
    if (need <= s->rec_cap) return CDC_OK;
    const uint64_t want = std::max<uint64_t>(need, s->rec_cap + s->rec_cap / 2);
    cdc::DevBuf bigger;
    if (!bigger.reserve(size_t(want) * sizeof(cdc_state_row))) return CDC_E_NOMEM;
    if (!copy(s, bigger.data(), s->recs.data(), size_t(s->nrecs) * sizeof(cdc_state_row), hipMemcpyDeviceToDevice) || !sync(s))
        return CDC_E_DEVICE;
    s->recs = std::move(bigger);
    s->rec_cap = want;
    return CDC_OK;
}

// Room for records [nrecs, after): the store, and, when they pass half the
// table's slots, a larger table in `bigger` (new_cap slots, not yet in use).
// Nothing of the aggregate changes but the store's allocation.
int room_for(cdc_state *s, uint64_t after, cdc::DevBuf &bigger, uint64_t &new_cap)
{
    const int rc = reserve_recs(s, after);
    if (rc != CDC_OK) return rc;
    new_cap = s->capacity;
    if (after > s->capacity / 2) {
        while (new_cap / 2 < after) new_cap *= 2;
        if (!bigger.reserve(size_t(new_cap) * 8)) return CDC_E_NOMEM;
    }
    return CDC_OK;
}

// Records [nrecs, after) lie in the store: enter them, or every record into
// the larger table room_for prepared, and count the winners for the statistics.
int enter_records(cdc_state *s, uint64_t after, cdc::DevBuf &bigger, uint64_t new_cap)
{
    const bool rebuild = new_cap != s->capacity;
    if (rebuild) {
        if (hipMemsetAsync(bigger.data(), 0xFF, size_t(new_cap) * 8, s->stream) != hipSuccess) return CDC_E_DEVICE;
        s->slots = std::move(bigger);
        s->capacity = new_cap;
    }
    int rc = cst::launch_insert(s->device, s->table(), rebuild ? 0 : s->nrecs, after, s->stream);
    if (rc != CDC_OK) return rc;
    s->nrecs = after;
    uint64_t counts[splan::kTypes + 1];
    rc = cst::launch_count(s->device, s->table(), s->counters(), s->stream);
    if (rc != CDC_OK) return rc;
    if (!copy(s, counts, s->counters(), sizeof(counts), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    for (uint32_t t = 0; t < splan::kTypes; ++t) s->stats.rows[t] = counts[t];
    s->stats.deleted_snapshots = counts[splan::kTypes];
    return CDC_OK;
}

int merge_locked(cdc_state *s, const cdc_state_src *srcs, uint32_t n, int32_t *status)
{
    int rc = ensure_device(s);
    if (rc != CDC_OK) return rc;
    const double t0 = now_s();

    // 1. the plaintexts: [plain sources | Decode's output]
    std::vector<uint32_t> stored, plain;
    uint64_t in_bytes = 0, plain_bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        status[i] = CDC_OK;
        if (srcs[i].form == CDC_STATE_STORED) {
            stored.push_back(i);
            in_bytes += srcs[i].len;
        } else if (srcs[i].len >> 32) {
            status[i] = CDC_E_UNSUPPORTED;
        } else {
            plain.push_back(i);
            plain_bytes += align_up(size_t(srcs[i].len), 16);
        }
    }
    const uint64_t out_base = align_up(size_t(plain_bytes), 256);
    const uint32_t m = uint32_t(stored.size());
    std::vector<uint64_t> off(m), len(m), oo(size_t(m) + 1, 0);
    std::vector<int32_t> dst(m, CDC_OK);
    cdc::DevBuf d_in, d_plain;
    if (m) {
        if (!d_in.reserve(size_t(in_bytes))) return CDC_E_NOMEM;
        uint64_t at = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const cdc_state_src &S = srcs[stored[j]];
            off[j] = at, len[j] = S.len;
            if (!copy(s, d_in.as<uint8_t>() + at, S.bytes, size_t(S.len), hipMemcpyHostToDevice)) return CDC_E_DEVICE;
            at += S.len;
        }
        if (!sync(s)) return CDC_E_DEVICE;
        // a state is mostly checksums, which do not compress: twice the encoded size holds all but odd ones
        uint64_t cap = align_up(size_t(in_bytes) * 2, 256) + 4096;
        for (int attempt = 0;; ++attempt) {
            if (!d_plain.reserve(size_t(out_base + cap))) return CDC_E_NOMEM;
            rc = cdc_decode_device(s->device, d_in.data(), off.data(), len.data(), m, s->compress, s->key_ptr(),
                                   d_plain.as<uint8_t>() + out_base, cap, oo.data(), dst.data(), s->stream);
            if (rc == CDC_E_NOSPACE && attempt == 0) {
                cap = align_up(size_t(oo[m]), 256) + 256;
                continue;
            }
            if (rc != CDC_OK) return rc == CDC_E_NOSPACE ? CDC_E_DEVICE : rc;
            break;
        }
        d_in.release();
    } else if (!d_plain.reserve(size_t(out_base) + 16)) {
        return CDC_E_NOMEM;
    }
    std::vector<cst::StateDesc> desc;
    std::vector<uint32_t> who;  // desc[k] is source who[k]; ascending
    {
        // the two kinds interleave in source order again
        std::vector<cst::StateDesc> tmp(n);
        std::vector<uint8_t> have(n, 0);
        uint64_t at = 0;
        for (uint32_t i : plain) {
            if (!copy(s, d_plain.as<uint8_t>() + at, srcs[i].bytes, size_t(srcs[i].len), hipMemcpyHostToDevice))
                return CDC_E_DEVICE;
            tmp[i].plain = at, tmp[i].len = srcs[i].len, have[i] = 1;
            at += align_up(size_t(srcs[i].len), 16);
        }
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = stored[j];
            status[i] = dst[j];
            if (status[i] != CDC_OK) continue;
            if ((oo[j + 1] - oo[j]) >> 32) {
                status[i] = CDC_E_UNSUPPORTED;
                continue;
            }
            tmp[i].plain = out_base + oo[j], tmp[i].len = oo[j + 1] - oo[j], have[i] = 1;
        }
        for (uint32_t i = 0; i < n; ++i)
            if (have[i]) {
                cst::StateDesc D{};
                D.plain = tmp[i].plain, D.len = tmp[i].len;
                desc.push_back(D);
                who.push_back(i);
            }
    }
    const double t1 = now_s();
    s->stats.decode_s += t1 - t0;

    // 2. the layouts
    const uint32_t k = uint32_t(desc.size());
    cdc::DevBuf d_desc, d_segs, d_idtab;
    const uint8_t *const dp = d_plain.as<uint8_t>();
    std::vector<cst::Seg> idsegs, locsegs;
    std::vector<uint64_t> first_rec(k, 0), nrec(k, 0);
    uint64_t ids = 0, news = 0;
    if (k) {
        if (!d_desc.reserve(size_t(k) * sizeof(cst::StateDesc))) return CDC_E_NOMEM;
        cst::StateDesc *const dd = d_desc.as<cst::StateDesc>();
        if (!copy(s, dd, desc.data(), size_t(k) * sizeof(cst::StateDesc), hipMemcpyHostToDevice)) return CDC_E_DEVICE;
        rc = cst::launch_plan(s->device, dd, k, dp, s->stream);
        if (rc != CDC_OK) return rc;
        if (!copy(s, desc.data(), dd, size_t(k) * sizeof(cst::StateDesc), hipMemcpyDeviceToHost) || !sync(s))
            return CDC_E_DEVICE;
        for (uint32_t q = 0; q < k; ++q) {
            cst::StateDesc &D = desc[q];
            status[who[q]] = D.status == CDC_OK ? CDC_OK : CDC_E_CORRUPT;
            first_rec[q] = s->nrecs + news;
            if (D.status != CDC_OK) continue;
            D.id_base = ids;
            const splan::Section &I = D.L.sec[splan::kSecIds];
            if (I.count) idsegs.push_back(cst::Seg{ids, I.count, D.plain + I.off, 0, q, 0});
            ids += I.count;
            // the type sections in SerializeStream's order, then the deleted snapshots
            for (uint32_t sec = splan::kSecFirstType; sec <= splan::kSections; ++sec) {
                const bool del = sec == splan::kSections;
                const splan::Section &C = D.L.sec[del ? splan::kSecDeleted : sec];
                if (!C.count) continue;
                locsegs.push_back(cst::Seg{news, C.count, D.plain + C.off, s->nrecs + news, q,
                                           del ? cst::kTypeDeleted : splan::type_of_section(sec)});
                news += C.count;
            }
            nrec[q] = s->nrecs + news - first_rec[q];
        }
    }

    // 3. ids, then records
    const uint64_t after = s->nrecs + news;
    cdc::DevBuf bigger;
    uint64_t new_cap = s->capacity;
    if (news) {
        rc = room_for(s, after, bigger, new_cap);
        if (rc != CDC_OK) return rc;
    }
    if (ids || news) {  // a state without a location can still be malformed in its ids
        const size_t nseg = idsegs.size() + locsegs.size();
        if (!d_segs.reserve(nseg * sizeof(cst::Seg)) || !d_idtab.reserve(size_t(ids) * 4)) return CDC_E_NOMEM;
        cst::StateDesc *const dd = d_desc.as<cst::StateDesc>();
        cst::Seg *const ds = d_segs.as<cst::Seg>();
        if (!copy(s, dd, desc.data(), size_t(k) * sizeof(cst::StateDesc), hipMemcpyHostToDevice) ||
            !copy(s, ds, idsegs.data(), idsegs.size() * sizeof(cst::Seg), hipMemcpyHostToDevice) ||
            !copy(s, ds + idsegs.size(), locsegs.data(), locsegs.size() * sizeof(cst::Seg), hipMemcpyHostToDevice))
            return CDC_E_DEVICE;
        if (ids && hipMemsetAsync(d_idtab.data(), 0xFF, size_t(ids) * 4, s->stream) != hipSuccess) return CDC_E_DEVICE;
        rc = cst::launch_index(s->device, dd, ds, uint32_t(idsegs.size()), ids, dp, d_idtab.as<uint32_t>(), s->stream);
        if (rc == CDC_OK)
            rc = cst::launch_resolve(s->device, dd, ds + idsegs.size(), uint32_t(locsegs.size()), news, dp,
                                     d_idtab.as<uint32_t>(), s->recs.as<cdc_state_row>(), s->stream);
        if (rc != CDC_OK) return rc;
        if (!copy(s, desc.data(), dd, size_t(k) * sizeof(cst::StateDesc), hipMemcpyDeviceToHost) || !sync(s))
            return CDC_E_DEVICE;
        for (uint32_t q = 0; q < k; ++q) {
            if (desc[q].status != CDC_OK || !desc[q].bad) continue;
            status[who[q]] = CDC_E_CORRUPT;  // nothing of it is entered: its records are voided (found = 0)
            if (nrec[q] && hipMemsetAsync(s->recs.as<cdc_state_row>() + first_rec[q], 0, size_t(nrec[q]) * sizeof(cdc_state_row),
                                          s->stream) != hipSuccess)
                return CDC_E_DEVICE;
        }
    }
    const double t2 = now_s();
    s->stats.index_s += t2 - t1;

    // 4. the table
    if (news) {
        rc = enter_records(s, after, bigger, new_cap);
        if (rc != CDC_OK) return rc;
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (status[i] == CDC_OK) {
            s->extends.insert(s->extends.end(), srcs[i].id, srcs[i].id + 32);
            ++s->stats.states;
        } else {
            ++s->stats.rejected;
        }
    }
    s->stats.insert_s += now_s() - t2;
    return CDC_OK;
}

// CDC_E_NOSPACE bookkeeping of cdc_state_rows and cdc_state_extends.
int report(uint64_t have, uint64_t cap, uint64_t *needed)
{
    if (needed) *needed = have;
    return have > cap ? CDC_E_NOSPACE : CDC_OK;
}

// cdc_state_lookup under the lock, the device up.
int lookup_locked(cdc_state *s, uint8_t type, const uint8_t *checksums, uint64_t n, cdc_state_row *out)
{
    const size_t qb = align_up(size_t(n) * 32, 256);
    if (!s->qbuf.reserve(qb + size_t(n) * sizeof(cdc_state_row))) return CDC_E_NOMEM;
    uint8_t *const dq = s->qbuf.as<uint8_t>();
    cdc_state_row *const dr = reinterpret_cast<cdc_state_row *>(dq + qb);
    if (!copy(s, dq, checksums, size_t(n) * 32, hipMemcpyHostToDevice)) return CDC_E_DEVICE;
    const int rc = cst::launch_lookup(s->device, s->table(), type, dq, n, dr, s->stream);
    if (rc != CDC_OK) return rc;
    if (!copy(s, out, dr, size_t(n) * sizeof(cdc_state_row), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    return CDC_OK;
}

// The mark bitmap covers every record the store has room for.  Grown, it
// keeps its bits and the new words are zero: record numbers never change.
int ensure_marks(cdc_state *s)
{
    const uint64_t need = align_up(size_t((std::max<uint64_t>(s->rec_cap, s->nrecs) + 31) / 32 + 1), 64);
    if (need <= s->mark_words) return CDC_OK;
    cdc::DevBuf bigger;
    if (!bigger.reserve(size_t(need) * 4)) return CDC_E_NOMEM;
    if (hipMemsetAsync(bigger.data(), 0, size_t(need) * 4, s->stream) != hipSuccess ||
        !copy(s, bigger.data(), s->marks.data(), size_t(s->mark_words) * 4, hipMemcpyDeviceToDevice) || !sync(s))
        return CDC_E_DEVICE;
    s->marks = std::move(bigger);
    s->mark_words = need;
    return CDC_OK;
}

// Records the host made (deletions), appended to the store and entered: step
// 4 of a merge for rows that need no resolving.
int append_records(cdc_state *s, const std::vector<cdc_state_row> &rows)
{
    const uint64_t after = s->nrecs + rows.size();
    cdc::DevBuf bigger;
    uint64_t new_cap = s->capacity;
    const int rc = room_for(s, after, bigger, new_cap);
    if (rc != CDC_OK) return rc;
    if (!copy(s, s->recs.as<cdc_state_row>() + s->nrecs, rows.data(), rows.size() * sizeof(cdc_state_row), hipMemcpyHostToDevice))
        return CDC_E_DEVICE;
    return enter_records(s, after, bigger, new_cap);
}

int sweep_locked(cdc_state *s, const cdc_sweep_opts &o, cdc_sweep *plan)
{
    cdc_sweep_stats &st = plan->stats;
    const uint64_t n = s->nrecs;
    if (!n) return CDC_OK;
    int rc = ensure_device(s);
    if (rc == CDC_OK) rc = ensure_marks(s);
    if (rc != CDC_OK) return rc;

    // a packfile holds at least one row: at most n keys, so the table is at most half full
    uint64_t pcap = cst::kMinSlots;
    while (pcap / 2 < n) pcap *= 2;
    const uint64_t ntiles = (n + cst::kSweepTile - 1) / cst::kSweepTile;
    cdc::Carver carve(256);
    const size_t o_slots = carve.take(size_t(pcap) * 8), o_extent = carve.take(size_t(pcap) * 8),
                 o_bytes = carve.take(size_t(pcap) * 8), o_rows = carve.take(size_t(pcap) * 8),
                 o_verdict = carve.take(size_t(pcap) * 4), o_live = carve.take(size_t((n + 63) / 64) * 8),
                 o_slot = carve.take(size_t(n) * 8), o_class = carve.take(size_t(n)),
                 o_tiles = carve.take(size_t(ntiles + 1) * 16);
    cdc::DevBuf work;
    if (!work.reserve(carve.bytes())) return CDC_E_NOMEM;
    uint8_t *const w = work.as<uint8_t>();
    cst::Packs K{cst::Table{reinterpret_cast<uint64_t *>(w + o_slots), pcap - 1, s->recs.as<cdc_state_row>()},
                 reinterpret_cast<uint64_t *>(w + o_extent), reinterpret_cast<uint64_t *>(w + o_bytes),
                 reinterpret_cast<uint64_t *>(w + o_rows), reinterpret_cast<int32_t *>(w + o_verdict)};
    cst::SweepCounts *const dc = s->sweep_counters();
    cst::SweepCounts c{};
    if (hipMemsetAsync(w + o_slots, 0xFF, size_t(pcap) * 8, s->stream) != hipSuccess ||
        hipMemsetAsync(w + o_extent, 0, o_live - o_extent, s->stream) != hipSuccess ||
        hipMemsetAsync(dc, 0, sizeof(c), s->stream) != hipSuccess || !sync(s))
        return CDC_E_DEVICE;

    const double t0 = now_s();
    rc = cst::launch_packs(s->device, K.P, n, dc, s->stream);
    if (rc != CDC_OK) return rc;
    if (!copy(s, &c, dc, sizeof(c), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    const double t1 = now_s();
    rc = cst::launch_sweep(s->device, s->table(), K, n, s->marks.as<uint32_t>(), o.keep_types,
                           reinterpret_cast<uint64_t *>(w + o_live), reinterpret_cast<uint64_t *>(w + o_slot), dc, s->stream);
    if (rc != CDC_OK) return rc;
    if (!sync(s)) return CDC_E_DEVICE;
    const double t2 = now_s();
    const uint64_t npacks = c.packs;
    cdc::DevBuf d_list;
    if (!d_list.reserve(size_t(npacks) * sizeof(cdc_sweep_pack))) return CDC_E_NOMEM;
    rc = cst::launch_verdict(s->device, K, o.repack_permille, d_list.as<cdc_sweep_pack>(), npacks, dc, s->stream);
    if (rc != CDC_OK) return rc;
    if (!sync(s)) return CDC_E_DEVICE;
    const double t3 = now_s();
    rc = cst::launch_classes(s->device, K, n, reinterpret_cast<uint64_t *>(w + o_live), reinterpret_cast<uint64_t *>(w + o_slot),
                             w + o_class, reinterpret_cast<uint64_t *>(w + o_tiles), dc, s->stream);
    if (rc != CDC_OK) return rc;
    if (!copy(s, &c, dc, sizeof(c), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    if (c.listed != npacks || c.kept + c.repack > c.live || c.live > n) return CDC_E_DEVICE;  // the stages disagree
    cdc::DevBuf d_rows;
    if (!d_rows.reserve(size_t(c.kept + c.repack) * sizeof(cdc_state_row))) return CDC_E_NOMEM;
    cdc_state_row *const dk = d_rows.as<cdc_state_row>(), *const dr = dk + c.kept;
    rc = cst::launch_compact(s->device, s->recs.as<cdc_state_row>(), n, w + o_class, reinterpret_cast<uint64_t *>(w + o_tiles),
                             dk, c.kept, dr, c.repack, s->stream);
    if (rc != CDC_OK) return rc;
    if (!sync(s)) return CDC_E_DEVICE;
    const double t4 = now_s();

    plan->packs.resize(size_t(npacks));
    plan->kept.resize(size_t(c.kept));
    plan->repack.resize(size_t(c.repack));
    if (!copy(s, plan->packs.data(), d_list.data(), size_t(npacks) * sizeof(cdc_sweep_pack), hipMemcpyDeviceToHost) ||
        !copy(s, plan->kept.data(), dk, size_t(c.kept) * sizeof(cdc_state_row), hipMemcpyDeviceToHost) ||
        !copy(s, plan->repack.data(), dr, size_t(c.repack) * sizeof(cdc_state_row), hipMemcpyDeviceToHost) || !sync(s))
        return CDC_E_DEVICE;
    std::sort(plan->packs.begin(), plan->packs.end(),
              [](const cdc_sweep_pack &a, const cdc_sweep_pack &b) { return a.first_record < b.first_record; });
    rc = swplan::group_repack(plan->repack.data(), c.repack, plan->packs.data(), npacks);
    if (rc != CDC_OK) return CDC_E_DEVICE;

    st.records = c.seen, st.live = c.live, st.dead = c.seen - c.live, st.losers = c.losers;
    st.packs = npacks, st.kept_rows = c.kept, st.repack_rows = c.repack;
    for (const cdc_sweep_pack &P : plan->packs) {
        st.live_bytes += P.live_bytes;
        if (P.verdict == CDC_SWEEP_KEEP) {
            ++st.keep;
            continue;
        }
        ++(P.verdict == CDC_SWEEP_DROP ? st.drop : st.repack);
        st.reclaimable_bytes += P.extent > P.live_bytes ? P.extent - P.live_bytes : 0;
    }
    st.packs_s = t1 - t0, st.sweep_s = t2 - t1, st.verdict_s = t3 - t2, st.compact_s = t4 - t3, st.download_s = now_s() - t4;
    return CDC_OK;
}

template <class T>
int hand_out(const std::vector<T> &have, T *out, uint64_t cap, uint64_t *needed)
{
    const uint64_t k = std::min<uint64_t>(have.size(), cap);
    if (k) std::memcpy(out, have.data(), size_t(k) * sizeof(T));
    return report(have.size(), cap, needed);
}

}  // namespace

extern "C" {

int cdc_state_new(int device, int compress, const uint8_t *key, cdc_state **out)
{
    if (!out || device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    *out = nullptr;
    try {
        cdc_state *s = new cdc_state();
        s->device = device;
        s->compress = compress;
        if (key) s->key.assign(key, key + 32);
        *out = s;
        return CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_state_free(cdc_state *s)
{
    if (!s) return;
    if (s->stream) (void)hipSetDevice(s->device);
    delete s;
}

int cdc_state_merge(cdc_state *s, const cdc_state_src *srcs, uint32_t n, int32_t *status)
{
    if (!s || (n && (!srcs || !status))) return CDC_E_INVALID;
    for (uint32_t i = 0; i < n; ++i)
        if ((srcs[i].form != CDC_STATE_PLAIN && srcs[i].form != CDC_STATE_STORED) || (!srcs[i].bytes && srcs[i].len))
            return CDC_E_INVALID;
    if (!n) return CDC_OK;
    try {
        std::lock_guard<std::mutex> lk(s->mu);
        return merge_locked(s, srcs, n, status);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_state_lookup_device(cdc_state *s, uint8_t type, const uint8_t *d_checksums, uint64_t n, cdc_state_row *d_out,
                            void *stream)
{
    if (!s || type >= splan::kTypes || (n && (!d_checksums || !d_out)) || (reinterpret_cast<uintptr_t>(d_out) & 15))
        return CDC_E_INVALID;
    if (!n) return CDC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    const int rc = ensure_device(s);
    if (rc != CDC_OK) return rc;
    return cst::launch_lookup(s->device, s->table(), type, d_checksums, n, d_out, stream);
}

int cdc_state_lookup(cdc_state *s, uint8_t type, const uint8_t *checksums, uint64_t n, cdc_state_row *out)
{
    if (!s || type >= splan::kTypes || (n && (!checksums || !out))) return CDC_E_INVALID;
    if (!n) return CDC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    const int rc = ensure_device(s);
    return rc != CDC_OK ? rc : lookup_locked(s, type, checksums, n, out);
}

int cdc_state_rows(cdc_state *s, uint8_t type, cdc_state_row *rows, uint64_t cap, uint64_t *needed)
{
    if (!s || type >= splan::kTypes || (cap && !rows)) return CDC_E_INVALID;
    if (needed) *needed = 0;
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t most = s->stats.rows[type];  // of type 0, the deleted ones come off
    if (!most) return CDC_OK;
    int rc = ensure_device(s);
    if (rc != CDC_OK) return rc;
    const uint64_t room = std::min(cap, most);
    if (!s->qbuf.reserve(size_t(room) * sizeof(cdc_state_row))) return CDC_E_NOMEM;
    rc = cst::launch_rows(s->device, s->table(), type, s->qbuf.as<cdc_state_row>(), room, s->row_counter(), s->stream);
    if (rc != CDC_OK) return rc;
    uint64_t have = 0;
    if (!copy(s, &have, s->row_counter(), 8, hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    if (!copy(s, rows, s->qbuf.data(), size_t(std::min(have, room)) * sizeof(cdc_state_row), hipMemcpyDeviceToHost) || !sync(s))
        return CDC_E_DEVICE;
    return report(have, cap, needed);
}

int cdc_state_extends(cdc_state *s, uint8_t *ids, uint64_t cap, uint64_t *needed)
{
    if (!s || (cap && !ids)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t have = s->extends.size() / 32;
    if (std::min(have, cap)) std::memcpy(ids, s->extends.data(), size_t(std::min(have, cap)) * 32);
    return report(have, cap, needed);
}

int cdc_state_info(cdc_state *s, cdc_state_stats *stats)
{
    if (!s || !stats || stats->struct_size != sizeof(cdc_state_stats)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(s->mu);
    *stats = s->stats;
    stats->struct_size = sizeof(cdc_state_stats);
    stats->capacity = s->capacity ? s->capacity : cst::kMinSlots;
    stats->records = s->nrecs;
    stats->device_bytes = s->rec_cap * sizeof(cdc_state_row) + s->capacity * 8;
    return CDC_OK;
}

int cdc_state_serialize(const cdc_state_row *rows, uint64_t n, int64_t timestamp_ns, int aggregate,
                        const uint8_t *extends, uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len)
{
    if ((n && !rows) || (nextends && !extends) || !len) return CDC_E_INVALID;
    try {
        return splan::serialize(rows, n, timestamp_ns, aggregate, extends, nextends, out, cap, len);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_state_serialize_deleted(const cdc_state_row *rows, uint64_t n, const uint8_t *deleted, const int64_t *deleted_ns,
                                uint64_t ndeleted, int64_t timestamp_ns, int aggregate, const uint8_t *extends,
                                uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len)
{
    if ((n && !rows) || (ndeleted && (!deleted || !deleted_ns)) || (nextends && !extends) || !len) return CDC_E_INVALID;
    try {
        return splan::serialize_deleted(rows, n, deleted, deleted_ns, ndeleted, timestamp_ns, aggregate, extends, nextends, out,
                                        cap, len);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_state_delete_snapshots(cdc_state *s, const uint8_t *checksums, uint64_t n, int64_t time_ns, int32_t *status)
{
    if (!s || (n && (!checksums || !status))) return CDC_E_INVALID;
    if (!n) return CDC_OK;
    try {
        std::lock_guard<std::mutex> lk(s->mu);
        for (uint64_t i = 0; i < n; ++i) status[i] = CDC_E_NOTFOUND;
        if (!s->stats.rows[0]) return CDC_OK;  // no snapshot row: nothing to ask the device
        int rc = ensure_device(s);
        if (rc != CDC_OK) return rc;
        std::vector<cdc_state_row> hits(size_t(n), cdc_state_row{}), gone;
        rc = lookup_locked(s, 0, checksums, n, hits.data());
        if (rc != CDC_OK) return rc;
        for (uint64_t i = 0; i < n; ++i) {
            if (!hits[size_t(i)].found) continue;
            status[i] = CDC_OK;
            cdc_state_row r{};  // what k_state_resolve makes of a DeletedSnapshots record, with the time in the location's place
            std::memcpy(r.checksum, checksums + 32 * i, 32);
            r.offset = uint32_t(uint64_t(time_ns)), r.length = uint32_t(uint64_t(time_ns) >> 32);
            r.type = uint8_t(cst::kTypeDeleted), r.found = 1;
            gone.push_back(r);
        }
        return gone.empty() ? CDC_OK : append_records(s, gone);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_state_mark(cdc_state *s, const uint8_t *refs, uint64_t n, uint8_t *found, uint64_t *missing)
{
    if (!s || (n && !refs)) return CDC_E_INVALID;
    for (uint64_t i = 0; i < n; ++i)
        if (refs[cst::kRefBytes * i] >= splan::kTypes) return CDC_E_INVALID;
    if (missing) *missing = 0;
    if (!n) return CDC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = ensure_device(s);
    if (rc == CDC_OK) rc = ensure_marks(s);
    if (rc != CDC_OK) return rc;
    const size_t rb = align_up(size_t(n) * cst::kRefBytes, 256);
    if (!s->qbuf.reserve(rb + size_t(n))) return CDC_E_NOMEM;
    uint8_t *const dq = s->qbuf.as<uint8_t>(), *const df = dq + rb;
    if (!copy(s, dq, refs, size_t(n) * cst::kRefBytes, hipMemcpyHostToDevice)) return CDC_E_DEVICE;
    rc = cst::launch_mark(s->device, s->table(), cst::kTypeOfRecord, dq, n, s->marks.as<uint32_t>(), df, s->stream);
    if (rc == CDC_OK) rc = cst::launch_missing(s->device, df, n, s->miss_counter(), s->stream);
    if (rc != CDC_OK) return rc;
    uint64_t miss = 0;
    if (!copy(s, &miss, s->miss_counter(), 8, hipMemcpyDeviceToHost) || (found && !copy(s, found, df, size_t(n), hipMemcpyDeviceToHost)) ||
        !sync(s))
        return CDC_E_DEVICE;
    if (missing) *missing = miss;
    return CDC_OK;
}

int cdc_state_mark_device(cdc_state *s, uint8_t type, const uint8_t *d_checksums, uint64_t n, uint8_t *d_found, void *stream)
{
    if (!s || type >= splan::kTypes || (n && !d_checksums)) return CDC_E_INVALID;
    if (!n) return CDC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = ensure_device(s);
    if (rc == CDC_OK) rc = ensure_marks(s);
    if (rc != CDC_OK) return rc;
    return cst::launch_mark(s->device, s->table(), type, d_checksums, n, s->marks.as<uint32_t>(), d_found, stream);
}

int cdc_state_clear_marks(cdc_state *s)
{
    if (!s) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->mark_words) return CDC_OK;  // nothing was ever marked
    if (hipSetDevice(s->device) != hipSuccess) return CDC_E_DEVICE;
    if (hipMemsetAsync(s->marks.data(), 0, size_t(s->mark_words) * 4, s->stream) != hipSuccess || !sync(s)) return CDC_E_DEVICE;
    return CDC_OK;
}

void cdc_sweep_default_opts(cdc_sweep_opts *opts)
{
    if (!opts) return;
    *opts = cdc_sweep_opts{};
    opts->struct_size = sizeof(cdc_sweep_opts);
    opts->keep_types = 1u << 0;
    opts->repack_permille = 500;
}

int cdc_state_sweep(cdc_state *s, const cdc_sweep_opts *opts, cdc_sweep **out)
{
    if (out) *out = nullptr;
    cdc_sweep_opts o;
    cdc_sweep_default_opts(&o);
    if (opts) {
        if (opts->struct_size != sizeof(cdc_sweep_opts)) return CDC_E_INVALID;
        o = *opts;
    }
    if (!s || !out || o.repack_permille > swplan::kMaxPermille || o.keep_types >> splan::kTypes) return CDC_E_INVALID;
    try {
        std::unique_ptr<cdc_sweep> plan(new cdc_sweep());  // freed on every way out, a bad_alloc of the row lists included
        plan->stats.struct_size = sizeof(cdc_sweep_stats);
        int rc;
        {
            std::lock_guard<std::mutex> lk(s->mu);
            rc = sweep_locked(s, o, plan.get());
        }
        if (rc != CDC_OK) return rc;
        *out = plan.release();
        return CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_sweep_packs(const cdc_sweep *p, cdc_sweep_pack *packs, uint64_t cap, uint64_t *needed)
{
    if (!p || (cap && !packs)) return CDC_E_INVALID;
    return hand_out(p->packs, packs, cap, needed);
}

int cdc_sweep_kept_rows(const cdc_sweep *p, cdc_state_row *rows, uint64_t cap, uint64_t *needed)
{
    if (!p || (cap && !rows)) return CDC_E_INVALID;
    return hand_out(p->kept, rows, cap, needed);
}

int cdc_sweep_repack_rows(const cdc_sweep *p, cdc_state_row *rows, uint64_t cap, uint64_t *needed)
{
    if (!p || (cap && !rows)) return CDC_E_INVALID;
    return hand_out(p->repack, rows, cap, needed);
}

int cdc_sweep_info(const cdc_sweep *p, cdc_sweep_stats *stats)
{
    if (!p || !stats || stats->struct_size != sizeof(cdc_sweep_stats)) return CDC_E_INVALID;
    *stats = p->stats;
    return CDC_OK;
}

void cdc_sweep_free(cdc_sweep *p) { delete p; }

}  // extern "C"
