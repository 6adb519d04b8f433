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
#include <mutex>
#include <new>
#include <vector>

#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "cdc_state.h"

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
    cdc::DevBuf words;         // kTypes + 1 counters, then the rows counter
    cdc::DevBuf qbuf;          // the host lookups' and cdc_state_rows' staging
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
    bool rebuild = false;
    cdc::DevBuf bigger;
    uint64_t new_cap = s->capacity;
    if (news) {
        rc = reserve_recs(s, after);
        if (rc != CDC_OK) return rc;
        if (after > s->capacity / 2) {
            while (new_cap / 2 < after) new_cap *= 2;
            if (!bigger.reserve(size_t(new_cap) * 8)) return CDC_E_NOMEM;
            rebuild = true;
        }
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
        if (rebuild) {
            if (hipMemsetAsync(bigger.data(), 0xFF, size_t(new_cap) * 8, s->stream) != hipSuccess) return CDC_E_DEVICE;
            s->slots = std::move(bigger);
            s->capacity = new_cap;
        }
        rc = cst::launch_insert(s->device, s->table(), rebuild ? 0 : s->nrecs, after, s->stream);
        if (rc != CDC_OK) return rc;
        s->nrecs = after;
        uint64_t counts[splan::kTypes + 1];
        rc = cst::launch_count(s->device, s->table(), s->counters(), s->stream);
        if (rc != CDC_OK) return rc;
        if (!copy(s, counts, s->counters(), sizeof(counts), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
        for (uint32_t t = 0; t < splan::kTypes; ++t) s->stats.rows[t] = counts[t];
        s->stats.deleted_snapshots = counts[splan::kTypes];
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
    int rc = ensure_device(s);
    if (rc != CDC_OK) return rc;
    const size_t qb = align_up(size_t(n) * 32, 256);
    if (!s->qbuf.reserve(qb + size_t(n) * sizeof(cdc_state_row))) return CDC_E_NOMEM;
    uint8_t *const dq = s->qbuf.as<uint8_t>();
    cdc_state_row *const dr = reinterpret_cast<cdc_state_row *>(dq + qb);
    if (!copy(s, dq, checksums, size_t(n) * 32, hipMemcpyHostToDevice)) return CDC_E_DEVICE;
    rc = cst::launch_lookup(s->device, s->table(), type, dq, n, dr, s->stream);
    if (rc != CDC_OK) return rc;
    if (!copy(s, out, dr, size_t(n) * sizeof(cdc_state_row), hipMemcpyDeviceToHost) || !sync(s)) return CDC_E_DEVICE;
    return CDC_OK;
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

}  // extern "C"
