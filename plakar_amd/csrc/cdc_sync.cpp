// cdc_sync_*: packfiles of one repository in, packfiles of another out
// (include/plakar_cdc.h, "sync").
//
// The reference's synchronize (cmd/plakar/subcommands/sync/sync.go:182-266)
// moves one blob at a time: GetBlob decodes it with the source's compression
// and key, PutBlob (snapshot/blobs.go:9-24) encodes it with the destination's
// and hands it to the packer channel, and packerJob (snapshot/snapshot.go:
// 51-92) appends it to a packfile that is flushed once Size() > MaxSize.  Here
// a run is a pipeline over batches of stored blobs planned up front
// (sync_plan.h), three stages on three threads and three streams:
//
//   reader   gathers the batch's stored blobs and uploads them (cdc_reader.h:
//            gather, on `readers` threads);
//   device   (the calling thread) one cdc_transcode_device_level call over the
//            blobs that were read: the check when verify is set, then the
//            re-key, open, seal, copy or re-encode;
//   packers  downloads the batch's output into a pinned slot, reports the
//            failed blobs, and `packers` threads append the surviving ones to
//            their own packfiles (cdc_packer_*), each handed to on_pack when
//            AddBlob says so and at the end.
//
// Two input slots and two output slots rotate: batch k + 1 is read and
// uploaded while batch k is on the device and batch k - 1 is downloaded and
// packed.  Transcode is synchronous and holds the per-device workspace, so the
// device stages of two batches never overlap.
#include <hip/hip_runtime.h>
#include <sys/random.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "cdc_reader.h"
#include "sync_plan.h"
#include "transcode_plan.h"

namespace {

using cdc::Clock;
using cdc::parallel_for;
using cdc::since;

static int random_bytes(uint8_t *p, size_t n)
{
    while (n) {
        const ssize_t k = getrandom(p, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return CDC_E_IO;
        p += k;
        n -= size_t(k);
    }
    return CDC_OK;
}

static bool compress_ok(int c) { return c == CDC_COMPRESS_NONE || c == CDC_COMPRESS_LZ4 || c == CDC_COMPRESS_GZIP; }

using InSlot = cdc::Arena;  // reader -> device stage: the batch's stored blobs
struct OutSlot {  // device stage -> packers
    cdc::DevBuf d;
    cdc::PinBuf h;
    std::vector<uint64_t> off;   // n + 1: the batch's blobs in the output; a failed one has no bytes
    std::vector<int32_t> status; // n
};

}  // namespace

struct cdc_sync {
    cdc::PackSource ps;  // device, the source's codec, the registered packfiles and their whole indexes (keep_rows), run lock
    cdc_sync_opts o{};
    std::vector<uint8_t> dkey, known;
    cdc_codec src{}, dst{};  // src: ps's compression and key
    hipStream_t stream[3] = {nullptr, nullptr, nullptr};  // upload, device stage, download
    InSlot in[2];
    OutSlot out[2];
    std::vector<cdc_packer *> packers;
    int dst_form = CDC_PACKFILE_PLAIN;              // cdc_sync_set_packfile_form
    std::unique_ptr<cdc::StoredCodec> dst_stored;   // the destination's stored-form codec, made by the first run that needs it
};

namespace {

struct Run {
    cdc_sync *S;
    cdc_backup_pack_fn on_pack;
    cdc_sync_blob_fn on_fail;
    void *ctx;
    splan::Plan plan;
    // the stages' hand-offs: counts of batches past each point
    cdc::Handoff hand;
    int uploaded = 0, consumed = 0, transcoded = 0, packed = 0;
    std::mutex sink_mu;  // on_pack is serialised; `stopped`: it returned a negative status
    bool stopped = false;
    cdc::StoredCodec *stored = nullptr;  // the destination's stored form: one codec for the run, used under sink_mu
    std::vector<uint8_t> tail;           // its scratch (sink_mu)
    cdc_sync_stats st{};

    const cdc_packfile_row &row(const splan::Item &it) const { return S->ps.loc.rows[it.pack][it.row]; }
};

// ---- reader stage ---------------------------------------------------------------
static void reader_stage(Run &X)
{
    cdc_sync *S = X.S;
    if (hipSetDevice(S->ps.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    for (int k = 0; k < int(X.plan.batches.size()); ++k) {
        if (!X.hand.wait_for(X.consumed, k - 1)) return;  // batch k - 2 has left this input slot
        const splan::Batch &B = X.plan.batches[k];
        const splan::Item *items = &X.plan.items[B.first];
        InSlot &I = S->in[k & 1];
        I.spans.resize(size_t(B.count));
        for (size_t b = 0; b < I.spans.size(); ++b) I.spans[b] = cdc::span_of(items[b].pack, X.row(items[b]));
        const int st = cdc::gather(S->ps.loc, I, S->o.readers, S->stream[0], &X.st.read_s, &X.st.h2d_s, nullptr);
        if (st != CDC_OK) return X.hand.abort_run(st);
        X.hand.advance(X.uploaded);
    }
}

// A first capacity for a batch's output: exact when the compression stays, a
// guess (the call reports the need) when the blobs are decoded and encoded again.
static uint64_t first_cap(const cdc_sync *S, const uint64_t *lens, size_t n)
{
    uint64_t total = 0, cap = 0;
    for (size_t i = 0; i < n; ++i) total += lens[i];
    if (S->src.compress == S->dst.compress) {
        cap = total + (S->dst.key ? 88 * uint64_t(n) + 28 * (total / 65536) : 0);
    } else {
        for (size_t i = 0; i < n; ++i)
            cap += cdc_encode_bound(lens[i] * (S->src.compress ? 4 : 1), S->dst.compress, S->dst.key != nullptr);
    }
    return std::max<uint64_t>(cap, 1u << 16);
}

// ---- device stage (the calling thread) --------------------------------------------
static void device_stage(Run &X)
{
    cdc_sync *S = X.S;
    std::vector<uint32_t> live;
    std::vector<uint64_t> off, len, oo;
    std::vector<int32_t> bst;
    std::vector<uint8_t> sums, rnd;
    for (int k = 0; k < int(X.plan.batches.size()); ++k) {
        auto t0 = Clock::now();
        if (!X.hand.wait_for(X.uploaded, k + 1)) return;
        X.st.device_wait_s += since(t0);
        if (!X.hand.wait_for(X.packed, k - 1)) return;  // batch k - 2 has left this output slot
        const splan::Batch &B = X.plan.batches[k];
        const splan::Item *items = &X.plan.items[B.first];
        InSlot &I = S->in[k & 1];
        OutSlot &O = S->out[k & 1];
        const uint32_t nb = uint32_t(B.count);
        t0 = Clock::now();
        // what was read goes through Transcode; a blob that was not has failed already
        live.clear();
        off.clear();
        len.clear();
        for (uint32_t b = 0; b < nb; ++b)
            if (I.pre[b] == CDC_OK) {
                live.push_back(b);
                off.push_back(I.eoff[b]);
                len.push_back(I.elen[b]);
            }
        const uint32_t m = uint32_t(live.size());
        oo.assign(size_t(m) + 1, 0);
        bst.assign(std::max<uint32_t>(m, 1), CDC_OK);
        if (S->o.verify) {
            sums.resize(size_t(m) * 32 + 1);
            for (uint32_t j = 0; j < m; ++j) std::memcpy(&sums[size_t(j) * 32], X.row(items[live[j]]).checksum, 32);
        }
        if (S->dst.key) {
            rnd.resize(size_t(m) * 56 + 1);
            const int st = random_bytes(rnd.data(), size_t(m) * 56);
            if (st != CDC_OK) return X.hand.abort_run(st);
        }
        if (m) {
            if (!O.d.reserve(first_cap(S, len.data(), m))) return X.hand.abort_run(CDC_E_NOMEM);
            for (;;) {
                const uint64_t cap = O.d.cap();
                const int st = cdc_transcode_device_level(S->ps.device, I.d.data(), off.data(), len.data(), m, &S->src, &S->dst,
                                                          S->o.verify ? sums.data() : nullptr,
                                                          S->dst.key ? rnd.data() : nullptr, O.d.as<uint8_t>(), cap,
                                                          oo.data(), bst.data(), S->o.level, S->stream[1]);
                if (st == CDC_E_NOSPACE && oo[m] > cap) {
                    if (!O.d.reserve(oo[m])) return X.hand.abort_run(CDC_E_NOMEM);
                    continue;
                }
                if (st != CDC_OK) return X.hand.abort_run(st == CDC_E_NOSPACE ? CDC_E_DEVICE : st);
                break;
            }
        }
        O.off.assign(size_t(nb) + 1, 0);
        O.status.assign(nb, CDC_OK);
        for (uint32_t b = 0; b < nb; ++b) O.status[b] = I.pre[b];
        tplan::spread_results(live.data(), m, oo.data(), bst.data(), nb, O.off.data(), O.status.data());
        X.st.transcode_s += since(t0);
        for (uint32_t b = 0; b < nb; ++b) {
            ++X.st.blobs;
            X.st.bytes_in += I.elen[b];
            if (O.status[b] != CDC_OK)
                ++X.st.failed;
            else
                X.st.bytes_out += O.off[b + 1] - O.off[b];
        }
        ++X.st.batches;
        X.hand.advance(X.consumed);
        X.hand.advance(X.transcoded);
    }
}

// ---- packer stage -------------------------------------------------------------------
// The packer's packfile, serialised in place, to PutPackfile (on_pack).
static void sink(Run &X, cdc_packer *p)
{
    const uint8_t *data = nullptr;
    uint64_t len = 0;
    int st = X.stored ? CDC_OK : cdc::packer_seal(p, X.S->o.timestamp, &data, &len);
    if (st == CDC_OK) {
        std::lock_guard<std::mutex> lk(X.sink_mu);
        if (!X.stopped && X.stored) {  // PutPackfile's form: the index and the footer through Encode
            st = cdc::seal_stored(*X.stored, p, X.S->o.timestamp, X.tail, &data, &len);
            if (st != CDC_OK) X.stopped = true;
        }
        if (!X.stopped) {
            ++X.st.packfiles;
            X.st.packed_bytes += len;
            const auto t0 = Clock::now();
            st = X.on_pack(X.ctx, data, len);
            X.st.callback_s += since(t0);
            if (st < 0) X.stopped = true;
        }
    }
    cdc_packer_reset(p);
    if (st < 0) X.hand.abort_run(st);
}

static void packer_stage(Run &X)
{
    cdc_sync *S = X.S;
    if (hipSetDevice(S->ps.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    const uint32_t np = uint32_t(S->packers.size());
    std::vector<uint32_t> bounds;
    for (int k = 0; k < int(X.plan.batches.size()); ++k) {
        if (!X.hand.wait_for(X.transcoded, k + 1)) return;
        const splan::Batch &B = X.plan.batches[k];
        const splan::Item *items = &X.plan.items[B.first];
        OutSlot &O = S->out[k & 1];
        const uint32_t nb = uint32_t(B.count);
        const uint64_t total = O.off[nb];
        auto t0 = Clock::now();
        if (!O.h.reserve(total)) return X.hand.abort_run(CDC_E_NOMEM);
        const uint8_t *const image = O.h.as<uint8_t>();
        if (total && (hipMemcpyAsync(O.h.data(), O.d.data(), total, hipMemcpyDeviceToHost, S->stream[2]) != hipSuccess ||
                      hipStreamSynchronize(S->stream[2]) != hipSuccess))
            return X.hand.abort_run(CDC_E_DEVICE);
        X.st.d2h_s += since(t0);
        if (X.on_fail) {
            t0 = Clock::now();
            for (uint32_t b = 0; b < nb; ++b)
                if (O.status[b] != CDC_OK) {
                    const cdc_packfile_row &R = X.row(items[b]);
                    X.on_fail(X.ctx, R.type, R.checksum, O.status[b]);
                }
            X.st.callback_s += since(t0);
        }
        t0 = Clock::now();
        const double cb0 = X.st.callback_s;  // no packer runs outside the step below
        splan::split(O.off.data(), nb, np, bounds);
        parallel_for(int(np), np, [&](size_t p) {
            cdc_packer *pk = S->packers[p];
            for (uint32_t b = bounds[p]; b < bounds[p + 1]; ++b) {
                if (O.status[b] != CDC_OK) continue;
                if (X.hand.failed()) return;
                const cdc_packfile_row &R = X.row(items[b]);
                const int st = cdc_packer_add_blob(pk, R.type, R.checksum, image + O.off[b], O.off[b + 1] - O.off[b]);
                if (st < 0) return X.hand.abort_run(st);
                if (st == 1) sink(X, pk);  // Size() > MaxSize: packerJob flushes (snapshot/snapshot.go:71)
            }
        });
        X.st.pack_s += since(t0) - (X.st.callback_s - cb0);
        X.hand.advance(X.packed);
    }
    // the last, partial packfiles
    const auto t0 = Clock::now();
    const double cb0 = X.st.callback_s;
    for (cdc_packer *pk : S->packers)
        if (cdc_packer_count(pk) && !X.hand.failed()) sink(X, pk);
    X.st.pack_s += since(t0) - (X.st.callback_s - cb0);
}

static int run_sync(cdc_sync *S, const uint8_t *wanted, uint64_t nwanted, cdc_backup_pack_fn on_pack,
                    cdc_sync_blob_fn on_fail, void *ctx, cdc_sync_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.S = S;
    X.on_pack = on_pack;
    X.on_fail = on_fail;
    X.ctx = ctx;
    std::vector<splan::Pack> packs;
    for (const auto &rows : S->ps.loc.rows) packs.push_back(splan::Pack{rows.data(), rows.size()});
    splan::plan(packs.data(), packs.size(), S->known.data(), S->o.nknown, wanted, nwanted, S->o.batch_bytes, X.plan);
    X.st.skipped = X.plan.skipped;
    X.st.path = int32_t(tplan::choose_path(S->src.compress, S->src.key != nullptr, S->dst.compress, S->dst.key != nullptr));
    for (cdc_packer *pk : S->packers) cdc_packer_reset(pk);
    if (!X.plan.batches.empty()) {
        if (hipSetDevice(S->ps.device) != hipSuccess) return CDC_E_DEVICE;
        if (S->dst_form == CDC_PACKFILE_STORED) {
            if (!S->dst_stored) {
                std::unique_ptr<cdc::StoredCodec> c(new cdc::StoredCodec());
                const int st = c->open(S->ps.device, S->dst.compress, S->dst.key);
                if (st != CDC_OK) return st;
                S->dst_stored = std::move(c);
            }
            X.stored = S->dst_stored.get();
        }
        auto guarded = [&X](void (*stage)(Run &)) {
            try {
                stage(X);
            } catch (...) {
                X.hand.abort_run(CDC_E_NOMEM);
            }
        };
        std::thread reader(guarded, reader_stage);
        std::thread packer(guarded, packer_stage);
        guarded(device_stage);
        reader.join();
        packer.join();
    }
    for (cdc_packer *pk : S->packers) cdc_packer_reset(pk);  // what a run that broke off left behind
    X.st.wall_s = since(w0);
    if (stats) {
        X.st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(X.st)));
        std::memcpy(stats, &X.st, X.st.struct_size);
    }
    return X.hand.fail;
}

}  // namespace

extern "C" {

void cdc_sync_default_opts(cdc_sync_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->verify = 1;
}

int cdc_sync_new(int device, const cdc_sync_opts *opts, cdc_sync **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts) || device < 0 || device >= cdc::kMaxDevices || !compress_ok(opts->src.compress) ||
        !compress_ok(opts->dst.compress) || !cdc::level_ok(opts->level) || opts->readers < 0 || opts->readers > 256 ||
        opts->packers < 0 || opts->packers > 256 || (opts->nknown && !opts->known) ||
        opts->nknown > SIZE_MAX / splan::kKeyBytes || !splan::sorted33(opts->known, opts->nknown))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *s = new (std::nothrow) cdc_sync();
    if (!s) return CDC_E_NOMEM;
    try {
        s->ps.open(device, opts->src.compress, opts->src.key);
        s->o = *opts;
        if (opts->dst.key) s->dkey.assign(opts->dst.key, opts->dst.key + 32);
        if (opts->nknown) s->known.assign(opts->known, opts->known + splan::kKeyBytes * opts->nknown);
        s->src = cdc_codec{s->ps.compress, s->ps.key_ptr()};
        s->dst = cdc_codec{opts->dst.compress, s->dkey.empty() ? nullptr : s->dkey.data()};
        s->o.src.key = s->o.dst.key = s->o.known = nullptr;
        if (!s->o.readers) s->o.readers = 8;
        if (!s->o.packers) s->o.packers = 8;
        if (!s->o.batch_bytes) s->o.batch_bytes = 64ull << 20;
        s->ps.loc.keep_rows = true;
        for (int p = 0; p < s->o.packers; ++p) {
            cdc_packer *pk = nullptr;
            if (cdc_packer_new(s->o.packfile_max, &pk) != CDC_OK) throw std::bad_alloc();
            s->packers.push_back(pk);
        }
    } catch (...) {
        cdc_sync_free(s);
        return CDC_E_NOMEM;
    }
    bool ok = hipSetDevice(device) == hipSuccess;
    for (int i = 0; i < 3; ++i) ok = ok && hipStreamCreateWithFlags(&s->stream[i], hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        cdc_sync_free(s);
        return CDC_E_DEVICE;
    }
    *out = s;
    return CDC_OK;
}

int cdc_sync_add_packfile(cdc_sync *s, const uint8_t *bytes, uint64_t len)
{
    return s && (bytes || !len) ? s->ps.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_sync_add_packfile_path(cdc_sync *s, const char *path)
{
    return s && path ? s->ps.add_path(path) : CDC_E_INVALID;
}

int cdc_sync_add_packfiles(cdc_sync *s, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return s ? s->ps.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_sync_run(cdc_sync *s, const uint8_t *wanted, uint64_t nwanted, cdc_backup_pack_fn on_pack, cdc_sync_blob_fn on_fail,
                 void *ctx, cdc_sync_stats *stats)
{
    if (!s || !on_pack || (stats && stats->struct_size < 8) || (wanted && !splan::sorted33(wanted, nwanted)))
        return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(s->ps.run_mu);
    try {
        return run_sync(s, wanted, nwanted, on_pack, on_fail, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_sync_set_packfile_form(cdc_sync *s, int form)
{
    if (!s || (form != CDC_PACKFILE_PLAIN && form != CDC_PACKFILE_STORED)) return CDC_E_INVALID;
    std::unique_lock<std::mutex> lk(s->ps.run_mu, std::try_to_lock);
    if (!lk.owns_lock()) return CDC_E_INVALID;  // a run is in progress
    s->dst_form = form;
    return CDC_OK;
}

void cdc_sync_free(cdc_sync *s)
{
    if (!s) return;
    s->ps.release(s->stream, 3);
    for (cdc_packer *pk : s->packers) cdc_packer_free(pk);
    if (!s->dkey.empty()) std::memset(s->dkey.data(), 0, s->dkey.size());
    delete s;  // the slots' buffers go with it, the streams drained above
}

}  // extern "C"
