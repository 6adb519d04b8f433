// cdc_grep_*: fixed strings in snapshot files, from packfiles and chunk lists to
// matching lines (include/plakar_cdc.h, "grep").
//
// The reference cannot look inside a file (Snapshot.Search matches names,
// sizes and content types); a caller had to restore the files and search on
// the host.  Here a run takes a batch of files, and per batch of whole files
//
//   read      the distinct encoded blobs gathered and uploaded (restore's plan:
//             a blob many files share is there once; cdc_reader.h: gather);
//   decode    the shared decode step over them (cdc_reader.h: decode_batch);
//   assemble  the images of the files laid out back to back;
//   table, scan, compact
//             cdc_grep_device's stages over the images (cdc::grep_texts), in
//             groups of files of at most max_lines lines;
//   d2h       one copy back of the group's hit records;
//   emit      want_text: the emit records (grep_plan.h), cdc_diff_emit_device
//             and one copy back of the text.
//
// The stages of a batch run in sequence on the calling thread, and the files
// are reported in file order once everything before them is known.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "cdc_reader.h"
#include "grep_plan.h"
#include "restore_plan.h"

namespace {

using cdc::Clock;
using cdc::since;

constexpr uint64_t kMaxBatch = 1ull << 30;
constexpr uint64_t kMaxLines = 1ull << 31;

}  // namespace

struct cdc_grep {
    cdc::PackSource src;  // device, codec, locator, run lock
    cdc_grep_opts o{};
    hipStream_t stream = nullptr;
    cdc::Arena in;  // the batch's encoded blobs
    cdc::PinBuf hhits, hout;
    cdc::DevBuf plain, image, hits, out;
};

namespace {

struct FileState {
    int status = CDC_OK;
    int64_t bad_chunk = -1;
    bool done = false;       // nothing more will be learnt about it
    int binary = 0;
    uint64_t size = 0, lines = 0, matched = 0;
    std::vector<uint32_t> blob;
    std::vector<cdc_grep_hit> hits;
    std::vector<uint8_t> text;
};

struct Run {
    cdc_grep *R;
    const cdc_grep_query *q;
    const cdc_check_file *files;
    int n;
    cdc_grep_file_fn on_file;
    void *ctx;
    std::vector<FileState> fs;
    int next = 0;  // the first file not reported yet
    cdc_grep_stats st{};

    void fail(int i, int status, int64_t chunk)
    {
        FileState &F = fs[size_t(i)];
        if (F.status != CDC_OK) return;
        F.status = status, F.bad_chunk = chunk;
    }
    // report, in file order, every file up to the first one that is not done
    void report()
    {
        for (; next < n && fs[size_t(next)].done; ++next) {
            FileState &F = fs[size_t(next)];
            st.failed_files += F.status != CDC_OK;
            if (on_file) {
                cdc_grep_result r{};
                r.index = next;
                r.status = F.status;
                r.bad_chunk = F.status != CDC_OK ? F.bad_chunk : -1;
                r.binary = F.binary;
                r.size = F.size, r.lines = F.lines, r.matched = F.matched;
                r.hits = F.hits.empty() ? nullptr : F.hits.data();
                r.nhits = F.hits.size();
                r.text = F.text.empty() ? nullptr : F.text.data();
                r.text_len = F.text.size();
                on_file(ctx, &r);
            }
            std::vector<cdc_grep_hit>().swap(F.hits);
            std::vector<uint8_t>().swap(F.text);
            std::vector<uint32_t>().swap(F.blob);
        }
    }
};

static cdc_grep_hit *hits_room(void *ctx, uint64_t records)
{
    cdc_grep *R = static_cast<cdc_grep *>(ctx);
    return R->hits.reserve(sizeof(cdc_grep_hit) * size_t(records)) ? R->hits.as<cdc_grep_hit>() : nullptr;
}

// One batch: the files `members` (indices into X.files), all found, not empty and within the budget.
static int run_batch(Run &X, const std::vector<int> &members)
{
    cdc_grep *R = X.R;
    hipStream_t st = R->stream;
    // ---- the plan: one batch of whole files
    std::vector<rplan::File> files;
    for (int i : members) files.push_back(rplan::File{X.files[i].nchunks, X.fs[size_t(i)].blob.data(), X.files[i].lengths});
    std::vector<rplan::Batch> batches;
    rplan::plan(files.data(), files.size(), ~0ull, batches);
    if (batches.size() != 1 || batches[0].pieces.size() != files.size()) return CDC_E_DEVICE;  // never: no budget
    const rplan::Batch &B = batches[0];
    const uint32_t nb = uint32_t(B.blobs.size());
    X.st.bytes += B.out_bytes;
    X.st.segments += B.segs.size();
    X.st.decoded_blobs += nb;
    ++X.st.batches;
    // ---- read and upload
    cdc::Arena &I = R->in;
    I.set_blobs(R->src.loc, B.blobs.data(), nb);
    int s = cdc::gather(R->src.loc, I, R->o.threads, st, &X.st.read_s, &X.st.h2d_s, &X.st.encoded_bytes);
    if (s != CDC_OK) return s;
    // ---- Decode and compare
    if (!R->plain.reserve(B.plain_bytes)) return CDC_E_NOMEM;
    uint8_t *const plain = R->plain.as<uint8_t>();
    cdc::Decoded D;
    D.set_blobs(true, R->src.loc, B.blobs.data(), nb);
    s = cdc::decode_batch(cdc::DecodeCtx{R->src.device, R->src.compress, R->src.key_ptr(), true, st}, I, plain, B.plain_bytes, D,
                          cdc::DecodeTally{&X.st.decoded_bytes, &X.st.decode_s, &X.st.verify_s});
    if (s != CDC_OK) return s;
    const std::vector<int32_t> &bst = D.bst;
    const std::vector<uint64_t> &pos = D.pos;
    const uint64_t plain_used = D.plain_used;
    // a failed blob fails its files: the first such chunk
    for (size_t p = 0; p < B.pieces.size(); ++p) {
        const rplan::Piece &P = B.pieces[p];
        for (uint64_t g = P.seg0; g < P.seg0 + P.nchunks; ++g)
            if (bst[B.segs[g].blob] != CDC_OK) {
                X.fail(members[p], bst[B.segs[g].blob], int64_t(g - P.seg0));
                break;
            }
    }
    // ---- the images of the files that go on
    auto t0 = Clock::now();
    std::vector<int> live;  // position in members
    std::vector<uint64_t> so, sl, sd, toff, tlen;
    for (size_t m = 0; m < members.size(); ++m) {
        if (X.fs[size_t(members[m])].status != CDC_OK) {
            X.fs[size_t(members[m])].done = true;
            continue;
        }
        live.push_back(int(m));
        const rplan::Piece &P = B.pieces[m];
        toff.push_back(P.dst_off);
        tlen.push_back(P.len);
        for (uint64_t g = P.seg0; g < P.seg0 + P.nchunks; ++g) {
            so.push_back(pos[B.segs[g].blob]);
            sl.push_back(B.segs[g].len);
            sd.push_back(B.segs[g].dst_off);
        }
    }
    if (live.empty()) return CDC_OK;
    if (!R->image.reserve(B.out_bytes)) return CDC_E_NOMEM;
    uint8_t *const image = R->image.as<uint8_t>();
    for (size_t k = 0; k < so.size(); ++k)
        if (sl[k] > plain_used || so[k] > plain_used - sl[k]) return CDC_E_DEVICE;  // the plan's places are inside what Decode wrote
    s = cdc_assemble_device(R->src.device, plain, plain_used, so.data(), sl.data(), sd.data(), so.size(), image, B.out_bytes, st);
    if (s != CDC_OK) return s;
    if (hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
    X.st.assemble_s += since(t0);
    // ---- the line counts, then groups of files of at most max_lines lines
    t0 = Clock::now();
    const uint32_t ntexts = uint32_t(toff.size());
    std::vector<uint64_t> counts(ntexts);
    uint64_t all = 0;
    s = cdc_line_table_device(R->src.device, image, B.out_bytes, toff.data(), tlen.data(), ntexts, nullptr, 0, counts.data(), &all, st);
    if (s != CDC_OK && s != CDC_E_NOSPACE) return s;
    X.st.table_s += since(t0);
    std::vector<std::vector<int>> groups(1);  // positions in live
    uint64_t glines = 0;
    for (size_t k = 0; k < live.size(); ++k) {
        if (counts[k] > R->o.max_lines) {
            X.fail(members[size_t(live[k])], CDC_E_NOSPACE, -1);
            X.fs[size_t(members[size_t(live[k])])].done = true;
            continue;
        }
        if (glines + counts[k] > R->o.max_lines) {
            groups.emplace_back();
            glines = 0;
        }
        groups.back().push_back(int(k));
        glines += counts[k];
    }
    const uint64_t limit = X.q->limit ? X.q->limit : 65536;
    const uint32_t max_line = X.q->max_line_bytes ? X.q->max_line_bytes : 4096;
    for (const std::vector<int> &G : groups) {
        if (G.empty()) continue;
        const size_t nf = G.size();
        std::vector<uint64_t> go(nf), gl(nf), lines(nf), matched(nf);
        std::vector<uint8_t> binary(nf);
        for (size_t k = 0; k < nf; ++k) go[k] = toff[size_t(G[k])], gl[k] = tlen[size_t(G[k])];
        uint64_t nhits = 0;
        double times[3] = {0, 0, 0};
        s = cdc::grep_texts(R->src.device, image, B.out_bytes, go.data(), gl.data(), uint32_t(nf), X.q->patterns, X.q->pattern_len,
                            X.q->npatterns, X.q->flags, limit, hits_room, R, lines.data(), matched.data(), binary.data(), &nhits, st,
                            times);
        if (s != CDC_OK) return s == CDC_E_NOSPACE ? CDC_E_NOMEM : s;
        X.st.table_s += times[0], X.st.scan_s += times[1], X.st.compact_s += times[2];
        // ---- the records back
        t0 = Clock::now();
        if (!R->hhits.reserve(sizeof(cdc_grep_hit) * size_t(nhits))) return CDC_E_NOMEM;
        cdc_grep_hit *const hh = R->hhits.as<cdc_grep_hit>();
        if (nhits && (hipMemcpyAsync(hh, R->hits.data(), sizeof(cdc_grep_hit) * size_t(nhits), hipMemcpyDeviceToHost, st) != hipSuccess ||
                      hipStreamSynchronize(st) != hipSuccess))
            return CDC_E_DEVICE;
        X.st.d2h_s += since(t0);
        // ---- the matching lines' text
        uint64_t out_bytes = 0;
        if (X.q->want_text && nhits) {
            t0 = Clock::now();
            std::vector<cdc_emit_rec> recs;
            recs.reserve(size_t(nhits));
            out_bytes = gplan::emit_records(hh, nhits, max_line, 0, recs);
            if (!R->out.reserve(out_bytes) || !R->hout.reserve(out_bytes)) return CDC_E_NOMEM;
            s = cdc_diff_emit_device(R->src.device, image, B.out_bytes, nullptr, 0, recs.data(), recs.size(), R->out.data(), out_bytes, st);
            if (s != CDC_OK) return s;
            if (hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
            X.st.emit_s += since(t0);
            t0 = Clock::now();
            if (hipMemcpyAsync(R->hout.data(), R->out.data(), out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return CDC_E_DEVICE;
            X.st.d2h_s += since(t0);
            X.st.out_bytes += out_bytes;
        }
        // ---- per file: its records, with the file's index and the line's place in the file
        uint64_t h0 = 0, o0 = 0;
        for (size_t k = 0; k < nf; ++k) {
            const int i = members[size_t(live[size_t(G[k])])];
            FileState &F = X.fs[size_t(i)];
            const uint64_t take = std::min(matched[k], limit);
            F.lines = lines[k], F.matched = matched[k], F.binary = binary[k];
            F.hits.assign(hh + h0, hh + h0 + take);
            uint64_t tbytes = 0;
            for (cdc_grep_hit &H : F.hits) {
                H.text = uint32_t(i);
                H.off -= go[k];
                X.st.occurrences += H.nocc;
                tbytes += uint64_t(std::min(H.len, max_line)) + 1;
            }
            if (out_bytes) F.text.assign(R->hout.as<uint8_t>() + o0, R->hout.as<uint8_t>() + o0 + tbytes), o0 += tbytes;
            h0 += take;
            X.st.lines += lines[k], X.st.matched_lines += matched[k], X.st.hits += take;
            F.done = true;
        }
    }
    return CDC_OK;
}

static void write_stats(cdc_grep_stats *stats, cdc_grep_stats &st)
{
    if (!stats) return;
    st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(st)));
    std::memcpy(stats, &st, st.struct_size);
}

static int run_files(cdc_grep *R, const cdc_grep_query *q, const cdc_check_file *files, int n, cdc_grep_file_fn on_file, void *ctx,
                     cdc_grep_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.R = R;
    X.q = q;
    X.files = files;
    X.n = n;
    X.on_file = on_file;
    X.ctx = ctx;
    X.fs.resize(size_t(n));
    X.st.files = uint64_t(n);
    std::vector<bool> used(R->src.loc.locs.size(), false);
    std::vector<int> members;
    uint64_t bytes = 0;
    int fail = CDC_OK;
    auto flush = [&] {
        if (members.empty() || fail != CDC_OK) return;
        if (hipSetDevice(R->src.device) != hipSuccess) {
            fail = CDC_E_DEVICE;
            return;
        }
        fail = run_batch(X, members);
        if (fail == CDC_OK) X.report();
        members.clear();
        bytes = 0;
    };
    for (int i = 0; i < n && fail == CDC_OK; ++i) {
        const cdc_check_file &P = files[i];
        FileState &S = X.fs[size_t(i)];
        S.blob.resize(size_t(P.nchunks));
        const int64_t miss = cdc::resolve(R->src.loc, P.checksums, P.nchunks, S.blob.data());
        if (miss >= 0) X.fail(i, CDC_E_NOTFOUND, miss);
        for (uint64_t c = 0; c < (miss < 0 ? P.nchunks : uint64_t(miss)); ++c) S.size += P.lengths[c];
        if (S.status == CDC_OK && S.size > R->o.batch_bytes) X.fail(i, CDC_E_NOSPACE, -1);
        if (S.status != CDC_OK || S.size == 0) {  // an empty file: 0 lines, no hit, no device work
            S.done = true;
            X.report();  // at once when no file before it waits for its batch
            continue;
        }
        for (uint32_t id : S.blob)
            if (!used[id]) {
                used[id] = true;
                ++X.st.distinct_blobs;
            }
        if (!members.empty() && bytes + S.size > R->o.batch_bytes) flush();
        members.push_back(i);
        bytes += S.size;
    }
    flush();
    // the files of a run that broke off
    for (int i = X.next; i < n; ++i) {
        FileState &S = X.fs[size_t(i)];
        if (!S.done) {
            if (S.status == CDC_OK) S.status = fail != CDC_OK ? fail : CDC_E_DEVICE;
            S.lines = S.matched = 0, S.binary = 0;
            S.hits.clear(), S.text.clear();
            S.done = true;
        }
    }
    X.report();
    X.st.wall_s = since(w0);
    write_stats(stats, X.st);
    return fail;
}

}  // namespace

extern "C" {

void cdc_grep_default_opts(cdc_grep_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
}

int cdc_grep_new(int device, const cdc_grep_opts *opts, cdc_grep **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts) || device < 0 || device >= cdc::kMaxDevices || opts->threads < 0 ||
        opts->threads > 256 || opts->batch_bytes > kMaxBatch || opts->max_lines > kMaxLines ||
        (opts->compress != CDC_COMPRESS_NONE && opts->compress != CDC_COMPRESS_LZ4 && opts->compress != CDC_COMPRESS_GZIP))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *c = new (std::nothrow) cdc_grep();
    if (!c) return CDC_E_NOMEM;
    try {
        c->src.open(device, opts->compress, opts->key);
        c->o = *opts;
        c->o.key = nullptr;
        if (!c->o.threads) c->o.threads = 8;
        if (!c->o.batch_bytes) c->o.batch_bytes = 256ull << 20;
        if (!c->o.max_lines) c->o.max_lines = 16ull << 20;
    } catch (...) {
        delete c;
        return CDC_E_NOMEM;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->stream = nullptr;
        cdc_grep_free(c);
        return CDC_E_DEVICE;
    }
    *out = c;
    return CDC_OK;
}

int cdc_grep_add_packfile(cdc_grep *g, const uint8_t *bytes, uint64_t len)
{
    return g && (bytes || !len) ? g->src.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_grep_add_packfile_path(cdc_grep *g, const char *path)
{
    return g && path ? g->src.add_path(path) : CDC_E_INVALID;
}

int cdc_grep_add_packfiles(cdc_grep *g, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return g ? g->src.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_grep_files(cdc_grep *g, const cdc_grep_query *q, const cdc_check_file *files, int n, cdc_grep_file_fn on_file, void *ctx,
                   cdc_grep_stats *stats)
{
    if (!g || !q || n < 0 || (n && !files) || (stats && stats->struct_size < 8) || q->struct_size != sizeof(*q) ||
        gplan::validate(q->patterns, q->pattern_len, q->npatterns, q->flags) != CDC_OK)
        return CDC_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (files[i].nchunks && (!files[i].checksums || !files[i].lengths)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(g->src.run_mu);
    try {
        return run_files(g, q, files, n, on_file, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_grep_free(cdc_grep *g)
{
    if (!g) return;
    g->src.release(&g->stream, 1);
    delete g;
}

}  // extern "C"
