// cdc_diff_script, cdc_diff_emit_plan and cdc_diff_*: unified diffs of snapshot
// files (include/plakar_cdc.h, "diff").
//
// The reference diffs one pair at a time: cmd/plakar/subcommands/diff/diff.go:
// 152-196 reads both files whole, splits them into lines, runs go-difflib's
// UnifiedDiff and prints the text.  Here a run takes a batch of pairs.  Pairs
// with equal object checksums or chunk lists are identical without a read;
// the others are laid into batches of whole pairs, and per batch
//
//   read      the distinct encoded blobs of both sides gathered and uploaded
//             (restore's plan: a blob the two versions share is there once;
//             cdc_reader.h: gather);
//   decode    the shared decode step over them (cdc_reader.h: decode_batch);
//   assemble  both images of every pair laid out back to back;
//   table     cdc_line_table_device over the images, the records copied back;
//   ids       cdc_line_ids_device: exact ids per pair;
//   match     the matcher and the emit plan on `threads` host threads, a pair
//             per task (diff_plan.h);
//   emit      cdc_diff_emit_device over all pairs' records, one copy back of
//             the batch's diff text, then the callbacks.
//
// The stages of a batch run in sequence on the calling thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cdc_reader.h"
#include "diff_plan.h"
#include "restore_plan.h"

namespace {

using cdc::Clock;
using cdc::parallel_for;
using cdc::since;

constexpr uint64_t kMaxBatch = 1ull << 30;
constexpr uint64_t kMaxLines = 1ull << 31;

}  // namespace

struct cdc_diff {
    cdc::PackSource src;  // device, codec, locator, run lock
    cdc_diff_opts o{};
    hipStream_t stream = nullptr;
    cdc::Arena in;  // the batch's encoded blobs
    cdc::PinBuf hrecs, hlit, hout;
    cdc::DevBuf plain, image, recs, lit, out;
};

namespace {

struct PairState {
    int status = CDC_OK;
    int bad_side = -1;
    int64_t bad_chunk = -1;
    bool skipped = false;      // identical without device work
    std::vector<uint32_t> blob[2];
    uint64_t size[2] = {0, 0};
};

struct Run {
    cdc_diff *R;
    const cdc_diff_pair *pairs;
    int n;
    cdc_diff_pair_fn on_pair;
    void *ctx;
    std::vector<PairState> ps;
    std::vector<uint8_t> reported;
    cdc_diff_stats st{};

    void report(int i, bool identical, uint64_t al, uint64_t bl, uint64_t hunks, const uint8_t *text, uint64_t len)
    {
        const PairState &P = ps[size_t(i)];
        reported[size_t(i)] = 1;
        st.failed_pairs += P.status != CDC_OK;
        st.identical_pairs += P.status == CDC_OK && identical;
        if (!on_pair) return;
        cdc_diff_result r{};
        r.index = i;
        r.status = P.status;
        r.bad_side = P.status != CDC_OK ? P.bad_side : -1;
        r.bad_chunk = P.status != CDC_OK ? P.bad_chunk : -1;
        r.identical = P.status == CDC_OK && identical;
        r.a_lines = al, r.b_lines = bl, r.hunks = hunks;
        r.text = len ? text : nullptr;
        r.text_len = len;
        on_pair(ctx, &r);
    }
    void fail(int i, int status, int side, int64_t chunk)
    {
        PairState &P = ps[size_t(i)];
        if (P.status != CDC_OK) return;
        P.status = status, P.bad_side = side, P.bad_chunk = chunk;
    }
};

static bool same_chunks(const cdc_check_file &a, const cdc_check_file &b)
{
    return a.nchunks == b.nchunks && (a.nchunks == 0 || (std::memcmp(a.checksums, b.checksums, 32 * a.nchunks) == 0 &&
                                                         std::memcmp(a.lengths, b.lengths, 4 * a.nchunks) == 0));
}

// One batch: the pairs `members` (indices into X.pairs), all found and within the budget.
static int run_batch(Run &X, const std::vector<int> &members)
{
    cdc_diff *R = X.R;
    hipStream_t st = R->stream;
    // ---- the plan: one batch of whole files, a0 b0 a1 b1 ...
    std::vector<rplan::File> files;
    for (int i : members)
        for (int s = 0; s < 2; ++s) {
            const cdc_check_file &F = s ? X.pairs[i].b : X.pairs[i].a;
            files.push_back(rplan::File{F.nchunks, X.ps[size_t(i)].blob[s].data(), F.lengths});
        }
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
    // a failed blob fails its pairs: the first such chunk, a's before b's (pieces are a0 b0 a1 b1 ...)
    for (size_t p = 0; p < B.pieces.size(); ++p) {
        const rplan::Piece &P = B.pieces[p];
        for (uint64_t g = P.seg0; g < P.seg0 + P.nchunks; ++g)
            if (bst[B.segs[g].blob] != CDC_OK) {
                X.fail(members[p / 2], bst[B.segs[g].blob], int(p & 1), int64_t(g - P.seg0));
                break;
            }
    }
    // ---- both images of the pairs that go on
    auto t0 = Clock::now();
    std::vector<int> live;       // position in members
    std::vector<uint64_t> so, sl, sd, toff, tlen;
    for (size_t m = 0; m < members.size(); ++m) {
        if (X.ps[size_t(members[m])].status != CDC_OK) continue;
        live.push_back(int(m));
        for (size_t p = 2 * m; p < 2 * m + 2; ++p) {
            const rplan::Piece &P = B.pieces[p];
            toff.push_back(P.dst_off);
            tlen.push_back(P.len);
            for (uint64_t g = P.seg0; g < P.seg0 + P.nchunks; ++g) {
                so.push_back(pos[B.segs[g].blob]);
                sl.push_back(B.segs[g].len);
                sd.push_back(B.segs[g].dst_off);
            }
        }
    }
    auto report_dead = [&] {
        for (int i : members)
            if (X.ps[size_t(i)].status != CDC_OK) X.report(i, false, 0, 0, 0, nullptr, 0);
    };
    if (live.empty()) {
        report_dead();
        return CDC_OK;
    }
    if (!R->image.reserve(B.out_bytes)) return CDC_E_NOMEM;
    uint8_t *const image = R->image.as<uint8_t>();
    for (size_t k = 0; k < so.size(); ++k)
        if (sl[k] > plain_used || so[k] > plain_used - sl[k]) return CDC_E_DEVICE;  // the plan's places are inside what Decode wrote
    s = cdc_assemble_device(R->src.device, plain, plain_used, so.data(), sl.data(), sd.data(), so.size(), image, B.out_bytes, st);
    if (s != CDC_OK) return s;
    if (hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
    X.st.assemble_s += since(t0);
    // ---- the line counts, then groups of pairs of at most max_lines lines
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
        const uint64_t nl = counts[2 * k] + counts[2 * k + 1];
        if (nl > R->o.max_lines) {
            X.fail(members[size_t(live[k])], CDC_E_NOSPACE, -1, -1);
            continue;
        }
        if (glines + nl > R->o.max_lines) {
            groups.emplace_back();
            glines = 0;
        }
        groups.back().push_back(int(k));
        glines += nl;
    }
    report_dead();
    const uint32_t context = uint32_t(R->o.context);
    for (const std::vector<int> &G : groups) {
        if (G.empty()) continue;
        const size_t np = G.size();
        // ---- the table of the group's texts
        t0 = Clock::now();
        std::vector<uint64_t> go(2 * np), gl(2 * np), gc(2 * np), line0(2 * np + 1, 0);
        for (size_t q = 0; q < np; ++q)
            for (int sd2 = 0; sd2 < 2; ++sd2) {
                go[2 * q + sd2] = toff[2 * size_t(G[q]) + sd2];
                gl[2 * q + sd2] = tlen[2 * size_t(G[q]) + sd2];
                line0[2 * q + sd2 + 1] = line0[2 * q + sd2] + counts[2 * size_t(G[q]) + sd2];
            }
        const uint64_t nlines = line0[2 * np];
        if (!R->recs.reserve(nlines * sizeof(cdc_line_rec)) || !R->hrecs.reserve(nlines * sizeof(cdc_line_rec))) return CDC_E_NOMEM;
        cdc_line_rec *const d_recs = R->recs.as<cdc_line_rec>(), *const hrecs = R->hrecs.as<cdc_line_rec>();
        uint64_t got = 0;
        s = cdc_line_table_device(R->src.device, image, B.out_bytes, go.data(), gl.data(), uint32_t(2 * np), d_recs, nlines, gc.data(),
                                  &got, st);
        if (s != CDC_OK) return s == CDC_E_NOSPACE ? CDC_E_DEVICE : s;
        if (hipMemcpyAsync(hrecs, d_recs, nlines * sizeof(cdc_line_rec), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return CDC_E_DEVICE;
        X.st.table_s += since(t0);
        X.st.lines += nlines;
        // ---- exact ids
        t0 = Clock::now();
        std::vector<uint64_t> pair0(np + 1);
        for (size_t q = 0; q <= np; ++q) pair0[q] = line0[2 * q];
        std::vector<uint32_t> ids(nlines);
        uint32_t rounds = 0;
        s = cdc::line_ids(R->src.device, image, hrecs, nlines, pair0.data(), uint32_t(np), R->o.hash_bits, ids.data(), &rounds, st,
                          R->o.threads);  // the table's own records: inside the image
        if (s != CDC_OK) return s;
        X.st.verify_rounds += rounds;
        for (size_t q = 0; q < np; ++q)
            for (uint64_t i = pair0[q]; i < pair0[q + 1]; ++i) X.st.distinct_lines += ids[i] == i - pair0[q];
        X.st.ids_s += since(t0);
        // ---- the matcher and the emit plan, a pair per task
        t0 = Clock::now();
        std::vector<dplan::Plan> plans(np);
        std::atomic<bool> oom{false};
        parallel_for(R->o.threads, np, [&](size_t q) {
            try {
                const uint64_t a0 = line0[2 * q], b0 = line0[2 * q + 1], e = line0[2 * q + 2];
                const std::vector<cdc_diff_op> ops =
                    dplan::script(ids.data() + a0, size_t(b0 - a0), ids.data() + b0, size_t(e - b0), context);
                const cdc_diff_pair &P = X.pairs[members[size_t(live[size_t(G[q])])]];
                dplan::emit_plan(ops.data(), ops.size(), hrecs + a0, hrecs + b0, P.from_name, P.to_name, 0, 0, plans[q]);
            } catch (...) {
                oom.store(true);
            }
        });
        if (oom.load()) return CDC_E_NOMEM;
        std::vector<uint64_t> out0(np + 1, 0), lit0(np + 1, 0);
        size_t nrecs = 0;
        for (size_t q = 0; q < np; ++q) {
            out0[q + 1] = out0[q] + plans[q].out_bytes;
            lit0[q + 1] = lit0[q] + plans[q].lit.size();
            nrecs += plans[q].recs.size();
            X.st.hunks += plans[q].hunks;
        }
        std::vector<cdc_emit_rec> recs;
        recs.reserve(nrecs);
        if (!R->hlit.reserve(lit0[np]) || !R->lit.reserve(lit0[np]) || !R->out.reserve(out0[np]) || !R->hout.reserve(out0[np]))
            return CDC_E_NOMEM;
        for (size_t q = 0; q < np; ++q) {
            for (cdc_emit_rec r : plans[q].recs) {
                r.dst_off += out0[q];
                if (r.flags & CDC_EMIT_LITERAL) r.src_off += lit0[q];
                recs.push_back(r);
            }
            std::memcpy(R->hlit.as<uint8_t>() + lit0[q], plans[q].lit.data(), plans[q].lit.size());
        }
        X.st.match_s += since(t0);
        // ---- emit and copy back
        t0 = Clock::now();
        if (out0[np]) {
            if (hipMemcpyAsync(R->lit.data(), R->hlit.data(), lit0[np], hipMemcpyHostToDevice, st) != hipSuccess) return CDC_E_DEVICE;
            s = cdc_diff_emit_device(R->src.device, image, B.out_bytes, R->lit.data(), lit0[np], recs.data(), recs.size(), R->out.data(),
                                     out0[np], st);
            if (s != CDC_OK) return s;
            if (hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
        }
        X.st.emit_s += since(t0);
        t0 = Clock::now();
        if (out0[np] && (hipMemcpyAsync(R->hout.data(), R->out.data(), out0[np], hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipStreamSynchronize(st) != hipSuccess))
            return CDC_E_DEVICE;
        X.st.d2h_s += since(t0);
        X.st.out_bytes += out0[np];
        for (size_t q = 0; q < np; ++q)
            X.report(members[size_t(live[size_t(G[q])])], plans[q].hunks == 0, gc[2 * q], gc[2 * q + 1], plans[q].hunks,
                     R->hout.as<uint8_t>() + out0[q], plans[q].out_bytes);
    }
    return CDC_OK;
}

static void write_stats(cdc_diff_stats *stats, cdc_diff_stats &st)
{
    if (!stats) return;
    st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(st)));
    std::memcpy(stats, &st, st.struct_size);
}

static int run_pairs(cdc_diff *R, const cdc_diff_pair *pairs, int n, cdc_diff_pair_fn on_pair, void *ctx, cdc_diff_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.R = R;
    X.pairs = pairs;
    X.n = n;
    X.on_pair = on_pair;
    X.ctx = ctx;
    X.ps.resize(size_t(n));
    X.reported.assign(size_t(n), 0);
    X.st.pairs = uint64_t(n);
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
        members.clear();
        bytes = 0;
    };
    for (int i = 0; i < n && fail == CDC_OK; ++i) {
        const cdc_diff_pair &P = pairs[i];
        PairState &S = X.ps[size_t(i)];
        if ((P.a.object_checksum && P.b.object_checksum && std::memcmp(P.a.object_checksum, P.b.object_checksum, 32) == 0) ||
            same_chunks(P.a, P.b)) {
            S.skipped = true;
            ++X.st.skipped_pairs;
            continue;
        }
        for (int s = 0; s < 2 && S.status == CDC_OK; ++s) {
            const cdc_check_file &F = s ? P.b : P.a;
            S.blob[s].resize(size_t(F.nchunks));
            const int64_t miss = cdc::resolve(R->src.loc, F.checksums, F.nchunks, S.blob[s].data());
            if (miss >= 0) X.fail(i, CDC_E_NOTFOUND, s, miss);
            for (uint64_t c = 0; c < F.nchunks && miss < 0; ++c) S.size[s] += F.lengths[c];
        }
        if (S.status == CDC_OK && S.size[0] + S.size[1] > R->o.batch_bytes) X.fail(i, CDC_E_NOSPACE, -1, -1);
        if (S.status != CDC_OK) continue;
        for (int s = 0; s < 2; ++s)
            for (uint32_t id : S.blob[s])
                if (!used[id]) {
                    used[id] = true;
                    ++X.st.distinct_blobs;
                }
        if (!members.empty() && bytes + S.size[0] + S.size[1] > R->o.batch_bytes) flush();
        members.push_back(i);
        bytes += S.size[0] + S.size[1];
    }
    flush();
    // the pairs no batch reported: skipped ones, those that failed before a batch, and those of a run that broke off
    for (int i = 0; i < n; ++i) {
        if (X.reported[size_t(i)]) continue;
        PairState &S = X.ps[size_t(i)];
        if (S.skipped) {
            X.report(i, true, 0, 0, 0, nullptr, 0);
            continue;
        }
        if (S.status == CDC_OK) S.status = fail != CDC_OK ? fail : CDC_E_DEVICE;
        X.report(i, false, 0, 0, 0, nullptr, 0);
    }
    X.st.wall_s = since(w0);
    write_stats(stats, X.st);
    return fail;
}

}  // namespace

extern "C" {

int cdc_diff_script(const uint32_t *a_ids, uint64_t na, const uint32_t *b_ids, uint64_t nb, int context, cdc_diff_op *ops,
                    uint64_t cap, uint64_t *nops)
{
    if ((na && !a_ids) || (nb && !b_ids) || context < 0 || na >= 0xFFFFFFFFull || nb >= 0xFFFFFFFFull || (cap && !ops))
        return CDC_E_INVALID;
    try {
        const std::vector<cdc_diff_op> v = dplan::script(a_ids, size_t(na), b_ids, size_t(nb), uint32_t(context));
        if (nops) *nops = v.size();
        if (v.size() > cap) return CDC_E_NOSPACE;
        if (!v.empty()) std::memcpy(ops, v.data(), v.size() * sizeof(cdc_diff_op));
        return CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_diff_emit_plan(const cdc_diff_op *ops, uint64_t nops, const cdc_line_rec *a_lines, uint64_t na,
                       const cdc_line_rec *b_lines, uint64_t nb, const char *from_name, const char *to_name, uint64_t dst_base,
                       uint64_t lit_base, cdc_emit_rec *recs, uint64_t rec_cap, uint8_t *lit, uint64_t lit_cap, uint64_t *nrecs,
                       uint64_t *lit_bytes, uint64_t *out_bytes)
{
    if ((nops && !ops) || (na && !a_lines) || (nb && !b_lines) || (rec_cap && !recs) || (lit_cap && !lit)) return CDC_E_INVALID;
    for (uint64_t k = 0; k < nops; ++k) {
        const cdc_diff_op &c = ops[k];
        if (c.tag > CDC_DIFF_INSERT || c.i1 > c.i2 || c.i2 > na || c.j1 > c.j2 || c.j2 > nb || (k && c.group < ops[k - 1].group))
            return CDC_E_INVALID;
    }
    try {
        dplan::Plan P;
        dplan::emit_plan(ops, size_t(nops), a_lines, b_lines, from_name, to_name, dst_base, lit_base, P);
        if (nrecs) *nrecs = P.recs.size();
        if (lit_bytes) *lit_bytes = P.lit.size();
        if (out_bytes) *out_bytes = P.out_bytes;
        if (P.recs.size() > rec_cap || P.lit.size() > lit_cap) return CDC_E_NOSPACE;
        if (!P.recs.empty()) std::memcpy(recs, P.recs.data(), P.recs.size() * sizeof(cdc_emit_rec));
        if (!P.lit.empty()) std::memcpy(lit, P.lit.data(), P.lit.size());
        return CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_diff_default_opts(cdc_diff_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
}

int cdc_diff_new(int device, const cdc_diff_opts *opts, cdc_diff **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts) || device < 0 || device >= cdc::kMaxDevices || opts->threads < 0 ||
        opts->threads > 256 || opts->context < 0 || opts->batch_bytes > kMaxBatch || opts->max_lines > kMaxLines ||
        opts->hash_bits < 0 || opts->hash_bits > 128 ||
        (opts->compress != CDC_COMPRESS_NONE && opts->compress != CDC_COMPRESS_LZ4 && opts->compress != CDC_COMPRESS_GZIP))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *c = new (std::nothrow) cdc_diff();
    if (!c) return CDC_E_NOMEM;
    try {
        c->src.open(device, opts->compress, opts->key);
        c->o = *opts;
        c->o.key = nullptr;
        if (!c->o.context) c->o.context = 3;
        if (!c->o.threads) c->o.threads = 8;
        if (!c->o.batch_bytes) c->o.batch_bytes = 256ull << 20;
        if (!c->o.max_lines) c->o.max_lines = 16ull << 20;
    } catch (...) {
        delete c;
        return CDC_E_NOMEM;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->stream = nullptr;
        cdc_diff_free(c);
        return CDC_E_DEVICE;
    }
    *out = c;
    return CDC_OK;
}

int cdc_diff_add_packfile(cdc_diff *d, const uint8_t *bytes, uint64_t len)
{
    return d && (bytes || !len) ? d->src.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_diff_add_packfile_path(cdc_diff *d, const char *path)
{
    return d && path ? d->src.add_path(path) : CDC_E_INVALID;
}

int cdc_diff_add_packfiles(cdc_diff *d, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return d ? d->src.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_diff_files(cdc_diff *d, const cdc_diff_pair *pairs, int n, cdc_diff_pair_fn on_pair, void *ctx, cdc_diff_stats *stats)
{
    if (!d || n < 0 || (n && !pairs) || (stats && stats->struct_size < 8)) return CDC_E_INVALID;
    for (int i = 0; i < n; ++i)
        for (const cdc_check_file *f : {&pairs[i].a, &pairs[i].b})
            if (f->nchunks && (!f->checksums || !f->lengths)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(d->src.run_mu);
    try {
        return run_pairs(d, pairs, n, on_pair, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_diff_free(cdc_diff *d)
{
    if (!d) return;
    d->src.release(&d->stream, 1);
    delete d;
}

}  // extern "C"
