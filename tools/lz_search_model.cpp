// A host model of the level-1 and level-9 match searches (k_lz_seq_wide and
// k_lz_seq_deep in plakar_amd/csrc/cdc_encode.hip): the kernels' steps lane by
// lane over one file of at most 4 MiB (one LZ4 block), the records sized as a
// gzip member by deflate_enc.h and as an LZ4 frame.  It is how a table shape or
// a parse rule is sized before it is built; on the two sets of
// tests/test_encode_best.py it gives the device's gzip byte counts at level 9
// and comes within 0.1 % of them at level 1 and for LZ4.
//
//   g++ -O2 -std=c++17 -o lz_search_model tools/lz_search_model.cpp
//   lz_search_model FILE WAYS BUCKET_BITS LAZY LAZY_MAX [WEIGHT]
//     WAYS 1: k_lz_seq_wide (BUCKET_BITS 14); WAYS 4, BUCKET_BITS 12, LAZY 2,
//     LAZY_MAX 128: k_lz_seq_deep.  LAZY 0: no look, 1: one look, 2: repeated.
//     WEIGHT w > 0: the ways and the look compare length * w - log2(distance).
//     DUMP_FROM=N in the environment prints the records from byte N on.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <array>
#include <memory>
#include <vector>
#include "../plakar_amd/csrc/deflate_enc.h"
using namespace std;
typedef vector<uint8_t> Bytes;
static const uint32_t SEG = 8192, HIST = 32768;
struct Cfg { int ways, bits, lazy /*0 none,1 once,2 repeat*/, lazymax; };

static uint32_t rd32(const uint8_t *d, uint32_t p) { uint32_t v; memcpy(&v, d + p, 4); return v; }
struct Hit { uint32_t len, c; };
static int WGT = 0;
static int ilog2(uint32_t x){return 31-__builtin_clz(x);}
static int score(uint32_t len,uint32_t dist){ return WGT ? int(len)*WGT - ilog2(dist) : int(len)*64; }

struct Tab {
    int ways, bits;
    vector<uint16_t> t;
    Tab(int w, int b) : ways(w), bits(b), t(size_t(w) << b, 0) {}
    uint32_t hash(uint32_t v) const { return (v * 2654435761u) >> (32 - bits); }
    void get(uint32_t h, uint16_t *o) const { memcpy(o, &t[size_t(h) * ways], 2 * ways); }
    void put_shift(uint32_t h, const uint16_t *old, uint32_t pos1) {
        uint16_t *b = &t[size_t(h) * ways];
        for (int w = ways - 1; w > 0; --w) b[w] = old[w - 1];
        b[0] = uint16_t(pos1);
    }
};

static Hit measure(const uint8_t *d, uint32_t P, const uint16_t *b, int ways, uint32_t end_lim)
{
    Hit best{0, 0};
    for (int w = 0; w < ways; ++w) {
        uint32_t cand = b[w];
        if (!cand) continue;
        uint32_t c = cand - 1;
        if (!(c < P && P - c <= HIST)) continue;
        uint32_t len = 0;
        while (P + len < end_lim && d[P + len] == d[c + len]) ++len;
        if (len >= 4 && (best.len == 0 || score(len,P-c) > score(best.len,P-best.c) || (score(len,P-c) == score(best.len,P-best.c) && c > best.c))) best = Hit{len, c};
    }
    return best;
}

static void seg_search(const uint8_t *win, uint32_t hist, uint32_t n, uint32_t rem, const Cfg &C, vector<dfl::Rec> &out)
{
    const uint32_t W = hist + n;
    vector<uint8_t> dv(W + 80, 0);
    memcpy(dv.data(), win, W);
    const uint8_t *d = dv.data();
    Tab T(C.ways, C.bits);
    const int WAYS = C.ways;
    uint16_t old[64][8];
    uint32_t hh[64];
    const uint32_t hstep = C.ways == 1 ? 256 : 64;  // k_lz_seq_wide enters four positions per lane and step
    for (uint32_t j0 = 0; j0 < hist; j0 += hstep) {
        // one step: every lane reads its bucket, then every lane writes (the last write to a bucket stays)
        vector<array<uint16_t, 8>> olds(hstep);
        vector<uint32_t> hs(hstep);
        for (uint32_t k = 0; k < hstep; ++k) { hs[k] = T.hash(rd32(d, j0 + k)); T.get(hs[k], olds[k].data()); }
        for (uint32_t k = 0; k < hstep; ++k) T.put_shift(hs[k], olds[k].data(), j0 + k + 1);
    }
    const uint32_t start_lim = hist + min(n >= 4 ? n - 3 : 0u, rem > 12 ? rem - 12 : 0u);
    const uint32_t end_lim = hist + min(n, rem > 5 ? rem - 5 : 0u);
    const uint32_t s_lim = start_lim, e_lim = end_lim;
    uint32_t cursor = hist, anchor = hist;
    while (cursor < s_lim) {
        const uint32_t stride = 1 + ((cursor - anchor) >> 6);
        int f = -1;
        bool valid[64];
        uint32_t pp[64];
        for (int l = 0; l < 64; ++l) {
            uint32_t p = cursor + l * stride;
            pp[l] = p;
            valid[l] = p < s_lim;
            if (!valid[l]) continue;
            uint32_t v = rd32(d, p);
            hh[l] = T.hash(v);
            T.get(hh[l], old[l]);
            bool ok = false;
            for (int w = 0; w < WAYS; ++w) {
                uint32_t cand = old[l][w], c = cand - 1;
                ok = ok || (cand && c < p && p - c <= HIST && rd32(d, c) == v);
            }
            if (ok && f < 0) f = l;
        }
        if (f < 0) {
            for (int l = 0; l < 64; ++l) if (valid[l]) T.put_shift(hh[l], old[l], pp[l] + 1);
            cursor += 64 * stride;
            continue;
        }
        uint32_t q = pp[f];
        Hit h;
        if (C.ways == 1) { h.c = old[f][0] - 1; h.len = 4; }  // level 1: first verified, extend later
        else h = measure(d, q, old[f], WAYS, e_lim);
        uint32_t cq = h.c, len = h.len;
        auto back = [&]() {
            uint32_t moved = 0;
            while (q > anchor && cq > 0 && d[q - 1] == d[cq - 1]) { --q; --cq; ++len; ++moved; }
            return moved;
        };
        if (C.ways == 1) {
            back();
            while (q + len < e_lim && d[q + len] == d[cq + len]) ++len;
        } else {
            for (bool looked = false;; looked = true) {
                uint32_t moved = back();
                if (moved || looked) break;
                bool took = false;
                while (C.lazy && len < (uint32_t)C.lazymax && q + 1 < s_lim) {
                    uint16_t b1[8];
                    T.get(T.hash(rd32(d, q + 1)), b1);
                    Hit nx = measure(d, q + 1, b1, WAYS, e_lim);
                    if (nx.len < 4 || score(nx.len, q + 1 - nx.c) <= score(len, q - cq)) break;
                    q += 1; cq = nx.c; len = nx.len; took = true;
                    if (C.lazy == 1) break;
                }
                if (!took) break;
            }
        }
        out.push_back(dfl::Rec{(q - hist) | ((q - cq) << 16), len});
        for (int l = 0; l < 64; ++l) if (valid[l] && pp[l] < q + len) T.put_shift(hh[l], old[l], pp[l] + 1);
        anchor = cursor = q + len;
    }
}

struct ByteRd { const uint8_t *p; uint32_t operator()(uint32_t i) const { return p[i]; } };

static uint64_t lz4_size(const Bytes &data, const vector<vector<dfl::Rec>> &recs)
{
    // one block (data <= 4 MiB): token + literal-length bytes + literals + 2 + matchlen bytes
    uint64_t out = 7 + 4 + 4;  // frame header, block header, end mark (approx.)
    uint64_t lit = 0;
    auto litbytes = [](uint64_t l) { return l >= 15 ? 1 + (l - 15) / 255 : 0; };
    for (size_t s = 0; s < recs.size(); ++s) {
        uint32_t pos = 0;
        for (auto &r : recs[s]) {
            uint32_t st = r.x & 0xFFFF, len = r.y;
            lit += st - pos;
            out += 1 + litbytes(lit) + lit + 2 + (len - 4 >= 15 ? 1 + (len - 4 - 15) / 255 : 0);
            lit = 0;
            pos = st + len;
        }
        uint32_t sl = uint32_t(min<uint64_t>(SEG, data.size() - s * SEG));
        lit += sl - pos;
    }
    out += 1 + litbytes(lit) + lit;
    return out;
}

static uint64_t gzip_size(const Bytes &data, const vector<vector<dfl::Rec>> &recs, const vector<uint32_t> &hist)
{
    using namespace dfl;
    Serial par;
    uint64_t P = 80;
    const uint64_t len = data.size();
    const uint32_t nspan = uint32_t((len + kSpan - 1) / kSpan);
    for (uint32_t sp = 0; sp < nspan; ++sp) {
        const uint32_t slen = uint32_t(min<uint64_t>(kSpan, len - uint64_t(sp) * kSpan));
        ByteRd rd{data.data() + uint64_t(sp) * kSpan};
        SpanView V{};
        V.len = slen;
        for (uint32_t g = 0; g < kSpanSegs; ++g) {
            size_t sg = size_t(sp) * kSpanSegs + g;
            V.rec[g] = sg < recs.size() ? recs[sg].data() : nullptr;
            V.nrec[g] = sg < recs.size() ? uint32_t(recs[sg].size()) : 0;
            V.hist[g] = sg < hist.size() ? hist[sg] : 0;
        }
        unique_ptr<uint32_t[]> lfreq(new uint32_t[kLitSlots]()), dfreq(new uint32_t[kDistSlots]());
        uint32_t xbits = 0;
        span_hist(par, V, rd, lfreq.get(), dfreq.get(), &xbits);
        unique_ptr<uint8_t[]> llen(new uint8_t[kNLit]), dlen(new uint8_t[kNDist]);
        unique_ptr<CodeWork> Wk(new CodeWork);
        unique_ptr<HdrWork> H(new HdrWork);
        build_lengths(par, lfreq.get(), kNLit, 15, llen.get(), *Wk);
        build_lengths(par, dfreq.get(), kNDist, 15, dlen.get(), *Wk);
        header_tokens(llen.get(), dlen.get(), *H);
        build_lengths(par, H->clfreq, kNCl, 7, H->cllen, *Wk);
        assign_codes(par, H->cllen, kNCl, H->clcode);
        unique_ptr<uint32_t[]> hw(new uint32_t[kHdrWords]());
        const uint32_t hdr_bits = write_header(*H, hw.get());
        const uint32_t dyn_bits = 3 + hdr_bits + body_bits(lfreq.get(), dfreq.get(), llen.get(), dlen.get(), xbits);
        const uint32_t fixed_bits = 3 + body_bits(lfreq.get(), dfreq.get(), nullptr, nullptr, xbits);
        uint64_t bits;
        choose_block(P, slen, fixed_bits, dyn_bits, bits);
        P += bits;
    }
    return (P + 7) / 8 + 8;
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        fprintf(stderr, "usage: %s FILE WAYS BUCKET_BITS LAZY LAZY_MAX [WEIGHT]\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    Bytes data;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + k);
    fclose(f);
    WGT = argc > 6 ? atoi(argv[6]) : 0;
    Cfg C{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
    const size_t nseg = (data.size() + SEG - 1) / SEG;
    vector<vector<dfl::Rec>> recs(nseg);
    vector<uint32_t> hist(nseg);
    uint64_t nrec = 0, mlen = 0;
    for (size_t s = 0; s < nseg; ++s) {
        uint32_t off = uint32_t(s * SEG);  // data <= 4 MiB: one block
        uint32_t h = min(off, HIST), n = uint32_t(min<uint64_t>(SEG, data.size() - off));
        hist[s] = h;
        seg_search(data.data() + off - h, h, n, uint32_t(data.size() - off), C, recs[s]);
        nrec += recs[s].size();
        if (getenv("DUMP_FROM")) for (auto &r : recs[s]) { uint32_t p = off + (r.x & 0xFFFF); if (p >= (uint32_t)atoi(getenv("DUMP_FROM"))) printf("  tok (%u, %u, %u)\n", p, r.y, r.x >> 16); }
        for (auto &r : recs[s]) mlen += r.y;
    }
    printf("ways %d bits %d lazy %d lazymax %d: gzip %llu lz4 %llu recs %llu avg len %.2f covered %.3f\n", C.ways, C.bits, C.lazy,
           C.lazymax, (unsigned long long)gzip_size(data, recs, hist), (unsigned long long)lz4_size(data, recs),
           (unsigned long long)nrec, double(mlen) / nrec, double(mlen) / data.size());
    return 0;
}
