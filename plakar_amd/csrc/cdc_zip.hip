// cdc_zip_pieces_device: many raw DEFLATE streams in one call, the deflate
// pass of archive's zip format (include/plakar_cdc.h).
//
// Kernels, in launch order (one call = n pieces of one device buffer):
//   k_lz4_seq     cdc_encode.hip's, unchanged: the match search per 8-KiB segment
//                 (k_lz_seq_wide at CDC_LEVEL_WIDE: a piece's segments may copy
//                 from up to 32 KiB before them inside the piece)
//   k_dfl_size    cdc_encode.hip's, unchanged: per 32-KiB span its size as fixed
//                 and as dynamic Huffman, the dynamic header, its CRC-32
//   k_zip_plan    one wave per piece: each span's form at its bit from bit 0,
//                 the piece's deflate bytes, the descriptor's form
//   k_zip_place   one workgroup: the exclusive scan of the pieces' output
//                 bytes, the total against out_cap
//   k_dfl_emit    cdc_encode.hip's, unchanged: a workgroup per span, its block
//   k_zip_fin     one wave per piece: local header, shared bytes, the stream's
//                 end, the CRC-32 register, the data descriptor
//
// This is a translation unit of its own so that cdc_encode.hip's code object
// stays what it was: with these kernels at the end of cdc_encode.hip every
// older kernel kept its instructions but lay 2,304 bytes further into the
// code object (the metadata in front of the text grew), whatever the source
// position.  The shared kernels are launched through the
// host stubs cdc_encode_dev.h declares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>

#include "cdc_internal.h"
#include "cdc_encode_dev.h"
#include "cdc_hostmem.h"
#include "deflate_enc.h"
#include "inflate_walk.h"

namespace enc {

// ---------------------------------------------------------------------------
// Every piece is one blob of a GZIP batch (cdc_encode.hip's k_lz4_seq,
// k_dfl_size and k_dfl_emit run unchanged; a last piece's last span is marked
// last, so its block carries BFINAL), and these three kernels stand in the
// place of k_enc_plan and k_gz_fin.
// ---------------------------------------------------------------------------
struct ZipArgs {
    const cdc_zip_piece *pc;  // n
    cdc_zip_piece_out *res;   // n
    const uint8_t *hdrs;      // the local headers' arena
    uint64_t *tot;            // [0]: the sum of the pieces' output bytes
};

constexpr uint32_t kDescSig = 0x08074B50u;  // 50 4b 07 08

// One wave per piece: k_gzs_plan's chain over the piece's spans from bit 0,
// then the piece's deflate bytes, the descriptor's form and its output bytes.
__global__ __launch_bounds__(64) void k_zip_plan(const Batch B, const ZipArgs A)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const uint32_t b0 = B.blob_span0[b], n = B.blob_span0[b + 1] - b0;
    uint64_t P = 0;
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t sp = b0 + s0 + lane;
        const bool in = s0 + lane < n;
        const uint32_t len = in ? B.spans[sp].len : 0u;
        const uint32_t fb = in ? B.sp[sp].fixed_bits : 0u, db = in ? B.sp[sp].dyn_bits : 0u;
        uint32_t ty = 0, nb = 0;
        uint64_t at = 0;
        const uint32_t cnt = min(64u, n - s0);
        for (uint32_t j = 0; j < cnt; ++j) {
            uint64_t bits;
            const uint32_t t = dfl::choose_block(P, uint32_t(__shfl(int(len), int(j))), uint32_t(__shfl(int(fb), int(j))),
                                                 uint32_t(__shfl(int(db), int(j))), bits);
            if (lane == j) {
                ty = t;
                nb = uint32_t(bits);
                at = P;
            }
            P += bits;
        }
        if (in) {
            SpanOut &o = B.sp[sp];
            o.type = ty;
            o.nbits = nb;
            o.bit = at;
        }
    }
    if (lane == 0) {
        const cdc_zip_piece pc = A.pc[b];
        // last: to the next byte boundary (no spans: the final empty stored block);
        // not last: the joiner (no spans: nothing at all)
        const uint64_t D = pc.last ? (n ? (P + 7) >> 3 : uint64_t(dfl::kFinalBytes)) : (n ? (P + dfl::joiner_bits(P)) >> 3 : 0ull);
        const uint64_t cs = pc.csize_before + D, us = pc.usize_before + pc.len;
        const uint32_t z64 = pc.last && (cs >= 0xFFFFFFFFull || us >= 0xFFFFFFFFull) ? 1u : 0u;
        cdc_zip_piece_out r;
        r.out_off = 0;
        r.out_len = (pc.first ? pc.hdr_len : 0u) + D + (pc.last ? (z64 ? 24u : 16u) : 0u);
        r.deflate_len = D;
        r.crc_reg = 0;
        r.zip64 = z64;
        A.res[b] = r;
    }
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o)
{
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), o)), hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), o));
    return uint64_t(hi) << 32 | lo;
}

// One workgroup: the exclusive scan of the pieces' output bytes, tile by tile
// (as k_enc_plan scans blobs): where each piece and its deflate bytes start,
// the total and the verdict against out_cap.
constexpr uint32_t kZipPlaceThreads = 256;

__global__ __launch_bounds__(kZipPlaceThreads) void k_zip_place(const Batch B, const ZipArgs A)
{
    __shared__ uint64_t wsum[kZipPlaceThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint64_t base = 0;  // alike in every thread
    for (uint32_t i0 = 0; i0 < B.nblobs; i0 += kZipPlaceThreads) {
        const uint32_t i = i0 + t;
        const bool in = i < B.nblobs;
        const uint64_t v = in ? A.res[i].out_len : 0ull;
        uint64_t x = v;  // inclusive over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = shfl_up64(x, o);
            if (lane >= uint32_t(o)) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint64_t pre = 0, tile = 0;
        for (uint32_t k = 0; k < kZipPlaceThreads / 64; ++k) {
            if (k < w) pre += wsum[k];
            tile += wsum[k];
        }
        if (in) {
            const uint64_t off = base + pre + x - v;
            A.res[i].out_off = off;
            B.out_off[i] = off + (A.pc[i].first ? A.pc[i].hdr_len : 0u);  // k_dfl_emit's frame_ptr: the deflate bytes
        }
        base += tile;
        __syncthreads();
    }
    if (t == 0) {
        A.tot[0] = base;
        A.tot[1] = 0;
        B.status[0] = base > B.out_cap ? uint64_t(uint32_t(CDC_E_NOSPACE)) : 0ull;
        B.status[1] = 0;
    }
}

// One wave per piece: the local header (first piece), the bytes two spans'
// blocks share, the stream's end (last: the final block's last byte, or the
// whole empty block of an entry with no bytes; else the joiner), the piece's
// CRC-32 register and, on a last piece, the data descriptor.
__global__ __launch_bounds__(64) void k_zip_fin(const Batch B, const ZipArgs A)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (B.status[0]) return;
    const cdc_zip_piece pc = A.pc[b];
    const uint64_t out_off = A.res[b].out_off, D = A.res[b].deflate_len;
    const uint32_t z64 = A.res[b].zip64;
    uint8_t *f = B.out + B.out_off[b];
    if (pc.first) {
        uint8_t *h = B.out + out_off;
        for (uint32_t i = lane; i < pc.hdr_len; i += 64) h[i] = A.hdrs[pc.hdr_off + i];
    }
    const uint64_t len = pc.len;
    const uint32_t s0 = B.blob_span0[b], n = B.blob_span0[b + 1] - s0;  // 0: an empty piece
    uint32_t acc = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const SpanOut &o = B.sp[s0 + k];
        const uint64_t done = min<uint64_t>(len, uint64_t(k + 1) * dfl::kSpan);
        acc ^= infw::crc_mul(o.crc, infw::crc_shift(len - done));
        if (k && (o.bit & 7u)) f[o.bit >> 3] = uint8_t(B.sp[s0 + k - 1].edge_hi | o.edge_lo);
    }
    for (int o = 32; o; o >>= 1) acc ^= __shfl_xor(acc, o);
    if (lane == 0) {
        if (n) {
            const SpanOut &o = B.sp[s0 + n - 1];
            const uint64_t E = o.bit + o.nbits;
            if (!pc.last) dfl::stream_end(f + (E >> 3), o.edge_hi, uint32_t(E & 7u), false);
            else if (E & 7u) f[E >> 3] = uint8_t(o.edge_hi);
        } else if (pc.last) {
            f[0] = 1;
            f[1] = f[2] = 0;
            f[3] = f[4] = 0xFF;
        }
        if (pc.last) {
            const uint32_t crc = ~(acc ^ infw::crc_mul(pc.crc_reg, infw::crc_shift(len)));
            const uint64_t cs = pc.csize_before + D, us = pc.usize_before + len;
            uint8_t *e = f + D;
            for (int i = 0; i < 4; ++i) {
                e[i] = uint8_t(kDescSig >> (8 * i));
                e[4 + i] = uint8_t(crc >> (8 * i));
            }
            const int w = z64 ? 8 : 4;
            for (int i = 0; i < w; ++i) {
                e[8 + i] = uint8_t(cs >> (8 * i));
                e[8 + w + i] = uint8_t(us >> (8 * i));
            }
        }
        A.res[b].crc_reg = acc;
    }
}

// ---------------------------------------------------------------------------
// Many raw DEFLATE streams in one call (see include/plakar_cdc.h).  The
// workspace is the zip path's own, one per device, so it shares nothing with
// cdc_encode_device's or a gzip stream's; a call holds its device's lock.
// ---------------------------------------------------------------------------
struct ZipWs {
    std::mutex mu;
    cdc::DevBuf ws;
    cdc::PinBuf stage;
};
static ZipWs *const g_zip_ws = new ZipWs[cdc::kMaxDevices];  // never destroyed (DevBuf)

}  // namespace enc

using namespace enc;

extern "C" int cdc_zip_pieces_device(int device, const void *d_src, uint64_t src_cap, const cdc_zip_piece *pieces, uint32_t n,
                                     const uint8_t *hdr_arena, uint64_t hdr_arena_len, uint8_t *d_out, uint64_t out_cap,
                                     cdc_zip_piece_out *outs, uint64_t *total, void *stream)
{
    return cdc_zip_pieces_device_level(device, d_src, src_cap, pieces, n, hdr_arena, hdr_arena_len, d_out, out_cap, outs,
                                       total, CDC_LEVEL_FAST, stream);
}

extern "C" int cdc_zip_pieces_device_level(int device, const void *d_src, uint64_t src_cap, const cdc_zip_piece *pieces,
                                           uint32_t n, const uint8_t *hdr_arena, uint64_t hdr_arena_len, uint8_t *d_out,
                                           uint64_t out_cap, cdc_zip_piece_out *outs, uint64_t *total, int level,
                                           void *stream)
{
    if (!cdc::level_ok(level)) return CDC_E_INVALID;
    if (!total || (n && (!pieces || !outs))) return CDC_E_INVALID;
    *total = 0;
    if (device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    uint64_t ng64 = 0, nsp64 = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const cdc_zip_piece &p = pieces[b];
        if (p.len > dfl::kMaxBlob) return CDC_E_UNSUPPORTED;  // a piece's bit positions and spans are planned like a blob's
        if (p.len && (!d_src || p.src_off > src_cap || p.len > src_cap - p.src_off)) return CDC_E_INVALID;
        if (p.first && (!p.hdr_len || !hdr_arena || p.hdr_off > hdr_arena_len || p.hdr_len > hdr_arena_len - p.hdr_off))
            return CDC_E_INVALID;
        const uint64_t nblk = (p.len + kBlockLZ - 1) / kBlockLZ;
        if (nblk) ng64 += (nblk - 1) * (kBlockLZ / kSegLZ) + (p.len - (nblk - 1) * kBlockLZ + kSegLZ - 1) / kSegLZ;
        nsp64 += (p.len + dfl::kSpan - 1) / dfl::kSpan;
    }
    if (ng64 > 0x7FFFFFFFull || nsp64 > 0x7FFFFFFFull) return CDC_E_UNSUPPORTED;
    if (!n) return CDC_OK;
    if (!d_out) return CDC_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t nb = n, ng = size_t(ng64), nsp = size_t(nsp64);
    cdc::Carver cv(16);
    const size_t o_blobs = cv.take(nb * sizeof(BlobDesc)), o_segs = cv.take(ng * sizeof(Seg)),
                 o_spans = cv.take(nsp * sizeof(Span)), o_bsp = cv.take((nb + 1) * 4),
                 o_pc = cv.take(nb * sizeof(cdc_zip_piece)), o_hdrs = cv.take(size_t(hdr_arena_len));
    const size_t h_prefix = cv.bytes();
    const size_t o_recs = cv.take(ng * kRecCap * sizeof(uint2)), o_nrec = cv.take(ng * 4), o_trail = cv.take(ng * 4);
    const size_t o_oo = cv.take((nb + 1) * 8), o_status = cv.take(16), o_tot = cv.take(16);
    const size_t o_res = cv.take(nb * sizeof(cdc_zip_piece_out));
    const size_t o_sp = cv.take(nsp * sizeof(SpanOut)), o_splens = cv.take(nsp * kSpanLens),
                 o_sphdr = cv.take(nsp * dfl::kHdrWords * 4);
    ZipWs &C = g_zip_ws[device];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.ws.reserve(cv.bytes())) return CDC_E_DEVICE;
    if (!C.stage.reserve(h_prefix)) return CDC_E_NOMEM;
    uint8_t *const ws = C.ws.as<uint8_t>(), *const hp = C.stage.as<uint8_t>();
    {
        BlobDesc *blobs = reinterpret_cast<BlobDesc *>(hp + o_blobs);
        Seg *segs = reinterpret_cast<Seg *>(hp + o_segs);
        Span *spans = reinterpret_cast<Span *>(hp + o_spans);
        uint32_t *bsp = reinterpret_cast<uint32_t *>(hp + o_bsp);
        size_t kg = 0, ks = 0;
        for (uint32_t b = 0; b < n; ++b) {
            const cdc_zip_piece &p = pieces[b];
            const uint32_t nblk = uint32_t((p.len + kBlockLZ - 1) / kBlockLZ);
            BlobDesc D{};
            D.src = p.src_off;
            D.len = p.len;
            D.nblk = nblk;
            blobs[b] = D;
            bsp[b] = uint32_t(ks);
            for (uint32_t k = 0; k < nblk; ++k) {
                const uint64_t src = p.src_off + k * kBlockLZ;
                const uint32_t blen = uint32_t(std::min<uint64_t>(kBlockLZ, p.len - k * kBlockLZ));
                const uint32_t nseg = (blen + kSegLZ - 1) / kSegLZ;
                for (uint32_t g = 0; g < nseg; g += dfl::kSpanSegs) {
                    Span P{};
                    P.src = src + uint64_t(g) * kSegLZ;
                    P.len = std::min<uint32_t>(dfl::kSpan, blen - g * kSegLZ);
                    P.blob = b;
                    P.seg0 = uint32_t(kg + g);
                    P.nseg = std::min<uint32_t>(dfl::kSpanSegs, nseg - g);
                    P.k = uint32_t(ks) - bsp[b];
                    P.last = p.last && k + 1 == nblk && g + dfl::kSpanSegs >= nseg;  // the entry's final block
                    spans[ks++] = P;
                }
                for (uint32_t g = 0; g < nseg; ++g) {
                    Seg G{};
                    G.src = src + uint64_t(g) * kSegLZ;
                    G.len = std::min<uint32_t>(kSegLZ, blen - g * kSegLZ);
                    G.rem = blen - g * kSegLZ;
                    G.hist = seg_hist(level, g * kSegLZ);
                    segs[kg + g] = G;
                }
                kg += nseg;
            }
        }
        bsp[n] = uint32_t(ks);
        if (kg != ng || ks != nsp) return CDC_E_INVALID;  // the counts and the plan disagree (a bug)
        std::memcpy(hp + o_pc, pieces, nb * sizeof(cdc_zip_piece));
        if (hdr_arena_len) std::memcpy(hp + o_hdrs, hdr_arena, size_t(hdr_arena_len));
    }
    Batch Bt{};
    Bt.base = static_cast<const uint8_t *>(d_src);
    Bt.nblobs = n;
    Bt.nsegs = uint32_t(ng);
    Bt.compress = 2;
    Bt.blobs = reinterpret_cast<BlobDesc *>(ws + o_blobs);
    Bt.segs = reinterpret_cast<Seg *>(ws + o_segs);
    Bt.out = d_out;
    Bt.out_cap = out_cap;
    Bt.recs = reinterpret_cast<uint2 *>(ws + o_recs);
    Bt.nrec = reinterpret_cast<uint32_t *>(ws + o_nrec);
    Bt.trail = reinterpret_cast<uint32_t *>(ws + o_trail);
    Bt.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    Bt.status = reinterpret_cast<uint64_t *>(ws + o_status);
    Bt.nspans = uint32_t(nsp);
    Bt.spans = reinterpret_cast<Span *>(ws + o_spans);
    Bt.blob_span0 = reinterpret_cast<uint32_t *>(ws + o_bsp);
    Bt.sp = reinterpret_cast<SpanOut *>(ws + o_sp);
    Bt.sp_lens = ws + o_splens;
    Bt.sp_hdr = reinterpret_cast<uint32_t *>(ws + o_sphdr);
    ZipArgs A{};
    A.pc = reinterpret_cast<const cdc_zip_piece *>(ws + o_pc);
    A.res = reinterpret_cast<cdc_zip_piece_out *>(ws + o_res);
    A.hdrs = ws + o_hdrs;
    A.tot = reinterpret_cast<uint64_t *>(ws + o_tot);
    uint64_t back[4] = {0, 0, 0, 0};  // status[0..1], tot[0..1]: consecutive 16-byte regions
    bool ok = o_tot == o_status + 16 && hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        launch_seq(Bt, level, ng, s);
        if (nsp) hipLaunchKernelGGL(k_dfl_size, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
        hipLaunchKernelGGL(k_zip_plan, dim3(n), dim3(64), 0, s, Bt, A);
        hipLaunchKernelGGL(k_zip_place, dim3(1), dim3(kZipPlaceThreads), 0, s, Bt, A);
        if (nsp) hipLaunchKernelGGL(k_dfl_emit, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
        hipLaunchKernelGGL(k_zip_fin, dim3(n), dim3(64), 0, s, Bt, A);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(back, ws + o_status, sizeof(back), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(outs, ws + o_res, nb * sizeof(cdc_zip_piece_out), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) return CDC_E_DEVICE;
    *total = back[2];
    return back[0] ? int(int32_t(uint32_t(back[0]))) : CDC_OK;
}
