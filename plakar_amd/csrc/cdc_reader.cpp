// cdc_reader.h: the context core, the gather and the decode step of the runs
// that read blobs out of registered packfiles.
#include "cdc_reader.h"

#include <algorithm>

namespace cdc {

// ---- the context core ---------------------------------------------------------------
int PackSource::add_memory(const uint8_t *bytes, uint64_t len)
{
    std::lock_guard<std::mutex> lk(run_mu);
    try {
        return loc.add_memory(bytes, len);
    } catch (...) {
        return CDC_E_NOMEM;
    }
}

int PackSource::add_path(const char *path)
{
    std::lock_guard<std::mutex> lk(run_mu);
    try {
        return loc.add_path(path);
    } catch (...) {
        return CDC_E_NOMEM;
    }
}

int PackSource::add_many(const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    if (add_packfiles_invalid(srcs, n, status)) return CDC_E_INVALID;
    std::unique_lock<std::mutex> lk(run_mu, std::try_to_lock);
    if (!lk.owns_lock()) return CDC_E_INVALID;  // a run is in progress
    try {
        return add_packfiles(loc, stored, device, compress, key_ptr(), srcs, n, status);
    } catch (...) {
        return CDC_E_NOMEM;
    }
}

void PackSource::release(hipStream_t *streams, int n)
{
    if (std::any_of(streams, streams + n, [](hipStream_t s) { return s != nullptr; })) (void)hipSetDevice(device);
    for (int i = 0; i < n; ++i)
        if (streams[i]) {
            (void)hipStreamSynchronize(streams[i]);
            (void)hipStreamDestroy(streams[i]);
            streams[i] = nullptr;
        }
    if (!key.empty()) std::memset(key.data(), 0, key.size());
}

// ---- the gather ---------------------------------------------------------------------
int gather_read(const Locator &loc, Arena &A, int threads, uint64_t tail, double *read_s, uint64_t *encoded_bytes)
{
    const auto t0 = Clock::now();
    const size_t nb = A.spans.size();
    A.total = lay_out(A.spans.data(), nb, A.eoff, A.elen);
    A.pre.resize(nb);
    const bool room = A.h.reserve(tail ? align_up(A.total, 16) + tail : A.total) && A.d.reserve(A.total);
    read_spans(loc, A.spans.data(), nb, A.eoff.data(), room ? A.h.as<uint8_t>() : nullptr, threads, A.pre.data());
    if (!room) return CDC_E_NOMEM;
    *read_s += since(t0);
    if (encoded_bytes) *encoded_bytes += A.total;
    return CDC_OK;
}

int gather(const Locator &loc, Arena &A, int threads, hipStream_t stream, double *read_s, double *h2d_s,
           uint64_t *encoded_bytes)
{
    const int st = gather_read(loc, A, threads, 0, read_s, encoded_bytes);
    if (st != CDC_OK) return st;
    const auto t0 = Clock::now();
    if (A.total && (hipMemcpyAsync(A.d.data(), A.h.data(), A.total, hipMemcpyHostToDevice, stream) != hipSuccess ||
                    hipStreamSynchronize(stream) != hipSuccess))
        return CDC_E_DEVICE;
    *h2d_s += since(t0);
    return CDC_OK;
}

// ---- the decode step ----------------------------------------------------------------
static void fold_reads(const Arena &A, Decoded &D)
{
    for (size_t b = 0; b < A.pre.size(); ++b)
        if (A.pre[b] != CDC_OK) D.bst[b] = A.pre[b];
}

int decode_together(const DecodeCtx &C, Arena &A, uint8_t *dst, uint64_t cap, Decoded &D, const DecodeTally &T)
{
    const uint32_t nb = uint32_t(D.len.size());
    D.oo.assign(size_t(nb) + 1, 0);
    D.bst.assign(std::max<uint32_t>(nb, 1), CDC_OK);
    for (uint32_t b = 0; b < nb; ++b)
        if (A.pre[b] != CDC_OK) A.elen[b] = 0;  // never read: nothing of it goes through Decode
    const int st = decode_checked(C.device, A.d.data(), A.eoff.data(), A.elen.data(), nb, C.compress, C.key,
                                  C.verify ? D.want.data() : nullptr, dst, cap, D.oo.data(), D.bst.data(), C.stream, T.decode_s,
                                  T.verify_s);
    if (st != CDC_OK) return st;
    D.pos.assign(D.oo.begin(), D.oo.end() - 1);
    D.plain_used = D.oo[nb];
    for (uint32_t b = 0; b < nb; ++b)
        if (D.bst[b] == CDC_OK && D.oo[b + 1] - D.oo[b] != D.len[b]) D.bst[b] = CDC_E_MISMATCH;
    *T.decoded_bytes += D.oo[nb];
    fold_reads(A, D);
    return CDC_OK;
}

int decode_one_by_one(const DecodeCtx &C, Arena &A, uint8_t *dst, uint64_t plain_bytes, Decoded &D, const DecodeTally &T)
{
    const uint32_t nb = uint32_t(D.len.size());
    D.pos.assign(nb, 0);
    for (uint32_t b = 0; b < nb; ++b) {
        uint64_t o2[2] = {0, 0};
        const int st = decode_checked(C.device, A.d.data(), &A.eoff[b], &A.elen[b], 1, C.compress, C.key,
                                      C.verify ? &D.want[size_t(b) * 32] : nullptr, dst + D.off[b], D.len[b], o2, &D.bst[b],
                                      C.stream, T.decode_s, T.verify_s);
        if (st == CDC_E_NOSPACE) {
            D.bst[b] = CDC_E_MISMATCH;
            o2[1] = 0;
        } else if (st != CDC_OK) {
            return st;
        }
        D.pos[b] = D.off[b];
        if (D.bst[b] == CDC_OK && o2[1] != D.len[b]) D.bst[b] = CDC_E_MISMATCH;
        *T.decoded_bytes += o2[1];
    }
    D.plain_used = plain_bytes;
    fold_reads(A, D);
    return CDC_OK;
}

}  // namespace cdc
