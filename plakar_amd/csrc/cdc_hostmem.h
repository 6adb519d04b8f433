// Host-side memory plumbing shared by every stage: the workspace carver, the
// owning device/pinned buffers, and the per-device facts (how many devices the
// library keeps state for, a device's CU count, the AES table upload).
// Internal; host code only (no __device__ or __global__ entity).
#pragma once

#include <stddef.h>

namespace cdc {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Lays consecutive regions out in one allocation: take() returns the region's
// offset and advances to the next multiple of `align`; bytes() is the total.
class Carver {
public:
    explicit Carver(size_t align) : align_(align) {}
    size_t take(size_t bytes)
    {
        const size_t o = off_;
        off_ = align_up(off_ + bytes, align_);
        return o;
    }
    size_t bytes() const { return off_; }

private:
    size_t align_, off_ = 0;
};

}  // namespace cdc

// Everything above builds with a plain host compiler (tests/c/carve_check.cpp).
#ifndef CDC_HOSTMEM_NO_HIP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>

#include "cdc_internal.h"

namespace cdc {

constexpr int kMaxDevices = 64;  // devices the library keeps per-device state for

namespace detail {
struct DevAlloc {
    static bool alloc(void **p, size_t n) { return hipMalloc(p, n) == hipSuccess; }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinAlloc {
    static bool alloc(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault) == hipSuccess; }
    static void free(void *p) { (void)hipHostFree(p); }
};
}  // namespace detail

// Move-only owner of one grow-only allocation.  The destructor releases, so a
// buffer whose owner lives as long as the process (the per-device caches) sits
// in an array made with `new` and never destroyed, as host_pool()'s pools do:
// a free from a static destructor could run after the HIP runtime shut down.
template <class A>
class Buf {
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }

    // Room for `need` bytes: nothing when it is there, else the old allocation
    // goes (its contents with it) and max(need, alloc, 16) bytes come.  False,
    // and an empty buffer, when that allocation fails.  An empty buffer
    // allocates even for need = 0, so after a true data() is never null.
    bool reserve(size_t need, size_t alloc = 0)
    {
        if (p_ && need <= cap_) return true;
        release();
        const size_t n = std::max<size_t>({need, alloc, 16});
        if (!A::alloc(&p_, n)) {
            p_ = nullptr;
            return false;
        }
        cap_ = n;
        return true;
    }
    void release()
    {
        if (p_) A::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void *data() const { return p_; }
    template <class T>
    T *as() const
    {
        return static_cast<T *>(p_);
    }
    size_t cap() const { return cap_; }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};
using DevBuf = Buf<detail::DevAlloc>;  // hipMalloc
using PinBuf = Buf<detail::PinAlloc>;  // hipHostMalloc(Default)

// The device's CU count, read once per device; 256 when the query fails.
inline int device_cus(int device)
{
    static std::atomic<int> cache[kMaxDevices];
    const bool slot = device >= 0 && device < kMaxDevices;
    int n = slot ? cache[device].load(std::memory_order_relaxed) : 0;
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (slot) cache[device].store(n, std::memory_order_relaxed);
    return n;
}

// Uploads Te0 and the S-box to the caller's own __device__ copies on every
// device, once per translation unit (each .hip file owns a copy: there is no
// relocatable device code, and an AesTables of its own).
struct AesTables {
    std::once_flag once;
    int status = CDC_OK;
};
template <class Te0, class Sbox>
int upload_aes_tables(AesTables &T, Te0 &d_te0, Sbox &d_sbox)
{
    std::call_once(T.once, [&] {
        uint32_t te0[256];
        uint8_t sbox[256];
        enc::build_tables(te0, sbox);
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) {
            T.status = CDC_E_DEVICE;
            return;
        }
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (int d = 0; d < n; ++d) {
            if (hipSetDevice(d) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(d_te0), te0, sizeof(te0)) != hipSuccess ||
                hipMemcpyToSymbol(HIP_SYMBOL(d_sbox), sbox, sizeof(sbox)) != hipSuccess)
                T.status = CDC_E_DEVICE;
        }
        (void)hipSetDevice(cur);
    });
    return T.status;
}

}  // namespace cdc

#endif  // CDC_HOSTMEM_NO_HIP
