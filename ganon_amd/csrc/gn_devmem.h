// gn_devmem.h -- the owners of device memory (GnDev) and of pinned host memory (GnPinned).
// Every buffer a handle struct or a function of the library allocates is a member or a local of one of these two types: the
// destructor frees it, so no handle keeps a list of what it has to free.  (gn_pinned_alloc / gn_pinned_free hand memory to the
// caller through the C ABI and are the one exception.)  Both types convert to T*, so kernel launches, pointer arithmetic and
// `if (s->d_x)` read as with raw pointers; templated pointer parameters (hipcub) take .get().
// The destructor frees on the current device's context: whoever destroys a handle sets the handle's device first.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

template <typename T>
class GnDev
{
    T*     p_ = nullptr;
    size_t n_ = 0; // elements allocated

public:
    GnDev() = default;
    GnDev(GnDev&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    GnDev& operator=(GnDev&& o) noexcept
    {
        if (this != &o)
        {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~GnDev() { reset(); }

    // hipFree waits for the device: a buffer is never freed under a kernel that still uses it
    void reset()
    {
        if (p_)
            (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    // max(n, 1) elements; what the object held is freed first.  Empty with capacity 0 on failure.
    hipError_t alloc(size_t n)
    {
        reset();
        n = n ? n : 1;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
        if (e != hipSuccess)
            p_ = nullptr;
        else
            n_ = n;
        return e;
    }
    // room for `need` elements: nothing happens when there is a buffer and they fit, else the buffer is freed and `grown`
    // (>= need) elements are allocated; the contents are not kept
    hipError_t reserve(size_t need, size_t grown) { return p_ && need <= n_ ? hipSuccess : alloc(grown > need ? grown : need); }
    // allocate n elements and copy them from the host (blocking)
    hipError_t upload(const T* host, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess || n == 0 ? e : hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice);
    }

    T*     get() const { return p_; }
    size_t cap() const { return n_; }
    operator T*() const { return p_; }
};

template <typename T>
class GnPinned
{
    T* p_ = nullptr;

public:
    GnPinned() = default;
    GnPinned(GnPinned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    GnPinned& operator=(GnPinned&& o) noexcept
    {
        if (this != &o)
        {
            reset();
            p_   = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~GnPinned() { reset(); }

    void reset()
    {
        if (p_)
            (void)hipHostFree(p_);
        p_ = nullptr;
    }
    hipError_t alloc(size_t n)
    {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), (n ? n : 1) * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess)
            p_ = nullptr;
        return e;
    }

    T* get() const { return p_; }
    T* operator->() const { return p_; }
    operator T*() const { return p_; }
};

// the two streams of an insert that uploads one staging chunk under the kernel of the one before (gn_filter_emplace_runs_window,
// gn_filter_emplace_path_window); destroyed with the call
struct GnStreamPair
{
    hipStream_t st[2] = { nullptr, nullptr };
    GnStreamPair() = default;
    GnStreamPair(const GnStreamPair&) = delete;
    GnStreamPair& operator=(const GnStreamPair&) = delete;
    ~GnStreamPair()
    {
        for (hipStream_t s : st)
            if (s)
                (void)hipStreamDestroy(s);
    }
};

static_assert(!std::is_copy_constructible<GnDev<int>>::value && !std::is_copy_assignable<GnDev<int>>::value, "GnDev owns its allocation");
static_assert(!std::is_copy_constructible<GnPinned<int>>::value && !std::is_copy_assignable<GnPinned<int>>::value, "GnPinned owns its allocation");
