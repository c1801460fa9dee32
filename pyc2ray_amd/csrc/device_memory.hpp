// device_memory.hpp -- who owns the library's device and pinned host memory, and for how long.
//   Owned<T, lifetime, pinned>  a field of State (asora_internal.hpp): the pointer and the bytes it was allocated with.  It reads
//                               as the raw T * wherever one is expected.  Every instance enters a registry when it is
//                               constructed; release_all() (api.hip) frees the mesh-lifetime ones by walking it, so a new buffer
//                               is a new field and nothing else.  The destructor frees nothing: State is destroyed after main
//                               returns, when the HIP runtime may be gone.
//   Scoped<T>                   memory of one call: freed by the destructor on every exit path.
// A HIP error returns through fail(10, ...), as everywhere in the library.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

namespace asora {

int fail(int code, const std::string &msg);   // records the message, returns code

#define ASORA_HIP_TRY(expr)                                                                     \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return ::asora::fail(10, std::string(#expr) + ": " + hipGetErrorName(e__) + " - " + \
                                         hipGetErrorString(e__));                               \
    } while (0)

// mesh: released by device_close and by a re-initialising device_init; process: never released
enum Lifetime { LIFETIME_MESH = 0, LIFETIME_PROCESS = 1 };

class OwnedMemory {
public:
    OwnedMemory(const OwnedMemory &) = delete;
    OwnedMemory &operator=(const OwnedMemory &) = delete;
    size_t bytes() const { return bytes_; }
    int release()
    {
        void *q = ptr_;
        ptr_ = nullptr; bytes_ = 0;
        if (q) ASORA_HIP_TRY(pinned_ ? hipHostFree(q) : hipFree(q));
        return 0;
    }
    static void release_all_of(Lifetime life) { for (OwnedMemory *m : registry()) if (m->life_ == life) (void)m->release(); }
    static void live(Lifetime life, long long &buffers, unsigned long long &bytes)     // the non-empty ones, what they were allocated with
    {
        buffers = 0; bytes = 0;
        for (const OwnedMemory *m : registry()) if (m->life_ == life && m->ptr_) { buffers += 1; bytes += m->bytes_; }
    }

protected:
    OwnedMemory(Lifetime life, bool pinned) : life_(life), pinned_(pinned) { registry().push_back(this); }
    ~OwnedMemory() = default;
    // (a function-local static: complete before the first holder, whichever unit's statics are initialised first)
    static std::vector<OwnedMemory *> &registry() { static std::vector<OwnedMemory *> r; return r; }
    int allocate_bytes(size_t bytes)
    {
        if (ptr_) return 0;
        ASORA_HIP_TRY(pinned_ ? hipHostMalloc(&ptr_, bytes, hipHostMallocDefault) : hipMalloc(&ptr_, bytes));
        bytes_ = bytes;
        return 0;
    }
    int reserve_bytes(size_t bytes, hipStream_t drain)
    {
        if (bytes <= bytes_) return 0;
        if (drain) ASORA_HIP_TRY(hipStreamSynchronize(drain));
        if (int rc = release()) return rc;
        return allocate_bytes(bytes);
    }
    void *ptr_ = nullptr;
    size_t bytes_ = 0;
    const Lifetime life_;
    const bool pinned_;
};

template <typename T, Lifetime LIFE, bool PINNED = false> struct Owned : OwnedMemory {
    Owned() : OwnedMemory(LIFE, PINNED) {}
    operator T *() const { return static_cast<T *>(ptr_); }
    T *operator->() const { return static_cast<T *>(ptr_); }
    T *get() const { return static_cast<T *>(ptr_); }
    size_t count() const { return bytes_ / sizeof(T); }                 // elements there is room for
    int allocate(size_t n) { return allocate_bytes(n * sizeof(T)); }    // if empty; a buffer that is there keeps its size
    // room for at least n elements: freed and allocated anew when too small (the contents are lost).  drain: a stream whose
    // work may still use the old buffer, waited for before it is freed
    int reserve(size_t n, hipStream_t drain = nullptr) { return reserve_bytes(n * sizeof(T), drain); }
    void adopt(T *p, size_t bytes) { ptr_ = p; bytes_ = bytes; }        // an allocation made elsewhere (the arena; a Scoped's give())
};
template <typename T> using MeshBuffer = Owned<T, LIFETIME_MESH>;
template <typename T> using MeshPinned = Owned<T, LIFETIME_MESH, true>;
template <typename T> using ProcessBuffer = Owned<T, LIFETIME_PROCESS>;
template <typename T> using ProcessPinned = Owned<T, LIFETIME_PROCESS, true>;

// Device memory as a bare pointer, for the collections that keep lists of pointers and have release functions of their own (the
// geometry tables, the pair and dispatch-order lists of raytrace.hip)
template <typename T> int device_allocate(T *&p, size_t n) { ASORA_HIP_TRY(hipMalloc(&p, n * sizeof(T))); return 0; }

// Device memory of one call.  A count of 0 allocates one element, so that the pointer is never null.
template <typename T> class Scoped {
public:
    Scoped() = default;
    Scoped(const Scoped &) = delete;
    Scoped &operator=(const Scoped &) = delete;
    ~Scoped() { if (ptr_) (void)hipFree(ptr_); }
    int allocate(size_t n) { return device_allocate(ptr_, std::max<size_t>(n, 1)); }
    operator T *() const { return ptr_; }
    T *get() const { return ptr_; }
    T *give() { T *p = ptr_; ptr_ = nullptr; return p; }    // the caller owns it from here

private:
    T *ptr_ = nullptr;
};

} // namespace asora
