// device_owner.h -- who owns what numeric.hip (the only includer) takes from the HIP runtime: an arena of device buffers, pinned
// host buffers and events that frees all of them in clear() and in its destructor.  WHICH arena a resource is taken from decides
// when it dies (DESIGN.md "Ownership of device resources"); nothing is pooled, sub-allocated or counted.  A failed call is reported
// like everywhere in numeric.hip: `false`, and the call with HIP's message in the error string the arena was constructed with.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

namespace mi355x {

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    err_ = std::string(#call) + ": " + hipGetErrorString(e_); return false; } } while (0)      // (wants a std::string named err_ in scope: a member, or a local reference)

class DeviceOwner {
    std::string& err_;
    std::vector<void*> dev_, pin_;
    std::vector<hipEvent_t> ev_;
public:
    explicit DeviceOwner(std::string& err) : err_(err) {}
    DeviceOwner(const DeviceOwner&) = delete; DeviceOwner& operator=(const DeviceOwner&) = delete;
    ~DeviceOwner() { clear(); }
    bool empty() const { return dev_.empty() && pin_.empty() && ev_.empty(); }
    void clear() {
        for (void* p : dev_) (void)hipFree(p);
        for (void* p : pin_) (void)hipHostFree(p);
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
        dev_.clear(); pin_.clear(); ev_.clear();
    }
    // a device buffer of max(count, 1) elements, contents undefined
    template <class T> bool raw(T** d, size_t count) {
        void* p = nullptr; HIPCHK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T))); dev_.push_back(p);
        *d = (T*)p; return true;
    }
    // ... zero-filled.  hipMemset runs on the legacy default stream, which the solver's non-blocking streams are NOT ordered behind:
    // the caller synchronises the device once, behind its last allocation, before a kernel on such a stream may touch the buffer
    template <class T> bool zeroed(T** d, size_t count) {
        if (!raw(d, count)) return false;
        HIPCHK(hipMemset(*d, 0, std::max<size_t>(count, 1) * sizeof(T))); return true;
    }
    // ... holding a copy of `h`
    template <class T, class A> bool upload(const std::vector<T, A>& h, const T** d) {
        T* p = nullptr; if (!raw(&p, h.size())) return false;
        if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        *d = p; return true;
    }
    template <class T> bool pinned(T** h, size_t count) {
        void* p = nullptr; HIPCHK(hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault)); pin_.push_back(p);
        *h = (T*)p; return true;
    }
    void adopt_pinned(void* p) { pin_.push_back(p); }      // (a pinned buffer made before the arena existed)
    bool event(hipEvent_t* e, unsigned flags = hipEventDefault) { HIPCHK(hipEventCreateWithFlags(e, flags)); ev_.push_back(*e); return true; }
    // one device buffer ahead of the rest (a buffer that is replaced by a larger one); a pointer the arena does not own, null included: nothing happens
    void free_device(void* p) { auto it = std::find(dev_.begin(), dev_.end(), p); if (it != dev_.end()) { (void)hipFree(p); dev_.erase(it); } }
};

} // namespace mi355x
