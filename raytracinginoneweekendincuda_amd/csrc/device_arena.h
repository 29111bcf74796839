// device_arena.h -- the one owner of device memory on the host side (device_scene.cpp): a scene's tables, a film's planes, the
// scratch arrays of a call.  An arena remembers its device and frees on that device whatever it handed out when it goes away.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

namespace rtow {

class DeviceArena {
public:
    explicit DeviceArena(int device = -1) : device_(device) {}
    DeviceArena(DeviceArena &&other) noexcept : device_(other.device_), blocks_(std::move(other.blocks_)) { other.blocks_.clear(); }
    DeviceArena &operator=(DeviceArena &&other) noexcept
    {
        std::swap(device_, other.device_);  // what this arena held goes away with `other`
        blocks_.swap(other.blocks_);
        return *this;
    }
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena()
    {
        if (blocks_.empty()) return;
        int prev = 0;
        hipGetDevice(&prev);
        hipSetDevice(device_);
        for (void *p : blocks_) hipFree(p);
        hipSetDevice(prev);
    }

    // `count` elements on the current device, which the caller has made the arena's; never a null or empty allocation: every
    // table pointer stays valid so that speculative loads stay in bounds
    template <class T>
    hipError_t alloc(size_t count, T *&out)
    {
        out = nullptr;
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        blocks_.push_back(p);
        out = static_cast<T *>(p);
        return hipSuccess;
    }

    // a copy of host[0 .. count); of nothing: the single element, zeroed
    template <class T>
    hipError_t upload(const T *host, size_t count, const T *&out)
    {
        T *p = nullptr;
        hipError_t e = alloc(count, p);
        if (e == hipSuccess) e = count ? hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(p, 0, sizeof(T));
        out = e == hipSuccess ? p : nullptr;
        return e;
    }
    template <class T>
    hipError_t upload(const std::vector<T> &host, const T *&out)
    {
        return upload(host.data(), host.size(), out);
    }

private:
    int device_;
    std::vector<void *> blocks_;
};

}  // namespace rtow
