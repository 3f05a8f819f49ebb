// hip_buf.h -- owners of device and pinned host memory for the host side of the two engines (host code only).
//
// A buffer is freed by its destructor, by release(), or by whatever replaces it (alloc, reserve past the capacity, move assignment): nobody keeps a
// list of pointers to free.  hipFree synchronises the device, so an owner is released where the raw pointer was freed before -- with the engine's
// device current and before its streams are destroyed -- and never left to a destructor that runs later.
// The structs handed to kernels stay PODs of raw pointers, filled from the owners (implicit conversion to T*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

struct HipDeviceMem {
	template <class T> static hipError_t get(T** p, size_t bytes) { return hipMalloc(p, bytes); }
	static void put(void* p) { (void)hipFree(p); }
};
struct HipPinnedMem {
	template <class T> static hipError_t get(T** p, size_t bytes) { return hipHostMalloc(p, bytes); }
	static void put(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
struct HipBuf {
	T* p = nullptr;
	size_t n = 0;   // elements
	HipBuf() = default;
	HipBuf(const HipBuf&) = delete;
	HipBuf& operator=(const HipBuf&) = delete;
	HipBuf(HipBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
	HipBuf& operator=(HipBuf&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
	~HipBuf() { release(); }
	void release() { if (p) Mem::put(p); p = nullptr; n = 0; }
	void swap(HipBuf& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); }
	// exactly `count` elements; what the buffer held is gone
	hipError_t alloc(size_t count) {
		release();
		const hipError_t r = Mem::get(&p, sizeof(T) * count);
		if (r != hipSuccess) p = nullptr; else n = count;
		return r;
	}
	// grow only, to exactly the size asked (no doubling); contents are not kept
	hipError_t reserve(size_t count) { return count <= n ? hipSuccess : alloc(count); }
	operator T*() const { return p; }
};
template <class T> using DevBuf = HipBuf<T, HipDeviceMem>;
template <class T> using PinBuf = HipBuf<T, HipPinnedMem>;
