// device_mem.h -- who owns the tracer library's device memory, streams, events and inter-process mappings (host code only).
//
// DevArray<T> is the one owner of a hipMalloc allocation: move-only, freed by reset() and by the destructor, and it converts to
// T * so that launch lines and copies read as with a bare pointer.  It does no pooling, no sub-allocation and no stream-ordered
// allocation: alloc() is one hipMalloc of count * sizeof(T) bytes, reset() one hipFree.  Nothing here waits for a stream:
// whoever resets an owner makes the streams that use its memory idle first; StreamDrain does that for the scratch memory of
// one call.
//
// DevHandle<H, Destroy> is the same for one HIP handle, destroyed by reset() and by the destructor; DevEvent, DevStream and
// IpcMapping are its three instantiations (an opened inter-process event is a DevEvent).  No pooling and no synchronisation
// either, and the same rule for all four owners: make the streams that use a handle -- or the stream itself -- idle, then reset.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace pol {

template <typename T>
class DevArray {
	T *p_ = nullptr;
	size_t cap_ = 0; // in elements
public:
	DevArray() = default;
	DevArray(const DevArray &) = delete;
	DevArray &operator=(const DevArray &) = delete;
	DevArray(DevArray &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	DevArray &operator=(DevArray &&o) noexcept {
		if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	~DevArray() { reset(); }

	void reset() {
		if (p_) (void)hipFree(p_);
		p_ = nullptr;
		cap_ = 0;
	}
	// `count` elements in place of whatever was held (freed first; empty after a failure).
	hipError_t alloc(size_t count) {
		reset();
		const hipError_t e = hipMalloc((void **)&p_, count * sizeof(T));
		if (e == hipSuccess) cap_ = count;
		else p_ = nullptr;
		return e;
	}
	// Grow only: at least `count` elements; the contents do not survive growing.
	hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : alloc(count); }

	size_t capacity() const { return cap_; }
	T *get() const { return p_; }
	operator T *() const { return p_; }
};

template <typename H, hipError_t (*Destroy)(H)>
class DevHandle {
	H h_ = nullptr;
public:
	DevHandle() = default;
	DevHandle(const DevHandle &) = delete;
	DevHandle &operator=(const DevHandle &) = delete;
	DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
	DevHandle &operator=(DevHandle &&o) noexcept {
		if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
		return *this;
	}
	~DevHandle() { reset(); }

	void reset() {
		if (h_) (void)Destroy(h_);
		h_ = nullptr;
	}
	// What make(&handle, args...) creates, in place of whatever was held (destroyed first; empty after a failure):
	// ev.create(hipEventCreateWithFlags, hipEventDisableTiming).
	template <typename... P, typename... A>
	hipError_t create(hipError_t (*make)(H *, P...), A &&...a) {
		reset();
		H x = nullptr;
		const hipError_t e = make(&x, static_cast<A &&>(a)...);
		if (e == hipSuccess) h_ = x;
		return e;
	}

	H get() const { return h_; }
	operator H() const { return h_; }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;
using IpcMapping = DevHandle<void *, hipIpcCloseMemHandle>;

// Declared AFTER the owners of a call's scratch memory, so that on every way out of the scope -- early returns included -- the
// stream is drained before that memory is freed (and before host buffers an asynchronous copy still writes go away).
struct StreamDrain {
	hipStream_t q;
	~StreamDrain() { (void)hipStreamSynchronize(q); }
};

} // namespace pol
