// device_mem.h -- who owns the tracer library's device memory (host code only).
//
// DevArray<T> is the one owner of a hipMalloc allocation: move-only, freed by reset() and by the destructor, and it converts to
// T * so that launch lines and copies read as with a bare pointer.  It does no pooling, no sub-allocation and no stream-ordered
// allocation: alloc() is one hipMalloc of count * sizeof(T) bytes, reset() one hipFree.  Nothing here waits for a stream:
// whoever resets an owner makes the streams that use its memory idle first; StreamDrain does that for the scratch memory of
// one call.
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

// Declared AFTER the owners of a call's scratch memory, so that on every way out of the scope -- early returns included -- the
// stream is drained before that memory is freed (and before host buffers an asynchronous copy still writes go away).
struct StreamDrain {
	hipStream_t q;
	~StreamDrain() { (void)hipStreamSynchronize(q); }
};

} // namespace pol
