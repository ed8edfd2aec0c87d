// pxz_handle.h — owners of what a pxz_handle holds on the device and in pinned host memory (private to the host runtime: pxz_runtime.h).
// Each frees what it holds in its destructor and is move-only, so that a handle, a cache entry or the scratch part of
// a handle that is destroyed, evicted or replaced gives its memory back without anyone listing it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <utility>

namespace pxz {

// A grow-only device allocation: a scratch buffer of the handle, or the one allocation behind a table set.
struct DeviceBuffer {
	void *ptr = nullptr;
	size_t cap = 0;

	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
	DeviceBuffer &operator=(DeviceBuffer &&o) noexcept  // (what this one held goes with o)
	{
		std::swap(ptr, o.ptr);
		std::swap(cap, o.cap);
		return *this;
	}
	~DeviceBuffer() { release(); }

	void release()
	{
		if (ptr) (void)hipFree(ptr);
		ptr = nullptr;
		cap = 0;
	}
	// At least `bytes`: what is there is kept when it is large enough, and freed BEFORE the larger block is allocated
	// otherwise (the contents are scratch).  false: the allocation failed, and the buffer is empty (ptr null, cap 0).
	bool reserve(size_t bytes)
	{
		if (cap >= bytes) return true;
		release();
		if (hipMalloc(&ptr, bytes) != hipSuccess) {
			ptr = nullptr;
			return false;
		}
		cap = bytes;
		return true;
	}
};

// A pinned host block that small per-call tables go through on their way to the device, and the event behind the last
// copy out of it: the block is written again only once that copy has run.
struct PinnedStaging {
	void *host = nullptr;
	size_t cap = 0;
	hipEvent_t copied = nullptr;

	PinnedStaging() = default;
	PinnedStaging(PinnedStaging &&o) noexcept { *this = std::move(o); }
	PinnedStaging &operator=(PinnedStaging &&o) noexcept  // (what this one held goes with o)
	{
		std::swap(host, o.host);
		std::swap(cap, o.cap);
		std::swap(copied, o.copied);
		return *this;
	}
	~PinnedStaging() { release(); }

	void release()
	{
		if (copied) (void)hipEventDestroy(copied);
		if (host) (void)hipHostFree(host);
		copied = nullptr;
		host = nullptr;
		cap = 0;
	}
	// Waits for the previous copy out of the block, grows the block if it is smaller than `bytes` (to `room` bytes when
	// that is more), fills it from src and queues its copy to the device address dst on the stream.
	hipError_t send(const void *src, size_t bytes, void *dst, hipStream_t stream, size_t room = 0)
	{
		hipError_t e = copied ? hipEventSynchronize(copied) : hipEventCreateWithFlags(&copied, hipEventDisableTiming);
		if (e != hipSuccess) return e;
		if (cap < bytes) {
			if (host) (void)hipHostFree(host);
			host = nullptr;
			cap = 0;
			if (room < bytes) room = bytes;
			if ((e = hipHostMalloc(&host, room, hipHostMallocDefault)) != hipSuccess) {
				host = nullptr;
				return e;
			}
			cap = room;
		}
		std::memcpy(host, src, bytes);
		if ((e = hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
		return hipEventRecord(copied, stream);
	}
};

}  // namespace pxz
