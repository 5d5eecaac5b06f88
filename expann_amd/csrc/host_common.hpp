// host_common.hpp -- host-side helpers shared by the translation units of libexpann_hip
// (expann_hip.hip: the brute-force index; expann_graph.hip: graph path and quantiser builds).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/expann_hip.h"

// every handle type has fail(code, message) -> code
#define HIP_TRY(h, expr)                                                                   \
	do {                                                                                   \
		hipError_t _e = (expr);                                                            \
		if (_e != hipSuccess)                                                              \
			return (h)->fail(EXPANN_ERR_HIP, std::string(#expr) + ": " +                   \
			                                       hipGetErrorString(_e));                 \
	} while (0)

// inside a helper that reports a hipError_t itself: the first error ends it (the caller wraps the helper in HIP_TRY)
#define HIP_OK(expr)                                   \
	do {                                               \
		if (hipError_t _e = (expr); _e != hipSuccess)  \
			return _e;                                 \
	} while (0)

namespace expann {

// the bound on k of every brute-force search (half the longest candidate list, kMaxCap in bf_options.hpp):
// a larger k is refused by value at the entry point, before any GPU work
constexpr size_t kMaxK = 8192;
inline std::string k_too_large() { return "k too large for the candidate buffers (k <= " + std::to_string(kMaxK) + ")"; }

// scoped device allocation for the entry points that need per-call temporaries
struct DevBuf {
	void* p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() {
		if (p)
			(void)hipFree(p);
	}
	hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
	template <typename T> T* as() const { return static_cast<T*>(p); }
};

// What a handle OWNS through HIP -- device memory, pinned host memory, a stream, an event: released when the handle
// goes away, converts to the raw pointer the kernels and HIP calls take (`hipMalloc(&h->d_x, n)` still works).
// Not copyable; movable, so that a group of them is forgotten as a value (`group = Group{}`); `reset()` releases now.
template <typename P, auto Release> struct HipOwned {
	P p = nullptr;
	HipOwned() = default;
	HipOwned(const HipOwned&) = delete;
	HipOwned& operator=(const HipOwned&) = delete;
	HipOwned(HipOwned&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
	HipOwned& operator=(HipOwned&& o) noexcept {  // (what this one held goes with `o`)
		std::swap(p, o.p);
		return *this;
	}
	~HipOwned() { reset(); }
	void reset() {
		if (p)
			(void)Release(p);
		p = nullptr;
	}
	P get() const { return p; }
	template <typename U> U* as() const { return (U*)p; }  // the same bytes as another element type
	operator P() const { return p; }
	P* operator&() { return &p; }
	explicit operator bool() const { return p != nullptr; }
};
template <typename T> using DevPtr = HipOwned<T*, hipFree>;
template <typename T> using PinPtr = HipOwned<T*, hipHostFree>;
using OwnedStream = HipOwned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = HipOwned<hipEvent_t, hipEventDestroy>;
// a DevPtr that only ever grows: ensure(n) keeps the allocation when it is large enough.  Growing
// frees the old block: work still in flight that reads it must have drained first (the callers with
// deferred searches outstanding synchronise their stream before they grow a shared buffer).
template <typename T> struct GrowPtr : DevPtr<T> {
	size_t bytes = 0;
	GrowPtr() = default;
	GrowPtr(GrowPtr&& o) noexcept : DevPtr<T>(std::move(o)), bytes(std::exchange(o.bytes, 0)) {}
	GrowPtr& operator=(GrowPtr&& o) noexcept {
		std::swap(this->p, o.p);
		std::swap(bytes, o.bytes);
		return *this;
	}
	hipError_t ensure(size_t need) {
		if (need <= bytes && this->p)
			return hipSuccess;
		this->reset();
		bytes = 0;
		const hipError_t e = hipMalloc((void**)&this->p, need ? need : 1);
		if (e == hipSuccess)
			bytes = need;
		return e;
	}
	void reset_all() {
		this->reset();
		bytes = 0;
	}
};
// Device memory a handle reads and may or may not own -- rows handed in by the caller, a padded copy that is an
// alias when no padding is needed: own() takes memory to free, borrow() memory of someone else.  Converts to any
// pointer type the kernels' parameter blocks take.  (Moved from, it borrows what it held: nothing is freed twice.)
struct MaybeOwnedPtr {
	void* p = nullptr;  // what is read
	DevPtr<void> mine;  // the same block where the handle owns it
	void own(void* q) {
		mine.reset();
		mine.p = p = q;
	}
	void borrow(const void* q) {
		mine.reset();
		p = const_cast<void*>(q);
	}
	template <typename U> operator U*() const { return (U*)p; }
	explicit operator bool() const { return p != nullptr; }
};

// The directory of a row-group labelling (expann_graph_set_row_groups, expann_set_row_groups): the distinct labels
// ascending with 0xFFFFFFFF (EXPANN_GROUP_ANY: the row belongs to no group) left out, their offsets, and each
// group's rows ascending -- rows[off[g], off[g + 1]) carry keys[g].  Made on the host with a stable sort by label:
// set time is no hot path.
struct GroupDirectory {
	std::vector<uint32_t> keys;  // [groups]
	std::vector<uint32_t> off;   // [groups + 1]
	std::vector<uint32_t> rows;  // [n]: the rows by (label, row); the first off.back() of them belong to a group
	size_t n_rows() const { return off.back(); }
	// the group that carries `label`, or keys.size() when no row does
	size_t find(uint32_t label) const {
		const auto it = std::lower_bound(keys.begin(), keys.end(), label);
		return (it != keys.end() && *it == label) ? (size_t)(it - keys.begin()) : keys.size();
	}
};
inline GroupDirectory build_group_directory(const uint32_t* lab, size_t n) {
	GroupDirectory d;
	d.rows.resize(n);
	for (size_t v = 0; v < n; ++v)
		d.rows[v] = (uint32_t)v;
	std::stable_sort(d.rows.begin(), d.rows.end(), [&](uint32_t a, uint32_t b) { return lab[a] < lab[b]; });
	size_t n_rows = n;  // rows labelled 0xFFFFFFFF sort last and belong to no group
	while (n_rows && lab[d.rows[n_rows - 1]] == 0xFFFFFFFFu)
		--n_rows;
	for (size_t i = 0; i < n_rows; ++i)
		if (i == 0 || lab[d.rows[i]] != lab[d.rows[i - 1]]) {
			d.keys.push_back(lab[d.rows[i]]);
			d.off.push_back((uint32_t)i);
		}
	d.off.push_back((uint32_t)n_rows);
	return d;
}
// The labels a set call was given, on the host: n of them in host (on_device = false) or device memory, the latter
// read in the order of `st` and waited for.  EXPANN_OK, or the HIP error on the handle `h`.
template <typename Handle>
int fetch_group_labels(Handle* h, const uint32_t* groups, size_t n, bool on_device, hipStream_t st, std::vector<uint32_t>& lab) {
	lab.resize(n);
	if (on_device) {
		HIP_TRY(h, hipMemcpyAsync(lab.data(), groups, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
		HIP_TRY(h, hipStreamSynchronize(st));
	} else
		std::memcpy(lab.data(), groups, sizeof(uint32_t) * n);
	return EXPANN_OK;
}

// what expann_*_last_error(NULL) reports: the failure of the last create call of this thread
extern thread_local std::string g_create_error;

int num_cus(int device);

}  // namespace expann
