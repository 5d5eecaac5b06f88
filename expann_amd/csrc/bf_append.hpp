// bf_append.hpp -- what an append to a built brute-force index does: THE list of the rules.  f16_scale_for() is the
// scale of the fp16 copy (ensure_f16 builds with it, an append compares with it); plan_append() reads what the handle
// holds and names the refusal, the base's new capacity and the fate of the fp16 copy; plan_reserve() does the same
// for expann_reserve.  expann_hip.hip carries the answers out and decides none by itself; tests/test_bf_append.py
// pins every rule without a device.
// Host arithmetic on the standard library alone: no HIP here, no allocation.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/expann_hip.h"

namespace expann {

// rows of one handle: n + 32 stays below 2^32 (expann_build's bound)
constexpr size_t kMaxRows = ((size_t)1 << 32) - 32;

// The fp16 copy holds the rows times a power of two that brings max |v| just under 2^15: e = floor(log2(32768 /
// maxabs)), clamped to +-40 so that s^2 and every scaled norm stay finite in fp32; all-zero rows: 1.  Unusable when
// the scaled maximum still exceeds 32768: non-finite (a NaN fails every comparison) or astronomically large values.
struct F16Scale {
	float scale = 1.0f;
	bool usable = true;
};
inline F16Scale f16_scale_for(float maxabs) {
	F16Scale r;
	if (maxabs > 0.0f && std::isfinite(maxabs)) {
		int e = (int)std::floor(std::log2(32768.0 / (double)maxabs));
		e = e < -40 ? -40 : (e > 40 ? 40 : e);
		r.scale = std::ldexp(1.0f, e);
	}
	r.usable = maxabs * r.scale <= 32768.0f;
	return r;
}
// max |v| of two sets of rows, a NaN winning (as the device's maximum of bit patterns lets it)
inline float maxabs_of(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

// what plan_append reads of a handle
struct AppendState {
	bool have_handle = true;  // (the entry point's first two checks, so that the order of the errors is one list)
	bool have_rows = true;    // rows != NULL, or n == 0
	bool on_device = false;   // the index holds rows on the device
	bool owned = false;       // ... in memory of its own (expann_build), not the caller's (expann_set_base_device)
	bool float_rows = true;   // F32 / F16 rows: the ones an fp16 copy is made of
	size_t n = 0;             // rows
	size_t capacity = 0;      // rows the base allocation holds
	float f16_scale = 0.0f;   // the fp16 copy: 0 none yet, < 0 the rows do not fit the fp16 range, > 0 its scale
	float maxabs = 0.0f;      // max |v| of the rows the copy was made from
};
enum class CopyAction {
	kNothing,  // no copy, a copy marked unusable (the longer index is unusable too), or 8-bit / int16 rows
	kExtend,   // the copy's scale is the longer index's: the new rows were converted in place
	kDrop      // the scale changed: the copy dies (and is rebuilt where a build would make it)
};
struct AppendPlan {
	int status = EXPANN_OK;
	const char* message = "";
	size_t n = 0;            // rows after the append
	size_t capacity = 0;     // of the base after the append
	bool realloc = false;    // a larger base is built aside and swapped in
	CopyAction copies = CopyAction::kNothing;
	// (every OTHER derived copy -- uint8 shadow, bf16 planes, int8 filter, the 8-bit indexes' terms -- is forgotten
	// in all three cases, whenever rows were added)
};

// The capacity grows by half (x 1.5) when an append does not fit: a run of appends copies O(total rows) -- at most
// three times the final size -- and the old and the new base are both live only while one is copied into the other.
inline size_t grown_capacity(size_t capacity, size_t need) {
	size_t c = capacity + capacity / 2;
	if (c < need)
		c = need;
	return c < kMaxRows - 1 ? c : kMaxRows - 1;
}

// expann_append(h, rows, n_new); maxabs_new = max |v| of the new rows (read only where a copy exists; the status
// and the capacity do not depend on it, so the entry point plans once before the device is touched and once after
// the append kernel has reported it)
inline AppendPlan plan_append(const AppendState& s, size_t n_new, float maxabs_new) {
	AppendPlan p;
	p.n = s.n;
	p.capacity = s.capacity;
	const auto refuse = [&p](int code, const char* msg) {
		p.status = code;
		p.message = msg;
		return p;
	};
	if (!s.have_handle)
		return refuse(EXPANN_ERR_INVALID_ARG, "handle == NULL");
	if (!s.have_rows && n_new)
		return refuse(EXPANN_ERR_INVALID_ARG, "rows == NULL");
	if (!s.on_device)
		return refuse(EXPANN_ERR_NOT_BUILT, "append before build(): expann_add stores rows until then");
	if (!s.owned)
		return refuse(EXPANN_ERR_UNSUPPORTED, "append to rows adopted by expann_set_base_device: they are the caller's memory");
	if (n_new >= kMaxRows || s.n + n_new >= kMaxRows)
		return refuse(EXPANN_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
	if (n_new == 0)
		return p;
	p.n = s.n + n_new;
	if (p.n > s.capacity) {
		p.realloc = true;
		p.capacity = grown_capacity(s.capacity, p.n);
	}
	if (s.float_rows && s.f16_scale > 0.0f) {
		const F16Scale f = f16_scale_for(maxabs_of(s.maxabs, maxabs_new));
		p.copies = (f.usable && f.scale == s.f16_scale) ? CopyAction::kExtend : CopyAction::kDrop;
	}
	return p;
}

// expann_reserve(h, n_rows) on a handle with rows on the device: room for n_rows rows at least.  (Before build()
// the value is remembered and expann_build allocates max(staged, reserved).)
inline AppendPlan plan_reserve(const AppendState& s, size_t n_rows) {
	AppendPlan p;
	p.n = s.n;
	p.capacity = s.capacity;
	if (!s.have_handle) {
		p.status = EXPANN_ERR_INVALID_ARG;
		p.message = "handle == NULL";
	} else if (s.on_device && !s.owned) {
		p.status = EXPANN_ERR_UNSUPPORTED;
		p.message = "reserve on rows adopted by expann_set_base_device: they are the caller's memory";
	} else if (n_rows >= kMaxRows) {
		p.status = EXPANN_ERR_UNSUPPORTED;
		p.message = "more than 2^32 rows per shard";
	} else if (s.on_device && n_rows > s.capacity) {
		p.realloc = true;
		p.capacity = n_rows;
	}
	return p;
}

}  // namespace expann
