// bf_remove.hpp -- what a remove from a built brute-force index does: THE list of the rules, beside bf_append.hpp's.
// plan_remove() reads what the handle holds and names the refusal and the fate of the fp16 copy; new_id() is the
// order-preserving shift of the survivors' ids, the arithmetic the device's compaction does word by word.
// expann_hip.hip carries the answers out and decides none by itself; tests/test_bf_remove.py pins every rule
// without a device.
// Host arithmetic on the standard library alone: no HIP here, no allocation.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bf_append.hpp"

namespace expann {

// The keep bitmap has the row filter's layout: bit r & 31 of word r >> 5, whole 128-row tiles, ones on the
// survivors, zero on the removed rows and from row n on.
inline size_t keep_words(size_t n) { return (n + 127) / 128 * 4; }

// The id of survivor `i` after the remove: the survivors before it.  word_rank[w] = survivors in the words before w
// (the prefix remove_word_rank_kernel writes); the rest is one popcount.
inline uint32_t new_id(const uint32_t* bits, const uint32_t* word_rank, uint32_t i) {
	return word_rank[i >> 5] + (uint32_t)__builtin_popcount(bits[i >> 5] & ((1u << (i & 31)) - 1u));
}
// the prefix itself, on the host (what the device's array holds); returns the survivors in all
inline uint32_t word_ranks(const uint32_t* bits, size_t n_words, uint32_t* word_rank) {
	uint32_t r = 0;
	for (size_t w = 0; w < n_words; ++w) {
		word_rank[w] = r;
		r += (uint32_t)__builtin_popcount(bits[w]);
	}
	return r;
}

enum class RemoveCopy {
	kNothing,  // no copy yet, or 8-bit / int16 rows: only the base is compacted
	kCompact,  // the survivors' scale is the copy's: rows and terms were gathered, the maxima recomputed
	kDrop      // the scale changed, or the rows were marked unusable (the mark is forgotten): the copy dies and is
	           // made again where a build would make it, else by the next search
};
struct RemovePlan {
	int status = EXPANN_OK;
	const char* message = "";
	size_t n = 0;  // rows after the remove
	RemoveCopy copies = RemoveCopy::kNothing;
	// (every OTHER derived copy, the row filter and the row groups are forgotten whenever a row was removed; the
	// base's capacity never changes)
};

// The checks made before the device is touched, in the header's order (have_rows: ids != NULL, or n_ids == 0).
inline RemovePlan plan_remove(const AppendState& s, size_t n_ids) {
	RemovePlan p;
	p.n = s.n;
	const auto refuse = [&p](int code, const char* msg) {
		p.status = code;
		p.message = msg;
		return p;
	};
	if (!s.have_handle)
		return refuse(EXPANN_ERR_INVALID_ARG, "handle == NULL");
	if (!s.have_rows && n_ids)
		return refuse(EXPANN_ERR_INVALID_ARG, "ids == NULL");
	if (!s.on_device)
		return refuse(EXPANN_ERR_NOT_BUILT, "remove before build()");
	if (!s.owned)
		return refuse(EXPANN_ERR_UNSUPPORTED, "remove from rows adopted by expann_set_base_device: they are the caller's memory");
	return p;
}

// ... and what the mark pass has shown: an id at or beyond n (bad_id), the survivors' count and max |v| over them
// (read only where a copy exists).  Decided before any allocation is swapped: a refusal leaves the handle as it was.
inline RemovePlan plan_remove(const AppendState& s, size_t n_ids, bool bad_id, size_t n_survivors, float maxabs_survivors) {
	RemovePlan p = plan_remove(s, n_ids);
	if (p.status != EXPANN_OK || n_ids == 0)
		return p;
	const auto refuse = [&p](int code, const char* msg) {
		p.status = code;
		p.message = msg;
		return p;
	};
	if (bad_id)
		return refuse(EXPANN_ERR_INVALID_ARG, "remove: an id at or beyond expann_size()");
	if (n_survivors == 0)
		return refuse(EXPANN_ERR_INVALID_ARG, "remove: would leave no row (an index is never empty)");
	p.n = n_survivors;
	if (!s.float_rows || s.f16_scale == 0.0f || n_survivors == s.n)
		return p;
	if (s.f16_scale < 0.0f) {
		p.copies = RemoveCopy::kDrop;  // the survivors may fit
		return p;
	}
	const F16Scale f = f16_scale_for(maxabs_survivors);
	p.copies = (f.usable && f.scale == s.f16_scale) ? RemoveCopy::kCompact : RemoveCopy::kDrop;
	return p;
}

}  // namespace expann
