// select_range.hpp -- the select of a range search (THE RANGE RULE, include/expann_hip.h): every row of a query's
// candidate list whose exact score is <= the query's radius, counted, ordered by (score, id) and written as a
// variable number of rows behind a fixed stride.
//
// The lists come from the threshold filters run with the caller's radii as tau.  A list of the matrix-core
// filter (fp16 forms) holds approximate keys of a SUPERSET of the in-range rows: every candidate is re-scored
// exactly -- no pruning, a candidate the k-best logic would drop can still be in range -- and cut at the radius.
// A list of the exact direct scan holds final keys of exactly the in-range rows.  A list that overflowed its
// capacity writes nothing but its query number to the overflow list (and, exact keys, its count: the scan's
// counter goes on counting past the capacity).
//
// One workgroup of THREADS threads per query slot on a static grid: no work counter, no loop that pulls work.
// THREADS = 64 is the one-wave form of the short lists (its barriers are a single wave's), 256 and 1 024 sort
// the long ones, up to kMaxCap keys in LDS.  Each launch serves the lists whose length lies in its [len_min,
// len_hi]; the others' workgroups leave at once.
#pragma once
#include "common.hpp"

namespace expann {

struct RangeSelectParams {
	const uint64_t* cand;      // [n_slots][cap] keys
	const uint32_t* cand_cnt;  // [n_slots] keys the scan found (it counts past cap)
	uint32_t cap;
	uint32_t n_slots;
	uint32_t len_min, len_hi;  // this launch serves the lists of len_min <= c <= len_hi keys (len_hi <= cap, <= lds_keys) ...
	uint32_t takes_overflow;   // ... and, when set, reports the lists of c > cap
	uint32_t lds_keys;         // keys of dynamic LDS (a power of two >= len_hi); one counter word behind them
	const uint32_t* slot_map;  // slot s belongs to the caller's query slot_map[s] (nullptr: s)
	const float* radii;        // [m] the caller's radii, true units
	// re-score (lists of the matrix-core filter): non-null, the keys carry approximate scores
	const void* rerank_base;   // [n_rows][dim] float or binary16 rows (the kernel's TR)
	const float* queries;      // [m][dim] the caller's queries
	uint32_t n_rows;
	uint32_t dim;
	uint32_t metric_ip;
	uint32_t max_results;
	uint64_t id_offset;
	uint64_t* out_ids;         // [m][max_results] (nullptr allowed when max_results == 0)
	float* out_dists;          // [m][max_results] or nullptr
	uint32_t* out_counts;      // [m]
	uint32_t* over_cnt;        // [1] length of over_list
	uint32_t* over_list;       // [over_cap] the caller's numbers of the queries whose list overflowed
	uint32_t over_cap;
};

template <typename TR, int THREADS>
__global__ __launch_bounds__(THREADS) void range_select_kernel(RangeSelectParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char range_smem[];
	uint64_t* const keys = reinterpret_cast<uint64_t*>(range_smem);
	uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(keys + p.lds_keys);  // (behind the keys: select.hpp on static LDS)
	const uint32_t slot = blockIdx.x, tid = threadIdx.x;
	if (slot >= p.n_slots)
		return;
	const uint32_t c = p.cand_cnt[slot];  // (uniform over the workgroup: every return below is the whole workgroup's)
	const uint32_t qo = p.slot_map ? p.slot_map[slot] : slot;
	const bool exact = p.rerank_base == nullptr;
	const bool count_only = p.max_results == 0;
	if (c > p.cap) {
		if (p.takes_overflow && tid == 0) {
			if (exact)
				p.out_counts[qo] = c;  // exact keys: the counter IS the number of rows in range
			const uint32_t pos = atomicAdd(p.over_cnt, 1u);
			if (pos < p.over_cap)
				p.over_list[pos] = qo;
		}
		return;
	}
	if (c < p.len_min || c > p.len_hi)
		return;
	if (exact && count_only) {
		if (tid == 0)
			p.out_counts[qo] = c;
		return;
	}
	uint32_t n2 = 2;
	while (n2 < c)
		n2 <<= 1;  // (c <= len_hi <= lds_keys, a power of two: n2 <= lds_keys)
	const uint64_t* src = p.cand + (size_t)slot * p.cap;
	for (uint32_t i = tid; i < n2; i += THREADS)
		keys[i] = i < c ? src[i] : kSentinelKey;
	if (tid == 0)
		*s_cnt = 0;
	__syncthreads();
	uint32_t count = c;
	if (!exact) {
		// exact re-score of EVERY candidate, select_topk_kernel's arithmetic: 16 lanes per row, lane l owns dims l,
		// l + 16, ... in increasing order, the partial sums meet in reduce16_ref_order -- scan_filter_f32_kernel's bits.
		// U rows per 16-lane group in flight; slot i is read and rewritten by the one group that owns it.
		constexpr uint32_t U = 4, G = THREADS / 16;
		const uint32_t l = tid & 15, grp = tid >> 4;
		const float* q = p.queries + (size_t)qo * p.dim + l;
		const float radius = p.radii[qo];
		const uint32_t nt = p.dim / 16;
		uint32_t mine = 0;
		for (uint32_t i0 = 0; i0 < c; i0 += U * G) {
			float acc[U];
			uint32_t row[U];
			bool live[U];
			const TR* r[U];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				const uint32_t i = i0 + u * G + grp;
				row[u] = i < c ? key_idx(keys[i]) : 0u;
				live[u] = i < c && row[u] < p.n_rows;  // (a row number outside the index is never read)
				row[u] = live[u] ? row[u] : 0u;
				r[u] = (const TR*)p.rerank_base + (size_t)row[u] * p.dim + l;
				acc[u] = 0.0f;
			}
			for (uint32_t t = 0; t < nt; ++t) {
				const float qv = q[16 * t];
				TR rv[U];
#pragma unroll
				for (uint32_t u = 0; u < U; ++u)
					rv[u] = r[u][16 * t];
#pragma unroll
				for (uint32_t u = 0; u < U; ++u) {
					if (p.metric_ip) {
						acc[u] = ref_dot<TR>(qv, rv[u], acc[u]);
					} else {
						const float diff = ref_diff<TR>(qv, rv[u]);
						acc[u] = __builtin_fmaf(diff, diff, acc[u]);
					}
				}
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				const float red = reduce16_ref_order(acc[u]);
				const float s = p.metric_ip ? -red : red;
				const uint32_t i = i0 + u * G + grp;
				const bool in = live[u] && s <= radius;  // (inclusive; a NaN radius or score is in range of nothing)
				if (l == 0 && i < c) {
					keys[i] = in ? make_key(s, row[u]) : kSentinelKey;
					mine += in ? 1u : 0u;
				}
			}
		}
		if (mine)
			atomicAdd(s_cnt, mine);
		__syncthreads();
		count = *s_cnt;
	}
	if (count_only) {
		if (tid == 0)
			p.out_counts[qo] = count;
		return;
	}
	// bitonic sort of the power-of-two padded list: ascending (score, id), the sentinels behind every real key
	for (uint32_t size = 2; size <= n2; size <<= 1) {
		for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
			for (uint32_t i = tid; i < (n2 >> 1); i += THREADS) {
				const uint32_t lo = 2 * i - (i & (stride - 1));
				const uint32_t hi = lo + stride;
				const bool up = ((lo & size) == 0);
				const uint64_t a = keys[lo], b = keys[hi];
				if ((a > b) == up) {
					keys[lo] = b;
					keys[hi] = a;
				}
			}
			__syncthreads();
		}
	}
	const uint32_t n_out = count < p.max_results ? count : p.max_results;
	for (uint32_t i = tid; i < p.max_results; i += THREADS) {
		const bool ok = i < n_out;  // (n_out <= count <= c <= n2: inside the list)
		const uint64_t key = ok ? keys[i] : kSentinelKey;
		p.out_ids[(size_t)qo * p.max_results + i] = ok ? (uint64_t)key_idx(key) + p.id_offset : ~0ull;
		if (p.out_dists)
			p.out_dists[(size_t)qo * p.max_results + i] = ok ? key_score(key) : __builtin_inff();
	}
	if (tid == 0)
		p.out_counts[qo] = count;
}

// list[i] = i: the overflow list of a pass whose every query goes to the next stage
static __global__ __launch_bounds__(kBlock) void range_iota_kernel(uint32_t* list, uint32_t n) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i < n)
		list[i] = i;
}

}  // namespace expann
