// select.hpp -- exact k-selection over a query's candidate keys, and the k-way merge of
// per-shard results.  The order is the reference's: ascending (score, id), i.e. the
// lexicographic std::pair order of the max-heaps in src/topk_t.h:11 and
// src/brute_force_engine.h:29-46 (k smallest, ties by lower id, output ascending).
#pragma once
#include "common.hpp"

namespace expann {

struct SelectParams {
	const uint64_t* cand;     // [m][cap] keys
	const uint32_t* cand_cnt; // [m], or nullptr: every query has fixed_count keys
	uint32_t fixed_count;
	uint32_t cap;
	uint32_t k;
	uint64_t id_offset;
	uint64_t* out_ids;        // [m][k] or nullptr
	float* out_dists;         // [m][k] or nullptr
	float* tau_out;           // [m] k-th smallest score, or nullptr
	const float* tau_prev;    // [m] carried forward when fewer than k keys (nullptr: +inf)
	uint32_t* tau_row_out;    // [m] row of the k-th smallest key (UINT32_MAX when carried) or nullptr
	const uint32_t* tau_row_prev;
	// re-rank (GEMM-form scan): when rerank_base != nullptr the keys hold only a row number
	// (low 32 bits); the exact reference-order score is recomputed here before the sort
	const float* rerank_base;     // [n][dim] (the _Float16 instances of the select kernels: binary16 rows behind the pointer)
	const float* rerank_queries;  // [m][dim]
	uint32_t dim;
	uint32_t metric_ip;
	// rerank pruning (L2 GEMM forms): the approximate key A = bn(1-eps) - 2 q.b satisfies
	//   A + qn(1-eps/2)  <=  reference-order score  <=  A + qn(1+eps/2) + 1.5 eps bn
	// (the slack eps is at least twice the worst-case evaluation error, scan_gemm_*.hpp), so a
	// candidate whose A exceeds the k-th smallest A by more than eps*(qn + 1.5*bn_max) cannot be
	// among the k best and need not be re-scored.  prune_eps == 0 disables it.
	float prune_eps;
	float prune_abs;          // absolute slack coefficient (fp16 form): + prune_abs*(|q| + |b|max)
	const float* bn_max;      // [1] max over rows of ||b||^2 (1-eps)
	uint32_t* overflow;       // [1] number of queries whose list overflowed cap
	uint32_t wave_done;       // select_wave_kernel already served the lists of <= wave_done keys
	uint32_t wave0_short;     // select_topk_kernel: lists of <= 2048 keys go through wave 0's wave path
	const float* qnrm;        // [m] ||q||^2 if the caller has it (pruning margin), else nullptr
	// rerank pruning of the int8 filter (scan_gemm_i8f.hpp), replacing prune_eps / prune_abs when row_w != nullptr:
	// key = kappa (units of 2 s^2), a row's upper bound is kappa + row_w[row] + q_w[query], its lower bound kappa;
	// a candidate whose kappa exceeds the k-th smallest upper bound cannot be among the k best
	const float* row_w;
	const float* q_w;
	// two-round re-rank of the int8 filter's lists (the TWO instances of the wave body; scan_gemm_i8f.hpp, "Two
	// rounds"): tau_f[slot] = the fp32 threshold thp[slot] was derived from (true units), inv_2s2 = 1 / (2 s^2).  The
	// R1 keys of smallest kappa are re-scored first, T = their k-th exact score; of the others only those with
	// tau_f + 2 s^2 kappa <= T are.  tau_f == nullptr: the single cut above ("rerank_rounds" = 1).
	const float* tau_f;
	double inv_2s2;
	// statistics ("rerank_stats"), or nullptr: rerank_cnt[query] = rows this select re-scored exactly (+= in the
	// redo pass's select, whose queries the main select has counted before)
	uint32_t* rerank_cnt;
	// speculative thresholds: the lists were filtered with spec_tau[q] (true units), tighter than
	// the proven threshold.  Where a query's result is emitted its k-th exact score S_k is known: fewer than k rows,
	// or S_k > spec_tau[q], and the query number is appended to redo_list through the counter in *redo_word (low
	// 20 bits: failing queries; from bit 20: redo overflows).  spec_tau == nullptr: no check.
	// With the query number goes what the failed list itself proves: redo_bound[slot] = S_k when the list held k
	// rows -- k distinct rows score <= S_k, so the index's k-th best does -- else +inf.
	const float* spec_tau;
	uint32_t* redo_word;
	uint32_t* redo_list;      // [redo_cap]
	uint32_t redo_cap;
	float* redo_bound;        // [redo_cap]
	// the redo pass's own select: query slot s (lists, counters, qnrm, q_w) belongs to query slot_map[s] (the
	// re-rank's query row, the output rows); slots at and beyond the failing count (*live_slots, low 20 bits) leave
	// at once, and an overflowing list adds 2^20 to *overflow (= the redo word) instead of 1
	const uint32_t* slot_map;
	const uint32_t* live_slots;
	uint32_t* redo_cand;      // [1] statistics: += the keys of every live slot's list
};
constexpr uint32_t kRedoCountMask = 0xFFFFFu;  // (a pass has at most 32 768 queries)
constexpr uint32_t kRedoOverflowUnit = 1u << 20;

// the check of a speculative threshold for query qi: has_kth = the list held k rows, s_k = the k-th exact score
__device__ inline void spec_check(const SelectParams& p, uint32_t qi, bool has_kth, float s_k) {
	if (!p.spec_tau || (has_kth && s_k <= p.spec_tau[qi]))
		return;
	const uint32_t slot = atomicAdd(p.redo_word, 1u) & kRedoCountMask;
	if (slot < p.redo_cap) {
		p.redo_list[slot] = qi;
		p.redo_bound[slot] = has_kth ? s_k : __builtin_inff();
	}
}

// the cutoff of the int8 filter's pruning from the k-th smallest (ordered) kappa + w_b: + w_q, + the margin
// for the fp32 rounding of keys and sums (scan_gemm_i8f.hpp); no k-th value (or an infinite one): no cut
__device__ inline float i8f_cutoff(uint32_t kth_ord, float wq) {
	if (kth_ord >= 0xFF800000u)
		return __builtin_inff();
	const float c = ordered_to_float(kth_ord) + wq;
	return c + __builtin_fabsf(c) * 0x1p-18f + 1.0f;
}
// ordered kappa + w_b of one candidate key (+inf when the row's w_b is, whatever its key)
__device__ inline uint32_t i8f_upper_ord(const SelectParams& p, uint64_t key) {
	const float v = key_score(key) + p.row_w[key_idx(key)];
	return float_to_ordered(v == v ? v : __builtin_inff());
}

// the kappa at and below which a row of the second round may still reach T (the k-th exact score of the first
// round): S >= tau_f + 2 s^2 kappa (scan_gemm_i8f.hpp), so a row can be dropped when kappa > x = (T - tau_f) / 2s^2.
// x is formed in fp64 (T - tau_f: one rounding, the stored 1 / 2s^2 and the product one each: < 2^-50 relative,
// covered by 2^-40 |x| + 2^-10) and rounded UP to fp32; a key is the fp32 rounding of its integer kappa and rounding
// is monotone, so kappa <= x implies key <= cut.  A NaN (no finite T or tau_f) keeps every row: !(key > cut).
__device__ inline float i8f_round2_cut(float t, float tau_f, double inv_2s2) {
	const double x = ((double)t - (double)tau_f) * inv_2s2;
	const double xu = x + (__builtin_fabs(x) * 0x1p-40 + 0x1p-10);
	float f = (float)xu;
	if ((double)f < xu)  // (the conversion rounded down: one step up; +inf stays)
		f = f == 0.0f ? __builtin_bit_cast(float, 1u)
		              : __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + (f > 0.0f ? 1u : 0xFFFFFFFFu));
	return f;
}

// statistics: *out = sum of counts (one workgroup; one same-address atomic per query in the
// select kernel would cost ~10 ns each, 100 us at 10^4 queries)
__global__ __launch_bounds__(1024) void sum_u32_kernel(const uint32_t* in, uint32_t n,
                                                       unsigned long long* out) {
	__shared__ unsigned long long red[16];
	unsigned long long s = 0;
	for (uint32_t i = threadIdx.x; i < n; i += 1024)
		s += in[i];
	for (int off = 32; off > 0; off >>= 1)
		s += __shfl_xor(s, off);
	if ((threadIdx.x & 63) == 0)
		red[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 16; ++w)
			s += red[w];
		out[0] = s;
	}
}

// min over the 64 lanes (result in every lane)
__device__ inline uint32_t wave_min_u32(uint32_t v) {
	// within rows of 16 by DPP rotations, then across the four rows
	v = min(v, (uint32_t)row_ror_i<8>((int)v));
	v = min(v, (uint32_t)row_ror_i<4>((int)v));
	v = min(v, (uint32_t)row_ror_i<2>((int)v));
	v = min(v, (uint32_t)row_ror_i<1>((int)v));
	v = min(v, (uint32_t)__shfl_xor((int)v, 16));
	v = min(v, (uint32_t)__shfl_xor((int)v, 32));
	return v;
}
__device__ inline uint64_t wave_min_u64(uint64_t v) {
	// the high word first (scores), the low word (rows) among the lanes that hold the min score
	const uint32_t hi = (uint32_t)(v >> 32);
	const uint32_t mhi = wave_min_u32(hi);
	const uint32_t lo = hi == mhi ? (uint32_t)v : 0xFFFFFFFFu;
	return ((uint64_t)mhi << 32) | wave_min_u32(lo);
}

// ---- one WAVE per query -------------------------------------------------------------------
// Lists of at most 2048 candidates (what the sampled thresholds leave) are ordered by a single
// wave: the chain count -> keys -> candidate rows -> output is three dependent memory round
// trips whatever the arithmetic, so the win over one 256-thread workgroup per query is 4x the
// queries in flight and no workgroup barriers.  With rerank_base the keys carry approximate
// scores of a GEMM-form scan (pruned, then re-scored exactly); without, final scores.  Longer
// lists are left to select_topk_kernel (which skips the queries served here: p.wave_done).

// the k smallest of the n_s <= 64*NE keys in list[], ascending, to the outputs (+ the next tau).
// Small k: k rounds of wave-min extraction, lane 0 writes.  Larger k: every lane ranks its keys
// by counting (all n_s keys stream past as LDS broadcasts) and writes them to their rank.
template <int NE>
__device__ inline void wave_emit_sorted(const SelectParams& p, const uint64_t* list, uint32_t n_s,
                                        uint32_t qi, int lane) {
	uint64_t e[NE];
#pragma unroll
	for (int j = 0; j < NE; ++j)
		e[j] = lane + 64 * j < (int)n_s ? list[lane + 64 * j] : kSentinelKey;
	if (p.k > 16) {
		uint32_t r[NE];
#pragma unroll
		for (int j = 0; j < NE; ++j)
			r[j] = 0;
		for (uint32_t i = 0; i < n_s; ++i) {
			const uint64_t x = list[i];
#pragma unroll
			for (int j = 0; j < NE; ++j)
				r[j] += x < e[j] ? 1u : 0u;
		}
#pragma unroll
		for (int j = 0; j < NE; ++j) {
			if (e[j] == kSentinelKey || r[j] >= p.k)
				continue;  // (keys are distinct: ranks are a permutation)
			if (p.out_ids)
				p.out_ids[(size_t)qi * p.k + r[j]] = (uint64_t)key_idx(e[j]) + p.id_offset;
			if (p.out_dists)
				p.out_dists[(size_t)qi * p.k + r[j]] = key_score(e[j]);
			if (r[j] == p.k - 1)
				spec_check(p, qi, true, key_score(e[j]));
			if (r[j] == p.k - 1 && p.tau_out) {
				p.tau_out[qi] = key_score(e[j]);
				if (p.tau_row_out)
					p.tau_row_out[qi] = key_idx(e[j]);
			}
		}
		for (uint32_t i = n_s + lane; i < p.k; i += 64) {  // fewer than k keys: padding
			if (p.out_ids)
				p.out_ids[(size_t)qi * p.k + i] = ~0ull;
			if (p.out_dists)
				p.out_dists[(size_t)qi * p.k + i] = __builtin_inff();
		}
		if (lane == 0 && n_s < p.k)
			spec_check(p, qi, false, 0.0f);
		if (lane == 0 && n_s < p.k && p.tau_out) {
			p.tau_out[qi] = p.tau_prev ? p.tau_prev[qi] : __builtin_inff();
			if (p.tau_row_out)
				p.tau_row_out[qi] = p.tau_row_prev ? p.tau_row_prev[qi] : 0xFFFFFFFFu;
		}
		return;
	}
	for (uint32_t r = 0; r < p.k; ++r) {
		uint64_t mn = e[0];
#pragma unroll
		for (int j = 1; j < NE; ++j)
			mn = e[j] < mn ? e[j] : mn;
		mn = wave_min_u64(mn);
		const bool ok = mn != kSentinelKey;
		if (lane == 0) {
			if (p.out_ids)
				p.out_ids[(size_t)qi * p.k + r] = ok ? (uint64_t)key_idx(mn) + p.id_offset : ~0ull;
			if (p.out_dists)
				p.out_dists[(size_t)qi * p.k + r] = ok ? key_score(mn) : __builtin_inff();
			if (r == p.k - 1)
				spec_check(p, qi, ok, key_score(mn));
			if (r == p.k - 1 && p.tau_out) {
				p.tau_out[qi] = ok ? key_score(mn) : (p.tau_prev ? p.tau_prev[qi] : __builtin_inff());
				if (p.tau_row_out)
					p.tau_row_out[qi] = ok ? key_idx(mn) : (p.tau_row_prev ? p.tau_row_prev[qi] : 0xFFFFFFFFu);
			}
		}
#pragma unroll
		for (int j = 0; j < NE; ++j)
			e[j] = e[j] == mn ? kSentinelKey : e[j];
	}
}

// k-th smallest of the 64*PER values held by a wave (duplicates counted; all-ones = absent):
// bisection on the value, one ballot + popcount per element and step -- 32 steps whatever k
template <int PER> __device__ inline uint32_t wave_kth_smallest_u32(const uint32_t (&v)[PER], uint32_t k) {
	uint32_t lo = 0, hi = 0xFFFFFFFFu;  // smallest x with count(v <= x) >= k
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		uint32_t cnt = 0;
#pragma unroll
		for (int j = 0; j < PER; ++j)
			cnt += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v[j] <= mid));
		if (cnt >= k)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

// k-th largest (0 = absent; 0 is returned when fewer than k values are present)
template <int PER> __device__ inline uint32_t wave_kth_largest_u32(const uint32_t (&v)[PER], uint32_t k) {
	uint32_t lo = 0, hi = 0xFFFFFFFFu;  // largest x with count(v >= x) >= k
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1);
		uint32_t cnt = 0;
#pragma unroll
		for (int j = 0; j < PER; ++j)
			cnt += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v[j] >= mid));
		if (cnt >= k)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// The same k-th largest when k <= 64 and PER is large: B = the k-th largest of the 64 per-lane
// maxima is a lower bound of the answer (k values >= B exist) and usually only a few more values
// reach it -- they are compacted into `scratch` (64 words of LDS, this wave's own) and the
// bisection runs over one value per lane instead of PER.  Falls back to the full bisection when
// more than 64 values reach B (ties, k close to the number of values).
// (j != 0: the j-th largest as well, j <= k, in .y -- it is among the values that reach B, so one more one-value
// bisection; .x = the k-th largest)
template <int PER>
__device__ inline uint2 wave_kth_largest_sparse_u32(const uint32_t (&v)[PER], uint32_t k, uint32_t* scratch,
                                                    int lane, uint32_t j = 0) {
	uint32_t mx[1] = {v[0]};
#pragma unroll
	for (int j = 1; j < PER; ++j)
		mx[0] = v[j] > mx[0] ? v[j] : mx[0];
	const uint32_t B = wave_kth_largest_u32<1>(mx, k);
	uint32_t total = 0;
#pragma unroll
	for (int j = 0; j < PER; ++j)
		total += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v[j] >= B));
	if (total > 64)
		return make_uint2(wave_kth_largest_u32<PER>(v, k), j ? wave_kth_largest_u32<PER>(v, j) : 0u);
	uint32_t base = 0;  // wave-uniform
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const unsigned long long mask = __builtin_amdgcn_ballot_w64(v[j] >= B);
		if (v[j] >= B)
			scratch[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                         __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u))] = v[j];
		base += (uint32_t)__builtin_popcountll(mask);
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	uint32_t w[1] = {lane < (int)total ? scratch[lane] : 0u};
	return make_uint2(wave_kth_largest_u32<1>(w, k), j ? wave_kth_largest_u32<1>(w, j) : 0u);
}

// one wave orders the list of query slot qi (c <= 64 * PER keys); list = 64 * PER keys of LDS
// (TR = element type of the re-rank rows: common.hpp ref_diff / ref_dot)
// TWO: the instances of the int8 filter's lists with the two-round re-rank (SelectParams::tau_f); the others hold
// none of its code
template <int PER, typename TR = float, bool TWO = false>
__device__ inline void select_wave_body(const SelectParams& p, uint32_t qi, uint32_t c, uint64_t* list,
                                        int lane) {
	const uint64_t* src = p.cand + (size_t)qi * p.cap;
	uint64_t kk[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		kk[j] = lane + 64 * j < (int)c ? src[lane + 64 * j] : kSentinelKey;
	const uint32_t l = lane & 15, grp = lane >> 4;  // 16 lanes per candidate row
	const uint32_t qo = p.slot_map ? p.slot_map[qi] : qi;  // (the query whose row is re-ranked and whose outputs are written)
	const float* q = p.rerank_queries + (size_t)qo * p.dim + l;
	float cutoff = __builtin_inff();
	// lists with FINAL scores (the 8-bit forms: no re-score) are cut at their k-th smallest score itself --
	// what is left to rank is k keys + ties instead of the whole list (k = 100 on uint8 rows: 535 keys, each
	// ranked against all of them, were 0.31 ms of a 2.4 ms step)
	const bool final_scores = p.rerank_base == nullptr;
	if (!TWO && (p.prune_eps > 0.0f || final_scores || p.row_w) && c > p.k) {
		float qn = 0.0f;
		if (final_scores || p.row_w) {
		} else if (p.qnrm) {
			qn = p.qnrm[qi];
		} else {
			for (uint32_t t = 0; t < p.dim / 16; ++t)
				qn = __builtin_fmaf(q[16 * t], q[16 * t], qn);
			qn = reduce16_ref_order(qn);
		}
		// k-th smallest approximate score (k-th DISTINCT one if scores repeat: a valid, looser cut)
		uint32_t sc[PER];
#pragma unroll
		for (int j = 0; j < PER; ++j)
			sc[j] = (p.row_w && kk[j] != kSentinelKey) ? i8f_upper_ord(p, kk[j]) : (uint32_t)(kk[j] >> 32);
		uint32_t kth = 0xFFFFFFFFu;
		if (p.k > 24) {
			kth = wave_kth_smallest_u32<PER>(sc, p.k);
		} else
		for (uint32_t r = 0; r < p.k; ++r) {
			uint32_t mn = sc[0];
#pragma unroll
			for (int j = 1; j < PER; ++j)
				mn = min(mn, sc[j]);
			mn = wave_min_u32(mn);
			if (mn == 0xFFFFFFFFu)
				break;
			kth = mn;
#pragma unroll
			for (int j = 0; j < PER; ++j)
				sc[j] = sc[j] == mn ? 0xFFFFFFFFu : sc[j];
		}
		if (final_scores) {
			cutoff = ordered_to_float(kth);
		} else if (p.row_w) {
			cutoff = i8f_cutoff(kth, p.q_w[qi]);
		} else {
			const float bmax = p.bn_max[0];
			cutoff = ordered_to_float(kth) + p.prune_eps * (qn + 1.5f * bmax) +
			         p.prune_abs * (__builtin_sqrtf(qn) + __builtin_sqrtf(bmax));
		}
	}
	uint32_t n_s = 0;  // wave-uniform
	uint32_t n1 = 0;   // TWO: keys of the first round, list[0, n1)
	if (TWO) {
		const uint32_t r1 = p.k <= 16 ? 16u : (p.k + 15u) & ~15u;
		if (c > r1 && p.q_w[qi] < __builtin_inff()) {
			// v = the r1-th smallest kappa (repeated values counted); -inf keys, rows without an interval, come first
			uint32_t sc[PER];
#pragma unroll
			for (int j = 0; j < PER; ++j)
				sc[j] = (uint32_t)(kk[j] >> 32);
			uint32_t v = 0xFFFFFFFFu;
			if (p.k > 24) {
				v = wave_kth_smallest_u32<PER>(sc, r1);
			} else {
				for (uint32_t cnt = 0; cnt < r1;) {
					uint32_t mn = sc[0];
#pragma unroll
					for (int j = 1; j < PER; ++j)
						mn = min(mn, sc[j]);
					mn = wave_min_u32(mn);
					if (mn == 0xFFFFFFFFu)
						break;
					v = mn;
#pragma unroll
					for (int j = 0; j < PER; ++j) {
						const bool eq = sc[j] == mn;
						cnt += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(eq));
						sc[j] = eq ? 0xFFFFFFFFu : sc[j];
					}
				}
			}
			// the first round's keys to the front of the list, the others behind them
#pragma unroll
			for (int j = 0; j < PER; ++j) {
				const bool hit = lane + 64 * j < (int)c && (uint32_t)(kk[j] >> 32) <= v;
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
				const uint32_t pos = n1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
				                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
				if (hit)
					list[pos] = kk[j];
				n1 += (uint32_t)__builtin_popcountll(mask);
			}
			uint32_t n_o = n1;
#pragma unroll
			for (int j = 0; j < PER; ++j) {
				const bool hit = lane + 64 * j < (int)c && (uint32_t)(kk[j] >> 32) > v;
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
				const uint32_t pos = n_o + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
				                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
				if (hit)
					list[pos] = kk[j];
				n_o += (uint32_t)__builtin_popcountll(mask);
			}
			n_s = n1;
		}
	}
	if (!TWO || n1 == 0) {
		n_s = 0;
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			const bool hit = lane + 64 * j < (int)c && key_score(kk[j]) <= cutoff;
			const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
			const uint32_t pos = n_s + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			if (hit)
				list[pos] = kk[j];
			n_s += (uint32_t)__builtin_popcountll(mask);
		}
	}
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: LDS ops are in order)
	auto rescore = [&](uint32_t begin) {
		// exact re-score, two candidates per 16-lane group in flight; slot i is read and rewritten
		// by the one group that owns it.  (Lists with final scores -- the 8-bit forms -- skip it.)
		for (uint32_t i0 = begin; p.rerank_base && i0 < n_s; i0 += 16) {
			constexpr int U = 4;  // candidates per 16-lane group in flight
			float acc[U];
			uint32_t row[U];
			const TR* r[U];
#pragma unroll
			for (int u = 0; u < U; ++u) {
				const uint32_t i = i0 + 4 * u + grp;
				row[u] = key_idx(list[i < n_s ? i : 0]);
				r[u] = (const TR*)p.rerank_base + (size_t)row[u] * p.dim + l;
				acc[u] = 0.0f;
			}
			// 8 dims of every candidate are requested before any is consumed (the trip count is a
			// run-time value: without this the loop waits for each load in turn); per candidate the
			// FMA chain still runs over t in increasing order, as the reference's lane does
			const uint32_t nt = p.dim / 16;
			for (uint32_t t0 = 0; t0 < nt; t0 += 8) {
				float qv[8];
				TR rv[U][8];
#pragma unroll
				for (int t = 0; t < 8; ++t)
					qv[t] = t0 + t < nt ? q[16 * (t0 + t)] : 0.0f;
#pragma unroll
				for (int u = 0; u < U; ++u)
#pragma unroll
					for (int t = 0; t < 8; ++t)
						rv[u][t] = t0 + t < nt ? r[u][16 * (t0 + t)] : (TR)0.0f;
#pragma unroll
				for (int u = 0; u < U; ++u)
#pragma unroll
					for (int t = 0; t < 8; ++t) {
						if (t0 + t >= nt)
							continue;  // (d = 64: four dims per lane)
						if (p.metric_ip) {
							acc[u] = ref_dot<TR>(qv[t], rv[u][t], acc[u]);
						} else {
							const float diff = ref_diff<TR>(qv[t], rv[u][t]);
							acc[u] = __builtin_fmaf(diff, diff, acc[u]);
						}
					}
			}
#pragma unroll
			for (int u = 0; u < U; ++u) {
				acc[u] = reduce16_ref_order(acc[u]);
				const uint32_t i = i0 + 4 * u + grp;
				if (l == 0 && i < n_s)
					list[i] = make_key(p.metric_ip ? -acc[u] : acc[u], row[u]);
			}
		}
	};
	rescore(0);
	if (TWO && n1 != 0) {
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		// T = the k-th smallest exact score of the first round (n1 >= r1 >= k keys; not finite: no cut)
		uint32_t t_ord;
		if (n1 <= 64) {
			const uint32_t w[1] = {lane < (int)n1 ? (uint32_t)(list[lane] >> 32) : 0xFFFFFFFFu};
			t_ord = wave_kth_smallest_u32<1>(w, p.k);
		} else {
			uint32_t w[PER];
#pragma unroll
			for (int j = 0; j < PER; ++j)
				w[j] = lane + 64 * j < (int)n1 ? (uint32_t)(list[lane + 64 * j] >> 32) : 0xFFFFFFFFu;
			t_ord = wave_kth_smallest_u32<PER>(w, p.k);
		}
		float cut = __builtin_inff();
		if (t_ord < 0xFF800000u)
			cut = i8f_round2_cut(ordered_to_float(t_ord), p.tau_f[qi], p.inv_2s2);
		// the second round: the others that can still reach T, compacted in place behind the first round's keys (a
		// key moves towards the front, and every lane has read its key before any lane writes)
		for (uint32_t i0 = n1; i0 < c; i0 += 64) {
			const uint32_t i = i0 + lane;
			const uint64_t key = list[i < c ? i : 0];
			const bool hit = i < c && !(key_score(key) > cut);
			const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
			const uint32_t pos = n_s + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			if (hit)
				list[pos] = key;
			n_s += (uint32_t)__builtin_popcountll(mask);
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		rescore(n1);
	}
	if (p.rerank_cnt && p.rerank_base && lane == 0)
		p.rerank_cnt[qo] = (p.slot_map ? p.rerank_cnt[qo] : 0u) + n_s;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	if (n_s <= 256)
		wave_emit_sorted<(PER < 4 ? PER : 4)>(p, list, n_s, qo, lane);
	else
		wave_emit_sorted<PER>(p, list, n_s, qo, lane);
}

// lists of at most 64 * PER keys; WAVES queries per workgroup (PER = 32: one, its list is 16 KB)
template <int PER, int WAVES, typename TR = float, bool TWO = false>
__global__ __launch_bounds__(64 * WAVES) void select_wave_kernel(SelectParams p, uint32_t m) {
	constexpr uint32_t kSelectWaveMax = 64 * PER;
	__shared__ uint64_t lists[WAVES][kSelectWaveMax];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.x * WAVES + wave;
	if (qi >= m)
		return;
	const uint32_t c = p.cand_cnt ? p.cand_cnt[qi] : p.fixed_count;
	if (c > kSelectWaveMax || c > p.cap || (c <= p.wave_done && p.wave_done != 0))
		return;  // longer lists: the next size up; shorter ones: already served
	select_wave_body<PER, TR, TWO>(p, qi, c, lists[wave], lane);
}

// One workgroup per query: bitonic sort of the (power-of-two padded) key list in LDS.
// (select_topk_kernel<float>: the rows behind rerank_base are float; <_Float16>: the rows of an EXPANN_DTYPE_F16 index)
// (TWO: the wave path's two-round instances, for the int8 filter's lists)
template <typename TR, bool TWO = false>
__global__ __launch_bounds__(kBlock) void select_topk_kernel(SelectParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	uint64_t* keys = reinterpret_cast<uint64_t*>(smem_raw);
	const uint32_t qi = blockIdx.x;
	const uint32_t tid = threadIdx.x;
	if (p.live_slots && qi >= (*p.live_slots & kRedoCountMask))
		return;  // (redo pass: a slot no failing query took)
	const uint32_t qo = p.slot_map ? p.slot_map[qi] : qi;
	uint32_t c = p.cand_cnt ? p.cand_cnt[qi] : p.fixed_count;
	if (p.redo_cand && tid == 0)
		atomicAdd(p.redo_cand, c);
	if (p.wave_done && c <= p.wave_done && c <= p.cap)
		return;  // served by a wave kernel (those leave overflowed lists, c > cap, to this one)
	if (p.wave0_short && c <= 2048 && c <= p.cap && 8 * (size_t)p.cap >= 16384) {
		// few queries in the launch: no separate wave kernels; wave 0 of this workgroup takes the
		// short list, the other waves leave
		if (tid < 64) {
			if (c <= 512)
				select_wave_body<8, TR, TWO>(p, qi, c, keys, (int)tid);
			else
				select_wave_body<32, TR, TWO>(p, qi, c, keys, (int)tid);
		}
		return;
	}
	if (c > p.cap) {
		if (tid == 0)
			atomicAdd(p.overflow, p.live_slots ? kRedoOverflowUnit : 1u);
		c = p.cap;
	}
	uint32_t n2 = 2;
	while (n2 < c)
		n2 <<= 1;
	const uint64_t* src = p.cand + (size_t)qi * p.cap;
	for (uint32_t i = tid; i < n2; i += kBlock)
		keys[i] = i < c ? src[i] : kSentinelKey;
	__syncthreads();
	auto bitonic = [&](uint32_t len) {
		for (uint32_t size = 2; size <= len; size <<= 1) {
			for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
				for (uint32_t i = tid; i < (len >> 1); i += kBlock) {
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
	};
	if (p.rerank_base) {
		const uint32_t l = tid & 15, grp = tid >> 4;  // 16 lanes per candidate row
		const float* q = p.rerank_queries + (size_t)qo * p.dim + l;
		uint32_t n_rescore = c;
		if ((p.prune_eps > 0.0f || p.row_w) && c > p.k) {
			// order by the approximate key, keep what can still reach the k best
			bitonic(n2);
			float cutoff;
			if (p.row_w) {
				// the k-th smallest upper bound is at most the largest of the first k keys' (sorted by kappa)
				uint32_t* s_max = reinterpret_cast<uint32_t*>(keys + p.cap) + 1;
				if (tid == 0)
					*s_max = 0;
				__syncthreads();
				uint32_t mx = 0;
				for (uint32_t i = tid; i < p.k; i += kBlock)
					mx = max(mx, i8f_upper_ord(p, keys[i]));
				if (mx)
					atomicMax(s_max, mx);
				__syncthreads();
				cutoff = i8f_cutoff(*s_max, p.q_w[qi]);
			} else {
				float qn = 0.0f;
				for (uint32_t t = 0; t < p.dim / 16; ++t)
					qn = __builtin_fmaf(q[16 * t], q[16 * t], qn);
				qn = reduce16_ref_order(qn);
				const float bmax = p.bn_max[0];
				cutoff = key_score(keys[p.k - 1]) + p.prune_eps * (qn + 1.5f * bmax) +
				         p.prune_abs * (__builtin_sqrtf(qn) + __builtin_sqrtf(bmax));
			}
			uint32_t cnt = 0;
			for (uint32_t i = tid; i < c; i += kBlock)
				cnt += key_score(keys[i]) <= cutoff ? 1u : 0u;
			// (counter lives behind the keys in the dynamic LDS region: a static __shared__ object
			// would shift the 16-byte alignment of the dynamic base)
			uint32_t* s_cnt = reinterpret_cast<uint32_t*>(keys + p.cap);
			if (tid == 0)
				*s_cnt = 0;
			__syncthreads();
			if (cnt)
				atomicAdd(s_cnt, cnt);
			__syncthreads();
			n_rescore = *s_cnt;  // keys are sorted: exactly the first *s_cnt qualify
			__syncthreads();
		}
		if (p.rerank_cnt && tid == 0)
			p.rerank_cnt[qo] = (p.slot_map ? p.rerank_cnt[qo] : 0u) + n_rescore;
		uint32_t n2r = 2;
		while (n2r < n_rescore)
			n2r <<= 1;
		// exact re-score: lane l owns dims l, l+16, ... in increasing order and the partial sums
		// meet in the _mm512_reduce_add_ps tree: bit-identical to scan_filter_f32_kernel's scores
		// (src/distance.h:136-147 / :181-190)
		for (uint32_t i0 = 0; i0 < n2r; i0 += kBlock / 16) {
			const uint32_t i = i0 + grp;
			const bool live = i < n_rescore;
			const uint32_t row = live ? key_idx(keys[i]) : 0u;
			const TR* r = (const TR*)p.rerank_base + (size_t)row * p.dim + l;
			float acc = 0.0f;
			for (uint32_t t = 0; t < p.dim / 16; ++t) {
				if (p.metric_ip) {
					acc = ref_dot<TR>(q[16 * t], r[16 * t], acc);
				} else {
					const float diff = ref_diff<TR>(q[16 * t], r[16 * t]);
					acc = __builtin_fmaf(diff, diff, acc);
				}
			}
			acc = reduce16_ref_order(acc);
			__syncthreads();  // every key of this pass has been read before any is overwritten
			if (l == 0 && i < n2r)
				keys[i] = live ? make_key(p.metric_ip ? -acc : acc, row) : kSentinelKey;
		}
		__syncthreads();
		n2 = n2r;
	}
	bitonic(n2);
	for (uint32_t i = tid; i < p.k; i += kBlock) {
		const uint64_t key = i < n2 ? keys[i] : kSentinelKey;
		const bool ok = key != kSentinelKey;
		if (p.out_ids)
			p.out_ids[(size_t)qo * p.k + i] = ok ? (uint64_t)key_idx(key) + p.id_offset : ~0ull;
		if (p.out_dists)
			p.out_dists[(size_t)qo * p.k + i] = ok ? key_score(key) : __builtin_inff();
	}
	if (tid == 0) {
		const uint64_t key = (p.k - 1 < n2) ? keys[p.k - 1] : kSentinelKey;
		spec_check(p, qo, key != kSentinelKey, key_score(key));
	}
	if (tid == 0 && p.tau_out) {
		const uint64_t key = (p.k - 1 < n2) ? keys[p.k - 1] : kSentinelKey;
		p.tau_out[qi] = key != kSentinelKey ? key_score(key)
		                                    : (p.tau_prev ? p.tau_prev[qi] : __builtin_inff());
		if (p.tau_row_out)
			p.tau_row_out[qi] = key != kSentinelKey
			                        ? key_idx(key)
			                        : (p.tau_row_prev ? p.tau_row_prev[qi] : 0xFFFFFFFFu);
	}
}

// max of a float array (single workgroup; used once per build for the rerank pruning bound)
__global__ __launch_bounds__(1024) void max_f32_kernel(const float* in, size_t n, float* out) {
	__shared__ float red[16];
	float m = -__builtin_inff();
	for (size_t i = threadIdx.x; i < n; i += 1024)
		m = in[i] > m ? in[i] : m;
	for (int off = 32; off > 0; off >>= 1) {
		const float o = __shfl_xor(m, off);
		m = o > m ? o : m;
	}
	if ((threadIdx.x & 63) == 0)
		red[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 16; ++w)
			m = red[w] > m ? red[w] : m;
		out[0] = m;
	}
}

// k-way merge of n_lists ascending (score, id) lists per query: ONE WAVE per query, every element
// finds its own place.  Lists are padded with (+inf, UINT64_MAX); order: score, then id (64-bit),
// then list number (distinct shards never tie on an id).  List g starts at in_ids + g*ids_stride /
// in_dists + g*dists_stride (elements): m*k each for separate [n_lists][m][k] arrays, the chunk size
// when every rank's chunk is [ids | dists], or the slice stride of the all-to-all exchange.
// Element i of list g has rank i + sum over the other lists of (entries ordered before it) -- a
// binary search per list in the sorted lists, no serial k-step chain (round 2's one-thread-per-query
// merge walked k x n_lists dependent global loads: latency-bound whatever m is, and its per-list
// cursor array lived in scratch).  STAGE: the n_lists x k entries of the query are first copied to
// LDS (12 B each) and searched there; else they are searched where they lie (lists too long for LDS).
template <bool STAGE>
__global__ __launch_bounds__(kWave) void merge_topk_kernel(const uint64_t* in_ids, const float* in_dists,
                                                            size_t ids_stride, size_t dists_stride,
                                                            uint32_t n_lists, uint32_t m, uint32_t k,
                                                            uint64_t* out_ids, float* out_dists) {
	extern __shared__ __attribute__((aligned(16))) unsigned char merge_smem[];
	const uint32_t qi = blockIdx.x, lane = threadIdx.x;
	if (qi >= m)
		return;
	const uint32_t total = n_lists * k;
	uint64_t* const s_id = reinterpret_cast<uint64_t*>(merge_smem);            // [total]
	uint32_t* const s_sc = reinterpret_cast<uint32_t*>(merge_smem + 8 * (size_t)total);  // [total]
	const size_t qoff = (size_t)qi * k;
	auto load = [&](uint32_t g, uint32_t i, uint64_t& id, uint32_t& sc) {
		if (STAGE) {
			id = s_id[g * k + i];
			sc = s_sc[g * k + i];
		} else {
			id = in_ids[g * ids_stride + qoff + i];
			sc = id == ~0ull ? 0xFFFFFFFFu : float_to_ordered(in_dists[g * dists_stride + qoff + i]);
		}
	};
	uint32_t n_valid = 0;
	if (STAGE) {
		for (uint32_t e = lane; e < total; e += kWave) {
			const uint32_t g = e / k, i = e - g * k;
			const uint64_t id = in_ids[g * ids_stride + qoff + i];
			s_id[e] = id;
			s_sc[e] = id == ~0ull ? 0xFFFFFFFFu : float_to_ordered(in_dists[g * dists_stride + qoff + i]);
		}
		__syncthreads();
	}
	for (uint32_t e = lane; e < total; e += kWave) {
		const uint32_t g = e / k, i = e - g * k;
		uint64_t id;
		uint32_t sc;
		load(g, i, id, sc);
		if (id == ~0ull)
			continue;  // padding: behind every real entry
		n_valid++;
		uint32_t rank = i;
		for (uint32_t g2 = 0; g2 < n_lists && rank < k; ++g2) {
			if (g2 == g)
				continue;
			// entries of list g2 ordered before (sc, id, g): none beyond position k - rank matter
			uint32_t lo = 0, hi = k - rank;
			while (lo < hi) {
				const uint32_t mid = (lo + hi) >> 1;
				uint64_t xid;
				uint32_t xsc;
				load(g2, mid, xid, xsc);
				const bool before = xsc < sc || (xsc == sc && (xid < id || (xid == id && g2 < g)));
				if (before)
					lo = mid + 1;
				else
					hi = mid;
			}
			rank += lo;
		}
		if (rank < k) {
			out_ids[qoff + rank] = id;
			out_dists[qoff + rank] = ordered_to_float(sc);
		}
	}
	// fewer than k real entries in all lists together: pad the tail
	for (int off = 32; off > 0; off >>= 1)
		n_valid += __shfl_xor(n_valid, off);
	for (uint32_t r = n_valid + lane; r < k; r += kWave) {
		out_ids[qoff + r] = ~0ull;
		out_dists[qoff + r] = __builtin_inff();
	}
}

}  // namespace expann
