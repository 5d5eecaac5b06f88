// scan_groups.hpp -- row groups of the brute-force engine (gfx950): the list kernel of a grouped search
// (expann_search_grouped) and its small helpers.
//
// A grouped batch names one group per query.  The host buckets the queries by group and, for every group of at
// most "group_list_rows" rows, cuts the work into items: one query tile (up to TQ queries of ONE group) against
// one row chunk (a range of 16-row steps of that group's slice of the directory's row array).  One launch serves
// every such group of the batch: THE GRID IS THE ITEM TABLE'S LENGTH, one workgroup per item -- no work counter,
// no atomics, no loop that pulls work (graph_flat_scan.hpp tells what a lane-0 atomic in front of a loop's back
// edge did).
//
// A list query owns a slot: slot s has the candidate list cand[s * cap ...], the counter cand_cnt[s], and belongs
// to the caller's query slot_query[s] (the select kernels' slot_map).  The slots of one group are consecutive, so
// an item names its queries as slot0 .. slot0 + nq - 1.  The kernel writes make_key(score, row) of list position
// p to cand[slot * cap + p], the sentinel key at the positions of its last step past the end of the list, and
// cand_cnt[slot] = the group's size; the select kernels finish from there (rerank_base == nullptr: final scores).
//
// Arithmetic: that of scan_filter_f32_any_kernel (scan_f32.hpp), so the keys are the reference's bits -- lane l of
// a 16-lane DPP row owns dims l, l + 16, ... of one row, v_fma_f32 in increasing order per query (ref_diff /
// ref_dot), reduce16_ref_order.  The tile's queries sit in LDS (TQ x dim floats, sized at launch).
#pragma once
#include "common.hpp"

namespace expann {

// one work item: 32 bytes, read through wave-uniform loads
struct GroupItem {
	uint32_t slot0;     // first list slot of the query tile
	uint32_t nq;        // queries of the tile, 1..TQ
	uint32_t list_off;  // the group's rows: group_rows[list_off, list_off + list_len)
	uint32_t list_len;
	uint32_t g0, g1;    // 16-row steps [g0, g1) of the list
	uint32_t pad[2];
};
static_assert(sizeof(GroupItem) == 32, "GroupItem");

struct GroupScanParams {
	const void* base;            // [n_rows][dim]
	uint32_t n_rows, dim;
	const void* queries;         // [m][dim], the caller's array
	const uint32_t* slot_query;  // [slots] the caller's query of each list slot
	const uint32_t* group_rows;  // the directory's row array (each group ascending)
	const GroupItem* items;      // [gridDim.x]
	uint32_t* cand_cnt;          // [slots]
	uint64_t* cand;              // [slots][cap]
	uint32_t cap;
};

constexpr int kGroupScanTQ = 8;

template <int TQ, bool IP, typename TR = float>
__global__ __launch_bounds__(kBlock) void group_list_scan_kernel(GroupScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char group_smem[];
	float* qs = reinterpret_cast<float*>(group_smem);  // [TQ][D]
	const uint32_t D = p.dim, DPL = D / 16;
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int l = lane & 15, rg = lane >> 4;
	const GroupItem it = p.items[blockIdx.x];
	const uint32_t slot0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.slot0);
	const uint32_t nq = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.nq);
	const uint32_t list_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.list_len);
	const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.g0);
	const uint32_t g1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.g1);
	const uint32_t* __restrict__ list = p.group_rows + (uint32_t)__builtin_amdgcn_readfirstlane((int)it.list_off);
	const TR* __restrict__ base = (const TR*)p.base;
	const float* __restrict__ queries = (const float*)p.queries;
	constexpr int U = sizeof(TR) == 2 ? 8 : 4;  // loads in flight per lane

	// the tile's queries -> LDS (a slot past nq repeats the last query; its keys are never written)
	for (uint32_t i = threadIdx.x; i < TQ * D; i += kBlock) {
		const uint32_t j = i / D;
		const uint32_t qi = p.slot_query[slot0 + (j < nq ? j : nq - 1)];
		qs[i] = queries[(size_t)qi * D + (i - j * D)];
	}
	if (g0 == 0 && threadIdx.x < nq)
		p.cand_cnt[slot0 + threadIdx.x] = list_len;
	__syncthreads();

	for (uint32_t g = g0; g < g1; ++g) {
		const uint32_t pos = g * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
		const uint32_t row = pos < list_len ? list[pos] : 0xFFFFFFFFu;
		const bool rvalid = row < p.n_rows;
		const TR* src = base + (size_t)(rvalid ? row : p.n_rows - 1) * D + l;
		const float* qsl = qs + l;
		float acc[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j)
			acc[j] = 0.0f;
		uint32_t t = 0;
		for (; t + U <= DPL; t += U) {  // (U loads in flight per lane)
			TR r[U];
#pragma unroll
			for (int u = 0; u < U; ++u)
				r[u] = src[16 * (t + u)];
#pragma unroll
			for (int u = 0; u < U; ++u)
#pragma unroll
				for (int j = 0; j < TQ; ++j) {
					const float qv = qsl[j * D + 16 * (t + u)];
					if (IP) {
						acc[j] = ref_dot<TR>(qv, r[u], acc[j]);
					} else {
						const float diff = ref_diff<TR>(qv, r[u]);
						acc[j] = __builtin_fmaf(diff, diff, acc[j]);
					}
				}
		}
		for (; t < DPL; ++t) {
			const TR rv = src[16 * t];
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				const float qv = qsl[j * D + 16 * t];
				if (IP) {
					acc[j] = ref_dot<TR>(qv, rv, acc[j]);
				} else {
					const float diff = ref_diff<TR>(qv, rv);
					acc[j] = __builtin_fmaf(diff, diff, acc[j]);
				}
			}
		}
		float s[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			const float red = reduce16_ref_order(acc[j]);
			s[j] = IP ? -red : red;
		}
		if (l == 0 && pos < p.cap) {
#pragma unroll
			for (int j = 0; j < TQ; ++j)
				if ((uint32_t)j < nq)
					p.cand[(size_t)(slot0 + j) * p.cap + pos] = rvalid ? make_key(s[j], row) : kSentinelKey;
		}
	}
}

// out[i] = in[idx[i]] over rows of row_words 32-bit words: the queries of one tier into contiguous staging
static __global__ __launch_bounds__(kBlock) void group_gather_rows_kernel(const uint32_t* __restrict__ in, const uint32_t* __restrict__ idx,
                                                                      uint32_t n_idx, uint32_t row_words, uint32_t* __restrict__ out) {
	const size_t total = (size_t)n_idx * row_words;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
		const size_t r = i / row_words;
		out[i] = in[(size_t)idx[r] * row_words + (i - r * row_words)];
	}
}

// the result rows of a tier back to the caller's rows: out[idx[i]] = in[i] (k cells per row; dists may be nullptr)
static __global__ __launch_bounds__(kBlock) void group_scatter_results_kernel(const uint64_t* __restrict__ in_ids, const float* __restrict__ in_dists,
                                                                          const uint32_t* __restrict__ idx, uint32_t n_idx, uint32_t k,
                                                                          uint64_t* __restrict__ out_ids, float* __restrict__ out_dists) {
	const size_t total = (size_t)n_idx * k;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
		const size_t r = i / k;
		const size_t o = (size_t)idx[r] * k + (i - r * k);
		out_ids[o] = in_ids[i];
		if (out_dists)
			out_dists[o] = in_dists[i];
	}
}

// padding for the queries whose group no row carries: rows idx[i] of the outputs
static __global__ __launch_bounds__(kBlock) void group_pad_rows_kernel(const uint32_t* __restrict__ idx, uint32_t n_idx, uint32_t k,
                                                                   uint64_t* __restrict__ out_ids, float* __restrict__ out_dists) {
	const size_t total = (size_t)n_idx * k;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
		const size_t r = i / k;
		const size_t o = (size_t)idx[r] * k + (i - r * k);
		out_ids[o] = ~0ull;
		if (out_dists)
			out_dists[o] = __builtin_inff();
	}
}

// the bitmap of one group from the labels: bit r & 31 of word r >> 5 = (groups[r] == label), zero from row n on;
// one thread per word (n_words covers whole tiles of the fp16 copy, as the row filter's own copy does)
static __global__ __launch_bounds__(kBlock) void group_bits_kernel(const uint32_t* __restrict__ groups, uint32_t n_rows, uint32_t label,
                                                               uint32_t* __restrict__ bits, uint32_t n_words) {
	const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
	if (w >= n_words)
		return;
	uint32_t v = 0;
	const uint32_t r0 = w * 32;
	for (uint32_t b = 0; b < 32; ++b)
		if (r0 + b < n_rows && groups[r0 + b] == label)
			v |= 1u << b;
	bits[w] = v;
}

}  // namespace expann
