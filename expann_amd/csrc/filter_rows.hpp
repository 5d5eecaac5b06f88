// filter_rows.hpp -- the row filter of the brute-force engine (gfx950): set-time kernels.
//
// A filter is a bitmap over the local rows (bit r & 31 of word r >> 5).  The fp16 matrix-core
// filters and the fused direct fp16 passes already reject a row whose row term is NaN -- that is
// how the padding rows of the fp16 copy stay out of the lists and the class maxima -- so a
// filtered search hands them row terms that are NaN on every disallowed row
// (filter_row_terms_kernel) and nothing else about them changes.  The exact direct scan
// (scan_f32.hpp) reads the bitmap itself, or walks the compacted list of allowed rows made here.
//
// The engine's copy of the bitmap covers the padded row count of the fp16 copy and is zero from
// row n on (filter_count_kernel clears what the caller left there), so no kernel reads a word
// outside it and no padding row is ever allowed.
// (The kernels are `static`: expann_hip.hip and expann_graph.hip both include this header.)
#pragma once
#include "common.hpp"

namespace expann {

constexpr uint32_t kFilterSegs = 256;  // contiguous word segments of the two set-time passes (one workgroup each)

// words per segment for a bitmap of n_words
__host__ __device__ inline uint32_t filter_seg_words(uint32_t n_words) { return (n_words + kFilterSegs - 1) / kFilterSegs; }

// out[r] = allowed(r) ? in[r] : NaN over the n_pad floats of one row-term array (the NaN padding stays NaN:
// its bits are zero).  n_pad is a multiple of 32 and at most 32 x the words of `bits`.
static __global__ __launch_bounds__(kBlock) void filter_row_terms_kernel(const uint32_t* __restrict__ bits,
                                                                    const float* __restrict__ in, float* __restrict__ out,
                                                                    uint32_t n_pad) {
	for (size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x; r < n_pad; r += (size_t)gridDim.x * kBlock) {
		const bool ok = (bits[r >> 5] >> (r & 31)) & 1u;
		out[r] = ok ? in[r] : __builtin_nanf("");
	}
}

// Pass 1 over the engine's copy: bits from row n on are cleared, the allowed rows are counted per segment and in
// total, and the residues mod 32 that hold an allowed row are collected (a class of the sampled passes is
// (chunk, row mod 32): the planner needs to know how many classes a filter can fill).
// stat[0] = allowed rows, stat[1] = OR of all words; seg_cnt[kFilterSegs].  stat is zero on entry.
static __global__ __launch_bounds__(kBlock) void filter_count_kernel(uint32_t* __restrict__ bits, uint32_t n_rows, uint32_t n_words,
                                                                uint32_t* __restrict__ stat, uint32_t* __restrict__ seg_cnt) {
	__shared__ uint32_t s_cnt, s_or;
	if (threadIdx.x == 0)
		s_cnt = 0, s_or = 0;
	__syncthreads();
	const uint32_t spw = filter_seg_words(n_words);
	const uint32_t w0 = blockIdx.x * spw;
	const uint32_t w1 = (w0 + spw < n_words) ? w0 + spw : n_words;
	const uint32_t full = n_rows >> 5, tail = n_rows & 31;
	uint32_t cnt = 0, orv = 0;
	for (uint32_t w = w0 + threadIdx.x; w < w1; w += kBlock) {
		uint32_t v = bits[w];
		if (w >= full) {
			const uint32_t keep = (w == full && tail) ? ((1u << tail) - 1u) : 0u;
			if (v & ~keep)
				bits[w] = v & keep;
			v &= keep;
		}
		cnt += (uint32_t)__builtin_popcount(v);
		orv |= v;
	}
	if (cnt)
		atomicAdd(&s_cnt, cnt);
	if (orv)
		atomicOr(&s_or, orv);
	__syncthreads();
	if (threadIdx.x == 0) {
		seg_cnt[blockIdx.x] = s_cnt;
		if (s_cnt)
			atomicAdd(&stat[0], s_cnt);
		if (s_or)
			atomicOr(&stat[1], s_or);
	}
}

// Pass 2: the allowed rows in ascending order, every `stride`-th of them (by rank among the allowed rows):
// list[j] = the allowed row of rank j * stride.  stride = 1 gives the complete list (the list path of a very
// selective filter); a larger stride an even sample of the allowed rows (level 0 of the threshold ladder).
// Same segments as pass 1, whose counts place each workgroup.
static __global__ __launch_bounds__(kBlock) void filter_compact_kernel(const uint32_t* __restrict__ bits, uint32_t n_words,
                                                                  const uint32_t* __restrict__ seg_cnt, uint32_t stride,
                                                                  uint32_t* __restrict__ list, uint32_t list_cap) {
	__shared__ uint32_t s_part[kBlock];
	__shared__ uint32_t s_base;
	const uint32_t spw = filter_seg_words(n_words);
	const uint32_t w0 = blockIdx.x * spw;
	const uint32_t w1 = (w0 + spw < n_words) ? w0 + spw : n_words;
	// a thread's own run of words
	const uint32_t wpt = (spw + kBlock - 1) / kBlock;
	uint32_t a = w0 + threadIdx.x * wpt, b = a + wpt;
	a = a < w1 ? a : w1;
	b = b < w1 ? b : w1;
	uint32_t cnt = 0;
	for (uint32_t w = a; w < b; ++w)
		cnt += (uint32_t)__builtin_popcount(bits[w]);
	s_part[threadIdx.x] = cnt;
	if (threadIdx.x == 0) {
		uint32_t base = 0;
		for (uint32_t s = 0; s < blockIdx.x; ++s)
			base += seg_cnt[s];
		s_base = base;
	}
	__syncthreads();
	uint32_t rank = s_base;
	for (uint32_t t = 0; t < threadIdx.x; ++t)
		rank += s_part[t];
	for (uint32_t w = a; w < b; ++w) {
		uint32_t v = bits[w];
		while (v) {
			const uint32_t bit = (uint32_t)__builtin_ctz(v);
			v &= v - 1;
			if (rank % stride == 0 && rank / stride < list_cap)
				list[rank / stride] = w * 32 + bit;
			++rank;
		}
	}
}

// a filter that allows no row: the outputs are padding only
static __global__ __launch_bounds__(kBlock) void fill_pad_kernel(uint64_t* __restrict__ ids, float* __restrict__ dists, size_t n) {
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
		ids[i] = ~0ull;
		if (dists)
			dists[i] = __builtin_inff();
	}
}

}  // namespace expann
