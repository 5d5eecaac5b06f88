// keep_bitmap.hpp -- the keep bitmap of a remove and the compaction by it (gfx950): what expann_remove
// (remove_rows.hpp) and expann_graph_remove (graph_remove.hpp) share.
//
// A keep bitmap in the row filter's layout (filter_rows.hpp: whole 128-row tiles, zero from row n on) starts as all
// ones; remove_mark_kernel clears one bit per id.  filter_count_kernel then clears the tail and counts the survivors
// per segment, remove_word_rank_kernel turns those counts into word_rank[w] -- the survivors before word w, which is
// filter_compact_kernel's arithmetic written out as an array -- and the new id of survivor i is
//     word_rank[i >> 5] + popcount(bits[i >> 5] & ((1u << (i & 31)) - 1))          (bf_remove.hpp: new_id).
// compact_rows_kernel moves a survivor's row as bytes, 16 per lane, whatever the dtype.
// (The kernels are `static`: expann_hip.hip and expann_graph.hip both include this header.)
#pragma once
#include "bf_remove.hpp"
#include "common.hpp"
#include "filter_rows.hpp"
#include "host_common.hpp"

namespace expann {

constexpr uint32_t kCompactRowsPerBlock = 128;  // one tile of the bitmap (4 words) per workgroup

// One bit cleared per id.  The id is compared with n BEFORE the bitmap is touched: an id out of range raises *flag
// and reads or writes nothing else.  A repeated id clears a clear bit.
static __global__ __launch_bounds__(kBlock) void remove_mark_kernel(const uint64_t* __restrict__ ids, size_t n_ids, uint32_t n,
                                                               uint32_t* __restrict__ bits, uint32_t* __restrict__ flag) {
	for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < n_ids; j += (size_t)gridDim.x * kBlock) {
		const uint64_t id = ids[j];
		if (id >= (uint64_t)n) {
			atomicOr(flag, 1u);
			continue;
		}
		const uint32_t r = (uint32_t)id;
		atomicAnd(&bits[r >> 5], ~(1u << (r & 31)));
	}
}

// word_rank[w] = set bits in the words before w.  filter_count_kernel's segments, whose counts place each workgroup,
// and filter_compact_kernel's run of words per thread.
static __global__ __launch_bounds__(kBlock) void remove_word_rank_kernel(const uint32_t* __restrict__ bits, uint32_t n_words,
                                                                    const uint32_t* __restrict__ seg_cnt,
                                                                    uint32_t* __restrict__ word_rank) {
	__shared__ uint32_t s_part[kBlock];
	__shared__ uint32_t s_base;
	const uint32_t spw = filter_seg_words(n_words);
	const uint32_t w0 = blockIdx.x * spw;
	const uint32_t w1 = (w0 + spw < n_words) ? w0 + spw : n_words;
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
		word_rank[w] = rank;
		rank += (uint32_t)__builtin_popcount(bits[w]);
	}
}

// The host side of the above: keep[2][words] -- the bitmap, then word_rank -- and stat[4 + kFilterSegs] -- {survivors,
// OR of the words, an id was out of range, a word for the caller}, then filter_count_kernel's segment counts.  Every
// step is enqueued on `st`; the caller reads stat()[0..3] back behind its own wait.
struct KeepBitmap {
	size_t n = 0, words = 0;  // rows covered; words of the bitmap (whole 128-row tiles)
	DevPtr<uint32_t> keep, stats;

	uint32_t* bits() const { return keep.get(); }
	uint32_t* word_rank() const { return keep.get() + words; }
	uint32_t* stat() const { return stats.get(); }

	// for n_rows rows, stat zeroed; the bits are the caller's to set: all_ones(), or a bitmap copied to bits()
	hipError_t alloc(size_t n_rows, hipStream_t st) {
		n = n_rows;
		words = keep_words(n_rows);
		HIP_OK(hipMalloc(&keep, sizeof(uint32_t) * std::max<size_t>(2 * words, 1)));
		HIP_OK(hipMalloc(&stats, sizeof(uint32_t) * (4 + kFilterSegs)));
		return hipMemsetAsync(stats, 0, sizeof(uint32_t) * (4 + kFilterSegs), st);
	}
	hipError_t all_ones(hipStream_t st) const { return words ? hipMemsetAsync(keep, 0xFF, sizeof(uint32_t) * words, st) : hipSuccess; }
	// one bit cleared per id (device memory); an id >= n raises stat()[2] instead
	void mark_ids(const uint64_t* d_ids, size_t n_ids, hipStream_t st) const {
		hipLaunchKernelGGL(remove_mark_kernel, dim3((uint32_t)std::min<size_t>((n_ids + kBlock - 1) / kBlock, 4096)), dim3(kBlock), 0,
		                   st, d_ids, n_ids, (uint32_t)n, bits(), stat() + 2);
	}
	// the tail cleared, stat()[0] = survivors, word_rank() filled
	void count_rank(hipStream_t st) const {
		hipLaunchKernelGGL(filter_count_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, bits(), (uint32_t)n, (uint32_t)words, stat(),
		                   stat() + 4);
		hipLaunchKernelGGL(remove_word_rank_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, (const uint32_t*)bits(), (uint32_t)words,
		                   (const uint32_t*)(stat() + 4), word_rank());
	}
};

struct CompactRowsParams {
	const uint32_t* bits;       // [n_tiles * 4] the keep bitmap
	const uint32_t* word_rank;  // [n_tiles * 4]
	const uint4* src;           // [n][chunks] the rows, 16 bytes a chunk
	uint4* dst;                 // [survivors][chunks]
	uint32_t chunks;            // 16-byte chunks per row (row bytes are a multiple of 16)
	const float *t0_src, *t1_src;  // one float per row carried along (the fp16 copy's two row terms), or nullptr
	float *t0_dst, *t1_dst;
};

// One workgroup per 128-row tile of the bitmap; the lanes walk the tile's chunks in order, so a wave reads 1 KiB
// runs of the source and writes runs that break only where a row was removed.  Rows from n on have a zero bit.
static __global__ __launch_bounds__(kBlock) void compact_rows_kernel(CompactRowsParams p) {
	__shared__ uint32_t s_bits[4], s_rank[4];
	if (threadIdx.x < 4) {
		s_bits[threadIdx.x] = p.bits[(size_t)blockIdx.x * 4 + threadIdx.x];
		s_rank[threadIdx.x] = p.word_rank[(size_t)blockIdx.x * 4 + threadIdx.x];
	}
	__syncthreads();
	const size_t row0 = (size_t)blockIdx.x * kCompactRowsPerBlock;
	const uint32_t total = kCompactRowsPerBlock * p.chunks;
	for (uint32_t j = threadIdx.x; j < total; j += kBlock) {
		const uint32_t r = j / p.chunks, c = j - r * p.chunks;
		const uint32_t word = s_bits[r >> 5], bit = r & 31;
		if (!((word >> bit) & 1u))
			continue;
		const size_t to = (size_t)s_rank[r >> 5] + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u));
		p.dst[to * p.chunks + c] = p.src[(row0 + r) * p.chunks + c];
		if (c == 0 && p.t0_src) {
			p.t0_dst[to] = p.t0_src[row0 + r];
			p.t1_dst[to] = p.t1_src[row0 + r];
		}
	}
}

}  // namespace expann
