// remove_rows.hpp -- the device side of expann_remove: the survivors of a built index compacted into allocations
// built aside (gfx950).
//
// The keep bitmap, its word ranks and compact_rows_kernel are keep_bitmap.hpp's (the graph's remove shares them).
// compact_rows_kernel moves a survivor's row as bytes, 16 per lane, whatever the dtype: the base row, and in a second
// launch the fp16 row together with the two row terms.  survivor_maxima_kernel is the norm pass: max ||b||^2 and
// max |v| over the survivors with the bits a fresh build computes (append_f16_rows_kernel's chain, nothing written
// per row).  The copy is wide and the norm pass reads 4 bytes per lane, as the build's sqnorm chain must: two
// launches, so that the bytes that move -- most of the traffic -- move at full width.
#pragma once
#include "append_rows.hpp"
#include "common.hpp"
#include "filter_rows.hpp"
#include "keep_bitmap.hpp"

namespace expann {

struct SurvivorMaximaParams {
	const void* rows;      // [n][d] the rows before the remove (TS elements)
	const uint32_t* bits;  // the keep bitmap
	uint32_t n, d;
	uint32_t* bnmax_bits;   // <- bit pattern of max ||b||^2 over the survivors (zeroed by the caller)
	uint32_t* maxabs_bits;  // <- bit pattern of max |v| over the survivors (zeroed by the caller)
};

// append_f16_rows_kernel's geometry and chain over the rows that stay: 16 lanes per row, sqnorm's FMA chain and
// reduce16_ref_order for the norm, a NaN norm left out (max_f32_kernel's `>`); the maximum of the values' bit
// patterns for max |v|, in which a NaN wins (maxabs_bits_kernel).  Maxima do not depend on the order of arrival, so
// a workgroup walks many 16-row groups (grid stride) and reduces once at its end: one pair of atomics per workgroup.
template <typename TS>
__global__ __launch_bounds__(kBlock) void survivor_maxima_kernel(SurvivorMaximaParams p) {
	__shared__ uint32_t red[2][kBlock / 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t n_groups = (p.n + kRowsPerGroup - 1) / kRowsPerGroup;
	uint32_t b = 0, nb = 0;
	for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		const uint32_t i = g * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
		const bool kept = i < p.n && ((p.bits[i >> 5] >> (i & 31)) & 1u);
		float acc = 0.0f;
		if (kept) {
			const TS* src = (const TS*)p.rows + (size_t)i * p.d + l;
#pragma unroll 8
			for (uint32_t t = 0; t < p.d / 16; ++t) {
				const float v = (float)src[16 * t];
				acc = __builtin_fmaf(v, v, acc);
				const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
				b = vb > b ? vb : b;
			}
		}
		acc = reduce16_ref_order(acc);
		if (kept && l == 0 && acc == acc) {
			const uint32_t ab = __builtin_bit_cast(uint32_t, acc);
			nb = ab > nb ? ab : nb;
		}
	}
	b = block_max_u32(b, red[0]);
	nb = block_max_u32(nb, red[1]);
	if (threadIdx.x == 0) {
		if (b != 0)
			atomicMax(p.maxabs_bits, b);
		if (nb != 0)
			atomicMax(p.bnmax_bits, nb);
	}
}

}  // namespace expann
