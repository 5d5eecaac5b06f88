// append_rows.hpp -- the device side of expann_append: the fp16 copy of a built index extended in place, and the
// digest that shows an extended copy to be the one a fresh build makes.
//
// append_f16_rows_kernel reads each new row ONCE from the base's tail and leaves, for that row, exactly what
// ensure_f16's four launches leave (convert_f16*_kernel, sqnorm*_kernel, max_f32_kernel, f16_terms_kernel twice):
// the scaled fp16 row, both row terms -- through f16_row_term, the one function f16_terms_kernel's row branch calls
// too -- and its share of max ||b||^2; and it reports max |v| of the new rows, which decides on the host whether the
// current scale is still the longer index's (bf_append.hpp).  It converts with the CURRENT scale, speculatively: when
// the scale turns out to have changed, what it wrote dies with the copy.
#pragma once
#include "common.hpp"
#include "scan_gemm_f16.hpp"

namespace expann {

struct AppendRowsParams {
	const void* rows;      // [n_new][d] the new rows in the base's tail (TS elements)
	uint32_t n_new, d, ld; // ld: row length of the fp16 copy (d, or d rounded up to 32 with zero columns past d)
	float scale;           // the copy's scale
	_Float16* out;         // [n_new][ld] the copy's tail
	float* bnorm;          // [n_new] lower row terms (d_bnorm_f16's tail)
	float* bns;            // [n_new] upper row terms (d_bns_f16's tail)
	float eps, abs_coef, mul;
	int ip;
	uint32_t* bnmax_bits;  // d_bnmax[2] as its bit pattern
	uint32_t* maxabs_bits; // <- bit pattern of max |v| over the new rows (zeroed by the caller)
};

// max of a value per lane over the workgroup; valid in thread 0
__device__ inline uint32_t block_max_u32(uint32_t b, uint32_t* red) {
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if ((threadIdx.x & 63) == 0)
		red[threadIdx.x >> 6] = b;
	__syncthreads();
	if (threadIdx.x == 0)
		for (int w = 1; w < kBlock / 64; ++w)
			b = red[w] > b ? red[w] : b;
	return b;
}

// 16 lanes per row, 16 rows per workgroup: sqnorm_any_kernel's FMA chain (lane l takes elements l, l + 16, ...) and
// reduce16_ref_order, so the norm has the bits a fresh build computes, at the compiled dims (sqnorm_kernel<D> is the
// same chain unrolled) and at the run-time ones.  One atomic per workgroup and array: norms are >= +0, so the unsigned
// order of their bit patterns is the float order; a NaN norm is left out, as max_f32_kernel's `>` leaves it out.
template <typename TS>
__global__ __launch_bounds__(kBlock) void append_f16_rows_kernel(AppendRowsParams p) {
	__shared__ uint32_t red[2][kBlock / 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const bool live = i < p.n_new;
	const uint32_t ii = live ? i : p.n_new - 1;
	const TS* src = (const TS*)p.rows + (size_t)ii * p.d + l;
	_Float16* dst = p.out + (size_t)ii * p.ld + l;
	float acc = 0.0f;
	uint32_t b = 0;
	for (uint32_t t = 0; t < p.d / 16; ++t) {
		const float v = (float)src[16 * t];
		if (live)
			dst[16 * t] = (_Float16)(v * p.scale);
		acc = __builtin_fmaf(v, v, acc);
		const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
		b = vb > b ? vb : b;
	}
	if (live)
		for (uint32_t c = p.d + l; c < p.ld; c += 16)
			p.out[(size_t)i * p.ld + c] = (_Float16)0.0f;
	acc = reduce16_ref_order(acc);
	uint32_t nb = 0;
	if (live && l == 0) {
		p.bnorm[i] = f16_row_term(acc, p.eps, p.abs_coef, p.mul, p.ip);
		p.bns[i] = f16_row_term(acc, -p.eps, -p.abs_coef, p.mul, p.ip);
		if (acc == acc)
			nb = __builtin_bit_cast(uint32_t, acc);
	}
	b = block_max_u32(live ? b : 0u, red[0]);
	nb = block_max_u32(nb, red[1]);
	if (threadIdx.x == 0) {
		if (b != 0)
			atomicMax(p.maxabs_bits, b);
		if (nb != 0)
			atomicMax(p.bnmax_bits, nb);
	}
}

// ---- the digest of the fp16 copy ("copies_digest") ------------------------------------------------------------
// sum mod 2^64 of mix(array, word index, word) over: the copy's rows [0, n_pad) x ld as 32-bit words, both row-term
// arrays over [0, n_pad), max ||b||^2 and the scale.  A sum, so the order in which workgroups arrive does not show.
__host__ __device__ inline uint64_t digest_mix64(uint64_t x) {  // (splitmix64's finaliser)
	x += 0x9E3779B97F4A7C15ull;
	x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
	x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t digest_term(uint32_t array, uint64_t index, uint32_t word) {
	return digest_mix64(digest_mix64(((uint64_t)array << 56) ^ index) ^ (uint64_t)word);
}
struct CopiesDigestParams {
	const uint32_t* rows;   // [n_row_words] the fp16 copy, two halves per word
	uint64_t n_row_words;
	const uint32_t* bnorm;  // [n_pad]
	const uint32_t* bns;    // [n_pad]
	uint64_t n_pad;
	const uint32_t* bnmax;  // d_bnmax[2]
	uint32_t scale_bits;
	unsigned long long* out;  // zeroed by the caller
};
__global__ __launch_bounds__(kBlock) void copies_digest_kernel(CopiesDigestParams p) {
	__shared__ uint64_t red[kBlock];
	uint64_t s = 0;
	const uint64_t total = p.n_row_words + 2 * p.n_pad;
	for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
		if (i < p.n_row_words)
			s += digest_term(1, i, p.rows[i]);
		else if (i < p.n_row_words + p.n_pad)
			s += digest_term(2, i - p.n_row_words, p.bnorm[i - p.n_row_words]);
		else
			s += digest_term(3, i - p.n_row_words - p.n_pad, p.bns[i - p.n_row_words - p.n_pad]);
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		s += digest_term(4, 0, p.bnmax[0]) + digest_term(5, 0, p.scale_bits);
	red[threadIdx.x] = s;
	__syncthreads();
	for (int off = kBlock / 2; off > 0; off >>= 1) {
		if ((int)threadIdx.x < off)
			red[threadIdx.x] += red[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		atomicAdd(p.out, (unsigned long long)red[0]);
}

}  // namespace expann
