// scan_gemm_f16.hpp -- the GEMM-form fp32 L2 candidate filter with ONE fp16 product per element
// on the matrix cores: a third of the MFMA work of the bf16x3 form (scan_gemm_bf16.hpp) and half its
// tile bytes.  This header holds the analysis and everything the fp16 kernels share; the kernels
// themselves are scan_gemm_f16x.hpp (d = 64 / 128), scan_gemm_f16kx.hpp (768 - 960) and the fp16 instances of
// scan_gemm_w8.hpp (256 / 512) and scan_gemm_kl.hpp (the dims known only at run time), all on v_mfma_f32_16x16x32_f16.
//
// Every value is scaled by a per-index power of two s (so that max|x|*s <= 2^15) and rounded
// once to fp16:  |x*s - fp16(x*s)| <= 2^-11 |x*s| + 2^-25  (normal + subnormal range).  Hence
//   |q.b - q16.b16 / s^2|  <=  (2^-10 + 2^-22) sum|q_i b_i|  +  2^-25/s * sum(|q_i| + |b_i|)
// and the squared-L2 test in expanded form keeps every row whose reference-order score is
// <= tau_q when evaluated with the slack
//      1.125 * 2^-10 * (||q||^2 + ||b||^2)  +  2^-24/s * sqrt(d) * (|q| + |b|)
// (the 12.5 % on top of 2^-10 covers the fp32 accumulation, the norms and the reference-order
// rounding, (4.25 d + 256) * 2^-24 at most, up to d = 256; beyond, gemm_f16_filter_eps(d) grows
// with d).  The slack admits ~10 % more candidates than the exact
// test; they are re-scored exactly by the select kernel, so ids and distances stay bit-identical
// to the direct scan.  Queries whose scaled components would leave the fp16 range make the
// engine use the bf16x3 form for that search.
//
// Layout / geometry: rows of d fp16 (2d bytes), staged by LDS-DMA as in scan_gemm_bf16.hpp.  A
// workgroup is 4 waves = 256 queries x 64 rows per step; each wave holds its 64 queries'
// fragments in registers and runs 2x2 MFMA tiles per step, so a row fragment read from LDS
// feeds two MFMAs.  Two workgroups share a CU (<= 80 KB of LDS, <= 256 VGPRs): the two waves on
// a SIMD belong to different workgroups with separate barriers, so one workgroup's barrier /
// epilogue / flush bubbles are covered by the other's MFMAs.
//
// The test  bn - 2 q.b <= theta_q  runs in the scaled domain: the accumulators START at
// theta'_q = theta_q s^2/2, the MFMAs add q16.b16, and a row passes when  acc >= bn'_b =
// bn_b s^2/2  -- one compare per pair, folded per lane into a v_max3 tree per 32x32 tile, so
// the common (no candidate) path costs 9 VALU instructions per tile.
//
// The fp16 copy of the index is padded to a multiple of 64 rows (zero rows whose bn' is NaN:
// no accumulator compares >= NaN), so staging needs no bounds handling.
#pragma once
#include "common.hpp"
#include "scan_gemm_bf16.hpp"
#include "scan_gemm_i8f.hpp"
#include "select.hpp"

namespace expann {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// relative slack of the filter on (||q||^2 + ||b||^2).  Beyond the input rounding (2^-10 + 2^-22)
// it has to cover, in units of u = 2^-24: d roundings of the fp32 accumulation at any association,
// each on a running magnitude <= |theta'| + sum|q16 b16| <= 4 (||q||^2 + ||b||^2) mul  (4d), the
// reference-order score (d/8 + 14), the two norms (d/16 + 5 each) and the threshold terms (~20):
// <= 4.25 d + 256.  Up to d = 256 the flat 12.5 % (2048 u) is at least that.
__host__ __device__ inline float gemm_f16_filter_eps(int d) {
	return d <= 256 ? 1.125f * 0.0009765625f
	                : 0.0009765625f + (4.0f + 4.25f * (float)d + 256.0f) * 5.9604644775390625e-08f;
}

// fp32 [n_values] * scale -> fp16 (round to nearest even); *maxabs_bits (optional, zeroed by the
// caller) receives the bit pattern of max |in| -- for non-negative floats the unsigned integer
// order is the float order, and a NaN (0x7fc00000 and up) wins, which the range check rejects
__global__ __launch_bounds__(kBlock) void convert_f16_kernel(const float* in, size_t n_values,
                                                             float scale, _Float16* out,
                                                             uint32_t* maxabs_bits) {
	uint32_t b = 0;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_values;
	     i += (size_t)gridDim.x * kBlock) {
		const float v = in[i];
		out[i] = (_Float16)(v * scale);
		const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
		b = vb > b ? vb : b;
	}
	if (maxabs_bits) {  // one atomic per workgroup
		__shared__ uint32_t red[kBlock / 64];
		for (int off = 32; off > 0; off >>= 1) {
			const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
			b = o > b ? o : b;
		}
		if ((threadIdx.x & 63) == 0)
			red[threadIdx.x >> 6] = b;
		__syncthreads();
		if (threadIdx.x == 0) {
			for (int w = 1; w < kBlock / 64; ++w)
				b = red[w] > b ? red[w] : b;
			if (b != 0)
				atomicMax(maxabs_bits, b);
		}
	}
}

// bit pattern of max |x| over an array (see convert_f16_kernel); *out zeroed by the caller
// (TS = the source's element type, here and in sqnorm_any_kernel / convert_f16_pad_kernel -- the prelude of an
// EXPANN_DTYPE_F16 index at every dim: _Float16 rows are converted to fp32 -- exactly -- and then treated as fp32
// rows are, so the scaled copy, the norms and max |x| are the bits an fp32 index of the same values gets)
template <typename TS = float>
__global__ __launch_bounds__(kBlock) void maxabs_bits_kernel(const TS* in, size_t n, uint32_t* out) {
	uint32_t b = 0;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
		const uint32_t v = __builtin_bit_cast(uint32_t, (float)in[i]) & 0x7fffffffu;
		b = v > b ? v : b;
	}
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if ((threadIdx.x & 63) == 0 && b != 0)
		atomicMax(out, b);
}

// out[i] = ||x_i||^2 (fp32, reference lane order); 16 lanes per row
template <int D>
__global__ __launch_bounds__(kBlock) void sqnorm_kernel(const float* x, uint32_t n, float* out) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t ii = i < n ? i : n - 1;
	const float* src = x + (size_t)ii * D + l;
	float acc = 0.0f;
#pragma unroll
	for (int t = 0; t < D / 16; ++t)
		acc = __builtin_fmaf(src[16 * t], src[16 * t], acc);
	acc = reduce16_ref_order(acc);
	if (i < n && l == 0)
		out[i] = acc;
}
// Query side of a search in ONE launch: scaled fp16 copy, ||q||^2 in the reference lane order and
// the bit pattern of max |q| (range check).  16 lanes per query row, as sqnorm_kernel.
// Latency mode (m <= 16: a single workgroup): q may be pinned host memory -- the kernel then also
// leaves a device copy in q_copy for the kernels that follow -- and zero_flags (the 8-word flag /
// statistics block that maxabs_bits points into) is cleared here instead of by a memset launch.
// Inner product (ip_ref != nullptr, round 3): the filter's slack eps (|q|^2 + |b|^2) bounds 2 eps |q| |b| tightly
// only when the two norms are alike.  Ranks under the inner product do not change when a query is multiplied by
// a positive constant, so the FILTER sees each query times a power of two c_q (exact) that brings |c_q q|^2 to
// *ip_ref (the largest row norm: the rows that reach a top-k under the inner product are the large ones):
// q16, qnrm and the range check are those of c_q q, qscale[i] = c_q; thresholds that arrive in true units are
// multiplied by it (f16_terms_kernel), the sampled pass's own are in the scaled domain already, and the exact
// re-rank reads the caller's queries.  (L2: c_q = 1.)
// i8f.q8 != nullptr (int8 filter, scan_gemm_i8f.hpp): the same launch also writes q~ and the query's terms.
template <int D>
__global__ __launch_bounds__(kBlock) void f16_query_prep_kernel(const float* q, uint32_t m, float scale,
                                                                _Float16* q16, float* qnrm,
                                                                uint32_t* maxabs_bits, float* q_copy,
                                                                uint32_t* zero_flags, const float* ip_ref,
                                                                float* qscale, I8fQueryArgs i8f) {
	__shared__ uint32_t red[kBlock / 64];
	if (zero_flags) {
		if (threadIdx.x < 8)
			zero_flags[threadIdx.x] = 0;
		__syncthreads();
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t ii = i < m ? i : m - 1;
	const float* src = q + (size_t)ii * D + l;
	float acc = 0.0f;
	uint32_t b = 0;
	float vals[D / 16];
#pragma unroll
	for (int t = 0; t < D / 16; ++t) {
		const float v = src[16 * t];
		vals[t] = v;
		acc = __builtin_fmaf(v, v, acc);
		const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
		b = vb > b ? vb : b;
	}
	acc = reduce16_ref_order(acc);
	acc = __shfl(acc, lane & ~15);  // (the reference order is the first lane's: one value for the 16 lanes)
	float c = 1.0f;
	if (ip_ref) {
		const float ref = ip_ref[0];
		if (acc > 0.0f && ref > 0.0f && acc < 3.0e38f && ref < 3.0e38f) {
			int e = (int)__builtin_rintf(0.5f * (__builtin_log2f(ref) - __builtin_log2f(acc)));
			e = e < -40 ? -40 : (e > 40 ? 40 : e);
			c = __builtin_ldexpf(1.0f, e);
		}
	}
#pragma unroll
	for (int t = 0; t < D / 16; ++t) {
		if (i < m) {
			q16[(size_t)i * D + l + 16 * t] = (_Float16)(vals[t] * c * scale);
			if (q_copy)
				q_copy[(size_t)i * D + l + 16 * t] = vals[t];
		}
	}
	if (i < m && l == 0) {
		qnrm[i] = acc * c * c;
		if (qscale)
			qscale[i] = c;
	}
	if (i8f.q8)  // (wave-uniform: the 16-lane sums inside need every lane)
		i8f_query_terms<D>(i8f, i, m, l, vals);
	b = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, b) * c);  // (max |c_q q|: what the fp16 range check is about)
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if (lane == 0)
		red[wave] = b;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kBlock / 64; ++w)
			b = red[w] > b ? red[w] : b;
		if (b != 0)
			atomicMax(maxabs_bits, b);
	}
}

// The prelude at a dim known at run time (scan_gemm_kl.hpp: the dims without a compiled fp16 form).
// The fp16 copies there have rows of ld = d rounded up to a multiple of 32 elements (whole MFMA k-steps),
// zero past d; norms and the range check are those of the d real elements.
// (_Float16 rows take this kernel at every dim: the same FMA chain and reduction as sqnorm_kernel<D>, same bits)
template <typename TS = float>
__global__ __launch_bounds__(kBlock) void sqnorm_any_kernel(const TS* x, uint32_t n, uint32_t d, float* out) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t ii = i < n ? i : n - 1;
	const TS* src = x + (size_t)ii * d + l;
	float acc = 0.0f;
	for (uint32_t t = 0; t < d / 16; ++t)
		acc = __builtin_fmaf((float)src[16 * t], (float)src[16 * t], acc);
	acc = reduce16_ref_order(acc);
	if (i < n && l == 0)
		out[i] = acc;
}
// fp32 [n][d] * scale -> fp16 [n][ld] (zero columns d .. ld-1)
template <typename TS = float>
__global__ __launch_bounds__(kBlock) void convert_f16_pad_kernel(const TS* in, size_t n, uint32_t d, uint32_t ld,
                                                                 float scale, _Float16* out) {
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n * ld; i += (size_t)gridDim.x * kBlock) {
		const size_t r = i / ld;
		const uint32_t c = (uint32_t)(i - r * ld);
		out[i] = c < d ? (_Float16)((float)in[r * d + c] * scale) : (_Float16)0.0f;
	}
}
// f16_query_prep_kernel<D> at run-time d: same outputs (q16 with rows of ld, zero-padded), same per-query
// ip_rescale power of two, same range flag, same one-workgroup latency path (zero_flags, q_copy).  The
// query is read twice (norm and max |q| first, then the scaled copy) instead of being held in registers.
__global__ __launch_bounds__(kBlock) void f16_query_prep_any_kernel(const float* q, uint32_t m, uint32_t d, uint32_t ld,
                                                                    float scale, _Float16* q16, float* qnrm,
                                                                    uint32_t* maxabs_bits, float* q_copy,
                                                                    uint32_t* zero_flags, const float* ip_ref,
                                                                    float* qscale) {
	__shared__ uint32_t red[kBlock / 64];
	if (zero_flags) {
		if (threadIdx.x < 8)
			zero_flags[threadIdx.x] = 0;
		__syncthreads();
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t ii = i < m ? i : m - 1;
	const float* src = q + (size_t)ii * d + l;
	float acc = 0.0f;
	uint32_t b = 0;
	for (uint32_t t = 0; t < d / 16; ++t) {
		const float v = src[16 * t];
		acc = __builtin_fmaf(v, v, acc);
		const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
		b = vb > b ? vb : b;
	}
	acc = reduce16_ref_order(acc);
	acc = __shfl(acc, lane & ~15);
	float c = 1.0f;
	if (ip_ref) {
		const float ref = ip_ref[0];
		if (acc > 0.0f && ref > 0.0f && acc < 3.0e38f && ref < 3.0e38f) {
			int e = (int)__builtin_rintf(0.5f * (__builtin_log2f(ref) - __builtin_log2f(acc)));
			e = e < -40 ? -40 : (e > 40 ? 40 : e);
			c = __builtin_ldexpf(1.0f, e);
		}
	}
	if (i < m) {
		for (uint32_t t = 0; t < ld / 16; ++t) {
			const uint32_t col = l + 16 * t;
			const float v = col < d ? src[16 * t] : 0.0f;
			q16[(size_t)i * ld + col] = (_Float16)(v * c * scale);
			if (q_copy && col < d)
				q_copy[(size_t)i * d + col] = v;
		}
		if (l == 0) {
			qnrm[i] = acc * c * c;
			if (qscale)
				qscale[i] = c;
		}
	}
	b = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, b) * c);
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if (lane == 0)
		red[wave] = b;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kBlock / 64; ++w)
			b = red[w] > b ? red[w] : b;
		if (b != 0)
			atomicMax(maxabs_bits, b);
	}
}

// The row term of a row with ||b||^2 = v (the formulas: f16_terms_kernel's comment below): what a build writes
// (f16_terms_kernel, tau == nullptr) and what an append writes for a new row (append_rows.hpp) -- one function, so
// that an extended array holds the bits a fresh build computes.  Its roundings are spelled out, because contraction
// into an FMA is otherwise decided per call site and the two kernels differed in the last bit.  They are the ones
// f16_terms_kernel's row branch compiled to before the function existed, so a build writes the row terms it always
// wrote: L2 rounds every operation on its own (v_pk_mul_f32 of both products, v_sub_f32); the inner product fuses
// eps v into the sum, e = fma(v, eps, abs sqrt(v)) (v_mul_f32, v_fmac_f32, then the sign flip).
__device__ __attribute__((always_inline)) inline float f16_row_term(float v, float eps, float abs_coef, float mul, int ip) {
#pragma clang fp contract(off)
	if (ip) {
		const float e = __builtin_fmaf(v, eps, abs_coef * __builtin_sqrtf(v));
		return -e * mul;
	}
	const float t = v * (1.0f - eps) - abs_coef * __builtin_sqrtf(v);
	return t * mul;
}

// rows:    out = (nrm*(1-eps) - abs*sqrt(nrm)) * mul                (tau == nullptr: f16_row_term)
// queries: out = (tau - (nrm*(1-eps) - abs*sqrt(nrm))) * mul
// mul = s^2/2, a power of two: the scaling is exact
// (eps, abs_coef negated: the UPPER row term (nrm*(1+eps) + abs*sqrt(nrm)) * mul of the sampled pass)
//
// Inner product (score = -q.b, ip != 0): |q.b - q16.b16/s^2| <= E/2 with the same
// E = eps (||q||^2 + ||b||^2) + abs (|q| + |b|), so with e(v) = eps v + abs sqrt(v):
//   rows:    out = -e(nrm) * mul          queries: out = (2 tau + e(nrm)) * mul
// and the kernel's test acc = theta' + q16.b16 >= bn' keeps every row with -q.b <= tau.
// (qscale: the queries' filter-side factors c_q of f16_query_prep_kernel -- inner product only, nullptr = 1 -- :
// nrm is already that of c_q q, a threshold in true units becomes c_q tau)
__global__ __launch_bounds__(kBlock) void f16_terms_kernel(const float* nrm, uint32_t n, float eps,
                                                           float abs_coef, const float* tau,
                                                           float mul, float* out, int ip, const float* qscale) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n)
		return;
	const float v = nrm[i];
	if (!tau) {
		out[i] = f16_row_term(v, eps, abs_coef, mul, ip);
		return;
	}
	if (ip) {
		const float e = v * eps + abs_coef * __builtin_sqrtf(v);
		out[i] = (2.0f * tau[i] * (qscale ? qscale[i] : 1.0f) + e) * mul;
		return;
	}
	const float t = v * (1.0f - eps) - abs_coef * __builtin_sqrtf(v);
	out[i] = (tau[i] - t) * mul;
}

struct GemmF16Params {
	const void* base_f16;    // [n_rows padded to 64][D] fp16, scaled by s
	const float* bnorm;      // [n_rows padded to 64] (||b||^2 (1-eps) - abs*|b|) * s^2/2; NaN padding
	uint32_t n_rows;
	uint32_t n_tiles_sel;
	uint32_t tile_stride;
	uint32_t tile_run;
	uint32_t tiles_per_block;
	uint32_t n_qtiles;
	const void* queries_f16; // [m][D] fp16, scaled by s
	const float* theta;      // [m] (tau - ||q||^2 (1-eps) + abs*|q|) * s^2/2
	float two_inv_s2;        // 2 / s^2 (exact: s is a power of two); inner product: 1 / s^2
	uint32_t m;
	uint32_t* cand_cnt;
	uint64_t* cand;
	uint32_t cap;
	uint32_t debug;          // ablation switches (bench only): 4 no epilogue, 8 no candidate path
	unsigned long long* clk; // [2] debug: shader-clock and 100 MHz ticks of workgroup 0 (or nullptr)
	// SAMPLE variant: out[(q * n_chunks + chunk) * 32 + c] = max over the chunk's rows of class c
	// (row mod 32) of g = q16.b16 - bn'  (larger g = nearer row); theta, cand* unused
	float* sample_out;
	uint32_t n_chunks;
	// blocks b and b+8 share an XCD (observed dispatch order): with xcd_map the 8 row chunks
	// {x, x+8, ...} and all their query tiles go to XCD x, so a tile is fetched into ONE L2
	// instead of eight.  Needs the chunk count to be a multiple of 8.
	uint32_t xcd_map;
	// scan_gemm_f16x_kernel only: row chunks of two sizes.  Chunks 0 .. n_big - 1 hold tiles_per_block
	// tiles, the chunks behind them tiles_small (0 = one size).  Workgroups start in block order, so
	// the launch ends on the small ones and drains in a third of the time (pick_tail_chunks).
	uint32_t n_big, tiles_small;
	// scan_gemm_f16x_kernel only: every wave appends its hits to a log of its own in global memory --
	// log[(4 blockIdx.x + wave) * log_cap + i] = {bn' - acc, row, query}, plain stores in the wave's own order, no
	// atomic and no returned value to wait for inside the MFMA kernel -- and leaves the count in
	// log_cnt; scatter_log_kernel then files the entries into the per-query lists (cand, cand_cnt).
	// *lost is incremented by a wave whose log or LDS queue overflowed (the host repeats the search
	// with scan_gemm_f16_kernel, whose direct appends have no such limit).
	uint4* log;
	uint32_t* log_cnt;
	uint32_t log_cap;
	uint32_t* lost;
	// scan_gemm_f16x_kernel only: persistent launch -- work_ctr[16 * x] = the next item of XCD x's queue
	// (zero at launch, one cache line each), n_items = the plain launch's grid; nullptr = plain launch
	uint32_t* work_ctr;
	uint32_t n_items;
	// scan_gemm_kl_kernel only: MFMA k-steps of 32 elements per row (the fp16 rows' length / 32)
	uint32_t ksteps;
	// scan_gemm_f16x_kernel's REDO instance only, the redo pass of the speculative thresholds: the m query slots are
	// compact copies of the failing queries; *live_q (low 20 bits) of them are taken -- a workgroup whose query
	// tile starts at or beyond that count leaves at once (the slots behind the count inside a tile hold theta' =
	// -inf).  nullptr: every query is live.
	const uint32_t* live_q;
};

// Per-wave hit logs -> per-query candidate lists.  The 64 queries of (query tile, wave w) receive
// hits from exactly the n_chunks logs of wave w in the workgroups (chunk, query tile); a workgroup
// here takes `chunks_per_block` of those logs: it counts its entries per query in LDS, reserves the
// slots of each query with ONE global atomicAdd (64 per workgroup instead of one per hit), then
// files the entries.  cand_cnt is zero when the kernel starts (sample_tau_kernel / the level's memset).
// grid = n_qtiles * 4 * n_groups; block index = (qtile * 4 + w) * n_groups + group.
struct GatherLogParams {
	const uint4* log;
	const uint32_t* log_cnt;
	uint32_t log_cap, n_chunks, n_qtiles, xcd_map, m;
	uint32_t n_groups, chunks_per_block;
	uint32_t* cand_cnt;
	uint64_t* cand;
	uint32_t cap;
	// fp16 logs (scan_gemm_f16x.hpp): an entry is {bits of bn' - acc, row, query}; the key is made HERE,
	// make_key((x + theta[query]) * key_mul, row) -- the arithmetic the scan's flush used to do behind a second
	// LDS round trip.
	const float* theta;
	float key_mul;
	// 8-bit logs (scan_gemm_i8w.hpp): an entry is {raw accumulator, row, query}; the exact integer score is made
	// HERE -- dot = acc - i_thp[query], L2 forms: i_bias[row] - 2 dot + i_qself[query], inner product: -dot --
	// instead of two global gathers per hit inside the MFMA kernel (whose vmcnt they shared with the stage
	// loads).  i_mode: 0 = not an 8-bit log, 1 = L2 forms, 2 = inner product.
	// i_mode 3, the int8 filter of fp32 rows (scan_gemm_i8f.hpp): the entry's fourth word is the row's bp (the scan
	// had it in a register), the key is kappa = bp - acc (units of 2 s^2), re-scored exactly by the select; -inf for a
	// row whose bp sits at a clamp limit -- a clamped row always does, and an unclamped row that lands exactly on a
	// limit is merely always re-scored.  No read of i_bias / i_rw per hit (two random 4-byte gathers, 2.1 M hits a
	// step at C2).  redo_stream_i8_kernel (scan_redo_i8.hpp) makes the same key where it files a hit.
	const int* i_thp;
	const int* i_bias;
	const int* i_qself;
	int i_mode;
	const float* i_rw;
	const uint32_t* live_q;  // redo pass of the fp16 form: as GemmF16Params::live_q (the query tiles no workgroup scanned have no
	                         // logs).  The int8 filter's redo scan files its own hits (scan_redo_i8.hpp) and has no gather
};
__global__ __launch_bounds__(kBlock) void gather_logs_kernel(GatherLogParams p) {
	__shared__ uint32_t cnt[64], base[64];
	const uint32_t grp = blockIdx.x % p.n_groups, qw = blockIdx.x / p.n_groups;
	const uint32_t qtile = qw >> 2, w = qw & 3;
	const uint32_t q0 = qtile * 256 + w * 64;
	if (p.live_q && qtile * 256 >= (*p.live_q & kRedoCountMask))
		return;
	if (threadIdx.x < 64)
		cnt[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint32_t c0 = grp * p.chunks_per_block;
	const uint32_t c1 = c0 + p.chunks_per_block < p.n_chunks ? c0 + p.chunks_per_block : p.n_chunks;
	auto log_of = [&](uint32_t c, uint32_t& n) -> const uint4* {
		const uint32_t bid = p.xcd_map ? ((c >> 3) * p.n_qtiles + qtile) * 8 + (c & 7) : c * p.n_qtiles + qtile;
		const uint32_t li = bid * 4 + w;
		n = p.log_cnt[li];
		if (n > p.log_cap)
			n = p.log_cap;
		return p.log + (size_t)li * p.log_cap;
	};
	for (uint32_t c = c0 + wv; c < c1; c += kBlock / 64) {  // one wave per log
		uint32_t n;
		const uint4* src = log_of(c, n);
		for (uint32_t i = lane; i < n; i += 64)
			atomicAdd(&cnt[(src[i].z - q0) & 63], 1u);
	}
	__syncthreads();
	if (threadIdx.x < 64) {
		const uint32_t n = cnt[threadIdx.x];
		base[threadIdx.x] = n ? atomicAdd(&p.cand_cnt[q0 + threadIdx.x], n) : 0u;
		cnt[threadIdx.x] = 0;
	}
	__syncthreads();
	for (uint32_t c = c0 + wv; c < c1; c += kBlock / 64) {
		uint32_t n;
		const uint4* src = log_of(c, n);
		for (uint32_t i = lane; i < n; i += 64) {
			const uint4 e = src[i];
			const uint32_t ql = (e.z - q0) & 63;
			const uint32_t slot = base[ql] + atomicAdd(&cnt[ql], 1u);
			if (slot < p.cap) {
				uint64_t key;
				if (p.i_mode == 3) {
					const int bp = (int)e.w;
					const float kappa = (float)(bp - (int)e.x);
					key = make_key(bp > kI8fBpMin && bp < kI8fBpMax ? kappa : -__builtin_inff(), e.y);
				} else if (p.i_mode) {
					const int dot = (int)e.x - p.i_thp[e.z];
					const int score = p.i_mode == 1 ? p.i_bias[e.y] - 2 * dot + p.i_qself[e.z] : -dot;
					key = make_key((float)score, e.y);
				} else {
					key = make_key((__builtin_bit_cast(float, e.x) + p.theta[e.z]) * p.key_mul, e.y);
				}
				p.cand[(size_t)e.z * p.cap + slot] = key;
			}
		}
	}
}

__device__ inline float max3f(float a, float b, float c) {
	return __builtin_fmaxf(__builtin_fmaxf(a, b), c);  // folds to v_max3_f32
}

// Wait until at most N of this wave's vector-memory operations (LDS-DMA stage loads) are still
// in flight and its LDS traffic has drained, then the workgroup barrier.  (__syncthreads() would
// drain the stage loads too: vmcnt(0).)
template <int N> __device__ inline void wait_vm_then_barrier() {
	asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

#ifndef EXPANN_F16_THREADS
#define EXPANN_F16_THREADS 256
#endif
constexpr int kF16Threads = EXPANN_F16_THREADS;  // 256: two workgroups per CU; 512: one
constexpr int kF16WgPerCu = 512 / kF16Threads;
constexpr int kF16Waves = kF16Threads / 64;
constexpr int kF16TQ = 64 * kF16Waves;       // queries per workgroup
static_assert(kF16Waves == 4 && kF16TQ == 256, "gather_logs_kernel files the logs of 4 waves x 64 queries per workgroup");
constexpr int kF16TB = 64;                   // rows per tile (= per workgroup step)
constexpr int kF16Prefetch = 2;              // tiles in flight ahead of the one being multiplied
constexpr int kF16Bufs = kF16Prefetch + 1;   // LDS tile buffers
constexpr int kF16WaveQueue = 88;            // candidate queue entries per wave, in LDS
constexpr int kF16EntryBytes = 80;
constexpr int kF16FlushEvery = 8;            // steps between looks at the queue fill
// Geometry by dimension (the int8 kernels use the same scheme, scan_gemm_i8q.hpp).  d = 64 / 128:
// 4 waves x 64 queries, two workgroups per CU.  d = 256: a wave's fragments of 64 queries would
// be 128 VGPRs, so 8 waves x 32 queries share each staged tile (one workgroup per CU), and the
// 16-byte chunks of a row go to (k-step, lane half) in natural order (2s + h): 8 fragment
// address registers serve all 16 k-steps.
template <int D> struct F16Geom {
	static constexpr int THREADS = D >= 256 ? 512 : kF16Threads;
	static constexpr int WAVES = THREADS / 64;
	static constexpr int TQW = D >= 256 ? 1 : 2;   // 32-query MFMA tiles per wave
	static constexpr int WGQ = WAVES * 32 * TQW;   // queries per workgroup
	static constexpr int NBUF = D >= 512 ? 2 : kF16Bufs;  // d = 512: two 64 KB tile buffers
	// d = 64: fragments of 64 queries are 32 VGPRs; with the accumulator start values read from
	// LDS each step the scan fits 168 VGPRs and THREE workgroups share a CU (as I8qGeom<128>)
	static constexpr bool TH_LDS = D == 64;
	static constexpr int QCAP = D >= 512 ? 32 : ((D >= 256 || TH_LDS) ? 56 : kF16WaveQueue);
	static constexpr bool NATURAL = D >= 256;
	static constexpr int WG_PER_CU = TH_LDS ? 3 : 512 / THREADS;
};
static_assert(F16Geom<128>::WGQ == kF16TQ && F16Geom<256>::WGQ == kF16TQ, "one query-tile size");
template <int D> constexpr int gemm_f16_lds_bytes() {
	using G = F16Geom<D>;
	// tiles + per-wave bn' slots + per-wave candidate queues + theta' + queue fills
	return G::NBUF * (kF16TB * D * 2 + G::WAVES * 256) + G::WAVES * G::QCAP * kF16EntryBytes + G::WGQ * 4 + 64 +
	       (G::TH_LDS ? G::WAVES * 2 * G::TQW * 16 * 4 : 0);
}
static_assert(gemm_f16_lds_bytes<64>() * 3 <= 160 * 1024 &&
                  gemm_f16_lds_bytes<128>() * F16Geom<128>::WG_PER_CU <= 160 * 1024 &&
                  gemm_f16_lds_bytes<256>() <= 160 * 1024 && gemm_f16_lds_bytes<512>() <= 160 * 1024,
              "LDS budget per CU");

// (Rounds 1-2 ran this filter -- full scan and sampled pass -- on v_mfma_f32_32x32x16_f16 in a kernel of this
// file, scan_gemm_f16_kernel<D, SAMPLE>; since round 3 every fp16 stream is one of the 16 x 16 x 32 kernels
// scan_gemm_f16x (d = 64 / 128), scan_gemm_w8 (256 / 512), f16kx (768 - 960), each with a SAMPLE instance.  What stays
// here is what they share: parameters, geometry and LDS budget, the index / query conversions, the hit logs'
// gather, the thresholds from the sampled pass.)

// tau[q] = an upper bound of the k-th smallest reference-order score over the sampled rows, from
// the n_vals class maxima of g written by the SAMPLE pass.  The SAMPLE pass subtracts the UPPER
// row term  bns = (||b||^2 (1+eps) + abs |b|) * mul  (the full scan subtracts the lower one), so
// for every row   score <= ||q||^2 (1+eps) + abs |q| - g/mul,   mul = s^2/2,   by the slack
// analysis at the top of this file -- row by row, with no worst-case norm of the index in it
// (one outlier row would otherwise inflate every threshold).  The k largest maxima belong to k
// different rows.  One wave per query.
struct SampleTauParams {
	const float* vals;   // [m][n_vals]
	uint32_t n_vals;
	uint32_t m;
	uint32_t k;
	const float* qnrm;   // [m] ||q||^2
	float eps, abs_coef, inv_mul;
	int ip;              // inner product: score <= e(||q||^2)/2 - g/s^2 (the SAMPLE pass subtracts +e(||b||^2) mul)
	float* tau;          // [m]
	uint32_t* tau_row;   // [m] <- 0xFFFFFFFF (no row tie-break: the GEMM forms do not use it)
	float* theta;        // [m] <- (tau - (||q||^2 (1-eps) - abs |q|)) * mul, as f16_terms_kernel
	float mul;
	uint32_t* cand_cnt;  // [m] <- 0 (the full scan's list counters)
	const float* qscale; // inner product: the queries' filter-side factors c_q (tau is stored in true units: / c_q); or nullptr
	// int8 filter (scan_gemm_i8f.hpp), or i8_thp == nullptr: thp[q] and w_q from tau and the prelude's A_q, W_q
	int* i8_thp;
	const float* i8_aq;
	const float* i8_wq_in;  // W_q, true units
	float* i8_wq;           // w_q, units of 2 s^2, for the select's pruning
	double i8_inv_2s2;
	// speculative threshold, or tau_s == nullptr: tau_s[q] comes from the j-th largest class
	// maximum, j < k, and theta', thp, w_q are made from IT -- the select checks the result against tau_s and the
	// redo pass searches the failing queries again with the proven tau.  Both are stored in true units.
	uint32_t j;
	float* tau_s;           // [m]
};
// the threshold (the filter's domain) that the class maximum with ordered bits ord stands for (0: no such value)
__device__ inline float sample_tau_of(const SampleTauParams& p, float qn, uint32_t ord) {
	float tau = __builtin_inff();
	if (ord != 0) {
		const float g = ordered_to_float(ord);
		if (p.ip)
			tau = 0.5f * (qn * p.eps + p.abs_coef * __builtin_sqrtf(qn)) - g * (0.5f * p.inv_mul);
		else
			tau = qn * (1.0f + p.eps) + p.abs_coef * __builtin_sqrtf(qn) - g * p.inv_mul;
		if (!(tau == tau))
			tau = __builtin_inff();
	}
	return tau;
}
// one thread: ord = ordered bits of the k-th largest g (0: fewer than k values) -> tau; ord_s = those of the
// j-th largest (= ord: no speculation) -> tau_s, theta', the int8 thresholds; the list counter
__device__ inline void sample_tau_store(const SampleTauParams& p, uint32_t qi, float qn, float tau_k, float tau);
__device__ inline void sample_tau_finish(const SampleTauParams& p, uint32_t qi, uint32_t ord, uint32_t ord_s) {
	const float qn = p.qnrm[qi];
	const float tau_k = sample_tau_of(p, qn, ord);
	const float tau = (p.tau_s && ord_s != ord) ? sample_tau_of(p, qn, ord_s) : tau_k;  // what the full scan filters with
	sample_tau_store(p, qi, qn, tau_k, tau);
}
// ... and what is stored: tau_k the proven threshold, tau the one the full scan filters with (both in the filter's domain)
__device__ inline void sample_tau_store(const SampleTauParams& p, uint32_t qi, float qn, float tau_k, float tau) {
	p.tau[qi] = (p.ip && p.qscale) ? tau_k / p.qscale[qi] : tau_k;  // (true units; theta' below stays in the filter's domain)
	if (p.tau_s)
		p.tau_s[qi] = (p.ip && p.qscale) ? tau / p.qscale[qi] : tau;
	p.tau_row[qi] = 0xFFFFFFFFu;
	p.theta[qi] = p.ip ? (2.0f * tau + qn * p.eps + p.abs_coef * __builtin_sqrtf(qn)) * p.mul
	                   : (tau - (qn * (1.0f - p.eps) - p.abs_coef * __builtin_sqrtf(qn))) * p.mul;
	if (p.i8_thp)
		i8f_thresholds(p.i8_aq[qi], p.i8_wq_in[qi], tau, p.i8_inv_2s2, &p.i8_thp[qi], &p.i8_wq[qi]);
	p.cand_cnt[qi] = 0;
}
// The same threshold by a whole 256-thread workgroup (n_vals <= 2048): radix select on the ordered
// bits, 8 bits per pass -- histogram in LDS, suffix sums by an 8-step scan, the thread whose bin
// holds the k-th largest fixes the digit.  A lone wave issues one instruction per >= 4 cycles, so
// the one-wave selection costs ~15 us when nothing else runs (the last workgroup of
// sample_direct_f16_kernel); this is ~2 us.  hist / ctl: 256 + 2 words of LDS.
__device__ inline void sample_tau_query_wg(const SampleTauParams& p, uint32_t qi, uint32_t* hist, uint32_t* ctl) {
	const uint32_t tid = threadIdx.x;
	const float* v = p.vals + (size_t)qi * p.n_vals;
	uint32_t ord[8];
#pragma unroll
	for (int j = 0; j < 8; ++j) {
		const uint32_t i = j * kBlock + tid;
		ord[j] = i < p.n_vals ? float_to_ordered(v[i]) : 0u;
	}
	uint32_t prefix = 0, mask = 0, krem = p.k;
	for (int pass = 3; pass >= 0; --pass) {
		const int sh = 8 * pass;
		__syncthreads();  // (the previous pass's readers are done with hist / ctl)
		hist[tid] = 0;
		if (tid == 0)
			ctl[0] = 0xFFFFFFFFu;
		__syncthreads();
#pragma unroll
		for (int j = 0; j < 8; ++j)
			if ((ord[j] & mask) == prefix)
				atomicAdd(&hist[(ord[j] >> sh) & 255u], 1u);
		__syncthreads();
		const uint32_t mine = hist[tid];
		// inclusive suffix sums: hist[t] <- sum of bins >= t
		for (int off = 1; off < 256; off <<= 1) {
			const uint32_t add = tid + off < 256 ? hist[tid + off] : 0u;
			__syncthreads();
			hist[tid] += add;
			__syncthreads();
		}
		const uint32_t above = hist[tid] - mine;  // values with a larger digit
		if (mine != 0 && above < krem && krem <= above + mine) {
			ctl[0] = tid;
			ctl[1] = krem - above;
		}
		__syncthreads();
		const uint32_t digit = ctl[0];
		if (digit == 0xFFFFFFFFu) {  // fewer than k values left: no threshold
			prefix = 0;
			break;
		}
		krem = ctl[1];
		prefix |= digit << sh;
		mask |= 0xFFu << sh;
	}
	if (tid == 0)
		sample_tau_finish(p, qi, prefix, prefix);  // (the direct kernels' queries keep proven thresholds)
}
// the work of one wave for query qi; scratch = 64 words of LDS of this wave's own
template <int PER>  // values per lane: n_vals <= 64 * PER
__device__ inline void sample_tau_query(const SampleTauParams& p, uint32_t qi, int lane, uint32_t* scratch) {
	const float* v = p.vals + (size_t)qi * p.n_vals;
	uint64_t keys[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const uint32_t i = j * 64 + lane;
		// larger g first: order by ~ordered(g); the index keeps equal values apart
		keys[j] = i < p.n_vals ? ((uint64_t)float_to_ordered(v[i]) << 32) | (0xFFFFFFFFu - i) : 0ull;
	}
	// bisection on the ordered value (32 steps whatever k and the list length; k <= 64: over the few
	// values that reach the k-th largest lane maximum)
	uint32_t ord[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		ord[j] = (uint32_t)(keys[j] >> 32);
	const bool spec = p.tau_s != nullptr && p.j < p.k;
	uint2 kj;  // the k-th and the j-th largest
	if (p.k <= 64) {
		kj = wave_kth_largest_sparse_u32<PER>(ord, p.k, scratch, lane, spec ? p.j : 0u);
	} else {
		kj.x = wave_kth_largest_u32<PER>(ord, p.k);
		kj.y = spec ? wave_kth_largest_u32<PER>(ord, p.j) : 0u;
	}
	if (lane == 0)
		sample_tau_finish(p, qi, kj.x, spec ? kj.y : kj.x);
}
template <int PER>
__global__ __launch_bounds__(kBlock) void sample_tau_kernel(SampleTauParams p) {
	__shared__ uint32_t scratch[kBlock / 64][64];
	const uint32_t qi = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
	if (qi >= p.m)
		return;  // (whole wave)
	sample_tau_query<PER>(p, qi, threadIdx.x & 63, scratch[threadIdx.x >> 6]);
}

// The thresholds of a speculating int8-filter search from the INT8 sampled pass (scan_gemm_i8f.hpp, "Sampled pass on
// int8"): vals = the class maxima of g = q~.b~ - cb written by scan_gemm_i8w_kernel<128, true, true>.  L2 only.
// tau_s = ||q||^2 - 2s^2 g_j is the centre of the j-th maximum's interval -- an estimate the select checks --, tau the
// proven bound from g_k; theta', thp, w_q and the zeroed counter come from the stored tau_s as after the fp16 pass.
struct SampleTauI8cParams {
	SampleTauParams t;     // (vals, eps, abs_coef, inv_mul unused; tau_s, j set)
	const int* vals;       // [m][n_vals]
	const float* wb_max;   // the largest finite row_w of the index (units of 2 s^2)
	double two_s2;         // 2 s^2, exact
};
template <int PER>
__global__ __launch_bounds__(kBlock) void sample_tau_i8c_kernel(SampleTauI8cParams pc) {
	__shared__ uint32_t scratch[kBlock / 64][64];
	const SampleTauParams& p = pc.t;
	const int lane = threadIdx.x & 63;
	const uint32_t qi = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
	if (qi >= p.m)
		return;  // (whole wave)
	const int* v = pc.vals + (size_t)qi * p.n_vals;
	// ordered like g; 0 = no value (INT_MIN: the class saw no row); the maximum of a class that held only rows
	// without a centre term (cb = kI8fCbNone) is below -2^29 and counts as none
	uint32_t ord[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const uint32_t i = j * 64 + lane;
		const int g = i < p.n_vals ? v[i] : -2147483647 - 1;
		ord[j] = g < -kI8fCbMax ? 0u : (uint32_t)g ^ 0x80000000u;
	}
	uint2 kj;  // the k-th and the j-th largest (j < k: the host launches this kernel for speculating searches only)
	if (p.k <= 64) {
		kj = wave_kth_largest_sparse_u32<PER>(ord, p.k, scratch[threadIdx.x >> 6], lane, p.j);
	} else {
		kj.x = wave_kth_largest_u32<PER>(ord, p.k);
		kj.y = wave_kth_largest_u32<PER>(ord, p.j);
	}
	if (lane == 0) {
		const float qn = p.qnrm[qi];
		float tau_k = __builtin_inff(), tau = __builtin_inff();
		if (kj.x != 0) {
			const double aq = (double)p.i8_aq[qi], wq = (double)p.i8_wq_in[qi];
			const double ulp_aq = __builtin_fabs(aq) * 0x1p-23 + 0x1p-149;
			const double term = pc.two_s2 * ((0.5 + 0x1p-9 + 0.5 * (double)pc.wb_max[0]) - (double)(int)(kj.x ^ 0x80000000u));
			const double b = aq + ulp_aq + wq + term;
			tau_k = f32_up(b + (__builtin_fabs(aq) + wq + __builtin_fabs(term)) * 0x1p-40);
			if (!(tau_k == tau_k))
				tau_k = __builtin_inff();
		}
		if (kj.y != 0) {
			tau = (float)((double)qn - pc.two_s2 * (double)(int)(kj.y ^ 0x80000000u));
			if (!(tau == tau))
				tau = __builtin_inff();
		}
		sample_tau_store(p, qi, qn, tau_k, tau);
	}
}

// ---- the redo pass of the speculative thresholds -------------------------------
// The select has appended the queries whose result the speculative threshold does not prove to `list` and counted
// them in *word (SelectParams::redo_word).  One wave per slot s < n_slots makes the compact operands of the redo scan:
// the fp16 (and int8) copy of query list[s], its norm, and theta' (thp, w_q) from tau_r = min(the PROVEN tau, the
// bound S_k' of the failed list: bound[s]); a slot nobody took gets zero rows and the thresholds no row passes.  More failing queries than slots: + 2^20 to *word, which the host
// reads with the other flags (the search is repeated without speculation).
struct RedoCompactParams {
	uint32_t* word;
	const uint32_t* list;    // [n_slots]
	uint32_t n_slots;
	uint32_t row_bytes;      // of a query's fp16 copy (a multiple of 16)
	const void* q16;         // [m] fp16 queries -> rq16 [n_slots]
	void* rq16;
	const float* qnrm;       // -> r_qnrm
	float* r_qnrm;
	const float* tau;        // [m] proven thresholds, true units
	const float* bound;      // [n_slots] SelectParams::redo_bound (true units, +inf: none), or nullptr: the proven tau alone
	const float* qscale;     // inner product with ip_rescale: c_q (the filter's domain = true units * c_q); or nullptr
	float eps, abs_coef, mul;
	int ip;
	float* r_theta;
	uint32_t* r_cnt;         // [n_slots] <- 0: the redo lists' counters
	// int8 filter (q8 != nullptr): rows of row_bytes / 2
	const void* q8;
	void* rq8;
	const float* i8_aq;
	const float* i8_wq_in;
	int* r_thp;
	float* r_wq;
	float* r_tau;            // [n_slots] <- tau_r, the threshold r_thp is derived from (the select's second round, SelectParams::tau_f)
	double i8_inv_2s2;
};
__global__ __launch_bounds__(kBlock) void redo_compact_kernel(RedoCompactParams p) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t s = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
	const uint32_t failed = *p.word & kRedoCountMask;
	if (blockIdx.x == 0 && threadIdx.x == 0 && failed > p.n_slots)
		atomicAdd(p.word, kRedoOverflowUnit);
	if (s >= p.n_slots)
		return;  // (whole wave)
	const bool live = s < failed;
	const uint32_t qi = live ? p.list[s] : 0u;
	const uint4* src = reinterpret_cast<const uint4*>((const unsigned char*)p.q16 + (size_t)qi * p.row_bytes);
	uint4* dst = reinterpret_cast<uint4*>((unsigned char*)p.rq16 + (size_t)s * p.row_bytes);
	for (uint32_t i = lane; i < p.row_bytes / 16; i += 64) {
		uint4 v = make_uint4(0u, 0u, 0u, 0u);
		if (live)
			v = src[i];
		dst[i] = v;
	}
	if (p.q8) {
		const uint32_t rb = p.row_bytes / 2;
		const uint32_t* s8 = reinterpret_cast<const uint32_t*>((const unsigned char*)p.q8 + (size_t)qi * rb);
		uint32_t* d8 = reinterpret_cast<uint32_t*>((unsigned char*)p.rq8 + (size_t)s * rb);
		for (uint32_t i = lane; i < rb / 4; i += 64)
			d8[i] = live ? s8[i] : 0u;
	}
	if (lane != 0)
		return;
	p.r_cnt[s] = 0;
	if (!live) {
		p.r_qnrm[s] = 0.0f;
		p.r_theta[s] = -__builtin_inff();
		if (p.q8) {
			p.r_thp[s] = (-2147483647 - 1) / 2;  // (the start value of a padded query slot, scan_gemm_i8w.hpp)
			p.r_wq[s] = __builtin_inff();
			p.r_tau[s] = __builtin_inff();
		}
		return;
	}
	const float qn = p.qnrm[qi];
	const float tau = p.bound ? __builtin_fminf(p.tau[qi], p.bound[s]) : p.tau[qi];
	const float tau_f = (p.ip && p.qscale) ? tau * p.qscale[qi] : tau;  // (c_q is a power of two: exact)
	p.r_qnrm[s] = qn;
	p.r_theta[s] = p.ip ? (2.0f * tau_f + qn * p.eps + p.abs_coef * __builtin_sqrtf(qn)) * p.mul
	                    : (tau_f - (qn * (1.0f - p.eps) - p.abs_coef * __builtin_sqrtf(qn))) * p.mul;
	if (p.q8) {
		i8f_thresholds(p.i8_aq[qi], p.i8_wq_in[qi], tau, p.i8_inv_2s2, p.r_thp + s, p.r_wq + s);
		p.r_tau[s] = tau;
	}
}

}  // namespace expann
