// scan_gemm_i8f.hpp -- the fp32 L2 candidate filter on the INT8 matrix cores: rows and queries quantised
// to int8 with ONE per-index scale, scanned by scan_gemm_i8w_kernel<128> (v_mfma_i32_16x16x64_i8: twice the
// K per cycle of the fp16 form's v_mfma_f32_16x16x32_f16), candidates re-scored exactly in fp32 by the
// select as after the fp16 filter -- ids and distances stay bit-identical.  The threshold tau comes from the fp16
// sampled pass (scan_gemm_f16.hpp) or, for a speculating search, from the int8 one ("Sampled pass on int8" below);
// this header holds the analysis and the prelude kernels.
//
// Quantisation.  One scale s > 0 per index (fp32; s^2 is exact in fp64).  For a row b and a query q
//     b~ = clamp(rint(b / s), -127, 127),   e_b = b - s b~      (q~, e_q alike)
// Any b~ is allowed: the errors are measured after the fact, so clipping (s = min(max|x|, 5.5 rms) / 127)
// only loosens the bound of the rows / queries that were clipped, never its validity.
// (rms: of all components -- unless those within the clip carry less than 1/16 of the index's energy, i.e. a few
// far-out rows set the rms and the scale would be several times too coarse for all the others: then the rms of the
// components within the clip, once, kI8fTrimEnergy; every other index keeps its scale bit for bit.)
//
// Exact bound.  q.b = (s q~ + e_q).(s b~ + e_b) = s^2 q~.b~ + q.e_b + e_q.b - e_q.e_b, so with
// P = s^2 q~.b~ (an exact integer q~.b~, |q~.b~| <= 128 * 127^2 < 2^21),
//     |q.b - P|  <=  E = |q| |e_b| + |e_q| |b| + |e_q| |e_b|.
// Separable form, AM-GM around one lambda > 0 per index on both sides:  2 |q| |e_b| <= lambda N_q + V_b / lambda,
// 2 |e_q| |b| <= lambda N_b + V_q / lambda, and 2 |e_q| |e_b| <= V_q + V_b.  The query's part of the second is also
// capped: 2 |e_q| |b| <= 2 B |e_q| with B >= max_b |b| (the fp16 prelude's largest row norm), and since
// min(a, x + y) <= x + min(a, y) for x >= 0,  2 |e_q| |b| <= lambda N_b + M_q,  M_q = min(2 B |e_q|, V_q / lambda):
// a query with a clipped component loosens its bound linearly in |e_q| (V_q / lambda alone sent two lists of
// 1 M iid rows x 4 096 queries to 49 k candidates), while a few far-out rows (a large B) do not loosen the others.
//     2 E  <=  lambda N_q + M_q + V_q  +  lambda N_b + c V_b,    N = |x|^2,  V = |e|^2,  c = 1 + 1/lambda.
// Reference-order score.  S = the fp32 score of the reference (16 lane sums of fma((q-b)^2), a 4-level tree;
// oracle_l2_f32) and D = |q - b|^2 = N_q + N_b - 2 q.b exactly:  |S - D| <= (d/16 + 7) u D (1 + 2^-20),
// u = 2^-24, and D <= 2 (N_q + N_b), hence |S - D| <= eps (N_q + N_b) + eta with
//     eps = (d/8 + 16) u,   eta = (d + 16) 2^-149  (subnormal products: an absolute half-ulp per operation).
// Together, for every pair:
//     S  >=  L = A_q + A_b - 2 P - eta,   A_q = N_q (1 - lambda - eps) - M_q - V_q,   A_b = N_b (1 - lambda - eps) - c V_b
//     S  <=  L + W_q + W_b,      W_q = 2 (lambda + eps) N_q + 2 M_q + 2 V_q + 2 eta,   W_b = 2 (lambda + eps) N_b + 2 c V_b
// N_x and V_x are summed in fp64 (relative error < d 2^-53 < 2^-40) and used as N_lo = N (1 - 2^-40),
// V_up = V (1 + 2^-40), so A_x is a lower and W_x an upper bound of the real-number terms; the few fp64
// operations that follow add < 2^-50 relative, covered by the margins below.
//
// Integer test.  tau_q >= the k-th smallest S (fp16 sampled pass, sample_tau_kernel), so every row of the
// k best has L <= tau_q, i.e.  q~.b~ >= A_b / 2s^2 + (A_q - eta - tau_q) / 2s^2.  With
//     bp[b]  = floor(A_b / 2s^2 - m_b)                 (index side, i8f_rows_kernel)
//     thp[q] = -floor((A_q - eta - tau_q) / 2s^2 - m_q)  (query side, sample_tau_finish)
// (m = 2^-30 |x| + 2^-10: the fp64 rounding of the quotient) both floors are <= their real values, so
// q~.b~ >= bp[b] - thp[q]  -- the i8w kernel's test  acc = thp[q] + q~.b~ >= bp[b]  -- holds for every such
// row: a superset of the k best reaches the candidate lists, with no slack left to chance.
// Int32 range.  thp is clamped into [-2^29, 2^29] and bp into [kI8fBpMin, kI8fBpMax] = [-2^29 - 2^22,
// 2^29 - 2^22], each clamp in the safe direction: a bp raised to kI8fBpMin hits every query (acc >= -2^29 -
// 2^21), a bp lowered to kI8fBpMax only adds hits; a thp raised to -2^29 only adds hits, one lowered to 2^29
// still hits every row (acc >= 2^29 - 2^21 > kI8fBpMax).  Padded query slots start at -2^30 and never reach
// kI8fBpMin, padding rows carry kI8qPadBp = 2^30, and |acc| <= 2^30 + 2^21 never wraps.
//
// Sampled pass on int8 (option "i8_sample"; sample_tau_i8c_kernel, scan_gemm_f16.hpp).  A speculating search needs
// no proven threshold before the scan -- the select checks tau_s -- so its sampled pass runs on the
// int8 copy too: scan_gemm_i8w_kernel<128, true, true> with the row term  cb[b] = rint(N_b / 2s^2)  in place of bp,
// class maxima of  g = q~.b~ - cb[b].  From the bounds above  A_x + W_x / 2 = N_x (+ eta on the query's side), so the
// centre of a pair's interval [L, L + W_q + W_b] is  N_q + N_b - 2 P - eta:  the score the quantised product stands
// for, off the true one by the quantisation noise alone (sd 0.40 on N(0, 1) rows at d = 128 against a mean width of
// 13.6).  tau_s = ||q||^2 - 2s^2 g_j, g_j the j-th largest class maximum: an estimate, no bound, and needs to be none.
// The PROVEN tau (the redo pass's threshold for a failed list with fewer than k rows) comes from g_k, the k-th
// largest class maximum.  For a row b:  S <= L + W_q + W_b = (A_q - eta) + W_q + (A_b + W_b) - 2 P  and
// A_b + W_b = N_b (1 + lambda + eps) + c V_b = N_b + W_b / 2.  The fp64 sum nn of i8f_rows_kernel has N_b <=
// nn (1 + 2^-40) and cb >= nn / 2s^2 - 1/2 - 2^-50 nn / 2s^2, so with cb <= kI8fCbMax = 2^29:  N_b <= 2s^2 (cb + 1/2 + 2^-9);
// P = 2s^2 q~.b~ = 2s^2 (g + cb) exactly; the stored aq is A_q - eta rounded down, A_q - eta <= aq + ulp(aq); and
// W_b / 2 <= 2s^2 wb_max / 2, wb_max = the largest row_w among the rows the pass can see.  It sees a row only when the
// row has an interval, its cb fits kI8fCbMax and row_w <= w_cap = twice the width of a row of the index's rms norm
// with unclipped components, 2 (2 (lambda + eps) d rms^2 + 2 c d s^2 / 12) / 2s^2 (I8fConsts::w_cap): every other row
// carries cb = kI8fCbNone and is no class maximum -- any subset of the rows may be sampled -- so one row with a
// clipped component (row_w 24 against a mean of 6.8 on 266 240 N(0, 1) rows) does not widen every query's tau.  Together
//     S  <=  aq + ulp(aq) + W_q + 2s^2 (1/2 + 2^-9 - g + wb_max / 2)
// for every row whose g the pass saw, decreasing in g.  The k largest class maxima belong to k different rows, each
// with g >= g_k, so the k-th smallest S of the index is at most that bound at g = g_k: tau, evaluated in fp64
// (five operations, < 2^-50 relative each, covered by a factor 1 + 2^-40 on every positive term) and rounded UP to
// fp32.  Fewer than k real maxima (g of a cb = kI8fCbNone row is below -2^29): tau = +inf, as the fp16 pass.
//
// Keys and pruning.  A hit's log entry is its raw accumulator and the row's bp; gather_logs_kernel (i_mode 3) keys it
// by kappa = -(acc - bp[b]) = bp - thp - q~.b~.  From the two floors (each below its real value by less than
// 1 + m <= 1.51 while |x| <= 2^29) and the query term stored rounded down in fp32 (aq = A_q - eta - delta,
// 0 <= delta <= ulp(aq) <= 2^-23 |aq| + 2^-149), (L - tau_q) / 2s^2 lies in [kappa, kappa + 4 + delta / 2s^2), so
//     S >= tau_q + 2s^2 kappa             S <= tau_q + 2s^2 (kappa + 4 + delta / 2s^2 + w_q + w_b),   w_x = W_x / 2s^2.
// The k best rows lie among the candidates, so the k-th smallest S is at most the k-th smallest upper bound,
// and a candidate whose lower bound exceeds it cannot be among the k best (not even by a tie):  the select
// keeps  kappa <= kth(kappa + w_b) + w_q  with w_q += 4 + (2^-23 |aq| + 2^-149) / 2s^2, row_w[b] = w_b, q_w[q] = w_q.  A row
// or query whose integer term was clamped has no such interval: its w is +inf (row: its key is -inf, it is
// always re-scored -- the gather gives that key to every bp AT a clamp limit, which a clamped row always is and an
// unclamped one that merely lands there may be: the safe direction; query: its list is not pruned).  The fp32 arithmetic of the keys and the cutoff adds
// < 2^-21 relative, covered by the select's 2^-18 |cutoff| + 1.
//
// Two rounds (the select's default, SelectParams::tau_f; "rerank_rounds" = 1 keeps the cut above).  The cut above knows
// interval bounds only and keeps rows up to about S_k + 2 W; one exact score proves most of them out.  The select
// re-scores first the R1 = max(16, k rounded up to 16) keys of smallest kappa (ties at the R1-th value all go along;
// -inf keys, rows without an interval, sort first by themselves) and takes T = the k-th smallest exact score among
// them (repeated scores counted).  Those are k different rows of the list, so T >= the list's -- and the index's --
// k-th smallest S.  Every other candidate has  S >= L >= tau_q + 2s^2 kappa  (the line above; tau_q is the fp32
// value thp[q] was derived from: tau_s when speculating, the proven tau otherwise, tau_r in the redo pass), so one
// with  kappa > x = (T - tau_q) / 2s^2  scores strictly more than T: it is not among the k best of the list and ties
// with none of them, and the emitted rows and the k-th score the speculation's check sees are those of the whole
// list.  Rounding: x is one fp64 expression per query, (double) T - (double) tau_q times the stored 1 / 2s^2 --
// three roundings, < 2^-50 relative, covered by + 2^-40 |x| + 2^-10 -- then rounded UP to fp32; a key is the fp32
// rounding of its integer kappa (|kappa| < 2^31) and rounding to nearest is monotone, so kappa <= x implies
// key <= cut: the select keeps !(key > cut).  No w_b or w_q enters, so the wave path no longer reads row_w per key.
// Safe branches: a list of at most R1 keys is re-scored whole in one round; w_q = +inf (thp clamped, or no tau:
// no interval) -- no cut; fewer than k finite scores in the first round (T = +inf or NaN) -- no cut.
// (1 M x d128 iid rows, 10 000 queries, k = 10: 121.4 -> 38.2 rows re-scored per query)
//
// Choice of lambda: it balances lambda N against V / lambda for a typical pair; with rounding errors of
// variance s^2 / 12 per component that is lambda ~ s / (sqrt(12) rms); a numpy model of 1 M x d128 iid N(0, 1) rows
// put the candidates lowest at 1.4 x that.  The clip, 5.5 rms, is DESIGN.md 4.4i's.
#pragma once
#include <cmath>
#include "common.hpp"

namespace expann {

constexpr int kI8fBpMin = -(1 << 29) - (1 << 22);
constexpr int kI8fBpMax = (1 << 29) - (1 << 22);
constexpr int kI8fThpLim = 1 << 29;
constexpr int kI8fCbMax = 1 << 29;   // largest centre row term of the int8 sampled pass (cb >= 0: N_b >= 0)
constexpr int kI8fCbNone = 1 << 30;  // cb of a row the sampled pass must not see (= kI8qPadBp, the padding rows')

// the analysis's per-index constants (host: i8f_consts)
struct I8fConsts {
	float s, inv_s;  // scale and 1 / s (any rounding of 1/s is fine: the errors are measured)
	double lo;       // 1 - lambda - eps
	double c;        // 1 + 1 / lambda
	double inv_lambda;
	double b2;       // 2 B (B >= max_b |b|)
	double wn;       // 2 (lambda + eps)
	double inv_2s2;  // 1 / (2 s^2)
	double eta;
	double w_cap;    // int8 sampled pass: rows with row_w above this are left out ("Sampled pass on int8")
};
// bnmax = the largest fp32 reference-order ||b||^2 (relative error < (d/16 + 6) u, far below the 2^-16 added)
inline I8fConsts i8f_consts(float s, float rms, float bnmax, int d) {
	I8fConsts k{};
	k.s = s;
	k.inv_s = 1.0f / s;
	const double u = 5.9604644775390625e-08;
	const double eps = ((double)d / 8.0 + 16.0) * u;
	const double lambda = rms > 0.0f ? 1.4 * (double)s / (3.4641016151377544 * (double)rms) : 0.01;
	k.lo = 1.0 - lambda - eps;
	k.c = 1.0 + 1.0 / lambda;
	k.inv_lambda = 1.0 / lambda;
	k.b2 = 2.0 * std::sqrt((double)bnmax * (1.0 + 0x1p-16)) * (1.0 + 0x1p-40);
	k.wn = 2.0 * (lambda + eps);
	k.inv_2s2 = 1.0 / (2.0 * (double)s * (double)s);
	k.eta = ((double)d + 16.0) * 1.401298464324817e-45;
	k.w_cap = 2.0 * (k.wn * (double)d * (double)rms * (double)rms + 2.0 * k.c * (double)d * (double)s * (double)s / 12.0) * k.inv_2s2;
	return k;
}

// the next fp32 value above (up) or below a finite f
__device__ inline float f32_step(float f, bool up) {
	if (f == 0.0f)
		return __builtin_bit_cast(float, up ? 1u : 0x80000001u);
	const uint32_t u = __builtin_bit_cast(uint32_t, f);
	return __builtin_bit_cast(float, ((u >> 31) == 0) == up ? u + 1 : u - 1);
}
// fp64 -> fp32 rounded down / up (a conversion rounds to nearest; step one ulp when it went the wrong way)
__device__ inline float f32_down(double x) {
	const float f = (float)x;
	return (double)f > x ? f32_step(f, false) : f;
}
__device__ inline float f32_up(double x) {
	const float f = (float)x;
	return (double)f < x ? f32_step(f, true) : f;
}
// int8 value of x at scale s
__device__ inline int i8f_quant(float x, float inv_s) {
	const float r = __builtin_rintf(x * inv_s);
	return r >= 127.0f ? 127 : (r <= -127.0f ? -127 : (int)r);  // (NaN -> -127: a non-finite index has no fp16 copy)
}

// Index statistics for the scale: sum of squares (fp64) and the bit pattern of max |x|; out zeroed by the caller
__global__ __launch_bounds__(kBlock) void i8f_stats_kernel(const float* in, size_t n, double* sumsq, uint32_t* maxabs_bits) {
	__shared__ double red[kBlock / 64];
	__shared__ uint32_t redb[kBlock / 64];
	double s = 0.0;
	uint32_t b = 0;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
		const float v = in[i];
		s += (double)v * (double)v;
		const uint32_t vb = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
		b = vb > b ? vb : b;
	}
	for (int off = 32; off > 0; off >>= 1) {
		s += __shfl_xor(s, off);
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if ((threadIdx.x & 63) == 0) {
		red[threadIdx.x >> 6] = s;
		redb[threadIdx.x >> 6] = b;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kBlock / 64; ++w) {
			s += red[w];
			b = redb[w] > b ? redb[w] : b;
		}
		atomicAdd(sumsq, s);
		if (b != 0)
			atomicMax(maxabs_bits, b);
	}
}

// The same sum over the components with |x| <= limit alone, and their number (the scale of an index whose few far-out
// rows carry nearly all of its energy: ensure_i8f); out zeroed by the caller
__global__ __launch_bounds__(kBlock) void i8f_trimmed_stats_kernel(const float* in, size_t n, float limit, double* sumsq,
                                                                   unsigned long long* count) {
	__shared__ double red[kBlock / 64];
	__shared__ unsigned long long redc[kBlock / 64];
	double s = 0.0;
	unsigned long long c = 0;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
		const float v = in[i];
		if (__builtin_fabsf(v) <= limit) {
			s += (double)v * (double)v;
			++c;
		}
	}
	for (int off = 32; off > 0; off >>= 1) {
		s += __shfl_xor(s, off);
		c += __shfl_xor(c, off);
	}
	if ((threadIdx.x & 63) == 0) {
		red[threadIdx.x >> 6] = s;
		redc[threadIdx.x >> 6] = c;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kBlock / 64; ++w) {
			s += red[w];
			c += redc[w];
		}
		atomicAdd(sumsq, s);
		atomicAdd(count, c);
	}
}

// Index side, one pass over the fp32 rows: the padded int8 copy (rows of D bytes, n_pad rows, zero rows
// behind the end), bp[b] and row_w[b] = w_b (+inf when bp was clamped).  16 lanes per row, each lane D / 16
// consecutive components (one 8-byte store at d = 128); padding rows get bp = kI8qPadBp (set by the caller's
// fill of bp, as scan_gemm_i8q's i8q_bp_kernel).
// cb[b] = rint(N_b / 2s^2), the centre row term of the int8 sampled pass ("Sampled pass on int8" above), or kI8fCbNone
// for a row without an interval, wider than w_cap or with a centre term beyond kI8fCbMax: never a class maximum.
template <int D>
__global__ __launch_bounds__(kBlock) void i8f_rows_kernel(const float* x, uint32_t n, I8fConsts k, int8_t* out,
                                                          int* bp, float* row_w, int* cb) {
	static_assert(D % 64 == 0, "whole 4-byte groups per lane");
	constexpr int PER = D / 16;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t ii = i < n ? i : n - 1;
	const float* src = x + (size_t)ii * D + l * PER;
	double nn = 0.0, vv = 0.0;
	uint32_t packed[PER / 4];
#pragma unroll
	for (int w = 0; w < PER / 4; ++w) {
		uint32_t pw = 0;
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const float v = src[4 * w + j];
			const int t = i8f_quant(v, k.inv_s);
			const double e = (double)v - (double)k.s * (double)t;
			nn += (double)v * (double)v;
			vv += e * e;
			pw |= ((uint32_t)t & 0xFFu) << (8 * j);
		}
		packed[w] = pw;
	}
#pragma unroll
	for (int off = 8; off > 0; off >>= 1) {
		nn += __shfl_xor(nn, off);
		vv += __shfl_xor(vv, off);
	}
	if (i >= n)
		return;
	uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)i * D + l * PER);
#pragma unroll
	for (int w = 0; w < PER / 4; ++w)
		dst[w] = packed[w];
	if (l == 0) {
		const double n_lo = nn * (1.0 - 0x1p-40), v_up = vv * (1.0 + 0x1p-40);
		const double xb = (n_lo * k.lo - k.c * v_up) * k.inv_2s2;
		const double xl = xb - (__builtin_fabs(xb) * 0x1p-30 + 0x1p-10);
		if (xl >= (double)kI8fBpMin && xl <= (double)kI8fBpMax) {
			bp[i] = (int)__builtin_floor(xl);
			row_w[i] = f32_up((k.wn * nn * (1.0 + 0x1p-40) + 2.0 * k.c * v_up) * k.inv_2s2 * (1.0 + 0x1p-40));
			const double xc = __builtin_rint(nn * k.inv_2s2);
			cb[i] = (xc <= (double)kI8fCbMax && (double)row_w[i] <= k.w_cap) ? (int)xc : kI8fCbNone;
		} else {  // (NaN lands here too)
			bp[i] = xl > 0.0 ? kI8fBpMax : kI8fBpMin;
			row_w[i] = __builtin_inff();
			cb[i] = kI8fCbNone;
		}
	}
}

// wb_max = the largest row_w among the rows with a centre term (the proven tau of the int8 sampled pass); row_w >= 0,
// so the bit patterns order like the values; *out_bits zeroed by the caller
__global__ __launch_bounds__(kBlock) void i8f_wbmax_kernel(const float* row_w, const int* cb, uint32_t n, uint32_t* out_bits) {
	uint32_t b = 0;
	for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
		const float w = row_w[i];
		const uint32_t wb = __builtin_bit_cast(uint32_t, w);
		if (cb[i] != kI8fCbNone && w >= 0.0f && w < __builtin_inff() && wb > b)
			b = wb;
	}
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)b, off);
		b = o > b ? o : b;
	}
	if ((threadIdx.x & 63) == 0 && b != 0)
		atomicMax(out_bits, b);
}

// Query side (f16_query_prep_kernel): q~ and the query's terms.  aq = A_q - eta rounded down, wq = W_q
// rounded up (true units; sample_tau_finish turns them into thp and w_q once tau is known).
struct I8fQueryArgs {
	int8_t* q8;  // [m][D] int8, or nullptr: the fp16 form alone
	float* aq;
	float* wq;
	I8fConsts k;
};
// lane l of a 16-lane group holds components l + 16 t (t < D/16) of query i in vals[]
template <int D>
__device__ inline void i8f_query_terms(const I8fQueryArgs& a, uint32_t i, uint32_t m, int l, const float* vals) {
	double nn = 0.0, vv = 0.0;
#pragma unroll
	for (int t = 0; t < D / 16; ++t) {
		const float v = vals[t];
		const int q = i8f_quant(v, a.k.inv_s);
		const double e = (double)v - (double)a.k.s * (double)q;
		nn += (double)v * (double)v;
		vv += e * e;
		if (i < m)
			a.q8[(size_t)i * D + l + 16 * t] = (int8_t)q;
	}
#pragma unroll
	for (int off = 8; off > 0; off >>= 1) {
		nn += __shfl_xor(nn, off);
		vv += __shfl_xor(vv, off);
	}
	if (i < m && l == 0) {
		const double v_up = vv * (1.0 + 0x1p-40);
		const double e_up = __builtin_sqrt(v_up) * (1.0 + 0x1p-40);  // |e_q| rounded up
		const double mq = __builtin_fmin(a.k.b2 * e_up, v_up * a.k.inv_lambda) * (1.0 + 0x1p-40);  // M_q
		a.aq[i] = f32_down((nn * (1.0 - 0x1p-40) * a.k.lo - mq - v_up - a.k.eta) * (1.0 - 0x1p-40));
		a.wq[i] = f32_up((a.k.wn * nn * (1.0 + 0x1p-40) + 2.0 * mq + 2.0 * v_up + 2.0 * a.k.eta) * (1.0 + 0x1p-40));
	}
}

// thp[q] and w_q from tau (true units) -- sample_tau_finish; thp clamped as in the analysis, w_q = +inf when
// the clamp (or a missing tau) voids the interval the select's pruning relies on
__device__ inline void i8f_thresholds(float aq, float wq_true, float tau, double inv_2s2, int* thp, float* wq) {
	const double xq = ((double)aq - (double)tau) * inv_2s2;
	const double xl = xq - (__builtin_fabs(xq) * 0x1p-30 + 0x1p-10);
	if (xl >= -(double)kI8fThpLim && xl <= (double)kI8fThpLim) {
		*thp = -(int)__builtin_floor(xl);
		// (+ ulp(aq): the fp32 rounding of A_q, header)
		const double ulp_aq = __builtin_fabs((double)aq) * 0x1p-23 + 0x1p-149;
		*wq = f32_up(((double)wq_true + ulp_aq) * inv_2s2 * (1.0 + 0x1p-40) + 4.0);
	} else {  // (tau = +inf or NaN: every row passes)
		*thp = xl > 0.0 ? -kI8fThpLim : kI8fThpLim;
		*wq = __builtin_inff();
	}
}

}  // namespace expann
