// scan_int8_any.hpp -- the exact kernels over 8-bit rows (scan_int8.hpp, scan_gemm_i8.hpp's preludes) with the
// dim known at RUN time: every multiple of 64 up to kMaxAnyDim bytes per row that has no instance of its own.
//
// Same scores, same contract.  The compiled kernels give lane l of a DPP row the contiguous bytes
// [l d/16, (l+1) d/16) of its base row and keep the TQ query slices in registers (TQ x d/64 dwords per lane:
// 64 per query at d = 4096).  Here lane l owns dwords l, l + 16, l + 32, ... of the row -- the 16 lanes of a row
// read one 64-byte segment per step, integer sums are exact in any order -- the TQ queries of the workgroup sit in
// LDS (TQ x kMaxAnyDim bytes; the four row groups of a wave read the same 64 bytes: broadcast), and the row is
// walked in pieces of four dwords per lane (four loads in flight), then dword by dword over what is left of an
// odd d/64.  Byte offsets of rows are 64-bit: n x d passes 2^32 near 1 M rows of d = 4096.
#pragma once
#include "scan_int8.hpp"

namespace expann {

// one dword of one (query, row) pair; kU8L2 / kI8L2 accumulate the dot product, the caller folds in the self terms
template <int MODE> __device__ inline int term_i8(int q, int b, int acc) {
	if (MODE == kI8L2Ref) {
		const int d = sub_bytes(q, b);
		return dot4<MODE>(d, d, acc);
	}
	return dot4<MODE>(q, b, acc);
}
// the reduced sum over the row -> the integer score (qself, bself: sum q^2, sum b^2 of the L2 forms)
template <int MODE> __device__ inline int finish_i8(int acc, int qself, int bself) {
	if (MODE == kU8L2 || MODE == kI8L2)
		return qself + bself - 2 * acc;
	if (MODE == kI8IP)
		return -acc;
	return acc;
}

template <int TQ, int MODE>
__global__ __launch_bounds__(kBlock) void scan_filter_i8_any_kernel(ScanParams p) {
	static_assert(MODE == kU8L2 || MODE == kI8L2 || MODE == kI8L2Ref || MODE == kI8IP, "8-bit rows");
	__shared__ int qs[TQ * (kMaxAnyDim / 4)];
	constexpr bool L2X = (MODE == kU8L2 || MODE == kI8L2);  // expanded form: needs sum q^2, sum b^2
	const uint32_t DW = p.dim / 4, NW = p.dim / 64;  // dwords per row, per lane
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	const uint32_t q0 = qtile * TQ;
	const int* __restrict__ base = (const int*)p.base;
	const int* __restrict__ queries = (const int*)p.queries;
	const bool level0 = (p.tau == nullptr);

	for (uint32_t i = threadIdx.x; i < TQ * DW; i += kBlock) {
		const uint32_t j = i / DW;
		const uint32_t qi = (q0 + j < p.m) ? q0 + j : p.m - 1;
		qs[i] = queries[(size_t)qi * DW + (i - j * DW)];
	}
	float tau[TQ];
#pragma unroll
	for (int j = 0; j < TQ; ++j) {
		const uint32_t qi = (q0 + j < p.m) ? q0 + j : p.m - 1;
		float tj = level0 ? __builtin_inff() : p.tau[qi];
		tj = (q0 + j < p.m) ? tj : -__builtin_inff();
		tau[j] = __builtin_bit_cast(float,
		                            __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tj)));
	}
	__syncthreads();
	const int* qsl = qs + l;
	int qself[TQ];  // sum q^2 over the whole query (L2 forms)
#pragma unroll
	for (int j = 0; j < TQ; ++j) {
		int self = 0;
		if (L2X) {
			for (uint32_t t = 0; t < NW; ++t) {
				const int v = qsl[j * DW + 16 * t];
				self = dot4<MODE>(v, v, self);
			}
			self = reduce16_i32(self);
		}
		qself[j] = self;
	}

	const uint32_t g0 = chunk * p.groups_per_block;
	uint32_t g1 = g0 + p.groups_per_block;
	if (g1 > p.n_groups_sel)
		g1 = p.n_groups_sel;
	uint64_t best[TQ];  // class minima (classmin level, scan_f32.hpp)
#pragma unroll
	for (int j = 0; j < TQ; ++j)
		best[j] = kSentinelKey;
	for (uint32_t g = g0; g < g1; ++g) {
		const uint32_t row = g * p.group_stride * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
		const bool rvalid = row < p.n_rows;
		const int* src = base + (size_t)(rvalid ? row : p.n_rows - 1) * DW + l;
		int acc[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j)
			acc[j] = 0;
		int bself = 0;
		uint32_t t = 0;
		for (; t + 4 <= NW; t += 4) {
			int r[4];
#pragma unroll
			for (int u = 0; u < 4; ++u)
				r[u] = src[16 * (t + u)];
#pragma unroll
			for (int u = 0; u < 4; ++u) {
				if (L2X)
					bself = dot4<MODE>(r[u], r[u], bself);
#pragma unroll
				for (int j = 0; j < TQ; ++j)
					acc[j] = term_i8<MODE>(qsl[j * DW + 16 * (t + u)], r[u], acc[j]);
			}
		}
		for (; t < NW; ++t) {
			const int rv = src[16 * t];
			if (L2X)
				bself = dot4<MODE>(rv, rv, bself);
#pragma unroll
			for (int j = 0; j < TQ; ++j)
				acc[j] = term_i8<MODE>(qsl[j * DW + 16 * t], rv, acc[j]);
		}
		if (L2X)
			bself = reduce16_i32(bself);
		float s[TQ];
		unsigned long long any = 0;
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			s[j] = (float)finish_i8<MODE>(reduce16_i32(acc[j]), qself[j], bself);
			any |= __builtin_amdgcn_ballot_w64(s[j] <= tau[j]);
		}
		if (level0 && p.classmin) {
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				const uint64_t key = rvalid ? make_key(s[j], row) : kSentinelKey;
				best[j] = key < best[j] ? key : best[j];
			}
		} else if (level0) {
			const uint32_t slot = g * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
			if (l == 0 && slot < p.cap) {
#pragma unroll
				for (int j = 0; j < TQ; ++j)
					if (q0 + j < p.m)
						p.cand[(size_t)(q0 + j) * p.cap + slot] = rvalid ? make_key(s[j], row) : kSentinelKey;
			}
		} else if (any) {
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				if (l == 0 && rvalid && q0 + j < p.m &&
				    (s[j] < tau[j] || (s[j] == tau[j] && row <= p.tau_row[q0 + j]))) {
					const uint32_t slot = atomicAdd(&p.cand_cnt[q0 + j], 1u);
					if (slot < p.cap)
						p.cand[(size_t)(q0 + j) * p.cap + slot] = make_key(s[j], row);
				}
			}
		}
	}
	if (level0 && p.classmin) {
		const uint32_t slot = chunk * 16 + wave * 4 + rg;
		if (l == 0 && slot < p.cap) {
#pragma unroll
			for (int j = 0; j < TQ; ++j)
				if (q0 + j < p.m)
					p.cand[(size_t)(q0 + j) * p.cap + slot] = best[j];
		}
	}
}

// scores[i] = score(query, base[ids[i]]) (score_ids_i8_kernel with the row length in p.dim)
template <int MODE>
__global__ __launch_bounds__(kBlock) void score_ids_i8_any_kernel(ScoreIdsI8Params p) {
	constexpr bool L2X = (MODE == kU8L2 || MODE == kI8L2);
	const uint32_t DW = p.dim / 4, NW = p.dim / 64;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t i = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const bool valid = i < p.n_ids;
	const uint64_t row = p.ids[valid ? i : p.n_ids - 1] - p.id_offset;
	const int* __restrict__ r = (const int*)p.base + (size_t)row * DW + l;
	const int* __restrict__ q = (const int*)p.query + l;
	int acc = 0, qself = 0, bself = 0;
	for (uint32_t t = 0; t < NW; ++t) {
		const int qv = q[16 * t], bv = r[16 * t];
		if (L2X) {
			qself = dot4<MODE>(qv, qv, qself);
			bself = dot4<MODE>(bv, bv, bself);
		}
		acc = term_i8<MODE>(qv, bv, acc);
	}
	const int tot = reduce16_i32(finish_i8<MODE>(acc, qself, bself));  // (the form is linear in the three sums)
	if (valid && l == 0)
		p.scores[i] = (float)tot;
}

// sum b^2 per row for the GEMM form (row_self_i8_kernel; uint8 rows: of b - 128); 16 lanes per row
template <int MODE>
__global__ __launch_bounds__(kBlock) void row_self_i8_any_kernel(const void* base, uint32_t n_rows, int* out,
                                                                 uint32_t dim) {
	const uint32_t DW = dim / 4, NW = dim / 64;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t row = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t rr = row < n_rows ? row : n_rows - 1;
	const int* src = (const int*)base + (size_t)rr * DW + l;
	int acc = 0;
	for (uint32_t t = 0; t < NW; ++t) {
		int v = src[16 * t];
		if (MODE == kU8L2)
			v ^= (int)0x80808080;
		acc = __builtin_amdgcn_sdot4(v, v, acc, false);
	}
	acc = reduce16_i32(acc);
	if (row < n_rows && l == 0)
		out[row] = acc;
}

// the query-side terms of the GEMM form (query_theta_i8_kernel): sum q^2, and with thresholds
// theta = floor(tau) - sum q^2 clamped into int32; 16 lanes per query
template <int MODE>
__global__ __launch_bounds__(kBlock) void query_theta_i8_any_kernel(const void* queries, uint32_t m, const float* tau,
                                                                    int* theta, int* qself, uint32_t dim) {
	const uint32_t DW = dim / 4, NW = dim / 64;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int l = lane & 15, rg = lane >> 4;
	const uint32_t qi = blockIdx.x * kRowsPerGroup + wave * kRowsPerWaveStep + rg;
	const uint32_t qq = qi < m ? qi : m - 1;
	const int* src = (const int*)queries + (size_t)qq * DW + l;
	int acc = 0;
	if (MODE != kI8IP) {
		for (uint32_t t = 0; t < NW; ++t) {
			int v = src[16 * t];
			if (MODE == kU8L2)
				v ^= (int)0x80808080;
			acc = __builtin_amdgcn_sdot4(v, v, acc, false);
		}
		acc = reduce16_i32(acc);
	}
	if (qi < m && l == 0 && !tau)
		qself[qi] = acc;
	if (qi < m && l == 0 && tau) {
		const float t = tau[qi];
		int ft;
		if (!(t < 2147483520.0f))
			ft = 2147483647;
		else if (t < -2147483520.0f)
			ft = -2147483647 - 1;
		else
			ft = (int)__builtin_floorf(t);
		long long th = (long long)ft - (long long)acc;
		if (th > 2147483647LL)
			th = 2147483647LL;
		if (th < -2147483648LL)
			th = -2147483648LL;
		theta[qi] = (int)th;
		qself[qi] = acc;
	}
}

}  // namespace expann
