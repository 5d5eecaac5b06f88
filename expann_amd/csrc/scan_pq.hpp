// scan_pq.hpp -- threshold-filter scan over product-quantised rows (EXPANN_DTYPE_PQ8, THE PQ RULE of expann_hip.h).
//
// A row is M one-byte codes; code i selects centroid codebooks[i][code] of sub-vector i (dsub = dim / M floats).  The
// score of (query, row) is a sum of M entries of the query's lookup tables T[i][c] (ADC): there is no product per row
// and no inner dimension, so no matrix instruction fits -- the kernel is an LDS gather.
//
// scan_pq_kernel<TQ, IP>: 256 threads, TQ queries per workgroup, one row per lane per step (256 rows a step).  It takes
// ScanParams (pq_codebooks, pq_m are its trailing fields) and honours the contract of the 8-bit direct scan exactly as
// scan_hamming_valu_kernel does: level 0 with every key at its slot, level 0 with class minima, levels that file
// (score, row) <= (tau, tau_row) through cand_cnt / cand.
//
// Tables: dynamic LDS, [M][256][TQ] fp32 -- the TQ queries of an entry are adjacent, so ONE ds_read_b128 (two at
// TQ = 8, a b64 / b32 at TQ = 2 / 1) serves every query of the tile for one code, and a bank conflict is paid once
// per code.  TQ is the largest of 8 / 4 / 2 / 1 with TQ * M * 1024 B <= 128 KB (pq_tile_for, bf_plan.hpp).
// Prologue: thread c builds entry c of every sub-quantiser for the TQ queries, in the rule's order -- one codebook
// value read from global memory (L2-resident: 128 KB at dim 128) meets the TQ query values, three unfused fp32
// operations each under L2 (sub, mul, add), two under IP.  pq_term is the one place the rule's "never an FMA" is
// spelled: #pragma clang fp contract(off).  The scan's sum is additions only.
// Scan: a lane's row is M contiguous bytes, read as M / 8 8-byte words; a wave's 64 rows are 64 M contiguous bytes.
// The words run through a two-deep register pipeline that crosses step boundaries: word t + 2 is requested before
// the eight gathers of word t, and no load sits under a divergent branch -- lanes past the end of the launch read
// the last row's address and only the filing is decided.  Per code: v_bfe_u32, one address add, the read(s) with
// the sub-quantiser's offset as the instruction's immediate (e * 1024 * TQ < 64 K), TQ v_add_f32.  The sum over i is
// one dependent chain per (row, query); the TQ chains and the eight independent reads of a word are the
// parallelism that covers the LDS latency.  The sum starts at 0.0f: 0.0f + T[0] is T[0] bit for bit because no table
// entry is -0.0 (each starts at +0.0 and +0.0 + x is never -0.0).
#pragma once
#include "common.hpp"
#include "scan_f32.hpp"

namespace expann {

constexpr int kPQRowsStep = kBlock;  // rows of a workgroup step: one per lane
__host__ __device__ constexpr uint32_t pq_lds_bytes(uint32_t tq, uint32_t M) { return tq * M * 256u * 4u; }

// one step of a table entry, THE PQ RULE: every operation rounds by itself (F: float, or a vector of floats taken
// element by element -- pq_encode.hpp steps two centroids at once)
template <bool IP, typename F = float> __device__ __attribute__((always_inline)) inline F pq_term(F T, F q, F c) {
#pragma clang fp contract(off)
	if (IP) {
		const F pr = q * c;
		return T + pr;
	}
	const F t = q - c;
	const F sq = t * t;
	return T + sq;
}

// the TQ adjacent floats of table entry `e` (index i * 256 + code)
template <int TQ> __device__ __attribute__((always_inline)) inline void pq_entry_store(float* tab, uint32_t e, const float (&t)[TQ]) {
	if constexpr (TQ == 8) {
		reinterpret_cast<float4*>(tab)[2 * e] = float4{t[0], t[1], t[2], t[3]};
		reinterpret_cast<float4*>(tab)[2 * e + 1] = float4{t[4], t[5], t[6], t[7]};
	} else if constexpr (TQ == 4) {
		reinterpret_cast<float4*>(tab)[e] = float4{t[0], t[1], t[2], t[3]};
	} else if constexpr (TQ == 2) {
		reinterpret_cast<float2*>(tab)[e] = float2{t[0], t[1]};
	} else {
		tab[e] = t[0];
	}
}
template <int TQ> __device__ __attribute__((always_inline)) inline void pq_entry_add(const float* tab, uint32_t e, float (&s)[TQ]) {
	if constexpr (TQ == 8) {
		const float4 a = reinterpret_cast<const float4*>(tab)[2 * e], b = reinterpret_cast<const float4*>(tab)[2 * e + 1];
		s[0] = s[0] + a.x, s[1] = s[1] + a.y, s[2] = s[2] + a.z, s[3] = s[3] + a.w;
		s[4] = s[4] + b.x, s[5] = s[5] + b.y, s[6] = s[6] + b.z, s[7] = s[7] + b.w;
	} else if constexpr (TQ == 4) {
		const float4 a = reinterpret_cast<const float4*>(tab)[e];
		s[0] = s[0] + a.x, s[1] = s[1] + a.y, s[2] = s[2] + a.z, s[3] = s[3] + a.w;
	} else if constexpr (TQ == 2) {
		const float2 a = reinterpret_cast<const float2*>(tab)[e];
		s[0] = s[0] + a.x, s[1] = s[1] + a.y;
	} else {
		s[0] = s[0] + tab[e];
	}
}

template <int TQ, bool IP> __global__ __launch_bounds__(kBlock) void scan_pq_kernel(ScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
	float* tab = reinterpret_cast<float*>(pq_smem);  // [M][256][TQ]
	const uint32_t M = p.pq_m, U = M / 8, dsub = p.dim / M;
	const uint32_t tid = threadIdx.x;
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	const uint32_t q0 = qtile * TQ;
	const float* __restrict__ cb = p.pq_codebooks;
	const float* __restrict__ queries = (const float*)p.queries;
	const uint2* __restrict__ base = (const uint2*)p.base;
	const bool level0 = (p.tau == nullptr);

	// ---- prologue: the tables of the tile's queries (slots past m repeat the last query and never file) ----
	const float* qrow[TQ];
	float tau[TQ];
#pragma unroll
	for (int j = 0; j < TQ; ++j) {
		const uint32_t qi = (q0 + j < p.m) ? q0 + j : p.m - 1;
		qrow[j] = queries + (size_t)qi * p.dim;
		float tj = level0 ? __builtin_inff() : p.tau[qi];
		tj = (q0 + j < p.m) ? tj : -__builtin_inff();
		tau[j] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tj)));
	}
	for (uint32_t i = 0; i < M; ++i) {
		const float* c = cb + ((size_t)i * 256 + tid) * dsub;
		float T[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j)
			T[j] = 0.0f;
		for (uint32_t d = 0; d < dsub; ++d) {
			const float cv = c[d];
#pragma unroll
			for (int j = 0; j < TQ; ++j)
				T[j] = pq_term<IP>(T[j], qrow[j][i * dsub + d], cv);
		}
		pq_entry_store<TQ>(tab, i * 256 + tid, T);
	}
	__syncthreads();

	// ---- scan ----
	const uint32_t g0 = chunk * p.groups_per_block;
	uint32_t g1 = g0 + p.groups_per_block;
	if (g1 > p.n_groups_sel)
		g1 = p.n_groups_sel;
	constexpr uint32_t groups_step = kPQRowsStep / kRowsPerGroup;  // 16-row groups per workgroup step
	const uint32_t gsub = tid >> 4, r16 = tid & 15;
	// the row of this lane in the step that starts at group gs, or the last row (a valid address) where there is none
	auto src_of = [&](uint32_t gs) -> const uint2* {
		const uint32_t g = gs + gsub;
		const uint32_t row = g * p.group_stride * kRowsPerGroup + r16;
		return base + (size_t)((g < g1 && row < p.n_rows) ? row : p.n_rows - 1) * U;
	};
	// the stream of 8-byte words (step by step, word by word), two requests ahead of the gathers
	uint32_t pf_gs = g0, pf_u = 0;
	const uint2* pf_src = src_of(g0);
	auto fetch = [&]() -> uint2 {
		const uint2 v = pf_src[pf_u];
		if (++pf_u == U) {  // (uniform)
			pf_u = 0;
			pf_gs += groups_step;
			pf_src = src_of(pf_gs);
		}
		return v;
	};
	uint2 w0 = fetch(), w1 = fetch();

	uint64_t best[TQ];  // class minima (classmin level, scan_f32.hpp): class = (workgroup, 16-lane row of the wave)
#pragma unroll
	for (int j = 0; j < TQ; ++j)
		best[j] = kSentinelKey;
	for (uint32_t gs = g0; gs < g1; gs += groups_step) {
		const uint32_t g = gs + gsub;
		const bool gvalid = g < g1;
		const uint32_t row = g * p.group_stride * kRowsPerGroup + r16;
		const bool rvalid = gvalid && row < p.n_rows;
		float s[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j)
			s[j] = 0.0f;
		for (uint32_t u = 0; u < U; ++u) {
			const uint2 w = w0;
			w0 = w1;
			w1 = fetch();
			const float* tu = tab + (size_t)u * (8 * 256 * TQ);
#pragma unroll
			for (int e = 0; e < 8; ++e) {
				const uint32_t code = ((e < 4 ? w.x : w.y) >> (8 * (e & 3))) & 255u;
				pq_entry_add<TQ>(tu, e * 256 + code, s);
			}
		}
		unsigned long long any = 0;
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			if (IP)
				s[j] = 0.0f - s[j];  // (never -0.0)
			any |= __builtin_amdgcn_ballot_w64(rvalid && s[j] <= tau[j]);
		}
		if (level0 && p.classmin) {
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				const uint64_t key = rvalid ? make_key(s[j], row) : kSentinelKey;
				best[j] = key < best[j] ? key : best[j];
			}
		} else if (level0) {
			const uint32_t slot = g * kRowsPerGroup + r16;
			if (gvalid && slot < p.cap) {
#pragma unroll
				for (int j = 0; j < TQ; ++j)
					if (q0 + j < p.m)
						p.cand[(size_t)(q0 + j) * p.cap + slot] = rvalid ? make_key(s[j], row) : kSentinelKey;
			}
		} else if (any) {
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				if (rvalid && q0 + j < p.m && (s[j] < tau[j] || (s[j] == tau[j] && row <= p.tau_row[q0 + j]))) {
					const uint32_t slot = atomicAdd(&p.cand_cnt[q0 + j], 1u);
					if (slot < p.cap)
						p.cand[(size_t)(q0 + j) * p.cap + slot] = make_key(s[j], row);
				}
			}
		}
	}
	if (level0 && p.classmin) {
		const uint32_t lane = tid & 63, wave = tid >> 6;
		const uint32_t slot = chunk * 16 + wave * 4 + (lane >> 4);
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			uint64_t b = best[j];
#pragma unroll
			for (int o = 8; o >= 1; o >>= 1) {
				const uint64_t other = __shfl_xor(b, o, 16);
				b = other < b ? other : b;
			}
			if ((lane & 15) == 0 && slot < p.cap && q0 + j < p.m)
				p.cand[(size_t)(q0 + j) * p.cap + slot] = b;
		}
	}
}

}  // namespace expann
