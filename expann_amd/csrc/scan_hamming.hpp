// scan_hamming.hpp -- threshold-filter scans over packed-bit rows (EXPANN_DTYPE_B1), score = popcount(q xor b).
//
// A row is dim / 8 bytes, dimension j = bit j % 8 of byte j / 8; dim is a multiple of 64, so a row is dim / 64
// 8-byte units.  Scores are integers in [0, dim] and leave both scans final, as float: no re-rank follows.  Both
// forms keep the keys (score, row) <= (tau, tau_row), so they are exact under ties -- the normal case here -- and
// file the same keys in the same candidate lists.
//
// 1. scan_hamming_valu_kernel: v_xor + v_bcnt_u32_b32 (which accumulates) per dword and pair.  It takes ScanParams
//    with the contract of the 8-bit direct scan (levels, class minima, the tie rule).  A row is spread over
//    L = 1, 2, 4 or 8 lanes by dim (ham_lanes_per_row): lane l of a row reads units l, l + L, ... -- at 8-byte rows
//    one lane owns a row and a wave reads 512 contiguous bytes; from 512 bits on the 8 lanes of a row read 64
//    contiguous bytes per step -- and the partial counts meet in at most three DPP adds.  The TQ queries of the
//    workgroup sit in LDS (lanes of equal l read one address: broadcast).
//
// 2. scan_hamming_mfma_kernel: v_mfma_i32_16x16x64_i8 on bytes in {0, 1}.
//    Encoding: 0/1, accumulator = popcount(q & b), score = pop(q) + pop(b) - 2 acc.  The +-1 encoding needs no row
//    term but costs one more VALU operation per dword of the widening (2 x - 1 on four bytes) on the side that is
//    short, and an odd/even case in the threshold; pop(b) is 4 bytes per row, made once at build (ham_popcount_kernel),
//    and the epilogue is scan_gemm_i8.hpp's  bias[row] - 2 acc <= theta_q  with theta_q = floor(tau_q) - pop(q).
//    Widening: 16 bits -> 4 dwords of bytes, per dword  ((bits >> 4 w) & 15) * 0x204081 & 0x01010101  -- v_bfe_u32,
//    v_mul_u32_u24 (full rate: both factors are below 2^24, and the four shifted copies of the nibble do not overlap,
//    so nothing carries), v_and_b32: 12 VALU instructions per 16 bits (11: the first dword needs no shift, an and
//    does the extract).
//    Geometry: 512 threads, 8 waves; the workgroup holds kHamTQ = 64 queries, WIDENED ONCE into LDS as bytes
//    ([64][dim + 16]: the 16-byte pad makes the 16 rows of a fragment read hit all 64 banks once), and walks tiles
//    of kHamTB = 512 rows.  A tile stays packed in LDS ([512][dim / 8 + 4]: 2 - 33 KiB); wave w owns its rows
//    [64 w, 64 w + 64) as four 16-row columns.  The k-loop is outermost at every dim: per k-step a wave reads its
//    four 16-query fragments (4 ds_read_b128), and per column one uint16 (index 4 s + lane / 16 of row lane % 16),
//    widens it (12 VALU) and issues 4 MFMAs -- 48 VALU instructions against 16 MFMAs of 8 passes per k-step, the
//    widening of a row fragment used by the four query fragments.  64 accumulator registers; no scratch.
//    (One residency rule instead of registers up to 512 bits and LDS beyond: the LDS reads are 4 per 16 MFMAs.)
//    The tile range, the thresholds and the epilogue (level 0 at fixed slots, so a search forced onto this form
//    launches nothing else; the rare hit with one ballot and one atomic per quarter wave) are scan_tile.hpp's.
//    LDS at dim = 1024: 66 560 + 67 584 bytes, one workgroup (two waves per SIMD) per CU; kPlanHamMfmaMaxDim
//    (bf_plan.hpp) is where this form ends.
#pragma once
#include "scan_tile.hpp"

namespace expann {

constexpr int kHamMaxDim = 4096;    // bits per row
constexpr int kHamValuRows = 256;   // rows of a workgroup step of the VALU form at one lane per row
static_assert(kHamTB == 512, "tile rows");  // (the matrix-core form's geometry: scan_tile.hpp)

__host__ __device__ constexpr uint32_t ham_lanes_per_row(uint32_t dim) {
	return dim >= 512 ? 8u : (dim >= 256 ? 4u : (dim >= 128 ? 2u : 1u));
}
__host__ __device__ constexpr uint32_t ham_q_stride(uint32_t dim) { return dim + 16; }      // bytes of a widened query in LDS
__host__ __device__ constexpr uint32_t ham_row_stride(uint32_t dim) { return dim / 8 + 4; }  // bytes of a packed row in LDS
__host__ __device__ constexpr uint32_t ham_mfma_lds_bytes(uint32_t dim) {
	return kHamTQ * ham_q_stride(dim) + kHamTB * ham_row_stride(dim);
}

__device__ inline int ham_pop(uint32_t x, int acc) { return (int)__builtin_popcount(x) + acc; }  // v_bcnt_u32_b32

// ---- 1. VALU form ---------------------------------------------------------------------------------------------
template <int TQ> __global__ __launch_bounds__(kBlock) void scan_hamming_valu_kernel(ScanParams p) {
	__shared__ uint2 qs[TQ * (kHamMaxDim / 64)];
	const uint32_t U = p.dim / 64;  // 8-byte units per row
	const uint32_t L = ham_lanes_per_row(p.dim), LSH = L == 8 ? 3u : (L == 4 ? 2u : (L == 2 ? 1u : 0u));
	const uint32_t tid = threadIdx.x;
	const uint32_t l = tid & (L - 1), sub = tid >> LSH;  // lane of the row; the row's slot in the step
	const uint32_t groups_step = (kBlock >> LSH) / kRowsPerGroup;  // 16-row groups per workgroup step: 16 / L
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	const uint32_t q0 = qtile * TQ;
	const uint2* __restrict__ base = (const uint2*)p.base;
	const uint2* __restrict__ queries = (const uint2*)p.queries;
	const bool level0 = (p.tau == nullptr);

	for (uint32_t i = tid; i < TQ * U; i += kBlock) {
		const uint32_t j = i / U;
		const uint32_t qi = (q0 + j < p.m) ? q0 + j : p.m - 1;
		qs[i] = queries[(size_t)qi * U + (i - j * U)];
	}
	float tau[TQ];
#pragma unroll
	for (int j = 0; j < TQ; ++j) {
		const uint32_t qi = (q0 + j < p.m) ? q0 + j : p.m - 1;
		float tj = level0 ? __builtin_inff() : p.tau[qi];
		tj = (q0 + j < p.m) ? tj : -__builtin_inff();
		tau[j] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tj)));
	}
	__syncthreads();

	const uint32_t g0 = chunk * p.groups_per_block;
	uint32_t g1 = g0 + p.groups_per_block;
	if (g1 > p.n_groups_sel)
		g1 = p.n_groups_sel;
	uint64_t best[TQ];  // class minima (classmin level, scan_f32.hpp): class = (workgroup, 16-lane row of the wave)
#pragma unroll
	for (int j = 0; j < TQ; ++j)
		best[j] = kSentinelKey;
	for (uint32_t gs = g0; gs < g1; gs += groups_step) {
		const uint32_t g = gs + (sub >> 4);
		const bool gvalid = g < g1;
		const uint32_t row = g * p.group_stride * kRowsPerGroup + (sub & 15);
		const bool rvalid = gvalid && row < p.n_rows;
		const uint2* src = base + (size_t)(rvalid ? row : p.n_rows - 1) * U;
		int acc[TQ];
#pragma unroll
		for (int j = 0; j < TQ; ++j)
			acc[j] = 0;
		for (uint32_t u = l; u < U; u += L) {
			const uint2 b = src[u];
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				const uint2 q = qs[j * U + u];
				acc[j] = ham_pop(q.y ^ b.y, ham_pop(q.x ^ b.x, acc[j]));
			}
		}
		// the L lanes of a row: xor 1 and xor 2 inside a quad, then the other quad of the 8 (row_half_mirror: all
		// four lanes of a quad hold the same sum by then)
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			if (L >= 2)
				acc[j] += __builtin_amdgcn_update_dpp(0, acc[j], 0xB1, 0xF, 0xF, false);
			if (L >= 4)
				acc[j] += __builtin_amdgcn_update_dpp(0, acc[j], 0x4E, 0xF, 0xF, false);
			if (L >= 8)
				acc[j] += __builtin_amdgcn_update_dpp(0, acc[j], 0x141, 0xF, 0xF, false);
		}
		float s[TQ];
		unsigned long long any = 0;
#pragma unroll
		for (int j = 0; j < TQ; ++j) {
			s[j] = (float)acc[j];
			any |= __builtin_amdgcn_ballot_w64(rvalid && s[j] <= tau[j]);
		}
		if (level0 && p.classmin) {
#pragma unroll
			for (int j = 0; j < TQ; ++j) {
				const uint64_t key = rvalid ? make_key(s[j], row) : kSentinelKey;
				best[j] = key < best[j] ? key : best[j];
			}
		} else if (level0) {
			const uint32_t slot = g * kRowsPerGroup + (sub & 15);
			if (l == 0 && gvalid && slot < p.cap) {
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

// ---- 2. matrix-core form ----------------------------------------------------------------------------------------
// score = pop(q) + pop(b) - 2 acc: integers in [0, dim], exact as floats
struct HamPolicy {
	static constexpr bool kFloatTies = false;
	__device__ static int row_term(const TileScanParams& p, uint32_t row, bool valid) { return valid ? p.rowterm[row] : 0; }
	__device__ static int combine(const TileScanParams&, int rt, int acc) { return rt - 2 * acc; }
	__device__ static int query_term(const TileScanParams& p, uint32_t qi) { return p.qterm[qi]; }
};

// 16 bits -> 16 bytes in {0, 1}, bit j in byte j
__device__ inline ham_i32x4 ham_widen16(uint32_t bits) {
	ham_i32x4 v;
#pragma unroll
	for (int w = 0; w < 4; ++w)
		v[w] = (int)(__umul24((bits >> (4 * w)) & 15u, 0x204081u) & 0x01010101u);
	return v;
}

// popcount per row (build: pop(b)) -- one thread per row, 8-byte loads
static __global__ __launch_bounds__(kBlock) void ham_popcount_kernel(const void* rows, uint32_t n, uint32_t dim, int* out) {
	const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
	if (r >= n)
		return;
	const uint32_t U = dim / 64;
	const uint2* src = (const uint2*)rows + (size_t)r * U;
	int acc = 0;
	for (uint32_t u = 0; u < U; ++u) {
		const uint2 v = src[u];
		acc = ham_pop(v.y, ham_pop(v.x, acc));
	}
	out[r] = acc;
}
// pop(q) per query and, with thresholds, theta = floor(tau) - pop(q) (tau = +inf: every row passes)
static __global__ __launch_bounds__(kBlock) void ham_theta_kernel(const void* queries, uint32_t m, uint32_t dim,
                                                                  const float* tau, int* theta, int* popq) {
	const uint32_t qi = blockIdx.x * kBlock + threadIdx.x;
	if (qi >= m)
		return;
	const uint32_t U = dim / 64;
	const uint2* src = (const uint2*)queries + (size_t)qi * U;
	int acc = 0;
	for (uint32_t u = 0; u < U; ++u) {
		const uint2 v = src[u];
		acc = ham_pop(v.y, ham_pop(v.x, acc));
	}
	popq[qi] = acc;
	if (tau) {
		const float t = tau[qi];
		const int ft = !(t < 1.0e9f) ? 1000000000 : (t < 0.0f ? -1 : (int)__builtin_floorf(t));
		theta[qi] = ft - acc;
	}
}

__global__ __launch_bounds__(kHamThreads) void scan_hamming_mfma_kernel(TileScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char ham_smem[];
	const uint32_t KS = p.klen / 64;   // k-steps
	const uint32_t P16 = p.klen / 16;  // uint16 pieces per row
	const uint32_t DWR = p.klen / 32;  // dwords per packed row
	const uint32_t QS = ham_q_stride(p.klen), RS = ham_row_stride(p.klen);
	unsigned char* const qbytes = ham_smem;
	unsigned char* const rows_lds = ham_smem + kHamTQ * QS;
	TileLane w;
	if (!tile_range(p, w))
		return;

	// the workgroup's queries, widened once
	for (uint32_t pi = w.tid; pi < kHamTQ * P16; pi += kHamThreads) {
		const uint32_t qq = pi / P16, c = pi - qq * P16;
		const uint32_t qi = (w.q0 + qq < p.m) ? w.q0 + qq : p.m - 1;
		const uint32_t bits = ((const uint16_t*)p.a_operand)[(size_t)qi * P16 + c];
		*reinterpret_cast<ham_i32x4*>(qbytes + qq * QS + c * 16) = ham_widen16(bits);
	}
	int th[4][4];
	tile_thresholds(p, w, th);

	const uint32_t* __restrict__ base_dw = (const uint32_t*)p.base;
	uint32_t* const rows_dw = reinterpret_cast<uint32_t*>(rows_lds);
	const uint32_t RSW = RS / 4;  // = DWR + 1: odd strides, the 16 rows of a column read 16 banks

	for (uint32_t t = w.t0; t < w.t1; ++t) {
		const uint32_t row0 = t * p.tile_stride * kHamTB;
		__syncthreads();  // (the queries are in place; the tile before has been read)
		for (uint32_t d = w.tid; d < kHamTB * DWR; d += kHamThreads) {
			const uint32_t r = d / DWR, c = d - r * DWR;
			const uint32_t grow = (row0 + r < p.n_rows) ? row0 + r : p.n_rows - 1;
			rows_dw[r * RSW + c] = base_dw[(size_t)grow * DWR + c];
		}
		__syncthreads();

		ham_i32x4 acc[4][kHamNT];
		tile_clear(acc);
		const unsigned char* const qf = qbytes + w.i * QS + 16 * w.g;
		const unsigned char* const rf = rows_lds + (w.wave * 64 + w.i) * RS + 2 * w.g;
		for (uint32_t s = 0; s < KS; ++s) {
			ham_i32x4 a[4];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const ham_i32x4*>(qf + 16 * tq * QS + 64 * s);
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const uint32_t bits = *reinterpret_cast<const uint16_t*>(rf + 16 * tc * RS + 8 * s);
				const ham_i32x4 f = ham_widen16(bits);
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq], f, acc[tq][tc], 0, 0, 0);
			}
		}
		tile_epilogue<HamPolicy>(p, w, t, acc, th);
	}
}

}  // namespace expann
