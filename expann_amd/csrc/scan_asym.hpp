// scan_asym.hpp -- packed-bit rows (EXPANN_DTYPE_B1) scored against int8 queries on the int8 matrix cores:
// THE ASYMMETRIC RULE of include/expann_hip.h,
//     score(q, b) = - sum_j q_j (2 b_j - 1) = sum_j q_j - 2 sum_j q_j b_j .
//
// scan_asym_mfma_kernel = scan_stream_mfma_kernel<AsymCodec> (scan_tile.hpp: the geometry, the streamed stage loop,
// the epilogue).  A = the query bytes as they are (signed); B = the row bits widened to bytes in {0, 1} in
// registers (ham_widen16 of scan_hamming.hpp: 12 VALU instructions per 16 bits, the widened fragment used by four
// query fragments).  The accumulator is sum q_j b_j, |acc| <= 128 x 4096 = 2^19.  No row term: the epilogue tests
// -2 acc <= theta_q  with theta_q = floor(tau_q) - sum q (asym_theta_kernel makes both per query), and the ties are
// decided on the integers.  Scores are negative as often as positive: make_key orders them (float_to_ordered), as it
// does for -dot of the inner-product families.
//
// The stages: chunks of kAsymKC = 512 bits (8 k-steps), so every dim up to 4096 bits runs on the matrix cores.
// One stage holds the packed row chunk [512][kAsymKC / 8 + 4] (34 816 B) and the query chunk as bytes
// [64][kAsymKC + 16] (33 792 B) -- the pads of scan_hamming.hpp, so the fragment reads stay conflict-free -- and
// there are two stages: 137 216 B of the CU's 160 KiB.  A thread's stage registers are 8 x 8 B of rows + 4 x 16 B of
// queries.  Above kAsymKC the re-read query chunks are as many bytes as the tile's rows.
//
// One form for every m >= 1: a VALU form for small batches is out of scope -- a batch below 64 queries pays for the
// whole 64-query fragment set.
// The queries must be 16-byte aligned (they are read as 16-byte pieces; dim % 64 == 0 keeps every query so).
#pragma once
#include "scan_hamming.hpp"

namespace expann {

constexpr uint32_t kAsymKC = 512;                        // bits of the reduction dimension per stage
constexpr uint32_t kAsymRowStride = kAsymKC / 8 + 4;     // bytes of a packed row chunk in LDS (17 dwords: odd)
constexpr uint32_t kAsymQStride = kAsymKC + 16;          // bytes of a query chunk in LDS
constexpr uint32_t kAsymStageBytes = kHamTB * kAsymRowStride + kHamTQ * kAsymQStride;
constexpr uint32_t kAsymLdsBytes = 2 * kAsymStageBytes;
static_assert(kAsymRowStride == ham_row_stride(kAsymKC) && kAsymQStride == ham_q_stride(kAsymKC), "the pads of scan_hamming.hpp");
static_assert(kAsymStageBytes == 34816 + 33792 && kAsymLdsBytes == 137216 && kAsymLdsBytes <= 160 * 1024, "LDS budget per CU");
static_assert(kHamThreads == 512 && kHamTB == 512 && kHamTQ == 64, "the staging below: a thread per row, 32 threads per query");

// sum q per query and, with thresholds, theta = floor(tau) - sum q (tau = +inf: every row passes).  16 lanes per query.
static __global__ __launch_bounds__(kBlock) void asym_theta_kernel(const void* queries, uint32_t m, uint32_t dim, const float* tau,
                                                                   int* theta, int* sumq) {
	const uint32_t qi = blockIdx.x * (kBlock / 16) + threadIdx.x / 16, l = threadIdx.x & 15;
	const ham_i32x4* src = (const ham_i32x4*)queries + (size_t)(qi < m ? qi : m - 1) * (dim / 16);
	int acc = 0;
	for (uint32_t v = l; v < dim / 16; v += 16) {
		const ham_i32x4 x = src[v];
#pragma unroll
		for (int w = 0; w < 4; ++w)
			acc += (int)(int8_t)x[w] + (int)(int8_t)(x[w] >> 8) + (int)(int8_t)(x[w] >> 16) + (x[w] >> 24);  // v_bfe_i32
	}
	acc = reduce16_i32(acc);
	if (qi >= m || l != 0)
		return;
	sumq[qi] = acc;
	if (tau) {
		const float t = tau[qi];
		const int ft = !(t < 1.0e9f) ? 1000000000 : (t < -1.0e9f ? -1000000000 : (int)__builtin_floorf(t));
		theta[qi] = ft - acc;
	}
}

// score = sum q - 2 acc, |score| < 2^20: exact as floats
struct AsymPolicy {
	static constexpr bool kFloatTies = false;
	__device__ static int row_term(const TileScanParams&, uint32_t, bool) { return 0; }
	__device__ static int combine(const TileScanParams&, int, int acc) { return -2 * acc; }
	__device__ static int query_term(const TileScanParams& p, uint32_t qi) { return p.qterm[qi]; }
};

__device__ __attribute__((always_inline)) inline uint32_t asym_row_lanes_log2(uint32_t kw) {
	return kw > 256 ? 3u : (kw > 128 ? 2u : (kw > 64 ? 1u : 0u));
}

// The staging of one (tile, chunk): global -> registers, registers -> LDS.  kw = the chunk's bits (a multiple of 64).
// Rows: a chunk is kw / 64 units of 8 bytes; L = 1, 2, 4 or 8 lanes share a row (the power of two that covers the
// units), so a wave's load covers runs of consecutive bytes, and a thread holds L units: r = tid / L + j (512 / L).
// Queries: 32 lanes per query read its kw / 16 pieces of 16 bytes, a thread holds 4: q = tid / 32 + 16 j.
struct AsymCodec {
	using Policy = AsymPolicy;
	static constexpr uint32_t kKC = kAsymKC, kRowStride = kAsymRowStride, kQStride = kAsymQStride, kStageBytes = kAsymStageBytes;
	static constexpr uint32_t kLaneBytes = 2;  // of a row, per lane and k-step: 16 bits
	struct Stage {
		uint2 rows[8];
		ham_i32x4 q[4];
	};
	__device__ __attribute__((always_inline)) static void load(Stage& s, const TileScanParams& p, uint32_t tid, uint32_t row0,
	                                                          uint32_t q0, uint32_t c, uint32_t kw, bool with_q) {
		const uint32_t LSH = asym_row_lanes_log2(kw), L = 1u << LSH, U = kw / 64, RU = p.klen / 64;
		const uint32_t u = tid & (L - 1), rsub = tid >> LSH;
		const uint2* __restrict__ base = (const uint2*)p.base;
		// No load sits under a branch: a guarded load makes the register "the loaded value or the old one", and the compiler
		// then waits for each load before it issues the next.  All 8 (and 4) are issued back to back instead, the ones
		// store() will not use from an address of the same tile and chunk that is valid anyway (a cache hit).
		const uint32_t uc = u < U ? u : U - 1;
#pragma unroll
		for (uint32_t j = 0; j < 8; ++j) {
			const uint32_t r = (rsub + j * (kHamTB >> LSH)) & (kHamTB - 1);
			const uint32_t grow = (row0 + r < p.n_rows) ? row0 + r : p.n_rows - 1;
			s.rows[j] = base[(size_t)grow * RU + c * (kAsymKC / 64) + uc];
		}
		if (with_q) {
			const uint32_t v = tid & 31, V = kw / 16;
			const uint32_t vc = v < V ? v : V - 1;
			const ham_i32x4* __restrict__ qsrc = (const ham_i32x4*)p.a_operand;
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) {
				const uint32_t qq = (tid >> 5) + 16 * j;
				const uint32_t qi = (q0 + qq < p.m) ? q0 + qq : p.m - 1;
				s.q[j] = qsrc[(size_t)qi * (p.klen / 16) + c * (kAsymKC / 16) + vc];
			}
		}
	}
	__device__ __attribute__((always_inline)) static void store(const Stage& s, unsigned char* rbuf, unsigned char* qbuf, uint32_t tid,
	                                                           uint32_t kw, bool with_q) {
		const uint32_t LSH = asym_row_lanes_log2(kw), L = 1u << LSH, U = kw / 64;
		const uint32_t u = tid & (L - 1), rsub = tid >> LSH;
#pragma unroll
		for (uint32_t j = 0; j < 8; ++j) {
			if (j < L && u < U) {
				const uint32_t r = rsub + j * (kHamTB >> LSH);
				uint32_t* dst = reinterpret_cast<uint32_t*>(rbuf + r * kAsymRowStride) + 2 * u;
				dst[0] = s.rows[j].x;
				dst[1] = s.rows[j].y;
			}
		}
		if (with_q) {
			const uint32_t v = tid & 31, V = kw / 16;
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j)
				if (v < V)
					*reinterpret_cast<ham_i32x4*>(qbuf + ((tid >> 5) + 16 * j) * kAsymQStride + 16 * v) = s.q[j];
		}
	}
	__device__ __attribute__((always_inline)) static ham_i32x4 b_fragment(const unsigned char* at) {
		return ham_widen16(*reinterpret_cast<const uint16_t*>(at));
	}
};

constexpr auto scan_asym_mfma_kernel = scan_stream_mfma_kernel<AsymCodec>;

}  // namespace expann
