// scan_i4.hpp -- 4-bit rows (EXPANN_DTYPE_I4) scored against int8 queries on the int8 matrix cores: THE I4 RULE of
// include/expann_hip.h.  A row is dim / 2 bytes, element 2 j the low nibble of byte j and element 2 j + 1 the high
// one, each a two's-complement value b_j in [-8, 7]; a query is dim signed bytes.
//     EXPANN_METRIC_IP: score = - sum_j q_j b_j          EXPANN_METRIC_L2: score = sum_j (q_j - b_j)^2
// an exact int32, reported and ranked as (float)score, then by lower id.
//
// gfx950 has no int4 matrix instruction: scan_i4_mfma_kernel = scan_stream_mfma_kernel<I4Codec> (scan_tile.hpp: the
// geometry, the streamed stage loop, the epilogue) widens the nibbles to bytes in registers in front of
// v_mfma_i32_16x16x64_i8.  Its own design is in three places.
//
// 1. Widening in offset binary, and a permuted query so that it costs nothing more.  A lane's B operand for one
//    k-step is 16 elements = 8 packed bytes = two dwords x.  y = x ^ 0x88888888 turns every nibble s into u = s + 8
//    in [0, 15]; y & 0x0F0F0F0F and (y >> 4) & 0x0F0F0F0F are two operand dwords (bytes in [0, 15], no per-byte sign
//    extension): 4 VALU instructions (v_xor, v_and, v_lshrrev, v_and) per 8 elements against 12 per 16 for bits.  The two dwords hold the EVEN and the ODD elements, so inside a 16-element group the k order of
//    the operand is  0 2 4 6 | 1 3 5 7 | 8 10 12 14 | 9 11 13 15.  A sum over k does not care about the order as long
//    as both operands agree: i4_theta_kernel writes a copy of the queries with this permutation inside every 16-byte
//    group, once per query, and the tile loop reads that copy -- no v_perm, nothing per tile.  The offset is undone
//    per query: q . b = q . u - 8 sum q.  The accumulator is acc = q . u, |acc| <= 128 x 15 x 4096 < 2^23.
//
// 2. Prep and row terms.  i4_theta_kernel (16 lanes per query, one 16-byte group per lane and step) writes the
//    permuted queries, the per-query term folded into one integer
//        IP: qterm = 8 sum q                     (score = -acc + qterm)
//        L2: qterm = sum q^2 + 16 sum q          (score = rowterm - 2 acc + qterm)
//    and, with thresholds, theta_q = floor(tau_q) - qterm.  The epilogue is  rowterm[row] - 2 acc <= theta_q  for L2
//    and  -acc <= theta_q  for IP; padded query slots hold kNever and never match.  i4_rowterm_kernel makes
//    rowterm = sum b^2 per row (4 bytes a row) once, when the rows arrive; IP has no row term.
//    Scores from 2^24 on (L2 above dim 896 only) round as floats, and the ranking is the float's: scores that round
//    to tau are ties of tau.  There theta_q carries a slack of 4 (half an ulp below 2^27; 135^2 x 4096 < 2^27), and
//    the rare path decides on the floats themselves: (float)score < tau, or equal and row <= tau_row.
//
// 3. Stages.  The reduction dimension is streamed in chunks of kI4KC = 128 elements (2 k-steps), the accumulators
//    live across the chunks of a tile.  A stage holds the packed row chunk [512][kI4KC / 2 + 16] (40 960 B) and the
//    permuted query chunk [64][kI4KC + 16] (9 216 B): 50 176 B, two stages 100 352 B of the CU's 160 KiB, one
//    workgroup (two waves per SIMD) per CU.  kI4KC = 256 would be 91 136 B a stage and does not fit twice.
//    The pads: a lane reads 8 bytes of a row (ds_read_b64), so half a wave -- 16 rows x 2 quarter-k lanes -- reads 4
//    consecutive dwords per row; a row stride of 20 dwords puts the 16 rows at 20 i mod 64 = sixteen distinct
//    multiples of 4, all 64 banks once (ham_row_stride's odd stride serves 2-byte reads, not these).  The query
//    stride of 36 dwords does the same for the 16-byte A reads (36 i mod 64: sixteen distinct multiples of 4).
//    Two stages, not three: the loads of stage i + 1 are in registers (4 x 16 B of rows + 16 B of queries per
//    thread) while stage i is multiplied, so global latency is covered by one stage of 32 MFMAs per wave already; a
//    third stage would only move the LDS store earlier, and the store is 5 ds_write_b128 per thread.
//    A chunk shorter than kI4KC is 64 elements: one k-step.
//
// One form for every m >= 1: a batch below 64 queries pays for the whole 64-query fragment set.
// Rows and queries must be 16-byte aligned on the device (read as 16-byte pieces; dim % 64 == 0 keeps every row so).
#pragma once
#include "scan_hamming.hpp"

namespace expann {

constexpr uint32_t kI4KC = 128;                     // elements of the reduction dimension per stage
constexpr uint32_t kI4RowStride = kI4KC / 2 + 16;   // bytes of a packed row chunk in LDS (20 dwords)
constexpr uint32_t kI4QStride = kI4KC + 16;         // bytes of a query chunk in LDS (36 dwords)
constexpr uint32_t kI4StageBytes = kHamTB * kI4RowStride + kHamTQ * kI4QStride;
constexpr uint32_t kI4LdsBytes = 2 * kI4StageBytes;
static_assert(kI4RowStride % 16 == 0 && kI4QStride % 16 == 0, "16-byte LDS stores");
static_assert((kI4RowStride / 4) % 64 == 20 && (kI4QStride / 4) % 64 == 36, "the bank reasoning of the header comment");
static_assert(kI4StageBytes == 40960 + 9216 && kI4LdsBytes == 100352 && kI4LdsBytes <= 160 * 1024, "LDS budget per CU");
static_assert(kHamTB * (256 / 2 + 16) + kHamTQ * (256 + 16) == 91136 && 2 * 91136 > 160 * 1024, "why not 256-element chunks");
static_assert(kHamThreads == 512 && kHamTB == 512 && kHamTQ == 64, "the staging below: 4 threads per row, 8 per query");

// sum b^2 per row -- one thread per row, 16-byte loads (rows arrive: expann_build, expann_set_base_device)
static __global__ __launch_bounds__(kBlock) void i4_rowterm_kernel(const void* rows, uint32_t n, uint32_t dim, int* out) {
	const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
	if (r >= n)
		return;
	const uint32_t P = dim / 32;  // 16-byte pieces per row
	const ham_i32x4* src = (const ham_i32x4*)rows + (size_t)r * P;
	int acc = 0;
	for (uint32_t v = 0; v < P; ++v) {
		const ham_i32x4 x = src[v];
#pragma unroll
		for (int w = 0; w < 4; ++w)
#pragma unroll
			for (int nb = 0; nb < 8; ++nb) {
				const int b = (int)((uint32_t)x[w] << (28 - 4 * nb)) >> 28;  // v_bfe_i32
				acc += b * b;
			}
	}
	out[r] = acc;
}

// The permuted copy of the queries, qterm per query and, with thresholds, theta = floor(tau) - qterm (tau = +inf:
// every row passes).  16 lanes per query; a lane's 16-byte piece is one 16-element group of the permutation.
static __global__ __launch_bounds__(kBlock) void i4_theta_kernel(const void* queries, uint32_t m, uint32_t dim, int l2,
                                                                 const float* tau, void* qperm, int* theta, int* qterm) {
	const uint32_t qi = blockIdx.x * (kBlock / 16) + threadIdx.x / 16, l = threadIdx.x & 15;
	const uint32_t qc = qi < m ? qi : m - 1;  // (lanes past m recompute the last query and write nothing)
	const ham_i32x4* src = (const ham_i32x4*)queries + (size_t)qc * (dim / 16);
	ham_i32x4* dst = (ham_i32x4*)qperm + (size_t)qc * (dim / 16);
	int s1 = 0, s2 = 0;
	for (uint32_t v = l; v < dim / 16; v += 16) {
		const ham_i32x4 x = src[v];
#pragma unroll
		for (int w = 0; w < 4; ++w)
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				const int q = (int)((uint32_t)x[w] << (24 - 8 * b)) >> 24;
				s1 += q;
				s2 += q * q;
			}
		// bytes 0 2 4 6 | 1 3 5 7 of a dword pair: the even bytes of (lo, hi), then the odd ones
		const auto even = [](uint32_t lo, uint32_t hi) {
			return (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi << 8) & 0xFF000000u);
		};
		ham_i32x4 y;
		y[0] = (int)even((uint32_t)x[0], (uint32_t)x[1]);
		y[1] = (int)even((uint32_t)x[0] >> 8, (uint32_t)x[1] >> 8);
		y[2] = (int)even((uint32_t)x[2], (uint32_t)x[3]);
		y[3] = (int)even((uint32_t)x[2] >> 8, (uint32_t)x[3] >> 8);
		if (qi < m)
			dst[v] = y;
	}
	s1 = reduce16_i32(s1);
	s2 = reduce16_i32(s2);
	if (qi >= m || l != 0)
		return;
	const int qt = l2 ? s2 + 16 * s1 : 8 * s1;
	qterm[qi] = qt;
	if (tau) {
		const float t = tau[qi];
		int ft = !(t < 1.0e9f) ? 1000000000 : (t < -1.0e9f ? -1000000000 : (int)__builtin_floorf(t));
		if (t >= 16777216.0f && t < 1.0e9f)  // scores that round to tau as floats are its ties: half an ulp below 2^27
			ft += 4;
		theta[qi] = ft - qt;
	}
}

// IP (no row terms): score = -acc + qterm.  L2: score = rowterm - 2 acc + qterm, which passes 2^24 above dim 896 --
// float ties (2. of the header comment).
struct I4Policy {
	static constexpr bool kFloatTies = true;
	__device__ static int row_term(const TileScanParams& p, uint32_t row, bool valid) {
		return (p.rowterm != nullptr && valid) ? p.rowterm[row] : 0;
	}
	__device__ static int combine(const TileScanParams& p, int rt, int acc) {
		return rt - (int)((uint32_t)acc << (p.rowterm != nullptr ? 1u : 0u));  // (rt is 0 without row terms)
	}
	__device__ static int query_term(const TileScanParams& p, uint32_t qi) { return p.qterm[qi]; }
};

// The staging of one (tile, chunk): global -> registers, registers -> LDS.  kw = the chunk's elements (64 or 128).
// Rows: a chunk is kw / 32 pieces of 16 bytes; 4 lanes share a row, so a wave's load covers runs of 64 consecutive
// bytes, and a thread holds 4 pieces: r = tid / 4 + 128 j.  Queries: 8 lanes per query read its kw / 16 pieces.
struct I4Codec {
	using Policy = I4Policy;
	static constexpr uint32_t kKC = kI4KC, kRowStride = kI4RowStride, kQStride = kI4QStride, kStageBytes = kI4StageBytes;
	static constexpr uint32_t kLaneBytes = 8;  // of a row, per lane and k-step: 16 nibbles
	struct Stage {
		ham_i32x4 rows[4];
		ham_i32x4 q;
	};
	__device__ __attribute__((always_inline)) static void load(Stage& s, const TileScanParams& p, uint32_t tid, uint32_t row0,
	                                                          uint32_t q0, uint32_t c, uint32_t kw, bool with_q) {
		const uint32_t U = kw / 32, RP = p.klen / 32;
		const uint32_t u = tid & 3, rsub = tid >> 2;
		const ham_i32x4* __restrict__ base = (const ham_i32x4*)p.base;
		// No load sits under a branch (scan_asym.hpp: a guarded load serialises the loads).  The pieces store() will not
		// use come from an address of the same tile and chunk that is valid anyway (a cache hit).
		const uint32_t uc = u < U ? u : U - 1;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const uint32_t r = rsub + j * (kHamTB / 4);
			const uint32_t grow = (row0 + r < p.n_rows) ? row0 + r : p.n_rows - 1;
			s.rows[j] = base[(size_t)grow * RP + c * (kI4KC / 32) + uc];
		}
		if (with_q) {
			const uint32_t v = tid & 7, V = kw / 16;
			const uint32_t vc = v < V ? v : V - 1;
			const uint32_t qq = tid >> 3;
			const uint32_t qi = (q0 + qq < p.m) ? q0 + qq : p.m - 1;
			s.q = ((const ham_i32x4*)p.a_operand)[(size_t)qi * (p.klen / 16) + c * (kI4KC / 16) + vc];
		}
	}
	__device__ __attribute__((always_inline)) static void store(const Stage& s, unsigned char* rbuf, unsigned char* qbuf, uint32_t tid,
	                                                           uint32_t kw, bool with_q) {
		const uint32_t U = kw / 32;
		const uint32_t u = tid & 3, rsub = tid >> 2;
		if (u < U) {
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j)
				*reinterpret_cast<ham_i32x4*>(rbuf + (rsub + j * (kHamTB / 4)) * kI4RowStride + 16 * u) = s.rows[j];
		}
		if (with_q && (tid & 7) < kw / 16)
			*reinterpret_cast<ham_i32x4*>(qbuf + (tid >> 3) * kI4QStride + 16 * (tid & 7)) = s.q;
	}
	// (1. of the header comment: offset binary, the even elements and the odd ones)
	__device__ __attribute__((always_inline)) static ham_i32x4 b_fragment(const unsigned char* at) {
		const uint2 x = *reinterpret_cast<const uint2*>(at);
		const uint32_t y0 = x.x ^ 0x88888888u, y1 = x.y ^ 0x88888888u;
		return ham_i32x4{(int)(y0 & 0x0F0F0F0Fu), (int)((y0 >> 4) & 0x0F0F0F0Fu), (int)(y1 & 0x0F0F0F0Fu),
		                 (int)((y1 >> 4) & 0x0F0F0F0Fu)};
	}
};

constexpr auto scan_i4_mfma_kernel = scan_stream_mfma_kernel<I4Codec>;

}  // namespace expann
