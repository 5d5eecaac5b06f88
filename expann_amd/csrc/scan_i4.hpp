// scan_i4.hpp -- 4-bit rows (EXPANN_DTYPE_I4) scored against int8 queries on the int8 matrix cores: THE I4 RULE of
// include/expann_hip.h.  A row is dim / 2 bytes, element 2 j the low nibble of byte j and element 2 j + 1 the high
// one, each a two's-complement value b_j in [-8, 7]; a query is dim signed bytes.
//     EXPANN_METRIC_IP: score = - sum_j q_j b_j          EXPANN_METRIC_L2: score = sum_j (q_j - b_j)^2
// an exact int32, reported and ranked as (float)score, then by lower id.
//
// gfx950 has no int4 matrix instruction: scan_i4_mfma_kernel widens the nibbles to bytes in registers in front of
// v_mfma_i32_16x16x64_i8.  Geometry (scan_hamming.hpp's): 512 threads in 8 waves, kHamTQ = 64 queries per workgroup
// as four 16-query A fragments, tiles of kHamTB = 512 rows; wave w owns rows [64 w, 64 w + 64) of the tile as four
// 16-row columns; 64 accumulator registers, no scratch.  Level 0 (no thresholds) writes the key of every (query,
// row) of its tiles at the row's fixed slot; the rare-hit epilogue applies the tie rule with one ballot and one
// atomic per quarter wave.  Its own design is in three places.
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
//    Overlap: the global loads of stage i + 1 are issued BEFORE the k-steps of stage i and stored to the other
//    stage's LDS after them.  No load sits under a branch.  One barrier per stage: it publishes stage i and says
//    that the buffer about to be overwritten has been read.
//    dim <= kI4KC: one chunk per tile, and the query chunk is staged ONCE per workgroup (in stage 0's query area).
//    A last chunk shorter than kI4KC (64 elements) is simply shorter: fewer loads kept, one k-step.
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

struct I4Params {
	const void* base;         // [n_rows][dim / 2] packed nibbles
	const int* rowterm;       // [n_rows] sum b^2 (L2); nullptr: inner product
	uint32_t n_rows;
	uint32_t n_tiles_sel;     // kHamTB-row tiles this launch visits: tile j of the launch is base tile j * tile_stride
	uint32_t tile_stride;
	uint32_t tiles_per_block;
	uint32_t n_qtiles;
	const void* queries;      // [m][dim] int8, permuted inside every 16-byte group (i4_theta_kernel)
	const int* theta;         // [m] floor(tau) - qterm (+ the float slack); unused at level 0
	const int* qterm;         // [m]
	const float* tau;         // [m] the threshold itself (rare path); unused at level 0
	const uint32_t* tau_row;  // [m] row of the threshold key
	uint32_t m;
	uint32_t* cand_cnt;
	uint64_t* cand;
	uint32_t cap;
	uint32_t dim;             // elements of a row = bytes of a query
	uint32_t level0;          // 1: no thresholds, the key of (query, row) goes to slot j * kHamTB + row in tile
};

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

// The staging of one (tile, chunk): global -> registers, registers -> LDS.  kw = the chunk's elements (64 or 128).
// Rows: a chunk is kw / 32 pieces of 16 bytes; 4 lanes share a row, so a wave's load covers runs of 64 consecutive
// bytes, and a thread holds 4 pieces: r = tid / 4 + 128 j.  Queries: 8 lanes per query read its kw / 16 pieces.
struct I4Stage {
	ham_i32x4 rows[4];
	ham_i32x4 q;
};
__device__ __attribute__((always_inline)) inline void i4_load(I4Stage& s, const I4Params& p, uint32_t tid, uint32_t row0,
                                                              uint32_t q0, uint32_t c, uint32_t kw, bool with_q) {
	const uint32_t U = kw / 32, RP = p.dim / 32;
	const uint32_t u = tid & 3, rsub = tid >> 2;
	const ham_i32x4* __restrict__ base = (const ham_i32x4*)p.base;
	// No load sits under a branch (scan_asym.hpp: a guarded load serialises the loads).  The pieces i4_store will not
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
		s.q = ((const ham_i32x4*)p.queries)[(size_t)qi * (p.dim / 16) + c * (kI4KC / 16) + vc];
	}
}
__device__ __attribute__((always_inline)) inline void i4_store(const I4Stage& s, unsigned char* rbuf, unsigned char* qbuf,
                                                               uint32_t tid, uint32_t kw, bool with_q) {
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

__global__ __launch_bounds__(kHamThreads) void scan_i4_mfma_kernel(I4Params p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char i4_smem[];
	constexpr uint32_t RS = kI4RowStride, QS = kI4QStride, QOFF = kHamTB * kI4RowStride;
	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const uint32_t i = lane & 15, g = lane >> 4;
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	const uint32_t q0 = qtile * kHamTQ;
	const uint32_t NC = (p.dim + kI4KC - 1) / kI4KC;  // chunks of the reduction dimension
	const bool stream_q = NC > 1;                    // (one chunk: the queries are staged once, in stage 0)
	const bool l2 = p.rowterm != nullptr;
	constexpr int kNever = -2147483647 - 1;

	const uint32_t t0 = chunk * p.tiles_per_block;
	uint32_t t1 = t0 + p.tiles_per_block;
	if (t1 > p.n_tiles_sel)
		t1 = p.n_tiles_sel;
	if (t0 >= t1)
		return;
	const uint32_t n_items = (t1 - t0) * NC;

	// thresholds of the lane's 16 queries: fragment tq, register e = query 16 tq + 4 g + e (a padded slot never matches)
	int th[4][4];
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const uint32_t qi = q0 + 16 * tq + 4 * g + e;
			th[tq][e] = (qi < p.m && !p.level0) ? p.theta[qi] : kNever;
		}

	I4Stage st;
	uint32_t t = t0, c = 0;
	uint32_t kw = p.dim < kI4KC ? p.dim : kI4KC;
	i4_load(st, p, tid, t * p.tile_stride * kHamTB, q0, 0, kw, true);
	i4_store(st, i4_smem, i4_smem + QOFF, tid, kw, true);

	ham_i32x4 acc[4][kHamNT];
	for (uint32_t it = 0; it < n_items; ++it) {
		const uint32_t row0 = t * p.tile_stride * kHamTB;
		uint32_t tn = t, cn = c + 1;
		if (cn == NC) {
			cn = 0;
			tn = t + 1;
		}
		const bool more = it + 1 < n_items;
		const uint32_t kwn = (p.dim - cn * kI4KC) < kI4KC ? (p.dim - cn * kI4KC) : kI4KC;
		if (more)  // in flight while this stage is multiplied
			i4_load(st, p, tid, tn * p.tile_stride * kHamTB, q0, cn, kwn, stream_q);
		__syncthreads();  // this stage is in place; the other one has been read

		unsigned char* const sbuf = i4_smem + (it & 1) * kI4StageBytes;
		unsigned char* const obuf = i4_smem + ((it + 1) & 1) * kI4StageBytes;
		if (c == 0) {
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
#pragma unroll
				for (int tc = 0; tc < kHamNT; ++tc)
					acc[tq][tc] = ham_i32x4{0, 0, 0, 0};
		}
		const unsigned char* const qf = (stream_q ? sbuf : i4_smem) + QOFF + i * QS + 16 * g;
		const unsigned char* const rf = sbuf + (wave * 64 + i) * RS + 8 * g;
		const uint32_t KS = kw / 64;
		for (uint32_t s = 0; s < KS; ++s) {
			ham_i32x4 a[4];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const ham_i32x4*>(qf + 16 * tq * QS + 64 * s);
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const uint2 x = *reinterpret_cast<const uint2*>(rf + 16 * tc * RS + 32 * s);
				const uint32_t y0 = x.x ^ 0x88888888u, y1 = x.y ^ 0x88888888u;
				const ham_i32x4 f = {(int)(y0 & 0x0F0F0F0Fu), (int)((y0 >> 4) & 0x0F0F0F0Fu), (int)(y1 & 0x0F0F0F0Fu),
				                     (int)((y1 >> 4) & 0x0F0F0F0Fu)};
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq], f, acc[tq][tc], 0, 0, 0);
			}
		}
		if (more)
			i4_store(st, obuf, obuf + QOFF, tid, kwn, stream_q);

		if (c == NC - 1) {
			// epilogue: lane (i, g) holds, for column tc, row 16 tc + i of the wave against queries 16 tq + 4 g + e
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const uint32_t local = wave * 64 + 16 * tc + i;
				const uint32_t brow = row0 + local;
				const bool bvalid = brow < p.n_rows;
				const int rt = (l2 && bvalid) ? p.rowterm[brow] : 0;
#pragma unroll
				for (int tq = 0; tq < 4; ++tq) {
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						const int tv = l2 ? rt - 2 * acc[tq][tc][e] : -acc[tq][tc][e];
						const uint32_t qi = q0 + 16 * tq + 4 * g + e;
						if (p.level0) {
							const uint32_t slot = t * kHamTB + local;
							if (qi < p.m && slot < p.cap)
								p.cand[(size_t)qi * p.cap + slot] =
								    bvalid ? make_key((float)(tv + p.qterm[qi]), brow) : kSentinelKey;
							continue;
						}
						bool hit = bvalid && tv <= th[tq][e];
						if (__builtin_amdgcn_ballot_w64(hit) == 0)
							continue;
						// rare path: the tie rule on the floats, then one atomic per quarter wave (its 16 lanes share the query)
						float sf = 0.0f;
						if (hit) {
							sf = (float)(tv + p.qterm[qi]);
							const float tau = p.tau[qi];
							hit = sf < tau || (sf == tau && brow <= p.tau_row[qi]);
						}
						const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
						const uint32_t seg = (uint32_t)(mask >> (lane & 48)) & 0xFFFFu;
						uint32_t slot0 = 0;
						if (i == 0 && seg)
							slot0 = atomicAdd(&p.cand_cnt[qi], (uint32_t)__builtin_popcount(seg));
						slot0 = __shfl(slot0, lane & 48);
						const uint32_t slot = slot0 + (uint32_t)__builtin_popcount(seg & ((1u << i) - 1u));
						if (hit && slot < p.cap)
							p.cand[(size_t)qi * p.cap + slot] = make_key((float)(tv + p.qterm[qi]), brow);
					}
				}
			}
		}
		t = tn;
		c = cn;
		kw = kwn;
	}
}

}  // namespace expann
