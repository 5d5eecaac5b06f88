// scan_asym.hpp -- packed-bit rows (EXPANN_DTYPE_B1) scored against int8 queries on the int8 matrix cores:
// THE ASYMMETRIC RULE of include/expann_hip.h,
//     score(q, b) = - sum_j q_j (2 b_j - 1) = sum_j q_j - 2 sum_j q_j b_j .
//
// scan_asym_mfma_kernel: v_mfma_i32_16x16x64_i8.  A = the query bytes as they are (signed); B = the row bits widened
// to bytes in {0, 1} in registers (ham_widen16 of scan_hamming.hpp: 12 VALU instructions per 16 bits, the widened
// fragment used by four query fragments).  The accumulator is sum q_j b_j, |acc| <= 128 x 4096 = 2^19.  No row term:
// the epilogue tests  -2 acc <= theta_q  with theta_q = floor(tau_q) - sum q (asym_theta_kernel makes both per
// query), and the rare path applies the tie rule (score, row) <= (tau, tau_row) with one ballot and one atomic per
// quarter wave, as the Hamming matrix-core epilogue does.  Level 0 (no thresholds) writes the key of every (query,
// row) of its tiles at the row's fixed slot, so the threshold ladder runs this kernel alone.  Scores are negative as
// often as positive: make_key orders them (float_to_ordered), as it does for -dot of the inner-product families.
//
// Geometry (scan_hamming.hpp's): 512 threads in 8 waves, kHamTQ = 64 queries per workgroup, tiles of kHamTB = 512
// rows; wave w owns rows [64 w, 64 w + 64) of the tile as four 16-row columns; 64 accumulator registers, no scratch.
//
// What is new here: the reduction dimension is STREAMED.  It is cut into chunks of kAsymKC = 512 bits (8 k-steps),
// the accumulators live across the chunks of a tile, and so every dim up to 4096 bits runs on the matrix cores.
// One stage holds the packed row chunk [512][kAsymKC / 8 + 4] (34 816 B) and the query chunk as bytes
// [64][kAsymKC + 16] (33 792 B) -- the pads of scan_hamming.hpp, so the fragment reads stay conflict-free -- and
// there are two stages: 137 216 B of the CU's 160 KiB, one workgroup (two waves per SIMD) per CU.
// Overlap: the global loads of stage i + 1 are issued into registers (8 x 8 B of rows + 4 x 16 B of queries per
// thread) BEFORE the k-steps of stage i and stored to the other stage's LDS after them, so they are in flight while
// the waves multiply.  One barrier per stage: it publishes stage i and, since every wave's store of stage i + 1
// follows its own k-steps of stage i - 1 ... i, it also says that the buffer about to be overwritten has been read.
// Small dims: with dim <= kAsymKC there is one chunk per tile and the query chunk is loaded ONCE per workgroup
// (into stage 0's query area; stage 1's stays unused); with dim < kAsymKC a tile's stage is simply shorter -- fewer
// loads and fewer k-steps at the same LDS strides (chosen over packing kAsymKC / dim tiles into a stage: the tile
// loop, the slots of level 0 and the epilogue stay those of one tile).  The last chunk of a dim that is no multiple
// of kAsymKC is shorter in the same way.
// Above kAsymKC the query chunks are re-read (from L2) for every tile: as many bytes as the tile's rows.
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

struct AsymParams {
	const void* base;         // [n_rows][dim / 8] packed bits
	uint32_t n_rows;
	uint32_t n_tiles_sel;     // kHamTB-row tiles this launch visits: tile j of the launch is base tile j * tile_stride
	uint32_t tile_stride;
	uint32_t tiles_per_block;
	uint32_t n_qtiles;
	const void* queries;      // [m][dim] int8
	const int* theta;         // [m] floor(tau) - sum q; unused at level 0
	const int* sumq;          // [m]
	const uint32_t* tau_row;  // [m] row of the threshold key
	uint32_t m;
	uint32_t* cand_cnt;
	uint64_t* cand;
	uint32_t cap;
	uint32_t dim;             // bits of a row = bytes of a query
	uint32_t level0;          // 1: no thresholds, the key of (query, row) goes to slot j * kHamTB + row in tile
};

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

// The staging of one (tile, chunk): global -> registers, registers -> LDS.  kw = the chunk's bits (a multiple of 64).
// Rows: a chunk is kw / 64 units of 8 bytes; L = 1, 2, 4 or 8 lanes share a row (the power of two that covers the
// units), so a wave's load covers runs of consecutive bytes, and a thread holds L units: r = tid / L + j (512 / L).
// Queries: 32 lanes per query read its kw / 16 pieces of 16 bytes, a thread holds 4: q = tid / 32 + 16 j.
struct AsymStage {
	uint2 rows[8];
	ham_i32x4 q[4];
};
__device__ __attribute__((always_inline)) inline uint32_t asym_row_lanes_log2(uint32_t kw) {
	return kw > 256 ? 3u : (kw > 128 ? 2u : (kw > 64 ? 1u : 0u));
}
__device__ __attribute__((always_inline)) inline void asym_load(AsymStage& s, const AsymParams& p, uint32_t tid, uint32_t row0,
                                                                uint32_t q0, uint32_t c, uint32_t kw, bool with_q) {
	const uint32_t LSH = asym_row_lanes_log2(kw), L = 1u << LSH, U = kw / 64, RU = p.dim / 64;
	const uint32_t u = tid & (L - 1), rsub = tid >> LSH;
	const uint2* __restrict__ base = (const uint2*)p.base;
	// No load sits under a branch: a guarded load makes the register "the loaded value or the old one", and the compiler
	// then waits for each load before it issues the next.  All 8 (and 4) are issued back to back instead, the ones
	// asym_store will not use from an address of the same tile and chunk that is valid anyway (a cache hit).
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
		const ham_i32x4* __restrict__ qsrc = (const ham_i32x4*)p.queries;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const uint32_t qq = (tid >> 5) + 16 * j;
			const uint32_t qi = (q0 + qq < p.m) ? q0 + qq : p.m - 1;
			s.q[j] = qsrc[(size_t)qi * (p.dim / 16) + c * (kAsymKC / 16) + vc];
		}
	}
}
__device__ __attribute__((always_inline)) inline void asym_store(const AsymStage& s, unsigned char* rbuf, unsigned char* qbuf,
                                                                 uint32_t tid, uint32_t kw, bool with_q) {
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

__global__ __launch_bounds__(kHamThreads) void scan_asym_mfma_kernel(AsymParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char asym_smem[];
	constexpr uint32_t RS = kAsymRowStride, QS = kAsymQStride, QOFF = kHamTB * kAsymRowStride;
	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const uint32_t i = lane & 15, g = lane >> 4;
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	const uint32_t q0 = qtile * kHamTQ;
	const uint32_t NC = (p.dim + kAsymKC - 1) / kAsymKC;  // chunks of the reduction dimension
	const bool stream_q = NC > 1;                        // (one chunk: the queries are staged once, in stage 0)
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

	AsymStage st;
	uint32_t t = t0, c = 0;
	uint32_t kw = p.dim < kAsymKC ? p.dim : kAsymKC;
	asym_load(st, p, tid, t * p.tile_stride * kHamTB, q0, 0, kw, true);
	asym_store(st, asym_smem, asym_smem + QOFF, tid, kw, true);

	ham_i32x4 acc[4][kHamNT];
	for (uint32_t it = 0; it < n_items; ++it) {
		const uint32_t row0 = t * p.tile_stride * kHamTB;
		uint32_t tn = t, cn = c + 1;
		if (cn == NC) {
			cn = 0;
			tn = t + 1;
		}
		const bool more = it + 1 < n_items;
		const uint32_t kwn = (p.dim - cn * kAsymKC) < kAsymKC ? (p.dim - cn * kAsymKC) : kAsymKC;
		if (more)  // in flight while this stage is multiplied
			asym_load(st, p, tid, tn * p.tile_stride * kHamTB, q0, cn, kwn, stream_q);
		__syncthreads();  // this stage is in place; the other one has been read

		unsigned char* const sbuf = asym_smem + (it & 1) * kAsymStageBytes;
		unsigned char* const obuf = asym_smem + ((it + 1) & 1) * kAsymStageBytes;
		if (c == 0) {
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
#pragma unroll
				for (int tc = 0; tc < kHamNT; ++tc)
					acc[tq][tc] = ham_i32x4{0, 0, 0, 0};
		}
		const unsigned char* const qf = (stream_q ? sbuf : asym_smem) + QOFF + i * QS + 16 * g;
		const unsigned char* const rf = sbuf + (wave * 64 + i) * RS + 2 * g;
		const uint32_t KS = kw / 64;
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
		if (more)
			asym_store(st, obuf, obuf + QOFF, tid, kwn, stream_q);

		if (c == NC - 1) {
			// epilogue: lane (i, g) holds, for column tc, row 16 tc + i of the wave against queries 16 tq + 4 g + e
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const uint32_t local = wave * 64 + 16 * tc + i;
				const uint32_t brow = row0 + local;
				const bool bvalid = brow < p.n_rows;
#pragma unroll
				for (int tq = 0; tq < 4; ++tq) {
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						const int tv = -2 * acc[tq][tc][e];
						const uint32_t qi = q0 + 16 * tq + 4 * g + e;
						if (p.level0) {
							const uint32_t slot = t * kHamTB + local;
							if (qi < p.m && slot < p.cap)
								p.cand[(size_t)qi * p.cap + slot] =
								    bvalid ? make_key((float)(tv + p.sumq[qi]), brow) : kSentinelKey;
							continue;
						}
						bool hit = bvalid && tv <= th[tq][e];
						if (__builtin_amdgcn_ballot_w64(hit) == 0)
							continue;
						// rare path: the tie rule, then one atomic per quarter wave (its 16 lanes share the query)
						hit = hit && (tv < th[tq][e] || brow <= p.tau_row[qi]);
						const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
						const uint32_t seg = (uint32_t)(mask >> (lane & 48)) & 0xFFFFu;
						uint32_t slot0 = 0;
						if (i == 0 && seg)
							slot0 = atomicAdd(&p.cand_cnt[qi], (uint32_t)__builtin_popcount(seg));
						slot0 = __shfl(slot0, lane & 48);
						const uint32_t slot = slot0 + (uint32_t)__builtin_popcount(seg & ((1u << i) - 1u));
						if (hit && slot < p.cap)
							p.cand[(size_t)qi * p.cap + slot] = make_key((float)(tv + p.sumq[qi]), brow);
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
