// scan_tile.hpp -- the tile-scan skeleton of the packed-row scans on the int8 matrix cores: scan_hamming_mfma_kernel
// (scan_hamming.hpp), scan_asym_mfma_kernel (scan_asym.hpp) and scan_i4_mfma_kernel (scan_i4.hpp) -- the two instances
// of scan_stream_mfma_kernel below --, scan_pq4_mfma_kernel<RESIDENT> (scan_pq4.hpp).
//
// Geometry: kHamThreads = 512 threads in 8 waves; a workgroup holds kHamTQ = 64 queries as four 16-query A fragments
// and walks tiles of kHamTB = 512 rows; wave w owns rows [64 w, 64 w + 64) of the tile as kHamNT = 4 16-row columns;
// v_mfma_i32_16x16x64_i8 into acc[4][kHamNT], 64 accumulator registers, no scratch.  Lane (i, g) = (lane % 16,
// lane / 16) holds, for column tc, row 16 tc + i of the wave against queries 16 tq + 4 g + e.
//
// What every form shares is here, once: the parameter struct, the workgroup's tile range, the thresholds of a lane's
// 16 queries, and the epilogue of a finished tile -- level 0 (no thresholds) writes the key of every (query, row) of
// its tiles at the row's fixed slot, so the threshold ladder runs these kernels alone; the later levels compare
// integers against theta and, on the rare hit, apply the tie rule (score, row) <= (tau, tau_row) with one ballot and one
// atomic per quarter wave (its 16 lanes share the query).  The two forms whose rows go through LDS with the reduction
// dimension streamed share their kernel as well: scan_stream_mfma_kernel below.
//
// A new row format supplies
//   - an epilogue POLICY: row_term(p, row, valid), the per-row int term; combine(p, rt, acc), the integer t that is
//     compared against theta; query_term(p, qi), with score = t + query_term; kFloatTies, whether scores can pass
//     2^24 and round as floats, so that the tie rule must be decided on the floats (scan_i4.hpp, 2.);
//   - its prep kernel (theta = floor(tau) - query_term, and whatever it does to the A operand);
//   - and either a CODEC for scan_stream_mfma_kernel -- the chunk size, the LDS strides, the stage registers, load /
//     store of a stage, the read and widening of one B fragment -- or a tile loop of its own (resident queries:
//     scan_hamming.hpp; codes from global memory to registers: scan_pq4.hpp).
#pragma once
#include "bf_plan.hpp"
#include "common.hpp"
#include "scan_f32.hpp"

namespace expann {

typedef int ham_i32x4 __attribute__((ext_vector_type(4)));

constexpr int kHamThreads = 512;    // 8 waves
constexpr int kHamTQ = 64;          // queries per workgroup (four 16-query fragments)
constexpr int kHamNT = 4;           // 16-row columns per wave
constexpr int kHamTB = (kHamThreads / 64) * 16 * kHamNT;  // rows per tile

struct TileScanParams {
	const void* base;         // [n_rows] packed rows of the form
	const int* rowterm;       // [n_rows] the per-row int term (Hamming: pop(b); 4-bit rows under L2: sum b^2), or nullptr
	uint32_t n_rows;
	uint32_t n_tiles_sel;     // kHamTB-row tiles this launch visits: tile j of the launch is base tile j * tile_stride
	uint32_t tile_stride;
	uint32_t tiles_per_block;
	uint32_t n_qtiles;
	const void* a_operand;    // per query, klen-dependent: the queries, their permuted copy, or the byte tables
	const int* theta;         // [m] floor(tau) - the query term (+ a form's float slack); unused at level 0
	const int* qterm;         // [m] the per-query int term, or nullptr where it is the constant below
	int qterm_const;          // 4-bit PQ: 128 M
	const float* tau;         // [m] the threshold itself (float ties); unused at level 0
	const uint32_t* tau_row;  // [m] row of the threshold key
	uint32_t m;
	uint32_t* cand_cnt;
	uint64_t* cand;
	uint32_t cap;
	uint32_t klen;            // the reduction length: dim, or M for 4-bit PQ
	uint32_t level0;          // 1: no thresholds, the key of (query, row) goes to slot j * kHamTB + row in tile
};
static_assert(kPlanAsymTile == kHamTB, "plan_asym_tiles (bf_plan.hpp) plans the tiles and fixed slots of this geometry");

// A thread's place in the geometry and its workgroup's range: queries [q0, q0 + kHamTQ), tiles [t0, t1).
struct TileLane {
	uint32_t tid, lane, wave, i, g, q0, t0, t1;
};
// false: the workgroup has no tile (the caller returns)
__device__ __attribute__((always_inline)) inline bool tile_range(const TileScanParams& p, TileLane& w) {
	w.tid = threadIdx.x;
	w.lane = w.tid & 63;
	w.wave = __builtin_amdgcn_readfirstlane(w.tid >> 6);
	w.i = w.lane & 15;
	w.g = w.lane >> 4;
	const uint32_t qtile = blockIdx.x % p.n_qtiles;
	const uint32_t chunk = blockIdx.x / p.n_qtiles;
	w.q0 = qtile * kHamTQ;
	w.t0 = chunk * p.tiles_per_block;
	w.t1 = w.t0 + p.tiles_per_block;
	if (w.t1 > p.n_tiles_sel)
		w.t1 = p.n_tiles_sel;
	return w.t0 < w.t1;
}

// thresholds of the lane's 16 queries: fragment tq, register e = query 16 tq + 4 g + e (a padded slot never matches)
__device__ __attribute__((always_inline)) inline void tile_thresholds(const TileScanParams& p, const TileLane& w, int (&th)[4][4]) {
	constexpr int kNever = -2147483647 - 1;
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const uint32_t qi = w.q0 + 16 * tq + 4 * w.g + e;
			th[tq][e] = (qi < p.m && !p.level0) ? p.theta[qi] : kNever;
		}
}

__device__ __attribute__((always_inline)) inline void tile_clear(ham_i32x4 (&acc)[4][kHamNT]) {
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int tc = 0; tc < kHamNT; ++tc)
			acc[tq][tc] = ham_i32x4{0, 0, 0, 0};
}

// The epilogue of tile t of the launch.  (Level 0 has a loop of its own: the compiler no longer unswitches the one
// loop on p.level0 once it is shared, and the test inside the 64 unrolled bodies costs ~1.6 us a tile.)
template <class Policy>
__device__ __attribute__((always_inline)) inline void tile_epilogue(const TileScanParams& p, const TileLane& w, uint32_t t,
                                                                    const ham_i32x4 (&acc)[4][kHamNT], const int (&th)[4][4]) {
	const uint32_t row0 = t * p.tile_stride * kHamTB;
	if (p.level0) {  // no thresholds: the key of every (query, row) at the row's fixed slot
#pragma unroll
		for (int tc = 0; tc < kHamNT; ++tc) {
			const uint32_t local = w.wave * 64 + 16 * tc + w.i;
			const uint32_t brow = row0 + local, slot = t * kHamTB + local;
			const bool bvalid = brow < p.n_rows;
			const int rt = Policy::row_term(p, brow, bvalid);
#pragma unroll
			for (int tq = 0; tq < 4; ++tq) {
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const int tv = Policy::combine(p, rt, acc[tq][tc][e]);
					const uint32_t qi = w.q0 + 16 * tq + 4 * w.g + e;
					if (qi < p.m && slot < p.cap)
						p.cand[(size_t)qi * p.cap + slot] =
						    bvalid ? make_key((float)(tv + Policy::query_term(p, qi)), brow) : kSentinelKey;
				}
			}
		}
		return;
	}
#pragma unroll
	for (int tc = 0; tc < kHamNT; ++tc) {
		const uint32_t brow = row0 + w.wave * 64 + 16 * tc + w.i;
		const bool bvalid = brow < p.n_rows;
		const int rt = Policy::row_term(p, brow, bvalid);
#pragma unroll
		for (int tq = 0; tq < 4; ++tq) {
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				const int tv = Policy::combine(p, rt, acc[tq][tc][e]);
				const uint32_t qi = w.q0 + 16 * tq + 4 * w.g + e;
				bool hit = bvalid && tv <= th[tq][e];
				if (__builtin_amdgcn_ballot_w64(hit) == 0)
					continue;
				// rare path: the tie rule -- on the integers, or on the floats where the scores round --, then one atomic
				// per quarter wave (its 16 lanes share the query)
				if (!Policy::kFloatTies) {
					hit = hit && (tv < th[tq][e] || brow <= p.tau_row[qi]);
				} else if (hit) {
					const float sf = (float)(tv + Policy::query_term(p, qi));
					const float tau = p.tau[qi];
					hit = sf < tau || (sf == tau && brow <= p.tau_row[qi]);
				}
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
				const uint32_t seg = (uint32_t)(mask >> (w.lane & 48)) & 0xFFFFu;
				uint32_t slot0 = 0;
				if (w.i == 0 && seg)
					slot0 = atomicAdd(&p.cand_cnt[qi], (uint32_t)__builtin_popcount(seg));
				slot0 = __shfl(slot0, w.lane & 48);
				const uint32_t slot = slot0 + (uint32_t)__builtin_popcount(seg & ((1u << w.i) - 1u));
				if (hit && slot < p.cap)
					p.cand[(size_t)qi * p.cap + slot] = make_key((float)(tv + Policy::query_term(p, qi)), brow);
			}
		}
	}
}

// Rows through LDS, the reduction dimension STREAMED: it is cut into chunks of Codec::kKC elements, the accumulators
// live across the chunks of a tile, and an item of the loop is one (tile, chunk).  A stage holds the packed row chunk
// [kHamTB][kRowStride] and the query chunk [kHamTQ][kQStride]; there are two stages, one workgroup (two waves per
// SIMD) per CU.
// Overlap: the global loads of item i + 1 are issued into registers (Codec::Stage) BEFORE the k-steps of item i and
// stored to the other stage's LDS after them, so they are in flight while the waves multiply.  One barrier per item:
// it publishes stage i and, since every wave's store of item i + 1 follows its own k-steps of item i, it also says
// that the buffer about to be overwritten has been read.
// klen <= kKC: one chunk per tile, and the query chunk is staged ONCE per workgroup (into stage 0's query area; stage
// 1's stays unused).  A chunk shorter than kKC -- a small klen, or the last chunk of a klen that is no multiple of
// kKC -- is simply shorter: fewer loads kept and fewer k-steps at the same LDS strides (chosen over packing several
// tiles into a stage: the tile loop, the slots of level 0 and the epilogue stay those of one tile).
// Above kKC the query chunks are re-read (from L2) for every tile.
template <class Codec> __global__ __launch_bounds__(kHamThreads) void scan_stream_mfma_kernel(TileScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char stream_smem[];
	constexpr uint32_t KC = Codec::kKC, RS = Codec::kRowStride, QS = Codec::kQStride, QOFF = kHamTB * Codec::kRowStride;
	TileLane w;
	if (!tile_range(p, w))
		return;
	const uint32_t NC = (p.klen + KC - 1) / KC;  // chunks of the reduction dimension
	const bool stream_q = NC > 1;                // (one chunk: the queries are staged once, in stage 0)
	const uint32_t n_items = (w.t1 - w.t0) * NC;
	int th[4][4];
	tile_thresholds(p, w, th);

	typename Codec::Stage st;
	uint32_t t = w.t0, c = 0;
	uint32_t kw = p.klen < KC ? p.klen : KC;
	Codec::load(st, p, w.tid, t * p.tile_stride * kHamTB, w.q0, 0, kw, true);
	Codec::store(st, stream_smem, stream_smem + QOFF, w.tid, kw, true);

	ham_i32x4 acc[4][kHamNT];
	for (uint32_t it = 0; it < n_items; ++it) {
		uint32_t tn = t, cn = c + 1;
		if (cn == NC) {
			cn = 0;
			tn = t + 1;
		}
		const bool more = it + 1 < n_items;
		const uint32_t kwn = (p.klen - cn * KC) < KC ? (p.klen - cn * KC) : KC;
		if (more)  // in flight while this stage is multiplied
			Codec::load(st, p, w.tid, tn * p.tile_stride * kHamTB, w.q0, cn, kwn, stream_q);
		__syncthreads();  // this stage is in place; the other one has been read

		unsigned char* const sbuf = stream_smem + (it & 1) * Codec::kStageBytes;
		unsigned char* const obuf = stream_smem + ((it + 1) & 1) * Codec::kStageBytes;
		if (c == 0)
			tile_clear(acc);
		const unsigned char* const qf = (stream_q ? sbuf : stream_smem) + QOFF + w.i * QS + 16 * w.g;
		const unsigned char* const rf = sbuf + (w.wave * 64 + w.i) * RS + Codec::kLaneBytes * w.g;
		const uint32_t KS = kw / 64;
		for (uint32_t s = 0; s < KS; ++s) {
			ham_i32x4 a[4];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const ham_i32x4*>(qf + 16 * tq * QS + 64 * s);
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const ham_i32x4 f = Codec::b_fragment(rf + 16 * tc * RS + 4 * Codec::kLaneBytes * s);
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq], f, acc[tq][tc], 0, 0, 0);
			}
		}
		if (more)
			Codec::store(st, obuf, obuf + QOFF, w.tid, kwn, stream_q);
		if (c == NC - 1) {
			tile_epilogue<typename Codec::Policy>(p, w, t, acc, th);
			// Nothing of the epilogue is in flight past this point (the next stage's loads were stored above).  Said to the
			// compiler: where a B fragment register of the k-steps is also a load destination of the epilogue's rare path,
			// it otherwise puts s_waitcnt vmcnt(0) INTO the k-step loop, behind the next stage's loads -- no overlap left.
			__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
		}
		t = tn;
		c = cn;
		kw = kwn;
	}
}

}  // namespace expann
