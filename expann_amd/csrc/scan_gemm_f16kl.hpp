// scan_gemm_f16kl.hpp -- the fp16 candidate filter of scan_gemm_f16.hpp (same slack analysis, parameters, hit
// logs and sampled pass) with the dim known at RUN time: every f32 dim from 64 to 4096 (multiples of 16)
// that has no compiled fp16 form of its own.  The forms of the compiled dims keep a workgroup's query tile
// in registers for the whole launch and fix D at compile time; a 4096-wide query tile does not fit there.
// Here a K loop streams BOTH operands through LDS, one MFMA k-step (32 elements) at a time.
//
// Geometry: 4 waves, 256 queries (wave w: queries 64 w .. 64 w + 63 of the workgroup, as the hit-log gather
// expects) x 128-row tiles.  A wave's step is 4 query tiles x 8 row-tile columns of 16 x 16 =
// 32 v_mfma_f32_16x16x32_f16 on 128 accumulator registers that stay on the output tile for all ld / 32
// k-steps of a row tile; lane l holds query l & 15 of tile tq / row l & 15 of column tc, 16-byte chunk
// l >> 4 of the k-step (the f16x fragment layout with one k-step per stage).
//
// One stage = one k-step of one row tile: 128 rows x 64 B + 256 queries x 64 B + the tile's 128 bn' (512 B),
// brought by LDS-DMA (global_load_lds): 6 pieces of 16 B per thread + one of 4 B.  Three stage buffers, two
// stages in flight ahead of the one multiplied, one workgroup barrier per k-step.  In a 64-B LDS row,
// logical chunk c of row r sits at physical chunk c ^ ((-(r >> 2)) & 3): the 16 lanes of every ds_read_b128
// lane group then hit 16 different bank quads.
//
// The fp16 copies (rows: ensure_f16, queries: f16_query_prep_any_kernel) have rows of ld = d rounded up to
// a multiple of 32 elements, zero past d, and the index is padded to whole 128-row tiles (bn' NaN).  The
// zero lanes add exact zeros to the accumulators -- no rounding, no error term -- and the norms are taken
// over the d real elements, so gemm_f16_filter_eps(d) of the real d holds as it stands.
// Byte offsets of rows and queries are 64-bit: n * ld * 2 passes 2^32 at ~0.5 M rows of d = 4096.
#pragma once
#include "scan_gemm_f16x.hpp"

namespace expann {

constexpr int kF16klTB = 128;       // rows per tile
constexpr int kF16klBufs = 3;       // stage buffers
constexpr int kF16klQcap = kF16WaveQueue;
constexpr int kF16klStageBytes = kF16klTB * 64 + kF16TQ * 64 + kF16klTB * 4;
constexpr int kF16klLds = kF16klBufs * kF16klStageBytes + kF16Waves * kF16klQcap * kF16EntryBytes;
static_assert(kF16klLds <= 160 * 1024, "LDS budget per CU");

__device__ inline uint32_t f16kl_swz(uint32_t r) { return (0u - (r >> 2)) & 3u; }

template <bool SAMPLE>
__global__ __launch_bounds__(kF16Threads, 1) void scan_gemm_f16kl_kernel(GemmF16Params p) {
	constexpr int WAVES = kF16Waves, WGQ = kF16TQ, TB = kF16klTB, QCAP = kF16klQcap;
	constexpr int NBUF = kF16klBufs, SB = kF16klStageBytes;
	constexpr int QOFF = TB * 64, BNOFF = QOFF + WGQ * 64;
	static_assert(kF16Threads == 256 && WAVES == 4, "4 waves x 64 queries per workgroup (gather_logs_kernel)");
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int l15 = lane & 15, lq = lane >> 4;
	const uint32_t KS = p.ksteps;
	const size_t ROWB = (size_t)KS * 64;  // bytes per fp16 row (ld elements)
	const uint32_t bid = blockIdx.x;
	uint32_t qtile = bid % p.n_qtiles;
	uint32_t chunk = bid / p.n_qtiles;
	if (p.xcd_map) {  // (as scan_gemm_f16x_kernel: the row chunks {x, x + 8, ..} of a query tile on XCD x)
		const uint32_t j = bid >> 3;
		qtile = j % p.n_qtiles;
		chunk = (bid & 7) + 8 * (j / p.n_qtiles);
	}
	const uint32_t wg_q0 = qtile * WGQ;
	const uint32_t q0 = wg_q0 + wave * 64;

	uint32_t t0 = chunk * p.tiles_per_block;
	uint32_t t1 = t0 + p.tiles_per_block;
	if (p.tiles_small && chunk >= p.n_big) {  // (GemmF16Params::n_big)
		t0 = p.n_big * p.tiles_per_block + (chunk - p.n_big) * p.tiles_small;
		t1 = t0 + p.tiles_small;
	}
	if (t1 > p.n_tiles_sel)
		t1 = p.n_tiles_sel;
	if (t0 >= t1) {
		if (SAMPLE) {
			for (uint32_t i = lane; i < 64 * 32; i += 64)
				if (q0 + (i >> 5) < p.m)
					p.sample_out[((size_t)(q0 + (i >> 5)) * p.n_chunks + chunk) * 32 + (i & 31)] = -__builtin_inff();
		} else if (lane == 0) {
			p.log_cnt[(size_t)bid * WAVES + wave] = 0;
		}
		return;
	}

	auto tile_row0 = [&](uint32_t t) -> uint32_t {
		return ((t / p.tile_run) * (p.tile_stride * p.tile_run) + (t % p.tile_run)) * TB;
	};

	// ---- staging: slot S = i * 256 + tid of a stage (16 B each); slots 0..511 rows, 512..1535 queries ----
	const uint32_t co = (((uint32_t)tid & 3u) ^ f16kl_swz((uint32_t)tid >> 2)) * 16u;  // (the same for every piece)
	const unsigned char* qsrc[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const uint32_t qr = (uint32_t)(i * 256 + tid) >> 2;
		const uint32_t qi = wg_q0 + qr < p.m ? wg_q0 + qr : p.m - 1;
		qsrc[i] = (const unsigned char*)p.queries_f16 + (size_t)qi * ROWB + co;
	}
	const unsigned char* const rbase = (const unsigned char*)p.base_f16 + co;
	const uint32_t rr = (uint32_t)tid >> 2;
	uint32_t st_t = t0, st_ks = 0;  // the next stage to issue (clamped to the last one: re-staged, never read)
	int st_buf = 0;
	auto stage_next = [&]() {
		const uint32_t t = st_t < t1 ? st_t : t1 - 1;
		const uint32_t ks = st_t < t1 ? st_ks : KS - 1;
		const uint32_t row0 = tile_row0(t);
		unsigned char* dst = smem + st_buf * SB + wave * 64 * 16;
#pragma unroll
		for (int i = 0; i < 2; ++i)
			__builtin_amdgcn_global_load_lds(
			    (const __attribute__((address_space(1))) void*)(rbase + (size_t)(row0 + i * 64 + rr) * ROWB + ks * 64u),
			    (__attribute__((address_space(3))) void*)(dst + i * 256 * 16), 16, 0, 0);
#pragma unroll
		for (int i = 0; i < 4; ++i)
			__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qsrc[i] + ks * 64u),
			                                 (__attribute__((address_space(3))) void*)(dst + (i + 2) * 256 * 16), 16, 0, 0);
		// the tile's 128 bn': waves 0 / 2 rows 0-63, waves 1 / 3 rows 64-127 (the same bytes twice: every
		// wave issues 7 loads per stage, so one vmcnt serves all)
		__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.bnorm + row0 + (wave & 1) * 64 + lane),
		                                 (__attribute__((address_space(3))) void*)(smem + st_buf * SB + BNOFF + (wave & 1) * 256),
		                                 4, 0, 0);
		st_buf = st_buf + 1 == NBUF ? 0 : st_buf + 1;
		if (++st_ks == KS) {
			st_ks = 0;
			++st_t;
		}
	};

	// ---- candidates: per-wave LDS queue -> per-wave hit log (scan_gemm_f16x_kernel's, 8 columns) ----
	struct QEntry {
		float acc[16];   // value i = query tile i >> 2, register i & 3
		float bn;
		uint32_t row;
		uint32_t qrow0;  // query of value 0; value i is + 16 (i >> 2) + (i & 3)
		uint32_t pad;
	};
	static_assert(sizeof(QEntry) == kF16EntryBytes, "queue entry size");
	QEntry* const queue = reinterpret_cast<QEntry*>(smem + NBUF * SB) + wave * QCAP;
	uint32_t wfill = 0, glog_n = 0;  // wave-uniform
	uint4* const my_log = SAMPLE ? nullptr : p.log + ((size_t)bid * WAVES + wave) * p.log_cap;
	auto flush_own = [&]() {
		const uint32_t n = wfill < (uint32_t)QCAP ? wfill : (uint32_t)QCAP;
		for (uint32_t b0 = 0; b0 < n * 16; b0 += 64) {
			const uint32_t i = b0 + lane;
			const QEntry& e = queue[i < n * 16 ? i >> 4 : 0];
			const uint32_t v = i & 15;
			const float c = e.acc[v], bn = e.bn;
			const bool hit = i < n * 16 && c >= bn;
			const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
			if (mask == 0)
				continue;
			const uint32_t pos = glog_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			if (hit && pos < p.log_cap)
				my_log[pos] = make_uint4(__builtin_bit_cast(uint32_t, bn - c), e.row, e.qrow0 + 16 * (v >> 2) + (v & 3), 0u);
			glog_n += (uint32_t)__builtin_popcountll(mask);
		}
		wfill = 0;
	};

	f32x4 th[4];  // accumulator start values: theta' of each accumulator register's query
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t qi = q0 + tq * 16 + 4 * lq + r;
			th[tq][r] = (qi < p.m && !SAMPLE) ? p.theta[qi] : -__builtin_inff();
		}
	f32x4 smax[2][4];  // SAMPLE: running maxima of g per (class parity, query tile)
#pragma unroll
	for (int par = 0; par < 2; ++par)
#pragma unroll
		for (int tq = 0; tq < 4; ++tq)
			smax[par][tq] = f32x4{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};

	const uint32_t fo = (uint32_t)l15 * 64u + (((uint32_t)lq ^ f16kl_swz((uint32_t)l15)) * 16u);
	stage_next();
	stage_next();
	f32x4 acc[4][8];
	int buf = 0;
	for (uint32_t t = t0; t < t1; ++t) {
		const uint32_t row0 = tile_row0(t);
		for (uint32_t ks = 0; ks < KS; ++ks) {
			// stage (t, ks) landed (only the next one's 7 loads may be in flight), every wave is done with the
			// buffer the stage after next goes to
			asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory");
			stage_next();
			const unsigned char* sb = smem + buf * SB;
			float bnv[8];
			if (ks == 0 || ks == KS - 1) {
				const float* bs = reinterpret_cast<const float*>(sb + BNOFF);
#pragma unroll
				for (int tc = 0; tc < 8; ++tc)
					bnv[tc] = bs[tc * 16 + l15];
			}
			if (ks == 0) {
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
#pragma unroll
					for (int tc = 0; tc < 8; ++tc) {
						if (SAMPLE) {  // the row term enters as the C operand: acc ends at g = q16.b16 - bn'
							const float nb = -bnv[tc];
							acc[tq][tc] = f32x4{nb, nb, nb, nb};
						} else {
							acc[tq][tc] = th[tq];
						}
					}
			}
			f16x8 a[4], b[8];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const f16x8*>(sb + QOFF + (wave * 64 + tq * 16) * 64 + fo);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
				b[tc] = *reinterpret_cast<const f16x8*>(sb + tc * 16 * 64 + fo);
			__builtin_amdgcn_s_setprio(1);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tq], b[tc], acc[tq][tc], 0, 0, 0);
			__builtin_amdgcn_s_setprio(0);
			buf = buf + 1 == NBUF ? 0 : buf + 1;
			if (ks + 1 < KS)
				continue;
			// ---- the row tile is complete ----
			if (SAMPLE) {
#pragma unroll
				for (int par = 0; par < 2; ++par)
#pragma unroll
					for (int tq = 0; tq < 4; ++tq)
#pragma unroll
						for (int r = 0; r < 4; ++r)
							smax[par][tq][r] = __builtin_fmaxf(
							    max3f(smax[par][tq][r], acc[tq][par][r], acc[tq][par + 2][r]),
							    max3f(acc[tq][par + 4][r], acc[tq][par + 6][r], -__builtin_inff()));
				continue;
			}
#pragma unroll
			for (int tc = 0; tc < 8; ++tc) {
				float g = -__builtin_inff();
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					g = max3f(g, max3f(acc[tq][tc][0], acc[tq][tc][1], acc[tq][tc][2]), acc[tq][tc][3]);
				const bool h = g >= bnv[tc];
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(h);
				if (mask == 0)
					continue;
				// a column adds at most 64 entries and the queue holds more: make room first, drop nothing
				static_assert(QCAP >= 64, "a tile column's hits fit an empty queue");
				if (wfill + (uint32_t)__builtin_popcountll(mask) > (uint32_t)QCAP)
					flush_own();
				const uint32_t slot = wfill + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
				                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
				if (h) {
					QEntry& e = queue[slot];
#pragma unroll
					for (int tq = 0; tq < 4; ++tq)
#pragma unroll
						for (int r = 0; r < 4; ++r)
							e.acc[tq * 4 + r] = acc[tq][tc][r];
					e.bn = bnv[tc];
					e.row = row0 + tc * 16 + l15;
					e.qrow0 = q0 + 4 * lq;
				}
				wfill += (uint32_t)__builtin_popcountll(mask);
			}
			if (wfill >= (uint32_t)QCAP * 3 / 4)
				flush_own();
		}
	}
	if (SAMPLE) {
#pragma unroll
		for (int par = 0; par < 2; ++par)
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const uint32_t qi = q0 + tq * 16 + 4 * lq + r;
					if (qi < p.m)
						p.sample_out[((size_t)qi * p.n_chunks + chunk) * 32 + par * 16 + l15] = smax[par][tq][r];
				}
	} else {
		flush_own();
		if (lane == 0) {
			p.log_cnt[(size_t)bid * WAVES + wave] = glog_n;
			if (glog_n > p.log_cap)
				atomicAdd(p.lost, 1u);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the re-staged tail: LDS must outlive the loads)
}

}  // namespace expann
