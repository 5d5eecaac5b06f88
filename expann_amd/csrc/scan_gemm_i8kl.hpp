// scan_gemm_i8kl.hpp -- the exact 8-bit filter of scan_gemm_i8q.hpp (g domain, same parameters, per-wave hit
// logs and SAMPLE instance as scan_gemm_i8w.hpp) with the dim known at RUN time: every 8-bit dim from 64 to 4096
// (multiples of 64) that has no compiled int8 form of its own.  The compiled forms keep a workgroup's query
// fragments in registers for the whole launch and fix D at compile time; a 4096-byte query does not fit there.
// Here a K loop streams BOTH operands through LDS, one v_mfma_i32_16x16x64_i8 k-step (64 bytes) at a time:
// scan_gemm_f16kl.hpp's pipeline -- a k-step of an fp16 row there and of an 8-bit row here are the same 64 bytes,
// so geometry, staging, swizzle and waits are that kernel's.
//
// Geometry: 4 waves, 256 queries (wave w: queries 64 w .. 64 w + 63 of the workgroup, as the hit-log gather
// expects) x 128-row tiles.  A wave's step is 4 query tiles x 8 row-tile columns of 16 x 16 = 32 MFMAs on 128
// accumulator registers that stay on the output tile for all d / 64 k-steps of a row tile; lane l holds query
// l & 15 of tile tq / row l & 15 of column tc, 16-byte chunk l >> 4 of the k-step.
//
// One stage = one k-step of one row tile: 128 rows x 64 B + 256 queries x 64 B + the tile's 128 bp (512 B),
// brought by LDS-DMA (global_load_lds): 6 pieces of 16 B per thread + one of 4 B.  Three stage buffers, two
// stages in flight ahead of the one multiplied, one workgroup barrier per k-step.  In a 64-B LDS row, logical
// chunk c of row r sits at physical chunk c ^ ((-(r >> 2)) & 3) (f16kl_swz): the 16 lanes of every ds_read_b128
// lane group hit 16 different bank quads.
//
// Rows are whole k-steps at every d % 64 == 0, so the engine's int8 copy (uint8 rows ^ 0x80, ensure_i8q) keeps
// d bytes per row; it is padded to whole 128-row tiles (zero rows, bp = kI8qPadBp).  Byte offsets of rows and
// queries are 64-bit.  The integer product is exact: no slack term, candidates leave with exact scores.
//
// Accumulator range at d = 4096 (operands are int8 on both sides, |x| <= 128):
//   |q.b| <= 128^2 x 4096 = 2^26;  bp = floor(sum b^2 / 2) <= 2^25;  |g| = |q.b - bp| <= 2^26 + 2^25
//   full scan: acc = q.b + thp, thp = -g_k or 2^30 ("keep every row") -> |acc| <= 2^30 + 2^26 < 2^31;
//              a padded query slot starts at INT_MIN / 2 = -2^30 -> acc <= 2^26 - 2^30 < 0 <= bp: never a hit
//   SAMPLE:    acc = q.b - bp, bp = 2^30 on the padding rows -> acc >= -2^30 - 2^26 > INT_MIN
//   scores:    sum (a - b)^2 <= 255^2 x 4096 < 2^28 (the gather's bias - 2 dot + qself, each term < 2^28)
// so nothing wraps in any mode (the worst case the uint8 metric can reach, 255^2 x 4096 ~ 2.7 x 10^8, included).
#pragma once
#include "scan_gemm_f16kl.hpp"
#include "scan_gemm_i8w.hpp"

namespace expann {

constexpr int kI8klTB = kF16klTB;   // rows per tile
constexpr int kI8klBufs = 3;        // stage buffers
constexpr int kI8klQcap = kF16WaveQueue;
constexpr int kI8klStageBytes = kI8klTB * 64 + kF16TQ * 64 + kI8klTB * 4;
constexpr int kI8klLds = kI8klBufs * kI8klStageBytes + kF16Waves * kI8klQcap * kF16EntryBytes;
static_assert(kI8klLds <= 160 * 1024, "LDS budget per CU");

template <bool SAMPLE>
__global__ __launch_bounds__(kF16Threads, 1) void scan_gemm_i8kl_kernel(GemmI8wParams pw) {
	const GemmI8qParams& p = pw.q;
	constexpr int WAVES = kF16Waves, WGQ = kF16TQ, TB = kI8klTB, QCAP = kI8klQcap;
	constexpr int NBUF = kI8klBufs, SB = kI8klStageBytes;
	constexpr int QOFF = TB * 64, BPOFF = QOFF + WGQ * 64;
	constexpr int kNever = -2147483647 - 1;
	static_assert(kF16Threads == 256 && WAVES == 4, "4 waves x 64 queries per workgroup (gather_logs_kernel)");
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int l15 = lane & 15, lq = lane >> 4;
	const uint32_t KS = p.ksteps;
	const size_t ROWB = (size_t)KS * 64;  // bytes per row
	const uint32_t bid = blockIdx.x;
	uint32_t qtile = bid % p.n_qtiles;
	uint32_t chunk = bid / p.n_qtiles;
	if (p.xcd_map) {  // (as scan_gemm_i8w_kernel: the row chunks {x, x + 8, ..} of a query tile on XCD x)
		const uint32_t j = bid >> 3;
		qtile = j % p.n_qtiles;
		chunk = (bid & 7) + 8 * (j / p.n_qtiles);
	}
	const uint32_t wg_q0 = qtile * WGQ;
	const uint32_t q0 = wg_q0 + wave * 64;

	const uint32_t t0 = chunk * p.tiles_per_block;
	uint32_t t1 = t0 + p.tiles_per_block;
	if (t1 > p.n_tiles_sel)
		t1 = p.n_tiles_sel;
	if (t0 >= t1) {
		if (SAMPLE) {
			for (uint32_t i = lane; i < 64 * 32; i += 64)
				if (q0 + (i >> 5) < p.m)
					p.sample_out[((size_t)(q0 + (i >> 5)) * p.n_chunks + chunk) * 32 + (i & 31)] = kNever;
		} else if (lane == 0) {
			pw.log_cnt[(size_t)bid * WAVES + wave] = 0;
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
		qsrc[i] = (const unsigned char*)p.queries + (size_t)qi * ROWB + co;
	}
	const unsigned char* const rbase = (const unsigned char*)p.base + co;
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
		// the tile's 128 bp: waves 0 / 2 rows 0-63, waves 1 / 3 rows 64-127 (the same bytes twice: every
		// wave issues 7 loads per stage, so one vmcnt serves all)
		__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.bp + row0 + (wave & 1) * 64 + lane),
		                                 (__attribute__((address_space(3))) void*)(smem + st_buf * SB + BPOFF + (wave & 1) * 256),
		                                 4, 0, 0);
		st_buf = st_buf + 1 == NBUF ? 0 : st_buf + 1;
		if (++st_ks == KS) {
			st_ks = 0;
			++st_t;
		}
	};

	// ---- candidates: per-wave LDS queue -> per-wave hit log (scan_gemm_i8w_kernel's entries, 8 columns) ----
	struct QEntry {
		int acc[16];     // value i = query tile i >> 2, register i & 3
		int bp;
		uint32_t row;
		uint32_t qrow0;  // query of value 0; value i is + 16 (i >> 2) + (i & 3)
		uint32_t pad;
	};
	static_assert(sizeof(QEntry) == kF16EntryBytes, "queue entry size");
	QEntry* const queue = reinterpret_cast<QEntry*>(smem + NBUF * SB) + wave * QCAP;
	uint32_t wfill = 0, glog_n = 0;  // wave-uniform
	uint4* const my_log = SAMPLE ? nullptr : pw.log + ((size_t)bid * WAVES + wave) * pw.log_cap;
	// a log entry is {raw accumulator, row, query}: gather_logs_kernel makes the exact score (GatherLogParams::i_mode)
	auto flush_own = [&]() {
		const uint32_t n = wfill < (uint32_t)QCAP ? wfill : (uint32_t)QCAP;
		for (uint32_t b0 = 0; b0 < n * 16; b0 += 64) {
			const uint32_t i = b0 + lane;
			const QEntry& e = queue[i < n * 16 ? i >> 4 : 0];
			const uint32_t v = i & 15;
			const int c = e.acc[v];
			const uint32_t row = e.row;
			const bool hit = i < n * 16 && c >= e.bp && row < p.n_rows;
			const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
			if (mask == 0)
				continue;
			const uint32_t pos = glog_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			if (hit && pos < pw.log_cap)
				my_log[pos] = make_uint4((uint32_t)c, row, e.qrow0 + 16 * (v >> 2) + (v & 3), 0u);
			glog_n += (uint32_t)__builtin_popcountll(mask);
		}
		wfill = 0;
	};

	i32x4 th[4];  // accumulator start values -g_k of each accumulator register's query
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t qi = q0 + tq * 16 + 4 * lq + r;
			th[tq][r] = (qi < p.m && !SAMPLE) ? p.thp[qi] : kNever / 2;
		}
	i32x4 smax[2][4];  // SAMPLE: running maxima of g per (class parity, query tile)
#pragma unroll
	for (int par = 0; par < 2; ++par)
#pragma unroll
		for (int tq = 0; tq < 4; ++tq)
			smax[par][tq] = i32x4{kNever, kNever, kNever, kNever};

	const uint32_t fo = (uint32_t)l15 * 64u + (((uint32_t)lq ^ f16kl_swz((uint32_t)l15)) * 16u);
	stage_next();
	stage_next();
	i32x4 acc[4][8];
	int buf = 0;
	for (uint32_t t = t0; t < t1; ++t) {
		const uint32_t row0 = tile_row0(t);
		for (uint32_t ks = 0; ks < KS; ++ks) {
			// stage (t, ks) landed (only the next one's 7 loads may be in flight), every wave is done with the
			// buffer the stage after next goes to
			asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory");
			stage_next();
			const unsigned char* sb = smem + buf * SB;
			int bpv[8];
			if (ks == 0 || ks == KS - 1) {
				const int* bs = reinterpret_cast<const int*>(sb + BPOFF);
#pragma unroll
				for (int tc = 0; tc < 8; ++tc)
					bpv[tc] = bs[tc * 16 + l15];
			}
			if (ks == 0) {
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
#pragma unroll
					for (int tc = 0; tc < 8; ++tc) {
						if (SAMPLE) {  // the row term enters as the C operand: acc ends at g = q.b - bp
							const int nb = -bpv[tc];
							acc[tq][tc] = i32x4{nb, nb, nb, nb};
						} else {
							acc[tq][tc] = th[tq];
						}
					}
			}
			i32x4 a[4], b[8];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const i32x4*>(sb + QOFF + (wave * 64 + tq * 16) * 64 + fo);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
				b[tc] = *reinterpret_cast<const i32x4*>(sb + tc * 16 * 64 + fo);
			__builtin_amdgcn_s_setprio(1);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq], b[tc], acc[tq][tc], 0, 0, 0);
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
							smax[par][tq][r] = max(max3i(smax[par][tq][r], acc[tq][par][r], acc[tq][par + 2][r]),
							                       max(acc[tq][par + 4][r], acc[tq][par + 6][r]));
				continue;
			}
#pragma unroll
			for (int tc = 0; tc < 8; ++tc) {
				int g = kNever;
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					g = max3i(g, max3i(acc[tq][tc][0], acc[tq][tc][1], acc[tq][tc][2]), acc[tq][tc][3]);
				const bool h = g >= bpv[tc];
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
					e.bp = bpv[tc];
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
			pw.log_cnt[(size_t)bid * WAVES + wave] = glog_n;
			if (glog_n > pw.log_cap)  // (the log is as large as this wave's share of the candidate lists)
				atomicAdd(pw.lost, 1u);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the re-staged tail: LDS must outlive the loads)
}

}  // namespace expann
