// scan_gemm_kl.hpp -- the candidate filters with the dim known at RUN time, one kernel for both operand types
// (scan_gemm_elem.hpp): E = F16Elem is the fp16 filter of scan_gemm_f16.hpp (same slack analysis, parameters, hit
// logs and sampled pass) for every f32 dim from 64 to 4096 (multiples of 16) that has no compiled fp16 form of its
// own; E = I8Elem is the exact 8-bit filter of scan_gemm_i8q.hpp (g domain, same parameters and hit logs) for
// every 8-bit dim from 64 to 4096 (multiples of 64) without a compiled int8 form.  The forms of the compiled dims
// keep a workgroup's query tile in registers for the whole launch and fix D at compile time; a 4096-wide query
// tile does not fit there.  Here a K loop streams BOTH operands through LDS, one MFMA k-step (64 bytes of a row:
// 32 fp16 or 64 int8 values) at a time.
//
// Geometry: 4 waves, 256 queries (wave w: queries 64 w .. 64 w + 63 of the workgroup, as the hit-log gather
// expects) x 128-row tiles.  A wave's step is 4 query tiles x 8 row-tile columns of 16 x 16 = 32 MFMAs on 128
// accumulator registers that stay on the output tile for all k-steps of a row tile; lane l holds query l & 15 of
// tile tq / row l & 15 of column tc, 16-byte chunk l >> 4 of the k-step.
//
// One stage = one k-step of one row tile: 128 rows x 64 B + 256 queries x 64 B + the tile's 128 row terms
// (512 B), brought by LDS-DMA (global_load_lds): 6 pieces of 16 B per thread + one of 4 B.  Three stage buffers,
// two stages in flight ahead of the one multiplied, one workgroup barrier per k-step.  In a 64-B LDS row, logical
// chunk c of row r sits at physical chunk c ^ ((-(r >> 2)) & 3): the 16 lanes of every ds_read_b128 lane group
// then hit 16 different bank quads.
//
// fp16: the copies (rows: ensure_f16, queries: f16_query_prep_any_kernel) have rows of ld = d rounded up to a
// multiple of 32 elements, zero past d, and the index is padded to whole 128-row tiles (bn' NaN).  The zero lanes
// add exact zeros to the accumulators -- no rounding, no error term -- and the norms are taken over the d real
// elements, so gemm_f16_filter_eps(d) of the real d holds as it stands.
// int8: rows are whole k-steps at every d % 64 == 0, so the engine's int8 copy (uint8 rows ^ 0x80, ensure_i8q)
// keeps d bytes per row; it is padded to whole 128-row tiles (zero rows, bp = kI8qPadBp).  The integer product is
// exact: no slack term, candidates leave with exact scores.  Accumulator range at d = 4096 (|x| <= 128):
//   |q.b| <= 128^2 x 4096 = 2^26;  bp = floor(sum b^2 / 2) <= 2^25;  |g| = |q.b - bp| <= 2^26 + 2^25
//   full scan: acc = q.b + thp, thp = -g_k or 2^30 ("keep every row") -> |acc| <= 2^30 + 2^26 < 2^31;
//              a padded query slot starts at INT_MIN / 2 = -2^30 -> acc <= 2^26 - 2^30 < 0 <= bp: never a hit
//   SAMPLE:    acc = q.b - bp, bp = 2^30 on the padding rows -> acc >= -2^30 - 2^26 > INT_MIN
//   scores:    sum (a - b)^2 <= 255^2 x 4096 < 2^28 (the gather's bias - 2 dot + qself, each term < 2^28)
// so nothing wraps in any mode (the worst case the uint8 metric can reach, 255^2 x 4096 ~ 2.7 x 10^8, included).
// Byte offsets of rows and queries are 64-bit: n * ld * 2 passes 2^32 at ~0.5 M rows of d = 4096.
//
// What the two instances do NOT share (each as the kernel of its own did before they were merged):
//   * the fp16 launch may end on smaller row chunks (GemmF16Params::n_big / tiles_small); GemmI8qParams has no
//     such fields;
//   * the int8 flush also tests row < n_rows (a padding row's bp = 2^30 is what an accumulator that started at the
//     "keep every row" value reaches; the fp16 padding's NaN term never compares true), and the two flushes read
//     the entry's term at different moments -- the generated code differs, so each keeps its own;
//   * a log entry holds bn' - acc as float bits, or the raw integer accumulator (E::log_entry).
// The sampled fold's second v_max3 takes "never" as its third operand on both sides (the fp16 kernel had it so;
// for integers the compiler drops it: no difference to the int8 code).
#pragma once
#include "scan_gemm_elem.hpp"

namespace expann {

constexpr int kKlTB = 128;       // rows per tile
constexpr int kKlBufs = 3;       // stage buffers
constexpr int kKlQcap = kF16WaveQueue;
constexpr int kKlStageBytes = kKlTB * 64 + kF16TQ * 64 + kKlTB * 4;
constexpr int kKlLds = kKlBufs * kKlStageBytes + kF16Waves * kKlQcap * kF16EntryBytes;
static_assert(kKlLds <= 160 * 1024, "LDS budget per CU");

__device__ inline uint32_t kl_swz(uint32_t r) { return (0u - (r >> 2)) & 3u; }

template <class E, bool SAMPLE>
__global__ __launch_bounds__(kF16Threads, 1) void scan_gemm_kl_kernel(typename E::LogParams pl) {
	using Term = typename E::Term;
	using Acc = typename E::Acc;
	using Frag = typename E::Frag;
	const auto& p = E::core(pl);
	constexpr int WAVES = kF16Waves, WGQ = kF16TQ, TB = kKlTB, QCAP = kKlQcap;
	constexpr int NBUF = kKlBufs, SB = kKlStageBytes;
	constexpr int QOFF = TB * 64, TERMOFF = QOFF + WGQ * 64;
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
	if (p.xcd_map) {  // (the row chunks {x, x + 8, ..} of a query tile on XCD x)
		const uint32_t j = bid >> 3;
		qtile = j % p.n_qtiles;
		chunk = (bid & 7) + 8 * (j / p.n_qtiles);
	}
	const uint32_t wg_q0 = qtile * WGQ;
	const uint32_t q0 = wg_q0 + wave * 64;

	uint32_t t0 = chunk * p.tiles_per_block;
	uint32_t t1 = t0 + p.tiles_per_block;
	if constexpr (!E::kExact) {  // (GemmF16Params::n_big: the fp16 launch's tail chunks)
		if (p.tiles_small && chunk >= p.n_big) {
			t0 = p.n_big * p.tiles_per_block + (chunk - p.n_big) * p.tiles_small;
			t1 = t0 + p.tiles_small;
		}
	}
	if (t1 > p.n_tiles_sel)
		t1 = p.n_tiles_sel;
	if (t0 >= t1) {
		if (SAMPLE) {
			for (uint32_t i = lane; i < 64 * 32; i += 64)
				if (q0 + (i >> 5) < p.m)
					p.sample_out[((size_t)(q0 + (i >> 5)) * p.n_chunks + chunk) * 32 + (i & 31)] = E::never();
		} else if (lane == 0) {
			pl.log_cnt[(size_t)bid * WAVES + wave] = 0;
		}
		return;
	}

	auto tile_row0 = [&](uint32_t t) -> uint32_t {
		return ((t / p.tile_run) * (p.tile_stride * p.tile_run) + (t % p.tile_run)) * TB;
	};

	// ---- staging: slot S = i * 256 + tid of a stage (16 B each); slots 0..511 rows, 512..1535 queries ----
	const uint32_t co = (((uint32_t)tid & 3u) ^ kl_swz((uint32_t)tid >> 2)) * 16u;  // (the same for every piece)
	const unsigned char* qsrc[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const uint32_t qr = (uint32_t)(i * 256 + tid) >> 2;
		const uint32_t qi = wg_q0 + qr < p.m ? wg_q0 + qr : p.m - 1;
		qsrc[i] = (const unsigned char*)E::queries(p) + (size_t)qi * ROWB + co;
	}
	const unsigned char* const rbase = (const unsigned char*)E::rows(p) + co;
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
		// the tile's 128 row terms: waves 0 / 2 rows 0-63, waves 1 / 3 rows 64-127 (the same bytes twice: every
		// wave issues 7 loads per stage, so one vmcnt serves all)
		__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(E::row_terms(p) + row0 + (wave & 1) * 64 + lane),
		                                 (__attribute__((address_space(3))) void*)(smem + st_buf * SB + TERMOFF + (wave & 1) * 256),
		                                 4, 0, 0);
		st_buf = st_buf + 1 == NBUF ? 0 : st_buf + 1;
		if (++st_ks == KS) {
			st_ks = 0;
			++st_t;
		}
	};

	// ---- candidates: per-wave LDS queue -> per-wave hit log (8 columns) ----
	using QEntry = ScanQEntry<E>;
	QEntry* const queue = reinterpret_cast<QEntry*>(smem + NBUF * SB) + wave * QCAP;
	uint32_t wfill = 0, glog_n = 0;  // wave-uniform
	uint4* const my_log = SAMPLE ? nullptr : pl.log + ((size_t)bid * WAVES + wave) * pl.log_cap;
	auto flush_own = [&]() {
		const uint32_t n = wfill < (uint32_t)QCAP ? wfill : (uint32_t)QCAP;
		for (uint32_t b0 = 0; b0 < n * 16; b0 += 64) {
			const uint32_t i = b0 + lane;
			const QEntry& e = queue[i < n * 16 ? i >> 4 : 0];
			const uint32_t v = i & 15;
			const Term c = e.acc[v];
			bool hit;
			if constexpr (E::kExact) {  // padding rows are told by their number; the term is read behind the range test
				const uint32_t row = e.row;
				hit = i < n * 16 && c >= e.term && row < p.n_rows;
			} else {  // a padding row's NaN term never compares true; the term is read beside the accumulator
				const Term term = e.term;
				hit = i < n * 16 && c >= term;
			}
			const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
			if (mask == 0)
				continue;
			const uint32_t pos = glog_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
			                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			if (hit && pos < pl.log_cap)
				my_log[pos] = E::log_entry(c, e.term, e.row, e.qrow0 + 16 * (v >> 2) + (v & 3));
			glog_n += (uint32_t)__builtin_popcountll(mask);
		}
		wfill = 0;
	};

	Acc th[4];  // accumulator start values (theta' / -g_k) of each accumulator register's query
#pragma unroll
	for (int tq = 0; tq < 4; ++tq)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t qi = q0 + tq * 16 + 4 * lq + r;
			th[tq][r] = (qi < p.m && !SAMPLE) ? E::starts(p)[qi] : E::no_query();
		}
	Acc smax[2][4];  // SAMPLE: running maxima of g per (class parity, query tile)
#pragma unroll
	for (int par = 0; par < 2; ++par)
#pragma unroll
		for (int tq = 0; tq < 4; ++tq)
			smax[par][tq] = Acc{E::never(), E::never(), E::never(), E::never()};

	const uint32_t fo = (uint32_t)l15 * 64u + (((uint32_t)lq ^ kl_swz((uint32_t)l15)) * 16u);
	stage_next();
	stage_next();
	Acc acc[4][8];
	int buf = 0;
	for (uint32_t t = t0; t < t1; ++t) {
		const uint32_t row0 = tile_row0(t);
		for (uint32_t ks = 0; ks < KS; ++ks) {
			// stage (t, ks) landed (only the next one's 7 loads may be in flight), every wave is done with the
			// buffer the stage after next goes to
			asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory");
			stage_next();
			const unsigned char* sb = smem + buf * SB;
			Term tv[8];  // the row terms of this lane's row in every column
			if (ks == 0 || ks == KS - 1) {
				const Term* ts = reinterpret_cast<const Term*>(sb + TERMOFF);
#pragma unroll
				for (int tc = 0; tc < 8; ++tc)
					tv[tc] = ts[tc * 16 + l15];
			}
			if (ks == 0) {
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
#pragma unroll
					for (int tc = 0; tc < 8; ++tc) {
						if (SAMPLE) {  // the row term enters as the C operand: acc ends at g = q.b - term
							const Term nt = -tv[tc];
							acc[tq][tc] = Acc{nt, nt, nt, nt};
						} else {
							acc[tq][tc] = th[tq];
						}
					}
			}
			Frag a[4], b[8];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const Frag*>(sb + QOFF + (wave * 64 + tq * 16) * 64 + fo);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
				b[tc] = *reinterpret_cast<const Frag*>(sb + tc * 16 * 64 + fo);
			__builtin_amdgcn_s_setprio(1);
#pragma unroll
			for (int tc = 0; tc < 8; ++tc)
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = E::mfma(a[tq], b[tc], acc[tq][tc]);
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
							smax[par][tq][r] = E::max2(E::max3(smax[par][tq][r], acc[tq][par][r], acc[tq][par + 2][r]),
							                           E::max3(acc[tq][par + 4][r], acc[tq][par + 6][r], E::never()));
				continue;
			}
#pragma unroll
			for (int tc = 0; tc < 8; ++tc) {
				Term g = E::never();
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					g = E::max3(g, E::max3(acc[tq][tc][0], acc[tq][tc][1], acc[tq][tc][2]), acc[tq][tc][3]);
				const bool h = g >= tv[tc];
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
					e.term = tv[tc];
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
			pl.log_cnt[(size_t)bid * WAVES + wave] = glog_n;
			if (glog_n > pl.log_cap)  // (the log is as large as this wave's share of the candidate lists)
				atomicAdd(pl.lost, 1u);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the re-staged tail: LDS must outlive the loads)
}

}  // namespace expann
