// scan_redo_i8.hpp -- the scan of the redo pass of the speculative thresholds over the int8 filter's copy
// (operands and integer domain: scan_gemm_i8f.hpp).  A handful of failing queries against every
// row: the pass is a read of the copy, so this kernel is a streaming loop and nothing else -- no LDS tiles, no
// workgroup barrier, no hit logs.  Each wave owns one contiguous range of 16-row columns, loads a column's rows
// straight from global memory into the B fragment of v_mfma_i32_16x16x64_i8 (16 bytes per lane and k-step: lane
// (l15, lq) holds bytes [64 s + 16 lq, +16) of row row0 + l15), multiplies it with the query groups that hold a
// live slot, and files a hit at once with gather_logs_kernel's i_mode-3 arithmetic: key = kappa = bp - acc, -inf
// where bp sits at a clamp limit, slot = atomicAdd(cand_cnt[q]), stored when slot < cap.  A list longer than cap
// keeps counting and drops the key; the redo select's overflow check sees cnt > cap.
//
// Fragments and start values are scan_gemm_i8w_kernel's: a[tq][s] = chunk 4 s + lq of query q0 + 16 tq + l15,
// accumulators start at thp, result register r of group tq = query q0 + 16 tq + 4 lq + r against row row0 + l15.
//
// What this relies on: redo_compact_kernel has zeroed cand_cnt of every slot and has given every slot nobody took
// zero bytes and the start value of a padded query slot (-2^30), which no row's bp is reached from; so the slots
// behind the live count inside a 16-slot group file nothing.  Padding rows carry bp = kI8qPadBp = 2^30 and zero
// bytes; the hit test checks the row number as well.
#pragma once
#include "scan_gemm_i8q.hpp"

namespace expann {

constexpr int kRedoStreamThreads = 256;
constexpr int kRedoStreamWaves = kRedoStreamThreads / 64;
constexpr int kRedoStreamU = 2;          // columns per pipeline stage: the next U are in flight under the current U
constexpr int kRedoStreamWavesPerCu = 16;  // the grid: 4 waves per SIMD (the kernel's registers allow them)

struct RedoStreamParams {
	const void* base;         // [n_cols * 16][128] int8, padding rows zero
	const int* bp;            // [n_cols * 16], kI8qPadBp on the padding
	uint32_t n_rows;
	uint32_t n_cols;          // 16-row columns of the padded copy
	uint32_t cols_per_wave;   // wave w of the grid owns columns [w * cols_per_wave, + cols_per_wave) below n_cols
	const void* queries;      // [n_slots][128] int8, compact (redo_compact_kernel)
	const int* thp;           // [n_slots]
	uint32_t n_slots;         // a multiple of 64
	const uint32_t* live_q;   // the redo word: its low 20 bits = failing queries (may exceed n_slots)
	uint32_t* cand_cnt;       // [n_slots], zero at launch
	uint64_t* cand;           // [n_slots][cap]
	uint32_t cap;
};

__global__ __launch_bounds__(kRedoStreamThreads, 4) void redo_stream_i8_kernel(RedoStreamParams p) {
	constexpr int U = kRedoStreamU, ROWB = 128, KS = 2;
	const int lane = threadIdx.x & 63;
	const int l15 = lane & 15, lq = lane >> 4;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kRedoStreamWaves + (threadIdx.x >> 6));
	const uint32_t c0 = wave * p.cols_per_wave;
	uint32_t c1 = c0 + p.cols_per_wave;
	if (c1 > p.n_cols)
		c1 = p.n_cols;
	uint32_t live = *p.live_q & kRedoCountMask;
	if (live > p.n_slots)
		live = p.n_slots;
	if (c0 >= c1 || live == 0)
		return;  // (whole wave)

	struct Col {
		i32x4 b[KS];
		int bp;
	};
	const unsigned char* const lane_rows = (const unsigned char*)p.base + l15 * ROWB + lq * 16;
	// column c of the range, or the range's last one where c is past it (loaded, never tested): no load leaves
	// the rows below n_cols * 16
	auto load = [&](Col (&f)[U], uint32_t c) {
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t cc = c + u < c1 ? c + u : c1 - 1;
			const unsigned char* src = lane_rows + (size_t)cc * (16 * ROWB);
#pragma unroll
			for (int s = 0; s < KS; ++s)
				f[u].b[s] = *reinterpret_cast<const i32x4*>(src + 64 * s);
			f[u].bp = p.bp[cc * 16 + l15];
		}
	};

	for (uint32_t q0 = 0; q0 < live; q0 += 64) {  // one walk of the range per 64-slot block
		const uint32_t groups = (live - q0 + 15) / 16;  // wave-uniform: query groups of this block with a live slot
		i32x4 a[4][KS], th[4];
#pragma unroll
		for (int tq = 0; tq < 4; ++tq) {
			const i32x4* src = reinterpret_cast<const i32x4*>((const unsigned char*)p.queries + (size_t)(q0 + tq * 16 + l15) * ROWB);
#pragma unroll
			for (int s = 0; s < KS; ++s)
				a[tq][s] = src[4 * s + lq];
#pragma unroll
			for (int r = 0; r < 4; ++r)
				th[tq][r] = p.thp[q0 + tq * 16 + 4 * lq + r];
		}
		auto column = [&](const Col& f, uint32_t c) {
			const uint32_t row = c * 16 + l15;
			const bool row_ok = row < p.n_rows;
#pragma unroll
			for (int tq = 0; tq < 4; ++tq) {
				if ((uint32_t)tq >= groups)
					break;
				i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq][0], f.b[0], th[tq], 0, 0, 0);
				acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq][1], f.b[1], acc, 0, 0, 0);
				const int top = max(max(acc[0], acc[1]), max(acc[2], acc[3]));
				if (__builtin_amdgcn_ballot_w64(top >= f.bp && row_ok) == 0)
					continue;
				uint32_t qlane = q0 + 4 * lq;
				asm volatile("" : "+v"(qlane));  // (query numbers and list addresses are made HERE: hoisted, 16 of each cost 48 registers)
#pragma unroll
				for (int r = 0; r < 4; ++r)
					if (acc[r] >= f.bp && row_ok) {
						const uint32_t qi = qlane + tq * 16 + r;
						const uint32_t slot = atomicAdd(&p.cand_cnt[qi], 1u);
						if (slot < p.cap) {
							const float kappa = (float)(f.bp - acc[r]);
							p.cand[(size_t)qi * p.cap + slot] =
							    make_key(f.bp > kI8fBpMin && f.bp < kI8fBpMax ? kappa : -__builtin_inff(), row);
						}
					}
			}
		};

		// two fragment sets in turn: the loads of one are in flight while the other is multiplied.  Every load is
		// issued on every path (past the range: its last column again), so the counted waits in front of the MFMAs
		// leave the younger set in flight
		auto columns = [&](const Col (&f)[U], uint32_t c) {
#pragma unroll
			for (int u = 0; u < U; ++u)
				if (c + u < c1)
					column(f[u], c + u);
		};
		Col f0[U], f1[U];
		load(f0, c0);
		for (uint32_t c = c0;; c += 2 * U) {
			load(f1, c + U);
			columns(f0, c);
			if (c + U >= c1)
				break;
			load(f0, c + 2 * U);
			columns(f1, c + U);
			if (c + 2 * U >= c1)
				break;
		}
	}
}

}  // namespace expann
