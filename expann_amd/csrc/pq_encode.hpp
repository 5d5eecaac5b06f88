// pq_encode.hpp -- product-quantiser codes and codebooks from fp32 rows (THE ENCODE RULE and THE TRAIN RULE of
// expann_hip.h): expann_pq_encode / expann_pq_encode_device / expann_pq_train.
//
// pq_encode_kernel<NCENT>: the hot path, n * dim * NCENT subtract-square-adds.  The rule is one sequential fp32 chain
// per (row, sub-quantiser, centroid), each operation rounded by itself; no matrix instruction computes a sum in that
// order with those roundings, so this is a VALU kernel.
//   Split: a workgroup (256 threads) owns kEncRows = 256 rows -- a lane owns a ROW -- and kEncGroup = 16
//   sub-quantisers; the grid is (row tiles, groups of sub-quantisers), so a small n still fills the machine and the
//   16 codes of a lane are 16 (PQ8) / 8 (PQ4) contiguous bytes of its output row.
//   Centroids: every lane of a wave meets the same centroid values, so they arrive as SCALAR operands: the codebooks
//   are first transposed to [M][dsub][NCENT] (pq_transpose_kernel; dim * NCENT floats, L2-resident), where the 16
//   centroids of a block at one j are 64 contiguous bytes -- one 16-dword scalar load per j.  Adjacent centroids are
//   adjacent registers, which is what the packed fp32 instructions want: pq_term<false> is stepped on pairs of
//   centroids, each half rounding by itself.  The ISA per j and 16 centroids: 16 v_sub_f32 with the centroid as the
//   scalar operand (the compiler does not pack an SGPR pair against a broadcast x), 8 v_pk_mul_f32, 8 v_pk_add_f32;
//   no v_fma / v_fmac / v_pk_fma anywhere in the kernel.
//   Rows: a tile [256 rows][36 columns] in LDS, loaded with coalesced 16-byte reads (rows are 16-byte aligned: dim is
//   a multiple of 8) and kept at a stride of 37 floats, odd, so the 64 lanes of a wave reading column j of their own
//   rows touch 64 distinct banks.  A tile starts at a multiple of four columns at or below the first one asked for
//   and serves every sub-quantiser that lies inside it (twelve of them at dsub 3, one at dsub 32).
//   Order: for a sub-quantiser, centroid blocks of 16 outermost; inside a block j = 0, 1, ... with x read from LDS
//   once per j (one ds_read_b32 per 32 VALU instructions), so nothing is ever held per lane but the 16
//   accumulators and there is no register limit on dsub.  What is limited is the tile: a sub-vector longer than
//   kEncChunk = 32 columns is STREAMED -- each centroid block walks it chunk by chunk, reloading the tile, and every
//   accumulator still sees j in order.  (The rows are then read NCENT / 16 times, from L2.)
//   Argmin: after a block the 16 sums are folded into the lane's (best D, best c) in ascending c with a strict <, so
//   the lower centroid wins a tie; no cross-lane step exists anywhere.
//   Codes: shifted into a 128-bit (PQ8) / 64-bit (PQ4, low nibble first) register value as they are found and stored
//   as one 16-byte or 8-byte piece straight from registers -- a lane's piece is contiguous in the output already,
//   LDS would add nothing.  With `codes_t` the kernel also writes one byte per code transposed, [M][n], for the trainer
//   (coalesced: consecutive lanes are consecutive rows).
//
// pq_update_kernel: step (b) of THE TRAIN RULE, deterministic by construction (no atomics).  A wave owns one
// (sub-quantiser, centroid): it walks column i of the transposed codes 64 rows at a time, ballots the lanes whose code
// is c, and visits the set bits from low to high; lane j adds X[r][i * dsub + j] into an fp64 accumulator (dsub over 64:
// eight accumulators a lane).  Four rows are fetched before their four adds, in order.  cnt is a sum of popcounts.
//
// pq_init_kernel: the rule's initial centroids, a gather.
#pragma once
#include "common.hpp"
#include "scan_pq.hpp"

namespace expann {

constexpr int kEncRows = kBlock;            // rows of a workgroup tile: one per lane
constexpr int kEncGroup = 16;               // sub-quantisers of a workgroup
constexpr int kEncBlockC = 16;              // centroids whose sums a lane carries at a time
constexpr int kEncChunk = 32;               // columns of a sub-vector served by one tile
constexpr int kEncTileW = kEncChunk + 4;    // a tile starts up to 3 columns early (16-byte reads)
constexpr int kEncStride = kEncTileW + 1;   // odd: a lane reading its own row is conflict-free

typedef float pq_float2 __attribute__((ext_vector_type(2)));  // two centroids of one packed fp32 instruction

// [M][ncent][dsub] -> [M][dsub][ncent]
__global__ __launch_bounds__(kBlock) void pq_transpose_kernel(const float* __restrict__ cb, float* __restrict__ cbt, uint32_t M,
                                                               uint32_t ncent, uint32_t dsub) {
	const uint32_t total = M * ncent * dsub;
	for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += gridDim.x * kBlock) {
		const uint32_t c = e % ncent, j = (e / ncent) % dsub, i = e / (ncent * dsub);
		cbt[e] = cb[((size_t)i * ncent + c) * dsub + j];
	}
}

// THE TRAIN RULE, init: centroid c of sub-quantiser i is sub-vector i of row floor(c * n / ncent)
__global__ __launch_bounds__(kBlock) void pq_init_kernel(const float* __restrict__ X, float* __restrict__ cb, uint32_t n, uint32_t dim,
                                                          uint32_t M, uint32_t ncent) {
	const uint32_t dsub = dim / M, total = dim * ncent;
	for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += gridDim.x * kBlock) {
		const uint32_t j = e % dsub, c = (e / dsub) % ncent, i = e / (dsub * ncent);
		const uint64_t r = (uint64_t)c * n / ncent;
		cb[e] = X[r * dim + i * dsub + j];
	}
}

// rows [n][dim] and codes [n][M] / [n][M / 2] 16-byte aligned; cbt [M][dsub][NCENT] (pq_transpose_kernel); codes_t
// [M][n], one byte per code; either output may be nullptr.  (Separate __restrict__ arguments: the centroid loads are
// scalar loads only where the compiler knows that no store of the kernel touches them.)
template <int NCENT>
__global__ __launch_bounds__(kBlock) void pq_encode_kernel(const float* __restrict__ rows, const float* __restrict__ cbt,
                                                            uint8_t* __restrict__ codes, uint8_t* __restrict__ codes_t, uint32_t n,
                                                            uint32_t dim, uint32_t M) {
	static_assert(NCENT % kEncBlockC == 0, "whole centroid blocks");
	__shared__ float tile[kEncRows * kEncStride];
	const uint32_t tid = threadIdx.x;
	const uint32_t dsub = dim / M;
	const uint32_t row0 = blockIdx.x * kEncRows, row = row0 + tid;
	const uint32_t i0 = blockIdx.y * kEncGroup;
	const uint32_t i1 = (i0 + kEncGroup < M) ? i0 + kEncGroup : M;
	const uint32_t col_end = i1 * dsub;  // (a multiple of 4 only at i1 = M: the reads below stop at dim, which is one)
	const float* xrow = tile + tid * kEncStride;
	uint32_t t0 = 0xFFFFFFFFu;  // first column of the tile in LDS (none yet); uniform, as all the control flow below
	uint32_t w[4] = {0, 0, 0, 0};  // the codes of this lane, the first one lowest once the group is complete
	for (uint32_t i = i0; i < i1; ++i) {
		float best = __builtin_inff();
		uint32_t bestc = 0;
		for (uint32_t c0 = 0; c0 < NCENT; c0 += kEncBlockC) {
			pq_float2 D[kEncBlockC / 2];  // centroids c0 + 2 e, c0 + 2 e + 1
#pragma unroll
			for (int e = 0; e < kEncBlockC / 2; ++e)
				D[e] = pq_float2{0.0f, 0.0f};
			for (uint32_t j0 = 0; j0 < dsub; j0 += kEncChunk) {
				const uint32_t len = (dsub - j0 < kEncChunk) ? dsub - j0 : kEncChunk;
				const uint32_t col = i * dsub + j0;
				if (t0 == 0xFFFFFFFFu || col < t0 || col + len > t0 + kEncTileW) {
					__syncthreads();  // (every lane is done with the tile that goes)
					t0 = col & ~3u;
					for (uint32_t e = tid; e < kEncRows * (kEncTileW / 4); e += kBlock) {
						const uint32_t r = e / (kEncTileW / 4), q = e % (kEncTileW / 4);
						const uint32_t cc = t0 + 4 * q;
						float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};
						if (row0 + r < n && cc < col_end && cc < dim)
							v = *reinterpret_cast<const float4*>(rows + (size_t)(row0 + r) * dim + cc);
						float* d = tile + r * kEncStride + 4 * q;
						d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
					}
					__syncthreads();
				}
				const float* x = xrow + (col - t0);
				const float4* cj = reinterpret_cast<const float4*>(cbt + ((size_t)col * NCENT + c0));
#pragma unroll 2
				for (uint32_t j = 0; j < len; ++j, cj += NCENT / 4) {
					const pq_float2 xv = pq_float2{x[j], x[j]};
					const float4 a = cj[0], b = cj[1], c = cj[2], d = cj[3];  // (uniform addresses: scalar loads)
					const pq_float2 cv[kEncBlockC / 2] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}, {c.x, c.y}, {c.z, c.w}, {d.x, d.y}, {d.z, d.w}};
#pragma unroll
					for (int e = 0; e < kEncBlockC / 2; ++e)
						D[e] = pq_term<false>(D[e], xv, cv[e]);
				}
			}
#pragma unroll
			for (int c = 0; c < kEncBlockC; ++c) {  // ascending c, strict <: a tie stays with the lower centroid
				const float Dc = (c & 1) ? D[c / 2].y : D[c / 2].x;
				const bool lt = Dc < best;
				best = lt ? Dc : best;
				bestc = lt ? c0 + c : bestc;
			}
		}
		if (codes_t && row < n)
			codes_t[(size_t)i * n + row] = (uint8_t)bestc;
		if (NCENT == 16) {
			w[0] = (w[0] >> 4) | (w[1] << 28);
			w[1] = (w[1] >> 4) | (bestc << 28);
		} else {
			w[0] = (w[0] >> 8) | (w[1] << 24);
			w[1] = (w[1] >> 8) | (w[2] << 24);
			w[2] = (w[2] >> 8) | (w[3] << 24);
			w[3] = (w[3] >> 8) | (bestc << 24);
		}
	}
	if (!codes || row >= n)
		return;
	if (NCENT == 16) {  // (M is a multiple of 16: the group is complete, 8 bytes)
		*reinterpret_cast<uint2*>(codes + (size_t)row * (M / 2) + i0 / 2) = uint2{w[0], w[1]};
		return;
	}
	uint8_t* dst = codes + (size_t)row * M + i0;
	if (i1 - i0 == kEncGroup && M % 16 == 0) {
		*reinterpret_cast<uint4*>(dst) = uint4{w[0], w[1], w[2], w[3]};
	} else if (i1 - i0 == kEncGroup) {  // (M = 8 mod 16: the rows are 8-byte aligned only)
		reinterpret_cast<uint2*>(dst)[0] = uint2{w[0], w[1]};
		reinterpret_cast<uint2*>(dst)[1] = uint2{w[2], w[3]};
	} else {  // (the last 8 codes of such an M: they were shifted half way down)
		*reinterpret_cast<uint2*>(dst) = uint2{w[2], w[3]};
	}
}

// THE TRAIN RULE, step (b).  One wave per (i, c); the sums in fp64, the rows of a centroid in ascending order.
__global__ __launch_bounds__(kBlock) void pq_update_kernel(const float* __restrict__ X, const uint8_t* __restrict__ codes_t,
                                                            float* __restrict__ cb, uint32_t n, uint32_t dim, uint32_t M, uint32_t ncent) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t pair = blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (pair >= M * ncent)
		return;
	const uint32_t i = pair / ncent, c = pair % ncent, dsub = dim / M, nu = (dsub + 63) / 64;
	const uint8_t* col = codes_t + (size_t)i * n;
	const float* xi = X + i * dsub;
	double s[8];
#pragma unroll
	for (int u = 0; u < 8; ++u)
		s[u] = 0.0;
	uint32_t cnt = 0;
	for (uint32_t r0 = 0; r0 < n; r0 += 64) {
		const uint32_t r = r0 + lane;
		unsigned long long mask = __builtin_amdgcn_ballot_w64(r < n && col[r] == c);
		cnt += (uint32_t)__builtin_popcountll(mask);
		while (mask) {  // up to four rows a turn: their loads first, then their adds in order
			uint32_t b[4];
			bool have[4];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				have[k] = mask != 0;
				b[k] = have[k] ? (uint32_t)__builtin_ctzll(mask) : 0;
				mask &= mask - 1;  // (0 stays 0)
			}
#pragma unroll
			for (int u = 0; u < 8; ++u) {
				const uint32_t j = u * 64 + lane;
				if ((uint32_t)u < nu && j < dsub) {
					float x[4];
#pragma unroll
					for (int k = 0; k < 4; ++k)
						x[k] = have[k] ? xi[(size_t)(r0 + b[k]) * dim + j] : 0.0f;
#pragma unroll
					for (int k = 0; k < 4; ++k)
						if (have[k])
							s[u] = s[u] + (double)x[k];
				}
			}
		}
	}
	if (cnt == 0)  // an empty cluster keeps its centroid
		return;
#pragma unroll
	for (int u = 0; u < 8; ++u) {
		const uint32_t j = u * 64 + lane;
		if (j < dsub)
			cb[((size_t)i * ncent + c) * dsub + j] = (float)(s[u] / (double)cnt);
	}
}

}  // namespace expann
