// scan_pq4.hpp -- 4-bit product-quantised rows (EXPANN_DTYPE_PQ4, THE PQ4 RULE of expann_hip.h): ADC as a one-hot
// product on the int8 matrix cores.
//
// A row is M nibbles; code i selects one of 16 centroids of sub-vector i.  The score sum_i T[i][code_i] is the dot
// product of the query's table [16 M] with the row's one-hot vector [16 M]: with the table quantised to bytes (steps
// 2-4 of the rule) it is an int8 GEMM with K = 16 M, exact in int32, on v_mfma_i32_16x16x64_i8.  scan_pq.hpp's "no
// matrix instruction fits" holds for 256 centroids, not for 16.
//
// The geometry, the tile range, the thresholds and the epilogue are scan_tile.hpp's, the float ties scan_i4.hpp's.
// The data movement is the opposite of the 4-bit rows': a row gives 1/32 of a byte per k-element, a query's table a
// whole byte -- so the tile loop is this kernel's own.
//
// 1. The B operand is made in registers and never touches LDS.  Lane (i, g) of the instruction holds, for one k-step,
//    the 16 k-bytes [16 g, 16 g + 16) of column i: exactly the one-hot of ONE nibble c -- four dwords, of which dword
//    c >> 2 is 1 << 8 (c & 3).  v_bfe_u32, a shift, four compare-and-selects: about 11 VALU instructions in front of
//    4 MFMAs (the fragment serves the four query fragments).
//    The k order is free as long as both operands agree, and pq4_tables_kernel writes the A operand in the order that
//    makes the row reads plain: a CHUNK is 16 sub-quantisers = 8 bytes of a row = 4 k-steps; lane (i, g) reads the
//    two bytes 8 u + 2 g of row i (chunk u) -- the four lanes of a row read its 8 consecutive bytes, the 16 rows of a
//    column 16 runs of 8 bytes -- and nibble j of that ushort is its operand of k-step j.  So sub-quantiser
//    16 u + 4 g + j sits at k-bytes [64 j + 16 g, +16) of chunk u: inside every chunk the tables are a 4 x 4 transpose.
//    The codes come straight from global memory, one ushort per column and chunk, two chunks ahead of the MFMAs that
//    use them (three sets of four registers); a fetch past the workgroup's range reads a valid address of its last
//    tile, so no load sits under a branch.
// 2. The A operand -- the tables of the 64 queries, signed bytes u - 128 -- is what LDS is for.
//    RESIDENT (M <= kPQ4ResidentMaxM = 128): [64][16 M + 16] bytes, loaded once per workgroup and kept for its whole
//    row range: 132 096 B at M = 128 of the CU's 160 KiB.  The tile loop has no barrier at all.
//    STREAMED (M > 128: 64 x 16 M bytes no longer fit): chunks of 256 bytes per query go through two stages of
//    [64][256 + 16] bytes (17 408 B each) as scan_i4's stages do -- the loads of chunk i + 1 are issued before the
//    MFMAs of chunk i and stored after them, one barrier per chunk of 64 MFMAs per wave.
//    Banks: a lane reads 16 bytes of a query (ds_read_b128); the 16 lanes of a quarter wave read 16 queries at the
//    same k offset, so the stride must put them on sixteen distinct multiples of 4 dwords: 4 x odd.  16 M + 16 bytes
//    is 4 (M + 1) dwords, M even; 272 bytes is 4 x 17.  Both are asserted below.
// 3. Prep.  pq4_tables_kernel (one workgroup per query, lane = (sub-quantiser mod 16, centroid)) builds T by the rule
//    with pq_term, takes min / max over the 16 centroids as DPP row reductions, the span as a max (exact in any
//    order), the bias as the rule's serial sum, and writes the A operand, bias and step.  S = acc + 128 M; the
//    constant 128 M travels as TileScanParams::qterm_const.  pq4_theta_kernel writes theta = floor(tau) - 128 M before every
//    level that has thresholds (tau is (float)S of the proven key, an exact integer or +inf).  pq4_finish_kernel
//    applies step 7 to the selected [m][k] outputs.
//
// One form for every m >= 1: a batch below 64 queries pays for the whole 64-query fragment set.
// Rows must be 8-byte aligned on the device (M / 2 is a multiple of 8, so every row is).
#pragma once
#include "scan_hamming.hpp"
#include "scan_pq.hpp"

namespace expann {

constexpr uint32_t kPQ4ChunkBytes = 256;      // A bytes of a query per chunk: 16 sub-quantisers x 16 centroids = 4 k-steps
constexpr uint32_t kPQ4ResidentMaxM = 128;    // above it the tables stream through two stages
constexpr uint32_t kPQ4StageStride = kPQ4ChunkBytes + 16;
constexpr uint32_t kPQ4StageBytes = kHamTQ * kPQ4StageStride;
__host__ __device__ constexpr uint32_t pq4_q_stride(uint32_t M) { return 16 * M + 16; }  // bytes of a resident query's tables in LDS
__host__ __device__ constexpr bool pq4_resident(uint32_t M) { return M <= kPQ4ResidentMaxM; }
__host__ __device__ constexpr uint32_t pq4_lds_bytes(uint32_t M) {
	return pq4_resident(M) ? kHamTQ * pq4_q_stride(M) : 2 * kPQ4StageBytes;
}
// (4 x odd dwords: 16 consecutive queries at one k offset start on sixteen distinct multiples of 4 banks)
__host__ __device__ constexpr bool pq4_stride_ok(uint32_t bytes) { return bytes % 16 == 0 && (bytes / 16) % 2 == 1; }
static_assert(pq4_stride_ok(pq4_q_stride(16)) && pq4_stride_ok(pq4_q_stride(48)) && pq4_stride_ok(pq4_q_stride(128)) &&
                  pq4_stride_ok(kPQ4StageStride),
              "the bank reasoning of the header comment");
static_assert(pq4_lds_bytes(kPQ4ResidentMaxM) == 132096 && pq4_lds_bytes(kPQ4ResidentMaxM) <= 160 * 1024 &&
                  kHamTQ * pq4_q_stride(kPQ4ResidentMaxM + 32) > 160 * 1024 && pq4_lds_bytes(256) == 34816,
              "LDS budget per CU: where the resident form ends");
static_assert(kHamThreads == 512 && kHamTB == 512 && kHamTQ == 64 && kHamNT == 4, "the staging below: 2 pieces of 16 bytes per thread and chunk");

// S = acc + 128 M, ranked as (float)S (ties on the floats, as the 4-bit rows')
struct PQ4Policy {
	static constexpr bool kFloatTies = true;
	__device__ static int row_term(const TileScanParams&, uint32_t, bool) { return 0; }
	__device__ static int combine(const TileScanParams&, int, int acc) { return acc; }
	__device__ static int query_term(const TileScanParams& p, uint32_t) { return p.qterm_const; }
};

__device__ __attribute__((always_inline)) inline float pq4_min16(float v) {
	v = __builtin_fminf(v, row_ror<8>(v));
	v = __builtin_fminf(v, row_ror<4>(v));
	v = __builtin_fminf(v, row_ror<2>(v));
	return __builtin_fminf(v, row_ror<1>(v));
}
__device__ __attribute__((always_inline)) inline float pq4_max16(float v) {
	v = __builtin_fmaxf(v, row_ror<8>(v));
	v = __builtin_fmaxf(v, row_ror<4>(v));
	v = __builtin_fmaxf(v, row_ror<2>(v));
	return __builtin_fmaxf(v, row_ror<1>(v));
}

// Steps 1-5 of THE PQ4 RULE for one query per workgroup.  Lane (s, c) = (tid / 16, tid % 16) builds entry c of the
// sub-quantisers s, s + 16, ...; the 16 centroids of a sub-quantiser are one DPP row.
template <bool IP> __global__ __launch_bounds__(kBlock) void pq4_tables_kernel(const float* queries, const float* codebooks, uint32_t M,
                                                                               uint32_t dsub, void* tables, float* bias, float* step) {
#pragma clang fp contract(off)
	__shared__ float T_s[256 * 16];
	__shared__ float lo_s[256];
	__shared__ float span_s[16];
	const uint32_t q = blockIdx.x, tid = threadIdx.x, c = tid & 15, sub = tid >> 4;
	const float* __restrict__ qv = queries + (size_t)q * M * dsub;
	float spread = 0.0f;
	for (uint32_t i = sub; i < M; i += 16) {
		const float* __restrict__ cv = codebooks + ((size_t)i * 16 + c) * dsub;
		float T = 0.0f;
		for (uint32_t d = 0; d < dsub; ++d)
			T = pq_term<IP>(T, qv[i * dsub + d], cv[d]);
		if (IP)
			T = 0.0f - T;  // (smaller is better under both metrics; never -0.0)
		const float lo = pq4_min16(T);
		spread = __builtin_fmaxf(spread, pq4_max16(T) - lo);
		T_s[i * 16 + c] = T;
		if (c == 0)
			lo_s[i] = lo;
	}
	if (c == 0)
		span_s[sub] = spread;  // (M >= 16: every one of the 16 slots has a sub-quantiser)
	__syncthreads();
	float span = span_s[0];
#pragma unroll
	for (int s = 1; s < 16; ++s)
		span = __builtin_fmaxf(span, span_s[s]);
	const float r = span > 0.0f ? __fdiv_rn(255.0f, span) : 0.0f;
	if (tid == 0) {
		float b = lo_s[0];
		for (uint32_t i = 1; i < M; ++i)
			b = b + lo_s[i];
		bias[q] = b;
		step[q] = span > 0.0f ? __fdiv_rn(span, 255.0f) : 0.0f;
	}
	// one dword = centroids 4 w .. 4 w + 3 of sub-quantiser i, at its place in the scan's k order
	uint32_t* __restrict__ dst = (uint32_t*)tables + (size_t)q * 4 * M;
	for (uint32_t d = tid; d < 4 * M; d += kBlock) {
		const uint32_t i = d >> 2, w = d & 3;
		const float lo = lo_s[i];
		uint32_t word = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const float t = T_s[i * 16 + 4 * w + b] - lo;
			const float u = __builtin_fminf(255.0f, __builtin_rintf(t * r));
			word |= (uint32_t)(((int)u - 128) & 255) << (8 * b);
		}
		const uint32_t g = (i >> 2) & 3, j = i & 3;
		dst[(i >> 4) * 64 + j * 16 + g * 4 + w] = word;
	}
}

// theta = floor(tau) - 128 M (tau = +inf: every row passes)
static __global__ __launch_bounds__(kBlock) void pq4_theta_kernel(const float* tau, uint32_t m, int qterm, int* theta) {
	const uint32_t qi = blockIdx.x * kBlock + threadIdx.x;
	if (qi >= m)
		return;
	const float t = tau[qi];
	const int ft = !(t < 1.0e9f) ? 1000000000 : (t < -1.0e9f ? -1000000000 : (int)__builtin_floorf(t));
	theta[qi] = ft - qterm;
}

// step 7 on the selected outputs: dist = bias + step * (float)S, two operations; the padding stays +inf
static __global__ __launch_bounds__(kBlock) void pq4_finish_kernel(float* dists, size_t total, uint32_t k, const float* bias,
                                                                   const float* step) {
#pragma clang fp contract(off)
	for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kBlock) {
		const size_t q = idx / k;
		const float S = dists[idx];
		if (S < __builtin_inff()) {
			const float pr = step[q] * S;
			dists[idx] = bias[q] + pr;
		}
	}
}

// the one-hot of a nibble as the 16 k-bytes of a B operand
__device__ __attribute__((always_inline)) inline ham_i32x4 pq4_onehot(uint32_t c) {
	const int v = 1 << ((c & 3u) * 8u);
	const uint32_t w = c >> 2;
	return ham_i32x4{w == 0 ? v : 0, w == 1 ? v : 0, w == 2 ? v : 0, w == 3 ? v : 0};
}

struct PQ4Codes {
	uint32_t w[kHamNT];  // per column: the lane's four nibbles of the chunk
};

template <bool RESIDENT> __global__ __launch_bounds__(kHamThreads) void scan_pq4_mfma_kernel(TileScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char pq4_smem[];
	TileLane w;
	if (!tile_range(p, w))
		return;
	const uint32_t tid = w.tid, wave = w.wave, i = w.i, g = w.g, q0 = w.q0, t0 = w.t0, t1 = w.t1;
	const uint32_t M = p.klen, NC = M / 16;  // chunks of the reduction dimension
	const uint32_t QS = RESIDENT ? pq4_q_stride(M) : kPQ4StageStride;
	const uint32_t n_items = (t1 - t0) * NC;
	int th[4][4];
	tile_thresholds(p, w, th);

	// the stream of row codes, (tile, chunk) by (tile, chunk): ushort 4 u + g of the lane's row in each column
	const unsigned short* __restrict__ rows = (const unsigned short*)p.base;
	const uint32_t RU = M / 4;  // ushorts per row
	uint32_t pf_t = t0, pf_c = 0;
	auto fetch = [&](PQ4Codes& o) {
		const uint32_t tt = pf_t < t1 ? pf_t : t1 - 1;  // (past the range: the last tile again, a valid address)
		const uint32_t r0 = tt * p.tile_stride * kHamTB + wave * 64 + i;
#pragma unroll
		for (int tc = 0; tc < kHamNT; ++tc) {
			const uint32_t r = r0 + 16 * tc < p.n_rows ? r0 + 16 * tc : p.n_rows - 1;
			o.w[tc] = rows[(size_t)r * RU + 4 * pf_c + g];
		}
		if (++pf_c == NC) {  // (uniform)
			pf_c = 0;
			++pf_t;
		}
	};
	PQ4Codes w0, w1;
	fetch(w0);
	fetch(w1);

	// the tables: 16-byte pieces, M per query (16 per chunk); slots past m repeat the last query and never file
	const ham_i32x4* __restrict__ tab = (const ham_i32x4*)p.a_operand;
	ham_i32x4 av[2];
	auto a_load = [&](uint32_t c) {
#pragma unroll
		for (uint32_t j = 0; j < 2; ++j) {
			const uint32_t pc = tid + j * kHamThreads, qq = pc >> 4, pv = pc & 15;
			const uint32_t qi = q0 + qq < p.m ? q0 + qq : p.m - 1;
			av[j] = tab[(size_t)qi * M + c * 16 + pv];
		}
	};
	auto a_store = [&](unsigned char* buf) {
#pragma unroll
		for (uint32_t j = 0; j < 2; ++j) {
			const uint32_t pc = tid + j * kHamThreads, qq = pc >> 4, pv = pc & 15;
			*reinterpret_cast<ham_i32x4*>(buf + qq * kPQ4StageStride + 16 * pv) = av[j];
		}
	};
	if (RESIDENT) {
		for (uint32_t pc = tid; pc < kHamTQ * M; pc += kHamThreads) {
			const uint32_t qq = pc / M, pv = pc - qq * M;
			const uint32_t qi = q0 + qq < p.m ? q0 + qq : p.m - 1;
			*reinterpret_cast<ham_i32x4*>(pq4_smem + qq * QS + 16 * pv) = tab[(size_t)qi * M + pv];
		}
		__syncthreads();
	} else {
		a_load(0);
		a_store(pq4_smem);
	}

	ham_i32x4 acc[4][kHamNT];
	uint32_t t = t0, c = 0;
	for (uint32_t it = 0; it < n_items; ++it) {
		const PQ4Codes cur = w0;
		w0 = w1;
		fetch(w1);  // two chunks ahead
		uint32_t tn = t, cn = c + 1;
		if (cn == NC) {
			cn = 0;
			tn = t + 1;
		}
		const bool more = it + 1 < n_items;
		if (!RESIDENT) {
			if (more)  // in flight while this stage is multiplied
				a_load(cn);
			__syncthreads();  // this stage is in place; the other one has been read
		}
		const unsigned char* const abuf = RESIDENT ? pq4_smem + c * kPQ4ChunkBytes : pq4_smem + (it & 1) * kPQ4StageBytes;
		if (c == 0)
			tile_clear(acc);
		const unsigned char* const qf = abuf + i * QS + 16 * g;
#pragma unroll
		for (int j = 0; j < 4; ++j) {  // k-step j of the chunk: nibble j of the lane's ushort
			ham_i32x4 a[4];
#pragma unroll
			for (int tq = 0; tq < 4; ++tq)
				a[tq] = *reinterpret_cast<const ham_i32x4*>(qf + 16 * tq * QS + 64 * j);
#pragma unroll
			for (int tc = 0; tc < kHamNT; ++tc) {
				const ham_i32x4 f = pq4_onehot((cur.w[tc] >> (4 * j)) & 15u);
#pragma unroll
				for (int tq = 0; tq < 4; ++tq)
					acc[tq][tc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[tq], f, acc[tq][tc], 0, 0, 0);
			}
		}
		if (!RESIDENT && more)
			a_store(pq4_smem + ((it + 1) & 1) * kPQ4StageBytes);
		if (c == NC - 1)
			tile_epilogue<PQ4Policy>(p, w, t, acc, th);
		t = tn;
		c = cn;
	}
}

}  // namespace expann
