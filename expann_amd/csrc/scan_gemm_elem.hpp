// scan_gemm_elem.hpp -- what the 16 x 16 MFMA scan kernels need to know about their operands.  A kernel that
// exists once per geometry (scan_gemm_kl.hpp, scan_gemm_w8.hpp) takes one of the two structs below as a template
// parameter; everything else about it -- block placement, staging, queues, step order, the sampled fold -- is
// written once.
//
//              fragment  accumulator / row term        MFMA                       "never"   candidates leave as
//   F16Elem    f16x8     float: acc + theta' >= bn'    v_mfma_f32_16x16x32_f16    -inf      approximate keys
//   I8Elem     i32x4     int:   acc - g_k   >= bp      v_mfma_i32_16x16x64_i8     INT_MIN   exact integer scores
//
// A k-step is 64 bytes of a row for both (32 fp16 values, 64 int8 values), so byte geometry, swizzles and
// staging never ask which one they move.  The parameter structs stay the hosts' (GemmF16Params; GemmI8qParams
// and, with the hit logs beside it, GemmI8wParams): core() gives the struct that holds the scan's own fields,
// whose names are the same on both sides, and the accessors below name the four that differ.
#pragma once
#include "scan_gemm_f16.hpp"
#include "scan_gemm_i8q.hpp"

namespace expann {

struct F16Elem {
	using Frag = f16x8;             // 64 bytes of a row per 4 lanes: one lane's share of a k-step
	using Acc = f32x4;
	using Term = float;             // an accumulator register, a row term, a start value
	using Params = GemmF16Params;   // kernels that append to the candidate lists themselves
	using LogParams = GemmF16Params;  // kernels that write per-wave hit logs
	template <int D> using Geom = F16Geom<D>;
	static constexpr int kBytes = 2;      // per element of a row
	static constexpr bool kExact = false;
	__device__ static Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
	__device__ static Term never() { return -__builtin_inff(); }
	__device__ static Term no_query() { return -__builtin_inff(); }  // start value of a query slot past m
	__device__ static Term max2(Term a, Term b) { return __builtin_fmaxf(a, b); }
	__device__ static Term max3(Term a, Term b, Term c) { return max3f(a, b, c); }
	__device__ static const GemmF16Params& core(const GemmF16Params& p) { return p; }
	__device__ static const void* rows(const GemmF16Params& c) { return c.base_f16; }
	__device__ static const void* queries(const GemmF16Params& c) { return c.queries_f16; }
	__device__ static const Term* row_terms(const GemmF16Params& c) { return c.bnorm; }
	__device__ static const Term* starts(const GemmF16Params& c) { return c.theta; }
	// a hit's log entry: bn' - acc as float bits (gather_logs_kernel adds theta' and makes the key)
	__device__ static uint4 log_entry(Term c, Term bn, uint32_t row, uint32_t query) {
		return make_uint4(__builtin_bit_cast(uint32_t, bn - c), row, query, 0u);
	}
};

struct I8Elem {
	using Frag = i32x4;
	using Acc = i32x4;
	using Term = int;
	using Params = GemmI8qParams;
	using LogParams = GemmI8wParams;
	template <int D> using Geom = I8qGeom<D>;
	static constexpr int kBytes = 1;
	static constexpr bool kExact = true;  // integer scores: padding rows are told by their number, not by a NaN term
	__device__ static Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
	__device__ static Term never() { return -2147483647 - 1; }
	__device__ static Term no_query() { return never() / 2; }  // dot + that never reaches a bp >= 0, and does not wrap
	__device__ static Term max2(Term a, Term b) { return max(a, b); }
	__device__ static Term max3(Term a, Term b, Term c) { return max3i(a, b, c); }
	__device__ static const GemmI8qParams& core(const GemmI8qParams& p) { return p; }
	__device__ static const GemmI8qParams& core(const GemmI8wParams& p) { return p.q; }
	__device__ static const void* rows(const GemmI8qParams& c) { return c.base; }
	__device__ static const void* queries(const GemmI8qParams& c) { return c.queries; }
	__device__ static const Term* row_terms(const GemmI8qParams& c) { return c.bp; }
	__device__ static const Term* starts(const GemmI8qParams& c) { return c.thp; }
	// a hit's log entry: the raw accumulator (gather_logs_kernel makes the exact score, GatherLogParams::i_mode)
	__device__ static uint4 log_entry(Term c, Term, uint32_t row, uint32_t query) {
		return make_uint4((uint32_t)c, row, query, 0u);
	}
};

// one entry of a wave's hit queue in LDS: the accumulators of a lane's tile column, their row term, the row, the
// first query (value i belongs to query qrow0 + 16 (i >> 2) + (i & 3))
template <class E> struct ScanQEntry {
	typename E::Term acc[16];
	typename E::Term term;
	uint32_t row;
	uint32_t qrow0;
	uint32_t pad;
};
static_assert(sizeof(ScanQEntry<F16Elem>) == kF16EntryBytes && sizeof(ScanQEntry<I8Elem>) == kF16EntryBytes,
              "queue entry size");

}  // namespace expann
