// bf_plan.hpp -- which scan serves a brute-force search: THE list of the rules.  plan_scan() reads what the handle
// knows, the call's shape and what earlier attempts of the same search learned, and names the kernel family, the
// extras that ride on it and, for a search the options rule out, the refusal.  expann_hip.hip looks its variant
// tables up by the answer and decides no family by itself; every crossover below was measured, and
// tests/test_bf_plan.py pins both sides of each without a device.
// Host arithmetic on the standard library alone: no HIP here, no allocation.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/expann_hip.h"

namespace expann {

// 8-bit row modes (IntMode of scan_int8.hpp; -1: float rows)
constexpr int kPlanU8L2 = 0, kPlanI8L2 = 1, kPlanI8L2Ref = 2, kPlanI8IP = 3, kPlanI16L2Ref = 4;
constexpr int kPlanMaxDim = 4096;  // kMaxAnyDim

// ---- the dims each family is compiled for (the variant tables of expann_hip.hip are checked against these) ----
struct DimTiles {
	int d;
	int tq[6];  // query tiles, zero-terminated
};
// the exact direct scan: compiled dims of fp32 rows; every other multiple of 16, and binary16 rows at every dim, take
// the run-time-dim kernels
constexpr DimTiles kScanF32Tiles[] = {{64, {1, 4, 16}},  {128, {1, 2, 4, 8, 16}}, {256, {1, 4, 8}}, {512, {1, 4}},
                                      {768, {1, 2}},     {832, {1, 2}},           {960, {1, 2}},    {1024, {1, 2}}};
constexpr DimTiles kScanF32AnyTiles = {0, {1, 2, 4}};
// ... of 8-bit rows (every mode but int16), of int16 rows; every other multiple of 64: the run-time-dim kernels
constexpr DimTiles kScanI8Tiles[] = {{64, {1, 16}},     {128, {1, 4, 16}}, {256, {1, 8}},
                                     {768, {1, 4, 8}}, {832, {1, 4}},     {960, {1, 4}}};
constexpr DimTiles kScanI16Tiles[] = {{64, {1, 4, 16}}, {128, {1, 8}}};
constexpr DimTiles kScanI8AnyTiles = {0, {1, 4, 8}};
// the fp16 filter streamed without the matrix cores (scan_direct_f16.hpp): queries per pass
constexpr DimTiles kDirectF16Tiles[] = {{64, {2, 4}}, {128, {2, 4}}, {256, {2, 4}}, {512, {1, 2}},
                                        {768, {1}},   {832, {1}},    {960, {1}}};
constexpr int kF16XDims[] = {64, 128};        // scan_gemm_f16x.hpp (the form with a redo instance of its scan: speculation)
constexpr int kF16YDims[] = {256, 512};       // scan_gemm_w8.hpp, fp16 instances
constexpr int kF16KXDims[] = {768, 832, 960};  // scan_gemm_f16kx.hpp
constexpr int kF16DbgDim = 128;               // the instance with the ablation switches compiled in
constexpr int kBf16Dims[] = {64, 128};        // scan_gemm_bf16.hpp
constexpr int kGemmI8Dims[] = {128, 256, 768};      // scan_gemm_i8.hpp: U8L2, I8L2, I8IP
constexpr int kI8qWDims[] = {128, 256};             // scan_gemm_i8w.hpp: the same three modes
constexpr int kI8qXDims[] = {768, 832, 960, 896};   // scan_gemm_w8.hpp, int8 instances
constexpr int kI8fDim = 128;                        // scan_gemm_i8f.hpp: the int8 filter of fp32 rows
constexpr size_t kI8MinRows = 2 * 256 * 64;         // the int8 hit-log forms: two 256-tile chunks of 64 rows at least

template <size_t N> constexpr bool has_dim(const int (&dims)[N], int d) {
	for (int x : dims)
		if (x == d)
			return true;
	return false;
}
template <size_t N> constexpr const DimTiles* tiles_of(const DimTiles (&tab)[N], int d) {
	for (const DimTiles& t : tab)
		if (t.d == d)
			return &t;
	return nullptr;
}
constexpr bool has_tile(const DimTiles* t, int tq) {
	for (int i = 0; t && t->tq[i]; ++i)
		if (t->tq[i] == tq)
			return true;
	return false;
}
constexpr size_t count_tiles(const DimTiles* t, size_t n) {
	size_t c = 0;
	for (size_t j = 0; j < n; ++j)
		for (int i = 0; t[j].tq[i]; ++i)
			++c;
	return c;
}
// the query tile: the forced one (or none), else the smallest that covers m, else the largest
constexpr int pick_tile(const DimTiles* t, size_t m, long forced_tq) {
	int best = 0;
	for (int i = 0; t && t->tq[i]; ++i) {
		const int tq = t->tq[i];
		if (forced_tq > 0) {
			if (tq == forced_tq)
				return tq;
			continue;
		}
		const bool covers = (size_t)tq >= m, b_covers = (size_t)best >= m;
		if (!best || (covers && (!b_covers || tq < best)) || (!covers && !b_covers && tq > best))
			best = tq;
	}
	return best;
}

constexpr bool any_dim_f32(int d) { return d >= 16 && d <= kPlanMaxDim && d % 16 == 0; }
// 8-bit rows (not int16) of a dim without a compiled instance
constexpr bool any_dim_i8(int d, int mode) {
	return mode >= 0 && mode != kPlanI16L2Ref && d >= 64 && d <= kPlanMaxDim && d % 64 == 0 && !tiles_of(kScanI8Tiles, d);
}

enum class ScanFamily : int {
	kDirect,   // the exact VALU scan (scan_f32.hpp / scan_int8.hpp and their run-time-dim forms)
	kF16X,     // fp16 single-product forms, by geometry: d = 64 / 128,
	kF16Y,     //   256 / 512,
	kF16KX,    //   768 / 832 / 960,
	kF16KL,    //   every other multiple of 16 from 64 up (dim known at run time),
	kF16Dbg,   //   and d = 128 under a "debug" value
	kBf16x3,   // fp32 L2 rows, d = 64 / 128
	kGemmI8,   // 8-bit rows on the int8 matrix cores, threshold ladder
	kI8qW,     // 8-bit rows, per-wave hit queues, by geometry: d = 128 / 256,
	kI8qX,     //   768 / 832 / 896 / 960,
	kI8qKL     //   every other multiple of 64
};
constexpr bool is_f16(ScanFamily f) { return f >= ScanFamily::kF16X && f <= ScanFamily::kF16Dbg; }

// the fp16 form of a dim (kDirect: none).  The index's fp16 copy has rows of whole 32-element k-steps for kF16KL.
constexpr ScanFamily f16_geometry(int d) {
	if (has_dim(kF16XDims, d))
		return ScanFamily::kF16X;
	if (has_dim(kF16YDims, d))
		return ScanFamily::kF16Y;
	if (has_dim(kF16KXDims, d))
		return ScanFamily::kF16KX;
	return d >= 64 && any_dim_f32(d) ? ScanFamily::kF16KL : ScanFamily::kDirect;
}
constexpr bool f16kl_dim(int d) { return f16_geometry(d) == ScanFamily::kF16KL; }

struct PlanIndex {
	int dtype = EXPANN_DTYPE_F32, int_mode = -1, metric = EXPANN_METRIC_L2, dim = 0;
	size_t n = 0;
	// the options the rules read
	long scan_kernel = 0, query_tile = 0, i8_filter = 1, u8_exact_opt = 1, sample_pass = 1, spec_rank = 0, debug = 0,
	     cand_capacity = 0;
	bool f16_ok = true;   // the rows fit the fp16 range (f16_scale >= 0: not yet known counts as yes)
	int i8f_state = 0;    // int8 filter: 0 not built, 1 built, 2 built but off for auto, -1 unusable
	int u8_exact = 0;     // uint8 shadow: 0 unknown, 1 serving, -1 the rows are not 8-bit integers
	bool filter_on = false;
	size_t n_allowed = 0;
};
struct PlanCall {
	size_t m = 0, k = 0;
	uint32_t cap = 0;  // the candidate lists' capacity the attempt starts with
};
// what a search learned between attempts
struct PlanAttempt {
	bool force_direct = false;  // a matrix-core filter overflowed at every capacity: massive near-ties
	bool no_f16 = false;        // the queries, or the rows, do not fit the fp16 range
	bool i8f_off = false;       // the int8 filter's lists overflowed
	bool spec_off = false;      // an attempt's failing queries did not fit the redo pass
};
struct ScanPlan {
	int status = EXPANN_OK;        // a refusal: its code ...
	const char* message = "";      // ... and text
	ScanFamily family = ScanFamily::kDirect;  // what SearchPass runs
	bool i8q = false;              // 8-bit rows: `i8q_family` tries first and hands back to `family` when its lists overflow
	ScanFamily i8q_family = ScanFamily::kDirect;
	bool u8_shadow = false;        // fp32 rows: the uint8 shadow may answer (if the rows and queries are 8-bit integers)
	int direct_tq = 0;             // the direct scan's query tile (0: no instance -- an unsupported dim / "query_tile")
	int direct_f16_tq = 0;         // fp16 form: scan_direct_f16 with this tile serves the last level and the sampled pass (0: MFMA)
	bool i8f = false;              // fp16 form: the int8 filter runs the full scan
	uint32_t i8f_min_cap = 0;      //   ... with lists of this many keys at least
	bool speculate = false;        // the attempt may filter with a speculative threshold
	bool sampled = false;          // direct / fp16 form: one sampled pass replaces the threshold ladder's first levels
	bool tie_fallback = false;     // lists that overflow at every capacity restart on the direct scan (force_direct)

	bool float_gemm() const { return is_f16(family) || family == ScanFamily::kBf16x3; }
};

// The int8 filter's auto region, from the A/B sweep of the two forms over n = 0.5 / 0.75 / 1 / 2 M rows, m = 2 048 /
// 4 096 / 10 000 queries, k = 1 / 10 / 16 / 32 on iid rows (profiles/r06_i8f_sweep.json): every measured point inside
// is faster by 4.8 % or more; k = 32 lost everywhere (up to -58 %), k = 10 at 500 k rows and at 1 M rows x 2 048
// queries lost.  Shapes between the grid points take the nearest grid point below them in n and m, above them in k.
constexpr bool i8f_auto_region(size_t n, size_t m, size_t k) {
	if (k <= 1)
		return n >= 500000 && m >= 2048;  // (+13 % .. +41 %)
	if (k <= 10)
		return (n >= 1000000 && m >= 4096) || (n >= 2000000 && m >= 2048);  // (+10 % .. +27 %)
	if (k <= 16)
		return (n >= 2000000 && m >= 2048) || (n >= 1000000 && m >= 10000);  // (+4.8 % .. +20 %)
	return false;
}
// Where the auto rank speculates ("spec_rank" 0), from the A/B against proven thresholds over bench.py's shapes
// (profiles/r07_spec_tau_ab.txt): the shorter lists have to pay for the redo pass, four launches that cost ~20 us when
// no query failed and ~100 us when some did.  They do where the lists are long: the int8 filter's (C2: 501 -> 215 per
// query, -11 % per step) and the fp16 form's at large k (1.25 M rows, k = 100: 703 -> 183, -5.1 %).  The fp16 form at
// k = 10 loses ~1 %, so does any form at 1 000 queries.  Shapes between the measured ones keep proven thresholds.
constexpr bool spec_auto_region(size_t m, size_t k, bool i8f) { return m >= 4096 && (i8f || k > 32); }

// the candidate lists' starting capacity: "cand_capacity" or 64 k, a power of two in [2 048 (auto), kMaxCap], never below
// 2 k where that fits (the caller refuses a k for which it does not)
constexpr uint32_t pow2ceil(uint32_t x) {
	uint32_t p = 1;
	while (p < x)
		p <<= 1;
	return p;
}
constexpr uint32_t plan_start_cap(long cand_capacity, size_t k, uint32_t max_cap) {
	const size_t want = 64 * k > 2048 ? 64 * k : 2048;
	uint32_t cap = cand_capacity > 0 ? (uint32_t)cand_capacity : pow2ceil((uint32_t)want);
	cap = pow2ceil(cap) < max_cap ? pow2ceil(cap) : max_cap;
	if (cand_capacity > 0 && (size_t)cap < 2 * k)
		cap = pow2ceil((uint32_t)(2 * k)) < max_cap ? pow2ceil((uint32_t)(2 * k)) : max_cap;
	return cap;
}

constexpr const char* kRefuseGemm =
    "GEMM-form scan (scan_kernel=2): 8-bit L2/IP with dim 128/256/768 (the fp32-input MFMA form of "
    "rounds 1-2 is gone: scan_kernel 3 = bf16x3, 4 = fp16)";
constexpr const char* kRefuseBf16 = "bf16x3 GEMM-form scan: f32 L2 with dim 64 or 128 only";
constexpr const char* kRefuseF16 = "fp16 GEMM-form scan: f32 with dim a multiple of 16 from 64 to 4096 only";

// the direct scan's query tile for m queries (0: none)
constexpr int direct_tile(const PlanIndex& x, size_t m) {
	if (x.int_mode < 0) {
		const DimTiles* t = x.dtype == EXPANN_DTYPE_F16 ? nullptr : tiles_of(kScanF32Tiles, x.dim);
		if (!t && !any_dim_f32(x.dim))
			return 0;
		return pick_tile(t ? t : &kScanF32AnyTiles, m, x.query_tile);
	}
	if (any_dim_i8(x.dim, x.int_mode))
		return pick_tile(&kScanI8AnyTiles, m, x.query_tile);
	return pick_tile(x.int_mode == kPlanI16L2Ref ? tiles_of(kScanI16Tiles, x.dim) : tiles_of(kScanI8Tiles, x.dim), m,
	                 x.query_tile);
}
// scan_direct_f16's tile for m queries: ONE pass (measured at 1 M x d128: a second pass, or 8 queries per pass --
// VALU-bound --, loses to the MFMA form), else 0
constexpr int direct_f16_tile(int d, size_t m) {
	const int tq = pick_tile(tiles_of(kDirectF16Tiles, d), m, 0);
	return (size_t)tq >= m ? tq : 0;
}

// Float rows on the matrix cores at all?  Measured crossovers at N = 1 M, d = 128.  bf16x3: m = 16: 0.34 vs 0.37 ms
// per step, m = 32: 0.49 vs 0.41 ms -- below ~24 queries the HBM-bound direct scan wins.  fp16 form (half the bytes
// per row, one sampled pass): 0.175 vs 0.175 ms at m = 4, 0.173 vs 0.199 at m = 8, 0.185 vs 0.31 at m = 16 -- from 5
// queries on it wins, and below where scan_direct_f16 streams the copy.  Under 4 096 rows nothing beats the direct scan.
constexpr bool float_gemm_wanted(const PlanIndex& x, size_t m) {
	const long sk = x.scan_kernel;
	const bool f16_choice = sk == 0 || sk == 4 || sk == 6;
	const bool f16_dim = f16_geometry(x.dim) != ScanFamily::kDirect;
	if (sk == 1 || x.int_mode >= 0)
		return false;
	if (x.dtype == EXPANN_DTYPE_F16 && !f16_choice)  // (binary16 rows: the fp16 form is the only matrix-core one)
		return false;
	const bool f16_serves = f16_dim && x.f16_ok && (f16_choice || x.metric != EXPANN_METRIC_IP);
	const size_t m_min = (x.metric == EXPANN_METRIC_IP || f16_serves) ? 5 : 24;
	const bool few = m < m_min && !(f16_serves && direct_f16_tile(x.dim, m));
	if (x.metric == EXPANN_METRIC_IP)  // inner product: only the fp16 form has it
		return f16_choice && x.f16_ok && f16_dim && !(sk == 0 && (few || x.n < 4096));
	if (sk == 0 && (few || x.n < 4096))
		return false;
	return has_dim(kBf16Dims, x.dim) || (f16_choice && f16_dim);
}

inline ScanPlan plan_scan(const PlanIndex& x, const PlanCall& c, const PlanAttempt& a) {
	ScanPlan p;
	const long sk = x.scan_kernel;
	const bool flt = x.int_mode < 0, f32 = x.dtype == EXPANN_DTYPE_F32, l2 = x.metric == EXPANN_METRIC_L2;
	const bool f16_choice = sk == 0 || sk == 4 || sk == 6;
	const bool dbg = (x.debug & ~16L) != 0;  // (bit 4 only prints the scan's clocks)
	const bool filt = x.filter_on;
	const bool mfma_mode = x.int_mode == kPlanU8L2 || x.int_mode == kPlanI8L2 || x.int_mode == kPlanI8IP;
	p.direct_tq = direct_tile(x, c.m);
	p.direct_f16_tq = sk == 0 ? direct_f16_tile(x.dim, c.m) : 0;

	// fp32 L2 rows that are all integers in [0, 255] (SIFT): with integer queries the uint8 engine's exact integer scores
	// ARE the fp32 scores, at the 8-bit kernels' speed (a second handle that knows nothing of a row filter)
	p.u8_shadow = f32 && l2 && sk == 0 && x.u8_exact_opt && !filt && (x.dim == 128 || x.dim == 256) && c.m >= 96 &&
	              x.n >= 65536 && c.k <= 256 && x.u8_exact >= 0;
	// 8-bit rows, from 96 queries x 65 536 rows on ("scan_kernel" 5: wherever the logs fit), k <= 256
	if (!flt && mfma_mode && (sk == 5 || (sk == 0 && c.m >= 96 && x.n >= 65536)) && x.n >= kI8MinRows && c.k <= 256) {
		p.i8q = true;
		if (has_dim(kI8qWDims, x.dim))
			p.i8q_family = ScanFamily::kI8qW;
		else if (has_dim(kI8qXDims, x.dim))
			p.i8q_family = ScanFamily::kI8qX;
		else if (any_dim_i8(x.dim, x.int_mode))
			p.i8q_family = ScanFamily::kI8qKL;
		else
			p.i8q = false;
	}

	// A row filter reaches the matrix cores through the fp16 forms' masked row terms only: no bf16x3 form (queries
	// outside the fp16 range go to the exact direct scan), no int8 filter, no speculative thresholds, whatever the
	// options say; a filter selective enough for the list path streams no base at all.  Binary16 rows have neither a
	// bf16x3 form nor an int8 filter -- both build their operands from fp32 storage.
	bool gemm = !a.force_direct && float_gemm_wanted(x, c.m);
	if (filt && (a.no_f16 || !f16_choice || x.n_allowed <= c.cap))
		gemm = false;
	const bool gemm_i8 = !a.force_direct && !flt && sk != 1 && !(sk == 0 && (c.m < 96 || x.n < 4096)) && mfma_mode &&
	                     has_dim(kGemmI8Dims, x.dim);
	if (gemm_i8)
		p.family = ScanFamily::kGemmI8;
	if (sk == 2 && !gemm_i8) {
		p.status = EXPANN_ERR_UNSUPPORTED;
		p.message = kRefuseGemm;
		return p;
	}
	const bool bf16 = gemm && f32 && l2 && has_dim(kBf16Dims, x.dim);  // (the inner product has the fp16 form alone)
	if (sk == 3 && !bf16 && !filt && x.dtype != EXPANN_DTYPE_F16) {
		p.status = EXPANN_ERR_UNSUPPORTED;
		p.message = kRefuseBf16;
		return p;
	}
	// the fp16 single-product form: the default where there is one; a search whose queries leave the fp16 range after
	// scaling is redone without it (no_f16)
	ScanFamily f16 = ScanFamily::kDirect;
	if (gemm && !a.no_f16 && f16_choice)
		f16 = (dbg && x.dim == kF16DbgDim) ? ScanFamily::kF16Dbg : f16_geometry(x.dim);
	const bool has_f16 = f16 != ScanFamily::kDirect;
	if ((sk == 4 || sk == 6) && !has_f16 && !a.no_f16 && !(filt && x.n_allowed <= c.cap)) {
		p.status = EXPANN_ERR_UNSUPPORTED;
		p.message = kRefuseF16;
		return p;
	}
	if (has_f16)
		p.family = f16;
	else if (bf16 && !(sk == 0 && c.m < 24))  // (bf16x3 pays from ~24 queries on; under a row filter `gemm` needs the fp16 form)
		p.family = ScanFamily::kBf16x3;
	p.tie_fallback = p.family != ScanFamily::kDirect && sk == 0;
	p.sampled = x.sample_pass && (has_f16 || (p.family == ScanFamily::kDirect && !filt));

	// The int8 filter for fp32 rows: L2, d = 128, the uint8 shadow not serving the index, no debug instance,
	// "scan_kernel" on auto; "i8_filter" 2 wherever that holds, 1 (auto) inside the measured region
	p.i8f = has_f16 && !a.i8f_off && !filt && x.i8_filter != 0 && sk == 0 && f32 && l2 && x.dim == kI8fDim && x.u8_exact != 1 &&
	        !dbg && x.i8f_state >= 0 && c.k <= 256 && x.n >= kI8MinRows &&
	        (x.i8_filter == 2 || (x.i8f_state != 2 && i8f_auto_region(x.n, c.m, c.k)));
	// (room for the lists of queries with a clipped component)
	p.i8f_min_cap = (p.i8f && x.cand_capacity <= 0) ? 4096 : 0;
	// speculation: the scan_gemm_f16x / i8w streams -- the forms that have a redo pass --, batches beyond
	// the latency mode's, no debug instance
	p.speculate = p.family == ScanFamily::kF16X && !dbg && c.m > 64 && !a.spec_off && !filt && x.spec_rank >= 0 &&
	              (x.spec_rank > 0 || spec_auto_region(c.m, c.k, p.i8f));
	return p;
}

// the fp16 copy is made at build time where an auto search of many queries would filter through it
inline bool f16_copy_at_build(const PlanIndex& x) {
	return x.scan_kernel == 0 && is_f16(plan_scan(x, PlanCall{4096, 1, 0}, PlanAttempt{}).family);
}

}  // namespace expann
