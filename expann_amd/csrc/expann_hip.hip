// expann_hip.hip -- the C ABI (include/expann_hip.h) over the gfx950 kernels.
//
// Host side of the hot path: owns device memory, plans the threshold levels, launches the
// scan / select / merge kernels on HIP streams.  No CPU fallback lives here: every compute
// entry point needs a HIP device and fails loudly without one.
#include "../../include/expann_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "bf_append.hpp"
#include "bf_remove.hpp"
#include "bf_options.hpp"
#include "bf_plan.hpp"
#include "host_common.hpp"
#include "scan_f32.hpp"
#include "scan_gemm_bf16.hpp"
#include "scan_gemm_f16.hpp"
#include "scan_gemm_f16x.hpp"
#include "scan_gemm_f16kx.hpp"
#include "scan_direct_f16.hpp"
#include "scan_gemm_i8.hpp"
#include "scan_gemm_i8q.hpp"
#include "scan_gemm_i8w.hpp"
#include "scan_redo_i8.hpp"
#include "scan_gemm_w8.hpp"
#include "scan_gemm_kl.hpp"
#include "scan_int8.hpp"
#include "scan_int8_any.hpp"
#include "filter_rows.hpp"
#include "scan_groups.hpp"
#include "append_rows.hpp"
#include "remove_rows.hpp"
#include "score_ids.hpp"
#include "select.hpp"
#include "select_range.hpp"

using namespace expann;

namespace expann {
thread_local std::string g_create_error;
}

namespace {

// (kMaxCap, the keys per query that fit the select kernel's LDS: bf_options.hpp, where an option's bound names it)
static_assert(kMaxK == kMaxCap / 2, "the bound on k: a candidate list holds at least 2k keys");
constexpr size_t kMaxQueriesPerPass = 32768;
constexpr int kEventPairs = 64;
constexpr uint32_t kAsyncRing = 256;  // outstanding searches of the deferred-check mode
// a ring slot: words 0-6 = the device's flag block (kFlagCopyBytes of it), words 8 / 9 the host's (defer_flags)
constexpr uint32_t kRingWords = 10, kRingScale = 8, kRingMark = 9;
// what a search reads back: flags (words 0-3), the candidate total (4-5), the redo lists' keys (6)
constexpr size_t kFlagCopyBytes = sizeof(uint32_t) * 7;
constexpr uint32_t kFilterListCap = kMaxCap;  // rows in the row filter's list (the longest candidate list)

struct Level {
	uint32_t n_groups_sel;
	uint32_t group_stride;
	uint32_t classmin_blocks = 0;  // > 0: level 0 keeps class minima (scan_f32.hpp), this many workgroups
	uint32_t list_rows = 0;        // > 0 (row filter, level 0): the keys of this many rows of the filter's list ...
	uint32_t list_step = 1;        // ... every list_step-th entry
};

}  // namespace

// The handle's state, grouped by who makes it and when it dies: each group is a base of expann_index (use sites
// read h->d_base_f16), and a group is forgotten as a value -- h->forget<RowCopies>() frees and resets every member
// it has, so a member added to a group needs no edit anywhere else.

// what expann_create fixes, and the options (bf_options.hpp)
struct Config : Options {
	int dim = 0, dtype = 0, metric = 0, device = 0;
	size_t elem = 4;    // bytes per stored element
	size_t q_elem = 4;  // bytes per query element at the ABI (f32 for F32/U8 rows, int8 for I8)
	int int_mode = -1;  // IntMode for 8-bit rows
	bool strict_u8 = false;          // (on the shadow) non-8-bit / fractional queries: hand back, no error
};

// the rows: staged on the host until build(), then on the device -- the handle's own copy, or the caller's memory
// (expann_set_base_device)
struct Rows {
	std::vector<unsigned char> staging;  // store_vector() rows until build()
	size_t n_staged = 0;
	MaybeOwnedPtr d_base;
	size_t n = 0;
	size_t capacity = 0;  // rows the handle's own allocation holds (>= n: expann_reserve, expann_append); 0 for the caller's memory
	size_t reserved = 0;  // expann_reserve before build(): expann_build allocates max(staged, reserved) rows
	uint64_t id_offset = 0;
};

struct HandleDeleter {
	void operator()(expann_index* h) const { expann_destroy(h); }
};
// fp32 index whose values are all integers in [0, 255] (SIFT): searches with integer queries
// go through an internal uint8 engine -- exact integer scores, equal to the fp32 ones bit for
// bit while d * 255^2 < 2^24 -- at the 8-bit kernels' speed
struct U8Shadow {
	int u8_exact = 0;                // 0 not examined, 1 yes (shadow built), -1 no
	DevPtr<void> d_base_u8;
	std::unique_ptr<expann_index, HandleDeleter> u8_shadow;  // (reads d_base_u8: declared after it, so it goes first)
};

// The fp16 copy every fp32 / fp16 search filters through, built lazily: the one derived copy an append extends in
// place (expann_append), so it is a group of its own.  Allocated for the base's capacity in whole tiles and
// initialised as a whole (zero rows, NaN terms); the scans read [0, f16_n_pad) and nothing behind it.
struct F16Copy {
	// [2]: max ||b||^2 of the rows.  Slot [1] is the bf16x3 form's (max of d_bnorm_bf, OtherCopies), written whenever
	// d_bnorm_bf is made.  INVARIANT: F16Copy is never forgotten while OtherCopies lives -- forget<F16Copy>() always
	// follows forget<OtherCopies>() (or both go as RowCopies) --, so slot [1] never dies under a live d_bnorm_bf; the
	// other way round is fine, ensure_bnorm_bf16 writes [1] again.
	DevPtr<float> d_bnmax;
	DevPtr<void> d_base_f16;         // [f16_rows_alloc][f16_ld] fp16 rows scaled by f16_scale (fp16 GEMM form)
	DevPtr<float> d_bnorm_f16;       // [f16_rows_alloc] ||b||^2 (1-eps) - abs |b|
	DevPtr<float> d_bns_f16;         // [f16_rows_alloc] ||b||^2 (1+eps) + abs |b|: the sampled pass's row term
	float f16_scale = 0.0f;          // power of two (bf_append.hpp: f16_scale_for); 0 = not built, < 0 = the rows do not fit
	float f16_maxabs = 0.0f;         // max |v| of the rows the copy holds: what the scale was chosen for
	size_t f16_n_pad = 0;            // rows the scans read: n in whole tiles
	size_t f16_tb = 0;               // ... of this many rows
	size_t f16_rows_alloc = 0;       // rows allocated: the base's capacity in whole tiles
};
// every other copy and term derived from the rows, built lazily, dead when the rows change -- an append included
struct OtherCopies : U8Shadow {
	DevPtr<float> d_bnorm_bf;        // ||b||^2 (1-eps) per row with the bf16x3 slack, built lazily
	DevPtr<void> d_base_split;       // [n][2][dim] bf16 hi/lo planes (bf16x3 GEMM form), lazily
	// int8 filter of fp32 rows (scan_gemm_i8f.hpp), built lazily beside the fp16 copy (whose sampled pass
	// gives its thresholds) and dropped with it
	DevPtr<void> d_base_i8f;         // [n padded to 64][dim] int8
	DevPtr<int> d_bp_i8f;            // [n padded] integer row terms; kI8qPadBp on the padding
	DevPtr<float> d_rw_i8f;          // [n] w_b (select pruning), +inf where bp was clamped
	DevPtr<int> d_cb_i8f;            // [n padded] centre row terms of the int8 sampled pass; kI8fCbNone: no such row
	DevPtr<float> d_wbmax_i8f;       // [1] the largest w_b among the rows with a centre term
	I8fConsts i8f{};
	int i8f_state = 0;               // 0 not built, 1 built, 2 built but off for auto (lists too long), -1 unusable
	DevPtr<int> d_bias_i;            // [n] sum b^2 per row (8-bit L2 GEMM form), built lazily
	MaybeOwnedPtr d_base_i8q;        // padded int8 copy of an 8-bit index (uint8 rows ^ 0x80) or alias of d_base
	DevPtr<int> d_bp_i8q;            // [n padded] floor(bias/2), scan_gemm_i8q.hpp
};
// all that is derived from the rows: forgotten together when the rows are replaced
struct RowCopies : F16Copy, OtherCopies {};

// row filter (expann_set_row_filter): the engine's copy of the bitmap, the allowed rows'
// count, an ascending list of them (complete up to kFilterListCap rows, an even sample beyond) and the masked
// copies of the fp16 forms' row terms (NaN on every disallowed row), made lazily after ensure_f16
struct RowFilter {
	bool filter_on = false;
	DevPtr<uint32_t> d_filter_bits;  // [filter_words]: whole 128-row tiles, zero from row n on
	size_t filter_words = 0;
	DevPtr<uint32_t> d_filter_stat;  // [2 + kFilterSegs]: count, OR of the words, per-segment counts
	DevPtr<uint32_t> d_filter_list;  // [kFilterListCap]
	uint32_t filter_list_len = 0, filter_list_stride = 1;
	size_t n_allowed = 0;
	uint32_t filter_residues = 0;    // bit r: some allowed row has row % 32 == r
	DevPtr<float> d_bnorm_f16_m;     // [f16_n_pad] d_bnorm_f16 under the filter
	DevPtr<float> d_bns_f16_m;       // [f16_n_pad] d_bns_f16 under the filter
	bool filter_terms_valid = false;
};

// row groups (expann_set_row_groups): the labels and each group's rows on the device, the
// directory's labels and offsets on the host, where a grouped search is planned; and that search's staging
struct RowGroups {
	bool groups_on = false;
	DevPtr<uint32_t> d_row_groups;   // [n]
	DevPtr<uint32_t> d_group_rows;   // [rows that carry a label other than 0xFFFFFFFF], by (label, row)
	GroupDirectory group_dir;        // keys and off (the rows live in d_group_rows)
	PinPtr<void> h_group_tab;        // pinned: [sorted query numbers | list slots' queries | work items]
	size_t h_group_tab_bytes = 0;
	GrowPtr<void> d_group_tab;
	GrowPtr<void> d_group_q;         // gathered queries of one tier
	GrowPtr<uint64_t> d_group_ids;   // ... and their result rows
	GrowPtr<float> d_group_dists;
};

// per-search workspace (grown on demand); survives a change of rows
struct Workspace {
	GrowPtr<uint8_t> d_q8;  // U8 rows: queries truncated to uint8
	GrowPtr<uint64_t> d_cand;
	DevPtr<uint32_t> d_cnt;          // [m_alloc]
	DevPtr<float> d_tau[2];
	DevPtr<float> d_tau_s;           // [m_alloc] speculative thresholds of the sampled pass, true units
	GrowPtr<void> d_redo;            // the redo pass's workspace: failing queries, their compact operands, their lists
	GrowPtr<void> d_rerank;          // "rerank_stats": [sum (8 bytes, 8 unused) | rows re-scored per query [m]]
	DevPtr<uint32_t> d_tau_row[2];
	size_t m_alloc = 0;
	DevPtr<uint32_t> d_overflow;     // [4]: overflow count
	unsigned long long* d_total = nullptr;  // (inside d_overflow's block)
	PinPtr<uint32_t> h_flags;        // pinned [4]
	// latency mode (expann_search with few queries): pinned staging [queries | ids | dists]; the
	// select kernels store the results straight into it, so a search costs one async H2D copy of
	// the queries, the kernels, and the flag read-back -- one host sync, no pageable copies
	PinPtr<void> h_pin;
	bool q_in_pinned_host = false;  // (expann_search -> search_pass: d_queries is pinned host memory)
	DevPtr<uint32_t> d_ticket;  // last-workgroup counter of sample_direct_f16_kernel (0 between launches)
	size_t h_pin_bytes = 0;
	DevPtr<void> d_log;              // per-wave hit logs of scan_gemm_f16x ([n_logs][log_cap] x 16 B)
	DevPtr<uint32_t> d_log_cnt;      // [n_logs]
	DevPtr<uint32_t> d_work_ctr;     // [8][16]: per-XCD item counters of the persistent scan launch
	size_t log_bytes = 0, log_cnt_n = 0;
	struct {                         // scatter_log_kernel of the scan just launched (run after its timing event)
		uint32_t n_logs = 0, log_cap = 0, cap = 0, n_chunks = 0, n_qtiles = 0, xcd_map = 0, m = 0;
		const float* theta = nullptr;  // fp16 logs: entries hold bn' - acc, the gather adds theta' and scales (GatherLogParams)
		float key_mul = 0.0f;
		const int *i_thp = nullptr, *i_bias = nullptr, *i_qself = nullptr;  // 8-bit logs: raw accumulators, scored by the gather
		int i_mode = 0;
		const float* i_rw = nullptr;  // (i_mode 3: the int8 filter of fp32 rows)
	} pending_scatter;
	GrowPtr<float> d_sample;         // [m][n_chunks][32] class maxima of the fp16 / int8 sample pass
	GrowPtr<void> d_q_split;         // [m][2][dim] bf16 (or [m][dim] fp16)
	DevPtr<float> d_qnrm;            // [m_alloc] ||q||^2 (fp16 form, inner product: of the filter-side query c_q q)
	DevPtr<float> d_qscale;          // [m_alloc] c_q: the power of two the fp16 filter sees a query multiplied by (inner product; L2: 1)
	DevPtr<float> d_i8f_q;           // [3][m_alloc]: A_q, W_q (prelude), w_q (thresholds)
	GrowPtr<void> d_q8f;             // [m][dim] int8 queries
	size_t i8f_q_m = 0;
	DevPtr<float> d_theta;           // [m_alloc] (int32 thetas for the 8-bit GEMM form)
	DevPtr<int> d_qself;             // [m_alloc]
	GrowPtr<void> d_q;               // host-API staging
	GrowPtr<uint64_t> d_ids;
	GrowPtr<float> d_dists;
	// deferred check (expann_sync): flag blocks of the outstanding searches, read back into a ring
	bool host_call = false;          // (expann_search: always the synchronous path)
	PinPtr<uint32_t> h_flag_ring;    // pinned [kAsyncRing][kRingWords]
	uint32_t async_pending = 0;
	bool group_lds_set = false;      // the grouped search's list kernel has its LDS limit raised (dims whose query tile exceeds 64 KiB)
	// range search (RangePass): [the three lists' lengths, 0 | queries stage 1's lists could not hold [m] | ... nor the
	// fp16 form's at kMaxCap keys [m] | queries with more than kMaxCap rows in range [m]], the gathered queries of
	// stages 2 / 3, stage 3's result rows, and the host-buffer call's radii and counts
	GrowPtr<uint32_t> d_range;
	GrowPtr<void> d_range_q;
	GrowPtr<uint64_t> d_range_ids;
	GrowPtr<float> d_range_dists;
	GrowPtr<float> d_range_radii;
	GrowPtr<uint32_t> d_range_counts;
	bool range_lds_set = false;      // the range select's 1 024-thread instances have their LDS limit raised
	DevPtr<uint32_t> d_append_flag;  // [4]: [0] bit pattern of max |v| of an append's rows; [2..3] the 64-bit "copies_digest"
};

// the counters expann_get_stat reads (kStatTable)
struct Stats {
	uint64_t stat_redo_queries = 0;  // queries the redo pass served in the last search (waiting form) / the last synced one
	uint64_t stat_redo_candidates = 0;  // keys the redo lists of those queries held (the redo select counts them)
	uint64_t stat_rerank_rows = 0;   // rows the last search's selects re-scored exactly (opt_rerank_stats)
	uint64_t stat_redo_overflows = 0;  // searches whose failing queries (or redo lists) did not fit the redo pass
	uint64_t stat_spec_rank = 0;     // j of the last search's thresholds (= k: proven thresholds)
	uint64_t stat_i8_sample = 0;     // 1: the last search's sampled pass ran on int8
	uint64_t stat_group[5] = {0, 0, 0, 0, 0};  // the last grouped search: list, filter, any, pad queries; filter passes
	uint64_t stat_range[3] = {0, 0, 0};  // the last range search: queries answered from a list, by the top-k pipeline; stage-1 retries
	// expann_append since create: calls, rows, appends that extended the fp16 copy in place, appends that had to drop
	// it (the scale changed), and reallocations of the base (expann_reserve's included)
	uint64_t stat_append[5] = {0, 0, 0, 0, 0};
	// expann_remove / expann_compact_row_filter since create: accepted calls, rows removed, removes that carried the
	// fp16 copy over, removes that dropped it or forgot an unusable mark
	uint64_t stat_remove[4] = {0, 0, 0, 0};
};

// streams, events, profiling, statistics, the last error
struct Runtime : Stats {
	OwnedStream stream;
	hipStream_t async_stream = nullptr;  // the stream of the outstanding deferred searches (the caller's, or `stream`)
	// the side stream of the select's long-list stages (launch_select_wave), and the events of its fork and join;
	// made at the first search that has such a stage
	OwnedStream side_stream;
	OwnedEvent side_ev[2];
	bool profiling = false;
	OwnedEvent ev[kEventPairs][2];
	bool ev_created = false;
	int ev_used = 0;
	expann_profile prof{};
	double prof_extra_ms = 0;        // scan time absorbed from the shadow
	mutable std::string err;
};

// (base order: the streams and events outlive every buffer when a handle is deleted)
struct expann_index : Config, Runtime, Workspace, Rows, RowCopies, RowFilter, RowGroups {
	// the row terms the fp16 forms read: the masked copies while a filter is set
	const float* bnorm_f16() const { return filter_on ? d_bnorm_f16_m.p : d_bnorm_f16.p; }
	const float* bns_f16() const { return filter_on ? d_bns_f16_m.p : d_bns_f16.p; }
	template <typename Group> void forget() { static_cast<Group&>(*this) = Group{}; }

	int fail(int code, const std::string& msg) const {
		err = msg;
		return code;
	}
};

// rows of floating-point values scored in fp32 by the reference's lane order: fp32 storage, or binary16 storage
// (EXPANN_DTYPE_F16: every exact kernel converts on load, every filter is built from the converted values, so an
// F16 index answers as the F32 index of the upcast rows does).  `dtype == EXPANN_DTYPE_F32` stays where fp32
// STORAGE is meant: the uint8 shadow, the int8 filter and the bf16x3 planes read d_base as float.
inline bool f16_rows(const expann_index* h) { return h->dtype == EXPANN_DTYPE_F16; }
inline bool float_rows(const expann_index* h) { return h->dtype == EXPANN_DTYPE_F32 || f16_rows(h); }

namespace expann {
int num_cus(int device) {
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess)
		return 256;
	return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
}
}  // namespace expann

namespace {

// ---- kernel dispatch ---------------------------------------------------------------
using ScanFn = void (*)(ScanParams);
struct ScanVariant {
	int d, tq;
	bool ip;
	ScanFn fn;
	const char* name;
	ScanFn fn_bits = nullptr;  // the instance that reads the row filter's bitmap (kRowsBitmap)
	ScanFn fn_list = nullptr;  // the instance that walks a list of rows (kRowsList)
};
#define SCAN_V(D, TQ)                                                                      \
	{D, TQ, false, scan_filter_f32_kernel<D, TQ, false>, "scan_filter_f32<" #D "," #TQ ",L2>", \
	 scan_filter_f32_kernel<D, TQ, false, kRowsBitmap>, scan_filter_f32_kernel<D, TQ, false, kRowsList>}, \
	{D, TQ, true, scan_filter_f32_kernel<D, TQ, true>, "scan_filter_f32<" #D "," #TQ ",IP>", \
	 scan_filter_f32_kernel<D, TQ, true, kRowsBitmap>, scan_filter_f32_kernel<D, TQ, true, kRowsList>}
const ScanVariant kScanF32[] = {
    SCAN_V(64, 1),  SCAN_V(64, 4),  SCAN_V(64, 16), SCAN_V(128, 1), SCAN_V(128, 2),
    SCAN_V(128, 4), SCAN_V(128, 8), SCAN_V(128, 16), SCAN_V(256, 1), SCAN_V(256, 4),
    SCAN_V(256, 8), SCAN_V(512, 1), SCAN_V(512, 4),  SCAN_V(768, 1), SCAN_V(768, 2),
    SCAN_V(832, 1), SCAN_V(832, 2), SCAN_V(960, 1),  SCAN_V(960, 2), SCAN_V(1024, 1),
    SCAN_V(1024, 2)};
#undef SCAN_V
// every other f32 dim (multiples of 16 up to kMaxAnyDim): the run-time-dim scan (d = 0 in the table)
#define SCAN_ANY_V(TQ)                                                                           \
	{0, TQ, false, scan_filter_f32_any_kernel<TQ, false>, "scan_filter_f32_any<" #TQ ",L2>",   \
	 scan_filter_f32_any_kernel<TQ, false, kRowsBitmap>, scan_filter_f32_any_kernel<TQ, false, kRowsList>}, \
	{0, TQ, true, scan_filter_f32_any_kernel<TQ, true>, "scan_filter_f32_any<" #TQ ",IP>",     \
	 scan_filter_f32_any_kernel<TQ, true, kRowsBitmap>, scan_filter_f32_any_kernel<TQ, true, kRowsList>}
const ScanVariant kScanF32Any[] = {SCAN_ANY_V(1), SCAN_ANY_V(2), SCAN_ANY_V(4)};
#undef SCAN_ANY_V
// binary16 rows (EXPANN_DTYPE_F16), every dim: the run-time-dim scan over _Float16 rows
#define SCAN_ANY_H(TQ)                                                                                              \
	{0, TQ, false, scan_filter_f32_any_kernel<TQ, false, kRowsAll, _Float16>, "scan_filter_f32_any<" #TQ ",L2,F16>", \
	 scan_filter_f32_any_kernel<TQ, false, kRowsBitmap, _Float16>, scan_filter_f32_any_kernel<TQ, false, kRowsList, _Float16>}, \
	{0, TQ, true, scan_filter_f32_any_kernel<TQ, true, kRowsAll, _Float16>, "scan_filter_f32_any<" #TQ ",IP,F16>", \
	 scan_filter_f32_any_kernel<TQ, true, kRowsBitmap, _Float16>, scan_filter_f32_any_kernel<TQ, true, kRowsList, _Float16>}
const ScanVariant kScanF16Any[] = {SCAN_ANY_H(1), SCAN_ANY_H(2), SCAN_ANY_H(4)};
#undef SCAN_ANY_H
static_assert(kPlanMaxDim == kMaxAnyDim, "bf_plan.hpp: the largest run-time dim");

// the instance of query tile tq (bf_plan.hpp's direct_tile) -- binary16 rows: no compiled-dim instances, the
// run-time-dim table of that element type at every dim
const ScanVariant* find_scan_f32(int d, bool ip, int tq, bool rows_f16) {
	static_assert(sizeof(kScanF16Any) == sizeof(kScanF32Any), "one F16 instance per run-time-dim F32 instance");
	const bool compiled = !rows_f16 && tiles_of(kScanF32Tiles, d);
	for (const auto& v : kScanF32)
		if (compiled && v.d == d && v.ip == ip && v.tq == tq)
			return &v;
	for (size_t i = 0; !compiled && i < sizeof(kScanF32Any) / sizeof(kScanF32Any[0]); ++i)
		if (kScanF32Any[i].ip == ip && kScanF32Any[i].tq == tq)
			return rows_f16 ? &kScanF16Any[i] : &kScanF32Any[i];
	return nullptr;
}

using ScoreFn = void (*)(ScoreIdsParams);
struct ScoreVariant {
	int d;
	bool ip;
	ScoreFn fn;
};
#define SCORE_V(D) {D, false, score_ids_f32_kernel<D, false>}, {D, true, score_ids_f32_kernel<D, true>}
const ScoreVariant kScoreF32[] = {SCORE_V(64),  SCORE_V(128), SCORE_V(256), SCORE_V(512),
                                  SCORE_V(768), SCORE_V(832), SCORE_V(960), SCORE_V(1024)};
#undef SCORE_V
const ScoreVariant kScoreF32Any[] = {{0, false, score_ids_f32_any_kernel<false>}, {0, true, score_ids_f32_any_kernel<true>}};
const ScoreVariant kScoreF16Any[] = {{0, false, score_ids_f32_any_kernel<false, _Float16>},
                                     {0, true, score_ids_f32_any_kernel<true, _Float16>}};

// 8-bit rows
struct ScanI8Variant {
	int d, tq, mode;
	ScanFn fn;
	const char* name;
};
#define SCAN_I8_M(D, TQ, MODE, MN) {D, TQ, MODE, scan_filter_i8_kernel<D, TQ, MODE>, "scan_filter_i8<" #D "," #TQ "," MN ">"}
#define SCAN_I8(D, TQ) SCAN_I8_M(D, TQ, kU8L2, "U8L2"), SCAN_I8_M(D, TQ, kI8L2, "I8L2"), \
	SCAN_I8_M(D, TQ, kI8L2Ref, "I8L2REF"), SCAN_I8_M(D, TQ, kI8IP, "I8IP")
// int16 rows: d ELEMENTS, kernels instantiated on 2 d bytes per row
#define SCAN_I16(DE, TQ) {DE, TQ, kI16L2Ref, scan_filter_i8_kernel<2 * DE, TQ, kI16L2Ref>, \
	"scan_filter_i16<" #DE "," #TQ ",L2REF>"}
const ScanI8Variant kScanI8[] = {SCAN_I8(64, 1),  SCAN_I8(64, 16), SCAN_I8(128, 1), SCAN_I8(128, 4),
                                 SCAN_I8(128, 16), SCAN_I8(256, 1), SCAN_I8(256, 8), SCAN_I8(768, 1),
                                 SCAN_I8(768, 4),  SCAN_I8(768, 8), SCAN_I8(832, 1), SCAN_I8(832, 4),
                                 SCAN_I8(960, 1),  SCAN_I8(960, 4),
                                 SCAN_I16(64, 1),  SCAN_I16(64, 4), SCAN_I16(64, 16), SCAN_I16(128, 1),
                                 SCAN_I16(128, 8)};
#undef SCAN_I16
#undef SCAN_I8
#undef SCAN_I8_M
// every other 8-bit dim (multiples of 64 up to kMaxAnyDim): the run-time-dim scan (d = 0 in the table)
#define SCAN_I8_ANY_M(TQ, MODE, MN) {0, TQ, MODE, scan_filter_i8_any_kernel<TQ, MODE>, "scan_filter_i8_any<" #TQ "," MN ">"}
#define SCAN_I8_ANY(TQ) SCAN_I8_ANY_M(TQ, kU8L2, "U8L2"), SCAN_I8_ANY_M(TQ, kI8L2, "I8L2"), \
	SCAN_I8_ANY_M(TQ, kI8L2Ref, "I8L2REF"), SCAN_I8_ANY_M(TQ, kI8IP, "I8IP")
const ScanI8Variant kScanI8Any[] = {SCAN_I8_ANY(1), SCAN_I8_ANY(4), SCAN_I8_ANY(8)};
#undef SCAN_I8_ANY
#undef SCAN_I8_ANY_M
static_assert(kU8L2 == kPlanU8L2 && kI8L2 == kPlanI8L2 && kI8L2Ref == kPlanI8L2Ref && kI8IP == kPlanI8IP &&
                  kI16L2Ref == kPlanI16L2Ref,
              "bf_plan.hpp: the 8-bit row modes");
const ScanI8Variant* find_scan_i8(int d, int mode, int tq) {
	const bool any = any_dim_i8(d, mode);
	for (const auto& v : kScanI8)
		if (!any && v.d == d && v.mode == mode && v.tq == tq)
			return &v;
	for (const auto& v : kScanI8Any)
		if (any && v.mode == mode && v.tq == tq)
			return &v;
	return nullptr;
}

using ScoreI8Fn = void (*)(ScoreIdsI8Params);
struct ScoreI8Variant {
	int d, mode;
	ScoreI8Fn fn;
};
#define SCORE_I8(D) {D, kU8L2, score_ids_i8_kernel<D, kU8L2>}, {D, kI8L2, score_ids_i8_kernel<D, kI8L2>}, \
	{D, kI8L2Ref, score_ids_i8_kernel<D, kI8L2Ref>}, {D, kI8IP, score_ids_i8_kernel<D, kI8IP>}
const ScoreI8Variant kScoreI8[] = {SCORE_I8(64), SCORE_I8(128), SCORE_I8(256), SCORE_I8(768), SCORE_I8(832), SCORE_I8(960),
                                   {64, kI16L2Ref, score_ids_i8_kernel<128, kI16L2Ref>},
                                   {128, kI16L2Ref, score_ids_i8_kernel<256, kI16L2Ref>}};
#undef SCORE_I8
const ScoreI8Variant kScoreI8Any[] = {{0, kU8L2, score_ids_i8_any_kernel<kU8L2>}, {0, kI8L2, score_ids_i8_any_kernel<kI8L2>},
                                      {0, kI8L2Ref, score_ids_i8_any_kernel<kI8L2Ref>}, {0, kI8IP, score_ids_i8_any_kernel<kI8IP>}};


// Does a level of ratio r fit lists of `cap` keys?  A level that scans r times the rows of the level before keeps
// C = #(its rows under the k-th best of the level before) rows per query; on iid rows E C = r k and
// Var C <= r (r + 1) k (r k from the draw of its own rows, r^2 k from the spread of the threshold; r (r - 1) k when
// the samples are nested).  It fits when mean + 6 standard deviations do -- at m * levels ~ 10^5 lists per search
// an overflow by chance then has probability ~ 10^-4 -- with cap / 32 left to the fp16 and int8 filters, which
// also keep the rows within their rounding error of the threshold, and two groups to the rounding of the levels'
// sizes.  (r k + 6 sqrt(v) <= room, written without the root.)
// Under a row filter (plan_levels_filtered) k-th bests and counts are over the allowed rows, of which a level's
// strided scan meets a random number: for a random filter of density p that adds at most r k (1 - p) to the
// variance, under 100 rows in quadrature at k = 8192 -- inside the cap / 32, not in the 6 sigma, and not covered by a
// test (the row filter's cases stop at k = 1000).
constexpr bool ratio_fits(double r, double k, uint32_t cap) {
	const double slack = (double)cap - cap / 32 - 2 * kRowsPerGroup - r * k;
	return slack >= 0 && 36.0 * r * (r + 1.0) * k <= slack * slack;
}
// the plans of k <= 7200 rest on this: at the floor of ratio 2 they fit the longest lists; k = cap / 2 does not
static_assert(ratio_fits(2.0, 7200, kMaxCap) && !ratio_fits(2.0, 7300, kMaxCap) && !ratio_fits(2.0, kMaxCap / 2, kMaxCap) &&
                  ratio_fits(1.78125, kMaxCap / 2, kMaxCap),
              "plan_levels: ratio 2 up to k = 7200, 1.78 at the bound");

// Threshold levels: level 0 keeps every row of a small strided sample (tau = +inf), each
// later level scans `ratio` times more rows with tau = k-th best score of the level before,
// the last level scans every row.  Expected survivors per query and level ~ ratio * k.
std::vector<Level> plan_levels(size_t n, size_t k, uint32_t cap, long ratio_opt) {
	const uint32_t n_groups = (uint32_t)((n + kRowsPerGroup - 1) / kRowsPerGroup);
	uint32_t s0 = std::max<uint32_t>(64, (uint32_t)((4 * k + kRowsPerGroup - 1) / kRowsPerGroup));
	s0 = std::min(s0, cap / kRowsPerGroup);
	std::vector<Level> lv;
	if (n_groups <= s0) {
		lv.push_back({n_groups, 1});
		return lv;
	}
	// survivors ~ ratio*k must stay well inside cap
	double max_ratio = std::max(2.0, (double)cap / (6.0 * (double)k));
	double ratio = std::min<double>((double)ratio_opt, max_ratio);
	if (ratio < 2.0)
		ratio = 2.0;
	// At the largest capacity no retry can lengthen the lists, and from k = 7293 on ratio 2 no longer fits them
	// (ratio_fits above).  Take the largest ratio that does: more levels, each shorter; k = cap / 2 ends at 1.78.
	// Only a plan that stands at the floor of 2 is touched, and every k <= 7200 fits there (the static_assert), so
	// those plan as before at every capacity; smaller capacities still grow on overflow.
	if (cap >= kMaxCap && ratio <= 2.0)
		while (ratio > 1.25 && !ratio_fits(ratio, (double)k, cap))
			ratio -= 1.0 / 64.0;
	const double span = (double)n_groups / (double)s0;
	int steps = (int)std::ceil(std::log(span) / std::log(ratio) - 1e-9);
	if (steps < 1)
		steps = 1;
	const double r = std::pow(span, 1.0 / steps);
	double cur = s0;
	lv.push_back({s0, n_groups / s0});
	for (int i = 1; i < steps; ++i) {
		cur *= r;
		uint32_t sel = (uint32_t)std::llround(cur);
		sel = std::min(sel, n_groups);
		lv.push_back({sel, std::max<uint32_t>(1, n_groups / sel)});
	}
	lv.push_back({n_groups, 1});
	return lv;
}

// The same ladder under a row filter.  It is planned on the ALLOWED rows -- a level's survivors
// are ~ratio * k when it holds ratio times the allowed rows of the level before -- and stretched by n / n_allowed
// to the physical groups a strided scan must visit to meet that many.  Level 0 cannot be a strided scan: a
// sample of 1 024 rows holds 1 024 p allowed ones, fewer than k under a selective filter (+inf thresholds, every
// list overflows).  It takes its rows from the filter's list instead -- an even sample of the allowed rows
// whatever their share and position.  n_allowed <= cap: the list is complete and is the whole search (one level,
// every allowed row's exact key, the select finishes).
std::vector<Level> plan_levels_filtered(size_t n, size_t n_allowed, uint32_t list_len, size_t k, uint32_t cap,
                                        long ratio_opt) {
	std::vector<Level> lv;
	if ((n_allowed + kRowsPerGroup - 1) / kRowsPerGroup * kRowsPerGroup <= cap && list_len == n_allowed) {
		Level l{(uint32_t)((n_allowed + kRowsPerGroup - 1) / kRowsPerGroup), 1};
		l.list_rows = (uint32_t)n_allowed;
		lv.push_back(l);
		return lv;
	}
	const uint32_t n_groups = (uint32_t)((n + kRowsPerGroup - 1) / kRowsPerGroup);
	lv = plan_levels(n_allowed, k, cap, ratio_opt);
	const double stretch = (double)n / (double)n_allowed;
	Level& l0 = lv.front();
	l0.list_rows = std::min<uint32_t>(l0.n_groups_sel * kRowsPerGroup, list_len);
	l0.list_step = std::max<uint32_t>(1, list_len / l0.list_rows);
	l0.n_groups_sel = (l0.list_rows + kRowsPerGroup - 1) / kRowsPerGroup;
	l0.group_stride = 1;
	for (size_t i = 1; i < lv.size(); ++i) {
		const uint32_t sel = (uint32_t)std::min<double>(n_groups, std::ceil(lv[i].n_groups_sel * stretch));
		lv[i].n_groups_sel = sel;
		lv[i].group_stride = std::max<uint32_t>(1, n_groups / sel);
	}
	if (lv.size() < 2)
		lv.push_back(Level{n_groups, 1});
	lv.back() = Level{n_groups, 1};
	return lv;
}

// grow one of the handle's shared buffers; deferred searches still in flight read the old block, so
// their stream is drained first (hipFree happens to synchronise the device: stated, not implied)
template <typename T> hipError_t grow_ws(expann_index* h, GrowPtr<T>& b, size_t need) {
	if (h->async_pending > 0 && (need > b.bytes || !b.p)) {
		const hipError_t e = hipStreamSynchronize(h->async_stream);
		if (e != hipSuccess)
			return e;
	}
	return b.ensure(need);
}

int ensure_workspace(expann_index* h, size_t m, uint32_t cap) {
	if (h->async_pending > 0 && m > h->m_alloc)  // (the per-query arrays below: as grow_ws)
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	if (m > h->m_alloc) {  // the per-query arrays grow together
		h->m_alloc = 0;
		for (DevPtr<float>* b : {std::addressof(h->d_qnrm), std::addressof(h->d_qscale), std::addressof(h->d_theta),
		                         std::addressof(h->d_tau[0]), std::addressof(h->d_tau[1]), std::addressof(h->d_tau_s)}) {
			b->reset();
			HIP_TRY(h, hipMalloc(&*b, sizeof(float) * m));
		}
		for (DevPtr<uint32_t>* b : {std::addressof(h->d_cnt), std::addressof(h->d_tau_row[0]),
		                            std::addressof(h->d_tau_row[1])}) {
			b->reset();
			HIP_TRY(h, hipMalloc(&*b, sizeof(uint32_t) * m));
		}
		h->d_qself.reset();
		HIP_TRY(h, hipMalloc(&h->d_qself, sizeof(int) * m));
		h->m_alloc = m;
	}
	HIP_TRY(h, grow_ws(h, h->d_cand, sizeof(uint64_t) * m * (size_t)cap));
	if (!h->d_overflow) {
		// flags [4 x u32] and statistics [2 x u64] share one allocation: one memset, one read-back
		HIP_TRY(h, hipMalloc(&h->d_overflow, sizeof(uint32_t) * 4 + sizeof(unsigned long long) * 2));
		// every word starts at zero: the paths clear only the words they use, and expann_sync /
		// the strict uint8 check read words 1..3 of searches that never wrote them
		HIP_TRY(h, hipMemset(h->d_overflow, 0, sizeof(uint32_t) * 4 + sizeof(unsigned long long) * 2));
		h->d_total = reinterpret_cast<unsigned long long*>(h->d_overflow + 4);
		HIP_TRY(h, hipHostMalloc((void**)&h->h_flags, sizeof(uint32_t) * 8, 0));
		HIP_TRY(h, hipHostMalloc((void**)&h->h_flag_ring, sizeof(uint32_t) * kRingWords * kAsyncRing, 0));
		HIP_TRY(h, hipMalloc(&h->d_ticket, sizeof(uint32_t)));
		HIP_TRY(h, hipMemset(h->d_ticket, 0, sizeof(uint32_t)));
		HIP_TRY(h, hipDeviceSynchronize());  // (once per handle: the counter is zero before any stream uses it)
	}
	return EXPANN_OK;
}

// ---- GEMM-form (MFMA) scan: dims it is built for ----------------------------------------
// the bf16x3 form (fp32 L2 rows), with the kernels of its row and query terms (gemm_terms.hpp)
using NormFn = void (*)(const float*, uint32_t, float, float*);
using ThetaFn = void (*)(const float*, uint32_t, const float*, float, float*);
using GemmBf16Fn = void (*)(GemmBf16Params);
struct GemmBf16Variant {
	int d;
	GemmBf16Fn scan;
	NormFn norms;
	ThetaFn theta;
	const char* name;
};
// (The compiler emits a kernel template's instances into the code object in the order in which the source first names
// them.  Naming the four term kernels here, ahead of the two scans, keeps that order -- terms of 64, of 128, then the
// scans -- as it was while the terms sat in a table of their own, so the device code of this file stays byte for byte
// what it was and a comparison of two builds' assembly shows kernel changes only.)
constexpr struct {
	NormFn norms;
	ThetaFn theta;
} kBf16Terms[] = {{row_norms_kernel<64>, query_theta_kernel<64>}, {row_norms_kernel<128>, query_theta_kernel<128>}};
const GemmBf16Variant kGemmBf16[] = {
    {64, scan_gemm_bf16x3_kernel<64>, kBf16Terms[0].norms, kBf16Terms[0].theta, "scan_gemm_bf16x3<64>"},
    {128, scan_gemm_bf16x3_kernel<128>, kBf16Terms[1].norms, kBf16Terms[1].theta, "scan_gemm_bf16x3<128>"}};

using GemmF16Fn = void (*)(GemmF16Params);
using SqnormFn = void (*)(const float*, uint32_t, float*);
using F16PrepFn = void (*)(const float*, uint32_t, float, _Float16*, float*, uint32_t*, float*, uint32_t*, const float*, float*,
                          I8fQueryArgs);
struct GemmF16Variant {
	int d;
	GemmF16Fn scan;
	GemmF16Fn sample;
	SqnormFn sqnorm;
	F16PrepFn prep;
	const char* name;
	int tb, wgq, threads, wg_per_cu, lds;  // rows per tile, queries per workgroup, launch geometry
	int hit_log;                           // scan writes per-wave hit logs (scan_gemm_f16x.hpp) + scatter_log_kernel
	GemmF16Fn scan_redo = nullptr;         // the scan's instance for the redo pass of the speculative thresholds, if built
};
// the 16x16x32 form of the full scan and of the sampled pass (scan_gemm_f16x.hpp)
#define F16X_V(D)                                                                                  \
	{D, scan_gemm_f16x_kernel<D, false>, scan_gemm_f16x_kernel<D, true>, sqnorm_kernel<D>,          \
	 f16_query_prep_kernel<D>, "scan_gemm_f16x<" #D ", false>", kF16TB, kF16TQ, kF16Threads,         \
	 f16x_wg_per_cu<D>(), gemm_f16x_lds_bytes<D>(), 1, scan_gemm_f16x_kernel<D, false, 0, true>}
// (d = 64 with two workgroups per CU measured slower than scan_gemm_f16_kernel<64>'s three: 6.55 M vs
// 6.83 M QPS at 1 M rows -- two k-steps per column leave too little MFMA per step; hence three here too)
// d = 256 / 512: the 8-waves-per-tile geometry on 16x16x32 (scan_gemm_w8.hpp, fp16 instances), hits appended directly
#define F16Y_V(D)                                                                                  \
	{D, scan_gemm_w8_kernel<F16Elem, D, false>, scan_gemm_w8_kernel<F16Elem, D, true>, sqnorm_kernel<D>, f16_query_prep_kernel<D>, \
	 "scan_gemm_f16y<" #D ", false>", kF16TB, F16Geom<D>::WGQ, F16Geom<D>::THREADS, F16Geom<D>::WG_PER_CU, \
	 gemm_f16_lds_bytes<D>(), 0}
// 512 < d <= 960: the k-split geometry on 16x16x32 (scan_gemm_f16kx.hpp)
#define F16KX_V(D)                                                                                 \
	{D, scan_gemm_f16kx_kernel<D, false>, scan_gemm_f16kx_kernel<D, true>, sqnorm_kernel<D>, f16_query_prep_kernel<D>, \
	 "scan_gemm_f16kx<" #D ", false>", F16kGeom<D>::TB, F16kGeom<D>::WGQ, F16kGeom<D>::THREADS, 1,     \
	 F16kGeom<D>::LDS_BYTES, 0}
const GemmF16Variant kGemmF16X[] = {F16X_V(64), F16X_V(128), F16Y_V(256), F16Y_V(512), F16KX_V(768), F16KX_V(832), F16KX_V(960)};
#undef F16KX_V
#undef F16Y_V
#undef F16X_V
// the same with the run-time ablation switches compiled in ("debug" option != 0)
const GemmF16Variant kGemmF16XDbg[] = {{128, scan_gemm_f16x_kernel<128, false, 1>, scan_gemm_f16x_kernel<128, true>,
                                        sqnorm_kernel<128>, f16_query_prep_kernel<128>, "scan_gemm_f16x<128, false>",
                                        kF16TB, kF16TQ, kF16Threads, 2, gemm_f16_lds_bytes<128>(), 1}};
// the fp16 filter with the dim known at run time (scan_gemm_kl.hpp, fp16 instances): every f32 dim from 64 up without a
// form of its own (d = 0 here; prelude: sqnorm_any_kernel / f16_query_prep_any_kernel)
const GemmF16Variant kGemmF16KL = {0, scan_gemm_kl_kernel<F16Elem, false>, scan_gemm_kl_kernel<F16Elem, true>, nullptr, nullptr,
                                   "scan_gemm_f16kl", kKlTB, kF16TQ, kF16Threads, 1, kKlLds, 1};
// row length of the index's fp16 copy: whole 32-element MFMA k-steps for the run-time-dim form
inline int f16_ld(int d) { return f16kl_dim(d) ? (d + 31) / 32 * 32 : d; }
// the variant of a plan's fp16 family (bf_plan.hpp) at dim d
const GemmF16Variant* find_f16(ScanFamily f, int d) {
	if (f == ScanFamily::kF16KL)
		return &kGemmF16KL;
	if (f == ScanFamily::kF16Dbg)
		return &kGemmF16XDbg[0];
	for (const auto& v : kGemmF16X)
		if (is_f16(f) && v.d == d)
			return &v;
	return nullptr;
}

// a handful of queries: the same filter streamed from HBM without the matrix cores
// (scan_direct_f16.hpp); tq = queries per pass
using SampleDirectFn = void (*)(SampleDirectParams);
struct DirectF16Variant {
	int d, tq, rps;
	GemmF16Fn fn;
	const char* name;
	SampleDirectFn sample;  // fused sampled pass + thresholds (nullptr: the MFMA SAMPLE pass serves)
	int cpw;                // its classes per workgroup
};
#define DF16_V(D, TQ) {D, TQ, DirectF16Geom<D>::RPS, scan_direct_f16_kernel<D, TQ>, "scan_direct_f16<" #D ", " #TQ ">", \
	sample_direct_f16_kernel<D, TQ>, DirectF16Geom<D>::RW * (kBlock / 64)}
#define DF16_VN(D, TQ) {D, TQ, DirectF16Geom<D>::RPS, scan_direct_f16_kernel<D, TQ>, "scan_direct_f16<" #D ", " #TQ ">", \
	nullptr, 0}
const DirectF16Variant kDirectF16[] = {DF16_V(64, 2),  DF16_V(64, 4),  DF16_V(128, 2), DF16_V(128, 4),
                                       DF16_V(256, 2), DF16_V(256, 4), DF16_V(512, 1), DF16_V(512, 2),
                                       DF16_VN(768, 1), DF16_VN(832, 1), DF16_VN(960, 1)};
#undef DF16_V
#undef DF16_VN
// the variant of tile tq (bf_plan.hpp's direct_f16_tile; 0: none)
const DirectF16Variant* find_direct_f16(int d, int tq) {
	for (const auto& v : kDirectF16)
		if (tq && v.d == d && v.tq == tq)
			return &v;
	return nullptr;
}

// fp16 copy of the base (scaled by a power of two), its slack-adjusted norms, max norm
int make_f16(expann_index* h, const GemmF16Variant* gf, hipStream_t st);
// (a failure on the way leaves no half-made copy behind -- arrays without a scale or a tile size --: the derived
// copies are forgotten as a whole and the next search starts over)
int ensure_f16(expann_index* h, const GemmF16Variant* gf, hipStream_t st) {
	if (h->d_base_f16 || h->f16_scale < 0.0f)
		return EXPANN_OK;
	const int rc = make_f16(h, gf, st);
	if (rc != EXPANN_OK)
		h->forget<RowCopies>();
	return rc;
}
int make_f16(expann_index* h, const GemmF16Variant* gf, hipStream_t st) {
	const size_t nv = h->n * (size_t)h->dim;
	DevBuf tmp, nrm;
	HIP_TRY(h, tmp.alloc(sizeof(float)));
	HIP_TRY(h, nrm.alloc(sizeof(float) * h->n));
	HIP_TRY(h, hipMemsetAsync(tmp.p, 0, sizeof(uint32_t), st));
	const bool hrows = f16_rows(h);  // binary16 source: converted on load, then the same prelude (same bits out)
	const _Float16* const base_h = (const _Float16*)h->d_base;
	if (hrows)
		hipLaunchKernelGGL(maxabs_bits_kernel<_Float16>, dim3(2048), dim3(kBlock), 0, st, base_h, nv, tmp.as<uint32_t>());
	else
		hipLaunchKernelGGL(maxabs_bits_kernel<float>, dim3(2048), dim3(kBlock), 0, st, (const float*)h->d_base, nv,
		                   tmp.as<uint32_t>());
	float maxabs = 0.0f;  // (a NaN pattern stays a NaN and fails the range check below)
	HIP_TRY(h, hipMemcpyAsync(&maxabs, tmp.p, sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));
	const F16Scale fs = f16_scale_for(maxabs);  // (bf_append.hpp: the rule an append compares with)
	const float scale = fs.scale;
	h->f16_maxabs = maxabs;
	if (!fs.usable) {  // non-finite or astronomically large values
		h->f16_scale = -1.0f;
		return EXPANN_OK;
	}
	// padded to whole tiles (64 rows; 128 for scan_gemm_kl): zero rows whose bn' is NaN (never a candidate).  The
	// allocation covers the base's capacity (a base that was never reserved or appended to: its n rows), so that an
	// append finds its tiles initialised; the scans read n_pad rows.
	const size_t tb = (size_t)std::max(kF16TB, gf->tb);
	const size_t n_pad = (h->n + tb - 1) / tb * tb;
	const size_t n_alloc = (std::max(h->n, h->capacity) + tb - 1) / tb * tb;
	const size_t ld = (size_t)f16_ld(h->dim);
	HIP_TRY(h, hipMalloc(&h->d_base_f16, n_alloc * ld * 2));
	HIP_TRY(h, hipMalloc(&h->d_bnorm_f16, sizeof(float) * n_alloc));
	HIP_TRY(h, hipMalloc(&h->d_bns_f16, sizeof(float) * n_alloc));
	HIP_TRY(h, hipMemsetAsync(h->d_base_f16, 0, n_alloc * ld * 2, st));
	HIP_TRY(h, hipMemsetAsync(h->d_bnorm_f16, 0xFF, sizeof(float) * n_alloc, st));  // 0xFFFFFFFF: a NaN
	HIP_TRY(h, hipMemsetAsync(h->d_bns_f16, 0xFF, sizeof(float) * n_alloc, st));
	if (!h->d_bnmax)
		HIP_TRY(h, hipMalloc(&h->d_bnmax, 4 * sizeof(float)));
	const uint32_t blocks16 = (uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup);
	if (hrows) {  // (ld == d on the dims with a compiled form: the padded convert is the plain one there)
		hipLaunchKernelGGL(convert_f16_pad_kernel<_Float16>, dim3(8192), dim3(kBlock), 0, st, base_h, h->n, (uint32_t)h->dim,
		                   (uint32_t)ld, scale, h->d_base_f16.as<_Float16>());
		hipLaunchKernelGGL(sqnorm_any_kernel<_Float16>, dim3(blocks16), dim3(kBlock), 0, st, base_h, (uint32_t)h->n,
		                   (uint32_t)h->dim, nrm.as<float>());
	} else if (gf->d == 0) {  // run-time dim: rows of ld elements, zero past d; norms over the d real ones
		hipLaunchKernelGGL(convert_f16_pad_kernel<float>, dim3(8192), dim3(kBlock), 0, st, (const float*)h->d_base, h->n,
		                   (uint32_t)h->dim, (uint32_t)ld, scale, h->d_base_f16.as<_Float16>());
		hipLaunchKernelGGL(sqnorm_any_kernel<float>, dim3(blocks16), dim3(kBlock), 0, st, (const float*)h->d_base,
		                   (uint32_t)h->n, (uint32_t)h->dim, nrm.as<float>());
	} else {
		hipLaunchKernelGGL(convert_f16_kernel, dim3((uint32_t)std::min<size_t>((nv + kBlock - 1) / kBlock, 8192)),
		                   dim3(kBlock), 0, st, (const float*)h->d_base, nv, scale, h->d_base_f16.as<_Float16>(),
		                   (uint32_t*)nullptr);
		hipLaunchKernelGGL(gf->sqnorm, dim3(blocks16), dim3(kBlock), 0, st, (const float*)h->d_base,
		                   (uint32_t)h->n, nrm.as<float>());
	}
	hipLaunchKernelGGL(max_f32_kernel, dim3(1), dim3(1024), 0, st, (const float*)nrm.p, h->n,
	                   h->d_bnmax + 2);
	const float abs_coef = std::ldexp(1.0f, -24) / scale * std::sqrt((float)h->dim);
	const int ipm = h->metric == EXPANN_METRIC_IP ? 1 : 0;
	hipLaunchKernelGGL(f16_terms_kernel, dim3((uint32_t)((h->n + kBlock - 1) / kBlock)), dim3(kBlock),
	                   0, st, (const float*)nrm.p, (uint32_t)h->n, gemm_f16_filter_eps(h->dim), abs_coef,
	                   (const float*)nullptr, 0.5f * scale * scale, h->d_bnorm_f16, ipm, (const float*)nullptr);
	hipLaunchKernelGGL(f16_terms_kernel, dim3((uint32_t)((h->n + kBlock - 1) / kBlock)), dim3(kBlock),
	                   0, st, (const float*)nrm.p, (uint32_t)h->n, -gemm_f16_filter_eps(h->dim), -abs_coef,
	                   (const float*)nullptr, 0.5f * scale * scale, h->d_bns_f16, ipm, (const float*)nullptr);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipStreamSynchronize(st));  // tmp/nrm are freed on return
	h->f16_scale = scale;
	h->f16_n_pad = n_pad;
	h->f16_tb = tb;
	h->f16_rows_alloc = n_alloc;
	return EXPANN_OK;
}

// The fp16 forms' row terms under the row filter: NaN on every disallowed row, made after ensure_f16 and again
// whenever the filter changed (one pass over n_pad floats per array, on the search's stream)
int ensure_filter_terms(expann_index* h, hipStream_t st) {
	if (!h->filter_on || !h->d_bnorm_f16 || (h->filter_terms_valid && h->d_bnorm_f16_m))
		return EXPANN_OK;
	if (h->f16_n_pad > h->filter_words * 32)
		return h->fail(EXPANN_ERR_HIP, "row filter: the bitmap is shorter than the fp16 copy");  // (both are whole 128-row tiles)
	if (!h->d_bnorm_f16_m) {
		HIP_TRY(h, hipMalloc(&h->d_bnorm_f16_m, sizeof(float) * h->f16_n_pad));
		HIP_TRY(h, hipMalloc(&h->d_bns_f16_m, sizeof(float) * h->f16_n_pad));
	}
	const dim3 grid((uint32_t)std::min<size_t>((h->f16_n_pad + kBlock - 1) / kBlock, 4096));
	hipLaunchKernelGGL(filter_row_terms_kernel, grid, dim3(kBlock), 0, st, h->d_filter_bits.as<const uint32_t>(),
	                   h->d_bnorm_f16.as<const float>(), h->d_bnorm_f16_m.as<float>(), (uint32_t)h->f16_n_pad);
	hipLaunchKernelGGL(filter_row_terms_kernel, grid, dim3(kBlock), 0, st, h->d_filter_bits.as<const uint32_t>(),
	                   h->d_bns_f16.as<const float>(), h->d_bns_f16_m.as<float>(), (uint32_t)h->f16_n_pad);
	HIP_TRY(h, hipGetLastError());
	h->filter_terms_valid = true;
	return EXPANN_OK;
}
// forget everything the filter derived (the rows changed, or the handle is rebuilt)
void drop_row_filter(expann_index* h) { h->forget<RowFilter>(); }
// forget the row groups (they belong to the rows they were set for)
void drop_row_groups(expann_index* h) { h->forget<RowGroups>(); }

// what the planner (bf_plan.hpp) reads of a handle
PlanIndex plan_index(const expann_index* h) {
	PlanIndex x;
	x.dtype = h->dtype;
	x.int_mode = h->int_mode;
	x.metric = h->metric;
	x.dim = h->dim;
	x.n = h->n;
	x.scan_kernel = h->opt_scan_kernel;
	x.query_tile = h->opt_query_tile;
	x.i8_filter = h->opt_i8_filter;
	x.u8_exact_opt = h->opt_u8_exact;
	x.sample_pass = h->opt_sample_pass;
	x.spec_rank = h->opt_spec_rank;
	x.debug = h->opt_debug;
	x.cand_capacity = h->opt_cand_capacity;
	x.f16_ok = h->f16_scale >= 0.0f;
	x.i8f_state = h->i8f_state;
	x.u8_exact = h->u8_exact;
	x.filter_on = h->filter_on;
	x.n_allowed = h->n_allowed;
	return x;
}

// the bf16x3 form's row terms and planes
int ensure_bnorm_bf16(expann_index* h, const GemmBf16Variant* gvb, hipStream_t st) {
	const uint32_t blocks = (uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup);
	if (!h->d_bnorm_bf) {
		HIP_TRY(h, hipMalloc(&h->d_bnorm_bf, sizeof(float) * h->n));
		hipLaunchKernelGGL(gvb->norms, dim3(blocks), dim3(kBlock), 0, st, (const float*)h->d_base,
		                   (uint32_t)h->n, 1.0f - gemm_bf16_filter_eps(h->dim), h->d_bnorm_bf);
		if (!h->d_bnmax)
			HIP_TRY(h, hipMalloc(&h->d_bnmax, 4 * sizeof(float)));
		hipLaunchKernelGGL(max_f32_kernel, dim3(1), dim3(1024), 0, st, (const float*)h->d_bnorm_bf, h->n, h->d_bnmax + 1);
		HIP_TRY(h, hipGetLastError());
	}
	if (!h->d_base_split) {
		const size_t nv = h->n * (size_t)h->dim;
		HIP_TRY(h, hipMalloc(&h->d_base_split, nv * 4));
		hipLaunchKernelGGL(split_bf16_kernel, dim3((uint32_t)((nv + kBlock - 1) / kBlock)),
		                   dim3(kBlock), 0, st, (const float*)h->d_base, h->n, h->dim,
		                   h->d_base_split.as<__bf16>());
		HIP_TRY(h, hipGetLastError());
	}
	return EXPANN_OK;
}

// ---- 8-bit GEMM form (int8 MFMA) -----------------------------------------------------------
using GemmI8Fn = void (*)(GemmI8Params);
using SelfI8Fn = void (*)(const void*, uint32_t, int*);
using ThetaI8Fn = void (*)(const void*, uint32_t, const float*, int*, int*);
struct GemmI8Variant {
	int d, mode;
	GemmI8Fn scan;
	SelfI8Fn self;
	ThetaI8Fn theta;
	const char* name;
};
#define GEMM_I8(D, MODE, MN) {D, MODE, scan_gemm_i8_kernel<D, MODE>, row_self_i8_kernel<D, MODE>, \
	query_theta_i8_kernel<D, MODE>, "scan_gemm_i8<" #D "," MN ">"}
const GemmI8Variant kGemmI8[] = {
    GEMM_I8(128, kU8L2, "U8L2"), GEMM_I8(128, kI8L2, "I8L2"), GEMM_I8(128, kI8IP, "I8IP"),
    GEMM_I8(256, kU8L2, "U8L2"), GEMM_I8(256, kI8L2, "I8L2"), GEMM_I8(256, kI8IP, "I8IP"),
    GEMM_I8(768, kU8L2, "U8L2"), GEMM_I8(768, kI8L2, "I8L2"), GEMM_I8(768, kI8IP, "I8IP")};
#undef GEMM_I8

const GemmI8Variant* find_gemm_i8(int d, int mode) {
	for (const auto& v : kGemmI8)
		if (v.d == d && v.mode == mode)
			return &v;
	return nullptr;
}

int ensure_bias_i8(expann_index* h, const GemmI8Variant* gv, hipStream_t st) {
	if (h->d_bias_i || h->int_mode == kI8IP)
		return EXPANN_OK;
	HIP_TRY(h, hipMalloc(&h->d_bias_i, sizeof(int) * h->n));
	const uint32_t blocks = (uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup);
	hipLaunchKernelGGL(gv->self, dim3(blocks), dim3(kBlock), 0, st, (const void*)h->d_base,
	                   (uint32_t)h->n, h->d_bias_i);
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

// one wave per query for lists of <= 512 keys, then (when the buffers allow longer lists) for
// <= 1024 and <= 2048; select_topk_kernel takes what is left (sel.wave_done = longest list served)
// `longest` = the longest list the batch is expected to hold (select_longest_list): a stage whose lists would be
// the rare tail is not launched -- an empty launch still costs ~5 us of the stream, 3 % of a step on a 125 k-row
// shard -- and select_topk_kernel's workgroup-per-query sort takes those few lists.  (The sort of a 600-key list
// with its re-rank takes 40-70 us, so a stage is worth its launch as soon as a handful of lists need it.)
// The longest list of a batch from the length `expect` the thresholds aim at (~1.2 frac x the rank of the class
// maximum the threshold is).  Proven thresholds (rank k): twice the expectation, the stages' classes since round 2.
// A speculative threshold of rank j: the lists' relative spread grows as the rank falls -- 10 000 queries at C2,
// longest / mean: 2.35 (int8 filter) and 2.5 (fp16 form) at rank 10, 3.3 / 3.4 at rank 5, 3.8 / 3.8 at rank 4
// (profiles/r07_spec_tau_ab.txt) -- which 1 + 4.5 / sqrt(j) follows.
uint32_t select_longest_list(double expect, uint32_t spec_j) {
	return spec_j ? (uint32_t)(expect * (1.0 + 4.5 / std::sqrt((double)spec_j))) : 2u * (uint32_t)expect;
}
// (rows_f16: sel.rerank_base holds binary16 rows -- the _Float16 instances of the same kernels)
// `side` (or nullptr): the stream of the stages behind the first.  The stages serve disjoint queries, write disjoint
// output rows and share only atomic counters, so with a side stream -- which the caller has made wait for the
// gather -- the long lists' stages run beside the short lists' <8,4> launch instead of behind it.
// (sel.tau_f set -- the int8 filter's lists, fp32 rows -- : the two-round instances)
void launch_select_wave(SelectParams& sel, size_t m, uint32_t cap, hipStream_t st, uint32_t longest, bool rows_f16 = false,
                        hipStream_t side = nullptr) {
	using WaveFn = void (*)(SelectParams, uint32_t);
	const bool two = sel.tau_f != nullptr;
	const WaveFn w8 = rows_f16 ? select_wave_kernel<8, 4, _Float16>
	                           : (two ? select_wave_kernel<8, 4, float, true> : select_wave_kernel<8, 4>);
	const WaveFn w16 = rows_f16 ? select_wave_kernel<16, 2, _Float16>
	                            : (two ? select_wave_kernel<16, 2, float, true> : select_wave_kernel<16, 2>);
	const WaveFn w32 = rows_f16 ? select_wave_kernel<32, 1, _Float16>
	                            : (two ? select_wave_kernel<32, 1, float, true> : select_wave_kernel<32, 1>);
	const hipStream_t st2 = side ? side : st;
	sel.wave_done = 0;
	hipLaunchKernelGGL(w8, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, st, sel, (uint32_t)m);
	sel.wave_done = 512;
	if (longest <= 512)
		return;
	if (cap > 512) {
		// (k = 100: ~920-entry lists -- half the registers and ballots of the 2048-key form)
		hipLaunchKernelGGL(w16, dim3((uint32_t)((m + 1) / 2)), dim3(128), 0, st2, sel, (uint32_t)m);
		sel.wave_done = 1024;
	}
	if (cap > 1024 && longest > 1024) {
		hipLaunchKernelGGL(w32, dim3((uint32_t)m), dim3(64), 0, st2, sel, (uint32_t)m);
		sel.wave_done = 2048;
	}
}
using SelectTopkFn = void (*)(SelectParams);
inline SelectTopkFn select_topk_fn(const expann_index* h, const SelectParams& sel) {
	if (sel.tau_f)  // (the int8 filter's lists: fp32 rows)
		return select_topk_kernel<float, true>;
	return f16_rows(h) ? select_topk_kernel<_Float16> : select_topk_kernel<float>;
}
// The select of a full scan's lists: the wave stages, the left-over launch, the statistics sum.
// When a second wave stage is launched at all (longest > 512) and "select_overlap" allows it, everything but the
// <8,4> stage goes to the handle's side stream: forked behind the gather by one event, joined into `st` by another
// before this returns -- whatever follows on `st` (the redo pass, the flag copy, the next search) sees every
// stage's output rows and counters.  No host wait.
int launch_select(expann_index* h, SelectParams& sel, size_t m, uint32_t cap, hipStream_t st, uint32_t longest,
                  bool sum_counts) {
	hipStream_t side = nullptr;
	if (h->opt_select_overlap && longest > 512 && cap > 512) {
		if (!h->side_stream) {
			HIP_TRY(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
			for (OwnedEvent& e : h->side_ev)
				HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
		}
		side = h->side_stream;
		HIP_TRY(h, hipEventRecord(h->side_ev[0], st));
		HIP_TRY(h, hipStreamWaitEvent(side, h->side_ev[0], 0));
	}
	const hipStream_t st2 = side ? side : st;
	launch_select_wave(sel, m, cap, st, longest, f16_rows(h), side);
	hipLaunchKernelGGL(select_topk_fn(h, sel), dim3((uint32_t)m), dim3(kBlock), sizeof(uint64_t) * cap + 16, st2, sel);
	// statistics: candidates of the full scan (i8f_cand_limit).  LAST on the side stream: one 1 024-thread workgroup that
	// runs 35 us beside the <8,4> stage (5 us alone), and in front of the <16,2> stage it made the side chain the span
	if (sum_counts)
		hipLaunchKernelGGL(sum_u32_kernel, dim3(1), dim3(1024), 0, st2, sel.cand_cnt, (uint32_t)m, h->d_total);
	HIP_TRY(h, hipGetLastError());
	if (side) {
		HIP_TRY(h, hipEventRecord(h->side_ev[1], side));
		HIP_TRY(h, hipStreamWaitEvent(st, h->side_ev[1], 0));
	}
	return EXPANN_OK;
}

// Per-wave hit logs of the scans that write them (scan_gemm_f16x.hpp, scan_gemm_i8w.hpp): one log
// per wave of the grid, together as large as the candidate lists they are filed into; the launch
// geometry is kept for launch_gather_logs.
int ensure_hit_logs(expann_index* h, uint32_t grid, int waves, size_t m, uint32_t cap, uint32_t n_chunks,
                    uint32_t n_qtiles, uint32_t xcd_map, hipStream_t st, uint4** log, uint32_t** log_cnt,
                    uint32_t* log_cap_out) {
	const uint32_t n_logs = grid * (uint32_t)waves;
	// four times a wave's average share of the candidate lists (queries sorted by cluster send a wave's
	// 64 queries to the same row chunk; memory that is never written costs nothing)
	const uint32_t log_cap = std::max<uint32_t>(
	    4096, pow2ceil((uint32_t)std::min<size_t>(4 * ((m * (size_t)cap + n_logs - 1) / n_logs), 1u << 20)));
	const size_t need = (size_t)n_logs * log_cap * 16;
	if (need > h->log_bytes || n_logs > h->log_cnt_n) {
		HIP_TRY(h, hipStreamSynchronize(st));
		h->d_log.reset();
		h->d_log_cnt.reset();
		h->log_bytes = h->log_cnt_n = 0;
		HIP_TRY(h, hipMalloc(&h->d_log, need));
		HIP_TRY(h, hipMalloc(&h->d_log_cnt, sizeof(uint32_t) * n_logs));
		h->log_bytes = need;
		h->log_cnt_n = n_logs;
	}
	*log = h->d_log.as<uint4>();
	*log_cnt = h->d_log_cnt;
	*log_cap_out = log_cap;
	h->pending_scatter.n_logs = n_logs;
	h->pending_scatter.log_cap = log_cap;
	h->pending_scatter.cap = cap;
	h->pending_scatter.n_chunks = n_chunks;
	h->pending_scatter.n_qtiles = n_qtiles;
	h->pending_scatter.xcd_map = xcd_map;
	h->pending_scatter.m = (uint32_t)m;
	h->pending_scatter.theta = nullptr;
	h->pending_scatter.key_mul = 0.0f;
	h->pending_scatter.i_mode = 0;
	return EXPANN_OK;
}

// after a scan that wrote hit logs: file them into the per-query candidate lists
void launch_gather_logs(expann_index* h, hipStream_t st) {
	if (!h->pending_scatter.n_logs)
		return;
	const auto ps = h->pending_scatter;
	h->pending_scatter.n_logs = 0;
	// ~1024 workgroups: the logs of a (query tile, wave) pair are split over n_groups of them
	const uint32_t want = std::max<uint32_t>(1, (1024 + ps.n_qtiles * 4 - 1) / (ps.n_qtiles * 4));
	const uint32_t cpb = std::max<uint32_t>(1, (ps.n_chunks + want - 1) / want);
	const uint32_t n_groups = (ps.n_chunks + cpb - 1) / cpb;
	GatherLogParams gp{h->d_log.as<const uint4>(), h->d_log_cnt.as<const uint32_t>(), ps.log_cap, ps.n_chunks,
	                   ps.n_qtiles, ps.xcd_map, ps.m, n_groups, cpb, h->d_cnt, h->d_cand, ps.cap, ps.theta, ps.key_mul,
	                   ps.i_thp, ps.i_bias, ps.i_qself, ps.i_mode, ps.i_rw};
	hipLaunchKernelGGL(gather_logs_kernel, dim3(ps.n_qtiles * 4 * n_groups), dim3(kBlock), 0, st, gp);
}

// Deferred check: the flag block of this search goes to the next ring slot and the call returns
// without waiting; expann_sync looks at the slots.  False when the caller has to wait as usual.
bool defer_flags(expann_index* h, hipStream_t st, int attempt) {
	if (!h->opt_async || h->host_call || attempt != 0 || h->strict_u8 || h->async_pending >= kAsyncRing)
		return false;
	if (hipMemcpyAsync(h->h_flag_ring + kRingWords * h->async_pending, h->d_overflow, kFlagCopyBytes,
	                   hipMemcpyDeviceToHost, st) != hipSuccess)
		return false;
	// ring words kRingScale / kRingMark are the host's: the fp16 scale of the search (set by the caller, 0 = none),
	// and 1 when word 1 (query values outside [0, 255]) belongs to this search (uint8 rows)
	h->h_flag_ring[kRingWords * h->async_pending + kRingScale] = 0;
	h->h_flag_ring[kRingWords * h->async_pending + kRingMark] = h->dtype == EXPANN_DTYPE_U8 ? 1u : 0u;
	h->async_pending++;
	h->async_stream = st;
	h->prof.deferred_searches++;
	return true;
}

// Row-chunk count of a tiled scan.  `slots` workgroups are resident at a time, so a launch of
// g chunks x n_qtiles workgroups runs in rounds: minimise rounds x (steps per workgroup +
// `overhead` steps of prologue / tail).  With xcd != nullptr a multiple of 8 whose rounding leaves
// exactly g chunks is preferred when it costs at most tol_pct % more: blocks b and b+8 share an
// XCD, so the kernels can then keep a row chunk's query tiles on ONE L2 (GemmF16Params::xcd_map).
uint32_t pick_row_chunks(uint32_t n_tiles, uint32_t n_qtiles, uint32_t slots, double overhead, uint32_t min_tiles,
                         uint32_t g_limit, long tol_pct, uint32_t* xcd) {
	const uint32_t gmax = std::max<uint32_t>(1, n_tiles / min_tiles);
	uint32_t chunks = 1, g8 = 0;
	double best = 1e300, best8 = 1e300;
	for (uint32_t g = 1; g <= std::min<uint32_t>(gmax, g_limit); ++g) {
		const uint32_t steps = (n_tiles + g - 1) / g;
		const uint64_t rounds = ((uint64_t)g * n_qtiles + slots - 1) / slots;
		const double cost = (double)rounds * (steps + overhead);
		if (cost < best * 0.999) {
			best = cost;
			chunks = g;
		}
		if (xcd && g % 8 == 0 && cost < best8 * 0.999 && (n_tiles + steps - 1) / steps == g) {
			best8 = cost;
			g8 = g;
		}
	}
	if (xcd) {
		*xcd = 0;
		if (g8 && best8 <= best * (1.0 + 0.01 * (double)tol_pct)) {
			chunks = g8;
			*xcd = 1;
		}
	}
	return chunks;
}

// Two chunk sizes for a launch of several rounds (scan_gemm_f16x): workgroups are dispatched in block
// order and a launch ends when its last workgroup does, so with equal chunks the last round drains
// for about half a workgroup's time (profiles/wg_times.py: 480 of 512 resident on average at C2).
// The chunks of all rounds but the last stay as they are; the rows of the last round are cut three
// times finer.  Both counts are multiples of 8 (xcd_map).  Returns false when the launch is too
// short to gain (fewer than 3 rounds) or the chunk count does not suit.
bool pick_tail_chunks(uint32_t n_tiles, uint32_t g, uint32_t n_qtiles, uint32_t slots, uint32_t min_tiles,
                      uint32_t* tiles_big, uint32_t* n_big, uint32_t* tiles_small, uint32_t* n_small) {
	const uint64_t rounds = ((uint64_t)g * n_qtiles + slots - 1) / slots;
	if (rounds < 3 || g % 8 != 0 || g < 24)
		return false;
	uint32_t nb = (uint32_t)(((rounds - 1) * slots / n_qtiles) / 8) * 8;  // chunks of the first rounds - 1 rounds
	nb = std::min(nb, g - 8);
	if (nb < 8)
		return false;
	const uint32_t ns = (3 * (g - nb) + 7) / 8 * 8;
	const uint32_t big = (uint32_t)(((uint64_t)n_tiles * 3 + (3 * nb + ns) - 1) / (3 * nb + ns));  // big = 3 small
	if ((uint64_t)nb * big >= n_tiles)
		return false;
	const uint32_t rest = n_tiles - nb * big;
	const uint32_t small = (rest + ns - 1) / ns;
	if (small < min_tiles || (uint64_t)(ns - 1) * small >= rest)  // (every small chunk must hold rows)
		return false;
	*tiles_big = big;
	*n_big = nb;
	*tiles_small = small;
	*n_small = ns;
	return true;
}

// ---- speculative thresholds -----------------------------------------------------
// tau_s = the j-th largest class maximum of the sampled pass, j < k.  A query fails the select's check when its
// k-th exact score lies above tau_s, i.e. when j rows of the sample beat the k-th best row of the index: at least
// j of the k - 1 better rows are in the sample, each with probability f (the sampled share of the rows) -- at most
// P(Bin(k - 1, f) >= j) (two of them in one class only loosen tau_s).
constexpr double kSpecFailTarget = 0.01;  // the auto rank's share of failing queries, at most
double spec_fail_share(size_t k, double f, uint32_t j) {
	if (j == 0)
		return 1.0;
	if (k <= 1 || j > k - 1)
		return 0.0;
	f = std::min(1.0, std::max(0.0, f));
	// 1 - sum_{i < j} C(k-1, i) f^i (1-f)^(k-1-i), term by term
	const double n = (double)(k - 1);
	double term = std::pow(1.0 - f, n), below = 0.0;
	for (uint32_t i = 0; i < j; ++i) {
		below += term;
		term = f < 1.0 ? term * (n - i) / (i + 1.0) * f / (1.0 - f) : 0.0;
	}
	return f < 1.0 ? std::max(0.0, 1.0 - below) : 1.0;
}
// the smallest j whose failing share is at most the target; k = speculation off (every j < k fails too often)
uint32_t spec_rank_auto(size_t k, double f) {
	for (uint32_t j = 1; j < k; ++j)
		if (spec_fail_share(k, f, j) <= kSpecFailTarget)
			return j;
	return (uint32_t)k;
}
// query slots of the redo pass: four times the failures the target allows, in whole query tiles
uint32_t spec_redo_slots(size_t m) {
	const size_t want = (size_t)std::ceil(4.0 * kSpecFailTarget * (double)m);
	return (uint32_t)(std::max<size_t>(1, (want + kF16TQ - 1) / kF16TQ) * kF16TQ);
}

// Rows read by the sampled pass = 1/frac.  Its cost falls with frac, the candidates of the full
// scan (~1.2 k frac per query) grow with it.  Measured optima: 12-16 at k = 10 (flat), 8 at
// k = 100 (3.44 ms per 2500 queries x 5 M rows against 3.65 at 5 and 3.62 at 16).
// (8-bit forms: the scan is twice as fast, the candidates cost the same: 5 at k = 100.)
// Round 2, scan_gemm_f16x with hit logs, C3's per-GPU shape (profiles/sweep_frac_k100.sh): 4, 6 and 8
// are even at k = 100 (3.69-3.70 ms per step: scan 2.67 / 2.80 / 2.91 ms at 468 / 703 / 922 candidates per
// query, ~55 cycles of a workgroup per hit), 10 and up lose (12: 4.17 ms; 24 overflows the lists).
// The sample's cost grows with the bytes of the index, the candidates' does not, so the optimum
// moves up on the largest shapes (profiles/sweep_frac_big.sh, ab_frac.sh: C5 = 30 x C2's bytes: 48
// is 3-4 % faster than 16, 96 overflows the lists; 10 M x d128: +1.7 %): ~bytes^0.3 from 8 x C2's
// bytes on, k <= 32 (between C2 and that, and at k = 100, the denser hits cost the scan what the
// sample saves: 1 M x d960, 4 M x d128, 10 M x d128 k = 100 all within +-1 %).
uint32_t sample_frac_for(const expann_index* h, size_t k) {
	if (h->opt_sample_frac > 0)
		return (uint32_t)h->opt_sample_frac;
	const double expo = float_rows(h) ? 0.3 : 0.5;
	const double bytes = (double)h->n * (double)h->dim * (float_rows(h) ? 2.0 : 1.0);
	double size = (bytes >= 8 * 2.56e8 && k <= 32) ? std::min(3.0, std::pow(bytes / 2.56e8, 0.3)) : 1.0;
	// (round 3, after the hits got cheaper -- lighter flush, keys made by the gather, pruned selects --
	// profiles/sweep_frac_r3.sh: k = 100 on 1.25 M rows: 6 beats 8 by 2.3 % (3.28 vs 3.36 ms), on 10 M rows 8 - 12 are
	// even: ~bytes^0.25 from C3's per-GPU shard on)
	if (float_rows(h) && k > 32)
		size = 0.75 * std::pow(std::max(1.0, bytes / 3.2e8), 0.25);
	const double f = 16.0 * std::pow(10.0 / (double)std::max<size_t>(1, k), expo) * size;
	return (uint32_t)std::min(48.0, std::max(4.0, std::round(f)));
}

// ---- 8-bit GEMM form, queue geometry (scan_gemm_i8q.hpp), d = 128 / 256 / 768 / 832 / 960 -----
using GemmI8qFn = void (*)(GemmI8qParams);
using SelfI8AnyFn = void (*)(const void*, uint32_t, int*, uint32_t);
using ThetaI8AnyFn = void (*)(const void*, uint32_t, const float*, int*, int*, uint32_t);
struct GemmI8qVariant {
	int d, mode;
	GemmI8qFn scan, sample;
	SelfI8Fn self;
	ThetaI8Fn theta;
	const char* name;
	int dq;  // physical row bytes of the engine's copy (> d: zero-padded, scan_gemm_i8q.hpp)
	int lds, threads, wg_per_cu;
	// scan_gemm_i8w.hpp: the full scan writes per-wave hit logs (gather_logs_kernel files them)
	void (*scan_w)(GemmI8wParams) = nullptr;
	int lds_w = 0, threads_w = 0, wg_per_cu_w = 0;
	void (*sample_w)(GemmI8wParams) = nullptr;  // the sampled pass on the same stream (SAMPLE instance; same launch geometry)
	// scan_gemm_kl.hpp (d = 0): rows per tile, and the preludes that take the dim at run time
	int tb = kF16TB;
	SelfI8AnyFn self_any = nullptr;
	ThetaI8AnyFn theta_any = nullptr;
};
// the 16x16x64 kernels of the 8-waves-per-tile geometries (scan_gemm_w8.hpp, int8 instances): d = 768, and d = 832 / 960 -- rows in
// 1024-byte slots -- with DR = d (the zero-padded k-steps are left out); scan and SAMPLE instance
#define GEMM_I8X_P(D, DQ, MODE, L2F, MN) {D, MODE, scan_gemm_w8_kernel<I8Elem, DQ, false, D, L2F>, \
	scan_gemm_w8_kernel<I8Elem, DQ, true, D, L2F>, row_self_i8_kernel<D, MODE>, query_theta_i8_kernel<D, MODE>, \
	"scan_gemm_i8x<" #DQ "," MN ">", DQ, gemm_i8q_lds_bytes<DQ>(), I8qGeom<DQ>::THREADS, I8qGeom<DQ>::WG_PER_CU}
const GemmI8qVariant kGemmI8x[] = {
    GEMM_I8X_P(768, 768, kU8L2, true, "U8L2"), GEMM_I8X_P(768, 768, kI8L2, true, "I8L2"), GEMM_I8X_P(768, 768, kI8IP, false, "I8IP"),
    GEMM_I8X_P(832, 1024, kU8L2, true, "U8L2"), GEMM_I8X_P(832, 1024, kI8L2, true, "I8L2"),
    GEMM_I8X_P(832, 1024, kI8IP, false, "I8IP"),
    GEMM_I8X_P(960, 1024, kU8L2, true, "U8L2"), GEMM_I8X_P(960, 1024, kI8L2, true, "I8L2"),
    GEMM_I8X_P(960, 1024, kI8IP, false, "I8IP"),
    GEMM_I8X_P(896, 1024, kU8L2, true, "U8L2"), GEMM_I8X_P(896, 1024, kI8L2, true, "I8L2"),
    GEMM_I8X_P(896, 1024, kI8IP, false, "I8IP")};
#undef GEMM_I8X_P
// d = 128 / 256: f16x's step structure on 16x16x64 with hit logs (scan_gemm_i8w.hpp)
#define GEMM_I8W(D, MODE, L2F, MN) {D, MODE, nullptr, nullptr, row_self_i8_kernel<D, MODE>, \
	query_theta_i8_kernel<D, MODE>, "scan_gemm_i8w<" #D "," MN ">", D, gemm_i8q_lds_bytes<D>(), kF16Threads, \
	I8wGeom<D>::WG_PER_CU, scan_gemm_i8w_kernel<D, L2F>, gemm_i8w_lds_bytes<D>(), kF16Threads, I8wGeom<D>::WG_PER_CU, \
	scan_gemm_i8w_kernel<D, L2F, true>}
const GemmI8qVariant kGemmI8w[] = {
    GEMM_I8W(128, kU8L2, true, "U8L2"), GEMM_I8W(128, kI8L2, true, "I8L2"), GEMM_I8W(128, kI8IP, false, "I8IP"),
    GEMM_I8W(256, kU8L2, true, "U8L2"), GEMM_I8W(256, kI8L2, true, "I8L2"), GEMM_I8W(256, kI8IP, false, "I8IP")};
// the int8 filter of fp32 rows (scan_gemm_i8f.hpp): the d = 128 i8w full scan on the index's int8 copy
const GemmI8qVariant kGemmI8F = GEMM_I8W(128, kI8L2, true, "F32L2");
// (its redo pass of the speculative thresholds has a kernel of its own: redo_stream_i8_kernel, scan_redo_i8.hpp)
#undef GEMM_I8W
// every other 8-bit dim (multiples of 64 up to 4096): the K-loop form with the dim known at run time
// (scan_gemm_kl.hpp, int8 instances; d = 0 here, rows in the index's own d bytes, 128-row tiles, hit logs)
#define GEMM_I8KL(MODE, MN) {0, MODE, nullptr, nullptr, nullptr, nullptr, "scan_gemm_i8kl<" MN ">", 0, kKlLds, kF16Threads, 1, \
	scan_gemm_kl_kernel<I8Elem, false>, kKlLds, kF16Threads, 1, scan_gemm_kl_kernel<I8Elem, true>, kKlTB, \
	row_self_i8_any_kernel<MODE>, query_theta_i8_any_kernel<MODE>}
const GemmI8qVariant kGemmI8KL[] = {GEMM_I8KL(kU8L2, "U8L2"), GEMM_I8KL(kI8L2, "I8L2"), GEMM_I8KL(kI8IP, "I8IP")};
#undef GEMM_I8KL
constexpr int kRetryGeneric = -1000;  // internal: the caller falls back to the threshold ladder
constexpr int kStrictReject = -1001;  // internal (uint8 shadow): these queries are not 8-bit integers

// the variant of a plan's q-form family (bf_plan.hpp)
const GemmI8qVariant* find_gemm_i8q(ScanFamily f, int d, int mode) {
	for (const auto& v : kGemmI8w)
		if (f == ScanFamily::kI8qW && v.d == d && v.mode == mode)
			return &v;
	for (const auto& v : kGemmI8x)
		if (f == ScanFamily::kI8qX && v.d == d && v.mode == mode)
			return &v;
	for (const auto& v : kGemmI8KL)
		if (f == ScanFamily::kI8qKL && v.mode == mode)
			return &v;
	return nullptr;
}

// Do the variant tables hold what bf_plan.hpp lists as compiled -- every entry listed, and as many as listed?
// (checked once, at the first expann_create: the planner answers from its lists, the launches from these tables)
static_assert(kI8MinRows == 2 * 256 * kF16TB, "bf_plan.hpp: two 256-tile chunks of the int8 hit-log forms");
bool plan_tables_match() {
	bool ok = kGemmF16XDbg[0].d == kF16DbgDim && kGemmI8F.d == kI8fDim;
	auto all = [&ok](const auto& tab, size_t listed, auto in) {
		size_t hits = 0;
		for (const auto& v : tab)
			hits += in(v) ? 1 : 0;
		ok = ok && hits == std::size(tab) && hits == listed;
	};
	const auto mfma_mode = [](int mode) { return mode == kU8L2 || mode == kI8L2 || mode == kI8IP; };
	all(kScanF32, 2 * count_tiles(kScanF32Tiles, std::size(kScanF32Tiles)),
	    [](const ScanVariant& v) { return has_tile(tiles_of(kScanF32Tiles, v.d), v.tq); });
	all(kScanF32Any, 2 * count_tiles(&kScanF32AnyTiles, 1), [](const ScanVariant& v) { return has_tile(&kScanF32AnyTiles, v.tq); });
	all(kScanI8, 4 * count_tiles(kScanI8Tiles, std::size(kScanI8Tiles)) + count_tiles(kScanI16Tiles, std::size(kScanI16Tiles)),
	    [](const ScanI8Variant& v) {
		    return has_tile(v.mode == kI16L2Ref ? tiles_of(kScanI16Tiles, v.d) : tiles_of(kScanI8Tiles, v.d), v.tq);
	    });
	all(kScanI8Any, 4 * count_tiles(&kScanI8AnyTiles, 1), [](const ScanI8Variant& v) { return has_tile(&kScanI8AnyTiles, v.tq); });
	all(kDirectF16, count_tiles(kDirectF16Tiles, std::size(kDirectF16Tiles)),
	    [](const DirectF16Variant& v) { return has_tile(tiles_of(kDirectF16Tiles, v.d), v.tq); });
	all(kGemmF16X, std::size(kF16XDims) + std::size(kF16YDims) + std::size(kF16KXDims), [](const GemmF16Variant& v) {
		return (has_dim(kF16XDims, v.d) && v.scan_redo) || has_dim(kF16YDims, v.d) || has_dim(kF16KXDims, v.d);
	});
	all(kGemmBf16, std::size(kBf16Dims), [](const GemmBf16Variant& v) { return has_dim(kBf16Dims, v.d); });
	all(kGemmI8, 3 * std::size(kGemmI8Dims), [&](const GemmI8Variant& v) { return has_dim(kGemmI8Dims, v.d) && mfma_mode(v.mode); });
	all(kGemmI8w, 3 * std::size(kI8qWDims), [&](const GemmI8qVariant& v) { return has_dim(kI8qWDims, v.d) && mfma_mode(v.mode); });
	all(kGemmI8x, 3 * std::size(kI8qXDims), [&](const GemmI8qVariant& v) { return has_dim(kI8qXDims, v.d) && mfma_mode(v.mode); });
	all(kGemmI8KL, 3, [&](const GemmI8qVariant& v) { return v.d == 0 && mfma_mode(v.mode); });
	return ok;
}

// int8 filter of fp32 rows: clip of the scale (s = min(max |x|, kI8fClipRms rms) / 127)
constexpr double kI8fClipRms = 5.5;
// ... and the share of the index's energy below which the components within that clip, not all of them, set the rms
// (ensure_i8f): far below anything rows of one population give (tests' 10 rows x 50 plus 200 components up to 200
// among 40 000 rows: 0.47)
constexpr double kI8fTrimEnergy = 1.0 / 16.0;
// its lists over the expectation 1.2 x rank x frac per query on iid rows, rank = k or the speculative threshold's j
// (C2: 501.3 at rank 10 = 2.61 x, 214.6 at rank 4 = 2.79 x; the fp16 form measures 176.5 and 69.9): the select's
// stages are sized by it
constexpr double kI8fListRatio = 2.8;
// ... and where it stops paying: at C2's shape the form gains 0.36 ms per step at 501 candidates per query (iid rows)
// and loses 0.67 ms at 963 (1 000 clusters); the straight line between crosses at ~660 = 3.4 x 1.2 k frac
// (measured with proven thresholds; under a speculative threshold of rank j the limit scales with j / k as the
// lists do -- i8f_cand_limit -- and the clustered rows still pass it on their first search)
constexpr double kI8fBreakEvenRatio = 3.4;
// Candidates of one search above which the int8 filter loses to the fp16 form (kI8fBreakEvenRatio): rows in tight
// clusters give it far longer lists than iid rows do.  Past this total an auto search turns the form off for the
// index (i8f_state 2, until set_base_device brings other rows): the rows, not the shape, decided, and they do not
// change between searches.
// (speculative thresholds: the lists' expectation is linear in the rank j of the class maximum, so is the limit)
uint64_t i8f_cand_limit(const expann_index* h, size_t m, size_t k, uint32_t spec_j = 0) {
	const double rank = spec_j ? (double)spec_j : (double)k;
	return (uint64_t)(kI8fBreakEvenRatio * 1.2 * rank * sample_frac_for(h, k) * (double)m);
}

// the index side of the int8 filter: scale from the rows' rms and max |x| (one fp64 reduction), the padded
// int8 copy, bp and w_b per row (i8f_rows_kernel)
int ensure_i8f(expann_index* h, hipStream_t st) {
	if (h->i8f_state != 0)
		return EXPANN_OK;
	const size_t nv = h->n * (size_t)h->dim;
	DevBuf tmp;
	HIP_TRY(h, tmp.alloc(16));
	HIP_TRY(h, hipMemsetAsync(tmp.p, 0, 16, st));
	hipLaunchKernelGGL(i8f_stats_kernel, dim3(2048), dim3(kBlock), 0, st, (const float*)h->d_base, nv, tmp.as<double>(),
	                   reinterpret_cast<uint32_t*>(tmp.as<double>() + 1));
	unsigned char hb[16];
	float bnmax = 0.0f;  // (the fp16 prelude's largest ||b||^2: B of the analysis)
	HIP_TRY(h, hipMemcpyAsync(hb, tmp.p, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipMemcpyAsync(&bnmax, h->d_bnmax + 2, sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));
	double sumsq;
	float maxabs;
	std::memcpy(&sumsq, hb, 8);
	std::memcpy(&maxabs, hb + 8, 4);
	double rms = std::sqrt(sumsq / (double)nv);
	float clip = (float)std::min<double>(maxabs, kI8fClipRms * rms);
	if (maxabs > clip && std::isfinite(clip) && clip > 0.0f) {
		// a few far-out rows may carry nearly all the energy (eight rows of 1e4 x N(0, 1) among 266 240 of N(0, 1): rms
		// 54, a scale 50 x too coarse for every other row, whose lists then overflow on every search): where the
		// components within the clip hold less than kI8fTrimEnergy of it, the scale comes from THEIR rms -- the
		// far-out rows are clipped (or their row term clamped) and always re-scored, as any clipped row is
		HIP_TRY(h, hipMemsetAsync(tmp.p, 0, 16, st));
		hipLaunchKernelGGL(i8f_trimmed_stats_kernel, dim3(2048), dim3(kBlock), 0, st, (const float*)h->d_base, nv, clip,
		                   tmp.as<double>(), reinterpret_cast<unsigned long long*>(tmp.as<double>() + 1));
		HIP_TRY(h, hipMemcpyAsync(hb, tmp.p, 16, hipMemcpyDeviceToHost, st));
		HIP_TRY(h, hipStreamSynchronize(st));
		double sumsq_in;
		unsigned long long n_in;
		std::memcpy(&sumsq_in, hb, 8);
		std::memcpy(&n_in, hb + 8, 8);
		if (n_in > 0 && sumsq_in < kI8fTrimEnergy * sumsq) {
			rms = std::sqrt(sumsq_in / (double)n_in);
			clip = (float)std::min<double>(maxabs, kI8fClipRms * rms);
		}
	}
	if (!(clip > 0.0f) || !std::isfinite(clip) || !std::isfinite(rms) || !std::isfinite(bnmax)) {
		h->i8f_state = -1;
		return EXPANN_OK;
	}
	h->i8f = i8f_consts(clip / 127.0f, (float)rms, bnmax, h->dim);
	const size_t n_pad = (h->n + kF16TB - 1) / kF16TB * kF16TB;
	HIP_TRY(h, hipMalloc(&h->d_base_i8f, n_pad * (size_t)h->dim));
	HIP_TRY(h, hipMalloc(&h->d_bp_i8f, sizeof(int) * n_pad));
	HIP_TRY(h, hipMalloc(&h->d_rw_i8f, sizeof(float) * h->n));
	HIP_TRY(h, hipMalloc(&h->d_cb_i8f, sizeof(int) * n_pad));
	HIP_TRY(h, hipMalloc(&h->d_wbmax_i8f, sizeof(float)));
	HIP_TRY(h, hipMemsetAsync(h->d_base_i8f, 0, n_pad * (size_t)h->dim, st));
	HIP_TRY(h, hipMemsetAsync(h->d_wbmax_i8f, 0, sizeof(float), st));
	static_assert(kI8fCbNone == kI8qPadBp, "the padding's row term serves both passes");
	for (int* terms : {h->d_bp_i8f.as<int>(), h->d_cb_i8f.as<int>()})  // (the padding: kI8qPadBp)
		hipLaunchKernelGGL(i8q_bp_kernel, dim3((uint32_t)((n_pad + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   (const int*)nullptr, (uint32_t)h->n, (uint32_t)n_pad, terms);
	hipLaunchKernelGGL(i8f_rows_kernel<128>, dim3((uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup)), dim3(kBlock), 0,
	                   st, (const float*)h->d_base, (uint32_t)h->n, h->i8f, h->d_base_i8f.as<int8_t>(),
	                   h->d_bp_i8f.as<int>(), h->d_rw_i8f.as<float>(), h->d_cb_i8f.as<int>());
	hipLaunchKernelGGL(i8f_wbmax_kernel, dim3(1024), dim3(kBlock), 0, st, h->d_rw_i8f.as<const float>(), h->d_cb_i8f.as<const int>(),
	                   (uint32_t)h->n, reinterpret_cast<uint32_t*>(h->d_wbmax_i8f.as<float>()));
	HIP_TRY(h, hipGetLastError());
	h->i8f_state = 1;
	return EXPANN_OK;
}

int ensure_i8q(expann_index* h, const GemmI8qVariant* gq, hipStream_t st) {
	if (h->d_base_i8q)
		return EXPANN_OK;
	const size_t n_pad = (h->n + gq->tb - 1) / gq->tb * gq->tb;
	const int dq = gq->dq ? gq->dq : h->dim;  // (the run-time-dim form keeps the index's row length)
	if (h->int_mode != kI8IP && !h->d_bias_i) {
		HIP_TRY(h, hipMalloc(&h->d_bias_i, sizeof(int) * h->n));
		const dim3 grid((uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup));
		if (gq->self_any)
			hipLaunchKernelGGL(gq->self_any, grid, dim3(kBlock), 0, st, (const void*)h->d_base, (uint32_t)h->n,
			                   h->d_bias_i.as<int>(), (uint32_t)h->dim);
		else
			hipLaunchKernelGGL(gq->self, grid, dim3(kBlock), 0, st, (const void*)h->d_base, (uint32_t)h->n, h->d_bias_i);
	}
	HIP_TRY(h, hipMalloc(&h->d_bp_i8q, sizeof(int) * n_pad));
	hipLaunchKernelGGL(i8q_bp_kernel, dim3((uint32_t)((n_pad + kBlock - 1) / kBlock)), dim3(kBlock), 0,
	                   st, h->int_mode != kI8IP ? h->d_bias_i.as<const int>() : (const int*)nullptr,
	                   (uint32_t)h->n, (uint32_t)n_pad, h->d_bp_i8q);
	if (dq != h->dim) {
		// own copy with rows padded to dq bytes (zeros in the int8 domain), whole 64-row tiles
		void* copy = nullptr;
		HIP_TRY(h, hipMalloc(&copy, n_pad * (size_t)dq));
		hipLaunchKernelGGL(i8q_pad_rows_kernel, dim3(8192), dim3(kBlock), 0, st, (const uint32_t*)h->d_base, h->n,
		                   (uint32_t)h->dim / 4, (uint32_t)dq / 4, n_pad,
		                   h->int_mode == kU8L2 ? 0x80808080u : 0u, (uint32_t*)copy);
		h->d_base_i8q.own(copy);
	} else if (h->int_mode == kU8L2 || n_pad != h->n) {
		// own copy: whole 64-row tiles (zero rows behind the end), uint8 rows mapped to int8
		void* copy = nullptr;
		HIP_TRY(h, hipMalloc(&copy, n_pad * (size_t)h->dim));
		const size_t words = h->n * (size_t)h->dim / 4, words_pad = n_pad * (size_t)h->dim / 4;
		hipLaunchKernelGGL(i8q_copy_xor_kernel, dim3(4096), dim3(kBlock), 0, st, (const uint32_t*)h->d_base,
		                   words, words_pad, h->int_mode == kU8L2 ? 0x80808080u : 0u, (uint32_t*)copy);
		h->d_base_i8q.own(copy);
	} else {
		h->d_base_i8q.borrow(h->d_base);
	}
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

// sample pass -> thresholds -> full scan -> select, all in the g domain (scan_gemm_i8q.hpp)
int search_i8q(expann_index* h, const GemmI8qVariant* gq, const void* d_queries, size_t m, size_t k,
               uint64_t* d_ids, float* d_dists, hipStream_t st, uint32_t cap) {
	const int cus = num_cus(h->device);
	const bool dbg = std::getenv("EXPANN_DEBUG_SYNC") != nullptr;
	auto mark = [&](const char* what) {
		if (dbg) {
			const hipError_t e = hipStreamSynchronize(st);
			std::fprintf(stderr, "[i8q] %s: %s\n", what, hipGetErrorString(e));
			std::fflush(stderr);
		}
	};
	int rc = ensure_i8q(h, gq, st);
	mark("ensure_i8q");
	if (rc != EXPANN_OK)
		return rc;
	const void* q8 = d_queries;
	const int dq = gq->dq ? gq->dq : h->dim;
	if (dq != h->dim) {  // rows of the padded geometry: queries padded (and mapped) the same way
		const size_t nb = m * (size_t)dq;
		HIP_TRY(h, grow_ws(h, h->d_q_split, nb));
		hipLaunchKernelGGL(i8q_pad_rows_kernel, dim3((uint32_t)std::min<size_t>((nb / 4 + kBlock - 1) / kBlock, 1024)),
		                   dim3(kBlock), 0, st, (const uint32_t*)d_queries, m, (uint32_t)h->dim / 4,
		                   (uint32_t)dq / 4, m, h->int_mode == kU8L2 ? 0x80808080u : 0u,
		                   h->d_q_split.as<uint32_t>());
		q8 = h->d_q_split;
	} else if (h->int_mode == kU8L2) {  // queries ^ 0x80 (d_queries is the uint8 conversion, d_q8)
		const size_t nb = m * (size_t)h->dim;
		HIP_TRY(h, grow_ws(h, h->d_q_split, nb));
		hipLaunchKernelGGL(i8q_copy_xor_kernel, dim3((uint32_t)std::min<size_t>((nb / 4 + kBlock - 1) / kBlock, 1024)),
		                   dim3(kBlock), 0, st, (const uint32_t*)d_queries, nb / 4, nb / 4, 0x80808080u,
		                   h->d_q_split.as<uint32_t>());
		q8 = h->d_q_split;
	}
	const uint32_t nt = (uint32_t)((h->n + gq->tb - 1) / gq->tb);
	const uint32_t run = (uint32_t)h->opt_sample_run;
	// (at least 256 tiles of 64 rows: the same rows with the 128-row tiles of the run-time-dim form)
	const uint32_t t_sel = std::max<uint32_t>(256 * kF16TB / gq->tb, nt / sample_frac_for(h, k)) / run * run;
	const uint32_t nqt = (uint32_t)((m + kF16TQ - 1) / kF16TQ);
	const uint32_t wg_slots = (uint32_t)(gq->sample_w ? gq->wg_per_cu_w : gq->wg_per_cu) * (uint32_t)cus;
	uint32_t chunks = std::max<uint32_t>(1, wg_slots / nqt);
	chunks = std::max<uint32_t>(chunks, (uint32_t)((8 * k + 31) / 32));
	chunks = std::min<uint32_t>(chunks, std::min<uint32_t>(64, t_sel / 4));
	if (t_sel * 2 > nt || (size_t)chunks * 32 < 8 * k)
		return kRetryGeneric;
	const int lds = gq->lds;
	const dim3 wg((uint32_t)gq->threads);
	for (int attempt = 0;; ++attempt) {
		rc = ensure_workspace(h, m, cap);
		if (rc != EXPANN_OK)
			return rc;
		HIP_TRY(h, hipMemsetAsync(h->d_overflow, 0, sizeof(uint32_t), st));
		HIP_TRY(h, hipMemsetAsync(h->d_total, 0, sizeof(unsigned long long) * 2, st));
		if (h->int_mode != kI8IP && gq->theta_any)
			hipLaunchKernelGGL(gq->theta_any, dim3((uint32_t)((m + kRowsPerGroup - 1) / kRowsPerGroup)),
			                   dim3(kBlock), 0, st, d_queries, (uint32_t)m, (const float*)nullptr,
			                   (int*)nullptr, h->d_qself.as<int>(), (uint32_t)h->dim);
		else if (h->int_mode != kI8IP)
			hipLaunchKernelGGL(gq->theta, dim3((uint32_t)((m + kRowsPerGroup - 1) / kRowsPerGroup)),
			                   dim3(kBlock), 0, st, d_queries, (uint32_t)m, (const float*)nullptr,
			                   (int*)nullptr, h->d_qself);
		HIP_TRY(h, grow_ws(h, h->d_sample, m * (size_t)chunks * 32 * sizeof(int)));
		GemmI8qParams sp{};
		sp.base = h->d_base_i8q;
		sp.bp = h->d_bp_i8q;
		sp.bias = h->int_mode != kI8IP ? h->d_bias_i : nullptr;
		sp.n_rows = (uint32_t)h->n;
		sp.n_tiles_sel = t_sel;
		sp.tile_stride = nt / t_sel;
		sp.tile_run = run;
		sp.tiles_per_block = (t_sel + chunks - 1) / chunks;
		const uint32_t schunks = (t_sel + sp.tiles_per_block - 1) / sp.tiles_per_block;
		sp.n_qtiles = nqt;
		sp.queries = q8;
		sp.m = (uint32_t)m;
		sp.sample_out = h->d_sample.as<int>();
		sp.n_chunks = schunks;
		sp.ksteps = (uint32_t)h->dim / 64;
		if (dbg)
			std::fprintf(stderr, "[i8q] sample: grid %u x %u, t_sel %u stride %u tpb %u chunks %u nt %u m %zu base %p bp %p q %p out %p (%zu B)\n",
			             schunks, nqt, t_sel, sp.tile_stride, sp.tiles_per_block, schunks, nt, m, sp.base,
			             (const void*)sp.bp, sp.queries, (void*)sp.sample_out, h->d_sample.bytes);
		mark("qself");
		if (gq->sample_w) {
			GemmI8wParams wsp{};
			wsp.q = sp;
			hipLaunchKernelGGL(gq->sample_w, dim3(schunks * nqt), dim3((uint32_t)gq->threads_w), gq->lds_w, st, wsp);
		} else {
			hipLaunchKernelGGL(gq->sample, dim3(schunks * nqt), wg, lds, st, sp);
		}
		mark("sample");
		SampleTauI8Params tp{};
		tp.vals = h->d_sample.as<const int>();
		tp.n_vals = schunks * 32;
		tp.m = (uint32_t)m;
		tp.k = (uint32_t)k;
		tp.thp = h->d_theta.as<int>();
		tp.cand_cnt = h->d_cnt;
		hipLaunchKernelGGL(tp.n_vals <= 512 ? sample_tau_i8_kernel<8>
		                                   : (tp.n_vals <= 1024 ? sample_tau_i8_kernel<16> : sample_tau_i8_kernel<32>),
		                   dim3((uint32_t)((m + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, tp);
		mark("tau");
		// the full scan
		GemmI8qParams fp = sp;
		fp.sample_out = nullptr;
		fp.n_tiles_sel = nt;
		fp.tile_stride = 1;
		fp.tile_run = 1;
		fp.thp = h->d_theta.as<const int>();
		fp.qself = h->d_qself;
		fp.cand_cnt = h->d_cnt;
		fp.cand = h->d_cand;
		fp.cap = cap;
		// (a retry after overflowed logs / lists stays on the same kernel: the logs grow with the lists)
		const GemmI8qVariant* gs = gq;
		const uint32_t scan_slots = gs->scan_w ? (uint32_t)gs->wg_per_cu_w * (uint32_t)cus : wg_slots;
		uint32_t fchunks = pick_row_chunks(nt, nqt, scan_slots, 4.0, 8, 2048, h->opt_xcd_tolerance,
		                                   (h->opt_debug & 1024) ? nullptr : &fp.xcd_map);
		fp.tiles_per_block = (nt + fchunks - 1) / fchunks;
		fchunks = (nt + fp.tiles_per_block - 1) / fp.tiles_per_block;
		GemmI8wParams wp{};
		if (gs->scan_w) {  // four hit logs per workgroup, one per 64 queries of its tile (may wait for the stream to grow them)
			wp.q = fp;
			rc = ensure_hit_logs(h, fchunks * nqt, 4, m, cap, fchunks, nqt, fp.xcd_map, st, &wp.log, &wp.log_cnt,
			                     &wp.log_cap);
			if (rc != EXPANN_OK)
				return rc;
			wp.lost = h->d_overflow;
			h->pending_scatter.i_thp = fp.thp;
			h->pending_scatter.i_bias = fp.bias;
			h->pending_scatter.i_qself = fp.qself;
			h->pending_scatter.i_mode = fp.bias ? 1 : 2;
		}
		const bool timed = h->profiling && h->ev_used < kEventPairs;
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		if (gs->scan_w)
			hipLaunchKernelGGL(gs->scan_w, dim3(fchunks * nqt), dim3((uint32_t)gs->threads_w), gs->lds_w, st, wp);
		else
			hipLaunchKernelGGL(gs->scan, dim3(fchunks * nqt), dim3((uint32_t)gs->threads), gs->lds, st, fp);
		if (timed) {
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][1], st));
			h->ev_used++;
		}
		launch_gather_logs(h, st);
		if (timed || !h->profiling) {
			h->prof.scan_launches++;
			h->prof.scan_rows += h->n;
			h->prof.scan_query_tiles += nqt;
			h->prof.query_tile = kF16TQ;
			h->prof.levels = 2;
			std::snprintf(h->prof.scan_kernel, sizeof(h->prof.scan_kernel), "%s", gs->name);
		}
		HIP_TRY(h, hipGetLastError());
		mark("scan");
		SelectParams sel{};
		sel.cand = h->d_cand;
		sel.cand_cnt = h->d_cnt;
		sel.cap = cap;
		sel.k = (uint32_t)k;
		sel.id_offset = h->id_offset;
		sel.out_ids = d_ids;
		sel.out_dists = d_dists;
		sel.dim = (uint32_t)h->dim;
		sel.overflow = h->d_overflow;
		if (h->profiling)
			hipLaunchKernelGGL(sum_u32_kernel, dim3(1), dim3(1024), 0, st, sel.cand_cnt, (uint32_t)m,
			                   h->d_total);
		launch_select_wave(sel, m, cap, st, select_longest_list(1.2 * (double)k * sample_frac_for(h, k), 0));
		mark("select_wave");
		hipLaunchKernelGGL(select_topk_kernel<float>, dim3((uint32_t)m), dim3(kBlock), sizeof(uint64_t) * cap + 16,
		                   st, sel);
		HIP_TRY(h, hipGetLastError());
		if (defer_flags(h, st, attempt)) {  // deferred check: expann_sync reads the flags
			h->h_flag_ring[kRingWords * (h->async_pending - 1) + kRingScale] = 0;
			return EXPANN_OK;
		}
		HIP_TRY(h, hipMemcpyAsync(h->h_flags, h->d_overflow, sizeof(uint32_t) * 4 + sizeof(unsigned long long),
		                          hipMemcpyDeviceToHost, st));
		HIP_TRY(h, hipStreamSynchronize(st));
		unsigned long long tot;
		std::memcpy(&tot, h->h_flags + 4, sizeof(tot));
		h->prof.candidates = tot;
		if (h->strict_u8 && (h->h_flags[1] != 0 || h->h_flags[3] != 0))
			return kStrictReject;
		if (h->dtype == EXPANN_DTYPE_U8 && h->h_flags[1] != 0)
			return h->fail(EXPANN_ERR_UNSUPPORTED,
			               std::to_string(h->h_flags[1]) +
			                   " query values outside [0,255]: the uint8 metric "
			                   "(dist2_compressed) is only defined for 8-bit valued queries");
		if (h->h_flags[0] == 0)
			return EXPANN_OK;
		h->prof.retries++;
		if (cap >= kMaxCap || attempt >= 2)
			return kRetryGeneric;  // massive ties: the ladder's direct kernel breaks them by row
		cap = std::min(cap * 4, kMaxCap);
	}
}

int search_pass(expann_index* h, const void* d_queries, size_t m, size_t k, uint64_t* d_ids,
                float* d_dists, hipStream_t st);

// Exact-uint8 shortcut of an fp32 index (fields of expann_index): examine the rows once; if all
// are integers in [0, 255] keep a uint8 copy behind an internal uint8 engine.
int build_u8_shadow(expann_index* h, hipStream_t st) {
	const size_t nv = h->n * (size_t)h->dim;
	DevBuf bad;
	HIP_TRY(h, bad.alloc(sizeof(uint32_t)));
	HIP_TRY(h, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), st));
	hipLaunchKernelGGL(count_non_u8_kernel, dim3(2048), dim3(kBlock), 0, st, (const float*)h->d_base, nv,
	                   bad.as<uint32_t>());
	uint32_t n_bad = 1;
	HIP_TRY(h, hipMemcpyAsync(&n_bad, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));
	if (n_bad != 0) {
		h->u8_exact = -1;
		return EXPANN_OK;
	}
	HIP_TRY(h, hipMalloc(&h->d_base_u8, nv));
	hipLaunchKernelGGL(cast_f32_u8_kernel, dim3(4096), dim3(kBlock), 0, st, (const float*)h->d_base, nv,
	                   h->d_base_u8.as<uint8_t>());
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipStreamSynchronize(st));
	expann_index* sh = nullptr;
	int rc = expann_create(h->dim, EXPANN_DTYPE_U8, EXPANN_METRIC_L2, h->device, &sh);
	if (rc == EXPANN_OK)
		rc = expann_set_base_device(sh, h->d_base_u8, h->n, h->id_offset);
	if (rc == EXPANN_OK && h->profiling)
		rc = expann_set_profiling(sh, 1);
	if (rc != EXPANN_OK) {
		if (sh)
			expann_destroy(sh);
		h->d_base_u8.reset();
		h->u8_exact = -1;  // (not fatal: the fp32 paths serve the index)
		return EXPANN_OK;
	}
	sh->strict_u8 = true;
	h->u8_shadow.reset(sh);
	h->u8_exact = 1;
	return EXPANN_OK;
}
void drop_u8_shadow(expann_index* h) { h->forget<U8Shadow>(); }
// the shadow's counters and scan time become the parent's
int absorb_shadow_profile(expann_index* h) {
	expann_index* sh = h->u8_shadow.get();
	double ms = 0;
	for (int i = 0; i < sh->ev_used; ++i) {
		HIP_TRY(h, hipEventSynchronize(sh->ev[i][1]));
		float t = 0;
		HIP_TRY(h, hipEventElapsedTime(&t, sh->ev[i][0], sh->ev[i][1]));
		ms += t;
	}
	sh->ev_used = 0;
	h->prof_extra_ms += ms;
	h->prof.scan_launches += sh->prof.scan_launches;
	h->prof.scan_rows += sh->prof.scan_rows;
	h->prof.scan_query_tiles += sh->prof.scan_query_tiles;
	h->prof.retries += sh->prof.retries;
	h->prof.deferred_searches += sh->prof.deferred_searches;
	h->prof.query_tile = sh->prof.query_tile;
	h->prof.levels = sh->prof.levels;
	h->prof.candidates = sh->prof.candidates;
	std::memcpy(h->prof.scan_kernel, sh->prof.scan_kernel, sizeof(h->prof.scan_kernel));
	sh->prof = expann_profile{};
	return EXPANN_OK;
}

// One sampled pass of the fp16 form gives every query the threshold of its full scan (4.6 of
// DESIGN.md): class maxima of g over 1/frac of the rows, their k-th largest -> tau, theta', and
// the list counters zeroed.  A handful of queries (dv, the plan's scan_direct_f16 variant): sampled pass and
// thresholds in ONE launch (scan_direct_f16.hpp); otherwise the MFMA SAMPLE kernel + sample_tau_kernel.  *done stays false
// when the index is too small for a sample (the caller runs the threshold ladder instead).
int sampled_pass_f16(expann_index* h, const GemmF16Variant* gvf, const DirectF16Variant* dv, size_t m, size_t k, bool ip,
                     int cus, float* d_tau, uint32_t* d_tau_row, hipStream_t st, bool* done, bool i8f, bool* i8f_done,
                     uint32_t* spec_j) {
	*done = false;
	*i8f_done = false;
	// speculative thresholds (*spec_j != 0 on entry: this search may have them): the MFMA SAMPLE pass below decides
	// the rank from the share of the rows it reads; the fused direct pass keeps proven thresholds
	const bool spec_ok = *spec_j != 0;
	*spec_j = 0;
	auto ensure_sample = [&](size_t need) -> int {
		HIP_TRY(h, grow_ws(h, h->d_sample, need));
		return EXPANN_OK;
	};
	SampleTauParams tp{};
	tp.m = (uint32_t)m;
	tp.k = (uint32_t)k;
	tp.qnrm = h->d_qnrm;
	tp.eps = gemm_f16_filter_eps(h->dim);
	tp.abs_coef = std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim);
	tp.inv_mul = 2.0f / (h->f16_scale * h->f16_scale);
	tp.ip = ip ? 1 : 0;
	tp.qscale = ip ? h->d_qscale.as<const float>() : nullptr;
	tp.tau = d_tau;
	tp.tau_row = d_tau_row;
	tp.theta = h->d_theta;
	tp.mul = 0.5f * h->f16_scale * h->f16_scale;
	tp.cand_cnt = h->d_cnt;
	if (i8f) {  // the int8 filter's thresholds from the same tau (scan_gemm_i8f.hpp)
		tp.i8_aq = h->d_i8f_q;
		tp.i8_wq_in = h->d_i8f_q + h->i8f_q_m;
		tp.i8_wq = h->d_i8f_q + 2 * h->i8f_q_m;
		tp.i8_thp = reinterpret_cast<int*>(h->d_i8f_q + 3 * h->i8f_q_m);
		tp.i8_inv_2s2 = h->i8f.inv_2s2;
	}

	// Row filter: the sample sees allowed rows only (masked row terms), so it is sized by them.  The thresholds
	// are the k-th largest of the class maxima, a class being (chunk, row mod 32) -- (workgroup, row mod RPS) in
	// the fused pass.  They are finite when k classes hold an allowed row and tight when the sample's best rows
	// seldom share a class: the sample is widened until it holds 8 k allowed rows in expectation (the unfiltered
	// plan's 8 k classes of >= 1 row), and the classes a filter can fill -- it may leave whole residues empty, all
	// but one when it allows every 32nd row -- must number 2 k: the k-th of C classes is then reached after
	// C ln(C / (C - k)) <= 1.39 k rows of the sample, lists 1.4 times the usual at worst.  Otherwise no sampled
	// pass: the ladder (plan_levels_filtered) serves.
	const bool filt = h->filter_on;
	const double dens = filt ? (double)h->n_allowed / (double)h->n : 1.0;
	const size_t need_classes = filt ? 2 * k : 8 * k;
	const DirectF16Variant* dvs = i8f ? nullptr : dv;
	if (dvs && dvs->sample) {
		const uint32_t steps_all = (uint32_t)((h->n + dvs->rps - 1) / dvs->rps);
		uint32_t sel =
		    std::max<uint32_t>(256u * 64u / (uint32_t)dvs->rps, steps_all / sample_frac_for(h, k));
		uint32_t live_cpw = (uint32_t)dvs->cpw;  // classes of a workgroup that can hold an allowed row
		if (filt) {
			sel = std::max<uint32_t>(sel, (uint32_t)std::min<double>(steps_all, std::ceil(8.0 * (double)k / (dvs->rps * dens))));
			uint32_t res = h->filter_residues;
			for (int w = 32; w > dvs->rps; w >>= 1)  // residues mod RPS (RPS = 64: at least those mod 32)
				res = (res | (res >> (w / 2))) & ((1u << (w / 2)) - 1u);
			live_cpw = (uint32_t)__builtin_popcount(res);
		}
		uint32_t wgs = std::min<uint32_t>(2048u / (uint32_t)dvs->cpw, sel / 4);
		if (sel * 2 <= steps_all && (size_t)wgs * live_cpw >= need_classes) {
			SampleDirectParams sp{};
			sp.g.base_f16 = h->d_base_f16;
			sp.g.bnorm = h->bns_f16();  // upper row term: thresholds hold row by row
			sp.g.n_rows = (uint32_t)h->n;
			sp.g.n_tiles_sel = sel;
			sp.g.tile_stride = steps_all / sel;
			sp.g.tiles_per_block = (sel + wgs - 1) / wgs;
			wgs = (sel + sp.g.tiles_per_block - 1) / sp.g.tiles_per_block;
			sp.g.queries_f16 = h->d_q_split;
			sp.g.m = (uint32_t)m;
			const int ra = ensure_sample(m * (size_t)wgs * dvs->cpw * sizeof(float));
			if (ra != EXPANN_OK)
				return ra;
			sp.t = tp;
			sp.t.vals = h->d_sample;
			sp.t.n_vals = wgs * (uint32_t)dvs->cpw;
			sp.ticket = h->d_ticket;
			DevBuf sclk;
			if (h->opt_debug & 16) {
				HIP_TRY(h, sclk.alloc(3 * 8));
				sp.g.clk = sclk.as<unsigned long long>();
			}
			hipLaunchKernelGGL(dvs->sample, dim3(wgs), dim3(kBlock), 0, st, sp);
			HIP_TRY(h, hipGetLastError());
			if (sp.g.clk) {
				unsigned long long c[3] = {0, 0, 0};
				HIP_TRY(h, hipStreamSynchronize(st));
				HIP_TRY(h, hipMemcpy(c, sp.g.clk, sizeof(c), hipMemcpyDeviceToHost));
				std::fprintf(stderr, "sample_direct_f16: %u workgroups, stream %.2f us, thresholds %.2f us\n", wgs,
				             (double)(c[1] - c[0]) / 100.0, (double)(c[2] - c[1]) / 100.0);
			}
			*done = true;
			return EXPANN_OK;
		}
	}
	const uint32_t nt = (uint32_t)((h->n + gvf->tb - 1) / gvf->tb);
	const uint32_t run = (uint32_t)h->opt_sample_run;
	uint32_t t_want = std::max<uint32_t>(256, nt / sample_frac_for(h, k));
	const uint32_t live_res = filt ? (uint32_t)__builtin_popcount(h->filter_residues) : 32u;
	if (filt)
		t_want = std::max<uint32_t>(t_want, (uint32_t)std::min<double>(nt, std::ceil(8.0 * (double)k / (gvf->tb * dens))));
	const uint32_t t_sel = t_want / run * run;
	const uint32_t nqt = (uint32_t)((m + gvf->wgq - 1) / gvf->wgq);
	// A speculating int8-filter search: the sampled pass on the int8 matrix cores too (scan_gemm_i8f.hpp, "Sampled
	// pass on int8"; option "i8_sample") -- the SAMPLE instance of the full scan's kernel over the same tiles, centre
	// row terms in place of bp, chunks as search_i8q picks them (C2: 19, 608 class maxima and the <16> tau instance;
	// capped at 16 to keep the <8> instance the step measured the same, 1.368-1.371 against 1.367-1.373 ms).  tau_s is
	// an estimate the select checks; the proven tau for the redo pass comes from the same maxima.
	if (i8f && spec_ok && !filt && gvf->tb == kF16TB && gvf->wgq == kF16TQ && h->opt_i8_sample > 0 &&
	    (h->opt_i8_sample == 2 || h->opt_spec_rank == 0)) {
		const uint32_t j = h->opt_spec_rank > 0 ? (uint32_t)std::min<size_t>((size_t)h->opt_spec_rank, k)
		                                        : spec_rank_auto(k, (double)t_sel / (double)nt);
		uint32_t ic = std::max<uint32_t>(1, ((uint32_t)kGemmI8F.wg_per_cu_w * (uint32_t)cus) / nqt);
		ic = std::max<uint32_t>(ic, (uint32_t)((8 * k + 31) / 32));
		ic = std::min<uint32_t>(ic, std::min<uint32_t>(64, t_sel / 4));
		if (j < k && t_sel * 2 <= nt && (size_t)ic * 32 >= 8 * k) {
			GemmI8wParams wsp{};
			GemmI8qParams& sp = wsp.q;
			sp.base = h->d_base_i8f;
			sp.bp = h->d_cb_i8f;
			sp.n_rows = (uint32_t)h->n;
			sp.n_tiles_sel = t_sel;
			sp.tile_stride = nt / t_sel;
			sp.tile_run = run;
			sp.tiles_per_block = (t_sel + ic - 1) / ic;
			ic = (t_sel + sp.tiles_per_block - 1) / sp.tiles_per_block;
			const int ri = ensure_sample(m * (size_t)ic * 32 * sizeof(int));
			if (ri != EXPANN_OK)
				return ri;
			sp.n_qtiles = nqt;
			sp.queries = h->d_q8f;
			sp.m = (uint32_t)m;
			sp.sample_out = h->d_sample.as<int>();
			sp.n_chunks = ic;
			sp.ksteps = (uint32_t)h->dim / 64;
			hipLaunchKernelGGL(kGemmI8F.sample_w, dim3(ic * nqt), dim3((uint32_t)kGemmI8F.threads_w), kGemmI8F.lds_w, st, wsp);
			SampleTauI8cParams cp{};
			cp.t = tp;
			cp.t.n_vals = ic * 32;
			cp.t.j = j;
			cp.t.tau_s = h->d_tau_s;
			cp.vals = h->d_sample.as<const int>();
			cp.wb_max = h->d_wbmax_i8f;
			cp.two_s2 = 2.0 * (double)h->i8f.s * (double)h->i8f.s;
			hipLaunchKernelGGL(cp.t.n_vals <= 512 ? sample_tau_i8c_kernel<8>
			                                      : (cp.t.n_vals <= 1024 ? sample_tau_i8c_kernel<16> : sample_tau_i8c_kernel<32>),
			                   dim3((uint32_t)((m + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, cp);
			HIP_TRY(h, hipGetLastError());
			*spec_j = j;
			*done = true;
			*i8f_done = true;
			h->stat_i8_sample = 1;
			return EXPANN_OK;
		}
	}
	uint32_t chunks = std::max<uint32_t>(1, ((uint32_t)gvf->wg_per_cu * (uint32_t)cus) / nqt);
	chunks = std::max<uint32_t>(chunks, (uint32_t)((8 * k + live_res - 1) / std::max(1u, live_res)));
	chunks = std::min<uint32_t>(chunks, std::min<uint32_t>(64, t_sel / 4));
	if (t_sel * 2 > nt || (size_t)chunks * live_res < need_classes)
		return EXPANN_OK;
	const int ra = ensure_sample(m * (size_t)chunks * 32 * sizeof(float));
	if (ra != EXPANN_OK)
		return ra;
	GemmF16Params fp{};
	fp.base_f16 = h->d_base_f16;
	fp.bnorm = h->bns_f16();
	fp.n_rows = (uint32_t)h->n;
	fp.n_tiles_sel = t_sel;
	fp.tile_stride = nt / t_sel;
	fp.tile_run = run;
	fp.tiles_per_block = (t_sel + chunks - 1) / chunks;
	chunks = (t_sel + fp.tiles_per_block - 1) / fp.tiles_per_block;
	fp.n_qtiles = nqt;
	fp.queries_f16 = h->d_q_split;
	fp.m = (uint32_t)m;
	fp.sample_out = h->d_sample;
	fp.n_chunks = chunks;
	fp.ksteps = (uint32_t)f16_ld(h->dim) / 32;
	hipLaunchKernelGGL(gvf->sample, dim3(chunks * nqt), dim3((uint32_t)gvf->threads), gvf->lds, st, fp);
	tp.vals = h->d_sample;
	tp.n_vals = chunks * 32;
	if (spec_ok) {
		const uint32_t j = h->opt_spec_rank > 0 ? (uint32_t)std::min<size_t>((size_t)h->opt_spec_rank, k)
		                                        : spec_rank_auto(k, (double)t_sel / (double)nt);
		if (j < k) {
			*spec_j = j;
			tp.j = j;
			tp.tau_s = h->d_tau_s;
		}
	}
	hipLaunchKernelGGL(tp.n_vals <= 512 ? sample_tau_kernel<8>
	                                   : (tp.n_vals <= 1024 ? sample_tau_kernel<16> : sample_tau_kernel<32>),
	                   dim3((uint32_t)((m + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, tp);
	HIP_TRY(h, hipGetLastError());
	*done = true;
	*i8f_done = i8f;
	return EXPANN_OK;
}

// The full scan of the int8 filter (scan_gemm_i8f.hpp): scan_gemm_i8w_kernel<128> over the index's int8 copy with
// the thresholds of the fp16 sampled pass, hit logs filed by gather_logs_kernel in i_mode 3
int launch_scan_i8f(expann_index* h, size_t m, int cus, uint32_t cap, hipStream_t st) {
	const GemmI8qVariant* gs = &kGemmI8F;
	const uint32_t nt = (uint32_t)((h->n + kF16TB - 1) / kF16TB);
	const uint32_t nqt = (uint32_t)((m + kF16TQ - 1) / kF16TQ);
	GemmI8qParams fp{};
	fp.base = h->d_base_i8f;
	fp.bp = h->d_bp_i8f;
	fp.n_rows = (uint32_t)h->n;
	fp.n_tiles_sel = nt;
	fp.tile_stride = 1;
	fp.tile_run = 1;
	fp.n_qtiles = nqt;
	fp.queries = h->d_q8f;
	fp.thp = reinterpret_cast<const int*>(h->d_i8f_q + 3 * h->i8f_q_m);
	fp.m = (uint32_t)m;
	fp.cand_cnt = h->d_cnt;
	fp.cand = h->d_cand;
	fp.cap = cap;
	uint32_t fchunks = pick_row_chunks(nt, nqt, (uint32_t)gs->wg_per_cu_w * (uint32_t)cus, 4.0, 8, 2048,
	                                   h->opt_xcd_tolerance, (h->opt_debug & 1024) ? nullptr : &fp.xcd_map);
	fp.tiles_per_block = (nt + fchunks - 1) / fchunks;
	fchunks = (nt + fp.tiles_per_block - 1) / fp.tiles_per_block;
	GemmI8wParams wp{};
	wp.q = fp;
	const int rc = ensure_hit_logs(h, fchunks * nqt, 4, m, cap, fchunks, nqt, fp.xcd_map, st, &wp.log, &wp.log_cnt,
	                               &wp.log_cap);
	if (rc != EXPANN_OK)
		return rc;
	wp.lost = h->d_overflow;
	h->pending_scatter.i_thp = fp.thp;
	h->pending_scatter.i_bias = fp.bp;
	h->pending_scatter.i_qself = nullptr;
	h->pending_scatter.i_rw = h->d_rw_i8f;
	h->pending_scatter.i_mode = 3;
	hipLaunchKernelGGL(gs->scan_w, dim3(fchunks * nqt), dim3((uint32_t)gs->threads_w), gs->lds_w, st, wp);
	return EXPANN_OK;
}

// The fp16-form scan of one threshold level (theta' is in h->d_theta): the MFMA kernel of the
// index's dimension over `rows_sel` sampled rows (last: all rows), or -- a handful of queries on
// the last level: dv, the plan's variant -- the same filter streamed from HBM (scan_direct_f16.hpp).
int launch_scan_f16(expann_index* h, const GemmF16Variant* gvf, const DirectF16Variant* dv, uint32_t rows_sel, bool last, size_t m, int cus,
                    bool ip, uint32_t cap, hipStream_t st, const char** kname, uint32_t* n_qtiles,
                    uint32_t* query_tile) {
	*query_tile = (uint32_t)gvf->wgq;
	// 64-row tiles, 256 queries per workgroup, two workgroups resident per CU
	GemmF16Params fp{};
	fp.base_f16 = h->d_base_f16;
	fp.bnorm = h->bnorm_f16();
	fp.n_rows = (uint32_t)h->n;
	const uint32_t nt = (uint32_t)((h->n + gvf->tb - 1) / gvf->tb);
	fp.n_tiles_sel = last ? nt : std::min(nt, (rows_sel + gvf->tb - 1) / gvf->tb);
	fp.tile_stride = std::max<uint32_t>(1, nt / fp.n_tiles_sel);
	fp.tile_run = 1;
	if (!last && fp.tile_stride >= 16 && fp.n_tiles_sel >= 16) {
		// sampled level: runs of 16 consecutive tiles (one 256 KiB stretch each at d = 128)
		fp.tile_run = 16;
		fp.n_tiles_sel = (fp.n_tiles_sel / 16) * 16;
	}
	fp.n_qtiles = (uint32_t)((m + gvf->wgq - 1) / gvf->wgq);
	uint32_t fchunks = pick_row_chunks(fp.n_tiles_sel, fp.n_qtiles, (uint32_t)gvf->wg_per_cu * (uint32_t)cus,
	                                   4.0, 8, 2048, h->opt_xcd_tolerance,
	                                   (h->opt_debug & 1024) ? nullptr : &fp.xcd_map);
	if (h->opt_scan_chunks > 0) {  // (experiments: force the row-chunk count)
		fchunks = (uint32_t)std::min<long>(h->opt_scan_chunks, std::max<uint32_t>(1, fp.n_tiles_sel / 8));
		fp.xcd_map = (fchunks % 8 == 0 && !(h->opt_debug & 1024)) ? 1 : 0;
		const uint32_t tpb = (fp.n_tiles_sel + fchunks - 1) / fchunks;
		if ((fp.n_tiles_sel + tpb - 1) / tpb != fchunks)
			fp.xcd_map = 0;
	}
	fp.tiles_per_block = (fp.n_tiles_sel + fchunks - 1) / fchunks;
	fchunks = (fp.n_tiles_sel + fp.tiles_per_block - 1) / fp.tiles_per_block;
	if (gvf->hit_log && fp.xcd_map && h->opt_tail_chunks && !h->opt_scan_chunks) {  // (scan_gemm_f16x reads n_big)
		uint32_t big, nb, small, ns;
		// (small chunks of >= 64 steps: at 40 -- 500 k rows -- their prologues cost more than the drain saves)
		if (pick_tail_chunks(fp.n_tiles_sel, fchunks, fp.n_qtiles, (uint32_t)gvf->wg_per_cu * (uint32_t)cus, 64, &big, &nb,
		                     &small, &ns)) {
			fp.tiles_per_block = big;
			fp.n_big = nb;
			fp.tiles_small = small;
			fchunks = nb + ns;
		}
	}
	fp.queries_f16 = h->d_q_split;
	fp.ksteps = (uint32_t)f16_ld(h->dim) / 32;
	fp.theta = h->d_theta;
	fp.two_inv_s2 = (ip ? 1.0f : 2.0f) / (h->f16_scale * h->f16_scale);
	fp.m = (uint32_t)m;
	fp.cand_cnt = h->d_cnt;
	fp.cand = h->d_cand;
	fp.cap = cap;
	fp.debug = (uint32_t)h->opt_debug & ~16u;
	DevBuf clk;
	if (h->opt_debug & 16) {
		HIP_TRY(h, clk.alloc((18 + 3 * 65536) * 8));  // (+ per-workgroup records of scan_gemm_f16x)
		HIP_TRY(h, hipMemsetAsync(clk.p, 0, (18 + 3 * 65536) * 8, st));
		fp.clk = clk.as<unsigned long long>();
	}
	if (dv && last) {
		// a handful of queries: stream the fp16 rows without the matrix cores, ~16
		// workgroups per CU, whole RPS-row steps (inside the copy's 64-row padding)
		fp.n_qtiles = (uint32_t)((m + dv->tq - 1) / dv->tq);
		fp.n_tiles_sel = (uint32_t)((h->n + dv->rps - 1) / dv->rps);
		const uint32_t want = std::max<uint32_t>(1, (16u * (uint32_t)cus) / fp.n_qtiles);
		fp.tiles_per_block = std::max<uint32_t>(8, (fp.n_tiles_sel + want - 1) / want);
		fchunks = (fp.n_tiles_sel + fp.tiles_per_block - 1) / fp.tiles_per_block;
		fp.xcd_map = 0;
		hipLaunchKernelGGL(dv->fn, dim3(fchunks * fp.n_qtiles), dim3(kBlock), 0, st, fp);
		*kname = dv->name;
		*query_tile = (uint32_t)dv->tq;
	} else {
		const uint32_t grid = fchunks * fp.n_qtiles;
		if (gvf->hit_log) {
			const int lrc = ensure_hit_logs(h, grid, gvf->threads / 64, m, cap, fchunks, fp.n_qtiles, fp.xcd_map, st,
			                                &fp.log, &fp.log_cnt, &fp.log_cap);
			if (lrc != EXPANN_OK)
				return lrc;
			fp.lost = h->d_overflow;
			h->pending_scatter.theta = fp.theta;
			h->pending_scatter.key_mul = fp.two_inv_s2;
		}
		uint32_t launch_grid = grid;
		const uint32_t resident = (uint32_t)gvf->wg_per_cu * (uint32_t)cus;
		// (built into the d = 128 instance; items shorter than ~160 steps -- a thousand queries over 1 M rows --
		// lose more to the per-item pull and prologue than the even end gains: 2.91 M vs 3.00 M QPS)
		if (gvf->hit_log && gvf->d == 128 && h->opt_persist && grid > resident &&
		    (fp.tiles_per_block >= 160 || h->opt_persist > 1)) {
			// persistent launch: what is resident pulls the `grid` items from per-XCD counters
			if (!h->d_work_ctr)
				HIP_TRY(h, hipMalloc(&h->d_work_ctr, sizeof(uint32_t) * 8 * 16));
			HIP_TRY(h, hipMemsetAsync(h->d_work_ctr, 0, sizeof(uint32_t) * 8 * 16, st));
			fp.work_ctr = h->d_work_ctr;
			fp.n_items = grid;
			launch_grid = resident;
		}
		hipLaunchKernelGGL(gvf->scan, dim3(launch_grid), dim3((uint32_t)gvf->threads), gvf->lds, st, fp);
		*kname = gvf->name;
	}
	*n_qtiles = fp.n_qtiles;
	if (fp.clk) {
		int occ = -1;
		hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)gvf->scan, gvf->threads, gvf->lds);
		std::fprintf(stderr, "scan_gemm_f16: %d workgroups per CU resident, grid %u\n", occ,
		             fchunks * fp.n_qtiles);
		unsigned long long c[18] = {0};
		HIP_TRY(h, hipMemcpy(c, fp.clk, sizeof(c), hipMemcpyDeviceToHost));
		std::fprintf(stderr, "scan_gemm_f16 wg0: %llu shader clocks in %.1f us = %.0f MHz\n", c[0],
		             c[1] / 100.0, c[1] ? c[0] * 100.0 / c[1] : 0.0);
		if (c[6])
			std::fprintf(stderr, "  per step (%llu steps): columns 0-1 %.0f, stage wait + barrier %.0f, columns 2-3 %.0f, tail + queue work %.0f cycles\n",
			             c[6], (double)c[2] / c[6], (double)c[3] / c[6], (double)c[4] / c[6], (double)c[5] / c[6]);
		if (const char* dump = std::getenv("EXPANN_WG_TIMES")) {  // per-workgroup start / end / place, for profiles/wg_times.py
			const uint32_t grid = std::min<uint32_t>(fchunks * fp.n_qtiles, 65536);
			std::vector<unsigned long long> rec(3 * (size_t)grid);
			HIP_TRY(h, hipMemcpy(rec.data(), fp.clk + 18, rec.size() * 8, hipMemcpyDeviceToHost));
			if (FILE* f = std::fopen(dump, "w")) {
				for (uint32_t b = 0; b < grid; ++b)
					std::fprintf(f, "%u %llu %llu %llu\n", b, rec[3 * b], rec[3 * b + 1], rec[3 * b + 2]);
				std::fclose(f);
			}
		}
		if (c[14])  // (scan_gemm_f16x: the last workgroup of the grid as well)
			std::fprintf(stderr, "scan_gemm_f16 last wg: %llu shader clocks in %.1f us = %.0f MHz, started %.1f us after wg0; per step (%llu): %.0f / %.0f / %.0f / %.0f\n",
			             c[8], c[9] / 100.0, c[9] ? c[8] * 100.0 / c[9] : 0.0, (double)(c[15] - c[7]) / 100.0, c[14],
			             (double)c[10] / c[14], (double)c[11] / c[14], (double)c[12] / c[14], (double)c[13] / c[14]);
	}
	return EXPANN_OK;
}

// The query side of the fp16 forms (SearchPass::prepare_queries, RangePass): scaled fp16 queries, ||q||^2, and the
// largest |q| (range check, read back at the end): one memset of the flag block, one kernel
// (latency mode, one workgroup: the kernel clears the flag block itself and, when the queries
// still sit in pinned host memory -- from_host --, leaves the device copy the later kernels read)
int launch_f16_query_prep(expann_index* h, const GemmF16Variant* gvf, const void* d_queries, size_t m, bool ip, bool from_host,
                          const I8fQueryArgs& qa, hipStream_t st) {
	const size_t nv = m * (size_t)h->dim;
	HIP_TRY(h, grow_ws(h, h->d_q_split, nv * 4));
	const bool one_wg = m <= (size_t)kRowsPerGroup;
	if (!one_wg)
		HIP_TRY(h, hipMemsetAsync(h->d_overflow, 0, 32, st));
	const dim3 prep_grid((uint32_t)((m + kRowsPerGroup - 1) / kRowsPerGroup));
	const float* ip_ref = (ip && h->opt_ip_rescale) ? (const float*)(h->d_bnmax + 2) : (const float*)nullptr;
	if (gvf->d == 0)  // (run-time dim: rows of f16_ld(d) elements, zero-padded)
		hipLaunchKernelGGL(f16_query_prep_any_kernel, prep_grid, dim3(kBlock), 0, st, (const float*)d_queries,
		                   (uint32_t)m, (uint32_t)h->dim, (uint32_t)f16_ld(h->dim), h->f16_scale,
		                   h->d_q_split.as<_Float16>(), h->d_qnrm, h->d_overflow + 2,
		                   from_host ? h->d_q.as<float>() : (float*)nullptr, one_wg ? h->d_overflow : (uint32_t*)nullptr,
		                   ip_ref, h->d_qscale.as<float>());
	else
		hipLaunchKernelGGL(gvf->prep, prep_grid, dim3(kBlock), 0, st, (const float*)d_queries, (uint32_t)m,
		                   h->f16_scale, h->d_q_split.as<_Float16>(), h->d_qnrm, h->d_overflow + 2,
		                   from_host ? h->d_q.as<float>() : (float*)nullptr, one_wg ? h->d_overflow : (uint32_t*)nullptr,
		                   ip_ref, h->d_qscale.as<float>(), qa);
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

// ---- one pass over <= kMaxQueriesPerPass queries, as a planner + steps -------------------------
// choose_kernels()   which kernel family serves this pass (plan_scan, bf_plan.hpp: row type, metric, batch size,
//                    options, what an earlier attempt learned) and the index's derived copies it needs
// prepare_queries()  the query-side conversions of that family (scaled fp16 / bf16 split)
// plan_thresholds()  threshold levels of this attempt: the ladder, class minima, or one sampled pass
// run_level(li)      scan of level li (direct / bf16x3 / fp16 / int8 MFMA filter) + selection
// check(attempt)     the one host wait: flags read back, retry with larger lists / another family
// the redo pass's workspace for R query slots (expann_index::d_redo), offsets in bytes: the failing queries'
// numbers, the per-slot list counters, theta', ||q||^2, w_q, thp, the bounds S_k' of the failed lists, the thresholds
// tau_r the redo scan filters with (true units: the two-round re-rank's tau_f), the fp16 and int8 copies, the
// candidate lists
struct RedoWs {
	size_t list, cnt, theta, qnrm, wq, thp, bound, tau, q16, q8, cand, total;
	RedoWs(uint32_t R, int dim, uint32_t cap) {
		list = 0;
		cnt = 4 * (size_t)R;
		theta = 8 * (size_t)R;
		qnrm = 12 * (size_t)R;
		wq = 16 * (size_t)R;
		thp = 20 * (size_t)R;
		bound = 24 * (size_t)R;
		tau = 28 * (size_t)R;
		q16 = 32 * (size_t)R;  // (R is a multiple of 256: every part starts on a 16-byte boundary)
		q8 = q16 + 2 * (size_t)R * (size_t)dim;
		cand = q8 + (size_t)R * (size_t)dim;
		total = cand + 8 * (size_t)R * (size_t)cap;
	}
};
// the direct scan's row chunks: ~16 workgroups per CU in total, at least 8 groups (128 rows) per workgroup
uint32_t direct_scan_chunks(uint32_t n_groups_sel, uint32_t n_qtiles, int cus) {
	const uint32_t target = (uint32_t)std::max<long>(1, (16L * cus + n_qtiles - 1) / n_qtiles);
	return std::min(target, std::max<uint32_t>(1, n_groups_sel / 8));
}

struct ScanSel {
	ScanFn fn = nullptr;
	int tq = 0;
	const char* name = "";
	ScanFn fn_bits = nullptr, fn_list = nullptr;  // (f32 rows: the row filter's instances)
};
struct SearchPass {
	expann_index* h;
	const void* d_queries;
	size_t m, k;
	uint64_t* d_ids;
	float* d_dists;
	hipStream_t st;
	bool ip;
	int cus;
	uint32_t cap;
	ScanSel svs;
	const ScanSel* sv = &svs;
	// the planner's choice (bf_plan.hpp) and its family's variant: at most one of the three is set
	ScanPlan plan;
	PlanAttempt learned;        // what the attempts so far learned
	const GemmI8Variant* gvi = nullptr;
	const GemmBf16Variant* gvb = nullptr;
	const GemmF16Variant* gvf = nullptr;
	const DirectF16Variant* dv = nullptr;  // fp16 form: scan_direct_f16 serves the last level and the sampled pass
	bool i8f = false;           // the int8 filter runs the full scan (fp16 prelude, scan_gemm_i8f.hpp)
	bool i8f_ready = false;     // its thresholds of this attempt are written
	bool i8f_ran = false;       // the last level of this attempt ran it
	bool flags_clean = false;   // the fp16 prelude has just zeroed the flag block
	// thresholds of the current attempt
	std::vector<Level> levels;
	uint32_t n_qtiles = 0;
	size_t li_start = 0;
	bool theta_ready = false;   // the sampled pass also wrote theta' and zeroed the list counters
	// speculative thresholds
	uint32_t spec_j = 0;        // this attempt's lists are filtered with the j-th class maximum, j < k (0: proven thresholds)
	uint32_t redo_slots = 0;    // R: query slots of the redo pass
	bool rerank_counted = false;  // "rerank_stats": the last level's selects counted the rows they re-scored

	enum Next { kDone, kRestart, kRetry };
	ScanPlan replan() const { return plan_scan(plan_index(h), PlanCall{m, k, cap}, learned); }
	int choose_kernels();
	int prepare_queries(bool* restart);
	int plan_thresholds();
	int run_level(size_t li);
	int run_redo(bool use_i8f);
	int check(int attempt, Next* next);
	int run();
};

int SearchPass::choose_kernels() {
	plan = replan();
	gvi = plan.family == ScanFamily::kGemmI8 ? find_gemm_i8(h->dim, h->int_mode) : nullptr;
	if (gvi) {
		int rc = ensure_bias_i8(h, gvi, st);
		if (rc != EXPANN_OK)
			return rc;
	}
	if (plan.status != EXPANN_OK)
		return h->fail(plan.status, plan.message);
	gvf = find_f16(plan.family, h->dim);
	dv = find_direct_f16(h->dim, plan.direct_f16_tq);
	i8f = plan.i8f;
	gvb = nullptr;
	for (const auto& v : kGemmBf16)
		if (plan.family == ScanFamily::kBf16x3 && v.d == h->dim)
			gvb = &v;
	if (gvb)
		return ensure_bnorm_bf16(h, gvb, st);
	return EXPANN_OK;
}

int SearchPass::prepare_queries(bool* restart) {
	*restart = false;
	if (gvf) {
		int rc = ensure_f16(h, gvf, st);
		if (rc != EXPANN_OK)
			return rc;
		if (h->f16_scale < 0.0f) {  // the index does not fit the fp16 range at any allowed scale
			learned.no_f16 = true;
			*restart = true;
			return EXPANN_OK;
		}
		rc = ensure_filter_terms(h, st);
		if (rc != EXPANN_OK)
			return rc;
		rc = ensure_workspace(h, m, cap);
		if (rc != EXPANN_OK)
			return rc;
		I8fQueryArgs qa{};
		if (i8f) {
			rc = ensure_i8f(h, st);
			if (rc != EXPANN_OK)
				return rc;
			// the plan again, now that the handle knows whether its rows take the int8 filter (i8f_state 1 / 2, or -1:
			// then without it, with the speculation and the list capacity of the fp16 form alone)
			plan = replan();
			i8f = plan.i8f;
			// (room for the lists of queries with a clipped component; with speculative thresholds the main lists are
			// shorter -- 819 at most at C2 -- but the redo pass's are proven-threshold lists: 1 178 at most)
			cap = std::max(cap, plan.i8f_min_cap);
		}
		if (i8f) {  // int8 queries and the per-query terms [A_q | W_q | w_q | thp]
			HIP_TRY(h, grow_ws(h, h->d_q8f, m * (size_t)h->dim));
			if (m > h->i8f_q_m) {
				if (h->async_pending > 0)
					HIP_TRY(h, hipStreamSynchronize(h->async_stream));
				h->d_i8f_q.reset();
				h->i8f_q_m = 0;
				HIP_TRY(h, hipMalloc(&h->d_i8f_q, 4 * sizeof(float) * m));
				h->i8f_q_m = m;
			}
			qa.q8 = h->d_q8f.as<int8_t>();
			qa.aq = h->d_i8f_q;
			qa.wq = h->d_i8f_q + h->i8f_q_m;
			qa.k = h->i8f;
		}
		const bool from_host = h->q_in_pinned_host && m <= (size_t)kRowsPerGroup;
		rc = launch_f16_query_prep(h, gvf, d_queries, m, ip, from_host, qa, st);
		if (rc != EXPANN_OK)
			return rc;
		flags_clean = true;
		if (from_host) {
			d_queries = h->d_q;
			h->q_in_pinned_host = false;
		}
	}
	if (gvb) {  // queries -> bf16 hi/lo planes
		const size_t nv = m * (size_t)h->dim;
		HIP_TRY(h, grow_ws(h, h->d_q_split, nv * 4));
		hipLaunchKernelGGL(split_bf16_kernel, dim3((uint32_t)((nv + kBlock - 1) / kBlock)),
		                   dim3(kBlock), 0, st, (const float*)d_queries, m, h->dim,
		                   h->d_q_split.as<__bf16>());
		HIP_TRY(h, hipGetLastError());
	}
	return EXPANN_OK;
}

int SearchPass::plan_thresholds() {
	int rc = ensure_workspace(h, m, cap);
	if (rc != EXPANN_OK)
		return rc;
	const bool filt = h->filter_on;
	levels = filt ? plan_levels_filtered(h->n, h->n_allowed, h->filter_list_len, k, cap, h->opt_sample_ratio)
	              : plan_levels(h->n, k, cap, h->opt_sample_ratio);
	n_qtiles = (uint32_t)((m + sv->tq - 1) / sv->tq);
	if (plan.family == ScanFamily::kDirect && plan.sampled && levels.size() >= 3) {
		// direct path: ONE sampled level of class minima (1/16 of the rows) instead of the
		// first two levels of the ladder -- a launch chain shorter by a scan, a select and a
		// memset, and ~10 k instead of ~32 k candidates in the full scan
		const uint32_t n_groups = (uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup);
		const uint32_t sel = n_groups / 16;
		uint32_t blocks = std::min<uint32_t>({128u, cap / 16, sel / 8});
		if (blocks * 16 >= 8 * k && blocks >= 16) {
			Level l0;
			l0.n_groups_sel = sel;
			l0.group_stride = 16;
			l0.classmin_blocks = blocks;
			levels.clear();
			levels.push_back(l0);
			levels.push_back(Level{n_groups, 1, 0});
		}
	}
	if (!flags_clean) {  // overflow count and statistics (words 1, 2: uint8 / fp16 range flags, kept)
		HIP_TRY(h, hipMemsetAsync(h->d_overflow, 0, sizeof(uint32_t), st));
		HIP_TRY(h, hipMemsetAsync(h->d_total, 0, sizeof(unsigned long long) * 2, st));
	}
	flags_clean = false;
	// fp16 form on a large index: ONE sampled pass (1/16 of the rows, class maxima per query,
	// scan_gemm_f16.hpp) gives the threshold of the full scan -- no direct level-0 scan, no
	// intermediate candidate lists and selects
	li_start = 0;
	theta_ready = false;
	i8f_ready = false;
	spec_j = 0;
	h->stat_i8_sample = 0;
	if (gvf && plan.sampled && levels.size() >= 2) {
		spec_j = (plan.speculate && !learned.spec_off) ? 1 : 0;  // (spec_off: learned since the plan was made)
		const int rs = sampled_pass_f16(h, gvf, dv, m, k, ip, cus, h->d_tau[levels.size() & 1],
		                                h->d_tau_row[levels.size() & 1], st, &theta_ready, i8f, &i8f_ready, &spec_j);
		if (rs != EXPANN_OK)
			return rs;
		if (theta_ready)
			li_start = levels.size() - 1;
	}
	h->stat_spec_rank = spec_j ? spec_j : k;
	if (spec_j) {  // the redo pass's workspace (the main select appends to its list)
		redo_slots = spec_redo_slots(m);
		HIP_TRY(h, grow_ws(h, h->d_redo, RedoWs(redo_slots, h->dim, cap).total));
	}
	return EXPANN_OK;
}

int SearchPass::run_level(size_t li) {
	const Level& L = levels[li];
	const bool first = (li == 0), last = (li + 1 == levels.size());
	ScanParams sp{};
	sp.base = h->d_base;
	sp.n_rows = (uint32_t)h->n;
	sp.n_groups_sel = L.n_groups_sel;
	sp.group_stride = L.group_stride;
	sp.n_qtiles = n_qtiles;
	sp.queries = d_queries;
	sp.m = (uint32_t)m;
	sp.tau = first ? nullptr : h->d_tau[(li + 1) & 1];
	sp.tau_row = first ? nullptr : h->d_tau_row[(li + 1) & 1];
	sp.cand_cnt = h->d_cnt;
	sp.cand = h->d_cand;
	sp.cap = cap;
	sp.dim = (uint32_t)h->dim;
	ScanFn scan_fn = sv->fn;
	if (h->filter_on) {  // level 0 walks the filter's list, the later levels read its bitmap
		scan_fn = L.list_rows ? sv->fn_list : sv->fn_bits;
		if (!scan_fn || (first && !L.list_rows))
			return h->fail(EXPANN_ERR_UNSUPPORTED, "row filter: no filtered instance of the direct scan");  // (f32 rows have both)
		sp.allow_bits = h->d_filter_bits;
		sp.row_list = h->d_filter_list;
		sp.list_len = L.list_rows;
		sp.list_stride = L.list_step;
	}
	uint32_t n_chunks = direct_scan_chunks(L.n_groups_sel, n_qtiles, cus);
	if (first && L.classmin_blocks) {
		n_chunks = L.classmin_blocks;
		sp.classmin = 1;
	}
	sp.groups_per_block = (L.n_groups_sel + n_chunks - 1) / n_chunks;
	n_chunks = (L.n_groups_sel + sp.groups_per_block - 1) / sp.groups_per_block;
	if (!first && !theta_ready)
		HIP_TRY(h, hipMemsetAsync(h->d_cnt, 0, sizeof(uint32_t) * m, st));
	const bool use_gemm = plan.float_gemm() && !first;
	const bool use_i8f = use_gemm && gvf && last && i8f && i8f_ready;  // (else the fp16 form scans)
	if (last)
		i8f_ran = use_i8f;
	const bool timed = last && h->profiling && h->ev_used < kEventPairs;
	uint32_t passes = n_qtiles;
	const char* kname = sv->name;
	uint32_t qt_used = (uint32_t)sv->tq;
	if (use_gemm) {
		// theta_q = tau_q - ||q||^2 (1-eps), then the MFMA filter over 128-row tiles
		const float f16_abs = gvf ? std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim)
		                          : 0.0f;
		if (gvf && theta_ready)
			;
		else if (gvf)
			hipLaunchKernelGGL(f16_terms_kernel, dim3((uint32_t)((m + kBlock - 1) / kBlock)),
			                   dim3(kBlock), 0, st, h->d_qnrm.as<const float>(), (uint32_t)m,
			                   gemm_f16_filter_eps(h->dim), f16_abs, (const float*)sp.tau,
			                   0.5f * h->f16_scale * h->f16_scale, h->d_theta, ip ? 1 : 0,
			                   ip ? h->d_qscale.as<const float>() : (const float*)nullptr);
		else
			hipLaunchKernelGGL(gvb->theta, dim3((uint32_t)((m + kRowsPerGroup - 1) / kRowsPerGroup)),
			                   dim3(kBlock), 0, st, (const float*)d_queries, (uint32_t)m,
			                   (const float*)sp.tau, 1.0f - gemm_bf16_filter_eps(h->dim), h->d_theta);
		const uint32_t tq_wg = gvf ? (uint32_t)gvf->wgq : kGemmBf16TQ;
		uint32_t tq_small = 0, gemm_qtiles = (uint32_t)((m + tq_wg - 1) / tq_wg);
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		if (use_i8f) {
			const int rl = launch_scan_i8f(h, m, cus, cap, st);
			if (rl != EXPANN_OK)
				return rl;
			kname = kGemmI8F.name;
			gemm_qtiles = (uint32_t)((m + kF16TQ - 1) / kF16TQ);
		} else if (gvf) {
			const int rl = launch_scan_f16(h, gvf, dv, L.n_groups_sel * kRowsPerGroup, last, m, cus, ip, cap, st, &kname,
			                               &gemm_qtiles, &tq_small);
			if (rl != EXPANN_OK)
				return rl;
		} else {  // (plan.float_gemm() without the fp16 form: bf16x3)
			GemmBf16Params bp{};
			bp.base_split = h->d_base_split;
			bp.bnorm = h->d_bnorm_bf;
			bp.n_rows = (uint32_t)h->n;
			const uint32_t n_tiles = (uint32_t)((h->n + kGemmTB - 1) / kGemmTB);
			const uint32_t tiles_sel = last ? n_tiles : std::min(n_tiles, (L.n_groups_sel * kRowsPerGroup + kGemmTB - 1) / kGemmTB);
			bp.n_tiles_sel = tiles_sel;
			bp.tile_stride = std::max<uint32_t>(1, n_tiles / tiles_sel);
			bp.tile_run = 1;
			if (!last && bp.tile_stride >= 8 && tiles_sel >= 8) {
				// sampled level: runs of 8 consecutive tiles (one 2 MiB page each at d=128)
				// instead of isolated tiles, same number of tiles
				bp.tile_run = 8;
				bp.n_tiles_sel = (tiles_sel / 8) * 8;
			}
			// One workgroup per CU is resident (128 KiB of LDS), so the launch runs in rounds
			// of `cus` workgroups: pick the row-chunk count that minimises
			// rounds x (steps per workgroup + ~2 steps of prologue).
			uint32_t gchunks = pick_row_chunks(tiles_sel, gemm_qtiles, (uint32_t)cus, 2.0, 4, 1024, 0, nullptr);
			bp.tiles_per_block = (tiles_sel + gchunks - 1) / gchunks;
			gchunks = (tiles_sel + bp.tiles_per_block - 1) / bp.tiles_per_block;
			bp.n_qtiles = gemm_qtiles;
			bp.queries_split = h->d_q_split;
			bp.theta = h->d_theta;
			bp.m = (uint32_t)m;
			bp.cand_cnt = h->d_cnt;
			bp.cand = h->d_cand;
			bp.cap = cap;
			bp.debug = (uint32_t)h->opt_debug;
			hipLaunchKernelGGL(gvb->scan, dim3(gchunks * gemm_qtiles), dim3(kGemmThreads),
			                   2 * kGemmTB * h->dim * sizeof(float), st, bp);
			kname = gvb->name;
		}
		passes = gemm_qtiles;
		qt_used = tq_small ? tq_small : tq_wg;  // (launch_scan_f16 reports the tile it used)
	} else if (gvi && !first) {
		hipLaunchKernelGGL(gvi->theta, dim3((uint32_t)((m + kRowsPerGroup - 1) / kRowsPerGroup)),
		                   dim3(kBlock), 0, st, d_queries, (uint32_t)m, (const float*)sp.tau,
		                   h->d_theta.as<int>(), h->d_qself);
		const uint32_t tb = (uint32_t)gemm_i8_tb(h->dim);
		GemmI8Params gp{};
		gp.base = h->d_base;
		gp.bias = h->d_bias_i;
		gp.n_rows = (uint32_t)h->n;
		const uint32_t n_tiles = (uint32_t)((h->n + tb - 1) / tb);
		gp.n_tiles_sel = last ? n_tiles
		                      : std::min(n_tiles, (L.n_groups_sel * kRowsPerGroup + tb - 1) / tb);
		gp.tile_stride = std::max<uint32_t>(1, n_tiles / gp.n_tiles_sel);
		gp.n_qtiles = (uint32_t)((m + kGemmI8TQ - 1) / kGemmI8TQ);
		gp.queries = d_queries;
		gp.theta = h->d_theta.as<const int>();
		gp.qself = h->d_qself;
		gp.m = (uint32_t)m;
		gp.cand_cnt = h->d_cnt;
		gp.cand = h->d_cand;
		gp.cap = cap;
		uint32_t gchunks = pick_row_chunks(gp.n_tiles_sel, gp.n_qtiles, (uint32_t)cus, 2.0, 4, 4096, 0, nullptr);
		gp.tiles_per_block = (gp.n_tiles_sel + gchunks - 1) / gchunks;
		gchunks = (gp.n_tiles_sel + gp.tiles_per_block - 1) / gp.tiles_per_block;
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		hipLaunchKernelGGL(gvi->scan, dim3(gchunks * gp.n_qtiles), dim3(kGemmThreads),
		                   2 * tb * h->dim, st, gp);
		passes = gp.n_qtiles;
		kname = gvi->name;
		qt_used = kGemmI8TQ;
	} else {
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		hipLaunchKernelGGL(scan_fn, dim3(n_chunks * n_qtiles), dim3(kBlock), 0, st, sp);
	}
	if (timed) {
		HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][1], st));
		h->ev_used++;
	}
	launch_gather_logs(h, st);
	if (last && (timed || !h->profiling)) {
		h->prof.scan_launches++;
		h->prof.scan_rows += h->n;
		h->prof.scan_query_tiles += passes;
		h->prof.query_tile = qt_used;
		h->prof.levels = (uint32_t)(levels.size() - li_start + (li_start ? 1 : 0));
		std::snprintf(h->prof.scan_kernel, sizeof(h->prof.scan_kernel), "%s", kname);
	}
	HIP_TRY(h, hipGetLastError());

	SelectParams sel{};
	sel.cand = h->d_cand;
	sel.cand_cnt = first ? nullptr : h->d_cnt;
	sel.fixed_count = (first && L.classmin_blocks) ? n_chunks * 16 : L.n_groups_sel * kRowsPerGroup;
	sel.cap = cap;
	sel.k = (uint32_t)k;
	sel.id_offset = h->id_offset;
	sel.out_ids = last ? d_ids : nullptr;
	sel.out_dists = last ? d_dists : nullptr;
	sel.tau_out = last ? nullptr : h->d_tau[li & 1];
	sel.tau_prev = first ? nullptr : h->d_tau[(li + 1) & 1];
	sel.tau_row_out = last ? nullptr : h->d_tau_row[li & 1];
	sel.tau_row_prev = first ? nullptr : h->d_tau_row[(li + 1) & 1];
	sel.rerank_base = use_gemm ? (const float*)h->d_base : nullptr;  // (binary16 rows: the _Float16 select instances)
	sel.rerank_queries = use_gemm ? (const float*)d_queries : nullptr;
	sel.dim = (uint32_t)h->dim;
	sel.metric_ip = ip ? 1u : 0u;
	// (inner product, fp16 form only: the approximate key is off by at most E_q + E_b in
	// total, half the L2 margins)
	const float pr = ip ? 1.0f : 2.0f;
	sel.prune_eps = use_gemm ? (gvf ? pr * gemm_f16_filter_eps(h->dim) : gemm_bf16_filter_eps(h->dim)) : 0.0f;
	sel.prune_abs = (use_gemm && gvf)
	                    ? pr * std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim)
	                    : 0.0f;
	sel.bn_max = h->d_bnmax ? h->d_bnmax + (gvf ? 2 : (gvb ? 1 : 0)) : nullptr;
	sel.qnrm = (use_gemm && gvf) ? h->d_qnrm : nullptr;
	if (use_i8f) {  // the int8 filter's own margins (scan_gemm_i8f.hpp) instead of the fp16 slack
		sel.prune_eps = 0.0f;
		sel.prune_abs = 0.0f;
		sel.row_w = h->d_rw_i8f;
		sel.q_w = h->d_i8f_q + 2 * h->i8f_q_m;
		if (h->opt_rerank_rounds != 1) {  // two rounds: tau_f = the threshold thp came from (sample_tau_finish)
			sel.tau_f = spec_j ? (const float*)h->d_tau_s : (const float*)h->d_tau[levels.size() & 1];
			sel.inv_2s2 = h->i8f.inv_2s2;
		}
	}
	rerank_counted = false;
	if (last && sel.rerank_base && h->opt_rerank_stats) {
		HIP_TRY(h, grow_ws(h, h->d_rerank, 16 + sizeof(uint32_t) * m));
		HIP_TRY(h, hipMemsetAsync(h->d_rerank, 0, 16 + sizeof(uint32_t) * m, st));
		sel.rerank_cnt = reinterpret_cast<uint32_t*>(h->d_rerank.as<unsigned char>() + 16);
		rerank_counted = true;
	}
	sel.overflow = h->d_overflow;
	if (last && spec_j) {  // the check of the speculative thresholds; failing queries go to the redo pass's list
		const RedoWs ws(redo_slots, h->dim, cap);
		sel.spec_tau = h->d_tau_s;
		sel.redo_word = h->d_overflow + 3;
		sel.redo_list = reinterpret_cast<uint32_t*>(h->d_redo.as<unsigned char>() + ws.list);
		sel.redo_cap = redo_slots;
		sel.redo_bound = reinterpret_cast<float*>(h->d_redo.as<unsigned char>() + ws.bound);
	}
	const bool sum_counts = last && sel.cand_cnt && (h->profiling || use_i8f);  // statistics: candidates of the full scan (i8f_cand_limit)
	if (m > 64 && sel.rerank_base && sel.cand_cnt) {
		// short lists (the usual case after a GEMM-form scan): one wave per query
		// (int8 filter: longer lists, ~500 at k = 10 -- DESIGN.md 4.4i)
		// (speculative thresholds: the expectation is linear in the rank of the class maximum)
		const uint32_t sj = last ? spec_j : 0u;
		const double expect = (use_i8f ? kI8fListRatio : 1.0) * 1.2 * (sj ? (double)sj : (double)k) * sample_frac_for(h, k);
		const int rs = launch_select(h, sel, m, cap, st, select_longest_list(expect, sj), sum_counts);
		if (rs != EXPANN_OK)
			return rs;
	} else {
		if (sum_counts)
			hipLaunchKernelGGL(sum_u32_kernel, dim3(1), dim3(1024), 0, st, sel.cand_cnt, (uint32_t)m, h->d_total);
		if (m <= 64)
			sel.wave0_short = 1;  // latency mode: one launch, wave 0 orders the short lists
		hipLaunchKernelGGL(select_topk_fn(h, sel), dim3((uint32_t)m), dim3(kBlock), sizeof(uint64_t) * cap + 16, st, sel);
		HIP_TRY(h, hipGetLastError());
	}
	if (last && spec_j)
		return run_redo(use_i8f);
	return EXPANN_OK;
}

// The redo pass of the speculative thresholds, always enqueued behind the select of a speculating
// search: compact operands of the failing queries with thresholds from the proven tau, a scan over the R query
// slots -- the int8 filter: a streaming kernel that files its own hits (scan_redo_i8.hpp); the fp16 form: the main
// scan's kernel (workgroups of a query tile no failing query took leave at once) and the logs' gather --, one select
// launch that writes the failing queries' output rows.  No host wait: the counts are read on the device.
int SearchPass::run_redo(bool use_i8f) {
	const RedoWs ws(redo_slots, h->dim, cap);
	unsigned char* const b = h->d_redo.as<unsigned char>();
	uint32_t* const word = h->d_overflow + 3;
	const uint32_t R = redo_slots;
	RedoCompactParams cp{};
	cp.word = word;
	cp.list = reinterpret_cast<const uint32_t*>(b + ws.list);
	cp.n_slots = R;
	cp.row_bytes = (uint32_t)h->dim * 2;
	cp.q16 = h->d_q_split;
	cp.rq16 = b + ws.q16;
	cp.qnrm = h->d_qnrm;
	cp.r_qnrm = reinterpret_cast<float*>(b + ws.qnrm);
	cp.tau = h->d_tau[levels.size() & 1];
	cp.bound = h->opt_redo_bound ? reinterpret_cast<const float*>(b + ws.bound) : nullptr;
	cp.qscale = (ip && h->opt_ip_rescale) ? h->d_qscale.as<const float>() : nullptr;
	cp.eps = gemm_f16_filter_eps(h->dim);
	cp.abs_coef = std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim);
	cp.mul = 0.5f * h->f16_scale * h->f16_scale;
	cp.ip = ip ? 1 : 0;
	cp.r_theta = reinterpret_cast<float*>(b + ws.theta);
	cp.r_cnt = reinterpret_cast<uint32_t*>(b + ws.cnt);
	if (use_i8f) {
		cp.q8 = h->d_q8f;
		cp.rq8 = b + ws.q8;
		cp.i8_aq = h->d_i8f_q;
		cp.i8_wq_in = h->d_i8f_q + h->i8f_q_m;
		cp.r_thp = reinterpret_cast<int*>(b + ws.thp);
		cp.r_wq = reinterpret_cast<float*>(b + ws.wq);
		cp.r_tau = reinterpret_cast<float*>(b + ws.tau);
		cp.i8_inv_2s2 = h->i8f.inv_2s2;
	}
	hipLaunchKernelGGL(redo_compact_kernel, dim3(R / (kBlock / 64)), dim3(kBlock), 0, st, cp);

	uint32_t* const r_cnt = cp.r_cnt;
	uint64_t* const r_cand = reinterpret_cast<uint64_t*>(b + ws.cand);
	if (use_i8f) {
		// the int8 filter's scan (scan_redo_i8.hpp): a streaming read of the copy that files its own hits.  A static
		// grid; every wave owns one contiguous range of 16-row columns, cut here from the wave count
		RedoStreamParams rp{};
		rp.base = h->d_base_i8f;
		rp.bp = h->d_bp_i8f;
		rp.n_rows = (uint32_t)h->n;
		rp.n_cols = (uint32_t)((h->n + kF16TB - 1) / kF16TB) * (kF16TB / 16);  // (the copy is padded to whole 64-row tiles)
		const uint32_t n_waves = (uint32_t)cus * kRedoStreamWavesPerCu;
		rp.cols_per_wave = (rp.n_cols + n_waves - 1) / n_waves;
		rp.cols_per_wave = (rp.cols_per_wave + kRedoStreamU - 1) / kRedoStreamU * kRedoStreamU;  // (whole pipeline stages)
		rp.queries = cp.rq8;
		rp.thp = cp.r_thp;
		rp.n_slots = R;
		rp.live_q = word;
		rp.cand_cnt = r_cnt;
		rp.cand = r_cand;
		rp.cap = cap;
		hipLaunchKernelGGL(redo_stream_i8_kernel, dim3(n_waves / kRedoStreamWaves), dim3(kRedoStreamThreads), 0, st, rp);
	} else {
		// the fp16 form: the same scan kernel over R query slots, one round of the resident workgroups per query tile
		// (a batch inside the target fills one tile); its hit logs are the main scan's, which the main gather has
		// read by now
		const uint32_t nt = (uint32_t)((h->n + kF16TB - 1) / kF16TB);
		const uint32_t nqt = R / kF16TQ;
		uint32_t chunks = pick_row_chunks(nt, 1, (uint32_t)gvf->wg_per_cu * (uint32_t)cus, 4.0, 8, 2048, 0, nullptr);
		chunks = std::min<uint32_t>(chunks, (uint32_t)(h->log_cnt_n / (4 * (size_t)nqt)));
		if (chunks == 0 || !h->d_log)
			return h->fail(EXPANN_ERR_HIP, "redo pass: the main scan left no hit logs");  // (the main scan allocates them)
		const uint32_t tpb = (nt + chunks - 1) / chunks;
		chunks = (nt + tpb - 1) / tpb;
		const uint32_t n_logs = chunks * nqt * 4;
		const uint32_t log_cap = (uint32_t)std::min<size_t>(1u << 16, h->log_bytes / ((size_t)n_logs * 16));
		GatherLogParams gp{};
		gp.log = h->d_log.as<const uint4>();
		gp.log_cnt = h->d_log_cnt.as<const uint32_t>();
		gp.log_cap = log_cap;
		gp.n_chunks = chunks;
		gp.n_qtiles = nqt;
		gp.m = R;
		gp.cand_cnt = r_cnt;
		gp.cand = r_cand;
		gp.cap = cap;
		gp.live_q = word;
		GemmF16Params fp{};
		fp.base_f16 = h->d_base_f16;
		fp.bnorm = h->bnorm_f16();
		fp.n_rows = (uint32_t)h->n;
		fp.n_tiles_sel = nt;
		fp.tile_stride = 1;
		fp.tile_run = 1;
		fp.tiles_per_block = tpb;
		fp.n_qtiles = nqt;
		fp.queries_f16 = cp.rq16;
		fp.theta = cp.r_theta;
		fp.two_inv_s2 = (ip ? 1.0f : 2.0f) / (h->f16_scale * h->f16_scale);
		fp.m = R;
		fp.cand_cnt = gp.cand_cnt;
		fp.cand = gp.cand;
		fp.cap = cap;
		fp.ksteps = (uint32_t)f16_ld(h->dim) / 32;
		fp.log = h->d_log.as<uint4>();
		fp.log_cnt = h->d_log_cnt;
		fp.log_cap = log_cap;
		fp.lost = h->d_overflow;
		fp.live_q = word;
		hipLaunchKernelGGL(gvf->scan_redo, dim3(chunks * nqt), dim3((uint32_t)gvf->threads), gvf->lds, st, fp);
		gp.theta = cp.r_theta;
		gp.key_mul = fp.two_inv_s2;
		const uint32_t want = std::max<uint32_t>(1, (1024 + nqt * 4 - 1) / (nqt * 4));
		gp.chunks_per_block = std::max<uint32_t>(1, (chunks + want - 1) / want);
		gp.n_groups = (chunks + gp.chunks_per_block - 1) / gp.chunks_per_block;
		hipLaunchKernelGGL(gather_logs_kernel, dim3(nqt * 4 * gp.n_groups), dim3(kBlock), 0, st, gp);
	}

	// the select of the R slots in one launch: wave 0 of a slot's workgroup orders a list of <= 2048 keys, the
	// whole workgroup a longer one; no check (these lists come from thresholds that are proven bounds)
	SelectParams sel{};
	sel.cand = r_cand;
	sel.cand_cnt = r_cnt;
	sel.cap = cap;
	sel.k = (uint32_t)k;
	sel.id_offset = h->id_offset;
	sel.out_ids = d_ids;
	sel.out_dists = d_dists;
	sel.rerank_base = (const float*)h->d_base;
	sel.rerank_queries = (const float*)d_queries;
	sel.dim = (uint32_t)h->dim;
	sel.metric_ip = ip ? 1u : 0u;
	const float pr = ip ? 1.0f : 2.0f;
	sel.bn_max = h->d_bnmax + 2;
	sel.qnrm = cp.r_qnrm;
	if (use_i8f) {
		sel.row_w = h->d_rw_i8f;
		sel.q_w = cp.r_wq;
		if (h->opt_rerank_rounds != 1) {
			sel.tau_f = cp.r_tau;
			sel.inv_2s2 = h->i8f.inv_2s2;
		}
	} else {
		sel.prune_eps = pr * gemm_f16_filter_eps(h->dim);
		sel.prune_abs = pr * std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim);
	}
	sel.overflow = word;
	sel.wave0_short = 1;
	sel.slot_map = cp.list;
	sel.live_slots = word;
	sel.redo_cand = h->d_overflow + 6;
	if (rerank_counted)
		sel.rerank_cnt = reinterpret_cast<uint32_t*>(h->d_rerank.as<unsigned char>() + 16);
	hipLaunchKernelGGL(select_topk_fn(h, sel), dim3(R), dim3(kBlock), sizeof(uint64_t) * cap + 16, st, sel);
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

int SearchPass::check(int attempt, Next* next) {
	*next = kDone;
	uint64_t reranked = 0;
	if (rerank_counted) {  // statistics on request: one more launch and a host wait, also in the deferred form
		unsigned long long* const total = h->d_rerank.as<unsigned long long>();
		hipLaunchKernelGGL(sum_u32_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<const uint32_t*>(total + 2),
		                   (uint32_t)m, total);
		unsigned long long v = 0;
		HIP_TRY(h, hipMemcpyAsync(&v, total, sizeof(v), hipMemcpyDeviceToHost, st));
		HIP_TRY(h, hipStreamSynchronize(st));
		reranked = v;
	}
	// overflow check (the only host sync of a search); flags and statistics are contiguous
	if (defer_flags(h, st, attempt)) {
		h->stat_rerank_rows += reranked;  // deferred check: expann_sync reads the flags
		float sc = gvf ? h->f16_scale : 0.0f;  // (fp16 form: the range check of max |q| needs the scale)
		uint32_t* const slot = h->h_flag_ring + kRingWords * (h->async_pending - 1);
		std::memcpy(&slot[kRingScale], &sc, sizeof(float));
		if (i8f_ran && h->opt_i8_filter == 1)  // (the mark's high bit: the int8 filter's candidate limit follows)
			slot[kRingMark] = 0x80000000u | (uint32_t)std::min<uint64_t>(i8f_cand_limit(h, m, k, spec_j), 0x3FFFFFFFu);
		if (spec_j)  // (the mark's bit 30: word 3 is this search's redo word, word 6 its redo lists' keys)
			slot[kRingMark] |= 0x40000000u;
		return EXPANN_OK;
	}
	HIP_TRY(h, hipMemcpyAsync(h->h_flags, h->d_overflow, kFlagCopyBytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));
	unsigned long long tot;
	std::memcpy(&tot, h->h_flags + 4, sizeof(tot));
	h->prof.candidates = tot;
	if (i8f_ran && h->opt_i8_filter == 1 && tot > i8f_cand_limit(h, m, k, spec_j))
		h->i8f_state = 2;
	if (std::getenv("EXPANN_DEBUG_LISTS")) {  // (diagnostics: the distribution of the candidate lists' lengths)
		std::vector<uint32_t> cnt(m);
		HIP_TRY(h, hipMemcpy(cnt.data(), h->d_cnt, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
		std::sort(cnt.begin(), cnt.end());
		std::fprintf(stderr, "[lists] attempt %d cap %u: min %u median %u p90 %u p99 %u max %u, overflow flag %u\n", attempt, cap,
		             cnt.front(), cnt[m / 2], cnt[m * 9 / 10], cnt[m * 99 / 100], cnt.back(), h->h_flags[0]);
	}
	if (gvf) {  // queries outside the fp16 range of this index: redo with the bf16x3 form
		float qmax;  // bit pattern of max |q| (flags word 2, read back with the overflow flags)
		std::memcpy(&qmax, &h->h_flags[2], sizeof(float));
		if (!(qmax * h->f16_scale <= 60000.0f)) {
			learned.no_f16 = true;
			h->prof.retries++;
			*next = kRestart;
			return EXPANN_OK;
		}
	}
	if (h->strict_u8 && (h->h_flags[1] != 0 || h->h_flags[3] != 0))
		return kStrictReject;
	if (h->dtype == EXPANN_DTYPE_U8 && h->h_flags[1] != 0)
		return h->fail(EXPANN_ERR_UNSUPPORTED,
		               std::to_string(h->h_flags[1]) +
		                   " query values outside [0,255]: the uint8 metric "
		                   "(dist2_compressed) is only defined for 8-bit valued queries");
	// speculative thresholds: word 3 = failing queries (low 20 bits) + 2^20 per redo overflow (more of them than
	// redo slots, or a redo list beyond its capacity): the search is repeated with proven thresholds
	const uint32_t redo_word = spec_j ? h->h_flags[3] : 0u;
	if (h->h_flags[0] == 0 && redo_word < kRedoOverflowUnit) {
		h->stat_redo_queries += redo_word;
		h->stat_redo_candidates += spec_j ? h->h_flags[6] : 0u;
		h->stat_rerank_rows += reranked;
		return EXPANN_OK;
	}
	h->prof.retries++;
	if (spec_j) {  // (whatever overflowed: no speculation from here on)
		learned.spec_off = true;
		if (redo_word >= kRedoOverflowUnit)
			h->stat_redo_overflows++;
		if (h->h_flags[0] == 0) {
			*next = kRestart;
			return EXPANN_OK;
		}
	}
	// some candidate list overflowed: retry with 4x the capacity
	if (i8f_ran) {  // the int8 filter's lists: the retry runs the fp16 form at the same capacity
		learned.i8f_off = true;
		*next = kRestart;
		return EXPANN_OK;
	}
	// (a hit log of the 16x16x32 form that overflowed counts like a list: the logs grow with the lists)
	if ((cap >= kMaxCap || attempt >= 3) && plan.tie_fallback) {
		// the GEMM forms cannot break exact ties by row number; the direct scan can
		learned.force_direct = true;
		*next = kRestart;
		return EXPANN_OK;
	}
	if (cap >= kMaxCap || attempt >= 3)
		return h->fail(EXPANN_ERR_OVERFLOW,
		               "candidate lists overflowed (" + std::to_string(h->h_flags[0]) +
		                   " queries) at capacity " + std::to_string(cap) +
		                   "; the data has more near-ties than the threshold filter supports");
	cap = std::min(cap * 4, kMaxCap);
	*next = kRetry;
	return EXPANN_OK;
}

int SearchPass::run() {
	for (;;) {  // (a restart: another kernel family serves the same queries)
		int rc = choose_kernels();
		if (rc != EXPANN_OK)
			return rc;
		bool restart = false;
		rc = prepare_queries(&restart);
		if (rc != EXPANN_OK)
			return rc;
		if (restart)
			continue;
		Next next = kDone;
		for (int attempt = 0;; ++attempt) {  // (a retry: the same family with larger candidate lists)
			rc = ensure_workspace(h, m, cap);
			if (rc == EXPANN_OK)
				rc = plan_thresholds();
			for (size_t li = li_start; rc == EXPANN_OK && li < levels.size(); ++li)
				rc = run_level(li);
			if (rc == EXPANN_OK)
				rc = check(attempt, &next);
			if (rc != EXPANN_OK || next != kRetry)
				break;
		}
		if (rc != EXPANN_OK || next == kDone)
			return rc;
	}
}

// One pipeline pass over <= kMaxQueriesPerPass queries (device pointers).
int search_pass(expann_index* h, const void* d_queries, size_t m, size_t k, uint64_t* d_ids,
                float* d_dists, hipStream_t st) {
	const bool ip = (h->metric == EXPANN_METRIC_IP);
	if (h->filter_on && h->n_allowed == 0) {  // nothing is allowed: the outputs' padding is the whole answer
		hipLaunchKernelGGL(fill_pad_kernel, dim3((uint32_t)std::min<size_t>((m * k + kBlock - 1) / kBlock, 1024)), dim3(kBlock),
		                   0, st, d_ids, d_dists, m * k);
		HIP_TRY(h, hipGetLastError());
		if (!h->opt_async || h->host_call)
			HIP_TRY(h, hipStreamSynchronize(st));
		return EXPANN_OK;
	}
	uint32_t cap = plan_start_cap(h->opt_cand_capacity, k, kMaxCap);
	const ScanPlan plan = plan_scan(plan_index(h), PlanCall{m, k, cap}, PlanAttempt{});
	if (plan.u8_shadow) {
		// rows that are all integers in [0, 255] (SIFT): with integer queries the uint8 engine's
		// exact integer scores ARE the fp32 scores (d * 255^2 < 2^24: every partial sum of the
		// reference is an exactly represented integer), at the 8-bit kernels' speed
		if (h->u8_exact == 0) {
			const int rb = build_u8_shadow(h, st);
			if (rb != EXPANN_OK)
				return rb;
		}
		if (h->u8_exact == 1) {
			const int rq = search_pass(h->u8_shadow.get(), d_queries, m, k, d_ids, d_dists, st);
			const int ra = absorb_shadow_profile(h);
			if (rq == EXPANN_OK)
				return ra;
			if (rq != kStrictReject)
				return h->fail(rq, h->u8_shadow->err);
		}
	}
	ScanSel svs;
	if (float_rows(h)) {
		if (const ScanVariant* v = find_scan_f32(h->dim, ip, plan.direct_tq, f16_rows(h)))
			svs = ScanSel{v->fn, v->tq, v->name, v->fn_bits, v->fn_list};
	} else {
		if (const ScanI8Variant* v = find_scan_i8(h->dim, h->int_mode, plan.direct_tq))
			svs = ScanSel{v->fn, v->tq, v->name};
	}
	if (!svs.fn)
		return h->fail(EXPANN_ERR_UNSUPPORTED,
		               "no scan kernel for dim " + std::to_string(h->dim) +
		                   " / query_tile " + std::to_string(h->opt_query_tile));
	if (h->dtype == EXPANN_DTYPE_U8) {
		// fp32 queries -> uint8 (trunc); values outside [0,255] are counted and rejected below
		const size_t nv = m * (size_t)h->dim;
		HIP_TRY(h, grow_ws(h, h->d_q8, nv));
		int rcw = ensure_workspace(h, m, 2048);
		if (rcw != EXPANN_OK)
			return rcw;
		HIP_TRY(h, hipMemsetAsync(h->d_overflow + 1, 0, sizeof(uint32_t), st));
		HIP_TRY(h, hipMemsetAsync(h->d_overflow + 3, 0, sizeof(uint32_t), st));
		hipLaunchKernelGGL(u8_query_prep_kernel, dim3((uint32_t)((nv + kBlock - 1) / kBlock)),
		                   dim3(kBlock), 0, st, (const float*)d_queries, nv, h->d_q8,
		                   h->d_overflow + 1, h->strict_u8 ? h->d_overflow + 3 : (uint32_t*)nullptr);
		HIP_TRY(h, hipGetLastError());
		d_queries = h->d_q8;
	}
	if ((size_t)cap < 2 * k)
		return h->fail(EXPANN_ERR_UNSUPPORTED, k_too_large());
	const int cus = num_cus(h->device);
	if (const GemmI8qVariant* gq = plan.i8q ? find_gemm_i8q(plan.i8q_family, h->dim, h->int_mode) : nullptr) {
		const int rq = search_i8q(h, gq, d_queries, m, k, d_ids, d_dists, st, cap);
		if (rq != kRetryGeneric)
			return rq;
	}
	SearchPass pass{h, d_queries, m, k, d_ids, d_dists, st, ip, cus, cap, svs};
	return pass.run();
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------
extern "C" {

int expann_abi_version(void) { return EXPANN_ABI_VERSION; }

int expann_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int expann_create(int dim, int dtype, int metric, int device, expann_index** out) {
	if (!out) {
		g_create_error = "out == NULL";
		return EXPANN_ERR_INVALID_ARG;
	}
	*out = nullptr;
	if (dim <= 0 || dim % 16 != 0) {
		g_create_error = "dim must be a positive multiple of 16 (the reference kernels require it)";
		return EXPANN_ERR_INVALID_ARG;
	}
	int int_mode = -1;
	if (dtype == EXPANN_DTYPE_F32 || dtype == EXPANN_DTYPE_F16) {  // (binary16 rows: the f32 rules)
		if (metric != EXPANN_METRIC_L2 && metric != EXPANN_METRIC_IP) {
			g_create_error = "metric must be EXPANN_METRIC_L2 or EXPANN_METRIC_IP for f32 / f16 rows";
			return EXPANN_ERR_INVALID_ARG;
		}
		if (dim > kMaxAnyDim) {
			g_create_error = "unsupported dim " + std::to_string(dim) + ": f32 / f16 rows take dim <= " +
			                 std::to_string(kMaxAnyDim);
			return EXPANN_ERR_UNSUPPORTED;
		}
	} else if (dtype == EXPANN_DTYPE_U8) {
		if (metric != EXPANN_METRIC_L2) {
			g_create_error = "uint8 rows support EXPANN_METRIC_L2 only (dist2_compressed)";
			return EXPANN_ERR_INVALID_ARG;
		}
		int_mode = kU8L2;
	} else if (dtype == EXPANN_DTYPE_I16) {
		if (metric != EXPANN_METRIC_L2) {
			g_create_error = "int16 rows support EXPANN_METRIC_L2 only (src/distance.h:14-27 semantics)";
			return EXPANN_ERR_INVALID_ARG;
		}
		int_mode = kI16L2Ref;
	} else if (dtype == EXPANN_DTYPE_I8) {
		if (metric == EXPANN_METRIC_L2)
			int_mode = kI8L2;
		else if (metric == EXPANN_METRIC_IP)
			int_mode = kI8IP;
		else if (metric == EXPANN_METRIC_L2_I8_REFCOMPAT)
			int_mode = kI8L2Ref;
		else {
			g_create_error = "unknown metric for int8 rows";
			return EXPANN_ERR_INVALID_ARG;
		}
	} else {
		g_create_error = "unknown dtype";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (int_mode >= 0 && dim % 64 != 0) {
		g_create_error = "8-bit rows need dim % 64 == 0 (src/distance.h:29-53, antitopo_engine.h:726)";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (int_mode >= 0 && int_mode != kI16L2Ref && dim > kMaxAnyDim) {
		g_create_error = "unsupported dim " + std::to_string(dim) + ": 8-bit rows take dim <= " +
		                 std::to_string(kMaxAnyDim);
		return EXPANN_ERR_UNSUPPORTED;
	}
	int ndev = expann_device_count();
	if (ndev <= 0) {
		g_create_error = "no HIP device visible: libexpann_hip has no CPU fallback";
		return EXPANN_ERR_NO_DEVICE;
	}
	if (device < 0 || device >= ndev) {
		g_create_error = "device index out of range";
		return EXPANN_ERR_INVALID_ARG;
	}
	PlanIndex px;
	px.dtype = dtype;
	px.int_mode = int_mode;
	px.dim = dim;
	static const bool tables_match = plan_tables_match();
	if (!tables_match) {
		g_create_error = "internal: bf_plan.hpp does not list the compiled scan kernels";
		return EXPANN_ERR_UNSUPPORTED;
	}
	if (!direct_tile(px, 1)) {
		g_create_error = "unsupported dim " + std::to_string(dim) +
		                 " (built: f32 any multiple of 16 up to 4096; 8-bit any multiple of 64 up to 4096; int16 64,128)";
		return EXPANN_ERR_UNSUPPORTED;
	}
	// (owned until the last step: every early return destroys the handle, its stream included)
	std::unique_ptr<expann_index, HandleDeleter> h(new expann_index());
	h->dim = dim;
	h->dtype = dtype;
	h->metric = metric;
	h->device = device;
	h->elem = (dtype == EXPANN_DTYPE_F32) ? 4 : ((dtype == EXPANN_DTYPE_I16 || dtype == EXPANN_DTYPE_F16) ? 2 : 1);
	h->q_elem = (dtype == EXPANN_DTYPE_I8) ? 1 : (dtype == EXPANN_DTYPE_I16 ? 2 : 4);
	h->int_mode = int_mode;
	static_cast<Options&>(*h) = options_from_env();
	if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess) {
		g_create_error = "hipSetDevice/hipStreamCreate failed";
		return EXPANN_ERR_HIP;
	}
	// every kernel this (dim, dtype, int_mode) can reach that needs more dynamic LDS than the default limit
	struct LdsNeed {
		const void* fn;
		int bytes;
		const char* label;
	};
	std::vector<LdsNeed> needs;
	// the select kernel sorts up to kMaxCap 8-byte keys in LDS (128 KiB of the CU's 160 KiB)
	const int sel_lds = (int)(sizeof(uint64_t) * kMaxCap + 16);
	needs.push_back({(const void*)select_topk_kernel<float>, sel_lds, "select_topk_kernel"});
	needs.push_back({(const void*)select_topk_kernel<_Float16>, sel_lds, "select_topk_kernel"});
	needs.push_back({(const void*)select_topk_kernel<float, true>, sel_lds, "select_topk_kernel"});
	for (const auto& v : kGemmF16X)
		if (v.d == dim) {  // (the sampled pass is launched with the scan's LDS size, never less than its own)
			needs.push_back({(const void*)v.scan, v.lds, "scan_gemm_f16x_kernel"});
			needs.push_back({(const void*)v.sample, v.lds, "scan_gemm_f16x_kernel"});
			if (v.scan_redo)
				needs.push_back({(const void*)v.scan_redo, v.lds, "scan_gemm_f16x_kernel"});
		}
	if ((dtype == EXPANN_DTYPE_F32 || dtype == EXPANN_DTYPE_F16) && f16kl_dim(dim)) {
		needs.push_back({(const void*)kGemmF16KL.scan, kGemmF16KL.lds, "scan_gemm_kl_kernel, fp16"});
		needs.push_back({(const void*)kGemmF16KL.sample, kGemmF16KL.lds, "scan_gemm_kl_kernel, fp16"});
	}
	if (kGemmF16XDbg[0].d == dim)
		needs.push_back({(const void*)kGemmF16XDbg[0].scan, kGemmF16XDbg[0].lds, "scan_gemm_f16x_kernel"});
	for (const auto& v : kGemmI8x)
		if (v.d == dim) {
			needs.push_back({(const void*)v.scan, v.lds, "scan_gemm_w8_kernel, int8"});
			needs.push_back({(const void*)v.sample, v.lds, "scan_gemm_w8_kernel, int8"});
		}
	for (const auto& v : kGemmI8w)
		if (v.d == dim) {
			needs.push_back({(const void*)v.scan_w, v.lds_w, "scan_gemm_i8w_kernel"});
			needs.push_back({(const void*)v.sample_w, v.lds_w, "scan_gemm_i8w_kernel"});
		}
	if (any_dim_i8(dim, int_mode))
		for (const auto& v : kGemmI8KL)
			if (v.mode == int_mode) {
				needs.push_back({(const void*)v.scan_w, v.lds_w, "scan_gemm_kl_kernel, int8"});
				needs.push_back({(const void*)v.sample_w, v.lds_w, "scan_gemm_kl_kernel, int8"});
			}
	for (const auto& v : kGemmBf16)
		if (v.d == dim)
			needs.push_back({(const void*)v.scan, 2 * kGemmTB * dim * (int)sizeof(float), "scan_gemm_bf16x3_kernel"});
	for (const auto& v : kGemmI8)
		if (v.d == dim && v.mode == int_mode)
			needs.push_back({(const void*)v.scan, 2 * gemm_i8_tb(dim) * dim, "scan_gemm_i8_kernel"});
	for (const LdsNeed& need : needs)
		if (hipFuncSetAttribute(need.fn, hipFuncAttributeMaxDynamicSharedMemorySize, need.bytes) != hipSuccess) {
			g_create_error = std::string("hipFuncSetAttribute(") + need.label + ") failed";
			return EXPANN_ERR_HIP;
		}
	*out = h.release();
	return EXPANN_OK;
}

void expann_destroy(expann_index* h) {
	if (!h)
		return;
	hipSetDevice(h->device);
	if (h->stream) hipStreamSynchronize(h->stream);
	if (h->side_stream) hipStreamSynchronize(h->side_stream);
	// (every buffer, stream and event, and the shadow handle, is a member that frees itself, device still current)
	delete h;
}

const char* expann_last_error(const expann_index* h) {
	return h ? h->err.c_str() : g_create_error.c_str();
}

int expann_add(expann_index* h, const void* rows, size_t n) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!rows && n)
		return h->fail(EXPANN_ERR_INVALID_ARG, "rows == NULL");
	if (h->d_base)
		return h->fail(EXPANN_ERR_INVALID_ARG, "index already built");
	const size_t bytes = n * (size_t)h->dim * h->elem;
	const unsigned char* src = static_cast<const unsigned char*>(rows);
	h->staging.insert(h->staging.end(), src, src + bytes);
	h->n_staged += n;
	return EXPANN_OK;
}

int expann_build(expann_index* h) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (h->d_base)
		return h->fail(EXPANN_ERR_INVALID_ARG, "index already built");
	if (h->n_staged == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "build() on an empty index");
	if (h->n_staged >= (1ull << 32) - 32)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_row_filter(h);
	drop_row_groups(h);
	void* rows = nullptr;
	const size_t capacity = std::max(h->n_staged, h->reserved);  // (expann_reserve before build(): room for the appends to come)
	HIP_TRY(h, hipMalloc(&rows, capacity * (size_t)h->dim * h->elem));
	h->d_base.own(rows);
	h->capacity = capacity;
	HIP_TRY(h, hipMemcpy(h->d_base, h->staging.data(), h->staging.size(), hipMemcpyHostToDevice));
	h->n = h->n_staged;
	std::vector<unsigned char>().swap(h->staging);
	// the fp16 copy every fp32 search of a built dim filters through: made here, inside the
	// reference's timed build span (basic_bench.h:63-71), not inside the first query
	if (f16_copy_at_build(plan_index(h)))
		return ensure_f16(h, find_f16(f16_geometry(h->dim), h->dim), h->stream);
	return EXPANN_OK;
}

int expann_set_base_device(expann_index* h, const void* d_rows, size_t n, uint64_t id_offset) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!d_rows || n == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "empty device base");
	if (n >= (1ull << 32) - 32)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
	// the derived copies, a filter and the groups belong to the rows they were made from; the workspace, the
	// options, the profiling state and the statistics stay
	h->forget<RowCopies>();
	drop_row_filter(h);
	drop_row_groups(h);
	h->d_base.borrow(d_rows);
	h->n = n;
	h->capacity = 0;
	h->id_offset = id_offset;
	return EXPANN_OK;
}

size_t expann_size(const expann_index* h) { return h ? (h->d_base ? h->n : h->n_staged) : 0; }

// ---- append -----------------------------------------------------------------
extern "C++" {
namespace {
// what bf_append.hpp's plans read of a handle
AppendState append_state(const expann_index* h, bool have_rows) {
	AppendState s;
	s.have_rows = have_rows;
	s.on_device = (bool)h->d_base;
	s.owned = (bool)h->d_base.mine;
	s.float_rows = float_rows(h);
	s.n = h->n;
	s.capacity = h->capacity;
	s.f16_scale = h->d_base_f16 || h->f16_scale < 0.0f ? h->f16_scale : 0.0f;
	s.maxabs = h->f16_maxabs;
	return s;
}

// every stream that may still read the rows or their copies has drained (the row filter's rule)
int append_wait(expann_index* h) {
	if (h->async_pending > 0)
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return EXPANN_OK;
}

// A base of `capacity` rows that holds the handle's rows, and -- where an fp16 copy exists and is shorter than
// `f16_rows` rows -- a copy of that many rows initialised as ensure_f16 initialises one and holding the current
// [0, f16_n_pad): built ASIDE in the order of `st`, while the old allocations stay live, and swapped in by commit()
// once everything has succeeded.  A call that fails on the way frees what it built and leaves the handle as it was.
struct GrownRows {
	DevPtr<void> base;
	DevPtr<void> f16;
	DevPtr<float> bnorm, bns;
	size_t capacity = 0, f16_rows = 0;

	int build(expann_index* h, size_t new_capacity, hipStream_t st) {
		const size_t row_bytes = (size_t)h->dim * h->elem;
		if (new_capacity > h->capacity) {
			HIP_TRY(h, hipMalloc(&base, new_capacity * row_bytes));
			HIP_TRY(h, hipMemcpyAsync(base, h->d_base, h->n * row_bytes, hipMemcpyDeviceToDevice, st));
			capacity = new_capacity;
		}
		const bool have_copy = h->d_base_f16 && h->f16_scale > 0.0f && h->f16_tb > 0;  // (a complete copy)
		const size_t want = have_copy ? (new_capacity + h->f16_tb - 1) / h->f16_tb * h->f16_tb : 0;
		if (want > h->f16_rows_alloc) {
			const size_t ld2 = (size_t)f16_ld(h->dim) * 2;
			HIP_TRY(h, hipMalloc(&f16, want * ld2));
			HIP_TRY(h, hipMalloc(&bnorm, sizeof(float) * want));
			HIP_TRY(h, hipMalloc(&bns, sizeof(float) * want));
			const size_t keep = h->f16_n_pad;
			HIP_TRY(h, hipMemcpyAsync(f16, h->d_base_f16, keep * ld2, hipMemcpyDeviceToDevice, st));
			HIP_TRY(h, hipMemcpyAsync(bnorm, h->d_bnorm_f16, sizeof(float) * keep, hipMemcpyDeviceToDevice, st));
			HIP_TRY(h, hipMemcpyAsync(bns, h->d_bns_f16, sizeof(float) * keep, hipMemcpyDeviceToDevice, st));
			HIP_TRY(h, hipMemsetAsync(f16.as<char>() + keep * ld2, 0, (want - keep) * ld2, st));
			HIP_TRY(h, hipMemsetAsync(bnorm + keep, 0xFF, sizeof(float) * (want - keep), st));  // 0xFFFFFFFF: a NaN
			HIP_TRY(h, hipMemsetAsync(bns + keep, 0xFF, sizeof(float) * (want - keep), st));
			f16_rows = want;
		}
		return EXPANN_OK;
	}
	// (after `st` has drained; keep_f16 = false: the copy is about to be dropped anyway)
	// THE one place where a handle's base moves: whatever aliases the base is re-pointed here, next to the swap.
	void commit(expann_index* h, bool keep_f16) {
		if (base) {
			h->d_base.own(std::exchange(base.p, nullptr));
			h->capacity = capacity;
			h->stat_append[4]++;
			// an 8-bit index whose rows need neither padding nor mapping filters through the base itself
			// (ensure_i8q): the alias follows the base; every other derived copy is memory of its own
			if (h->d_base_i8q && !h->d_base_i8q.mine)
				h->d_base_i8q.borrow(h->d_base);
		}
		if (f16 && keep_f16) {
			h->d_base_f16 = std::move(f16);
			h->d_bnorm_f16 = std::move(bnorm);
			h->d_bns_f16 = std::move(bns);
			h->f16_rows_alloc = f16_rows;
		}
	}
};

// "copies_digest": the fp16 copy as 64 bits (append_rows.hpp), 0 when there is none; computed on demand, with a host
// wait, never on a search path
uint64_t copies_digest(expann_index* h) {
	if (!h->d_base_f16 || !(h->f16_scale > 0.0f))
		return 0;
	const auto run = [h](unsigned long long* out) {
		HIP_TRY(h, hipSetDevice(h->device));
		if (!h->d_append_flag)
			HIP_TRY(h, hipMalloc(&h->d_append_flag, 4 * sizeof(uint32_t)));
		unsigned long long* d_out = (unsigned long long*)(h->d_append_flag + 2);
		HIP_TRY(h, hipMemsetAsync(d_out, 0, sizeof(*d_out), h->stream));
		CopiesDigestParams dp;
		dp.rows = h->d_base_f16.as<const uint32_t>();
		dp.n_row_words = (uint64_t)h->f16_n_pad * (uint64_t)f16_ld(h->dim) / 2;
		dp.bnorm = h->d_bnorm_f16.as<const uint32_t>();
		dp.bns = h->d_bns_f16.as<const uint32_t>();
		dp.n_pad = h->f16_n_pad;
		dp.bnmax = h->d_bnmax.as<const uint32_t>() + 2;
		dp.scale_bits = __builtin_bit_cast(uint32_t, h->f16_scale);
		dp.out = d_out;
		const uint64_t total = dp.n_row_words + 2 * dp.n_pad;
		hipLaunchKernelGGL(copies_digest_kernel, dim3((uint32_t)std::min<uint64_t>((total + kBlock - 1) / kBlock, 4096)),
		                   dim3(kBlock), 0, h->stream, dp);
		HIP_TRY(h, hipGetLastError());
		HIP_TRY(h, hipMemcpyAsync(out, d_out, sizeof(*out), hipMemcpyDeviceToHost, h->stream));
		HIP_TRY(h, hipStreamSynchronize(h->stream));
		return (int)EXPANN_OK;
	};
	unsigned long long v = 0;
	return run(&v) == EXPANN_OK ? (uint64_t)v : 0;
}

// rows: n_new of them in host (on_device = false) or device memory, read in the order of `user_st`
int append_rows(expann_index* h, const void* rows, size_t n_new, bool on_device, hipStream_t user_st) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	const AppendState state = append_state(h, rows != nullptr);
	AppendPlan plan = plan_append(state, n_new, 0.0f);  // (the status and the capacity: no device call before them)
	if (plan.status != EXPANN_OK)
		return h->fail(plan.status, plan.message);
	h->stat_append[0]++;
	if (n_new == 0)
		return EXPANN_OK;
	HIP_TRY(h, hipSetDevice(h->device));
	if (const int rc = append_wait(h))
		return rc;
	hipStream_t st = user_st ? user_st : h->stream;
	const size_t row_bytes = (size_t)h->dim * h->elem;
	const bool have_copy = state.float_rows && state.f16_scale > 0.0f;
	GrownRows grown;
	if (const int rc = grown.build(h, plan.capacity, st))
		return rc;
	// the new rows: to the tail of the base
	char* const tail = (grown.base ? grown.base.as<char>() : (char*)h->d_base) + h->n * row_bytes;
	HIP_TRY(h, hipMemcpyAsync(tail, rows, n_new * row_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
	// ... and, converted with the current scale, to the tail of the fp16 copy: one launch, which also reports max |v|
	float maxabs_new = 0.0f;
	if (have_copy) {
		if (!h->d_append_flag)
			HIP_TRY(h, hipMalloc(&h->d_append_flag, 4 * sizeof(uint32_t)));
		HIP_TRY(h, hipMemsetAsync(h->d_append_flag, 0, sizeof(uint32_t), st));
		const size_t ld = (size_t)f16_ld(h->dim);
		AppendRowsParams ap;
		ap.rows = tail;
		ap.n_new = (uint32_t)n_new;
		ap.d = (uint32_t)h->dim;
		ap.ld = (uint32_t)ld;
		ap.scale = h->f16_scale;
		ap.out = (grown.f16 ? grown.f16.as<_Float16>() : h->d_base_f16.as<_Float16>()) + h->n * ld;
		ap.bnorm = (grown.f16 ? grown.bnorm.p : h->d_bnorm_f16.p) + h->n;
		ap.bns = (grown.f16 ? grown.bns.p : h->d_bns_f16.p) + h->n;
		ap.eps = gemm_f16_filter_eps(h->dim);
		ap.abs_coef = std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim);
		ap.mul = 0.5f * h->f16_scale * h->f16_scale;
		ap.ip = h->metric == EXPANN_METRIC_IP ? 1 : 0;
		ap.bnmax_bits = h->d_bnmax.as<uint32_t>() + 2;
		ap.maxabs_bits = h->d_append_flag;
		const dim3 grid((uint32_t)((n_new + kRowsPerGroup - 1) / kRowsPerGroup));
		if (f16_rows(h))
			hipLaunchKernelGGL(append_f16_rows_kernel<_Float16>, grid, dim3(kBlock), 0, st, ap);
		else
			hipLaunchKernelGGL(append_f16_rows_kernel<float>, grid, dim3(kBlock), 0, st, ap);
	}
	// the one host wait of an append.  A failure behind the launch may have left terms of rows the handle does not
	// count in the live arrays: the derived copies are forgotten, the rows themselves are as they were.
	hipError_t e = have_copy ? hipGetLastError() : hipSuccess;
	if (e == hipSuccess && have_copy)
		e = hipMemcpyAsync(&maxabs_new, h->d_append_flag, sizeof(float), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		if (have_copy)
			h->forget<RowCopies>();
		return h->fail(EXPANN_ERR_HIP, std::string("append: ") + hipGetErrorString(e));
	}
	plan = plan_append(state, n_new, maxabs_new);
	// the rows are in: everything that described the shorter index goes
	grown.commit(h, plan.copies == CopyAction::kExtend);
	h->n = plan.n;
	h->stat_append[1] += n_new;
	h->forget<OtherCopies>();
	drop_row_filter(h);
	drop_row_groups(h);
	if (plan.copies == CopyAction::kExtend) {
		h->f16_n_pad = (plan.n + h->f16_tb - 1) / h->f16_tb * h->f16_tb;
		h->f16_maxabs = maxabs_of(state.maxabs, maxabs_new);
		h->stat_append[2]++;
	} else if (plan.copies == CopyAction::kDrop) {
		// the scale changed: the speculative rows die with the copy, which is made again now where a build makes it.
		// The rows are in, so the append has succeeded whatever becomes of the copy: if it cannot be made now,
		// what is left of the attempt goes and the next search makes it, and reports what fails then.
		h->forget<F16Copy>();  // (d_bnmax[1] goes with it: OtherCopies, which owns that slot, is forgotten already)
		h->stat_append[3]++;
		if (f16_copy_at_build(plan_index(h)))
			(void)ensure_f16(h, find_f16(f16_geometry(h->dim), h->dim), h->stream);  // (forgets what it began when it fails)
	}
	return EXPANN_OK;
}
}  // namespace
}  // extern "C++"

int expann_append(expann_index* h, const void* rows, size_t n) { return append_rows(h, rows, n, false, nullptr); }

int expann_append_device(expann_index* h, const void* d_rows, size_t n, void* stream) {
	return append_rows(h, d_rows, n, true, (hipStream_t)stream);
}

int expann_reserve(expann_index* h, size_t n_rows) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	const AppendPlan plan = plan_reserve(append_state(h, true), n_rows);
	if (plan.status != EXPANN_OK)
		return h->fail(plan.status, plan.message);
	if (!h->d_base) {  // remembered for expann_build
		h->reserved = std::max(h->reserved, n_rows);
		return EXPANN_OK;
	}
	if (!plan.realloc)
		return EXPANN_OK;
	HIP_TRY(h, hipSetDevice(h->device));
	if (const int rc = append_wait(h))
		return rc;
	GrownRows grown;
	if (const int rc = grown.build(h, plan.capacity, h->stream))
		return rc;
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	grown.commit(h, true);
	return EXPANN_OK;
}

// ---- remove -----------------------------------------------------------------
extern "C++" {
namespace {
// A base of the SAME capacity that holds the survivors of a remove in their old order, and -- where a usable fp16
// copy exists -- fp16 arrays of the same f16_rows_alloc, initialised as make_f16 initialises them (zero rows, NaN
// terms) and holding the survivors' rows and terms, with the two maxima recomputed: built ASIDE in the order of
// `st`, while the old allocations stay live, and swapped in by commit() once the one host wait has shown that
// everything succeeded.  GrownRows' shape; a call that fails on the way frees what it built and leaves the handle as
// it was.  Nothing aliases the base after commit(): the int8 operand that may (d_base_i8q) is forgotten with
// OtherCopies before the swap.
struct CompactedRows {
	KeepBitmap keep;  // (stat word 3: the max |v| bits of the survivors)
	DevPtr<void> base, f16;
	DevPtr<float> bnorm, bns, bnmax;
	DevBuf ids;
	uint32_t seen[4] = {0, 0, 0, 0};  // keep.stat()[0..3] on the host
	bool have_copy = false;

	// ids == nullptr: the keep bitmap is the row filter in force
	int build(expann_index* h, const uint64_t* id_list, size_t n_ids, bool on_device, hipStream_t st) {
		const size_t n = h->n, row_bytes = (size_t)h->dim * h->elem;
		HIP_TRY(h, keep.alloc(n, st));
		if (!id_list) {
			if (h->filter_words != keep_words(n))
				return h->fail(EXPANN_ERR_HIP, "compact_row_filter: the bitmap does not cover the rows");  // (both are whole 128-row tiles)
			HIP_TRY(h, hipMemcpyAsync(keep.bits(), h->d_filter_bits, sizeof(uint32_t) * keep.words, hipMemcpyDeviceToDevice, st));
		} else {
			HIP_TRY(h, keep.all_ones(st));
			if (!on_device) {
				HIP_TRY(h, ids.alloc(sizeof(uint64_t) * n_ids));
				HIP_TRY(h, hipMemcpyAsync(ids.p, id_list, sizeof(uint64_t) * n_ids, hipMemcpyHostToDevice, st));
				id_list = ids.as<const uint64_t>();
			}
			keep.mark_ids(id_list, n_ids, st);
		}
		keep.count_rank(st);
		HIP_TRY(h, hipGetLastError());
		const dim3 tiles((uint32_t)(keep.words / 4));
		HIP_TRY(h, hipMalloc(&base, h->capacity * row_bytes));
		CompactRowsParams cp{};
		cp.bits = keep.bits();
		cp.word_rank = keep.word_rank();
		cp.src = (const uint4*)h->d_base;
		cp.dst = base.as<uint4>();
		cp.chunks = (uint32_t)(row_bytes / 16);
		hipLaunchKernelGGL(compact_rows_kernel, tiles, dim3(kBlock), 0, st, cp);
		have_copy = float_rows(h) && h->d_base_f16 && h->f16_scale > 0.0f && h->f16_tb > 0;  // (a complete copy)
		if (have_copy) {
			const size_t ld2 = (size_t)f16_ld(h->dim) * 2, alloc = h->f16_rows_alloc;
			HIP_TRY(h, hipMalloc(&f16, alloc * ld2));
			HIP_TRY(h, hipMalloc(&bnorm, sizeof(float) * alloc));
			HIP_TRY(h, hipMalloc(&bns, sizeof(float) * alloc));
			HIP_TRY(h, hipMalloc(&bnmax, 4 * sizeof(float)));
			HIP_TRY(h, hipMemsetAsync(f16, 0, alloc * ld2, st));
			HIP_TRY(h, hipMemsetAsync(bnorm, 0xFF, sizeof(float) * alloc, st));  // 0xFFFFFFFF: a NaN
			HIP_TRY(h, hipMemsetAsync(bns, 0xFF, sizeof(float) * alloc, st));
			HIP_TRY(h, hipMemsetAsync(bnmax, 0, 4 * sizeof(float), st));
			cp.src = h->d_base_f16.as<const uint4>();
			cp.dst = f16.as<uint4>();
			cp.chunks = (uint32_t)(ld2 / 16);
			cp.t0_src = h->d_bnorm_f16;
			cp.t1_src = h->d_bns_f16;
			cp.t0_dst = bnorm;
			cp.t1_dst = bns;
			hipLaunchKernelGGL(compact_rows_kernel, tiles, dim3(kBlock), 0, st, cp);
			SurvivorMaximaParams mp;
			mp.rows = h->d_base;
			mp.bits = keep.bits();
			mp.n = (uint32_t)n;
			mp.d = (uint32_t)h->dim;
			mp.bnmax_bits = bnmax.as<uint32_t>() + 2;
			mp.maxabs_bits = keep.stat() + 3;
			const dim3 grid((uint32_t)std::min<size_t>((n + kRowsPerGroup - 1) / kRowsPerGroup, 8192));
			if (f16_rows(h))
				hipLaunchKernelGGL(survivor_maxima_kernel<_Float16>, grid, dim3(kBlock), 0, st, mp);
			else
				hipLaunchKernelGGL(survivor_maxima_kernel<float>, grid, dim3(kBlock), 0, st, mp);
		}
		HIP_TRY(h, hipGetLastError());
		// the one host wait of a remove
		HIP_TRY(h, hipMemcpyAsync(seen, keep.stat(), sizeof(seen), hipMemcpyDeviceToHost, st));
		HIP_TRY(h, hipStreamSynchronize(st));
		return EXPANN_OK;
	}
	// (after `st` has drained and plan_remove has accepted)  The rows are replaced: everything that described the
	// longer index goes, the fp16 copy excepted where the plan carries it over.
	void commit(expann_index* h, const RemovePlan& plan) {
		h->stat_remove[1] += h->n - plan.n;
		h->forget<OtherCopies>();
		drop_row_filter(h);
		drop_row_groups(h);
		h->d_base.own(std::exchange(base.p, nullptr));  // (the capacity is the old one: no "base_reallocs")
		h->n = plan.n;
		if (plan.copies == RemoveCopy::kCompact) {
			h->d_base_f16 = std::move(f16);
			h->d_bnorm_f16 = std::move(bnorm);
			h->d_bns_f16 = std::move(bns);
			h->d_bnmax = std::move(bnmax);  // (slot [1] went with OtherCopies)
			h->f16_n_pad = (plan.n + h->f16_tb - 1) / h->f16_tb * h->f16_tb;
			h->f16_maxabs = __builtin_bit_cast(float, seen[3]);
			h->stat_remove[2]++;
		} else if (plan.copies == RemoveCopy::kDrop) {
			// append's kDrop: the copy (or the mark) dies and is made again now where a build makes it.  The rows
			// are out, so the remove has succeeded whatever becomes of the copy.
			h->forget<F16Copy>();
			h->stat_remove[3]++;
			if (f16_copy_at_build(plan_index(h)))
				(void)ensure_f16(h, find_f16(f16_geometry(h->dim), h->dim), h->stream);  // (forgets what it began when it fails)
		}
	}
};

// ids: n_ids of them in host (on_device = false) or device memory, read in the order of `user_st`; ids == nullptr with
// from_filter: the rows the row filter in force disallows
int remove_rows(expann_index* h, const uint64_t* ids, size_t n_ids, bool on_device, hipStream_t user_st, bool from_filter,
                size_t* n_removed) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (from_filter && !h->filter_on)
		return h->fail(EXPANN_ERR_INVALID_ARG, "compact_row_filter: no row filter in force");
	const AppendState state = append_state(h, from_filter || ids != nullptr);
	RemovePlan plan = plan_remove(state, n_ids);  // (no device call before these checks)
	if (plan.status != EXPANN_OK)
		return h->fail(plan.status, plan.message);
	if (from_filter && h->n_allowed == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "compact_row_filter: the filter allows no row (an index is never empty)");
	if (n_removed)
		*n_removed = 0;
	if (n_ids == 0) {
		h->stat_remove[0]++;
		return EXPANN_OK;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	if (const int rc = append_wait(h))
		return rc;
	if (from_filter && h->n_allowed == h->n) {  // nothing to remove: the filter goes, every copy stays
		drop_row_filter(h);
		h->stat_remove[0]++;
		return EXPANN_OK;
	}
	CompactedRows aside;
	if (const int rc = aside.build(h, from_filter ? nullptr : ids, n_ids, on_device, user_st ? user_st : h->stream))
		return rc;
	plan = plan_remove(state, n_ids, aside.seen[2] != 0, aside.seen[0], __builtin_bit_cast(float, aside.seen[3]));
	if (plan.status != EXPANN_OK)
		return h->fail(plan.status, plan.message);
	const size_t removed = h->n - plan.n;
	h->stat_remove[0]++;
	if (removed)
		aside.commit(h, plan);
	if (n_removed)
		*n_removed = removed;
	return EXPANN_OK;
}
}  // namespace
}  // extern "C++"

int expann_remove(expann_index* h, const uint64_t* ids, size_t n_ids, size_t* n_removed) {
	return remove_rows(h, ids, n_ids, false, nullptr, false, n_removed);
}

int expann_remove_device(expann_index* h, const uint64_t* d_ids, size_t n_ids, void* stream, size_t* n_removed) {
	return remove_rows(h, d_ids, n_ids, true, (hipStream_t)stream, false, n_removed);
}

int expann_compact_row_filter(expann_index* h, size_t* n_removed) {
	return remove_rows(h, nullptr, 1, false, nullptr, true, n_removed);
}

int expann_search_device(expann_index* h, const void* d_queries, size_t m, size_t k,
                         uint64_t* d_ids, float* d_dists, void* stream) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "search before build()");
	if (k == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "k == 0");
	if (k > kMaxK)  // (by value, before any GPU work: never a matter of the data)
		return h->fail(EXPANN_ERR_UNSUPPORTED, k_too_large());
	if (m == 0)
		return EXPANN_OK;
	if (!d_queries || !d_ids)
		return h->fail(EXPANN_ERR_INVALID_ARG, "NULL query/ids pointer");
	HIP_TRY(h, hipSetDevice(h->device));
	hipStream_t st = stream ? (hipStream_t)stream : h->stream;
	// all searches of a handle share one workspace: deferred searches still running on ANOTHER
	// stream are drained before this one is enqueued (their flag blocks stay in the ring for
	// expann_sync); on one stream the stream order does this
	if (h->async_pending > 0 && h->async_stream != st) {
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
		h->async_stream = st;
	}
	const size_t qbytes = (size_t)h->dim * h->q_elem;
	h->stat_redo_queries = 0;
	h->stat_redo_candidates = 0;
	h->stat_rerank_rows = 0;
	for (size_t q0 = 0; q0 < m; q0 += kMaxQueriesPerPass) {
		const size_t mm = std::min(kMaxQueriesPerPass, m - q0);
		int rc = search_pass(h, (const char*)d_queries + q0 * qbytes, mm, k, d_ids + q0 * k,
		                     d_dists ? d_dists + q0 * k : nullptr, st);
		if (rc != EXPANN_OK)
			return rc;
	}
	return EXPANN_OK;
}

int expann_sync(expann_index* h) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (h->async_pending == 0)
		return EXPANN_OK;
	HIP_TRY(h, hipSetDevice(h->device));
	const uint32_t n = h->async_pending;
	h->async_pending = 0;
	HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	uint32_t bad = 0;
	uint64_t redo_queries = 0, redo_candidates = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t* f = h->h_flag_ring + kRingWords * i;
		const uint32_t mark = f[kRingMark];
		float qmax, scale;
		std::memcpy(&qmax, &f[2], sizeof(float));
		std::memcpy(&scale, &f[kRingScale], sizeof(float));
		const bool redo_word = (mark & 0x40000000u) != 0;  // (speculative thresholds: word 3 is the search's redo word)
		if (redo_word && f[3] >= kRedoOverflowUnit)
			h->stat_redo_overflows++;
		else if (redo_word)
			redo_queries += f[3], redo_candidates += f[6];
		if (f[0] != 0 || (mark == 1 && f[1] != 0) || (scale > 0.0f && !(qmax * scale <= 60000.0f)) ||
		    (redo_word && f[3] >= kRedoOverflowUnit))
			++bad;
		unsigned long long tot;
		std::memcpy(&tot, f + 4, sizeof(tot));
		h->prof.candidates = tot;
		if ((mark & 0x80000000u) && tot > (mark & 0x3FFFFFFFu) && h->i8f_state == 1)  // (i8f_cand_limit)
			h->i8f_state = 2;
	}
	h->stat_redo_queries = redo_queries;
	h->stat_redo_candidates = redo_candidates;
	if (bad)
		return h->fail(EXPANN_ERR_OVERFLOW, std::to_string(bad) + " of " + std::to_string(n) +
		                                        " deferred searches need the synchronous retry "
		                                        "(candidate overflow or queries outside the filter's range): "
		                                        "repeat them with async_search = 0");
	return EXPANN_OK;
}

int expann_search(expann_index* h, const void* queries, size_t m, size_t k, uint64_t* ids,
                  float* dists) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "search before build()");
	if (k == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "k == 0");
	if (k > kMaxK)  // (by value, before any GPU work: never a matter of the data)
		return h->fail(EXPANN_ERR_UNSUPPORTED, k_too_large());
	if (m == 0)
		return EXPANN_OK;
	if (!queries || !ids)
		return h->fail(EXPANN_ERR_INVALID_ARG, "NULL query/ids pointer");
	if (h->async_pending) {  // deferred searches first
		const int rs = expann_sync(h);
		if (rs != EXPANN_OK)
			return rs;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t qbytes = m * (size_t)h->dim * h->q_elem;
	HIP_TRY(h, h->d_q.ensure(qbytes));
	if (m * k <= 16384 && qbytes <= (256u << 10) && m <= kMaxQueriesPerPass && h->opt_latency_mode) {
		const size_t ids_off = (qbytes + 63) / 64 * 64;
		const size_t dists_off = ids_off + sizeof(uint64_t) * m * k;
		const size_t need = dists_off + sizeof(float) * m * k;
		if (need > h->h_pin_bytes) {
			h->h_pin.reset();
			h->h_pin_bytes = 0;
			const size_t want = std::max<size_t>(need, 64u << 10);
			HIP_TRY(h, hipHostMalloc(&h->h_pin, want, hipHostMallocDefault));
			h->h_pin_bytes = want;
		}
		char* pin = h->h_pin.as<char>();
		std::memcpy(pin, queries, qbytes);
		// fp32 index with its fp16 copy in place and at most one workgroup of queries: the query
		// prep kernel reads them straight from pinned memory (and makes the device copy); otherwise
		// one async copy
		const void* dq = h->d_q;
		// (a row filter's list path runs no prep kernel: planned with the longest lists, it is not an fp16 family)
		if (h->d_base_f16 && h->f16_scale > 0.0f && h->opt_scan_kernel == 0 && m <= (size_t)kRowsPerGroup &&
		    is_f16(plan_scan(plan_index(h), PlanCall{m, k, kMaxCap}, PlanAttempt{}).family)) {
			h->q_in_pinned_host = true;
			dq = pin;
		} else {
			HIP_TRY(h, hipMemcpyAsync(h->d_q, pin, qbytes, hipMemcpyHostToDevice, h->stream));
		}
		// (search_pass ends with the flag read-back and a stream sync: the results are complete)
		h->host_call = true;
		int rc = expann_search_device(h, dq, m, k, (uint64_t*)(pin + ids_off), (float*)(pin + dists_off),
		                              h->stream);
		h->host_call = false;
		if (h->q_in_pinned_host) {  // (a path that did not run the prep kernel read the queries over PCIe)
			h->q_in_pinned_host = false;
		}
		if (rc != EXPANN_OK)
			return rc;
		std::memcpy(ids, pin + ids_off, sizeof(uint64_t) * m * k);
		if (dists)
			std::memcpy(dists, pin + dists_off, sizeof(float) * m * k);
		return EXPANN_OK;
	}
	HIP_TRY(h, h->d_ids.ensure(sizeof(uint64_t) * m * k));
	HIP_TRY(h, h->d_dists.ensure(sizeof(float) * m * k));
	HIP_TRY(h, hipMemcpyAsync(h->d_q, queries, qbytes, hipMemcpyHostToDevice, h->stream));
	h->host_call = true;
	int rc = expann_search_device(h, h->d_q, m, k, h->d_ids, h->d_dists, h->stream);
	h->host_call = false;
	if (rc != EXPANN_OK)
		return rc;
	HIP_TRY(h, hipMemcpyAsync(ids, h->d_ids, sizeof(uint64_t) * m * k, hipMemcpyDeviceToHost,
	                          h->stream));
	if (dists)
		HIP_TRY(h, hipMemcpyAsync(dists, h->d_dists, sizeof(float) * m * k,
		                          hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return EXPANN_OK;
}

int expann_merge_topk_strided_device(int device, const uint64_t* d_in_ids, const float* d_in_dists,
                                     size_t ids_stride, size_t dists_stride, size_t n_lists, size_t m,
                                     size_t k, uint64_t* d_out_ids, float* d_out_dists, void* stream) {
	if (!d_in_ids || !d_in_dists || !d_out_ids || !d_out_dists || n_lists == 0 || n_lists > 64 ||
	    k == 0) {
		g_create_error = "expann_merge_topk_device: bad arguments (1 <= n_lists <= 64)";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (m == 0)
		return EXPANN_OK;
	if (hipSetDevice(device) != hipSuccess) {
		g_create_error = "hipSetDevice failed";
		return EXPANN_ERR_HIP;
	}
	if (m >= (1ull << 31) || n_lists * k >= (1ull << 31)) {
		g_create_error = "expann_merge_topk_device: m or n_lists * k beyond 2^31";
		return EXPANN_ERR_INVALID_ARG;
	}
	// one wave per query; the query's n_lists * k entries staged in LDS while they fit 48 KiB
	const size_t lds = n_lists * k * 12;
	if (lds <= (48u << 10))
		hipLaunchKernelGGL(merge_topk_kernel<true>, dim3((uint32_t)m), dim3(kWave), lds, (hipStream_t)stream, d_in_ids,
		                   d_in_dists, ids_stride, dists_stride, (uint32_t)n_lists, (uint32_t)m, (uint32_t)k, d_out_ids,
		                   d_out_dists);
	else
		hipLaunchKernelGGL(merge_topk_kernel<false>, dim3((uint32_t)m), dim3(kWave), 0, (hipStream_t)stream, d_in_ids,
		                   d_in_dists, ids_stride, dists_stride, (uint32_t)n_lists, (uint32_t)m, (uint32_t)k, d_out_ids,
		                   d_out_dists);
	if (hipGetLastError() != hipSuccess) {
		g_create_error = "merge_topk_kernel launch failed";
		return EXPANN_ERR_HIP;
	}
	return EXPANN_OK;
}

int expann_merge_topk_device(int device, const uint64_t* d_in_ids, const float* d_in_dists,
                             size_t n_lists, size_t m, size_t k, uint64_t* d_out_ids,
                             float* d_out_dists, void* stream) {
	return expann_merge_topk_strided_device(device, d_in_ids, d_in_dists, m * k, m * k, n_lists, m, k,
	                                        d_out_ids, d_out_dists, stream);
}

int expann_score_ids(expann_index* h, const void* query, const uint64_t* ids, size_t n_ids,
                     float cutoff, uint64_t* kept_ids, float* kept_scores, size_t* n_kept) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "score_ids before build()");
	if (!n_kept || (n_ids && (!query || !ids || !kept_ids || !kept_scores)))
		return h->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	*n_kept = 0;
	if (n_ids == 0)
		return EXPANN_OK;
	if (n_ids >= (1ull << 32))
		return h->fail(EXPANN_ERR_INVALID_ARG, "more than 2^32 ids");
	for (size_t i = 0; i < n_ids; ++i)
		if (ids[i] < h->id_offset || ids[i] - h->id_offset >= h->n)
			return h->fail(EXPANN_ERR_INVALID_ARG, "id out of range");
	HIP_TRY(h, hipSetDevice(h->device));
	DevBuf b_query, b_idl, b_sc, b_q8s, b_bad;
	const size_t qb = (size_t)h->dim * h->q_elem;
	HIP_TRY(h, b_query.alloc(qb));
	HIP_TRY(h, b_idl.alloc(sizeof(uint64_t) * n_ids));
	HIP_TRY(h, b_sc.alloc(sizeof(float) * n_ids));
	void *d_query = b_query.p, *d_idl = b_idl.p, *d_sc = b_sc.p, *d_q8s = nullptr;
	uint32_t* d_bad = nullptr;
	HIP_TRY(h, hipMemcpyAsync(d_query, query, qb, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(h, hipMemcpyAsync(d_idl, ids, sizeof(uint64_t) * n_ids, hipMemcpyHostToDevice, h->stream));
	const uint32_t blocks = (uint32_t)((n_ids + kRowsPerGroup - 1) / kRowsPerGroup);
	uint32_t bad_host = 0;
	if (float_rows(h)) {
		const ScoreVariant* sv = nullptr;
		for (const auto& v : kScoreF32)
			if (v.d == h->dim && v.ip == (h->metric == EXPANN_METRIC_IP) && !f16_rows(h))
				sv = &v;
		if (!sv && any_dim_f32(h->dim))
			sv = f16_rows(h) ? &kScoreF16Any[h->metric == EXPANN_METRIC_IP ? 1 : 0]
			                 : &kScoreF32Any[h->metric == EXPANN_METRIC_IP ? 1 : 0];
		if (!sv)
			return h->fail(EXPANN_ERR_UNSUPPORTED, "no score kernel for this dim");
		ScoreIdsParams sp{h->d_base, d_query, (const uint64_t*)d_idl, h->id_offset,
		                  (uint32_t)n_ids, (float*)d_sc, (uint32_t)h->dim};
		hipLaunchKernelGGL(sv->fn, dim3(blocks), dim3(kBlock), 0, h->stream, sp);
	} else {
		const ScoreI8Variant* sv = nullptr;
		for (const auto& v : kScoreI8)
			if (v.d == h->dim && v.mode == h->int_mode)
				sv = &v;
		if (!sv && any_dim_i8(h->dim, h->int_mode))
			for (const auto& v : kScoreI8Any)
				if (v.mode == h->int_mode)
					sv = &v;
		if (!sv)
			return h->fail(EXPANN_ERR_UNSUPPORTED, "no 8-bit score kernel for this dim");
		const void* qptr = d_query;
		if (h->dtype == EXPANN_DTYPE_U8) {
			HIP_TRY(h, b_q8s.alloc((size_t)h->dim));
			HIP_TRY(h, b_bad.alloc(sizeof(uint32_t)));
			d_q8s = b_q8s.p;
			d_bad = b_bad.as<uint32_t>();
			HIP_TRY(h, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), h->stream));
			hipLaunchKernelGGL(u8_query_prep_kernel, dim3((uint32_t)((h->dim + kBlock - 1) / kBlock)),
			                   dim3(kBlock), 0, h->stream, (const float*)d_query, (size_t)h->dim,
			                   (uint8_t*)d_q8s, d_bad, (uint32_t*)nullptr);
			HIP_TRY(h, hipMemcpyAsync(&bad_host, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost,
			                          h->stream));
			qptr = d_q8s;
		}
		ScoreIdsI8Params sp{h->d_base, qptr, (const uint64_t*)d_idl, h->id_offset, (uint32_t)n_ids,
		                    (float*)d_sc, (uint32_t)h->dim};
		hipLaunchKernelGGL(sv->fn, dim3(blocks), dim3(kBlock), 0, h->stream, sp);
	}
	// the `d < cutoff` filter, order kept (src/quantizer.h:42-46): compacted on the device, only the
	// survivors and their count come back
	DevBuf b_kid, b_ksc, b_cnt;
	HIP_TRY(h, b_kid.alloc(sizeof(uint64_t) * n_ids));
	HIP_TRY(h, b_ksc.alloc(sizeof(float) * n_ids));
	HIP_TRY(h, b_cnt.alloc(sizeof(uint32_t)));
	FilterScoresParams fp{(const uint64_t*)d_idl, (const float*)d_sc, (uint32_t)n_ids, cutoff, b_kid.as<uint64_t>(),
	                      b_ksc.as<float>(), b_cnt.as<uint32_t>()};
	hipLaunchKernelGGL(filter_scores_kernel, dim3(1), dim3(1024), 0, h->stream, fp);
	HIP_TRY(h, hipGetLastError());
	uint32_t kept = 0;
	HIP_TRY(h, hipMemcpyAsync(&kept, b_cnt.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	if (bad_host)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "query values outside [0,255] for the uint8 metric");
	if (kept) {
		HIP_TRY(h, hipMemcpyAsync(kept_ids, b_kid.p, sizeof(uint64_t) * kept, hipMemcpyDeviceToHost, h->stream));
		HIP_TRY(h, hipMemcpyAsync(kept_scores, b_ksc.p, sizeof(float) * kept, hipMemcpyDeviceToHost, h->stream));
		HIP_TRY(h, hipStreamSynchronize(h->stream));
	}
	*n_kept = kept;
	return EXPANN_OK;
}

// (graph search, the antitopo engine handle and the quantiser builds: expann_graph.hip)

int expann_set_profiling(expann_index* h, int enable) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	HIP_TRY(h, hipSetDevice(h->device));
	if (enable && !h->ev_created) {
		for (int i = 0; i < kEventPairs; ++i) {
			HIP_TRY(h, hipEventCreate(&h->ev[i][0]));
			HIP_TRY(h, hipEventCreate(&h->ev[i][1]));
		}
		h->ev_created = true;
	}
	h->profiling = enable != 0;
	h->ev_used = 0;
	h->prof = expann_profile{};
	h->prof_extra_ms = 0;
	if (h->u8_shadow)
		return expann_set_profiling(h->u8_shadow.get(), enable);
	return EXPANN_OK;
}

int expann_get_profile(expann_index* h, expann_profile* out) {
	if (!h || !out)
		return EXPANN_ERR_INVALID_ARG;
	HIP_TRY(h, hipSetDevice(h->device));
	double ms = 0;
	for (int i = 0; i < h->ev_used; ++i) {
		HIP_TRY(h, hipEventSynchronize(h->ev[i][1]));
		float t = 0;
		HIP_TRY(h, hipEventElapsedTime(&t, h->ev[i][0], h->ev[i][1]));
		ms += t;
	}
	h->prof.scan_ms = ms + h->prof_extra_ms;
	// (launches beyond the event pool are neither timed nor counted while profiling)
	*out = h->prof;
	h->ev_used = 0;
	h->prof_extra_ms = 0;
	h->prof = expann_profile{};
	return EXPANN_OK;
}

int expann_get_stat(expann_index* h, const char* name, uint64_t* out) {
	if (!h || !name || !out)
		return EXPANN_ERR_INVALID_ARG;
	using H = const expann_index*;
	static const struct {
		const char* name;
		uint64_t (*read)(H);
	} kStatTable[] = {
	    {"redo_queries", [](H h) { return h->stat_redo_queries; }},
	    {"redo_candidates", [](H h) { return h->stat_redo_candidates; }},
	    {"redo_overflows", [](H h) { return h->stat_redo_overflows; }},
	    {"spec_rank", [](H h) { return h->stat_spec_rank; }},
	    {"i8_sample", [](H h) { return h->stat_i8_sample; }},
	    {"rerank_rows", [](H h) { return h->stat_rerank_rows; }},
	    {"base_bytes", [](H h) { return h->d_base ? (uint64_t)h->n * (uint64_t)h->dim * h->elem : 0; }},
	    {"filter_active", [](H h) -> uint64_t { return h->filter_on ? 1 : 0; }},
	    {"filter_rows", [](H h) -> uint64_t { return h->filter_on ? h->n_allowed : expann_size(h); }},
	    {"groups_active", [](H h) -> uint64_t { return h->groups_on ? 1 : 0; }},
	    {"group_count", [](H h) -> uint64_t { return h->groups_on ? h->group_dir.keys.size() : 0; }},
	    {"group_list_queries", [](H h) { return h->stat_group[0]; }},
	    {"group_filter_queries", [](H h) { return h->stat_group[1]; }},
	    {"group_any_queries", [](H h) { return h->stat_group[2]; }},
	    {"group_pad_queries", [](H h) { return h->stat_group[3]; }},
	    {"group_filter_passes", [](H h) { return h->stat_group[4]; }},
	    {"range_list_queries", [](H h) { return h->stat_range[0]; }},
	    {"range_topk_queries", [](H h) { return h->stat_range[1]; }},
	    {"range_retries", [](H h) { return h->stat_range[2]; }},
	    {"append_calls", [](H h) { return h->stat_append[0]; }},
	    {"append_rows", [](H h) { return h->stat_append[1]; }},
	    {"append_extends", [](H h) { return h->stat_append[2]; }},
	    {"append_rebuilds", [](H h) { return h->stat_append[3]; }},
	    {"base_reallocs", [](H h) { return h->stat_append[4]; }},
	    {"remove_calls", [](H h) { return h->stat_remove[0]; }},
	    {"remove_rows", [](H h) { return h->stat_remove[1]; }},
	    {"remove_compacts", [](H h) { return h->stat_remove[2]; }},
	    {"remove_rebuilds", [](H h) { return h->stat_remove[3]; }},
	    {"base_capacity_rows", [](H h) -> uint64_t { return h->d_base ? h->capacity : h->reserved; }},
	    {"copies_digest", [](H h) { return copies_digest(const_cast<expann_index*>(h)); }},
	};
	for (const auto& s : kStatTable)
		if (!std::strcmp(name, s.name)) {
			*out = s.read(h);
			return EXPANN_OK;
		}
	return h->fail(EXPANN_ERR_INVALID_ARG, std::string("unknown statistic ") + name);
}

uint32_t expann_spec_rank_auto(size_t k, uint32_t sample_frac) {
	return spec_rank_auto(k, sample_frac ? 1.0 / (double)sample_frac : 1.0);
}

// ---- row filter ------------------------------------------------------------------------
namespace {
// The engine's own buffers for a filter of the current rows; the filter is off until filter_finish.  *words = the
// words of the engine's bitmap: whole tiles of the fp16 copy (<= 128 rows each).
int filter_begin(expann_index* h, size_t* words_out) {
	const size_t words = (h->n + 127) / 128 * 4;
	if (words != h->filter_words || !h->d_filter_bits) {
		h->filter_on = false;
		h->d_filter_bits.reset();
		h->filter_words = 0;
		HIP_TRY(h, hipMalloc(&h->d_filter_bits, sizeof(uint32_t) * words));
		h->filter_words = words;
	}
	if (!h->d_filter_stat)
		HIP_TRY(h, hipMalloc(&h->d_filter_stat, sizeof(uint32_t) * (2 + kFilterSegs)));
	if (!h->d_filter_list)
		HIP_TRY(h, hipMalloc(&h->d_filter_list, sizeof(uint32_t) * kFilterListCap));
	h->filter_on = false;  // (until the new filter is complete)
	h->filter_terms_valid = false;
	*words_out = words;
	return EXPANN_OK;
}

// The bits are in d_filter_bits (in the order of `st`): count, residues and the list of allowed rows; the filter is on.
int filter_finish(expann_index* h, hipStream_t st, size_t words) {
	HIP_TRY(h, hipMemsetAsync(h->d_filter_stat, 0, sizeof(uint32_t) * (2 + kFilterSegs), st));
	hipLaunchKernelGGL(filter_count_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, h->d_filter_bits.as<uint32_t>(),
	                   (uint32_t)h->n, (uint32_t)words, h->d_filter_stat.as<uint32_t>(), h->d_filter_stat + 2);
	HIP_TRY(h, hipGetLastError());
	uint32_t stat[2] = {0, 0};
	HIP_TRY(h, hipMemcpyAsync(stat, h->d_filter_stat, sizeof(stat), hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));  // the planner needs the count on the host: one wait per filter change
	h->n_allowed = stat[0];
	h->filter_residues = stat[1];
	h->filter_list_stride = (uint32_t)std::max<size_t>(1, (h->n_allowed + kFilterListCap - 1) / kFilterListCap);
	h->filter_list_len = (uint32_t)((h->n_allowed + h->filter_list_stride - 1) / h->filter_list_stride);
	if (h->n_allowed) {
		hipLaunchKernelGGL(filter_compact_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, h->d_filter_bits.as<const uint32_t>(),
		                   (uint32_t)words, h->d_filter_stat.as<const uint32_t>() + 2, h->filter_list_stride,
		                   h->d_filter_list.as<uint32_t>(), kFilterListCap);
		HIP_TRY(h, hipGetLastError());
		HIP_TRY(h, hipStreamSynchronize(st));
	}
	h->filter_on = true;
	return EXPANN_OK;
}

// bits: n_words words in host (on_device = false) or device memory, read in the order of `st`
int set_row_filter(expann_index* h, const uint32_t* bits, size_t n_words, bool on_device, hipStream_t user_st) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!bits)
		return h->fail(EXPANN_ERR_INVALID_ARG, "row filter: NULL bits");
	if (!float_rows(h))
		return h->fail(EXPANN_ERR_UNSUPPORTED,
		               "row filter: fp32 / fp16 rows only (8-bit and int16 rows have integer row terms)");
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "row filter before build()");
	const size_t need_words = (h->n + 31) / 32;
	if (n_words < need_words)
		return h->fail(EXPANN_ERR_INVALID_ARG, "row filter: " + std::to_string(n_words) + " words for " +
		                                           std::to_string(h->n) + " rows (need " + std::to_string(need_words) + ")");
	HIP_TRY(h, hipSetDevice(h->device));
	// deferred searches still read the old filter: as before a search on another stream, they are waited for
	// (their flag blocks stay in the ring for expann_sync)
	if (h->async_pending > 0)
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	hipStream_t st = user_st ? user_st : h->stream;
	size_t words = 0;
	if (const int rc = filter_begin(h, &words))
		return rc;
	HIP_TRY(h, hipMemsetAsync(h->d_filter_bits, 0, sizeof(uint32_t) * words, st));
	HIP_TRY(h, hipMemcpyAsync(h->d_filter_bits, bits, sizeof(uint32_t) * need_words,
	                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
	return filter_finish(h, st, words);
}

// ---- row groups ---------------------------------------------------------
// "group_list_rows" = 0: every group the select can sort takes the list kernel.  Measured on 1 M x d128, k = 10
// (profiles/bf_groups_ab.txt, part c): groups of 1 024 .. 16 384 rows, 10 and 100 queries per group -- the list kernel
// was never slower than the filter passes (x 0.005 .. x 0.82 of their time), so there is no crossover below kMaxCap
constexpr uint32_t kGroupListRowsAuto = kMaxCap;
// keys of one list pass's candidate lists (1 GiB): bounds the slots of a pass together with kMaxQueriesPerPass
constexpr size_t kGroupPassKeys = (size_t)1 << 27;

// labels: n of them in host (on_device = false) or device memory, read in the order of `user_st`
int set_row_groups(expann_index* h, const uint32_t* groups, size_t n, bool on_device, hipStream_t user_st) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!groups)
		return h->fail(EXPANN_ERR_INVALID_ARG, "row groups: NULL labels");
	if (!float_rows(h))
		return h->fail(EXPANN_ERR_UNSUPPORTED,
		               "row groups: fp32 / fp16 rows only (the filter passes of large groups need the row filter)");
	if (n != expann_size(h))
		return h->fail(EXPANN_ERR_INVALID_ARG,
		               "row groups: " + std::to_string(n) + " labels for " + std::to_string(expann_size(h)) + " rows");
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "row groups before build()");
	HIP_TRY(h, hipSetDevice(h->device));
	// deferred searches are waited for, as before a filter change (their flag blocks stay in the ring for expann_sync)
	if (h->async_pending > 0)
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	hipStream_t st = user_st ? user_st : h->stream;
	std::vector<uint32_t> lab;
	if (int rc = fetch_group_labels(h, groups, n, on_device, st, lab))
		return rc;
	GroupDirectory dir = build_group_directory(lab.data(), n);
	DevPtr<uint32_t> b_lab, b_rows;  // built aside: a failed call leaves the groups as they were
	HIP_TRY(h, hipMalloc(&b_lab, sizeof(uint32_t) * n));
	HIP_TRY(h, hipMalloc(&b_rows, sizeof(uint32_t) * std::max<size_t>(dir.n_rows(), 1)));
	HIP_TRY(h, hipMemcpy(b_lab, lab.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
	if (dir.n_rows())
		HIP_TRY(h, hipMemcpy(b_rows, dir.rows.data(), sizeof(uint32_t) * dir.n_rows(), hipMemcpyHostToDevice));
	std::vector<uint32_t>().swap(dir.rows);  // (the rows live on the device)
	std::swap(h->d_row_groups.p, b_lab.p);   // (the old buffers go with the locals)
	std::swap(h->d_group_rows.p, b_rows.p);
	h->group_dir = std::move(dir);
	h->groups_on = true;
	return EXPANN_OK;
}

// the checks of a grouped search, expann_search's first and in its order; *empty: m == 0, nothing to do
int grouped_args(expann_index* h, const void* queries, const uint32_t* query_groups, size_t m, size_t k, const uint64_t* ids,
                 bool* empty) {
	*empty = false;
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "search before build()");
	if (k == 0)
		return h->fail(EXPANN_ERR_INVALID_ARG, "k == 0");
	if (k > kMaxK)
		return h->fail(EXPANN_ERR_UNSUPPORTED, k_too_large());
	if (m == 0) {
		*empty = true;
		return EXPANN_OK;
	}
	if (!queries || !ids)
		return h->fail(EXPANN_ERR_INVALID_ARG, "NULL query/ids pointer");
	if (!query_groups)
		return h->fail(EXPANN_ERR_INVALID_ARG, "NULL query_groups");
	if (!h->groups_on)
		return h->fail(EXPANN_ERR_NOT_BUILT, "grouped search: no row groups are set (expann_set_row_groups)");
	if (h->filter_on)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "grouped search under a row filter: combining the bitmap with groups is not offered");
	return EXPANN_OK;
}

// One tier of a grouped batch through the plain pipeline: the queries idx[0, cnt) (device array of the caller's query
// numbers) are gathered into contiguous staging, search_pass serves them -- under whatever filter is in force --
// and the result rows are scattered back.
int grouped_tier(expann_index* h, const void* d_queries, const uint32_t* d_idx, size_t cnt, size_t k, uint64_t* d_ids,
                 float* d_dists, hipStream_t st) {
	const uint32_t row_words = (uint32_t)h->dim;  // (fp32 queries)
	for (size_t q0 = 0; q0 < cnt; q0 += kMaxQueriesPerPass) {
		const size_t mm = std::min(kMaxQueriesPerPass, cnt - q0);
		const size_t q_need = sizeof(uint32_t) * mm * row_words, i_need = sizeof(uint64_t) * mm * k;
		const size_t d_need = d_dists ? sizeof(float) * mm * k : 0;
		if (q_need > h->d_group_q.bytes || i_need > h->d_group_ids.bytes || d_need > h->d_group_dists.bytes)
			HIP_TRY(h, hipStreamSynchronize(st));  // (growing frees the old block: the tier before has drained first)
		HIP_TRY(h, h->d_group_q.ensure(q_need));
		HIP_TRY(h, h->d_group_ids.ensure(i_need));
		if (d_dists)
			HIP_TRY(h, h->d_group_dists.ensure(d_need));
		const uint32_t grid = (uint32_t)std::min<size_t>((mm * row_words + kBlock - 1) / kBlock, 4096);
		hipLaunchKernelGGL(group_gather_rows_kernel, dim3(grid), dim3(kBlock), 0, st, (const uint32_t*)d_queries, d_idx + q0,
		                   (uint32_t)mm, row_words, h->d_group_q.as<uint32_t>());
		HIP_TRY(h, hipGetLastError());
		float* const t_dists = d_dists ? h->d_group_dists.get() : nullptr;
		const int rc = search_pass(h, h->d_group_q, mm, k, h->d_group_ids, t_dists, st);
		if (rc != EXPANN_OK)
			return rc;
		const uint32_t grid2 = (uint32_t)std::min<size_t>((mm * k + kBlock - 1) / kBlock, 4096);
		hipLaunchKernelGGL(group_scatter_results_kernel, dim3(grid2), dim3(kBlock), 0, st, (const uint64_t*)h->d_group_ids.get(),
		                   (const float*)t_dists, d_idx + q0, (uint32_t)mm, (uint32_t)k, d_ids, d_dists);
		HIP_TRY(h, hipGetLastError());
		// (the staging is reused by the next pass and the next tier: in stream order)
	}
	return EXPANN_OK;
}

using GroupScanFn = void (*)(GroupScanParams);
GroupScanFn group_scan_fn(const expann_index* h) {
	const bool ip = h->metric == EXPANN_METRIC_IP;
	if (f16_rows(h))
		return ip ? group_list_scan_kernel<kGroupScanTQ, true, _Float16> : group_list_scan_kernel<kGroupScanTQ, false, _Float16>;
	return ip ? group_list_scan_kernel<kGroupScanTQ, true, float> : group_list_scan_kernel<kGroupScanTQ, false, float>;
}

// A grouped search on device buffers (the checks are done): plan on the host, enqueue on `st`, return when it has drained.
int grouped_search_device(expann_index* h, const void* d_queries, const uint32_t* qg, size_t m, size_t k, uint64_t* d_ids,
                          float* d_dists, hipStream_t st) {
	if (m >= (1ull << 32))
		return h->fail(EXPANN_ERR_UNSUPPORTED, "grouped search: more than 2^32 queries");
	struct HostCall {  // every pass below is the waiting form, whatever "async_search" says; no filter is left behind
		expann_index* h;
		bool was;
		~HostCall() {
			h->host_call = was;
			h->filter_on = false;
		}
	} guard{h, h->host_call};
	h->host_call = true;
	for (uint64_t& s : h->stat_group)
		s = 0;
	h->stat_redo_queries = 0;
	h->stat_redo_candidates = 0;
	h->stat_rerank_rows = 0;
	const GroupDirectory& dir = h->group_dir;
	const size_t G = dir.keys.size();
	const uint32_t L = h->opt_group_list_rows > 0 ? (uint32_t)h->opt_group_list_rows : kGroupListRowsAuto;

	// all ANY, in order: the plain search in place
	bool all_any = true;
	for (size_t i = 0; i < m && all_any; ++i)
		all_any = qg[i] == EXPANN_GROUP_ANY;
	if (all_any) {
		h->stat_group[2] = m;
		const size_t qbytes = (size_t)h->dim * h->q_elem;
		for (size_t q0 = 0; q0 < m; q0 += kMaxQueriesPerPass) {
			const size_t mm = std::min(kMaxQueriesPerPass, m - q0);
			const int rc = search_pass(h, (const char*)d_queries + q0 * qbytes, mm, k, d_ids + q0 * k,
			                           d_dists ? d_dists + q0 * k : nullptr, st);
			if (rc != EXPANN_OK)
				return rc;
		}
		HIP_TRY(h, hipStreamSynchronize(st));
		return EXPANN_OK;
	}

	// bucket the queries: group number, G = ANY, G + 1 = a label no row carries; a stable counting sort when the
	// directory is small beside the batch, a sort of (bucket, query) pairs otherwise
	std::vector<uint32_t> bucket(m), perm(m);
	for (size_t i = 0; i < m; ++i) {
		const size_t gi = qg[i] == EXPANN_GROUP_ANY ? G : dir.find(qg[i]);
		bucket[i] = (uint32_t)(qg[i] != EXPANN_GROUP_ANY && gi == G ? G + 1 : gi);
	}
	if (G + 2 <= 4 * m + 4096) {
		std::vector<uint32_t> start(G + 3, 0);
		for (size_t i = 0; i < m; ++i)
			start[bucket[i] + 1]++;
		for (size_t b = 0; b < G + 2; ++b)
			start[b + 1] += start[b];
		for (size_t i = 0; i < m; ++i)
			perm[start[bucket[i]]++] = (uint32_t)i;
	} else {
		std::vector<uint64_t> ord(m);
		for (size_t i = 0; i < m; ++i)
			ord[i] = ((uint64_t)bucket[i] << 32) | i;
		std::sort(ord.begin(), ord.end());
		for (size_t i = 0; i < m; ++i)
			perm[i] = (uint32_t)ord[i];
	}

	// the tiers: runs of one bucket in perm
	struct Run {
		uint32_t bucket, begin, end;
	};
	std::vector<Run> list_runs, filter_runs;
	Run any_run{0, 0, 0}, pad_run{0, 0, 0};
	uint32_t max_s = 0;
	for (size_t a = 0; a < m;) {
		const uint32_t b = bucket[perm[a]];
		size_t e = a + 1;
		while (e < m && bucket[perm[e]] == b)
			++e;
		const Run r{b, (uint32_t)a, (uint32_t)e};
		if (b == G + 1)
			pad_run = r, h->stat_group[3] = e - a;
		else if (b == G)
			any_run = r, h->stat_group[2] = e - a;
		else {
			const uint32_t s = dir.off[b + 1] - dir.off[b];
			if (s <= L) {
				list_runs.push_back(r);
				h->stat_group[0] += e - a;
				max_s = std::max(max_s, s);
			} else {
				filter_runs.push_back(r);
				h->stat_group[1] += e - a;
			}
		}
		a = e;
	}
	h->stat_group[4] = filter_runs.size();

	// the list tier: slots (one per query, a group's consecutive), passes of slots, work items
	const int cus = num_cus(h->device);
	uint32_t cap = std::max<uint32_t>(2048, pow2ceil(max_s));  // (2048: the select's wave path; a whole number of 16-row steps)
	cap = std::min(std::max(cap, pow2ceil((uint32_t)(2 * k))), kMaxCap);
	const size_t pass_slots = std::min(kMaxQueriesPerPass, kGroupPassKeys / cap);
	struct ListPass {
		uint32_t slot_begin, slots, item_begin, items;
	};
	std::vector<ListPass> passes;
	std::vector<uint32_t> slot_query;
	std::vector<GroupItem> items;
	if (!list_runs.empty()) {
		constexpr uint32_t TQ = kGroupScanTQ;
		uint64_t tile_steps = 0;
		for (const Run& r : list_runs) {
			const uint32_t s = dir.off[r.bucket + 1] - dir.off[r.bucket];
			tile_steps += (uint64_t)((r.end - r.begin + TQ - 1) / TQ) * ((s + kRowsPerGroup - 1) / kRowsPerGroup);
		}
		// ~16 workgroups per CU in total, at least 8 steps (128 rows) per workgroup: the direct scan's rule
		const uint32_t steps_per_item = (uint32_t)std::max<uint64_t>(8, (tile_steps + 16ull * cus - 1) / (16ull * cus));
		slot_query.reserve(h->stat_group[0]);
		ListPass cur{0, 0, 0, 0};
		for (const Run& r : list_runs) {
			const uint32_t s = dir.off[r.bucket + 1] - dir.off[r.bucket];
			const uint32_t steps = (s + kRowsPerGroup - 1) / kRowsPerGroup;
			for (uint32_t a = r.begin; a < r.end; a += TQ) {
				const uint32_t nq = std::min<uint32_t>(TQ, r.end - a);
				if (cur.slots + nq > pass_slots) {  // (a tile never straddles two passes)
					passes.push_back(cur);
					cur = ListPass{cur.slot_begin + cur.slots, 0, (uint32_t)items.size(), 0};
				}
				for (uint32_t g0 = 0; g0 < steps; g0 += steps_per_item) {
					GroupItem it{};
					it.slot0 = cur.slots;  // (relative to the pass)
					it.nq = nq;
					it.list_off = dir.off[r.bucket];
					it.list_len = s;
					it.g0 = g0;
					it.g1 = std::min(steps, g0 + steps_per_item);
					items.push_back(it);
					cur.items++;
				}
				for (uint32_t j = 0; j < nq; ++j)
					slot_query.push_back(perm[a + j]);
				cur.slots += nq;
			}
		}
		passes.push_back(cur);
	}

	// one upload through pinned staging: [perm | slot_query | items]
	const size_t off_slot = sizeof(uint32_t) * m;
	const size_t off_items = (off_slot + sizeof(uint32_t) * slot_query.size() + 31) / 32 * 32;
	const size_t tab_bytes = off_items + sizeof(GroupItem) * items.size();
	if (tab_bytes > h->h_group_tab_bytes) {
		h->h_group_tab.reset();
		h->h_group_tab_bytes = 0;
		const size_t want = std::max<size_t>(tab_bytes + tab_bytes / 2, 64u << 10);
		HIP_TRY(h, hipHostMalloc(&h->h_group_tab, want, hipHostMallocDefault));
		h->h_group_tab_bytes = want;
	}
	HIP_TRY(h, h->d_group_tab.ensure(h->h_group_tab_bytes));
	char* const tab = h->h_group_tab.as<char>();
	std::memcpy(tab, perm.data(), sizeof(uint32_t) * m);
	if (!slot_query.empty())
		std::memcpy(tab + off_slot, slot_query.data(), sizeof(uint32_t) * slot_query.size());
	if (!items.empty())
		std::memcpy(tab + off_items, items.data(), sizeof(GroupItem) * items.size());
	HIP_TRY(h, hipMemcpyAsync(h->d_group_tab, tab, tab_bytes, hipMemcpyHostToDevice, st));
	const char* const d_tab = h->d_group_tab.as<char>();
	const uint32_t* const d_perm = reinterpret_cast<const uint32_t*>(d_tab);
	const uint32_t* const d_slot_query = reinterpret_cast<const uint32_t*>(d_tab + off_slot);
	const GroupItem* const d_items = reinterpret_cast<const GroupItem*>(d_tab + off_items);

	// labels no row carries: padding
	if (pad_run.end > pad_run.begin) {
		const size_t cnt = pad_run.end - pad_run.begin;
		hipLaunchKernelGGL(group_pad_rows_kernel, dim3((uint32_t)std::min<size_t>((cnt * k + kBlock - 1) / kBlock, 4096)),
		                   dim3(kBlock), 0, st, d_perm + pad_run.begin, (uint32_t)cnt, (uint32_t)k, d_ids, d_dists);
		HIP_TRY(h, hipGetLastError());
	}
	// ANY: the plain search
	if (any_run.end > any_run.begin) {
		const int rc = grouped_tier(h, d_queries, d_perm + any_run.begin, any_run.end - any_run.begin, k, d_ids, d_dists, st);
		if (rc != EXPANN_OK)
			return rc;
	}
	// filter groups, in turn: the group's bitmap through the row filter's own path (one host wait each), the filtered
	// search of its queries
	for (const Run& r : filter_runs) {
		size_t words = 0;
		if (const int rc = filter_begin(h, &words))
			return rc;
		hipLaunchKernelGGL(group_bits_kernel, dim3((uint32_t)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   h->d_row_groups.as<const uint32_t>(), (uint32_t)h->n, dir.keys[r.bucket],
		                   h->d_filter_bits.as<uint32_t>(), (uint32_t)words);
		HIP_TRY(h, hipGetLastError());
		if (const int rc = filter_finish(h, st, words))
			return rc;
		const int rc = grouped_tier(h, d_queries, d_perm + r.begin, r.end - r.begin, k, d_ids, d_dists, st);
		h->filter_on = false;
		if (rc != EXPANN_OK)
			return rc;
	}
	// list groups: one scan launch and one select launch per pass (the passes above have drained: the workspace is free)
	if (!passes.empty()) {
		const size_t lds = sizeof(float) * kGroupScanTQ * (size_t)h->dim;
		const GroupScanFn fn = group_scan_fn(h);
		if (lds > (64u << 10) && !h->group_lds_set) {
			HIP_TRY(h, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
			h->group_lds_set = true;
		}
		uint32_t most_slots = 0;
		for (const ListPass& lp : passes)
			most_slots = std::max(most_slots, lp.slots);
		if (const int rc = ensure_workspace(h, most_slots, cap))  // (once: no buffer grows under a pass in flight)
			return rc;
		for (const ListPass& lp : passes) {
			GroupScanParams gp{};
			gp.base = h->d_base;
			gp.n_rows = (uint32_t)h->n;
			gp.dim = (uint32_t)h->dim;
			gp.queries = d_queries;
			gp.slot_query = d_slot_query + lp.slot_begin;
			gp.group_rows = h->d_group_rows;
			gp.items = d_items + lp.item_begin;
			gp.cand_cnt = h->d_cnt;
			gp.cand = h->d_cand;
			gp.cap = cap;
			const bool timed = h->profiling && h->ev_used < kEventPairs;
			if (timed)
				HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
			hipLaunchKernelGGL(fn, dim3(lp.items), dim3(kBlock), lds, st, gp);
			if (timed) {
				HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][1], st));
				h->ev_used++;
			}
			HIP_TRY(h, hipGetLastError());
			SelectParams sel{};
			sel.cand = h->d_cand;
			sel.cand_cnt = h->d_cnt;
			sel.cap = cap;
			sel.k = (uint32_t)k;
			sel.id_offset = h->id_offset;
			sel.out_ids = d_ids;
			sel.out_dists = d_dists;
			sel.dim = (uint32_t)h->dim;
			sel.metric_ip = h->metric == EXPANN_METRIC_IP ? 1u : 0u;
			sel.overflow = h->d_overflow;
			sel.wave0_short = 1;  // (lists of <= 2048 keys: one wave orders them; longer ones: the whole workgroup)
			sel.slot_map = d_slot_query + lp.slot_begin;
			hipLaunchKernelGGL(select_topk_fn(h, sel), dim3(lp.slots), dim3(kBlock), sizeof(uint64_t) * cap + 16, st, sel);
			HIP_TRY(h, hipGetLastError());
		}
	}
	HIP_TRY(h, hipStreamSynchronize(st));
	return EXPANN_OK;
}

// ---- range search (THE RANGE RULE, include/expann_hip.h) ----------------------------------------
// The threshold machine with the caller's radii as tau: no sampled pass, no threshold estimate.  A pass of its own
// beside SearchPass, built from the same launch helpers; the plain and grouped searches launch what they did.
//   stage 1  every query, lists of cap0 keys: the fp16 single-product form (its keys re-scored exactly by the range
//            select) where the plan (bf_plan.hpp) gives one and the queries fit its range, else the exact direct scan
//   stage 2  the queries whose list did not fit, gathered, at kMaxCap keys: the fp16 form again where stage 1 ran it
//            with shorter lists, then -- for what is left -- the exact direct scan, whose counter goes on counting, so
//            the count is exact whatever it is, and the range select over exact keys
//   stage 3  the queries with more than kMaxCap rows in range: their max_results nearest rows are all in range, so
//            they are what the plain pipeline returns for k = max_results
// One host wait per stage that runs (it reads the next stage's list length); a search whose every list fit has one.
// cap0 and the split between the one-wave and the workgroup forms of the select: profiles/range_search_ab.txt.
constexpr uint32_t kRangeCap0 = 1024;      // stage 1's list capacity at least, unless "cand_capacity" sets it (range_search_device)
constexpr uint32_t kRangeWaveMax = 512;    // lists up to this many keys: the one-wave select
constexpr uint32_t kRangeBlockMax = 4096;  // ... up to this many: 256 threads; beyond: 1 024 threads
constexpr size_t kRangeRetryChunk = 2048;  // queries of one stage-2 launch (2 048 x kMaxCap keys = 256 MiB of lists)

// (a diagnostic like EXPANN_DEBUG_LISTS, not an option: EXPANN_RANGE_WAVE_MAX moves the split for the sweep of
// profiles/range_search_ab.py, which found no difference up to 512 keys; unset, the constant holds)
inline uint32_t range_wave_max() {
	static const uint32_t v = [] {
		const char* e = std::getenv("EXPANN_RANGE_WAVE_MAX");
		return e ? (uint32_t)std::min(2048L, std::max(0L, std::atol(e))) : kRangeWaveMax;
	}();
	return v;
}

// the range select over n_slots lists of capacity cap (a power of two): one launch per form that has lists to serve
int launch_range_select(expann_index* h, RangeSelectParams rp, uint32_t n_slots, uint32_t cap, hipStream_t st) {
	using Fn = void (*)(RangeSelectParams);
	const bool hr = f16_rows(h);
	const Fn f64 = hr ? range_select_kernel<_Float16, 64> : range_select_kernel<float, 64>;
	const Fn f256 = hr ? range_select_kernel<_Float16, 256> : range_select_kernel<float, 256>;
	const Fn f1024 = hr ? range_select_kernel<_Float16, 1024> : range_select_kernel<float, 1024>;
	if (!h->range_lds_set) {  // (kMaxCap keys: 128 KiB of the CU's 160 KiB, as select_topk_kernel)
		const int lds = (int)(sizeof(uint64_t) * kMaxCap + 16);
		HIP_TRY(h, hipFuncSetAttribute((const void*)range_select_kernel<float, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
		HIP_TRY(h, hipFuncSetAttribute((const void*)range_select_kernel<_Float16, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
		h->range_lds_set = true;
	}
	rp.cap = cap;
	rp.n_slots = n_slots;
	const uint32_t wave_max = std::min(range_wave_max(), cap);
	auto launch = [&](Fn fn, uint32_t threads, uint32_t len_min, uint32_t len_hi) {
		rp.len_min = len_min;
		rp.len_hi = len_hi;
		rp.takes_overflow = len_hi >= cap ? 1u : 0u;
		rp.lds_keys = std::max<uint32_t>(2, pow2ceil(len_hi));
		hipLaunchKernelGGL(fn, dim3(n_slots), dim3(threads), sizeof(uint64_t) * rp.lds_keys + 16, st, rp);
	};
	uint32_t from = 0;
	if (wave_max > 0) {
		launch(f64, 64, 0, wave_max);
		from = wave_max + 1;
	}
	if (from <= cap && from <= kRangeBlockMax) {
		launch(f256, 256, from, std::min(cap, kRangeBlockMax));
		from = std::min(cap, kRangeBlockMax) + 1;
	}
	if (from <= cap)
		launch(f1024, 1024, from, cap);
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

struct RangePass {
	expann_index* h;
	const void* d_queries;
	const float* d_radii;
	size_t m;
	uint32_t max_results;
	uint64_t* d_ids;
	float* d_dists;
	uint32_t* d_counts;
	hipStream_t st;
	bool ip;
	int cus;
	uint32_t cap0;
	uint32_t n_retry = 0, n_mid = 0, n_big = 0;

	// d_range: [0] / [1] / [2] the lengths of the three lists behind them, m query numbers each
	uint32_t* word(int w) const { return h->d_range.get() + w; }
	uint32_t* retry_list() const { return h->d_range.get() + 4; }          // stage 1's lists could not hold them
	uint32_t* mid_list() const { return h->d_range.get() + 4 + m; }        // nor the fp16 form's at kMaxCap keys
	uint32_t* big_list() const { return h->d_range.get() + 4 + 2 * m; }    // more than kMaxCap rows in range

	ScanPlan plan(size_t mq) const { return plan_scan(plan_index(h), PlanCall{mq, max_results, cap0}, PlanAttempt{}); }
	const GemmF16Variant* f16_form(const ScanPlan& p) const;
	int direct_scan(const void* d_q, size_t mq, int tq, uint32_t cap, const char** kname);
	int filter_stage(bool want_f16, const uint32_t* list, size_t mq, uint32_t cap, int over_word, uint32_t* over_list,
	                 uint32_t* n_over, bool* used_f16, bool* out_of_range);
	int stage3();
	int run();
};

// the fp16 single-product form of a stage's plan (that of a top-k search of as many queries), or nullptr: the exact
// direct scan (never the bf16x3 form or the debug instance, whatever the options say)
const GemmF16Variant* RangePass::f16_form(const ScanPlan& p) const {
	return is_f16(p.family) ? find_f16(f16_geometry(h->dim), h->dim) : nullptr;
}

// the exact direct scan of every row for the mq queries at d_q: tau = h->d_tau[0], tau_row all ones (every row
// that ties with the radius is in range), lists and counters in h->d_cand / h->d_cnt; tq: the plan's query tile
int RangePass::direct_scan(const void* d_q, size_t mq, int tq, uint32_t cap, const char** kname) {
	const ScanVariant* v = find_scan_f32(h->dim, ip, tq, f16_rows(h));
	if (!v)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "no scan kernel for dim " + std::to_string(h->dim) + " / query_tile " +
		                                           std::to_string(h->opt_query_tile));
	HIP_TRY(h, hipMemsetAsync(h->d_cnt, 0, sizeof(uint32_t) * mq, st));
	HIP_TRY(h, hipMemsetAsync(h->d_tau_row[0], 0xFF, sizeof(uint32_t) * mq, st));
	ScanParams sp{};
	sp.base = h->d_base;
	sp.n_rows = (uint32_t)h->n;
	sp.n_groups_sel = (uint32_t)((h->n + kRowsPerGroup - 1) / kRowsPerGroup);
	sp.group_stride = 1;
	sp.n_qtiles = (uint32_t)((mq + v->tq - 1) / v->tq);
	sp.queries = d_q;
	sp.m = (uint32_t)mq;
	sp.tau = h->d_tau[0];
	sp.tau_row = h->d_tau_row[0];
	sp.cand_cnt = h->d_cnt;
	sp.cand = h->d_cand;
	sp.cap = cap;
	sp.dim = (uint32_t)h->dim;
	uint32_t n_chunks = direct_scan_chunks(sp.n_groups_sel, sp.n_qtiles, cus);
	sp.groups_per_block = (sp.n_groups_sel + n_chunks - 1) / n_chunks;
	n_chunks = (sp.n_groups_sel + sp.groups_per_block - 1) / sp.groups_per_block;
	hipLaunchKernelGGL(v->fn, dim3(n_chunks * sp.n_qtiles), dim3(kBlock), 0, st, sp);
	HIP_TRY(h, hipGetLastError());
	*kname = v->name;
	return EXPANN_OK;
}

// One stage over mq queries -- the whole pass (list == nullptr), or the queries list[0, mq) gathered into staging --
// with candidate lists of `cap` keys: the scan (the fp16 form where wanted and available, else the exact direct
// scan), the range select, which answers every query whose list fit and appends the others' numbers to over_list
// (its length: word(over_word), *n_over on the host), and the stage's one host wait.  A hit log that overflowed
// leaves entries missing from lists that look complete, so then EVERY query of the stage is passed on.
int RangePass::filter_stage(bool want_f16, const uint32_t* list, size_t mq, uint32_t cap, int over_word, uint32_t* over_list,
                            uint32_t* n_over, bool* used_f16, bool* out_of_range) {
	*out_of_range = false;
	const ScanPlan stage = plan(mq);
	const GemmF16Variant* gvf = want_f16 ? f16_form(stage) : nullptr;
	if (gvf) {
		const int rc = ensure_f16(h, gvf, st);
		if (rc != EXPANN_OK)
			return rc;
		if (h->f16_scale < 0.0f)  // the index does not fit the fp16 range at any allowed scale
			gvf = nullptr;
	}
	*used_f16 = gvf != nullptr;
	int rc = ensure_workspace(h, mq, cap);  // (it may grow the lists: the stage before has drained)
	if (rc != EXPANN_OK)
		return rc;
	const void* dq = d_queries;
	const float* dr = d_radii;
	if (list) {  // the stage's queries and radii into contiguous staging, as a grouped search's tier
		const uint32_t row_words = (uint32_t)h->dim;  // (fp32 queries)
		HIP_TRY(h, h->d_range_q.ensure(sizeof(uint32_t) * mq * row_words));  // (grows only while the stream is drained)
		const uint32_t grid = (uint32_t)std::min<size_t>((mq * row_words + kBlock - 1) / kBlock, 4096);
		hipLaunchKernelGGL(group_gather_rows_kernel, dim3(grid), dim3(kBlock), 0, st, (const uint32_t*)d_queries, list,
		                   (uint32_t)mq, row_words, h->d_range_q.as<uint32_t>());
		hipLaunchKernelGGL(group_gather_rows_kernel, dim3((uint32_t)((mq + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   (const uint32_t*)d_radii, list, (uint32_t)mq, 1u, h->d_tau[0].as<uint32_t>());
		HIP_TRY(h, hipGetLastError());
		dq = h->d_range_q;
		dr = h->d_tau[0];
	}
	const bool name_scan = list == nullptr;  // ("scan_kernel" and the scan's time are stage 1's)
	const bool timed = name_scan && h->profiling && h->ev_used < kEventPairs;
	const char* kname = "";
	uint32_t passes = 0, qt_used = 0;
	if (gvf) {
		rc = ensure_filter_terms(h, st);  // (no filter is in force: the row terms are the plain ones)
		if (rc != EXPANN_OK)
			return rc;
		rc = launch_f16_query_prep(h, gvf, dq, mq, ip, false, I8fQueryArgs{}, st);
		if (rc != EXPANN_OK)
			return rc;
		// theta' from the caller's radii: a true-unit tau, times c_q under the inner product's rescale
		hipLaunchKernelGGL(f16_terms_kernel, dim3((uint32_t)((mq + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   h->d_qnrm.as<const float>(), (uint32_t)mq, gemm_f16_filter_eps(h->dim),
		                   std::ldexp(1.0f, -24) / h->f16_scale * std::sqrt((float)h->dim), dr,
		                   0.5f * h->f16_scale * h->f16_scale, h->d_theta, ip ? 1 : 0,
		                   ip ? h->d_qscale.as<const float>() : (const float*)nullptr);
		HIP_TRY(h, hipMemsetAsync(h->d_cnt, 0, sizeof(uint32_t) * mq, st));
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		rc = launch_scan_f16(h, gvf, find_direct_f16(h->dim, stage.direct_f16_tq), (uint32_t)h->n, true, mq, cus, ip, cap, st,
		                     &kname, &passes, &qt_used);
		if (rc != EXPANN_OK)
			return rc;
	} else {
		HIP_TRY(h, hipMemsetAsync(h->d_overflow, 0, 32, st));
		if (!list)
			HIP_TRY(h, hipMemcpyAsync(h->d_tau[0], d_radii, sizeof(float) * mq, hipMemcpyDeviceToDevice, st));
		if (timed)
			HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][0], st));
		rc = direct_scan(dq, mq, stage.direct_tq, cap, &kname);
		if (rc != EXPANN_OK)
			return rc;
	}
	if (timed) {
		HIP_TRY(h, hipEventRecord(h->ev[h->ev_used][1], st));
		h->ev_used++;
	}
	launch_gather_logs(h, st);
	HIP_TRY(h, hipGetLastError());
	RangeSelectParams rp{};
	rp.cand = h->d_cand;
	rp.cand_cnt = h->d_cnt;
	rp.slot_map = list;
	rp.radii = d_radii;
	rp.rerank_base = gvf ? (const void*)h->d_base : nullptr;
	rp.queries = (const float*)d_queries;
	rp.n_rows = (uint32_t)h->n;
	rp.dim = (uint32_t)h->dim;
	rp.metric_ip = ip ? 1u : 0u;
	rp.max_results = max_results;
	rp.id_offset = h->id_offset;
	rp.out_ids = d_ids;
	rp.out_dists = d_dists;
	rp.out_counts = d_counts;
	rp.over_cnt = word(over_word);
	rp.over_list = over_list;
	rp.over_cap = (uint32_t)m;
	rc = launch_range_select(h, rp, (uint32_t)mq, cap, st);
	if (rc != EXPANN_OK)
		return rc;
	// the host wait of the stage: the scan's flags (lost log entries, the largest |q|) and the overflow list's length
	HIP_TRY(h, hipMemcpyAsync(h->h_flags, h->d_overflow, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipMemcpyAsync(h->h_flags + 4, word(over_word), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(h, hipStreamSynchronize(st));
	const uint32_t before = *n_over;
	*n_over = h->h_flags[4];
	bool far = false;  // queries outside the fp16 range of this index
	if (gvf) {
		float qmax;  // bit pattern of max |q| (flags word 2)
		std::memcpy(&qmax, &h->h_flags[2], sizeof(float));
		far = !(qmax * h->f16_scale <= 60000.0f);
	}
	if (name_scan && !far && (timed || !h->profiling)) {  // the profile's counters and "scan_kernel": stage 1's scan that stands
		h->prof.scan_launches++;
		h->prof.scan_rows += h->n;
		h->prof.scan_query_tiles += passes;
		h->prof.query_tile = qt_used;
		h->prof.levels = 1;
		std::snprintf(h->prof.scan_kernel, sizeof(h->prof.scan_kernel), "%s", kname);
	}
	if (gvf) {
		if (far && !list) {
			// stage 1: the pass starts again on the exact direct scan.  This attempt's select has already appended the
			// queries whose list overflowed: the list is emptied, and the attempt leaves neither a timed event pair nor
			// a count in the profile -- the direct scan is the scan of stage 1
			HIP_TRY(h, hipMemsetAsync(word(over_word), 0, sizeof(uint32_t), st));
			*n_over = before;
			if (timed)
				h->ev_used--;
			*out_of_range = true;
			return EXPANN_OK;
		}
		if (far || h->h_flags[0] != 0) {  // every query of the stage goes on, once: the list's length is put back first
			if (list)
				HIP_TRY(h, hipMemcpyAsync(over_list + before, list, sizeof(uint32_t) * mq, hipMemcpyDeviceToDevice, st));
			else
				hipLaunchKernelGGL(range_iota_kernel, dim3((uint32_t)((mq + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
				                   over_list + before, (uint32_t)mq);
			HIP_TRY(h, hipGetLastError());
			*n_over = before + (uint32_t)mq;
			h->h_flags[7] = *n_over;
			HIP_TRY(h, hipMemcpyAsync(word(over_word), h->h_flags + 7, sizeof(uint32_t), hipMemcpyHostToDevice, st));
			HIP_TRY(h, hipStreamSynchronize(st));  // (h_flags[7] is read by the copy)
		}
	}
	return EXPANN_OK;
}

int RangePass::stage3() {
	const uint32_t row_words = (uint32_t)h->dim;
	const size_t k = max_results, nb = n_big;  // (nb <= m <= kMaxQueriesPerPass: one pass of the plain pipeline)
	HIP_TRY(h, h->d_range_q.ensure(sizeof(uint32_t) * nb * row_words));
	HIP_TRY(h, h->d_range_ids.ensure(sizeof(uint64_t) * nb * k));
	if (d_dists)
		HIP_TRY(h, h->d_range_dists.ensure(sizeof(float) * nb * k));
	const uint32_t grid = (uint32_t)std::min<size_t>((nb * row_words + kBlock - 1) / kBlock, 4096);
	hipLaunchKernelGGL(group_gather_rows_kernel, dim3(grid), dim3(kBlock), 0, st, (const uint32_t*)d_queries, big_list(), (uint32_t)nb,
	                   row_words, h->d_range_q.as<uint32_t>());
	HIP_TRY(h, hipGetLastError());
	float* const t_dists = d_dists ? h->d_range_dists.get() : nullptr;
	const int rc = search_pass(h, h->d_range_q, nb, k, h->d_range_ids, t_dists, st);
	if (rc != EXPANN_OK)
		return rc;
	const uint32_t grid2 = (uint32_t)std::min<size_t>((nb * k + kBlock - 1) / kBlock, 4096);
	hipLaunchKernelGGL(group_scatter_results_kernel, dim3(grid2), dim3(kBlock), 0, st, (const uint64_t*)h->d_range_ids.get(),
	                   (const float*)t_dists, big_list(), (uint32_t)nb, (uint32_t)k, d_ids, d_dists);
	HIP_TRY(h, hipGetLastError());
	return EXPANN_OK;
}

int RangePass::run() {
	HIP_TRY(h, grow_ws(h, h->d_range, sizeof(uint32_t) * (4 + 3 * m)));
	HIP_TRY(h, hipMemsetAsync(h->d_range, 0, sizeof(uint32_t) * 4, st));
	bool f16 = false, far = false, unused = false;
	int rc = filter_stage(true, nullptr, m, cap0, 0, retry_list(), &n_retry, &f16, &far);
	if (rc == EXPANN_OK && far)
		rc = filter_stage(false, nullptr, m, cap0, 0, retry_list(), &n_retry, &f16, &far);
	if (rc != EXPANN_OK)
		return rc;
	char stage1_kernel[sizeof(h->prof.scan_kernel)];  // ("scan_kernel" names the scan of stage 1)
	std::memcpy(stage1_kernel, h->prof.scan_kernel, sizeof(stage1_kernel));
	// stage 2: at kMaxCap keys.  Where stage 1 ran the fp16 form with shorter lists, that form again first -- the
	// direct scan of many queries is the slow one -- and the exact direct scan for what is left
	for (size_t q0 = 0; rc == EXPANN_OK && q0 < n_retry; q0 += kRangeRetryChunk) {
		const size_t R = std::min(kRangeRetryChunk, (size_t)n_retry - q0);
		if (f16 && cap0 < kMaxCap && f16_form(plan(R)))
			rc = filter_stage(true, retry_list() + q0, R, kMaxCap, 1, mid_list(), &n_mid, &unused, &far);
		else
			rc = filter_stage(false, retry_list() + q0, R, kMaxCap, 2, big_list(), &n_big, &unused, &far);
	}
	for (size_t q0 = 0; rc == EXPANN_OK && q0 < n_mid; q0 += kRangeRetryChunk)
		rc = filter_stage(false, mid_list() + q0, std::min(kRangeRetryChunk, (size_t)n_mid - q0), kMaxCap, 2, big_list(), &n_big,
		                  &unused, &far);
	if (rc == EXPANN_OK && n_big > 0 && max_results > 0)
		rc = stage3();
	std::memcpy(h->prof.scan_kernel, stage1_kernel, sizeof(stage1_kernel));
	if (rc != EXPANN_OK)
		return rc;
	h->stat_range[0] += m - n_big;
	h->stat_range[1] += n_big;
	h->stat_range[2] += n_retry;
	return EXPANN_OK;
}

// the checks of a range search, in the header's order, all before the device is touched
int range_args(expann_index* h, const void* queries, const float* radii, size_t max_results, const uint64_t* ids,
               const uint32_t* counts) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (!queries || !radii || !counts || (!ids && max_results > 0))
		return h->fail(EXPANN_ERR_INVALID_ARG, "range search: NULL queries / radii / counts / ids pointer");
	if (max_results > kMaxK)  // (by value, before any GPU work, as k is)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "range search: max_results beyond " + std::to_string(kMaxK));
	if (!float_rows(h))
		return h->fail(EXPANN_ERR_UNSUPPORTED, "range search: EXPANN_DTYPE_F32 and EXPANN_DTYPE_F16 rows only");
	if (!h->d_base)
		return h->fail(EXPANN_ERR_NOT_BUILT, "range search before build()");
	if (h->filter_on)
		return h->fail(EXPANN_ERR_UNSUPPORTED, "range search under a row filter is not offered");
	return EXPANN_OK;
}

// A range search on device buffers (the checks are done): enqueue on `st`, return when it has drained.
int range_search_device(expann_index* h, const void* d_queries, const float* d_radii, size_t m, size_t max_results,
                        uint64_t* d_ids, float* d_dists, uint32_t* d_counts, hipStream_t st) {
	struct HostCall {  // stage 3's passes are the waiting form, whatever "async_search" says
		expann_index* h;
		bool was;
		~HostCall() { h->host_call = was; }
	} guard{h, h->host_call};
	h->host_call = true;
	for (uint64_t& s : h->stat_range)
		s = 0;
	// stage 1's capacity: "cand_capacity", else room for twice the rows the caller asks for -- a caller that expects
	// long rows sizes max_results for them -- within 1 GiB of lists per pass
	uint32_t cap0 = h->opt_cand_capacity > 0 ? (uint32_t)std::min<long>(h->opt_cand_capacity, kMaxCap)
	                                         : std::max<uint32_t>(kRangeCap0, pow2ceil((uint32_t)(2 * max_results)));
	cap0 = std::min(std::max<uint32_t>(pow2ceil(cap0), 64), kMaxCap);
	if (h->opt_cand_capacity <= 0)
		while (cap0 > kRangeCap0 && (size_t)cap0 * std::min(m, kMaxQueriesPerPass) > ((size_t)1 << 27))
			cap0 >>= 1;
	const int cus = num_cus(h->device);
	const size_t qbytes = (size_t)h->dim * h->q_elem;
	for (size_t q0 = 0; q0 < m; q0 += kMaxQueriesPerPass) {
		const size_t mm = std::min(kMaxQueriesPerPass, m - q0);
		RangePass pass{h, (const char*)d_queries + q0 * qbytes, d_radii + q0, mm, (uint32_t)max_results,
		               d_ids ? d_ids + q0 * max_results : nullptr, d_dists ? d_dists + q0 * max_results : nullptr, d_counts + q0,
		               st, h->metric == EXPANN_METRIC_IP, cus, cap0};
		const int rc = pass.run();
		if (rc != EXPANN_OK)
			return rc;
	}
	HIP_TRY(h, hipStreamSynchronize(st));
	return EXPANN_OK;
}

}  // namespace

int expann_set_row_filter(expann_index* h, const uint32_t* allow_bits, size_t n_words) {
	return set_row_filter(h, allow_bits, n_words, false, nullptr);
}

int expann_set_row_filter_device(expann_index* h, const uint32_t* d_allow_bits, size_t n_words, void* stream) {
	return set_row_filter(h, d_allow_bits, n_words, true, (hipStream_t)stream);
}

int expann_clear_row_filter(expann_index* h) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (h->async_pending > 0) {  // (searches enqueued under the filter finish under it)
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	}
	h->filter_on = false;
	return EXPANN_OK;
}

int expann_set_row_groups(expann_index* h, const uint32_t* groups, size_t n) {
	return set_row_groups(h, groups, n, false, nullptr);
}

int expann_set_row_groups_device(expann_index* h, const uint32_t* d_groups, size_t n, void* stream) {
	return set_row_groups(h, d_groups, n, true, (hipStream_t)stream);
}

int expann_clear_row_groups(expann_index* h) {
	if (!h)
		return EXPANN_ERR_INVALID_ARG;
	if (h->async_pending > 0) {
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->async_stream));
	}
	drop_row_groups(h);
	return EXPANN_OK;
}

int expann_search_grouped_device(expann_index* h, const void* d_queries, const uint32_t* query_groups, size_t m, size_t k,
                                 uint64_t* d_ids, float* d_dists, void* stream) {
	bool empty = false;
	if (const int rc = grouped_args(h, d_queries, query_groups, m, k, d_ids, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	if (h->async_pending) {  // deferred searches first
		const int rs = expann_sync(h);
		if (rs != EXPANN_OK)
			return rs;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	return grouped_search_device(h, d_queries, query_groups, m, k, d_ids, d_dists, stream ? (hipStream_t)stream : h->stream);
}

int expann_search_grouped(expann_index* h, const void* queries, const uint32_t* query_groups, size_t m, size_t k,
                          uint64_t* ids, float* dists) {
	bool empty = false;
	if (const int rc = grouped_args(h, queries, query_groups, m, k, ids, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	if (h->async_pending) {  // deferred searches first
		const int rs = expann_sync(h);
		if (rs != EXPANN_OK)
			return rs;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t qbytes = m * (size_t)h->dim * h->q_elem;
	HIP_TRY(h, h->d_q.ensure(qbytes));
	HIP_TRY(h, h->d_ids.ensure(sizeof(uint64_t) * m * k));
	HIP_TRY(h, h->d_dists.ensure(sizeof(float) * m * k));
	HIP_TRY(h, hipMemcpyAsync(h->d_q, queries, qbytes, hipMemcpyHostToDevice, h->stream));
	const int rc = grouped_search_device(h, h->d_q, query_groups, m, k, h->d_ids, h->d_dists, h->stream);
	if (rc != EXPANN_OK)
		return rc;
	HIP_TRY(h, hipMemcpyAsync(ids, h->d_ids, sizeof(uint64_t) * m * k, hipMemcpyDeviceToHost, h->stream));
	if (dists)
		HIP_TRY(h, hipMemcpyAsync(dists, h->d_dists, sizeof(float) * m * k, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return EXPANN_OK;
}

int expann_range_search_device(expann_index* h, const void* d_queries, const float* d_radii, size_t m, size_t max_results,
                               uint64_t* d_ids, float* d_dists, uint32_t* d_counts, void* stream) {
	if (const int rc = range_args(h, d_queries, d_radii, max_results, d_ids, d_counts))
		return rc;
	if (m == 0)
		return EXPANN_OK;
	if (h->async_pending) {  // deferred searches first
		const int rs = expann_sync(h);
		if (rs != EXPANN_OK)
			return rs;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	return range_search_device(h, d_queries, d_radii, m, max_results, d_ids, d_dists, d_counts,
	                           stream ? (hipStream_t)stream : h->stream);
}

int expann_range_search(expann_index* h, const void* queries, const float* radii, size_t m, size_t max_results, uint64_t* ids,
                        float* dists, uint32_t* counts) {
	if (const int rc = range_args(h, queries, radii, max_results, ids, counts))
		return rc;
	if (m == 0)
		return EXPANN_OK;
	if (h->async_pending) {  // deferred searches first
		const int rs = expann_sync(h);
		if (rs != EXPANN_OK)
			return rs;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t qbytes = m * (size_t)h->dim * h->q_elem, cells = m * max_results;
	HIP_TRY(h, h->d_q.ensure(qbytes));
	HIP_TRY(h, h->d_range_radii.ensure(sizeof(float) * m));
	HIP_TRY(h, h->d_range_counts.ensure(sizeof(uint32_t) * m));
	if (cells) {
		HIP_TRY(h, h->d_ids.ensure(sizeof(uint64_t) * cells));
		if (dists)
			HIP_TRY(h, h->d_dists.ensure(sizeof(float) * cells));
	}
	HIP_TRY(h, hipMemcpyAsync(h->d_q, queries, qbytes, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(h, hipMemcpyAsync(h->d_range_radii, radii, sizeof(float) * m, hipMemcpyHostToDevice, h->stream));
	const int rc = range_search_device(h, h->d_q, h->d_range_radii, m, max_results, cells ? h->d_ids.get() : nullptr,
	                                   (cells && dists) ? h->d_dists.get() : nullptr, h->d_range_counts, h->stream);
	if (rc != EXPANN_OK)
		return rc;
	HIP_TRY(h, hipMemcpyAsync(counts, h->d_range_counts, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, h->stream));
	if (cells) {
		HIP_TRY(h, hipMemcpyAsync(ids, h->d_ids, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost, h->stream));
		if (dists)
			HIP_TRY(h, hipMemcpyAsync(dists, h->d_dists, sizeof(float) * cells, hipMemcpyDeviceToHost, h->stream));
	}
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return EXPANN_OK;
}

int expann_set_option(expann_index* h, const char* name, long value) {
	if (!h || !name)
		return EXPANN_ERR_INVALID_ARG;
	std::string msg;
	const int rc = set_option(*h, name, value, &msg);  // (bf_options.hpp: the table of names and rules)
	return rc == EXPANN_OK ? rc : h->fail(rc, msg);
}

}  // extern "C"
