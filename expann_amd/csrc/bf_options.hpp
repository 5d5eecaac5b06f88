// bf_options.hpp -- the options of the brute-force handle (expann_set_option): THE list of them.  Each has one row
// in kOptionTable -- its name, the environment variable that sets its starting value (or none), where it is stored
// and the rule a value passes through -- and expann_set_option and expann_create decide no value by themselves.
// Host arithmetic on the standard library alone: no HIP here, so that a plain C++ compiler can test the table.
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/expann_hip.h"

namespace expann {

constexpr uint32_t kMaxCap = 16384;  // keys per query that fit the select kernel's LDS: the longest candidate list

struct Options {
	long opt_query_tile = 0, opt_cand_capacity = 0;
	long opt_debug = 0;
	long opt_scan_kernel = 0;        // 0 auto, 1 direct (scan_filter), 2 GEMM form on fp32 / int8
	                                 // MFMA, 3 GEMM form on bf16 MFMA with the 3-term split
	long opt_scan_chunks = 0;
	long opt_ip_rescale = 1;         // fp16 form, inner product: the filter sees each query times a power of two (f16_query_prep_kernel)
	long opt_sample_pass = 1;        // fp16 form: one sampled class-maxima pass instead of the level ladder
	long opt_u8_exact = 1;           // fp32 rows that are all integers in [0, 255]: the uint8 shadow (U8Shadow)
	long opt_latency_mode = 1;       // few queries from host buffers: results land in pinned memory
	long opt_async = 0;              // deferred check (expann_sync)
	long opt_tail_chunks = 1;        // scan_gemm_f16x: the last round's row chunks three times finer (pick_tail_chunks)
	long opt_persist = 1;            // scan_gemm_f16x: resident workgroups pull (query tile, row chunk) items per XCD
	long opt_redo_bound = 1;         // debug: 0 = the redo pass's thresholds from the proven tau alone
	long opt_select_overlap = 1;     // debug: 0 = the select stages of long lists on the caller's stream
	long opt_i8_filter = 1;          // fp32 L2 d = 128: the int8 filter (scan_gemm_i8f.hpp): 0 off, 1 auto, 2 wherever supported
	long opt_i8_sample = 1;          // its sampled pass on int8 too: 0 off, 1 where it speculates at the auto rank, 2 wherever it speculates
	long opt_spec_rank = 0;          // speculative thresholds: 0 auto, j >= 1: the j-th class maximum (j >= k: off)
	long opt_rerank_rounds = 2;      // int8 filter's lists: 2 = re-ranked in two rounds, 1 = the single cut
	long opt_rerank_stats = 0;       // 1 = count the rows the selects re-score ("rerank_rows"; adds launches and a host wait)
	long opt_xcd_tolerance = 3;      // % of modelled cost given up for an XCD-aligned chunk count
	long opt_sample_run = 1;         // consecutive 64-row tiles per sampled stretch.  1: the sample
	                                 // is spread as finely as tiles allow -- with rows stored by
	                                 // cluster, stretches of 16 tiles skipped whole clusters and the
	                                 // full scan drowned in candidates (90 k instead of 2.8 M QPS on
	                                 // 1000 contiguous clusters); on iid rows the two differ by < 1 %
	long opt_sample_frac = 0;        // the sampled pass reads 1/frac of the rows; 0 = by k (sample_frac_for)
	long opt_sample_ratio = 32;
	long opt_group_list_rows = 0;    // "group_list_rows": 0 = kGroupListRowsAuto
};

// what a value passes through on its way into an Options
enum class OptionRule {
	kClamp,     // stored, clamped to [lo, hi] (LONG_MIN / LONG_MAX: no bound on that side)
	kFlag,      // v != 0
	kOneOrTwo,  // 1 if v == 1, else 2
	kInRange,   // outside [lo, hi]: EXPANN_ERR_INVALID_ARG, the value stays
	kRemoved    // an A/B switch whose 0 side is gone: 0 is EXPANN_ERR_UNSUPPORTED, anything else is accepted; nothing is stored
};
struct OptionRow {
	const char* name;
	const char* env;  // sets the starting value at expann_create, through atol and the same rule; nullptr: none
	long Options::*value;
	OptionRule rule;
	long lo, hi;
};
inline constexpr OptionRow kOptionTable[] = {
    {"query_tile", nullptr, &Options::opt_query_tile, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"cand_capacity", nullptr, &Options::opt_cand_capacity, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"debug", nullptr, &Options::opt_debug, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"scan_kernel", nullptr, &Options::opt_scan_kernel, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"scan_chunks", nullptr, &Options::opt_scan_chunks, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"ip_rescale", nullptr, &Options::opt_ip_rescale, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"sample_pass", nullptr, &Options::opt_sample_pass, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"u8_exact", nullptr, &Options::opt_u8_exact, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"latency_mode", nullptr, &Options::opt_latency_mode, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"async_search", nullptr, &Options::opt_async, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"tail_chunks", "EXPANN_TAIL_CHUNKS", &Options::opt_tail_chunks, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"persist", "EXPANN_PERSIST", &Options::opt_persist, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    // (the two debug options of the search's tail: A/B runs)
    {"redo_bound", "EXPANN_REDO_BOUND", &Options::opt_redo_bound, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"select_overlap", "EXPANN_SELECT_OVERLAP", &Options::opt_select_overlap, OptionRule::kClamp, LONG_MIN, LONG_MAX},
    {"i8_filter", "EXPANN_I8_FILTER", &Options::opt_i8_filter, OptionRule::kClamp, 0, 2},
    {"i8_sample", "EXPANN_I8_SAMPLE", &Options::opt_i8_sample, OptionRule::kClamp, 0, 2},
    {"spec_rank", "EXPANN_SPEC_RANK", &Options::opt_spec_rank, OptionRule::kClamp, 0, LONG_MAX},
    {"rerank_rounds", "EXPANN_RERANK_ROUNDS", &Options::opt_rerank_rounds, OptionRule::kOneOrTwo, 0, 0},  // (A/B runs against the single cut)
    {"rerank_stats", nullptr, &Options::opt_rerank_stats, OptionRule::kFlag, 0, 0},
    {"xcd_tolerance", nullptr, &Options::opt_xcd_tolerance, OptionRule::kClamp, 0, LONG_MAX},
    {"sample_run", nullptr, &Options::opt_sample_run, OptionRule::kClamp, 1, 64},
    {"sample_frac", nullptr, &Options::opt_sample_frac, OptionRule::kClamp, 0, LONG_MAX},
    {"sample_ratio", nullptr, &Options::opt_sample_ratio, OptionRule::kClamp, 2, LONG_MAX},
    {"group_list_rows", nullptr, &Options::opt_group_list_rows, OptionRule::kInRange, 0, (long)kMaxCap},
    // (rounds 1-2: A/B switches between the 32x32 kernels and the 16x16 ones; the 32x32 kernels are gone)
    {"f16x", nullptr, nullptr, OptionRule::kRemoved, 0, 0},
    {"i8x", nullptr, nullptr, OptionRule::kRemoved, 0, 0},
    {"i8w", nullptr, nullptr, OptionRule::kRemoved, 0, 0},
};

// `name` = `value` by the name's rule.  EXPANN_OK, or the error's code with its text in *msg: a rule's own, or
// EXPANN_ERR_INVALID_ARG for a name that is not in the table
inline int set_option(Options& o, const char* name, long value, std::string* msg) {
	for (const OptionRow& r : kOptionTable) {
		if (std::strcmp(name, r.name))
			continue;
		switch (r.rule) {
		case OptionRule::kClamp:
			o.*r.value = value < r.lo ? r.lo : (value > r.hi ? r.hi : value);
			break;
		case OptionRule::kFlag:
			o.*r.value = value ? 1 : 0;
			break;
		case OptionRule::kOneOrTwo:
			o.*r.value = value == 1 ? 1 : 2;
			break;
		case OptionRule::kInRange:
			if (value < r.lo || value > r.hi) {
				*msg = std::string(name) + ": " + std::to_string(r.lo) + " (auto) or 1.." + std::to_string(r.hi);
				return EXPANN_ERR_INVALID_ARG;
			}
			o.*r.value = value;
			break;
		case OptionRule::kRemoved:
			if (value == 0) {
				*msg = std::string(name) + " = 0: the 32 x 32 MFMA forms of rounds 1-2 were removed in round 3";
				return EXPANN_ERR_UNSUPPORTED;
			}
			break;
		}
		return EXPANN_OK;
	}
	*msg = std::string("unknown option ") + name;
	return EXPANN_ERR_INVALID_ARG;
}

// the starting values of a new handle: the defaults, and what the environment sets
inline Options options_from_env() {
	Options o;
	std::string unused;
	for (const OptionRow& r : kOptionTable)
		if (const char* e = r.env ? std::getenv(r.env) : nullptr)
			(void)set_option(o, r.name, std::atol(e), &unused);
	return o;
}

}  // namespace expann
