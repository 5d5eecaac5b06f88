// graph_options.hpp -- the options of the graph handle (expann_graph_set_option): THE list of them.  Each has one row
// in kGraphOptionTable -- its name, where it is stored and the rule a value must pass -- and
// expann_graph_set_option decides no value by itself.  Host arithmetic on the standard library alone, as
// bf_options.hpp: no HIP here, so that a plain C++ compiler can test the table.
#pragma once
#include <cstring>
#include <string>

#include "../../include/expann_hip.h"

namespace expann {

struct GraphOptions {
	long opt_flat_rows = 0;  // "filter_flat_rows": 0 = kGraphFlatRowsAuto
	long opt_cand_cap = 0;   // "cand_capacity": the heap a search starts with, 0 = graph_first_cand_cap
	long opt_redo_cap = 0;   // "redo_capacity": the redo launch's heap, 0 = the largest whose working set fits
};

// a heap capacity: 0 = auto, else a power of two in [8, hi]
constexpr bool graph_capacity_ok(long v, long hi) { return v == 0 || (v >= 8 && (v & (v - 1)) == 0 && v <= hi); }

struct GraphOptionRow {
	const char* name;
	long GraphOptions::*value;
	bool (*ok)(long);  // the rule; a value it refuses is EXPANN_ERR_INVALID_ARG, and the stored one stays
	const char* must;  // ... with the name and this as the message
};
inline constexpr GraphOptionRow kGraphOptionTable[] = {
    // rows, not a capacity: any count
    {"filter_flat_rows", &GraphOptions::opt_flat_rows, [](long v) { return v >= 0; }, " must be >= 0 (0 = auto)"},
    {"cand_capacity", &GraphOptions::opt_cand_cap, [](long v) { return graph_capacity_ok(v, 1L << 20); },
     " must be 0 or a power of two >= 8"},
    // (at most 8192, the LDS limit of the heap)
    {"redo_capacity", &GraphOptions::opt_redo_cap, [](long v) { return graph_capacity_ok(v, 8192); },
     " must be 0 or a power of two >= 8 and <= 8192"},
};

// `name` = `value` by the name's rule.  EXPANN_OK, or EXPANN_ERR_INVALID_ARG with its text in *msg: the rule's, or
// that of a name that is not in the table
inline int set_graph_option(GraphOptions& o, const char* name, long value, std::string* msg) {
	for (const GraphOptionRow& r : kGraphOptionTable)
		if (!std::strcmp(name, r.name)) {
			if (!r.ok(value)) {
				*msg = std::string(name) + r.must;
				return EXPANN_ERR_INVALID_ARG;
			}
			o.*r.value = value;
			return EXPANN_OK;
		}
	*msg = std::string("unknown option: ") + name;
	return EXPANN_ERR_INVALID_ARG;
}

}  // namespace expann
