// bf_plan_hook.cpp -- prints what expann_amd/csrc/bf_plan.hpp plans, for tests/test_bf_plan.py.  Reads one case per line
// from stdin, "key=value" pairs separated by blanks (keys as in `set` below; what a line leaves out keeps the default of
// PlanIndex / PlanCall / PlanAttempt), and answers one tab-separated line per case:
//   status family i8q u8_shadow direct_tq direct_f16_tq i8f i8f_min_cap speculate sampled tie_fallback message
// ("-" for no q-form and for no message).  Includes nothing of the project but that header.
#include "bf_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace expann;

static const char* family_name(ScanFamily f) {
	switch (f) {
	case ScanFamily::kDirect: return "direct";
	case ScanFamily::kF16X: return "f16x";
	case ScanFamily::kF16Y: return "f16y";
	case ScanFamily::kF16KX: return "f16kx";
	case ScanFamily::kF16KL: return "f16kl";
	case ScanFamily::kF16Dbg: return "f16dbg";
	case ScanFamily::kBf16x3: return "bf16x3";
	case ScanFamily::kGemmI8: return "gemm_i8";
	case ScanFamily::kI8qW: return "i8q_w";
	case ScanFamily::kI8qX: return "i8q_x";
	case ScanFamily::kI8qKL: return "i8q_kl";
	}
	return "?";
}

static bool set(PlanIndex& x, PlanCall& c, PlanAttempt& a, const std::string& key, long long v) {
	if (key == "dtype") x.dtype = (int)v;
	else if (key == "int_mode") x.int_mode = (int)v;
	else if (key == "metric") x.metric = (int)v;
	else if (key == "dim") x.dim = (int)v;
	else if (key == "n") x.n = (size_t)v;
	else if (key == "scan_kernel") x.scan_kernel = (long)v;
	else if (key == "query_tile") x.query_tile = (long)v;
	else if (key == "i8_filter") x.i8_filter = (long)v;
	else if (key == "u8_exact_opt") x.u8_exact_opt = (long)v;
	else if (key == "sample_pass") x.sample_pass = (long)v;
	else if (key == "spec_rank") x.spec_rank = (long)v;
	else if (key == "debug") x.debug = (long)v;
	else if (key == "cand_capacity") x.cand_capacity = (long)v;
	else if (key == "f16_ok") x.f16_ok = v != 0;
	else if (key == "i8f_state") x.i8f_state = (int)v;
	else if (key == "u8_exact") x.u8_exact = (int)v;
	else if (key == "filter_on") x.filter_on = v != 0;
	else if (key == "n_allowed") x.n_allowed = (size_t)v;
	else if (key == "m") c.m = (size_t)v;
	else if (key == "k") c.k = (size_t)v;
	else if (key == "cap") c.cap = (uint32_t)v;
	else if (key == "force_direct") a.force_direct = v != 0;
	else if (key == "no_f16") a.no_f16 = v != 0;
	else if (key == "i8f_off") a.i8f_off = v != 0;
	else if (key == "spec_off") a.spec_off = v != 0;
	else return false;
	return true;
}

int main() {
	char line[4096];
	while (std::fgets(line, sizeof(line), stdin)) {
		PlanIndex x;
		PlanCall c;
		PlanAttempt a;
		c.m = 1000;
		c.k = 10;
		c.cap = 2048;
		for (char* tok = std::strtok(line, " \t\n"); tok; tok = std::strtok(nullptr, " \t\n")) {
			char* eq = std::strchr(tok, '=');
			if (!eq || !set(x, c, a, std::string(tok, eq), std::atoll(eq + 1))) {
				std::fprintf(stderr, "bf_plan_hook: bad field %s\n", tok);
				return 2;
			}
		}
		const ScanPlan p = plan_scan(x, c, a);
		std::printf("%d\t%s\t%s\t%d\t%d\t%d\t%d\t%u\t%d\t%d\t%d\t%s\n", p.status, family_name(p.family),
		            p.i8q ? family_name(p.i8q_family) : "-", (int)p.u8_shadow, p.direct_tq, p.direct_f16_tq, (int)p.i8f, p.i8f_min_cap,
		            (int)p.speculate, (int)p.sampled, (int)p.tie_fallback, p.message[0] ? p.message : "-");
	}
	return 0;
}
