// bf_options_hook.cpp -- prints what expann_amd/csrc/bf_options.hpp decides, for tests/test_bf_options.py.
//   bf_options_hook table          every row of kOptionTable: its default and environment name, then the stored value,
//                                  return code and message after setting each probe value on a fresh Options
//   bf_options_hook env            a fresh Options filled from this process's environment
//   bf_options_hook set NAME V     one set of any name (unknown ones included)
// Lines are tab-separated; "-" stands for "none".
#include "bf_options.hpp"

#include <cstdio>

using namespace expann;

static void print_value(const OptionRow& r, const Options& o) {
	if (r.value)
		std::printf("%ld", o.*r.value);
	else
		std::printf("-");
}

int main(int argc, char** argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "table") {
		const long probes[] = {-5, -1, 0, 1, 2, 3, 64, 65, 16384, 16385, 1000000};
		for (const OptionRow& r : kOptionTable) {
			std::printf("row\t%s\t", r.name);
			print_value(r, Options{});
			std::printf("\t%s\n", r.env ? r.env : "-");
			for (long v : probes) {
				Options o;
				std::string msg;
				const int rc = set_option(o, r.name, v, &msg);
				std::printf("set\t%s\t%ld\t", r.name, v);
				print_value(r, o);
				std::printf("\t%d\t%s\n", rc, msg.empty() ? "-" : msg.c_str());
			}
		}
		return 0;
	}
	if (mode == "env") {
		const Options o = options_from_env();
		for (const OptionRow& r : kOptionTable) {
			std::printf("env\t%s\t", r.name);
			print_value(r, o);
			std::printf("\n");
		}
		return 0;
	}
	if (mode == "set" && argc == 4) {
		const Options before;
		Options o;
		std::string msg;
		const int rc = set_option(o, argv[2], std::atol(argv[3]), &msg);
		bool changed = false;
		for (const OptionRow& r : kOptionTable)
			changed = changed || (r.value && o.*r.value != before.*r.value);
		std::printf("%d\t%s\t%s\n", rc, msg.empty() ? "-" : msg.c_str(), changed ? "changed" : "unchanged");
		return 0;
	}
	std::fprintf(stderr, "usage: bf_options_hook table | env | set NAME VALUE\n");
	return 2;
}
