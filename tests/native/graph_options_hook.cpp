// graph_options_hook.cpp -- prints what expann_amd/csrc/graph_options.hpp decides, for tests/test_graph_options.py.
//   graph_options_hook table          every row of kGraphOptionTable: its default, then the stored value, return code
//                                     and message after setting each probe value on a fresh GraphOptions
//   graph_options_hook set NAME V W   a set of V, then of W, of any name (unknown ones included) on one GraphOptions:
//                                     the return code, message and stored values after each
// Lines are tab-separated; "-" stands for "none".
#include "graph_options.hpp"

#include <cstdio>
#include <cstdlib>

using namespace expann;

static void print_values(const GraphOptions& o) {
	for (const GraphOptionRow& r : kGraphOptionTable)
		std::printf("\t%s=%ld", r.name, o.*r.value);
}

int main(int argc, char** argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "table") {
		const long probes[] = {-1, 0, 1, 7, 8, 12, 4096, 8192, 16384, 1L << 20, 1L << 21};
		for (const GraphOptionRow& r : kGraphOptionTable) {
			std::printf("row\t%s\t%ld\n", r.name, GraphOptions{}.*r.value);
			for (long v : probes) {
				GraphOptions o;
				std::string msg;
				const int rc = set_graph_option(o, r.name, v, &msg);
				std::printf("set\t%s\t%ld\t%ld\t%d\t%s\n", r.name, v, o.*r.value, rc, msg.empty() ? "-" : msg.c_str());
			}
		}
		return 0;
	}
	if (mode == "set" && argc == 5) {
		GraphOptions o;
		for (int i = 3; i < 5; ++i) {
			std::string msg;
			const int rc = set_graph_option(o, argv[2], std::atol(argv[i]), &msg);
			std::printf("%d\t%s", rc, msg.empty() ? "-" : msg.c_str());
			print_values(o);
			std::printf("\n");
		}
		return 0;
	}
	std::fprintf(stderr, "usage: graph_options_hook table | set NAME VALUE VALUE\n");
	return 2;
}
