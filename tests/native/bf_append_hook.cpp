// bf_append_hook.cpp -- prints what expann_amd/csrc/bf_append.hpp decides, for tests/test_bf_append.py.  Reads one
// case per line from stdin: a verb, then "key=value" pairs separated by blanks (what a line leaves out keeps the
// default of AppendState), and answers one tab-separated line per case:
//   scale   maxabs=<float>                       ->  scale usable
//   append  <state> n_new=.. maxabs_new=<float>  ->  status n capacity realloc copies
//   reserve <state> n_rows=..                    ->  status n capacity realloc copies
//   grow    n=.. step=.. count=..                ->  reallocs capacity   (count appends of step rows onto n rows)
// copies: nothing / extend / drop.  Floats are read by strtof ("inf", "nan" included).  Includes nothing of the
// project but that header.
#include "bf_append.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace expann;

static const char* copies_name(CopyAction c) {
	return c == CopyAction::kExtend ? "extend" : (c == CopyAction::kDrop ? "drop" : "nothing");
}

int main() {
	char line[4096];
	while (std::fgets(line, sizeof(line), stdin)) {
		AppendState s;
		size_t n_new = 0, n_rows = 0, step = 0, count = 0;
		float maxabs = 0.0f, maxabs_new = 0.0f;
		char* verb = std::strtok(line, " \t\n");
		if (!verb)
			continue;
		for (char* tok = std::strtok(nullptr, " \t\n"); tok; tok = std::strtok(nullptr, " \t\n")) {
			char* eq = std::strchr(tok, '=');
			if (!eq) {
				std::fprintf(stderr, "bf_append_hook: bad field %s\n", tok);
				return 2;
			}
			const std::string key(tok, eq);
			const char* v = eq + 1;
			if (key == "have_handle") s.have_handle = std::atoi(v) != 0;
			else if (key == "have_rows") s.have_rows = std::atoi(v) != 0;
			else if (key == "on_device") s.on_device = std::atoi(v) != 0;
			else if (key == "owned") s.owned = std::atoi(v) != 0;
			else if (key == "float_rows") s.float_rows = std::atoi(v) != 0;
			else if (key == "n") s.n = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "capacity") s.capacity = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "f16_scale") s.f16_scale = std::strtof(v, nullptr);
			else if (key == "state_maxabs") s.maxabs = std::strtof(v, nullptr);
			else if (key == "n_new") n_new = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "n_rows") n_rows = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "step") step = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "count") count = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "maxabs") maxabs = std::strtof(v, nullptr);
			else if (key == "maxabs_new") maxabs_new = std::strtof(v, nullptr);
			else {
				std::fprintf(stderr, "bf_append_hook: bad field %s\n", tok);
				return 2;
			}
		}
		if (!std::strcmp(verb, "scale")) {
			const F16Scale f = f16_scale_for(maxabs);
			std::printf("%.17g\t%d\n", (double)f.scale, (int)f.usable);
		} else if (!std::strcmp(verb, "append") || !std::strcmp(verb, "reserve")) {
			const AppendPlan p = verb[0] == 'a' ? plan_append(s, n_new, maxabs_new) : plan_reserve(s, n_rows);
			if ((p.status == EXPANN_OK) != (p.message[0] == 0)) {
				std::fprintf(stderr, "bf_append_hook: status %d with message '%s'\n", p.status, p.message);
				return 3;
			}
			std::printf("%d\t%zu\t%zu\t%d\t%s\n", p.status, p.n, p.capacity, (int)p.realloc, copies_name(p.copies));
		} else if (!std::strcmp(verb, "grow")) {
			s.on_device = s.owned = true;
			s.capacity = s.n;
			size_t reallocs = 0;
			for (size_t i = 0; i < count; ++i) {
				const AppendPlan p = plan_append(s, step, 0.0f);
				if (p.status != EXPANN_OK || p.capacity < p.n)
					return 4;
				reallocs += p.realloc;
				s.n = p.n;
				s.capacity = p.capacity;
			}
			std::printf("%zu\t%zu\n", reallocs, s.capacity);
		} else {
			std::fprintf(stderr, "bf_append_hook: bad verb %s\n", verb);
			return 2;
		}
	}
	return 0;
}
