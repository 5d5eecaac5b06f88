// bf_remove_hook.cpp -- prints what expann_amd/csrc/bf_remove.hpp decides, for tests/test_bf_remove.py.  Reads one
// case per line from stdin: a verb, then "key=value" pairs separated by blanks (what a line leaves out keeps the
// default of AppendState), and answers one tab-separated line per case:
//   check   <state> n_ids=..                                          ->  status
//       (the checks made before the device is touched)
//   remove  <state> n_ids=.. bad_id=0/1 survivors=.. maxabs=<float>   ->  status n copies
//       (what the mark pass has shown: an id out of range, the survivors' count, max |v| over them)
//   newid   bits=<hex>,<hex>,...                                       ->  survivors new-ids
//       (new-ids: comma-separated "old:new" for every set bit of the bitmap, in ascending order)
// copies: nothing / compact / drop.  Floats are read by strtof ("inf", "nan" included).  Includes nothing of the
// project but that header.
#include "bf_remove.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace expann;

static const char* copies_name(RemoveCopy c) {
	return c == RemoveCopy::kCompact ? "compact" : (c == RemoveCopy::kDrop ? "drop" : "nothing");
}

int main() {
	char line[8192];
	while (std::fgets(line, sizeof(line), stdin)) {
		AppendState s;
		size_t n_ids = 0, survivors = 0;
		bool bad_id = false;
		float maxabs = 0.0f;
		std::vector<uint32_t> bits;
		char* verb = std::strtok(line, " \t\n");
		if (!verb)
			continue;
		for (char* tok = std::strtok(nullptr, " \t\n"); tok; tok = std::strtok(nullptr, " \t\n")) {
			char* eq = std::strchr(tok, '=');
			if (!eq) {
				std::fprintf(stderr, "bf_remove_hook: bad field %s\n", tok);
				return 2;
			}
			const std::string key(tok, eq);
			const char* v = eq + 1;
			if (key == "have_handle") s.have_handle = std::atoi(v) != 0;
			else if (key == "have_ids") s.have_rows = std::atoi(v) != 0;
			else if (key == "on_device") s.on_device = std::atoi(v) != 0;
			else if (key == "owned") s.owned = std::atoi(v) != 0;
			else if (key == "float_rows") s.float_rows = std::atoi(v) != 0;
			else if (key == "n") s.n = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "capacity") s.capacity = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "f16_scale") s.f16_scale = std::strtof(v, nullptr);
			else if (key == "state_maxabs") s.maxabs = std::strtof(v, nullptr);
			else if (key == "n_ids") n_ids = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "bad_id") bad_id = std::atoi(v) != 0;
			else if (key == "survivors") survivors = (size_t)std::strtoull(v, nullptr, 10);
			else if (key == "maxabs") maxabs = std::strtof(v, nullptr);
			else if (key == "bits") {
				for (const char* q = v; *q;) {
					char* end = nullptr;
					bits.push_back((uint32_t)std::strtoul(q, &end, 16));
					q = *end == ',' ? end + 1 : end;
				}
			} else {
				std::fprintf(stderr, "bf_remove_hook: bad field %s\n", tok);
				return 2;
			}
		}
		if (!std::strcmp(verb, "check") || !std::strcmp(verb, "remove")) {
			const RemovePlan p = verb[0] == 'c' ? plan_remove(s, n_ids) : plan_remove(s, n_ids, bad_id, survivors, maxabs);
			if ((p.status == EXPANN_OK) != (p.message[0] == 0)) {
				std::fprintf(stderr, "bf_remove_hook: status %d with message '%s'\n", p.status, p.message);
				return 3;
			}
			if (verb[0] == 'c')
				std::printf("%d\n", p.status);
			else
				std::printf("%d\t%zu\t%s\n", p.status, p.n, copies_name(p.copies));
		} else if (!std::strcmp(verb, "newid")) {
			std::vector<uint32_t> rank(bits.size());
			const uint32_t total = word_ranks(bits.data(), bits.size(), rank.data());
			std::printf("%u\t", total);
			bool first = true;
			for (uint32_t i = 0; i < 32 * (uint32_t)bits.size(); ++i)
				if ((bits[i >> 5] >> (i & 31)) & 1u) {
					std::printf("%s%u:%u", first ? "" : ",", i, new_id(bits.data(), rank.data(), i));
					first = false;
				}
			std::printf("\n");
		} else {
			std::fprintf(stderr, "bf_remove_hook: bad verb %s\n", verb);
			return 2;
		}
	}
	return 0;
}
