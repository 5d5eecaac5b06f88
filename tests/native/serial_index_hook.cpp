// serial_index_hook.cpp -- test hook (compiled by tests/graph_filter_helpers.py with g++): the serial host
// builder of include/expann/antitopo_index.h with the configuration expann_antitopo_create gives it (M0 = 2M,
// ortho_count = 1, ortho_factor = 0.5, ortho_bias = 0, prune_overflow = 0), its own level draws, and the index
// file in the reference's layout -- what expann_antitopo_store + expann_antitopo_save write.  No device.
#include <cstddef>
#include <exception>

#include "expann/antitopo_index.h"

extern "C" int serial_index(size_t dim, const float* rows, size_t n, size_t M, size_t ef_construction, const char* path) {
	try {
		expann::antitopo_config c;
		c.M = M;
		c.M0 = 2 * M;
		c.ef_search_mult = 1;
		c.ef_construction = ef_construction;
		c.ortho_count = 1;
		c.ortho_factor = 0.5f;
		c.ortho_bias = 0.0f;
		c.prune_overflow = 0;
		expann::antitopo_index idx(dim, c);
		for (size_t v = 0; v < n; ++v)
			idx.insert(rows + v * dim);
		idx.write_index(path);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
