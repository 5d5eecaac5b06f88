// serial_build_hook.cpp -- test hook (compiled by tests/test_graph_build_oracle.py with g++): the serial
// host builder of include/expann/antitopo_index.h (insert_with_level, one vertex at a time) behind the
// strided-array layout of expann_graph_build_batched, so that the oracle's batched restatement at
// max_batch = 1 can be compared with it edge for edge.  No device.
#include <cstddef>
#include <cstdint>

#include "expann/antitopo_index.h"

extern "C" int serial_build(size_t dim, const float* vectors, size_t n, const uint8_t* levels, size_t M, size_t M0,
                            size_t ef_construction, size_t prune_overflow, float ortho_factor, float ortho_bias,
                            uint32_t* ids0, float* d0, uint32_t* deg0, size_t stride0, const int32_t* upper_idx,
                            size_t U, uint32_t* idsu, float* du, uint32_t* degu, size_t strideu,
                            uint32_t* max_layer, uint32_t* starting_vertex) {
	expann::antitopo_config c;
	c.M = M;
	c.M0 = M0;
	c.ef_construction = ef_construction;
	c.ortho_count = 1;
	c.ortho_factor = ortho_factor;
	c.ortho_bias = ortho_bias;
	c.prune_overflow = prune_overflow;
	expann::antitopo_index idx(dim, c);
	for (size_t v = 0; v < n; ++v)
		idx.insert_with_level(vectors + v * dim, levels[v]);
	for (size_t v = 0; v < n; ++v)
		for (size_t l = 0; l < idx.hadj_flat_with_lengths[v].size(); ++l) {
			const auto& el = idx.hadj_flat_with_lengths[v][l];
			const size_t st = l == 0 ? stride0 : strideu;
			const size_t row = l == 0 ? v : (l - 1) * U + (size_t)upper_idx[v];
			if (el.size() > st)
				return 1;
			for (size_t i = 0; i < el.size(); ++i) {
				(l == 0 ? ids0 : idsu)[row * st + i] = (uint32_t)el[i].second;
				(l == 0 ? d0 : du)[row * st + i] = el[i].first;
			}
			(l == 0 ? deg0 : degu)[row] = (uint32_t)el.size();
		}
	*max_layer = (uint32_t)idx.max_layer;
	*starting_vertex = (uint32_t)idx.starting_vertex;
	return 0;
}
