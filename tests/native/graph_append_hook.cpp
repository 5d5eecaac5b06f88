// graph_append_hook.cpp -- the host half of the refresh after a device append (gpu_antitopo_engine::refresh_host),
// without a device: a serial build, to_strided, the upper-layer arrays moved to a LARGER row stride (the device keeps
// them at a capacity), then from_strided(g, nullptr, ...) as refresh_host calls it -- the index must come back edge
// for edge, write_index byte for byte.  Exits 0 and prints "ok", or says what differed.
// (tests/test_graph_append_abi.py builds it, with the address and undefined-behaviour sanitizers where it can.)
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "expann/antitopo_index.h"

static std::string slurp(const std::string& p) {
	std::ifstream in(p, std::ios::binary);
	return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
	if (argc != 2)
		return 2;
	const std::string dir = argv[1];
	const size_t d = 16, n = 700;
	expann::antitopo_config c;
	c.M = 4;
	c.M0 = 8;
	c.ef_construction = 20;
	expann::antitopo_index ix(d, c);
	std::mt19937 rng(7);
	std::normal_distribution<float> dist(0.0f, 1.0f);
	std::vector<float> row(d);
	for (size_t i = 0; i < n; ++i) {
		for (float& v : row)
			v = dist(rng);
		ix.insert(row.data());
	}
	if (ix.max_layer < 3) {
		std::fprintf(stderr, "only %zu layers: the check shows nothing about the upper arrays\n", ix.max_layer);
		return 1;
	}
	ix.write_index(dir + "/before.index");
	auto g = ix.to_strided({}, 64);
	// the device's layout: row (l - 1) * U_cap + upper_idx[v]
	const size_t U_cap = g.U + g.U / 2 + 64;
	expann::antitopo_index::strided_graph w = g;
	w.U = U_cap;
	w.idsu.assign(U_cap * g.n_upper_layers * g.strideu, 0xFFFFFFFFu);
	w.du.assign(U_cap * g.n_upper_layers * g.strideu, -1.0f);
	w.degu.assign(U_cap * g.n_upper_layers, 0);
	for (size_t l = 0; l < g.n_upper_layers; ++l)
		for (size_t u = 0; u < g.U; ++u) {
			const size_t from = l * g.U + u, to = l * U_cap + u;
			w.degu[to] = g.degu[from];
			for (size_t i = 0; i < g.strideu; ++i) {
				w.idsu[to * g.strideu + i] = g.idsu[from * g.strideu + i];
				w.du[to * g.strideu + i] = g.du[from * g.strideu + i];
			}
		}
	ix.adjacency_stale = true;
	ix.hadj_flat_with_lengths.clear();  // (stale: whatever it holds must not matter)
	ix.hadj_flat.clear();
	ix.from_strided(w, nullptr, ix.max_layer, ix.starting_vertex);
	ix.adjacency_stale = false;
	if (ix.size() != n) {
		std::fprintf(stderr, "size %zu after from_strided\n", ix.size());
		return 1;
	}
	ix.write_index(dir + "/after.index");
	if (slurp(dir + "/before.index") != slurp(dir + "/after.index")) {
		std::fprintf(stderr, "the index file differs after to_strided / from_strided at a wider upper stride\n");
		return 1;
	}
	// and the serial builder goes on from the refreshed index
	for (float& v : row)
		v = dist(rng);
	ix.insert(row.data());
	std::printf("ok %zu layers %zu upper vertices\n", ix.max_layer, g.U);
	return 0;
}
