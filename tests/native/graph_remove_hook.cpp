// graph_remove_hook.cpp -- antitopo_index::remove_rows (THE GRAPH REMOVE RULE, expann_hip.h) without a device: a
// serial build of 700 rows, written as before.index; then, each from a copy of that index, the cases
//   a  70 random ids, unordered and with repeats
//   b  the starting vertex together with every vertex of the top layer: max_layer drops
//   c  6 of the 8 neighbours of one vertex: more distinct candidates than max(ef_construction, M0)
//   d  one vertex's whole one- and two-hop neighbourhood: its row ends empty
//   e  all rows but one
// written as case_<x>.index with the ids given as case_<x>.ids (uint64), and 100 more inserts after each.  The
// refusals leave the index byte for byte as it was.  Exits 0 and prints "ok", or says what went wrong.
// (tests/test_graph_remove_abi.py builds it, with the address and undefined-behaviour sanitizers where it can, and
// compares every file with the NumPy restatement of the rule.)
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include <set>
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
		std::fprintf(stderr, "only %zu layers: the check shows nothing about the upper layers\n", ix.max_layer);
		return 1;
	}
	ix.write_index(dir + "/before.index");

	std::vector<std::pair<std::string, std::vector<uint64_t>>> cases;
	{  // a
		std::vector<uint64_t> ids;
		for (int i = 0; i < 70; ++i)
			ids.push_back(rng() % n);
		for (int i = 0; i < 10; ++i)
			ids.push_back(ids[(size_t)i * 3]);
		cases.emplace_back("a", ids);
	}
	{  // b
		std::vector<uint64_t> ids{ix.starting_vertex};
		for (size_t v = 0; v < n; ++v)
			if (ix.hadj_flat[v].size() == ix.max_layer && v != ix.starting_vertex)
				ids.push_back(v);
		cases.emplace_back("b", ids);
	}
	{  // c: the vertex with a full bottom row whose neighbours' rows hold the most distinct vertices
		size_t best_v = n, best_cnt = 0;
		for (size_t v = 0; v < n; ++v) {
			if (ix.hadj_flat[v][0].size() != c.M0)
				continue;
			std::set<size_t> seen;
			for (size_t i = 0; i < 6; ++i)
				for (size_t w : ix.hadj_flat[ix.hadj_flat[v][0][i]][0])
					seen.insert(w);
			if (seen.size() > best_cnt) {
				best_cnt = seen.size();
				best_v = v;
			}
		}
		if (best_v == n) {
			std::fprintf(stderr, "no vertex with %zu neighbours\n", c.M0);
			return 1;
		}
		std::vector<uint64_t> ids;
		for (size_t i = 0; i < 6; ++i)
			ids.push_back(ix.hadj_flat[best_v][0][i]);
		cases.emplace_back("c", ids);
	}
	{  // d: a level-0 vertex
		size_t v = 0;
		while (ix.hadj_flat[v].size() != 1 || ix.hadj_flat[v][0].empty())
			++v;
		std::set<size_t> s;
		for (size_t a : ix.hadj_flat[v][0]) {
			s.insert(a);
			for (size_t b : ix.hadj_flat[a][0])
				if (b != v)
					s.insert(b);
		}
		cases.emplace_back("d", std::vector<uint64_t>(s.begin(), s.end()));
	}
	{  // e
		std::vector<uint64_t> ids;
		for (size_t v = n; v-- > 0;)
			if (v != 123)
				ids.push_back(v);
		cases.emplace_back("e", ids);
	}

	// the refusals: nothing changes
	{
		expann::antitopo_index w = ix;
		std::vector<uint64_t> all(n), past{3, n};
		for (size_t v = 0; v < n; ++v)
			all[v] = v;
		int refused = 0;
		try {
			w.remove_rows(all.data(), all.size());
		} catch (const std::invalid_argument&) {
			++refused;
		}
		try {
			w.remove_rows(past.data(), past.size());
		} catch (const std::invalid_argument&) {
			++refused;
		}
		size_t none = 7;
		w.remove_rows(nullptr, 0, &none);
		w.write_index(dir + "/refused.index");
		if (refused != 2 || none != 0 || slurp(dir + "/refused.index") != slurp(dir + "/before.index")) {
			std::fprintf(stderr, "a refused removal changed the index (%d refusals)\n", refused);
			return 1;
		}
	}

	for (auto& cs : cases) {
		expann::antitopo_index w = ix;
		std::set<uint64_t> distinct(cs.second.begin(), cs.second.end());
		size_t removed = 0;
		w.remove_rows(cs.second.data(), cs.second.size(), &removed);
		if (removed != distinct.size() || w.size() != n - distinct.size()) {
			std::fprintf(stderr, "case %s: %zu removed, size %zu\n", cs.first.c_str(), removed, w.size());
			return 1;
		}
		w.write_index(dir + "/case_" + cs.first + ".index");
		std::ofstream out(dir + "/case_" + cs.first + ".ids", std::ios::binary);
		out.write(reinterpret_cast<const char*>(cs.second.data()), (std::streamsize)(cs.second.size() * 8));
		// the serial builder goes on from what is left
		std::mt19937 r2(11);
		for (int i = 0; i < 100; ++i) {
			for (float& v : row)
				v = dist(r2);
			w.insert(row.data());
		}
		if (w.size() != n - distinct.size() + 100) {
			std::fprintf(stderr, "case %s: the inserts after the removal failed\n", cs.first.c_str());
			return 1;
		}
	}
	std::printf("ok %zu layers\n", ix.max_layer);
	return 0;
}
