// expann_graph_remove_check.cpp -- drives gpu_antitopo_engine<float> through build, query, remove_rows, query,
// append_rows, remove_rows, save (THE GRAPH REMOVE RULE, expann_hip.h), beside a TWIN that takes every step on the
// host: antitopo_index::remove_rows -- the C++ statement of the rule -- on a copy of the index, store_rows_batched for
// the append, and an upload.  After every step the two host graphs must agree row by row -- every (vertex, layer)
// list as a sorted set of (distance bits, id), the freedom THE BATCH RULE leaves an appended graph -- and every answer
// bit for bit.  Prints "ok ..." and exits 0, or says what differed and exits 1.  (tests/test_gpu_graph_remove.py runs it.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "expann/gpu_antitopo_engine.h"

using engine = gpu_antitopo_engine<float>;

static bool same_graph(const expann::antitopo_index& a, const expann::antitopo_index& b) {
	if (a.size() != b.size() || a.max_layer != b.max_layer || a.starting_vertex != b.starting_vertex ||
	    a.hadj_flat_with_lengths.size() != b.hadj_flat_with_lengths.size())
		return false;
	if (std::memcmp(a.vectors.data(), b.vectors.data(), a.vectors.size() * sizeof(float)) != 0)
		return false;
	for (size_t v = 0; v < a.hadj_flat_with_lengths.size(); ++v) {
		if (a.hadj_flat_with_lengths[v].size() != b.hadj_flat_with_lengths[v].size())
			return false;
		for (size_t l = 0; l < a.hadj_flat_with_lengths[v].size(); ++l) {
			auto x = a.hadj_flat_with_lengths[v][l], y = b.hadj_flat_with_lengths[v][l];
			std::sort(x.begin(), x.end());
			std::sort(y.begin(), y.end());
			if (x != y) {
				std::fprintf(stderr, "vertex %zu layer %zu differs\n", v, l);
				return false;
			}
		}
	}
	return true;
}

static bool same_answers(engine& a, engine& b, const std::vector<float>& q, size_t m, size_t k, const char* when) {
	std::vector<uint64_t> ia(m * k), ib(m * k);
	std::vector<float> da(m * k), db(m * k);
	a.query_k_batch(q.data(), m, k, ia.data(), da.data());
	b.query_k_batch(q.data(), m, k, ib.data(), db.data());
	for (size_t i = 0; i < m * k; ++i)
		if (ia[i] != ib[i] || std::memcmp(&da[i], &db[i], sizeof(float)) != 0) {
			std::fprintf(stderr, "%s: query %zu rank %zu: %llu (%g) from the engine, %llu (%g) from the twin\n", when, i / k,
			             i % k, (unsigned long long)ia[i], da[i], (unsigned long long)ib[i], db[i]);
			return false;
		}
	return true;
}

int main() {
	const size_t d = 64, n0 = 2600, n1 = 150, m = 40, k = 10;
	std::mt19937 rng(777);
	std::normal_distribution<float> dist(0.0f, 1.0f);
	std::vector<float> rows((n0 + n1) * d), queries(m * d);
	for (float& v : rows)
		v = dist(rng);
	for (float& v : queries)
		v = dist(rng);
	try {
		gpu_antitopo_engine_config cfg(12, 24, 4, 50, 1, 0.5f, 0.0f, 0);
		engine eng(cfg), twin(cfg);
		eng.index.dim = twin.index.dim = d;
		eng.store_rows_batched(rows.data(), n0, 500);
		eng._build();
		twin.index = eng.index;
		twin.upload();
		if (!same_answers(eng, twin, queries, m, k, "before the remove"))
			return 1;
		// 200 ids, unordered, some twice
		std::vector<uint64_t> ids;
		for (int i = 0; i < 200; ++i)
			ids.push_back(rng() % n0);
		for (int i = 0; i < 20; ++i)
			ids.push_back(ids[(size_t)i * 7]);
		size_t removed = 0, removed_twin = 0;
		int rc = eng.remove_rows(ids.data(), ids.size(), &removed);
		if (rc != EXPANN_OK || !eng.index.adjacency_stale) {
			std::fprintf(stderr, "remove_rows: status %d: %s%s\n", rc, eng.remove_error.c_str(), expann_graph_last_error(eng.graph));
			return 1;
		}
		twin.index.remove_rows(ids.data(), ids.size(), &removed_twin);
		twin.upload();
		if (removed != removed_twin || eng.index.size() != n0 - removed || removed < 150) {
			std::fprintf(stderr, "%zu rows removed, the twin removed %zu\n", removed, removed_twin);
			return 1;
		}
		if (!same_answers(eng, twin, queries, m, k, "after the remove"))
			return 1;
		// a refused call changes nothing
		const uint64_t past[2] = {3, eng.index.size()};
		if (eng.remove_rows(past, 2, &removed) != EXPANN_ERR_INVALID_ARG || removed != 0 ||
		    !same_answers(eng, twin, queries, m, k, "after a refused remove"))
			return 1;
		// append, remove again (the survivors' ids have moved), save
		size_t done = 0;
		rc = eng.append_rows(rows.data() + n0 * d, n1, &done);
		if (rc != EXPANN_OK || done != n1) {
			std::fprintf(stderr, "append_rows after the remove: status %d: %s\n", rc, expann_graph_last_error(eng.graph));
			return 1;
		}
		twin.store_rows_batched(rows.data() + n0 * d, n1);
		twin._build();
		if (!same_answers(eng, twin, queries, m, k, "after the append"))
			return 1;
		std::vector<uint64_t> ids2;
		for (int i = 0; i < 60; ++i)
			ids2.push_back(rng() % eng.index.size());
		ids2.push_back(eng.index.size() - 1);  // an appended row
		rc = eng.remove_rows(ids2.data(), ids2.size(), &removed);
		if (rc != EXPANN_OK) {
			std::fprintf(stderr, "second remove_rows: status %d: %s%s\n", rc, eng.remove_error.c_str(), expann_graph_last_error(eng.graph));
			return 1;
		}
		twin.index.remove_rows(ids2.data(), ids2.size(), &removed_twin);
		twin.upload();
		if (removed != removed_twin || !same_answers(eng, twin, queries, m, k, "after the second remove"))
			return 1;
		uint64_t on_device = 0, calls = 0, touched = 0;
		expann_graph_get_stat(eng.graph, "remove_device", &on_device);
		expann_graph_get_stat(eng.graph, "remove_calls", &calls);
		expann_graph_get_stat(eng.graph, "remove_touched_rows", &touched);
		if (on_device != 2 || calls != 2 || touched == 0) {
			std::fprintf(stderr, "remove_device = %llu, remove_calls = %llu, remove_touched_rows = %llu\n",
			             (unsigned long long)on_device, (unsigned long long)calls, (unsigned long long)touched);
			return 1;
		}
		eng.refresh_host();  // what save_index does first
		if (eng.index.adjacency_stale || !same_graph(eng.index, twin.index)) {
			std::fprintf(stderr, "the host graph after remove, append, remove is not the twin's\n");
			return 1;
		}
		std::printf("ok: %zu rows, %zu + %zu removed, %zu appended, %llu rows repaired on the device\n", n0,
		            n0 + n1 - eng.index.size() - removed, removed, n1, (unsigned long long)touched);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
