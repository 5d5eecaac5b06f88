// expann_graph_append_check.cpp -- the reference's antitopo_engine is incremental (_store_vector inserts into the
// live graph).  Drives gpu_antitopo_engine<float> through store, build, query, append_rows, query, a second append,
// save, and compares with a twin that was given the same rows by store_rows_batched before its build: the two index
// files row by row -- every (vertex, layer) list as a sorted set of (distance bits, id) -- and every answer, bit for
// bit.  Prints "ok ..." and exits 0, or says what differed and exits 1.  (tests/test_gpu_graph_append.py runs it.)
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

int main() {
	const size_t d = 64, n0 = 2600, n1 = 200, n2 = 90, m = 40, k = 10;
	std::mt19937 rng(4242);
	std::normal_distribution<float> dist(0.0f, 1.0f);
	std::vector<float> rows((n0 + n1 + n2) * d), queries(m * d);
	for (float& v : rows)
		v = dist(rng);
	for (float& v : queries)
		v = dist(rng);
	try {
		gpu_antitopo_engine_config cfg(12, 24, 4, 50, 1, 0.5f, 0.0f, 0);
		engine grown(cfg), twin(cfg);
		grown.index.dim = twin.index.dim = d;
		grown.store_rows_batched(rows.data(), n0, 500);
		grown._build();
		std::vector<uint64_t> a(m * k), b(m * k);
		std::vector<float> da(m * k), db(m * k);
		grown.query_k_batch(queries.data(), m, k, a.data(), da.data());
		if (grown.reserve(n0 + n1) != EXPANN_OK) {
			std::fprintf(stderr, "reserve: %s\n", expann_graph_last_error(grown.graph));
			return 1;
		}
		size_t done = 0;
		int rc = grown.append_rows(rows.data() + n0 * d, n1, &done);
		if (rc != EXPANN_OK || done != n1 || grown.index.size() != n0 + n1 || !grown.index.adjacency_stale) {
			std::fprintf(stderr, "append_rows: status %d, %zu rows in: %s\n", rc, done, expann_graph_last_error(grown.graph));
			return 1;
		}
		rc = grown.append_rows(rows.data() + (n0 + n1) * d, n2, &done);  // (past the reserved capacity: the handle grows)
		if (rc != EXPANN_OK || done != n2) {
			std::fprintf(stderr, "second append_rows: status %d: %s\n", rc, expann_graph_last_error(grown.graph));
			return 1;
		}
		uint64_t on_device = 0, reallocs = 0;
		expann_graph_get_stat(grown.graph, "append_device", &on_device);
		expann_graph_get_stat(grown.graph, "graph_reallocs", &reallocs);
		if (on_device != 2 || reallocs != 1) {
			std::fprintf(stderr, "append_device = %llu, graph_reallocs = %llu\n", (unsigned long long)on_device,
			             (unsigned long long)reallocs);
			return 1;
		}
		grown.query_k_batch(queries.data(), m, k, a.data(), da.data());
		twin.store_rows_batched(rows.data(), n0, 500);
		twin.store_rows_batched(rows.data() + n0 * d, n1);
		twin.store_rows_batched(rows.data() + (n0 + n1) * d, n2);
		twin._build();
		twin.query_k_batch(queries.data(), m, k, b.data(), db.data());
		size_t appended_hits = 0;
		for (size_t i = 0; i < m * k; ++i) {
			if (a[i] != b[i] || std::memcmp(&da[i], &db[i], sizeof(float)) != 0) {
				std::fprintf(stderr, "query %zu rank %zu: %llu (%g) after the appends, %llu (%g) from the twin\n", i / k, i % k,
				             (unsigned long long)a[i], da[i], (unsigned long long)b[i], db[i]);
				return 1;
			}
			appended_hits += a[i] >= n0;
		}
		grown.refresh_host();  // what save_index, store_rows and _build() do first
		if (grown.index.adjacency_stale || !same_graph(grown.index, twin.index)) {
			std::fprintf(stderr, "the host graph after the appends is not the twin's\n");
			return 1;
		}
		if (appended_hits == 0) {
			std::fprintf(stderr, "no appended row among the answers: the check shows nothing\n");
			return 1;
		}
		std::printf("ok: %zu + %zu + %zu rows, %zu queries, k = %zu, %zu answers are appended rows\n", n0, n1, n2, m, k,
		            appended_hits);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
