// expann_append_check.cpp -- the reference's engine has no frozen state (src/brute_force_engine.h:20-46): store,
// build, query, store, query.  Drives gpu_brute_force_engine<float> through that sequence and compares every answer
// with a second engine that was given all the rows before its build.  Prints "ok ..." and exits 0, or says what
// differed and exits 1.  (tests/test_gpu_append.py runs it.)
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "expann/gpu_brute_force_engine.h"

int main() {
	const size_t d = 128, n0 = 4500, n1 = 300, m = 40, k = 10;
	std::mt19937 rng(12345);
	std::normal_distribution<float> dist(0.0f, 1.0f);
	std::vector<float> rows((n0 + n1 + 1) * d), queries(m * d);
	for (float& v : rows)
		v = dist(rng);
	for (float& v : queries)
		v = dist(rng);
	try {
		gpu_brute_force_engine<float> grown, whole, early;
		grown.store_rows(rows.data(), n0, d);
		grown._build();
		early.store_rows(rows.data(), n0, d);
		early._build();
		std::vector<uint64_t> a(m * k), b(m * k);
		std::vector<float> da(m * k), db(m * k);
		grown.query_k_batch(queries.data(), m, k, a.data(), da.data());
		early.query_k_batch(queries.data(), m, k, b.data(), db.data());
		if (a != b || da != db) {
			std::fprintf(stderr, "the two engines differ before anything was appended\n");
			return 1;
		}
		// store after build: a batch, then one vector through the CRTP interface
		grown.reserve(n0 + n1 + 1);
		grown.store_rows(rows.data() + n0 * d, n1, d);
		vec<float> last(d);
		for (size_t i = 0; i < d; ++i)
			last[i] = rows[(n0 + n1) * d + i];
		grown.store_vector(last);
		whole.store_rows(rows.data(), n0 + n1 + 1, d);
		whole._build();
		grown.query_k_batch(queries.data(), m, k, a.data(), da.data());
		whole.query_k_batch(queries.data(), m, k, b.data(), db.data());
		size_t appended_hits = 0;
		for (size_t i = 0; i < m * k; ++i) {
			if (a[i] != b[i] || da[i] != db[i]) {
				std::fprintf(stderr, "query %zu rank %zu: %llu (%g) after the append, %llu (%g) from the engine built in one go\n",
				             i / k, i % k, (unsigned long long)a[i], da[i], (unsigned long long)b[i], db[i]);
				return 1;
			}
			appended_hits += a[i] >= n0;
		}
		// the appended vector finds itself, with the next id
		const std::vector<size_t> self = grown.query_k(last, 1);
		if (self.size() != 1 || self[0] != n0 + n1 || grown.stored != n0 + n1 + 1) {
			std::fprintf(stderr, "the appended vector did not get id %zu\n", n0 + n1);
			return 1;
		}
		if (appended_hits == 0) {
			std::fprintf(stderr, "no appended row among the answers: the check shows nothing\n");
			return 1;
		}
		std::printf("ok: %zu + %zu rows, %zu queries, k = %zu, %zu answers are appended rows\n", n0, n1 + 1, m, k, appended_hits);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
