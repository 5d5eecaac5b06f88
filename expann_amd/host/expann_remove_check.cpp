// expann_remove_check.cpp -- store, build, query, remove, query, append, query on one gpu_brute_force_engine<float>;
// after each change every answer is compared with a second engine that was given the surviving rows before its
// build.  Prints "ok ..." and exits 0, or says what differed and exits 1.  (tests/test_gpu_remove.py runs it.)
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "expann/gpu_brute_force_engine.h"

namespace {
// the answers of `live` against those of an engine built from `rows` in one go
bool same_as_fresh(gpu_brute_force_engine<float>& live, const std::vector<float>& rows, size_t d, const std::vector<float>& queries,
                   size_t m, size_t k, const char* when) {
	gpu_brute_force_engine<float> fresh;
	fresh.store_rows(rows.data(), rows.size() / d, d);
	fresh._build();
	std::vector<uint64_t> a(m * k), b(m * k);
	std::vector<float> da(m * k), db(m * k);
	live.query_k_batch(queries.data(), m, k, a.data(), da.data());
	fresh.query_k_batch(queries.data(), m, k, b.data(), db.data());
	for (size_t i = 0; i < m * k; ++i)
		if (a[i] != b[i] || da[i] != db[i]) {
			std::fprintf(stderr, "%s: query %zu rank %zu: %llu (%g) on the live engine, %llu (%g) on the fresh one\n", when, i / k,
			             i % k, (unsigned long long)a[i], da[i], (unsigned long long)b[i], db[i]);
			return false;
		}
	if (live.stored != rows.size() / d) {
		std::fprintf(stderr, "%s: the live engine counts %zu rows, not %zu\n", when, live.stored, rows.size() / d);
		return false;
	}
	return true;
}
}  // namespace

int main() {
	const size_t d = 128, n0 = 4500, n1 = 200, m = 40, k = 10;
	std::mt19937 rng(4321);
	std::normal_distribution<float> dist(0.0f, 1.0f);
	std::vector<float> rows(n0 * d), more(n1 * d), queries(m * d);
	for (float& v : rows)
		v = dist(rng);
	for (float& v : more)
		v = dist(rng);
	for (float& v : queries)
		v = dist(rng);
	try {
		gpu_brute_force_engine<float> live;
		live.store_rows(rows.data(), n0, d);
		live._build();
		if (!same_as_fresh(live, rows, d, queries, m, k, "after build"))
			return 1;
		// remove: every seventh row, row 0 and the last row, one id twice, in descending order
		std::vector<uint64_t> ids;
		for (size_t i = n0; i-- > 0;)
			if (i % 7 == 0 || i == n0 - 1)
				ids.push_back(i);
		ids.push_back(ids[3]);
		std::vector<float> kept;
		size_t expect = 0;
		for (size_t i = 0; i < n0; ++i) {
			if (i % 7 == 0 || i == n0 - 1) {
				++expect;
				continue;
			}
			kept.insert(kept.end(), rows.begin() + i * d, rows.begin() + (i + 1) * d);
		}
		const size_t removed = live.remove_rows(ids.data(), ids.size());
		if (removed != expect) {
			std::fprintf(stderr, "remove_rows reported %zu rows, expected %zu\n", removed, expect);
			return 1;
		}
		if (!same_as_fresh(live, kept, d, queries, m, k, "after the remove"))
			return 1;
		// a survivor finds itself at its new id: old row 8 has lost rows 0 and 7 below it
		vec<float> probe(d);
		for (size_t i = 0; i < d; ++i)
			probe[i] = rows[8 * d + i];
		const std::vector<size_t> self = live.query_k(probe, 1);
		if (self.size() != 1 || self[0] != 6) {
			std::fprintf(stderr, "old row 8 is not at id 6 after the remove\n");
			return 1;
		}
		// append: the new rows get the ids from the new size on
		live.store_rows(more.data(), n1, d);
		kept.insert(kept.end(), more.begin(), more.end());
		if (!same_as_fresh(live, kept, d, queries, m, k, "after the append"))
			return 1;
		std::printf("ok: %zu rows, %zu removed, %zu appended, %zu queries, k = %zu\n", n0, removed, n1, m, k);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
