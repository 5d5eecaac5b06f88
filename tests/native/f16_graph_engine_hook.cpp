// f16_graph_engine_hook.cpp -- test hook, a stand-alone program (compiled by tests/test_graph_f16_abi.py with g++; no
// device, no library): the host side of gpu_antitopo_engine<float> with config::rows_f16 -- rounding on insert, the
// refusals, the index file and the pack to halves -- with the C ABI calls it makes stubbed below.  The stub of
// expann_graph_create_f16 keeps the halves it is handed, so the program can compare them with the rows.  Built with
// -fsanitize=address,undefined it is also how that host code is run under the sanitizers.
//
//   f16_graph_engine_hook rows.f32 n dim M ef_construction out.index out.halves bad.index
//
// rows.f32: n * dim floats.  Writes the index file of the engine (out.index) and the halves the upload handed to the
// C ABI (out.halves); bad.index is an index file whose rows are NOT binary16 values: loading it must be refused
// before anything is uploaded.  Exit status 0, or the number of the check that failed.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <stdexcept>
#include <vector>

#include "expann/gpu_antitopo_engine.h"

namespace {
struct Upload {
	int f16_calls = 0, f32_calls = 0, destroys = 0;
	std::vector<uint16_t> halves;
	size_t n = 0;
	int dim = 0;
} g_up;
int g_dummy_handle;
}  // namespace

extern "C" {
int expann_graph_create(int, int, const float*, size_t, uint32_t, uint32_t, const uint64_t*, const uint32_t*, expann_graph** out) {
	++g_up.f32_calls;
	*out = reinterpret_cast<expann_graph*>(&g_dummy_handle);
	return EXPANN_OK;
}
int expann_graph_create_f16(int dim, int, const void* rows_f16, size_t n, uint32_t, uint32_t, const uint64_t*,
                            const uint32_t*, expann_graph** out) {
	++g_up.f16_calls;
	g_up.dim = dim;
	g_up.n = n;
	const uint16_t* h = static_cast<const uint16_t*>(rows_f16);
	g_up.halves.assign(h, h + n * (size_t)dim);  // (reads every half the caller says is there)
	*out = reinterpret_cast<expann_graph*>(&g_dummy_handle);
	return EXPANN_OK;
}
void expann_graph_destroy(expann_graph* g) {
	if (g)
		++g_up.destroys;
}
const char* expann_graph_last_error(const expann_graph*) { return "stub"; }
int expann_graph_clear_row_filter(expann_graph*) { return EXPANN_OK; }
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main(int argc, char** argv) {
	if (argc != 9)
		return 100;
	const size_t n = std::strtoull(argv[2], nullptr, 10), dim = std::strtoull(argv[3], nullptr, 10);
	const size_t M = std::strtoull(argv[4], nullptr, 10), efc = std::strtoull(argv[5], nullptr, 10);
	std::vector<float> rows(n * dim);
	{
		FILE* f = std::fopen(argv[1], "rb");
		if (!f || std::fread(rows.data(), sizeof(float), rows.size(), f) != rows.size())
			return 101;
		std::fclose(f);
	}
	try {
		gpu_antitopo_engine<float>::config cfg(M, 2 * M, 1, efc, 1, 0.5f, 0.0f, 0);
		cfg.rows_f16 = true;
		gpu_antitopo_engine<float> eng(cfg);
		eng.index.dim = dim;
		eng.store_rows(rows.data(), n - 1);
		// a NaN, and a value that rounds to +inf, anywhere in a call: refused, nothing of the call is inserted
		std::vector<float> bad(rows.begin(), rows.begin() + 3 * dim);
		for (float poison : {std::numeric_limits<float>::quiet_NaN(), 70000.0f, -65520.0f}) {
			bad[2 * dim + 5] = poison;
			bool refused = false;
			try {
				eng.store_rows(bad.data(), 3);
			} catch (const std::invalid_argument&) {
				refused = true;
			}
			if (!refused || eng.index.size() != n - 1)
				return 1;
		}
		vec<float> last(dim);  // (the last row through store_vector: both entries round)
		for (size_t i = 0; i < dim; ++i)
			last[i] = rows[(n - 1) * dim + i];
		eng.store_vector(last);
		if (eng.index.size() != n)
			return 2;
		// the host keeps (float) of the rounded halves: what the builders saw and what the file holds
		for (size_t i = 0; i < n * dim; ++i)
			if (!same_bits(eng.index.vectors[i], expann::f16_bits_to_f32(expann::f32_to_f16_bits(rows[i]))))
				return 3;
		eng.index.write_index(argv[6]);
		eng.upload();
		if (g_up.f16_calls != 1 || g_up.f32_calls != 0 || g_up.n != n || g_up.dim != (int)dim)
			return 4;
		for (size_t i = 0; i < n * dim; ++i)
			if (g_up.halves[i] != expann::f32_to_f16_bits(rows[i]))
				return 5;
		if (eng.param_list().at("rows") != "f16")
			return 6;
		FILE* f = std::fopen(argv[7], "wb");
		if (!f || std::fwrite(g_up.halves.data(), 2, g_up.halves.size(), f) != g_up.halves.size())
			return 102;
		std::fclose(f);
		// an index file of rows that are not binary16 values: refused, nothing uploaded, the old graph stays
		gpu_antitopo_engine<float> other(cfg);
		other.index.dim = dim;
		other.index.read_index(argv[8]);
		bool refused = false;
		try {
			other.upload();
		} catch (const std::invalid_argument&) {
			refused = true;
		}
		if (!refused || g_up.f16_calls != 1 || g_up.f32_calls != 0 || other.graph)
			return 7;
		// the same file loads into an fp32 engine, and the engine's own file loads back into an f16 one
		cfg.rows_f16 = false;
		gpu_antitopo_engine<float> plain(cfg);
		plain.index.read_index(argv[8]);
		plain.upload();
		if (g_up.f32_calls != 1)
			return 8;
		other.index.read_index(argv[6]);
		other.upload();
		if (g_up.f16_calls != 2 || g_up.halves.size() != n * dim)
			return 9;
	} catch (const std::exception& ex) {
		std::fprintf(stderr, "f16_graph_engine_hook: %s\n", ex.what());
		return 10;
	}
	return 0;
}
