// f16_engine_hook.cpp -- test hook (compiled by tests/test_gpu_f16_rows.py with g++ against libexpann_hip.so):
// the C++ surface of the fp16-row index.  gpu_brute_force_engine<float> with config::rows_f16 takes float rows,
// rounds them to binary16 on the host (include/expann/half.h) and hands the library EXPANN_DTYPE_F16 rows;
// queries stay float.  (gpu_brute_force_engine<uint8_t>::config has no rows_f16: naming it there does not compile.)
#include <cstddef>
#include <cstdint>
#include <exception>

#include "expann/gpu_brute_force_engine.h"

static_assert(!std::is_same<gpu_brute_force_engine<float>::config, gpu_brute_force_engine<uint8_t>::config>::value,
              "rows_f16 belongs to the float engine's config only");

extern "C" int f16_engine_query(const float* rows, size_t n, size_t dim, int metric, const float* queries, size_t m,
                                size_t k, uint64_t* ids, float* dists) {
	try {
		gpu_brute_force_engine<float>::config cfg(0, metric);
		cfg.rows_f16 = true;
		gpu_brute_force_engine<float> eng(cfg);
		eng.store_rows(rows, n - 1, dim);
		vec<float> last(dim);  // (the last row through store_vector: both entries round)
		for (size_t i = 0; i < dim; ++i)
			last[i] = rows[(n - 1) * dim + i];
		eng.store_vector(last);
		eng.build();
		if (eng.param_list().at("rows") != "f16")
			return 2;
		eng.query_k_batch(queries, m, k, ids, dists);
		return 0;
	} catch (const std::exception&) {
		return 1;
	}
}
