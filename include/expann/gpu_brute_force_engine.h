// gpu_brute_force_engine.h -- drop-in MI355X counterpart of the reference's
// brute_force_engine<T> (upstream src/brute_force_engine.h:9-46).
//
// Same CRTP shape (ann_engine<T, Derived>: _name/_param_list/_store_vector/_build/_query_k,
// src/ann_engine.h:16-29) so that basic_bench::get_benchmark_data(ann_engine<T,Engine>&)
// (src/basic_bench.h:58-59) accepts it unchanged, plus what the reference's job machinery
// needs and brute_force_engine lacks: a nested `config` and an Engine(config) constructor
// (src/bench_runner.h:33,116,120-122).  All compute goes through the C ABI of
// include/expann_hip.h; this header holds no arithmetic.
//
// Semantics kept from the reference: store_vector copies the row and assigns ids in
// insertion order (:20-22); build on an empty index is an error (:25 asserts); query_k
// returns the ids of the min(k, n) rows with the smallest (dist2, id), ascending (:28-46).
// Errors from the ABI become std::runtime_error (the job wrapper turns them into the
// variant's error string, src/bench_runner.h:18,27).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ann_engine.h"
#include "expann_hip.h"
#include "half.h"

struct gpu_brute_force_engine_config {
	int device = 0;
	int metric = EXPANN_METRIC_L2;
	long query_tile = 0;  // 0 = auto
	// more than one entry: the base is row-sharded over these devices behind the same engine
	// (expann_sharded_*: contiguous row ranges, one RCCL all-gather of the per-shard top-k, merge);
	// results are bit-identical to the single-device engine
	std::vector<int> devices;
	gpu_brute_force_engine_config() = default;
	gpu_brute_force_engine_config(int _device, int _metric = EXPANN_METRIC_L2, long _query_tile = 0)
	    : device(_device), metric(_metric), query_tile(_query_tile) {}
	gpu_brute_force_engine_config(std::vector<int> _devices, int _metric = EXPANN_METRIC_L2, long _query_tile = 0)
	    : device(_devices.empty() ? 0 : _devices[0]), metric(_metric), query_tile(_query_tile),
	      devices(std::move(_devices)) {}
};

// gpu_brute_force_engine<float>::config: the same, plus rows_f16.  When set, every stored float is rounded to
// IEEE binary16 (expann::f32_to_f16_bits: nearest even, overflow to +-inf, NaN kept, subnormals produced) and the
// library holds EXPANN_DTYPE_F16 rows: half the device memory and upload, results those of an engine over the
// rounded values, bit for bit.  Queries stay vec<float>.  Only the float engine's config has the member, so
// naming it for any other T does not compile.
struct gpu_brute_force_engine_config_f32 : gpu_brute_force_engine_config {
	using gpu_brute_force_engine_config::gpu_brute_force_engine_config;
	gpu_brute_force_engine_config_f32() = default;
	gpu_brute_force_engine_config_f32(const gpu_brute_force_engine_config& c) : gpu_brute_force_engine_config(c) {}
	bool rows_f16 = false;
};
inline bool gpu_brute_force_rows_f16(const gpu_brute_force_engine_config_f32& c) { return c.rows_f16; }
inline bool gpu_brute_force_rows_f16(const gpu_brute_force_engine_config&) { return false; }

template <typename T>
struct gpu_brute_force_engine : public ann_engine<T, gpu_brute_force_engine<T>> {
	using config = typename std::conditional<std::is_same<T, float>::value, gpu_brute_force_engine_config_f32,
	                                         gpu_brute_force_engine_config>::type;
	config conf;
	expann_index* handle = nullptr;
	expann_sharded* sharded = nullptr;  // conf.devices.size() > 1
	size_t dimension = 0;
	size_t stored = 0;
	// the reference's engine has no frozen state (src/brute_force_engine.h:20-46): rows stored after _build() are
	// appended to the built index (expann_append) and get the next ids; the sharded form refuses them
	bool built = false;
	size_t reserve_rows = 0;  // reserve() before the first row

	gpu_brute_force_engine() = default;
	explicit gpu_brute_force_engine(config c) : conf(c) {}
	gpu_brute_force_engine(const gpu_brute_force_engine&) = delete;
	gpu_brute_force_engine& operator=(const gpu_brute_force_engine&) = delete;
	~gpu_brute_force_engine() {
		expann_destroy(handle);
		expann_sharded_destroy(sharded);
	}

	void _store_vector(const vec<T>& v) {
		if (!opened())
			open(v.size());
		if (v.size() != dimension)
			throw std::runtime_error("gpu_brute_force_engine: row dimension changed");
		std::vector<T> row(dimension);
		for (size_t i = 0; i < dimension; ++i)
			row[i] = v.at(i);
		add_rows(row.data(), 1);
		++stored;
	}
	// batch form of store_vector (cf. store_many_vectors, src/pyrunner.cpp:60-82)
	void store_rows(const T* rows, size_t n, size_t dim) {
		if (!opened())
			open(dim);
		add_rows(rows, n);
		stored += n;
	}
	void _build() {
		if (!opened())
			throw std::runtime_error("gpu_brute_force_engine: build() on an empty index");
		check(sharded ? expann_sharded_build(sharded) : expann_build(handle));
		built = true;
	}
	// Extension: room for at least n rows (expann_reserve), so that rows stored after build() up to there do not
	// reallocate the base.  Before the first row there is no handle yet: the value is passed on when it is made.
	void reserve(size_t n) {
		if (sharded)
			throw std::runtime_error("gpu_brute_force_engine: reserve: the sharded engine does not grow");
		if (!handle) {
			reserve_rows = n;
			return;
		}
		check(expann_reserve(handle, n));
	}
	// Extension: rows removed from the built index (expann_remove, THE REMOVE RULE).  ids are the ids a query returns,
	// in any order, repeats counted once; the survivors keep their order and move down to fill the gaps, so the
	// caller keeps any external id map; the next stored row gets the id size().  A row filter and row groups are
	// cleared.  Returns the number of rows removed.  One device; the sharded form does not offer it.
	size_t remove_rows(const uint64_t* ids, size_t n) {
		single("remove_rows");
		size_t removed = 0;
		check(expann_remove(handle, ids, n, &removed));
		stored -= removed;
		return removed;
	}
	// ... every row the row filter in force disallows (expann_compact_row_filter); the filter is cleared
	size_t compact_row_filter() {
		single("compact_row_filter");
		size_t removed = 0;
		check(expann_compact_row_filter(handle, &removed));
		stored -= removed;
		return removed;
	}
	std::vector<size_t> _query_k(const vec<T>& v, size_t k) {
		std::vector<T> q(dimension);
		for (size_t i = 0; i < dimension; ++i)
			q[i] = v.at(i);
		std::vector<uint64_t> ids(k);
		query_k_batch(q.data(), 1, k, ids.data(), nullptr);
		std::vector<size_t> ret;
		for (size_t i = 0; i < k && ids[i] != UINT64_MAX; ++i)
			ret.push_back(size_t(ids[i]));
		return ret;
	}
	// Extension (the reference has no batch API): ids[m][k] / dists[m][k], rows ascending,
	// padded with UINT64_MAX / +inf when fewer than k rows exist.  dists may be nullptr.
	void query_k_batch(const T* queries, size_t m, size_t k, uint64_t* ids, float* dists) {
		if (!opened())
			throw std::runtime_error("gpu_brute_force_engine: query before build()");
		check(sharded ? expann_sharded_search(sharded, queries, m, k, ids, dists)
		              : expann_search(handle, queries, m, k, ids, dists));
	}
	// Extension: row filter (expann_set_row_filter).  Bit r & 31 of word r >> 5 allows row r; while it is set,
	// queries return the nearest among the allowed rows, as an index of only those rows would.  One device, float
	// rows; the sharded form does not offer it.
	void set_row_filter(const uint32_t* bits, size_t n_words) {
		single("set_row_filter");
		check(expann_set_row_filter(handle, bits, n_words));
	}
	// the same from device memory, read in the order of `stream` (a hipStream_t; nullptr = the engine's own)
	void set_row_filter_device(const uint32_t* d_bits, size_t n_words, void* stream = nullptr) {
		single("set_row_filter_device");
		check(expann_set_row_filter_device(handle, d_bits, n_words, stream));
	}
	void clear_row_filter() {
		single("clear_row_filter");
		check(expann_clear_row_filter(handle));
	}
	// Extension: row groups (expann_set_row_groups).  groups[n] gives every local row a uint32 label; a grouped batch
	// then names one label per query (host memory) and query i returns only rows with groups[r] == query_groups[i]
	// (EXPANN_GROUP_ANY: every row, the plain search bit for bit).  nullptr drops the groups.  One device, float rows.
	void set_row_groups(const uint32_t* groups, size_t n) {
		single("set_row_groups");
		check(groups ? expann_set_row_groups(handle, groups, n) : expann_clear_row_groups(handle));
	}
	void query_k_batch_grouped(const T* queries, const uint32_t* query_groups, size_t m, size_t k, uint64_t* ids, float* dists) {
		single("query_k_batch_grouped");
		check(expann_search_grouped(handle, queries, query_groups, m, k, ids, dists));
	}
	// Extension: range search (expann_range_search, THE RANGE RULE).  counts[i] = the exact number of rows with
	// score <= radii[i]; ids / dists [m][max_results] hold the min(counts[i], max_results) nearest of them, ascending,
	// padded with UINT64_MAX / +inf (dists may be nullptr; max_results == 0 only counts).  One device, float rows.
	void range_query_batch(const T* queries, const float* radii, size_t m, size_t max_results, uint64_t* ids, float* dists,
	                       uint32_t* counts) {
		single("range_query_batch");
		check(expann_range_search(handle, queries, radii, m, max_results, ids, dists, counts));
	}
	const std::string _name() { return "GPU Brute-Force Engine (MI355X)"; }
	const param_list_t _param_list() {
		param_list_t pl;
		pl["device"] = std::to_string(conf.device);
		if (sharded) {
			std::string d;
			for (int x : conf.devices)
				d += (d.empty() ? "" : ",") + std::to_string(x);
			pl["devices"] = d;
			pl["shards"] = std::to_string(expann_sharded_shards(sharded));
		}
		pl["metric"] = conf.metric == EXPANN_METRIC_IP ? "ip" : "l2";
		pl["query_tile"] = std::to_string(conf.query_tile);
		if (gpu_brute_force_rows_f16(conf))
			pl["rows"] = "f16";
		return pl;
	}

private:
	// the row types the library stores (include/expann_hip.h, expann_dtype); anything else is a
	// compile-time error rather than a silently wrong row type
	static constexpr int dtype_of() {
		static_assert(std::is_same<T, float>::value || std::is_same<T, uint8_t>::value ||
		                  std::is_same<T, int8_t>::value || std::is_same<T, int16_t>::value,
		              "gpu_brute_force_engine<T>: T must be float, uint8_t, int8_t or int16_t");
		return std::is_same<T, float>::value     ? EXPANN_DTYPE_F32
		       : std::is_same<T, uint8_t>::value ? EXPANN_DTYPE_U8
		       : std::is_same<T, int8_t>::value  ? EXPANN_DTYPE_I8
		                                         : EXPANN_DTYPE_I16;
	}
	bool opened() const { return handle || sharded; }
	// n rows of `dimension` elements to the library -- staged before _build(), appended after it --: as they are, or
	// rounded to binary16 (config::rows_f16)
	void add_rows(const T* rows, size_t n) {
		const void* src = rows;
		std::vector<uint16_t> half;
		if (gpu_brute_force_rows_f16(conf)) {
			half.resize(n * dimension);
			for (size_t i = 0; i < half.size(); ++i)
				half[i] = expann::f32_to_f16_bits(float(rows[i]));
			src = half.data();
		}
		if (sharded)
			check(expann_sharded_add(sharded, src, n));
		else
			check(built ? expann_append(handle, src, n) : expann_add(handle, src, n));
	}
	// the row filter's entry points: a built single-device engine
	void single(const char* what) const {
		if (!handle)
			throw std::runtime_error(std::string("gpu_brute_force_engine: ") + what +
			                         (sharded ? ": the sharded engine has no row filter" : " before build()"));
	}
	void open(size_t dim) {
		dimension = dim;
		const int dtype = gpu_brute_force_rows_f16(conf) ? int(EXPANN_DTYPE_F16) : dtype_of();
		if (conf.devices.size() > 1) {
			int rc = expann_sharded_create(int(dim), dtype, conf.metric, conf.devices.data(),
			                               int(conf.devices.size()), &sharded);
			if (rc != EXPANN_OK)
				throw std::runtime_error(std::string("expann_sharded_create: ") + expann_sharded_last_error(nullptr));
			if (conf.query_tile)
				check(expann_sharded_set_option(sharded, "query_tile", conf.query_tile));
			return;
		}
		int rc = expann_create(int(dim), dtype, conf.metric, conf.devices.empty() ? conf.device : conf.devices[0],
		                       &handle);
		if (rc != EXPANN_OK)
			throw std::runtime_error(std::string("expann_create: ") + expann_last_error(nullptr));
		if (conf.query_tile)
			check(expann_set_option(handle, "query_tile", conf.query_tile));
		if (reserve_rows)
			check(expann_reserve(handle, reserve_rows));
	}
	void check(int rc) {
		if (rc != EXPANN_OK)
			throw std::runtime_error(std::string("expann_hip: ") +
			                         (sharded ? expann_sharded_last_error(sharded) : expann_last_error(handle)));
	}
};
