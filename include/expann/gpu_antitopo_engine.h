// gpu_antitopo_engine.h -- drop-in MI355X counterpart of the reference's graph engine
// `antitopo_engine<T>` (upstream src/antitopo_engine.h:104-260) behind the same CRTP shape
// (ann_engine<T, Derived>, src/ann_engine.h:16-29) and the same `config` convention
// (src/bench_runner.h:33,116,120-122; antitopo_engine_config, src/antitopo_engine.h:72-101).
//
// Division of labour: the graph is BUILT on the host (antitopo_index.h, a restatement of
// _store_vector / prune_edges; or read from an index file written by the reference itself,
// read_index/write_index), the QUERY side -- greedy descent, best-first bottom-layer search with
// its candidate scoring and queues, uint8 path and re-score -- runs on the GPU through
// expann_graph_search.  _query_k keeps the reference's "sticky" ef_search (:858-859).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "ann_engine.h"
#include "antitopo_index.h"
#include "expann_hip.h"
#include "half.h"

struct gpu_antitopo_engine_config : public expann::antitopo_config {
	int device = 0;
	std::string index_filename;
	bool read_index = false, write_index = false;
	// bottom-layer scoring of the walk (expann_graph_compression); -1: what use_compression says (0 or 1).
	// 2 = the ranged int8 walk, which the reference has no switch for.
	int compression_mode = -1;
	int mode() const { return compression_mode < 0 ? (use_compression ? 1 : 0) : compression_mode; }
	// Extension: the device keeps the rows as IEEE binary16 (expann_graph_create_f16): half the gathered bytes of a
	// hop and half the device copy.  Every stored float is rounded to the nearest-even binary16 AS IT COMES IN and
	// (float) of that is what the host keeps: the builders and the index file see exactly the values the device
	// holds, so no rounding happens after the edges were chosen.  Set before the first row is stored.
	bool rows_f16 = false;
	gpu_antitopo_engine_config() = default;
	// same argument order as antitopo_engine_config (src/antitopo_engine.h:88-101)
	gpu_antitopo_engine_config(size_t _M, size_t _M0, size_t _ef_search_mult, size_t _ef_construction,
	                           size_t _ortho_count, float _ortho_factor, float _ortho_bias,
	                           size_t _prune_overflow, bool _use_compression = false,
	                           bool _use_largest_direction_filtering = false,
	                           std::string _index_filename = "", bool _read_index = false,
	                           bool _write_index = false) {
		M = _M; M0 = _M0; ef_search_mult = _ef_search_mult; ef_construction = _ef_construction;
		ortho_count = _ortho_count; ortho_factor = _ortho_factor; ortho_bias = _ortho_bias;
		prune_overflow = _prune_overflow; use_compression = _use_compression;
		use_largest_direction_filtering = _use_largest_direction_filtering;
		index_filename = _index_filename; read_index = _read_index; write_index = _write_index;
	}
};

template <typename T>
struct gpu_antitopo_engine : public ann_engine<T, gpu_antitopo_engine<T>> {
	using config = gpu_antitopo_engine_config;
	config conf;
	expann::antitopo_index index;
	expann_graph* graph = nullptr;
	std::optional<size_t> ef_search;
	size_t num_distcomps = 0;  // RECORD_STATS counter (src/antitopo_engine.h:125-129)
	uint64_t device_distcomps_seen = 0;  // the graph handle's device counter at the last sync()
	bool resident = false;  // the graph handle holds the builder's state (append_rows; a new handle starts without)

	explicit gpu_antitopo_engine(config c) : conf(c) { index.conf = c; }
	gpu_antitopo_engine(const gpu_antitopo_engine&) = delete;
	gpu_antitopo_engine& operator=(const gpu_antitopo_engine&) = delete;
	~gpu_antitopo_engine() { expann_graph_destroy(graph); }

	void set_ef_search(size_t e) {  // src/antitopo_engine.h:189-195
		ef_search = e;
		index.has_ef_search = true;
		index.ef_search = e;
	}

	// rows_f16: `count` floats rounded to binary16 and back; a NaN, or a value that rounds to +-inf, is refused
	// before anything is stored
	static std::vector<float> rounded_to_f16(const float* x, size_t count) {
		std::vector<float> r(count);
		for (size_t i = 0; i < count; ++i) {
			const uint16_t h = expann::f32_to_f16_bits(x[i]);
			if ((h & 0x7c00u) == 0x7c00u)
				throw std::invalid_argument("gpu_antitopo_engine: rows_f16 refuses a NaN or a value beyond binary16's range "
				                            "(component " + std::to_string(i) + ")");
			r[i] = expann::f16_bits_to_f32(h);
		}
		return r;
	}
	// ---- Extension: appends to the built graph (THE GRAPH APPEND RULE, expann_hip.h) ----
	// the engines append_rows serves with store_rows_batched + _build(), as before: binary16 rows, several ortho entry
	// points, fewer than store_rows_batched's n_serial rows
	bool append_on_host() const {
		return conf.rows_f16 || conf.ortho_count != 1 || conf.read_index || index.size() < 2048 || index.size() > (8u << 20);
	}
	// After an append on the device the host's adjacency is that of the graph before it (index.adjacency_stale);
	// everything that reads index.hadj_* calls this first.  The download is reached through a pointer that
	// append_rows sets where it sets the flag: a program that never appends does not refer to the append's library
	// calls (the native test hooks stub the few calls of the library they use).
	void (gpu_antitopo_engine::*download_fn)() = nullptr;
	void refresh_host() {
		if (index.adjacency_stale)
			(this->*download_fn)();
	}
	// the builder's state from the device, from_strided
	void download_adjacency() {
		size_t shape[6];
		auto check = [&](int rc) {
			if (rc != EXPANN_OK)
				throw std::runtime_error(std::string("gpu_antitopo_engine: reading the graph back: ") + expann_graph_last_error(graph));
		};
		check(expann_graph_build_state_shape(graph, shape));
		expann::antitopo_index::strided_graph g;
		g.n = shape[0];
		g.U = shape[1];  // (the row stride of the upper arrays: the device's capacity)
		g.n_upper_layers = shape[2];
		g.stride0 = shape[4];
		g.strideu = shape[5];
		g.levels.resize(g.n);
		g.upper_idx.resize(g.n);
		g.ids0.resize(g.n * g.stride0);
		g.d0.resize(g.n * g.stride0);
		g.deg0.resize(g.n);
		g.idsu.resize(g.U * g.n_upper_layers * g.strideu);
		g.du.resize(g.U * g.n_upper_layers * g.strideu);
		g.degu.resize(g.U * g.n_upper_layers);
		check(expann_graph_read_build_state(graph, g.levels.data(), g.upper_idx.data(), g.ids0.data(), g.d0.data(),
		                                    g.deg0.data(), g.idsu.data(), g.du.data(), g.degu.data()));
		if (g.n != index.size())
			throw std::runtime_error("gpu_antitopo_engine: the device graph and the host rows differ in size");
		index.from_strided(g, nullptr, index.max_layer, index.starting_vertex);
		index.adjacency_stale = false;
	}
	// What the host route carries over a re-upload: the graph handle's seven remove counters, then its six append
	// counters, in the order of GraphStats::Removes, remove_repair_ns and GraphStats::Appends (expann_graph.hip).
	void read_carried_stats(uint64_t* out, int first, int count) const {
		static const char* const names[13] = {"remove_calls", "remove_rows", "remove_touched_rows", "remove_truncated_rows",
		                                      "remove_device", "remove_host", "remove_repair_ns",
		                                      "append_calls", "append_rows", "append_batches",
		                                      "append_device", "append_host", "graph_reallocs"};
		for (int i = 0; i < count; ++i)
			if (expann_graph_get_stat(graph, names[first + i], out + i) != EXPANN_OK)
				out[i] = 0;
	}
	void read_append_stats(uint64_t* six) const { read_carried_stats(six, 7, 6); }
	// The builder's view of the graph handed to the handle, once (the first append or remove on the device route).
	// *on_host is set when the handle cannot take it (EXPANN_ERR_UNSUPPORTED): the call goes the host route.
	int adopt_on_device(bool* on_host) {
		if (resident)
			return EXPANN_OK;
		refresh_host();
		const auto g = index.to_strided({}, 64);
		bool fits = true;  // (rows of a graph built with these M / M0: a foreign index file may hold longer ones)
		for (size_t v = 0; v < g.n && fits; ++v)
			fits = g.deg0[v] <= conf.M0;
		for (size_t r = 0; r < g.degu.size() && fits; ++r)
			fits = g.degu[r] <= conf.M;
		const int rc = !fits ? EXPANN_ERR_UNSUPPORTED
		                     : expann_graph_adopt_build_state(graph, conf.M, conf.M0, conf.ef_construction, conf.prune_overflow,
		                                                      conf.ortho_factor, conf.ortho_bias, g.levels.data(),
		                                                      g.upper_idx.data(), g.ids0.data(), g.d0.data(), g.deg0.data(),
		                                                      g.stride0, g.U, g.n_upper_layers, g.idsu.data(), g.du.data(),
		                                                      g.degu.data(), g.strideu);
		if (rc == EXPANN_ERR_UNSUPPORTED)
			*on_host = true;
		else if (rc != EXPANN_OK)
			return rc;
		else
			resident = true;
		return EXPANN_OK;
	}
	// `n` rows appended to the built graph.  Returns the expann_status (message: expann_graph_last_error(graph));
	// *n_appended: the rows that are in -- n, or fewer with EXPANN_ERR_OVERFLOW.  Throws what store_rows_batched and
	// _build() throw on the host route.
	int append_rows(const float* rows, size_t n, size_t* n_appended = nullptr) {
		if (n_appended)
			*n_appended = 0;
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (n == 0)
			return EXPANN_OK;
		if (!rows)
			return EXPANN_ERR_INVALID_ARG;
		bool on_host = append_on_host();
		if (!on_host) {  // the handle's first append: the builder's view, uploaded once
			const int rc = adopt_on_device(&on_host);
			if (rc != EXPANN_OK)
				return rc;
		}
		if (on_host) {
			refresh_host();
			uint64_t carried[6];
			read_append_stats(carried);
			store_rows_batched(rows, n);
			_build();
			(void)expann_graph_note_host_append(graph, carried, n);
			if (n_appended)
				*n_appended = n;
			return EXPANN_OK;
		}
		const expann::mt19937_ref gen_before = index.gen;
		std::vector<uint8_t> lv(n);
		for (size_t i = 0; i < n; ++i)
			lv[i] = (uint8_t)std::min<size_t>(index.draw_level(), 250);
		uint32_t ml = 0, sv = 0;
		size_t done = 0;
		const int rc = expann_graph_append(graph, rows, n, lv.data(), &ml, &sv, &done);
		if (rc != EXPANN_OK && rc != EXPANN_ERR_OVERFLOW) {
			index.gen = gen_before;
			return rc;
		}
		if (done < n) {  // the generator stands after the draws of the rows that are in
			index.gen = gen_before;
			for (size_t i = 0; i < done; ++i)
				(void)index.draw_level();
		}
		if (done) {
			index.vectors.insert(index.vectors.end(), rows, rows + done * index.dim);
			index.visited.resize(index.size(), 0);
			index.max_layer = ml;
			index.starting_vertex = sv;
			index.adjacency_stale = true;
			download_fn = &gpu_antitopo_engine::download_adjacency;
		}
		if (n_appended)
			*n_appended = done;
		return rc;
	}
	// ---- Extension: rows taken out of the built graph (THE GRAPH REMOVE RULE, expann_hip.h) ----
	void read_remove_stats(uint64_t* thirteen) const { read_carried_stats(thirteen, 0, 13); }
	std::string remove_error;  // what an engine-level refusal of the last remove_rows / compact_row_filter said
	// The rows `ids` (any order, repeats allowed) taken out.  Returns the expann_status (message: remove_error, or when
	// that is empty expann_graph_last_error(graph)); *n_removed: the distinct ids.  The routes are append_rows'.
	// Refusals -- an id >= size, a removal that would leave no row -- are decided before anything changes.  Throws
	// what _build() throws on the host route.
	int remove_rows(const uint64_t* ids, size_t n, size_t* n_removed = nullptr) {
		remove_error.clear();
		if (n_removed)
			*n_removed = 0;
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (n == 0)
			return EXPANN_OK;
		if (!ids)
			return EXPANN_ERR_INVALID_ARG;
		const size_t n_old = index.size();
		std::vector<char> gone(n_old, 0);
		size_t n_gone = 0;
		for (size_t i = 0; i < n; ++i) {
			if (ids[i] >= n_old) {
				remove_error = "remove: id " + std::to_string(ids[i]) + " at or beyond size()";
				return EXPANN_ERR_INVALID_ARG;
			}
			n_gone += !gone[ids[i]];
			gone[ids[i]] = 1;
		}
		if (n_gone == n_old) {
			remove_error = "remove: would leave no row (a graph is never empty)";
			return EXPANN_ERR_INVALID_ARG;
		}
		bool on_host = append_on_host();
		if (!on_host) {
			const int rc = adopt_on_device(&on_host);
			if (rc != EXPANN_OK)
				return rc;
		}
		if (on_host) {
			refresh_host();
			uint64_t carried[13];
			read_remove_stats(carried);
			size_t removed = 0;
			index.remove_rows(ids, n, &removed);
			_build();
			(void)expann_graph_note_host_remove(graph, carried, removed);
			if (n_removed)
				*n_removed = removed;
			return EXPANN_OK;
		}
		uint32_t ml = 0, sv = 0;
		size_t removed = 0;
		const int rc = expann_graph_remove(graph, ids, n, &ml, &sv, &removed);
		if (rc != EXPANN_OK)
			return rc;
		// the host's copy of the rows, compacted here: the one piece of work proportional to the size
		size_t to = 0;
		for (size_t v = 0; v < n_old; ++v)
			if (!gone[v]) {
				if (to != v)
					std::copy(index.vectors.begin() + v * index.dim, index.vectors.begin() + (v + 1) * index.dim,
					          index.vectors.begin() + to * index.dim);
				++to;
			}
		index.vectors.resize(to * index.dim);
		index.visited.assign(to, 0);
		index.max_layer = ml;
		index.starting_vertex = sv;
		index.adjacency_stale = true;
		download_fn = &gpu_antitopo_engine::download_adjacency;
		if (n_removed)
			*n_removed = removed;
		return rc;
	}
	// remove_rows of the rows the bitmap filter in force disallows: tombstones made permanent.  No filter in force, or
	// one that allows no row: EXPANN_ERR_INVALID_ARG.  A filter that allows every row removes nothing and is cleared.
	int compact_row_filter(size_t* n_removed = nullptr) {
		remove_error.clear();
		if (n_removed)
			*n_removed = 0;
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		const size_t n_old = index.size();
		std::vector<uint32_t> bits((n_old + 31) / 32);
		const int rc = expann_graph_read_row_filter(graph, bits.data(), bits.size());
		if (rc != EXPANN_OK)
			return rc;
		std::vector<uint64_t> ids;
		for (size_t v = 0; v < n_old; ++v)
			if (!((bits[v >> 5] >> (v & 31)) & 1u))
				ids.push_back(v);
		if (ids.empty()) {
			clear_row_filter();
			return EXPANN_OK;
		}
		return remove_rows(ids.data(), ids.size(), n_removed);
	}
	// room for n_rows rows on the device, so that appends up to there reallocate nothing
	int reserve(size_t n_rows) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (append_on_host())
			return EXPANN_OK;
		return expann_graph_reserve(graph, n_rows);
	}
	// write_index of the graph as it is now
	void save_index(const std::string& path) {
		refresh_host();
		index.write_index(path);
	}

	void _store_vector(const vec<T>& v) {
		if (conf.read_index)
			return;  // :312-313
		refresh_host();
		if (index.dim == 0)
			index.dim = v.size();
		std::vector<float> row(index.dim);
		for (size_t i = 0; i < index.dim; ++i)
			row[i] = float(v.at(i));
		if (conf.rows_f16)
			row = rounded_to_f16(row.data(), row.size());
		index.insert(row.data());
	}
	// Extension: `n` rows of index.dim floats through the serial builder (rows_f16: rounded first, all or none)
	void store_rows(const float* rows, size_t n) {
		if (conf.read_index || n == 0)
			return;
		refresh_host();
		if (index.dim == 0)
			throw std::runtime_error("gpu_antitopo_engine: dimension not set");
		std::vector<float> rounded;
		if (conf.rows_f16) {
			rounded = rounded_to_f16(rows, n * index.dim);
			rows = rounded.data();
		}
		for (size_t i = 0; i < n; ++i)
			index.insert(rows + i * index.dim);
	}
	// Extension: `n` rows through the batched GPU builder (expann_graph_build_batched,
	// csrc/graph_build.hpp).  The first rows of an empty engine -- until n_serial are stored -- go
	// through the serial restatement and seed the batches; level draws stay the reference's sequence.
	// Returns the builder's statistics {batches, dropped reverse edges, rows re-pruned, 0}.
	std::vector<uint64_t> store_rows_batched(const float* rows, size_t n, size_t n_serial = 2048, size_t max_batch = 0) {
		std::vector<uint64_t> stats(4, 0);
		if (conf.read_index || n == 0)
			return stats;
		refresh_host();
		if (index.dim == 0)
			throw std::runtime_error("gpu_antitopo_engine: dimension not set");
		std::vector<float> rounded;  // (rows_f16: the batched builder receives the upcast fp32 rows)
		if (conf.rows_f16) {
			rounded = rounded_to_f16(rows, n * index.dim);
			rows = rounded.data();
		}
		if (conf.ortho_count != 1) {  // (several ortho entry points: serial path only)
			for (size_t i = 0; i < n; ++i)
				index.insert(rows + i * index.dim);
			return stats;
		}
		std::vector<uint8_t> lv(n);
		for (size_t i = 0; i < n; ++i)
			lv[i] = (uint8_t)std::min<size_t>(index.draw_level(), 250);
		size_t i = 0;
		for (; i < n && index.size() < n_serial; ++i)
			index.insert_with_level(rows + i * index.dim, lv[i]);
		if (i == n)
			return stats;
		const size_t built = index.size();
		auto g = index.to_strided(std::vector<uint8_t>(lv.begin() + i, lv.end()), 64);
		std::vector<float> all(index.vectors);
		all.insert(all.end(), rows + i * index.dim, rows + n * index.dim);
		uint32_t ml = (uint32_t)index.max_layer, sv = (uint32_t)index.starting_vertex;
		int rc = expann_graph_build_batched(int(index.dim), conf.device, all.data(), g.n, g.levels.data(), built, &ml, &sv,
		                                    conf.M, conf.M0, conf.ef_construction, conf.prune_overflow,
		                                    conf.ortho_factor, conf.ortho_bias, max_batch, g.ids0.data(), g.d0.data(),
		                                    g.deg0.data(), g.stride0, g.upper_idx.data(), g.U, g.n_upper_layers,
		                                    g.idsu.data(), g.du.data(), g.degu.data(), g.strideu, stats.data());
		if (rc != EXPANN_OK)
			throw std::runtime_error(std::string("expann_graph_build_batched: ") + expann_graph_last_error(nullptr));
		std::vector<float>().swap(all);
		index.from_strided(g, rows + i * index.dim, ml, sv);
		return stats;
	}
	void _build() {  // :467-493
		refresh_host();
		if (conf.write_index && !conf.index_filename.empty())
			index.write_index(conf.index_filename);
		if (conf.read_index)
			index.read_index(conf.index_filename);
		if (index.size() == 0)
			throw std::runtime_error("gpu_antitopo_engine: build() on an empty index");
		upload();
		num_distcomps = 0;
	}
	// rows_f16: the host rows as binary16 bit patterns.  Every value must be one already -- rows stored through this
	// engine are; an index file read from elsewhere may not be, and is refused rather than rounded under its edges.
	std::vector<uint16_t> pack_rows_f16() const {
		std::vector<uint16_t> h(index.vectors.size());
		for (size_t i = 0; i < h.size(); ++i) {
			const float x = index.vectors[i];
			h[i] = expann::f32_to_f16_bits(x);
			const float back = expann::f16_bits_to_f32(h[i]);
			if ((h[i] & 0x7c00u) == 0x7c00u || std::memcmp(&back, &x, sizeof(x)) != 0)
				throw std::invalid_argument("gpu_antitopo_engine: rows_f16 needs rows that are exactly binary16 values (row " +
				                            std::to_string(i / index.dim) + ")");
		}
		return h;
	}
	void upload() {
		std::vector<uint16_t> halves;
		if (conf.rows_f16)
			halves = pack_rows_f16();  // (throws before the device is touched and before the old graph goes)
		refresh_host();
		const auto fg = index.flatten();
		expann_graph_destroy(graph);
		graph = nullptr;
		resident = false;
		device_distcomps_seen = 0;
		int rc = conf.rows_f16
		             ? expann_graph_create_f16(int(index.dim), conf.device, halves.data(), index.size(), fg.n_layers,
		                                       fg.starting_vertex, fg.layer_offsets.data(), fg.neighbours.data(), &graph)
		             : expann_graph_create(int(index.dim), conf.device, index.vectors.data(), index.size(),
		                                   fg.n_layers, fg.starting_vertex, fg.layer_offsets.data(),
		                                   fg.neighbours.data(), &graph);
		if (rc != EXPANN_OK)
			throw std::runtime_error(std::string(conf.rows_f16 ? "expann_graph_create_f16: " : "expann_graph_create: ") +
			                         expann_graph_last_error(nullptr));
	}
	std::vector<size_t> _query_k(const vec<T>& v, size_t k) {
		std::vector<float> q(index.dim);
		for (size_t i = 0; i < index.dim; ++i)
			q[i] = float(v.at(i));
		std::vector<uint64_t> ids(k);
		std::vector<float> dists(k);
		query_k_batch(q.data(), 1, k, ids.data(), dists.data());
		std::vector<size_t> ret;
		for (size_t i = 0; i < k && ids[i] != UINT64_MAX; ++i)
			ret.push_back(size_t(ids[i]));
		return ret;
	}
	// Extension: m queries in one launch.  distcomps (per query) may be nullptr.
	void query_k_batch(const float* queries, size_t m, size_t k, uint64_t* ids, float* dists,
	                   uint32_t* distcomps = nullptr) {
		if (!graph)
			throw std::runtime_error("gpu_antitopo_engine: query before build()");
		if (!ef_search.has_value())
			set_ef_search(k * conf.ef_search_mult);  // :858-859
		std::vector<uint32_t> dc(m);
		int rc = expann_graph_search_mode(graph, queries, m, k, ef_search.value(), conf.mode(), ids, dists,
		                                  dc.data());
		if (rc != EXPANN_OK)
			throw std::runtime_error(std::string("expann_graph_search: ") +
			                         expann_graph_last_error(graph));
		for (size_t i = 0; i < m; ++i) {
			num_distcomps += dc[i];
			if (distcomps)
				distcomps[i] = dc[i];
		}
	}
	// Extension: the same on device buffers, enqueued on `stream` (nullptr = the graph handle's) without waiting:
	// expann_graph_search_device with the sticky ef_search and conf.mode() of query_k_batch.  Returns the
	// expann_status (message: expann_graph_last_error(graph)); results are valid after sync().
	int query_k_batch_device(const float* d_queries, size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (k == 0)
			return expann_graph_search_device(graph, d_queries, m, k, 1, conf.mode(), d_ids, d_dists, nullptr, stream);
		if (!ef_search.has_value())
			set_ef_search(k * conf.ef_search_mult);  // :858-859
		return expann_graph_search_device(graph, d_queries, m, k, ef_search.value(), conf.mode(), d_ids, d_dists, nullptr,
		                                  stream);
	}
	// Extension: the row filter of the queries from now on (expann_graph_set_row_filter; nullptr clears it).  A
	// run-time property of the uploaded graph: upload() -- build and load -- starts without one, and it is not
	// written to the index file.  Returns the expann_status (message: expann_graph_last_error(graph)).
	int set_row_filter(const uint32_t* allow_bits, size_t n_words) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		return allow_bits ? expann_graph_set_row_filter(graph, allow_bits, n_words) : expann_graph_clear_row_filter(graph);
	}
	// the same from device bits, read in the order of `stream` (expann_graph_set_row_filter_device)
	int set_row_filter_device(const uint32_t* d_allow_bits, size_t n_words, void* stream) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		return expann_graph_set_row_filter_device(graph, d_allow_bits, n_words, stream);
	}
	void clear_row_filter() {
		if (graph)
			(void)expann_graph_clear_row_filter(graph);
	}
	// Extension: row groups (THE GROUP RULE, expann_hip.h): a label per row, and searches in which every query names
	// the group it may return.  Like the row filter a run-time property of the uploaded graph: upload() starts
	// without groups and they are not written to the index file.  nullptr clears them.  All return the
	// expann_status (message: expann_graph_last_error(graph)).
	int set_row_groups(const uint32_t* groups, size_t n) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		return groups ? expann_graph_set_row_groups(graph, groups, n) : expann_graph_clear_row_groups(graph);
	}
	int set_row_groups_device(const uint32_t* d_groups, size_t n, void* stream) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		return expann_graph_set_row_groups_device(graph, d_groups, n, stream);
	}
	void clear_row_groups() {
		if (graph)
			(void)expann_graph_clear_row_groups(graph);
	}
	// m queries, query i within group query_groups[i] (EXPANN_GROUP_ANY: every row), with the sticky ef_search and
	// conf.mode() of query_k_batch; distcomps (per query) may be nullptr
	int query_k_batch_grouped(const float* queries, const uint32_t* query_groups, size_t m, size_t k, uint64_t* ids,
	                          float* dists, uint32_t* distcomps = nullptr) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (k == 0)
			return expann_graph_search_grouped(graph, queries, query_groups, m, k, 1, conf.mode(), ids, dists, nullptr);
		if (!ef_search.has_value())
			set_ef_search(k * conf.ef_search_mult);  // :858-859
		std::vector<uint32_t> dc(m);
		const int rc = expann_graph_search_grouped(graph, queries, query_groups, m, k, ef_search.value(), conf.mode(), ids,
		                                           dists, dc.data());
		if (rc != EXPANN_OK)
			return rc;
		for (size_t i = 0; i < m; ++i) {
			num_distcomps += dc[i];
			if (distcomps)
				distcomps[i] = dc[i];
		}
		return rc;
	}
	// the same on device buffers, enqueued on `stream` without waiting; results are valid after sync()
	int query_k_batch_grouped_device(const float* d_queries, const uint32_t* d_query_groups, size_t m, size_t k,
	                                 uint64_t* d_ids, float* d_dists, void* stream) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (k == 0)
			return expann_graph_search_grouped_device(graph, d_queries, d_query_groups, m, k, 1, conf.mode(), d_ids, d_dists,
			                                          nullptr, stream);
		if (!ef_search.has_value())
			set_ef_search(k * conf.ef_search_mult);  // :858-859
		return expann_graph_search_grouped_device(graph, d_queries, d_query_groups, m, k, ef_search.value(), conf.mode(),
		                                          d_ids, d_dists, nullptr, stream);
	}
	// Extension: range search by the walk (THE RANGE WALK RULE, expann_hip.h): per query the rows within radii[i]
	// (squared L2) that the walk scored -- ids / dists [m][max_results] ascending and padded, counts[m] the in-range
	// rows scored.  fp32 bottom layer whatever conf.mode() says; the sticky ef_search of query_k_batch, set when unset
	// as query_k_batch sets it with k = max(1, max_results).  dists and distcomps may be nullptr, ids too with
	// max_results == 0.  Returns the expann_status (message: expann_graph_last_error(graph)).
	int range_query_batch(const float* queries, const float* radii, size_t m, size_t max_results, uint64_t* ids,
	                      float* dists, uint32_t* counts, uint32_t* distcomps = nullptr) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (!ef_search.has_value())
			set_ef_search(std::max<size_t>(1, max_results) * conf.ef_search_mult);  // :858-859
		std::vector<uint32_t> dc(m);
		const int rc = expann_graph_range_search(graph, queries, radii, m, max_results, ef_search.value(), ids, dists, counts,
		                                         dc.data());
		if (rc != EXPANN_OK)
			return rc;
		for (size_t i = 0; i < m; ++i) {
			num_distcomps += dc[i];
			if (distcomps)
				distcomps[i] = dc[i];
		}
		return rc;
	}
	// the same on device buffers, enqueued on `stream` without waiting; results are valid after sync()
	int range_query_batch_device(const float* d_queries, const float* d_radii, size_t m, size_t max_results, uint64_t* d_ids,
	                             float* d_dists, uint32_t* d_counts, void* stream) {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		if (!ef_search.has_value())
			set_ef_search(std::max<size_t>(1, max_results) * conf.ef_search_mult);  // :858-859
		return expann_graph_range_search_device(graph, d_queries, d_radii, m, max_results, ef_search.value(), d_ids, d_dists,
		                                        d_counts, nullptr, stream);
	}
	// expann_graph_sync; the distance evaluations the device counted since the last sync go to num_distcomps
	int sync() {
		if (!graph)
			return EXPANN_ERR_NOT_BUILT;
		const int rc = expann_graph_sync(graph);
		uint64_t total = 0;
		if (expann_graph_get_stat(graph, "distcomps", &total) == EXPANN_OK && total >= device_distcomps_seen) {
			num_distcomps += size_t(total - device_distcomps_seen);
			device_distcomps_seen = total;
		}
		return rc;
	}
	const std::string _name() { return "GPU Anti-Topo Engine+ (MI355X)"; }
	const param_list_t _param_list() {  // :242-259
		param_list_t pl;
		pl["M"] = std::to_string(conf.M);
		pl["M0"] = std::to_string(conf.M0);
		pl["ef_search_mult"] = std::to_string(conf.ef_search_mult);
		pl["ef_construction"] = std::to_string(conf.ef_construction);
		pl["ortho_count"] = std::to_string(conf.ortho_count);
		pl["ortho_factor"] = std::to_string(conf.ortho_factor);
		pl["ortho_bias"] = std::to_string(conf.ortho_bias);
		pl["prune_overflow"] = std::to_string(conf.prune_overflow);
		pl["use_compression"] = std::to_string(conf.mode() != EXPANN_GRAPH_FP32);
		if (conf.mode() == EXPANN_GRAPH_RANGED_Q8)
			pl["compression_mode"] = "ranged";
		pl["use_largest_direction_filtering"] = std::to_string(conf.use_largest_direction_filtering);
		pl["num_distcomps"] = std::to_string(num_distcomps);
		if (conf.rows_f16)
			pl["rows"] = "f16";
		return pl;
	}
};
