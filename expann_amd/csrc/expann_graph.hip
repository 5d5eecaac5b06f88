// expann_graph.hip -- C ABI of the graph path (expann_graph_*, expann_antitopo_*) and of the
// quantiser builds (expann_quantize_*): SURVEY 8 rows a-7..a-11, a-13, f-2, f-3.  The brute-force
// index lives in expann_hip.hip; both files share host_common.hpp.
#include "../../include/expann_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "bf_remove.hpp"
#include "filter_rows.hpp"
#include "graph_append.hpp"
#include "graph_build.hpp"
#include "graph_builder_state.hpp"
#include "graph_flat_scan.hpp"
#include "graph_options.hpp"
#include "graph_remove.hpp"
#include "graph_search.hpp"
#include "host_common.hpp"
#include "quantize.hpp"

using namespace expann;

// The handle's state, grouped by who makes it and when it dies, as expann_index's (expann_hip.hip, whose groups have
// the names without "Graph"): bases of expann_graph (use sites read g->d_adj0) whose members free themselves, so a
// group is forgotten as a value, g->forget<GraphRowGroups>(), and a member added to one needs no edit anywhere else.

// what expann_graph_create fixes
struct GraphRows {
	int dim = 0, device = 0;
	size_t n = 0;
	uint32_t n_layers = 0, starting_vertex = 0, max_degree0 = 0;
	// the rows: [n][dim] floats, or -- rows_f16, a handle made by expann_graph_create_f16 -- [n][dim] binary16 values;
	// the flag picks the _Float16 instances of the walk, the scan and the quantisers, and nothing else
	DevPtr<void> d_vectors;
	bool rows_f16 = false;
	DevPtr<uint32_t> d_layer_off;
	DevPtr<uint32_t> d_neighbours;
	DevPtr<uint32_t> d_adj0;  // [n][stride0] layer-0 lists at a fixed stride, padded with UINT32_MAX
	uint32_t stride0 = 0;
	// rows that d_vectors, d_adj0 and the visited sets have room for: n at create, more after expann_graph_reserve or
	// an append that grew them (THE GRAPH APPEND RULE)
	size_t cap_rows = 0;
};

// the byte copies of the rows, each made at the first use of its mode
struct GraphRowBytes {
	DevPtr<uint8_t> d_compressed;
	// quantizer_ranged_q8 copy of the rows (bytes in [0, 127]) with its scale_factor / offset;
	// ranged_state: 0 = not built yet, 1 = usable, -1 = the quantiser is unusable
	DevPtr<uint8_t> d_ranged;
	float ranged_scale = 0, ranged_offset = 0;
	int ranged_state = 0;
};

// one visited set per workgroup of the search grid, made at create
struct GraphVisited {
	DevPtr<uint8_t> d_visited;  // epoch bytes [slots][n], or -- vis_words != 0 -- bitsets [slots][vis_words]
	uint32_t vis_words = 0;
	DevPtr<uint32_t> d_epochs;
	uint32_t slots = 0;
};

// what the searches share, made at the handle's first one (graph_dev_init), and the bookkeeping of the device-buffer
// searches (expann_graph_search_device / expann_graph_sync)
struct GraphDeviceSearches {
	// One counter slot per search: {overflow flag, first launch's query counter, redo count, redo launch's query
	// counter, and -- grouped searches -- the scan's query counter and the queries walked, scanned, padded}; a search
	// resets its slot in stream order.  Slots [0, kGraphMaxOutstanding) belong to the
	// outstanding device-buffer searches (the sync reads them all), the last one to the host-buffer call.
	DevPtr<uint32_t> d_dev_ctr;            // [kGraphMaxOutstanding + 1][kGraphCtrWords]
	PinPtr<uint32_t> h_dev_ctr;            // the same, read back
	DevPtr<unsigned long long> d_dc_total; // [1] distcomps of every device search since create
	PinPtr<unsigned long long> h_dc_total;
	GrowPtr<uint32_t> d_redo_list;         // [largest m seen]
	hipStream_t dev_stream = nullptr;      // the stream of the outstanding searches (the caller's, or `stream`: borrowed)
	uint32_t dev_outstanding = 0;          // searches enqueued since the last drain (= slots in use)
	OwnedEvent ev_dev[3];                  // before the first launch, after it, after the redo launch
	bool dev_timed = false, dev_timed_redo = false;  // ev_dev hold the last search (and its redo launch)
	uint64_t pend_redo_queries = 0, pend_overflows = 0;  // what the drains since the last sync found
};

// The builder's view of the graph, resident from the handle's first append (expann_graph_adopt_build_state), in the
// types of graph_builder_state.hpp: `arrays`, the fixed-stride rows of a BuildGraph sized to GraphRows::cap_rows, with
// upper-layer capacities of their own ([L_cap][U_cap], laid out again when the upper vertices or the layers outgrow
// them); `scratch`, a batch's; `cfg`, the parameters it was adopted with.  BuildGraph::vec is d_vectors: the rows are
// not kept twice.  The CSR and d_adj0 are remade from it after every append and remove (graph_append.hpp).
struct GraphBuildState {
	bool resident = false;
	BuildConfig cfg;
	BuilderArrays arrays;
	BuildScratch scratch;
	size_t U = 0;                         // upper-layer vertices
	size_t edge_cap = 0, off_cap = 0;     // words of d_neighbours / d_layer_off
	size_t tiles_cap = 0;
	DevPtr<uint32_t> d_tile_sums; // [tiles_cap] the scan's tile sums
	OwnedEvent ev_tables[2];      // around the last rebuild of the walk's tables
	uint64_t tables_ns = 0, n_edges = 0;  // its device time; the edges of the CSR it made
};

// row filter (expann_graph_set_row_filter): the handle's copy of the bitmap, zero from n on, and the allowed
// vertices as an ascending list (what the scan of a sparse filter reads), both made at set time
struct GraphRowFilter {
	DevPtr<uint32_t> d_allow;       // [ceil(n / 32)]
	DevPtr<uint32_t> d_allow_list;  // [n_allowed]
	bool filter_on = false;
	uint32_t n_allowed = 0;
};

// row groups (expann_graph_set_row_groups): every row's label, and the directory made on the host at set time -- the
// distinct labels ascending (0xFFFFFFFF left out), their offsets, and each group's rows ascending
struct GraphRowGroups {
	DevPtr<uint32_t> d_row_groups;  // [n]
	DevPtr<uint32_t> d_group_keys;  // [n_groups]
	DevPtr<uint32_t> d_group_off;   // [n_groups + 1]
	DevPtr<uint32_t> d_group_rows;  // [rows that carry a label other than 0xFFFFFFFF]
	bool groups_on = false;
	uint32_t n_groups = 0;
};

// the counters behind expann_graph_get_stat (kGraphStatTable)
struct GraphStats {
	uint64_t stat_flat = 0;  // searches answered without a walk
	// queries of grouped searches by how they were served {walk, scan, pad}: counted in words 5..7 of a search's
	// counter slot, folded in when the search is checked
	uint64_t stat_group[3] = {0, 0, 0};
	uint64_t stat_redo_queries = 0, stat_redo_overflows = 0, stat_deferred = 0, stat_distcomps = 0;
	uint64_t stat_range = 0;  // range searches since create, from either entry point
	double stat_redo_ms = 0;
	// appends and removes (device / host: the route that served the call; reallocs: capacity growths; touched,
	// truncated: rows).  The host route re-uploads the graph into a new handle and carries these over as arrays
	// (expann_graph_note_host_append / _remove), in the order of the fields.
	struct Appends { uint64_t calls = 0, rows = 0, batches = 0, device = 0, host = 0, reallocs = 0; } stat_append;
	struct Removes { uint64_t calls = 0, rows = 0, touched = 0, truncated = 0, device = 0, host = 0; } stat_remove;
	uint64_t remove_repair_ns = 0;  // the device time of the last remove's touch + gather + prune
};

// the handle's own stream, the host-buffer calls' events, launch plans, statistics, the last error
struct GraphRuntime : GraphStats {
	OwnedStream stream;
	OwnedEvent ev0, ev1;
	OwnedEvent ev2;  // behind the redo launch of a host-buffer grouped search (made at the first one)
	double last_ms = 0;
	// attribute, occupancy and grid of a launch, per (instance, LDS size)
	struct LaunchPlan {
		const void* fn;
		size_t lds;
		uint32_t resident;
	};
	std::vector<LaunchPlan> plans;
	mutable std::string err;
};

// (base order: the stream and its events outlive every buffer when a handle is deleted)
struct expann_graph : GraphOptions, GraphRuntime, GraphRows, GraphBuildState, GraphRowBytes, GraphVisited,
                      GraphDeviceSearches, GraphRowFilter, GraphRowGroups {
	template <typename Group> void forget() { static_cast<Group&>(*this) = Group{}; }
	int fail(int code, const std::string& msg) const {
		err = msg;
		return code;
	}
};

namespace {
using GraphFn = void (*)(GraphSearchParams);
struct GraphVariant {
	int d;
	int mode;       // expann_graph_compression
	int filtered;   // kFilterNone, kFilterBitmap (THE FILTER RULE, graph_search.hpp), kFilterGroups (THE GROUP RULE) or
	                // kFilterRange (THE RANGE WALK RULE)
	bool f16;       // the instance over binary16 rows (TR = _Float16)
	GraphFn fn;
};
#define GRAPH_VF(D, F)                                                                 \
	{D, kGraphF32, F, false, graph_search_kernel<D, kGraphF32, 0, F>},                 \
	{D, kGraphU8Cast, F, false, graph_search_kernel<D, kGraphU8Cast, 0, F>},           \
	{D, kGraphRangedQ8, F, false, graph_search_kernel<D, kGraphRangedQ8, 0, F>}
#define GRAPH_V(D) GRAPH_VF(D, kFilterNone), GRAPH_VF(D, kFilterBitmap)
// binary16 rows: the run-time-dim instances serve every dim and mode; d = 128 has compiled instances as well
#define GRAPH_HF(D, MODE, F) {D, MODE, F, true, graph_search_kernel<D, MODE, 0, F, _Float16>}
#define GRAPH_H(D, MODE) GRAPH_HF(D, MODE, kFilterNone), GRAPH_HF(D, MODE, kFilterBitmap)
#define GRAPH_R(D) {D, kGraphF32, kFilterRange, false, graph_search_kernel<D, kGraphF32, 0, kFilterRange>}
const GraphVariant kGraph[] = {GRAPH_V(64),  GRAPH_V(128), GRAPH_V(256), GRAPH_V(512),
                               GRAPH_V(768), GRAPH_V(832), GRAPH_V(960), GRAPH_V(0),
                               GRAPH_H(128, kGraphF32), GRAPH_H(128, kGraphU8Cast), GRAPH_H(128, kGraphRangedQ8),
                               GRAPH_H(0, kGraphF32), GRAPH_H(0, kGraphU8Cast), GRAPH_H(0, kGraphRangedQ8),
                               // row groups: d = 128 and the run-time-dim instance, as for binary16 rows
                               GRAPH_VF(128, kFilterGroups), GRAPH_VF(0, kFilterGroups),
                               GRAPH_HF(128, kGraphF32, kFilterGroups), GRAPH_HF(128, kGraphU8Cast, kFilterGroups),
                               GRAPH_HF(128, kGraphRangedQ8, kFilterGroups), GRAPH_HF(0, kGraphF32, kFilterGroups),
                               GRAPH_HF(0, kGraphU8Cast, kFilterGroups), GRAPH_HF(0, kGraphRangedQ8, kFilterGroups),
                               // the range walk: fp32 bottom layer only, every compiled dim and the run-time-dim instance;
                               // binary16 rows as above
                               GRAPH_R(64), GRAPH_R(128), GRAPH_R(256), GRAPH_R(512), GRAPH_R(768), GRAPH_R(832),
                               GRAPH_R(960), GRAPH_R(0), GRAPH_HF(128, kGraphF32, kFilterRange),
                               GRAPH_HF(0, kGraphF32, kFilterRange)};
#undef GRAPH_R
#undef GRAPH_H
#undef GRAPH_HF
#undef GRAPH_V
#undef GRAPH_VF
// quantizer_simple<uint8_t> of n_values floats: launches of at most 2^30 values (a dispatch's grid is
// counted in 32-bit work-items: 1.05 M rows x 4096 in one launch would wrap)
// (TS: float, or _Float16 for the rows of an expann_graph_create_f16 handle)
template <typename TS>
void launch_quantize_simple_u8(const TS* in, size_t n_values, uint8_t* out, hipStream_t st) {
	const size_t chunk = size_t(1) << 30;
	for (size_t off = 0; off < n_values; off += chunk) {
		const size_t nv = std::min(chunk, n_values - off);
		hipLaunchKernelGGL(quantize_simple_u8_kernel<TS>, dim3((uint32_t)((nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   in + off, nv, out + off);
	}
}
// the compiled instance of `dim`, else the run-time-dim one (d = 0)
const GraphVariant* graph_variant(int dim, int mode, int filtered, bool f16) {
	const GraphVariant* any = nullptr;
	for (const auto& v : kGraph)
		if (v.mode == mode && v.filtered == filtered && v.f16 == f16) {
			if (v.d == dim)
				return &v;
			if (v.d == 0)
				any = &v;
		}
	return any;
}
// the dims the graph path takes (checked before any device lookup): a multiple of 16 up to 4096;
// returns EXPANN_OK or the error, with its message in g_create_error
int graph_dim_error(const char* fn, int dim) {
	if (dim <= 0 || dim % 16 != 0) {
		g_create_error = std::string(fn) + ": dim must be a positive multiple of 16";
		return EXPANN_ERR_INVALID_ARG;
	}
	if ((uint32_t)dim > kGraphMaxAnyDim) {
		g_create_error = std::string(fn) + ": dim " + std::to_string(dim) + " exceeds the graph path's limit of 4096";
		return EXPANN_ERR_UNSUPPORTED;
	}
	return EXPANN_OK;
}
// the instrumented instance (EXPANN_GRAPH_STAMPS=1, d = 128): per-phase shader clocks of a hop
const GraphVariant kGraphDbg[] = {{128, kGraphF32, kFilterNone, false, graph_search_kernel<128, kGraphF32, 1>},
                                  {128, kGraphU8Cast, kFilterNone, false, graph_search_kernel<128, kGraphU8Cast, 1>},
                                  {128, kGraphRangedQ8, kFilterNone, false, graph_search_kernel<128, kGraphRangedQ8, 1>}};
// the same over binary16 rows (fp32 walk only)
const GraphVariant kGraphDbgF16 = {128, kGraphF32, kFilterNone, true, graph_search_kernel<128, kGraphF32, 1, kFilterNone, _Float16>};
const char* const kGraphModeName[] = {"f32", "u8", "q8"};

// min / max of n_values floats, then their quantizer_ranged_q8 bytes and scale_factor / offset (quantize.hpp);
// d_minmax[2] is scratch.  Launches of at most 2^30 values, as launch_quantize_simple_u8.
template <typename TS>
hipError_t launch_quantize_ranged_q8(const TS* in, size_t n_values, uint32_t* d_minmax, int8_t* out,
                                     float* d_scale_offset, hipStream_t st) {
	// min starts at FLT_MAX, max at FLT_MIN (smallest positive normal): src/quantizer.h:217-218
	const uint32_t init[2] = {float_to_ordered(3.402823466e+38f), float_to_ordered(1.175494351e-38f)};
	hipError_t e = hipMemcpyAsync(d_minmax, init, sizeof(init), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);  // `init` is a stack buffer
	if (e != hipSuccess)
		return e;
	const uint32_t blocks = (uint32_t)std::min<size_t>((n_values + kBlock - 1) / kBlock, 4096);
	hipLaunchKernelGGL(minmax_f32_kernel<TS>, dim3(blocks), dim3(kBlock), 0, st, in, n_values, d_minmax);
	const size_t chunk = size_t(1) << 30;
	for (size_t off = 0; off < n_values; off += chunk) {
		const size_t nv = std::min(chunk, n_values - off);
		hipLaunchKernelGGL(quantize_ranged_q8_kernel<TS>, dim3((uint32_t)((nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
		                   in + off, nv, (const uint32_t*)d_minmax, out + off, d_scale_offset);
	}
	e = hipGetLastError();
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	return e;
}

// the ranged mode's copy of the rows and its quantiser, made at first use (EXPANN_OK, or the error on g)
int graph_ensure_ranged(expann_graph* g) {
	const char* unusable = "the ranged quantiser is unusable on these rows: scale_factor is not finite and positive "
	                       "(all components equal?)";
	if (g->ranged_state < 0)
		return g->fail(EXPANN_ERR_INVALID_ARG, unusable);
	if (g->ranged_state > 0)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	const size_t nv = g->n * (size_t)g->dim;
	DevBuf b_mm, b_so;
	DevPtr<uint8_t> b_rows;  // built aside: the handle takes it when the quantiser is usable
	HIP_TRY(g, b_mm.alloc(2 * sizeof(uint32_t)));
	HIP_TRY(g, b_so.alloc(2 * sizeof(float)));
	HIP_TRY(g, hipMalloc(&b_rows, nv));
	HIP_TRY(g, g->rows_f16 ? launch_quantize_ranged_q8(g->d_vectors.as<const _Float16>(), nv, b_mm.as<uint32_t>(),
	                                                   b_rows.as<int8_t>(), b_so.as<float>(), g->stream)
	                       : launch_quantize_ranged_q8(g->d_vectors.as<const float>(), nv, b_mm.as<uint32_t>(),
	                                                   b_rows.as<int8_t>(), b_so.as<float>(), g->stream));
	float so[2] = {0, 0};
	HIP_TRY(g, hipMemcpy(so, b_so.p, sizeof(so), hipMemcpyDeviceToHost));
	if (!std::isfinite(so[0]) || !(so[0] > 0.0f) || !std::isfinite(so[1])) {
		g->ranged_state = -1;  // (the copy is dropped with b_rows)
		return g->fail(EXPANN_ERR_INVALID_ARG, unusable);
	}
	g->d_ranged = std::move(b_rows);
	g->ranged_scale = so[0];
	g->ranged_offset = so[1];
	g->ranged_state = 1;
	return EXPANN_OK;
}

constexpr size_t kGraphMaxLds = 160 * 1024;     // the working set a search may take of a CU's LDS
constexpr uint32_t kGraphMaxOutstanding = 256;  // device-buffer searches between two drains
constexpr uint32_t kGraphCtrWords = 8;          // counter words per search
// "filter_flat_rows" on auto: a filter that allows at most this many rows is scanned, not walked.  The largest
// measured count at which the scan still beats the walk or the walk still overflows, on the C4 graph (DESIGN 4.9f,
// profiles/graph_filter_ab.txt: at 128 000 rows the scan takes 49 ms against the walk's 110 ms, at 256 000 rows
// 125 ms against 42 ms; the walk overflows its redo capacity up to 32 000 rows).
constexpr uint32_t kGraphFlatRowsAuto = 128000;
// (kGraphFlatMaxKeys, the min(k, allowed) the scan keeps in LDS, is graph_search.hpp's: the group kernels decide by it)

// the argument checks of a search, a NULL handle first, in the order the header documents, all before the device is
// touched; *empty: m == 0, nothing to do
int graph_search_args(expann_graph* g, const void* queries, size_t m, size_t k, size_t ef_search, int mode,
                      const void* ids, const void* dists, bool* empty) {
	*empty = false;
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (mode < EXPANN_GRAPH_FP32 || mode > EXPANN_GRAPH_RANGED_Q8)
		return g->fail(EXPANN_ERR_INVALID_ARG, "mode must be 0 (fp32), 1 (uint8 cast) or 2 (ranged int8)");
	if (k == 0 || ef_search == 0)
		return g->fail(EXPANN_ERR_INVALID_ARG, "k == 0 or ef_search == 0");
	if (m == 0) {
		*empty = true;
		return EXPANN_OK;
	}
	if (!queries || !ids || !dists)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	if (ef_search > 4096)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "ef_search > 4096");
	if (mode != EXPANN_GRAPH_FP32 && g->dim % 64 != 0)  // (the reference's dist2_compressed works in 64-dim blocks)
		return g->fail(EXPANN_ERR_UNSUPPORTED, mode == EXPANN_GRAPH_RANGED_Q8
		                                           ? "the ranged int8 walk needs dim % 64 == 0"
		                                           : "the uint8 walk (use_compression) needs dim % 64 == 0");
	return EXPANN_OK;
}

// the heap capacity a search starts with
uint32_t graph_first_cand_cap(size_t ef_search) {
	uint32_t cand_cap = 256;
	while (cand_cap < 16 * ef_search && cand_cap < 8192)
		cand_cap *= 2;
	return cand_cap;
}

// everything of a launch's parameters that the handle, the mode and (k, ef) decide; the caller adds the
// queries, the outputs, cand_cap and the counters
GraphSearchParams graph_base_params(const expann_graph* g, int mode, size_t k, size_t ef_search) {
	GraphSearchParams p{};
	p.vectors = g->d_vectors.as<const float>();  // (rows_f16: halves, read by the _Float16 instances only)
	p.compressed = mode == EXPANN_GRAPH_RANGED_Q8 ? g->d_ranged : g->d_compressed;
	p.q_scale = g->ranged_scale;
	p.q_offset = g->ranged_offset;
	p.layer_off = g->d_layer_off;
	p.neighbours = g->d_neighbours;
	p.adj0 = g->d_adj0;
	p.stride0 = g->stride0;
	p.n = (uint32_t)g->n;
	p.n_layers = g->n_layers;
	p.starting_vertex = g->starting_vertex;
	p.k = (uint32_t)k;
	p.ef = (uint32_t)ef_search;
	p.near_cap = p.ef;  // (the range walk's is larger: graph_enqueue_range)
	p.max_degree = g->max_degree0;
	p.list_cap = std::max<uint32_t>(std::max<uint32_t>(g->stride0, (uint32_t)ef_search), 4);
	p.visited = g->d_visited;
	p.vis_bits = g->d_visited.as<uint32_t>();
	p.vis_words = g->vis_words;
	p.epochs = g->d_epochs;
	p.dim = (uint32_t)g->dim;
	p.allow_bits = g->filter_on ? g->d_allow.get() : nullptr;
	if (const char* e = std::getenv("EXPANN_GRAPH_DEBUG"))
		p.debug = (uint32_t)std::atol(e);
	return p;
}

// dynamic LDS of a launch: the two heaps, a hop's list, and -- run-time-dim instance -- the query (and its bytes)
size_t graph_lds_bytes(const GraphSearchParams& p, uint32_t cand_cap, bool run_time_dim, bool use_compression) {
	size_t lds = sizeof(md_pair) * ((size_t)p.near_cap + 1 + cand_cap + 1) + (sizeof(uint32_t) + sizeof(float)) * p.list_cap;
	if (run_time_dim)
		lds += (size_t)p.dim * (sizeof(float) + (use_compression ? 1 : 0));
	return lds;
}

// host wait for the device-buffer searches still in flight (their counters stay where they are)
hipError_t graph_wait_outstanding(expann_graph* g) {
	return g->dev_outstanding ? hipStreamSynchronize(g->dev_stream) : hipSuccess;
}

// wait for the outstanding device-buffer searches and collect their counters for the next sync
int graph_drain(expann_graph* g) {
	if (!g->dev_outstanding)
		return EXPANN_OK;
	HIP_TRY(g, hipStreamSynchronize(g->dev_stream));
	HIP_TRY(g, hipMemcpy(g->h_dev_ctr, g->d_dev_ctr, sizeof(uint32_t) * kGraphCtrWords * g->dev_outstanding,
	                     hipMemcpyDeviceToHost));
	HIP_TRY(g, hipMemcpy(g->h_dc_total, g->d_dc_total, sizeof(unsigned long long), hipMemcpyDeviceToHost));
	for (uint32_t s = 0; s < g->dev_outstanding; ++s) {
		const uint32_t* c = g->h_dev_ctr + (size_t)s * kGraphCtrWords;
		g->pend_overflows += c[0] != 0;
		g->pend_redo_queries += c[2];
		for (int j = 0; j < 3; ++j)  // (zero after any search but a grouped one)
			g->stat_group[j] += c[5 + j];
	}
	g->stat_distcomps = *g->h_dc_total;
	g->dev_outstanding = 0;
	return EXPANN_OK;
}

// counter slots, their pinned mirror, and the events and distcomps total of the device-buffer searches, made at
// the handle's first search
int graph_dev_init(expann_graph* g) {
	if (g->d_dev_ctr)
		return EXPANN_OK;
	for (OwnedEvent& ev : g->ev_dev)
		if (!ev)
			HIP_TRY(g, hipEventCreate(&ev));
	if (!g->h_dev_ctr)
		HIP_TRY(g, hipHostMalloc((void**)&g->h_dev_ctr, sizeof(uint32_t) * kGraphCtrWords * (kGraphMaxOutstanding + 1)));
	if (!g->h_dc_total)
		HIP_TRY(g, hipHostMalloc((void**)&g->h_dc_total, sizeof(unsigned long long)));
	if (!g->d_dc_total) {
		HIP_TRY(g, hipMalloc(&g->d_dc_total, sizeof(unsigned long long)));
		HIP_TRY(g, hipMemset(g->d_dc_total, 0, sizeof(unsigned long long)));
	}
	HIP_TRY(g, hipMalloc(&g->d_dev_ctr, sizeof(uint32_t) * kGraphCtrWords * (kGraphMaxOutstanding + 1)));
	return EXPANN_OK;
}

// workgroups of `fn` resident at once with `lds` bytes each; the attribute and the occupancy query run once per
// (instance, LDS size) and handle.  The attribute is set to the largest working set a search may have, so that
// plans of one instance do not undo each other's.
int graph_plan(expann_graph* g, const void* fn, size_t lds, uint32_t* resident) {
	for (const auto& pl : g->plans)
		if (pl.fn == fn && pl.lds == lds) {
			*resident = pl.resident;
			return EXPANN_OK;
		}
	HIP_TRY(g, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGraphMaxLds));
	int per_cu = 0;
	HIP_TRY(g, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, lds));
	*resident = (uint32_t)std::max(1, per_cu) * (uint32_t)num_cus(g->device);
	g->plans.push_back({fn, lds, *resident});
	return EXPANN_OK;
}

// the byte copy of the rows that `mode` walks, made at its first use on the handle's own stream and complete on
// return, on whichever stream the walk then runs (EXPANN_OK, or the error on g)
int graph_ensure_bytes(expann_graph* g, int mode) {
	if (mode == EXPANN_GRAPH_RANGED_Q8)  // quantizer_ranged_q8::build, src/quantizer.h:213-232
		return graph_ensure_ranged(g);
	if (mode == EXPANN_GRAPH_U8_CAST && !g->d_compressed) {  // quantizer_simple<uint8_t>::build, :485-486
		HIP_TRY(g, hipMalloc(&g->d_compressed, g->n * (size_t)g->dim));
		if (g->rows_f16)
			launch_quantize_simple_u8(g->d_vectors.as<const _Float16>(), g->n * (size_t)g->dim, g->d_compressed, g->stream);
		else
			launch_quantize_simple_u8(g->d_vectors.as<const float>(), g->n * (size_t)g->dim, g->d_compressed, g->stream);
		HIP_TRY(g, hipGetLastError());
		HIP_TRY(g, hipStreamSynchronize(g->stream));
	}
	return EXPANN_OK;
}

// A search, planned: the walk of all queries at the first heap capacity, and the REDO launch that walks the
// queries whose candidates heap overflowed again at a larger one and overwrites their rows.
struct GraphSearchPlan {
	GraphFn fn = nullptr;
	GraphSearchParams first{}, redo{};
	size_t lds = 0, lds_redo = 0;
	uint32_t grid = 0, grid_redo = 0;
	bool has_redo = false;  // false: no larger capacity to go to, an overflow of the first launch is final
};

// Plans the search whose queries, outputs (and distcomps total / stamps) `p` names, with the counter slot `ctr`:
// capacities, working sets, grids and both launches' parameters.  Enqueues nothing, except that growing the redo
// list first waits for the searches that may still use it.
int graph_search_plan(expann_graph* g, const GraphVariant* gv, GraphSearchParams p, uint32_t* ctr, GraphSearchPlan* pl) {
	const bool any_dim = gv->d == 0, use_compression = gv->mode != EXPANN_GRAPH_FP32;
	const uint32_t cand_cap = g->opt_cand_cap ? (uint32_t)g->opt_cand_cap : graph_first_cand_cap(p.ef);
	pl->fn = gv->fn;
	pl->lds = graph_lds_bytes(p, cand_cap, any_dim, use_compression);
	if (pl->lds > kGraphMaxLds)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "graph search working set exceeds LDS");
	// the redo launch's heap: the largest power of two up to 8192 whose working set fits
	uint32_t redo_cap = (uint32_t)g->opt_redo_cap;
	if (!redo_cap)
		for (redo_cap = 8192; redo_cap > cand_cap && graph_lds_bytes(p, redo_cap, any_dim, use_compression) > kGraphMaxLds;)
			redo_cap /= 2;
	pl->has_redo = redo_cap > cand_cap;
	pl->lds_redo = pl->has_redo ? graph_lds_bytes(p, redo_cap, any_dim, use_compression) : 0;
	if (pl->lds_redo > kGraphMaxLds)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "graph search: the working set at \"redo_capacity\" exceeds LDS");
	// as many workgroups as are resident at once (registers and LDS of this instance), each with a visited array
	// of its own; they pull queries from a counter
	uint32_t resident = 0;
	if (int rc = graph_plan(g, (const void*)gv->fn, pl->lds, &resident))
		return rc;
	pl->grid = (uint32_t)std::min<size_t>(p.m, std::min<uint32_t>(g->slots, resident));
	p.cand_cap = cand_cap;
	p.error = ctr;
	p.next_query = ctr + 1;
	pl->first = p;
	if (!pl->has_redo)
		return EXPANN_OK;
	if (int rc = graph_plan(g, (const void*)gv->fn, pl->lds_redo, &resident))
		return rc;
	// sized without knowing how many queries overflowed: the workgroups that find the list empty leave after one atomic
	pl->grid_redo = (uint32_t)std::min<size_t>(p.m, std::min<uint32_t>(g->slots, resident));
	if (sizeof(uint32_t) * p.m > g->d_redo_list.bytes || !g->d_redo_list) {  // (a grow frees the list in use)
		HIP_TRY(g, graph_wait_outstanding(g));
		HIP_TRY(g, g->d_redo_list.ensure(sizeof(uint32_t) * p.m));
	}
	pl->first.redo_list = g->d_redo_list;
	pl->first.redo_count = ctr + 2;
	pl->redo = p;  // (no redo list: an overflow here raises the error flag)
	pl->redo.cand_cap = redo_cap;
	pl->redo.query_map = g->d_redo_list;
	pl->redo.m_dev = ctr + 2;
	pl->redo.next_query = ctr + 3;
	return EXPANN_OK;
}

// the reset of the search's counter slot and its first launch on `st`, between two events
int graph_enqueue_first(expann_graph* g, const GraphSearchPlan& pl, hipStream_t st, hipEvent_t before, hipEvent_t after) {
	HIP_TRY(g, hipMemsetAsync(pl.first.error, 0, sizeof(uint32_t) * kGraphCtrWords, st));
	HIP_TRY(g, hipEventRecord(before, st));
	hipLaunchKernelGGL(pl.fn, dim3(pl.grid), dim3(64), pl.lds, st, pl.first);
	HIP_TRY(g, hipEventRecord(after, st));
	HIP_TRY(g, hipGetLastError());
	return EXPANN_OK;
}

// the redo launch (pl.has_redo) on `st`, behind the first one, and the event after it
int graph_enqueue_redo(expann_graph* g, const GraphSearchPlan& pl, hipStream_t st, hipEvent_t after) {
	hipLaunchKernelGGL(pl.fn, dim3(pl.grid_redo), dim3(64), pl.lds_redo, st, pl.redo);
	HIP_TRY(g, hipEventRecord(after, st));
	HIP_TRY(g, hipGetLastError());
	return EXPANN_OK;
}

// ---- searches under a row filter that do not walk ---------------------------------------------
// how a search of k neighbours is served under the filter in force: by the walk (no filter, or a dense one), by the
// exact scan of the allowed rows (at most "filter_flat_rows" of them), or -- no row allowed -- by padding alone
enum GraphServe { kServeWalk, kServeScan, kServePad };
GraphServe graph_serve(const expann_graph* g, size_t k) {
	if (!g->filter_on)
		return kServeWalk;
	if (g->n_allowed == 0)
		return kServePad;
	const uint32_t flat_rows = g->opt_flat_rows ? (uint32_t)std::min<long>(g->opt_flat_rows, 0x7FFFFFFFL) : kGraphFlatRowsAuto;
	const size_t kk = std::min<size_t>(k, g->n_allowed);
	if (g->n_allowed > flat_rows || kk > kGraphFlatMaxKeys || graph_flat_lds_bytes((uint32_t)kk, (uint32_t)g->dim) > kGraphMaxLds)
		return kServeWalk;
	return kServeScan;
}

// what an exact scan takes from the parameters `w` of the walk it stands in for -- the rows, the queries, the
// outputs, the distcomps total -- with the keys it keeps in LDS and its query counter
GraphFlatParams graph_flat_params(const GraphSearchParams& w, uint32_t kk, uint32_t* next_query) {
	GraphFlatParams f{};
	f.vectors = w.vectors;
	f.dim = w.dim;
	f.queries = w.queries;
	f.m = w.m;
	f.k = w.k;
	f.kk = kk;
	f.out_ids = w.out_ids;
	f.out_dists = w.out_dists;
	f.out_distcomps = w.out_distcomps;
	f.next_query = next_query;
	f.distcomps_total = w.distcomps_total;
	return f;
}

// the scan of the allowed rows for the search whose queries and outputs `w` names (a walk's parameters: the scan
// takes what it shares with them), with the counter slot `ctr`, on `st` between two events
int graph_enqueue_flat(expann_graph* g, const GraphSearchParams& w, uint32_t* ctr, hipStream_t st, hipEvent_t before,
                       hipEvent_t after) {
	GraphFlatParams f = graph_flat_params(w, std::min<uint32_t>(w.k, g->n_allowed), ctr + 1);
	f.list = g->d_allow_list;
	f.n_list = g->n_allowed;
	const size_t lds = graph_flat_lds_bytes(f.kk, f.dim);
	uint32_t resident = 0;
	void (*const scan)(GraphFlatParams) = g->rows_f16 ? graph_flat_scan_kernel<_Float16> : graph_flat_scan_kernel<float>;
	if (int rc = graph_plan(g, (const void*)scan, lds, &resident))
		return rc;
	HIP_TRY(g, hipMemsetAsync(ctr, 0, sizeof(uint32_t) * kGraphCtrWords, st));
	HIP_TRY(g, hipEventRecord(before, st));
	hipLaunchKernelGGL(scan, dim3((uint32_t)std::min<size_t>(w.m, resident)), dim3(64), lds, st, f);
	HIP_TRY(g, hipEventRecord(after, st));
	HIP_TRY(g, hipGetLastError());
	++g->stat_flat;
	return EXPANN_OK;
}

// a filter that allows no row, device buffers: padding and distcomps 0 in the order of `st`
int graph_enqueue_pad(expann_graph* g, const GraphSearchParams& w, uint32_t* ctr, hipStream_t st) {
	const size_t cells = (size_t)w.m * w.k;
	HIP_TRY(g, hipMemsetAsync(ctr, 0, sizeof(uint32_t) * kGraphCtrWords, st));
	hipLaunchKernelGGL(fill_pad_kernel, dim3((uint32_t)std::min<size_t>((cells + kBlock - 1) / kBlock, 1024)), dim3(kBlock), 0,
	                   st, w.out_ids, w.out_dists, cells);
	HIP_TRY(g, hipGetLastError());
	if (w.out_distcomps)
		HIP_TRY(g, hipMemsetAsync(w.out_distcomps, 0, sizeof(uint32_t) * w.m, st));
	++g->stat_flat;
	return EXPANN_OK;
}

// bits: n_words words in host (on_device = false) or device memory, read in the order of `user_st` (nullptr = the
// handle's own stream).  The new copy and list are made aside and put in place when complete: a failed call
// leaves the filter as it was.
int graph_set_row_filter(expann_graph* g, const uint32_t* bits, size_t n_words, bool on_device, hipStream_t user_st) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!bits)
		return g->fail(EXPANN_ERR_INVALID_ARG, "row filter: NULL bits");
	const size_t need_words = (g->n + 31) / 32;
	if (n_words < need_words)
		return g->fail(EXPANN_ERR_INVALID_ARG, "row filter: " + std::to_string(n_words) + " words for " +
		                                           std::to_string(g->n) + " rows (need " + std::to_string(need_words) + ")");
	HIP_TRY(g, hipSetDevice(g->device));
	// searches in flight still read the old filter: they are waited for (their counters stay for the next sync)
	HIP_TRY(g, graph_wait_outstanding(g));
	hipStream_t st = user_st ? user_st : g->stream;
	GraphRowFilter f;
	DevPtr<uint32_t> b_stat;
	HIP_TRY(g, hipMalloc(&f.d_allow, sizeof(uint32_t) * need_words));
	HIP_TRY(g, hipMalloc(&b_stat, sizeof(uint32_t) * (2 + kFilterSegs)));
	HIP_TRY(g, hipMemcpyAsync(f.d_allow, bits, sizeof(uint32_t) * need_words,
	                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
	HIP_TRY(g, hipMemsetAsync(b_stat, 0, sizeof(uint32_t) * (2 + kFilterSegs), st));
	hipLaunchKernelGGL(filter_count_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, f.d_allow.get(), (uint32_t)g->n,
	                   (uint32_t)need_words, b_stat.get(), b_stat.get() + 2);
	HIP_TRY(g, hipGetLastError());
	uint32_t stat[2] = {0, 0};
	HIP_TRY(g, hipMemcpyAsync(stat, b_stat, sizeof(stat), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipStreamSynchronize(st));  // walk or scan is chosen on the host: one wait per filter change
	f.n_allowed = stat[0];
	if (f.n_allowed) {
		HIP_TRY(g, hipMalloc(&f.d_allow_list, sizeof(uint32_t) * f.n_allowed));
		hipLaunchKernelGGL(filter_compact_kernel, dim3(kFilterSegs), dim3(kBlock), 0, st, (const uint32_t*)f.d_allow.get(),
		                   (uint32_t)need_words, (const uint32_t*)b_stat.get() + 2, 1u, f.d_allow_list.get(), f.n_allowed);
		HIP_TRY(g, hipGetLastError());
		HIP_TRY(g, hipStreamSynchronize(st));
	}
	if (st != g->stream)
		HIP_TRY(g, hipStreamSynchronize(g->stream));
	f.filter_on = true;
	static_cast<GraphRowFilter&>(*g) = std::move(f);  // (the old filter goes with the local)
	return EXPANN_OK;
}

// ---- row groups (THE GROUP RULE) ---------------------------------------------------------------
// groups: n labels in host (on_device = false) or device memory, read in the order of `user_st` (nullptr = the
// handle's own stream).  The directory is made on the host with a stable sort by label -- set time is no hot path --
// and everything is built aside and swapped in when complete: a failed call leaves the groups as they were.
int graph_set_row_groups(expann_graph* g, const uint32_t* groups, size_t n, bool on_device, hipStream_t user_st) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!groups)
		return g->fail(EXPANN_ERR_INVALID_ARG, "row groups: NULL labels");
	if (n != g->n)
		return g->fail(EXPANN_ERR_INVALID_ARG, "row groups: " + std::to_string(n) + " labels for " + std::to_string(g->n) + " rows");
	HIP_TRY(g, hipSetDevice(g->device));
	// searches in flight still read the old groups: they are waited for (their counters stay for the next sync)
	HIP_TRY(g, graph_wait_outstanding(g));
	hipStream_t st = user_st ? user_st : g->stream;
	std::vector<uint32_t> lab;
	if (int rc = fetch_group_labels(g, groups, n, on_device, st, lab))
		return rc;
	const GroupDirectory dir = build_group_directory(lab.data(), n);  // (host_common.hpp: shared with the brute-force index)
	const std::vector<uint32_t>&keys = dir.keys, &off = dir.off, &order = dir.rows;
	const size_t n_rows = dir.n_rows();
	GraphRowGroups b;
	HIP_TRY(g, hipMalloc(&b.d_row_groups, sizeof(uint32_t) * n));
	HIP_TRY(g, hipMalloc(&b.d_group_keys, sizeof(uint32_t) * std::max<size_t>(keys.size(), 1)));
	HIP_TRY(g, hipMalloc(&b.d_group_off, sizeof(uint32_t) * off.size()));
	HIP_TRY(g, hipMalloc(&b.d_group_rows, sizeof(uint32_t) * std::max<size_t>(n_rows, 1)));
	HIP_TRY(g, hipMemcpy(b.d_row_groups, lab.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
	if (!keys.empty())
		HIP_TRY(g, hipMemcpy(b.d_group_keys, keys.data(), sizeof(uint32_t) * keys.size(), hipMemcpyHostToDevice));
	HIP_TRY(g, hipMemcpy(b.d_group_off, off.data(), sizeof(uint32_t) * off.size(), hipMemcpyHostToDevice));
	if (n_rows)
		HIP_TRY(g, hipMemcpy(b.d_group_rows, order.data(), sizeof(uint32_t) * n_rows, hipMemcpyHostToDevice));
	HIP_TRY(g, hipStreamSynchronize(g->stream));
	b.n_groups = (uint32_t)keys.size();
	b.groups_on = true;
	static_cast<GraphRowGroups&>(*g) = std::move(b);  // (the old groups go with the local)
	return EXPANN_OK;
}

// the checks of a grouped search behind graph_search_args, in the header's order, before the device is touched
int graph_grouped_args(expann_graph* g, const void* query_groups) {
	if (!query_groups)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL query_groups");
	if (!g->groups_on)
		return g->fail(EXPANN_ERR_NOT_BUILT, "grouped search: no row groups are set (expann_graph_set_row_groups)");
	if (g->filter_on)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "grouped search under a row filter: combining the bitmap with groups is not offered");
	return EXPANN_OK;
}

// A grouped search, enqueued on `st` with the counter slot `ctr` and nothing waited for: the slot's reset, the scan
// launch (the queries group_serve sends to it, and the padding of empty groups), the walk's first launch (the
// others) and its redo launch as graph_search_plan plans it.  (The scan goes first, not last: the launches are
// serialised on one stream and write disjoint rows, so the answer is the same; this way the two events around scan +
// first walk and the one behind the redo launch give expann_graph_last_kernel_ms the sum of all launches while
// "redo_kernel_ns" stays the redo launch alone, and the redo launch keeps its place right behind the walk.)  `p` names queries and outputs (graph_base_params
// after graph_ensure_bytes: the walk reads the mode's byte copy of the rows); events: before the
// launches, after scan + first walk, after the redo launch (when *has_redo).
int graph_enqueue_grouped(expann_graph* g, GraphSearchParams p, const uint32_t* d_query_groups, int mode, uint32_t* ctr,
                          hipStream_t st, hipEvent_t* ev, bool* has_redo) {
	const GraphVariant* gv = graph_variant(g->dim, mode, kFilterGroups, g->rows_f16);
	if (!gv)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "no graph kernel for this dim");
	p.allow_bits = nullptr;
	p.row_groups = g->d_row_groups;
	p.query_groups = d_query_groups;
	p.group_keys = g->d_group_keys;
	p.group_off = g->d_group_off;
	p.n_groups = g->n_groups;
	p.flat_rows = g->opt_flat_rows ? (uint32_t)std::min<long>(g->opt_flat_rows, 0x7FFFFFFFL) : kGraphFlatRowsAuto;
	p.group_walked = ctr + 5;
	GraphSearchPlan pl;
	if (int rc = graph_search_plan(g, gv, p, ctr, &pl))
		return rc;
	GraphGroupScanParams s{};
	s.f = graph_flat_params(p, std::min<uint32_t>(p.k, kGraphFlatMaxKeys), ctr + 4);
	s.query_groups = d_query_groups;
	s.group_keys = g->d_group_keys;
	s.group_off = g->d_group_off;
	s.group_rows = g->d_group_rows;
	s.n_groups = g->n_groups;
	s.flat_rows = p.flat_rows;
	s.scanned = ctr + 6;
	s.padded = ctr + 7;
	const size_t lds = graph_flat_lds_bytes(s.f.kk, s.f.dim);
	uint32_t resident = 0;
	void (*const scan)(GraphGroupScanParams) = g->rows_f16 ? graph_group_scan_kernel<_Float16> : graph_group_scan_kernel<float>;
	if (int rc = graph_plan(g, (const void*)scan, lds, &resident))
		return rc;
	HIP_TRY(g, hipMemsetAsync(ctr, 0, sizeof(uint32_t) * kGraphCtrWords, st));
	HIP_TRY(g, hipEventRecord(ev[0], st));
	hipLaunchKernelGGL(scan, dim3((uint32_t)std::min<size_t>(p.m, resident)), dim3(64), lds, st, s);
	hipLaunchKernelGGL(pl.fn, dim3(pl.grid), dim3(64), pl.lds, st, pl.first);
	HIP_TRY(g, hipEventRecord(ev[1], st));
	HIP_TRY(g, hipGetLastError());
	*has_redo = pl.has_redo;
	if (pl.has_redo)
		if (int rc = graph_enqueue_redo(g, pl, st, ev[2]))
			return rc;
	return EXPANN_OK;
}

// ---- range search (THE RANGE WALK RULE) -----------------------------------------------------------
// the argument checks of a range search, a NULL handle first, in the order the header documents, all before the device
// is touched; *empty: m == 0, nothing to do
int graph_range_args(expann_graph* g, const void* queries, const void* radii, size_t m, size_t max_results, size_t ef_search,
                     const void* ids, const void* counts, bool* empty) {
	*empty = false;
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (ef_search == 0)
		return g->fail(EXPANN_ERR_INVALID_ARG, "range search: ef_search == 0");
	if (m == 0) {
		*empty = true;
		return EXPANN_OK;
	}
	if (!queries || !radii || !counts || (!ids && max_results > 0))
		return g->fail(EXPANN_ERR_INVALID_ARG, "range search: NULL pointer");
	if (ef_search > 4096)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "range search: ef_search > 4096");
	if (max_results > 4096)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "range search: max_results > 4096");
	if (g->filter_on)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "range search under a row filter is not offered");
	return EXPANN_OK;
}

// A range search, enqueued on `st` with the counter slot `ctr` and nothing waited for: the slot's reset, the range
// walk's first launch and its redo launch as graph_search_plan plans it.  `p` names queries and outputs
// (graph_base_params at mode 0 with k = max_results); events: before the first launch, after it, after the redo launch
// (when *has_redo).
int graph_enqueue_range(expann_graph* g, GraphSearchParams p, const float* d_radii, uint32_t* d_counts, uint32_t* ctr,
                        hipStream_t st, hipEvent_t* ev, bool* has_redo) {
	const GraphVariant* gv = graph_variant(g->dim, EXPANN_GRAPH_FP32, kFilterRange, g->rows_f16);
	if (!gv)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "no graph kernel for this dim");
	p.allow_bits = nullptr;
	p.radii = d_radii;
	p.max_results = p.k;
	p.out_counts = d_counts;
	p.near_cap = std::max(p.ef, p.k);
	p.list_cap = std::max(p.list_cap, p.near_cap);  // (the drain writes the whole queue to the hop's list)
	GraphSearchPlan pl;
	if (int rc = graph_search_plan(g, gv, p, ctr, &pl))
		return rc;
	if (int rc = graph_enqueue_first(g, pl, st, ev[0], ev[1]))
		return rc;
	*has_redo = pl.has_redo;
	if (pl.has_redo)
		if (int rc = graph_enqueue_redo(g, pl, st, ev[2]))
			return rc;
	++g->stat_range;
	return EXPANN_OK;
}

// EXPANN_GRAPH_STAMPS: a launch's shader clocks, mean over the workgroups of its grid, per hop
int graph_print_stamps(expann_graph* g, int mode, size_t ef_search, float ms, uint32_t grid, size_t m, const void* d_stamps) {
	std::vector<unsigned long long> st(8 * (size_t)grid);
	HIP_TRY(g, hipMemcpy(st.data(), d_stamps, st.size() * 8, hipMemcpyDeviceToHost));
	double tot[8] = {0};
	for (uint32_t b = 0; b < grid; ++b)
		for (int i = 0; i < 8; ++i)
			tot[i] += (double)st[8 * (size_t)b + i];
	const double hops = tot[6] > 0 ? tot[6] : 1, all = tot[0] + tot[1] + tot[2] + tot[3] + tot[4] + tot[5];
	std::fprintf(stderr,
	             "graph_search<%d,%s> ef %zu: %.3f ms, %u workgroups, %.1f hops / query, %.1f queue insertions / hop; "
	             "shader clocks per hop: pop + broadcast %.0f, adjacency + visited %.0f, gathers + scoring %.0f, "
	             "serial queue update %.0f; per query: setup + descent %.0f, output %.0f; shares %.1f / %.1f / %.1f / "
	             "%.1f / %.1f / %.1f %%\n",
	             g->dim, kGraphModeName[mode], ef_search, ms, grid, tot[6] / (double)m, tot[7] / hops,
	             tot[1] / hops, tot[2] / hops, tot[3] / hops, tot[4] / hops, tot[0] / (double)m, tot[5] / (double)m,
	             100 * tot[1] / all, 100 * tot[2] / all, 100 * tot[3] / all, 100 * tot[4] / all, 100 * tot[0] / all,
	             100 * tot[5] / all);
	return EXPANN_OK;
}

// ---- the two forms of a search ------------------------------------------------------------------
// Device buffers: what every such search does before its launches.  The stream (NULL = the handle's own); the
// handle's first search makes the counter slots; one set of visited arrays, so searches overlap in stream order only
// -- a search on another stream than the outstanding ones waits for them, one that finds every slot taken drains them,
// and nothing else is waited for; the byte copy of the rows when the walk will read one (`bytes`; before the
// parameters: they name it); then the parameters with the caller's buffers and the distcomps total, and the slot.
struct GraphDevSearch {
	hipStream_t st = nullptr;
	uint32_t* ctr = nullptr;
	GraphSearchParams p{};
};
int graph_dev_begin(expann_graph* g, void* stream, int mode, bool bytes, const float* d_queries, size_t m, size_t k,
                    size_t ef_search, uint64_t* d_ids, float* d_dists, uint32_t* d_distcomps, GraphDevSearch* s) {
	hipStream_t st = stream ? (hipStream_t)stream : g->stream;
	if (int rc = graph_dev_init(g))
		return rc;
	if (g->dev_outstanding && st != g->dev_stream)
		HIP_TRY(g, graph_wait_outstanding(g));
	if (g->dev_outstanding >= kGraphMaxOutstanding)
		if (int rc = graph_drain(g))
			return rc;
	if (bytes)
		if (int rc = graph_ensure_bytes(g, mode))
			return rc;
	s->st = st;
	s->ctr = g->d_dev_ctr + (size_t)g->dev_outstanding * kGraphCtrWords;
	s->p = graph_base_params(g, mode, k, ef_search);
	s->p.queries = d_queries;
	s->p.m = (uint32_t)m;
	s->p.out_ids = d_ids;
	s->p.out_dists = d_dists;
	s->p.out_distcomps = d_distcomps;
	s->p.distcomps_total = g->d_dc_total;
	return EXPANN_OK;
}
// ... and after them: the search is outstanding on `st`, and the next sync reads its time from ev_dev (`timed`: [0]
// and [1] hold it; `timed_redo`: [2] its redo launch)
void graph_dev_commit(expann_graph* g, hipStream_t st, bool timed, bool timed_redo) {
	g->dev_stream = st;
	++g->dev_outstanding;
	++g->stat_deferred;
	g->dev_timed = timed;
	g->dev_timed_redo = timed_redo;
}

// Host buffers: the staging of one call on the handle's own stream -- device copies of the queries (and of their
// groups, or of their radii with the counts to come back) and of the result arrays, and the host-buffer calls' counter slot: the one behind those of the device-buffer
// searches, which stay as they are for the next sync.  The caller enqueues and waits between begin() and finish().
struct GraphHostStage {
	DevBuf b_q, b_qg, b_ids, b_d, b_dc, b_r, b_cnt;
	uint32_t *ctr = nullptr, *h_ctr = nullptr;
	size_t m = 0, k = 0;
	// allocates, uploads (query_groups == nullptr: there are none; radii != nullptr: a range search, b_r and b_cnt) and
	// points *p at the buffers
	int begin(expann_graph* g, const float* queries, const uint32_t* query_groups, size_t m_, size_t k_, GraphSearchParams* p,
	          const float* radii = nullptr) {
		m = m_;
		k = k_;
		hipStream_t st = g->stream;
		const size_t qb = m * (size_t)g->dim * sizeof(float);
		HIP_TRY(g, b_q.alloc(qb));
		if (query_groups)
			HIP_TRY(g, b_qg.alloc(sizeof(uint32_t) * m));
		HIP_TRY(g, b_ids.alloc(sizeof(uint64_t) * m * k));
		HIP_TRY(g, b_d.alloc(sizeof(float) * m * k));
		HIP_TRY(g, b_dc.alloc(sizeof(uint32_t) * m));
		HIP_TRY(g, hipMemcpyAsync(b_q.p, queries, qb, hipMemcpyHostToDevice, st));
		if (query_groups)
			HIP_TRY(g, hipMemcpyAsync(b_qg.p, query_groups, sizeof(uint32_t) * m, hipMemcpyHostToDevice, st));
		if (radii) {
			HIP_TRY(g, b_r.alloc(sizeof(float) * m));
			HIP_TRY(g, b_cnt.alloc(sizeof(uint32_t) * m));
			HIP_TRY(g, hipMemcpyAsync(b_r.p, radii, sizeof(float) * m, hipMemcpyHostToDevice, st));
		}
		p->queries = b_q.as<float>();
		p->m = (uint32_t)m;
		p->out_ids = b_ids.as<uint64_t>();
		p->out_dists = b_d.as<float>();
		p->out_distcomps = b_dc.as<uint32_t>();
		ctr = g->d_dev_ctr + (size_t)kGraphMaxOutstanding * kGraphCtrWords;
		h_ctr = g->h_dev_ctr + (size_t)kGraphMaxOutstanding * kGraphCtrWords;
		return EXPANN_OK;
	}
	// the slot read back behind what was enqueued, and the wait for all of it
	int read_slot(expann_graph* g) {
		hipStream_t st = g->stream;
		HIP_TRY(g, hipMemcpyAsync(h_ctr, ctr, sizeof(uint32_t) * kGraphCtrWords, hipMemcpyDeviceToHost, st));
		HIP_TRY(g, hipStreamSynchronize(st));
		return EXPANN_OK;
	}
	// the results into the caller's arrays (distcomps may be nullptr; a range search: its counts, and ids -- with no rows
	// to return -- and dists may be nullptr too)
	int copy_out(expann_graph* g, uint64_t* ids, float* dists, uint32_t* distcomps, uint32_t* counts = nullptr) {
		if (ids && m * k)
			HIP_TRY(g, hipMemcpy(ids, b_ids.p, sizeof(uint64_t) * m * k, hipMemcpyDeviceToHost));
		if (dists && m * k)
			HIP_TRY(g, hipMemcpy(dists, b_d.p, sizeof(float) * m * k, hipMemcpyDeviceToHost));
		if (distcomps)
			HIP_TRY(g, hipMemcpy(distcomps, b_dc.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
		if (counts)
			HIP_TRY(g, hipMemcpy(counts, b_cnt.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
		return EXPANN_OK;
	}
	// ... and what the slot (read_slot) says of the walks: an overflow that no redo launch served is the call's error
	int finish(expann_graph* g, uint64_t* ids, float* dists, uint32_t* distcomps, uint32_t* counts = nullptr) {
		if (int rc = copy_out(g, ids, dists, distcomps, counts))
			return rc;
		if (h_ctr[0])
			return g->fail(EXPANN_ERR_OVERFLOW, "graph search: candidates queue overflowed its LDS capacity");
		return EXPANN_OK;
	}
};
}  // namespace

struct GraphDeleter {
	void operator()(expann_graph* g) const { expann_graph_destroy(g); }
};
// expann_graph_create (elem_bytes = 4, `fn` its name) and expann_graph_create_f16 (2): one body, so both make the
// same checks in the same order, all before the device is touched
static int graph_create(const char* fn_name, size_t elem_bytes, int dim, int device, const void* vectors, size_t n,
                        uint32_t n_layers, uint32_t starting_vertex, const uint64_t* layer_offsets,
                        const uint32_t* neighbours, expann_graph** out) {
	const std::string fn(fn_name);
	if (!out) {
		g_create_error = "out == NULL";
		return EXPANN_ERR_INVALID_ARG;
	}
	*out = nullptr;
	if (int rc = graph_dim_error(fn_name, dim))
		return rc;
	if (!vectors || !layer_offsets || n == 0 || n_layers == 0 || starting_vertex >= n ||
	    n >= (1ull << 32) - 64 || (!neighbours && layer_offsets[(size_t)n_layers * (n + 1) - 1])) {
		g_create_error = fn + ": bad arguments";
		return EXPANN_ERR_INVALID_ARG;
	}
	// CSR offsets: start at 0, never decrease (a corrupt index file must not turn into
	// out-of-bounds reads on the device)
	if (layer_offsets[0] != 0) {
		g_create_error = fn + ": layer_offsets[0] != 0";
		return EXPANN_ERR_INVALID_ARG;
	}
	for (size_t i = 1; i < (size_t)n_layers * (n + 1); ++i)
		if (layer_offsets[i] < layer_offsets[i - 1]) {
			g_create_error = fn + ": layer_offsets decrease";
			return EXPANN_ERR_INVALID_ARG;
		}
	const uint64_t n_edges = layer_offsets[(size_t)n_layers * (n + 1) - 1];
	if (n_edges >= (1ull << 32)) {
		g_create_error = "more than 2^32 edges";
		return EXPANN_ERR_UNSUPPORTED;
	}
	int ndev = expann_device_count();
	if (ndev <= 0) {
		g_create_error = "no HIP device visible: libexpann_hip has no CPU fallback";
		return EXPANN_ERR_NO_DEVICE;
	}
	if (device < 0 || device >= ndev) {
		g_create_error = "device index out of range";
		return EXPANN_ERR_INVALID_ARG;
	}
	// the validity of every neighbour id is the caller's contract; check it once here so a
	// corrupt index cannot make the kernel read out of bounds
	for (uint64_t e = 0; e < n_edges; ++e)
		if (neighbours[e] >= n) {
			g_create_error = "neighbour id out of range";
			return EXPANN_ERR_INVALID_ARG;
		}
	// (owned until the last step: every early return destroys the handle and what it holds by then)
	std::unique_ptr<expann_graph, GraphDeleter> g(new expann_graph());
	g->dim = dim;
	g->device = device;
	g->n = g->cap_rows = n;
	g->n_layers = n_layers;
	g->starting_vertex = starting_vertex;
	g->rows_f16 = elem_bytes == 2;
	std::vector<uint32_t> off32((size_t)n_layers * (n + 1));
	for (size_t i = 0; i < off32.size(); ++i)
		off32[i] = (uint32_t)layer_offsets[i];
	for (size_t v = 0; v < n; ++v)
		g->max_degree0 = std::max(g->max_degree0, off32[v + 1] - off32[v]);
	auto hip_failed = [&](const char* what) {  // the HIP call that failed, by name
		g_create_error = fn + ": " + what;
		return EXPANN_ERR_HIP;
	};
	if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&g->stream) != hipSuccess)
		return hip_failed("hipSetDevice/hipStreamCreate");
	if (hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess)
		return hip_failed("hipEventCreate");
	const size_t vbytes = n * (size_t)dim * elem_bytes;
	if (hipMalloc(&g->d_vectors, vbytes) != hipSuccess ||
	    hipMalloc(&g->d_layer_off, off32.size() * sizeof(uint32_t)) != hipSuccess ||
	    hipMalloc(&g->d_neighbours, std::max<uint64_t>(n_edges, 1) * sizeof(uint32_t)) != hipSuccess)
		return hip_failed("hipMalloc");
	if (hipMemcpy(g->d_vectors, vectors, vbytes, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(g->d_layer_off, off32.data(), off32.size() * sizeof(uint32_t),
	              hipMemcpyHostToDevice) != hipSuccess ||
	    (n_edges && hipMemcpy(g->d_neighbours, neighbours, n_edges * sizeof(uint32_t),
	                          hipMemcpyHostToDevice) != hipSuccess))
		return hip_failed("hipMemcpy");
	{
		// layer 0 once more at a fixed stride: a hop then reads its list at cur * stride without first
		// fetching the row's offsets (one dependent HBM round trip less per hop)
		g->stride0 = std::max<uint32_t>(4, (g->max_degree0 + 3) / 4 * 4);
		std::vector<uint32_t> adj((size_t)n * g->stride0, 0xFFFFFFFFu);
		for (size_t v = 0; v < n; ++v)
			std::copy(neighbours + off32[v], neighbours + off32[v + 1], adj.begin() + v * g->stride0);
		if (hipMalloc(&g->d_adj0, adj.size() * sizeof(uint32_t)) != hipSuccess)
			return hip_failed("hipMalloc(adj0)");
		if (hipMemcpy(g->d_adj0, adj.data(), adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
			return hip_failed("hipMemcpy(adj0)");
	}
	// one visited array per workgroup of the (persistent) search grid; bounded to ~1/8 of a 288 GB
	// HBM.  The walk is a chain of dependent memory round trips: what hides them is waves per CU
	// (the kernel needs ~60 VGPRs and ~10 KB of LDS at ef = 60: 16 workgroups fit a CU).
	const int cus = num_cus(device);
	uint64_t slots = (uint64_t)cus * 16;
	// visited sets: bitsets (cleared after every query) up to 8 M vertices, epoch bytes beyond
	g->vis_words = n <= (8u << 20) ? (uint32_t)((n + 8191) / 8192 * 256) : 0u;
	if (std::getenv("EXPANN_GRAPH_VISITED_BYTES"))  // (A/B switch: round 2's epoch bytes at any size)
		g->vis_words = 0;
	const uint64_t per_slot = g->vis_words ? (uint64_t)g->vis_words * 4 : (uint64_t)n;
	while (slots > 64 && slots * per_slot > (32ull << 30))
		slots /= 2;
	g->slots = (uint32_t)slots;
	if (hipMalloc(&g->d_visited, slots * per_slot) != hipSuccess ||
	    hipMalloc(&g->d_epochs, slots * sizeof(uint32_t)) != hipSuccess)
		return hip_failed("hipMalloc(visited)");
	if (hipMemset(g->d_visited, 0, slots * per_slot) != hipSuccess ||
	    hipMemset(g->d_epochs, 0, slots * sizeof(uint32_t)) != hipSuccess)
		return hip_failed("hipMemset");
	*out = g.release();
	return EXPANN_OK;
}

extern "C" {

int expann_graph_create(int dim, int device, const float* vectors, size_t n, uint32_t n_layers,
                        uint32_t starting_vertex, const uint64_t* layer_offsets,
                        const uint32_t* neighbours, expann_graph** out) {
	return graph_create("expann_graph_create", sizeof(float), dim, device, vectors, n, n_layers, starting_vertex,
	                    layer_offsets, neighbours, out);
}

int expann_graph_create_f16(int dim, int device, const void* rows_f16, size_t n, uint32_t n_layers,
                            uint32_t starting_vertex, const uint64_t* layer_offsets,
                            const uint32_t* neighbours, expann_graph** out) {
	return graph_create("expann_graph_create_f16", 2, dim, device, rows_f16, n, n_layers, starting_vertex, layer_offsets,
	                    neighbours, out);
}

void expann_graph_destroy(expann_graph* g) {
	if (!g)
		return;
	hipSetDevice(g->device);
	if (g->stream) hipStreamSynchronize(g->stream);
	if (g->dev_outstanding) hipStreamSynchronize(g->dev_stream);
	delete g;
}

const char* expann_graph_last_error(const expann_graph* g) {
	return g ? g->err.c_str() : g_create_error.c_str();
}

double expann_graph_last_kernel_ms(const expann_graph* g) { return g ? g->last_ms : 0.0; }

int expann_graph_search(expann_graph* g, const float* queries, size_t m, size_t k,
                        size_t ef_search, int use_compression, uint64_t* ids, float* dists,
                        uint32_t* distcomps) {
	return expann_graph_search_mode(g, queries, m, k, ef_search, use_compression ? EXPANN_GRAPH_U8_CAST : EXPANN_GRAPH_FP32,
	                                ids, dists, distcomps);
}

int expann_graph_ranged_params(expann_graph* g, float* scale_factor, float* offset) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!scale_factor || !offset)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	if (g->dim % 64 != 0)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "the ranged int8 walk needs dim % 64 == 0");
	if (int rc = graph_ensure_ranged(g))
		return rc;
	*scale_factor = g->ranged_scale;
	*offset = g->ranged_offset;
	return EXPANN_OK;
}

int expann_graph_search_mode(expann_graph* g, const float* queries, size_t m, size_t k, size_t ef_search, int mode,
                             uint64_t* ids, float* dists, uint32_t* distcomps) {
	bool empty = false;
	if (int rc = graph_search_args(g, queries, m, k, ef_search, mode, ids, dists, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));  // (one set of visited arrays: device-buffer searches in flight go first)
	const GraphServe serve = graph_serve(g, k);
	if (serve == kServePad) {  // the filter allows no row: nothing to walk or scan
		std::fill(ids, ids + m * k, UINT64_MAX);
		std::fill(dists, dists + m * k, std::numeric_limits<float>::infinity());
		if (distcomps)
			std::fill(distcomps, distcomps + m, 0u);
		++g->stat_flat;
		g->last_ms = 0;
		return EXPANN_OK;
	}
	const GraphVariant* gv = graph_variant(g->dim, mode, g->filter_on ? kFilterBitmap : kFilterNone, g->rows_f16);
	if (!gv)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "no graph kernel for this dim");
	const bool stamps = std::getenv("EXPANN_GRAPH_STAMPS") != nullptr && g->dim == 128 && !g->filter_on &&
	                    (!g->rows_f16 || mode == EXPANN_GRAPH_FP32);
	if (stamps)
		gv = g->rows_f16 ? &kGraphDbgF16 : &kGraphDbg[mode];
	if (int rc = graph_dev_init(g))
		return rc;
	if (serve == kServeWalk)
		if (int rc = graph_ensure_bytes(g, mode))
			return rc;
	hipStream_t st = g->stream;
	GraphSearchParams p = graph_base_params(g, mode, k, ef_search);
	GraphHostStage stage;
	if (int rc = stage.begin(g, queries, nullptr, m, k, &p))
		return rc;
	DevBuf b_stamps;
	const size_t stamp_bytes = sizeof(unsigned long long) * 8 * g->slots;
	if (stamps)
		HIP_TRY(g, b_stamps.alloc(stamp_bytes));
	p.stamps = b_stamps.as<unsigned long long>();
	if (serve == kServeScan) {  // a sparse filter: the exact scan of the allowed rows
		if (int rc = graph_enqueue_flat(g, p, stage.ctr, st, g->ev0, g->ev1))
			return rc;
		HIP_TRY(g, hipStreamSynchronize(st));
		float ms = 0;
		HIP_TRY(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
		g->last_ms = ms;
		return stage.copy_out(g, ids, dists, distcomps);
	}
	GraphSearchPlan pl;
	if (int rc = graph_search_plan(g, gv, p, stage.ctr, &pl))
		return rc;
	double ms_total = 0;
	// a launch, the wait for it and the slot read back
	auto run = [&](bool redo, size_t walked) -> int {
		if (stamps)
			HIP_TRY(g, hipMemsetAsync(b_stamps.p, 0, stamp_bytes, st));
		if (redo)
			HIP_TRY(g, hipEventRecord(g->ev0, st));
		if (int rc = redo ? graph_enqueue_redo(g, pl, st, g->ev1) : graph_enqueue_first(g, pl, st, g->ev0, g->ev1))
			return rc;
		if (int rc = stage.read_slot(g))
			return rc;
		float ms = 0;
		HIP_TRY(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
		ms_total += ms;
		return stamps ? graph_print_stamps(g, mode, ef_search, ms, redo ? pl.grid_redo : pl.grid, walked, b_stamps.p)
		              : EXPANN_OK;
	};
	if (int rc = run(false, m))
		return rc;
	// this call has waited anyway, so the redo launch goes out only when the first one listed queries for it
	if (stage.h_ctr[2])
		if (int rc = run(true, stage.h_ctr[2]))
			return rc;
	g->last_ms = ms_total;
	return stage.finish(g, ids, dists, distcomps);
}

int expann_graph_search_device(expann_graph* g, const float* d_queries, size_t m, size_t k, size_t ef_search, int mode,
                               uint64_t* d_ids, float* d_dists, uint32_t* d_distcomps, void* stream) {
	bool empty = false;
	if (int rc = graph_search_args(g, d_queries, m, k, ef_search, mode, d_ids, d_dists, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	const GraphServe serve = graph_serve(g, k);
	const GraphVariant* gv = graph_variant(g->dim, mode, g->filter_on ? kFilterBitmap : kFilterNone, g->rows_f16);
	if (!gv)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "no graph kernel for this dim");
	GraphDevSearch s;
	if (int rc = graph_dev_begin(g, stream, mode, serve == kServeWalk, d_queries, m, k, ef_search, d_ids, d_dists, d_distcomps, &s))
		return rc;
	if (serve != kServeWalk) {  // a sparse or empty filter: the scan, or padding alone, in the same stream order
		if (int rc = serve == kServeScan ? graph_enqueue_flat(g, s.p, s.ctr, s.st, g->ev_dev[0], g->ev_dev[1])
		                                 : graph_enqueue_pad(g, s.p, s.ctr, s.st))
			return rc;
		graph_dev_commit(g, s.st, serve == kServeScan, false);
		if (serve == kServePad)
			g->last_ms = 0;
		return EXPANN_OK;
	}
	GraphSearchPlan pl;
	if (int rc = graph_search_plan(g, gv, s.p, s.ctr, &pl))
		return rc;
	// both launches go out without a wait: the redo launch finds its queries, or none, in device memory
	if (int rc = graph_enqueue_first(g, pl, s.st, g->ev_dev[0], g->ev_dev[1]))
		return rc;
	if (pl.has_redo)
		if (int rc = graph_enqueue_redo(g, pl, s.st, g->ev_dev[2]))
			return rc;
	graph_dev_commit(g, s.st, true, pl.has_redo);
	return EXPANN_OK;
}

int expann_graph_sync(expann_graph* g) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	HIP_TRY(g, hipSetDevice(g->device));
	if (int rc = graph_drain(g))
		return rc;
	if (g->dev_timed) {  // the last search's launches, from its events
		float ms = 0, ms_redo = 0;
		HIP_TRY(g, hipEventElapsedTime(&ms, g->ev_dev[0], g->ev_dev[1]));
		if (g->dev_timed_redo)
			HIP_TRY(g, hipEventElapsedTime(&ms_redo, g->ev_dev[1], g->ev_dev[2]));
		g->last_ms = (double)ms + (double)ms_redo;
		g->stat_redo_ms = ms_redo;
		g->dev_timed = false;
	}
	const uint64_t overflows = g->pend_overflows;
	g->stat_redo_queries = g->pend_redo_queries;
	g->stat_redo_overflows += overflows;
	g->pend_overflows = g->pend_redo_queries = 0;
	if (overflows)
		return g->fail(EXPANN_ERR_OVERFLOW, "graph search: candidates queue overflowed its LDS capacity in " +
		                                        std::to_string(overflows) + " search(es) since the last sync");
	return EXPANN_OK;
}

int expann_graph_set_option(expann_graph* g, const char* name, long value) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!name)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL option name");
	std::string msg;
	const int rc = set_graph_option(*g, name, value, &msg);  // (graph_options.hpp: the table and its rules)
	return rc ? g->fail(rc, msg) : EXPANN_OK;
}

int expann_graph_set_row_filter(expann_graph* g, const uint32_t* allow_bits, size_t n_words) {
	return graph_set_row_filter(g, allow_bits, n_words, false, nullptr);
}

int expann_graph_set_row_filter_device(expann_graph* g, const uint32_t* d_allow_bits, size_t n_words, void* stream) {
	return graph_set_row_filter(g, d_allow_bits, n_words, true, (hipStream_t)stream);
}

int expann_graph_clear_row_filter(expann_graph* g) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (g->dev_outstanding) {  // (searches enqueued under the filter finish under it)
		HIP_TRY(g, hipSetDevice(g->device));
		HIP_TRY(g, graph_wait_outstanding(g));
	}
	g->filter_on = false;
	return EXPANN_OK;
}

int expann_graph_set_row_groups(expann_graph* g, const uint32_t* groups, size_t n) {
	return graph_set_row_groups(g, groups, n, false, nullptr);
}

int expann_graph_set_row_groups_device(expann_graph* g, const uint32_t* d_groups, size_t n, void* stream) {
	return graph_set_row_groups(g, d_groups, n, true, (hipStream_t)stream);
}

int expann_graph_clear_row_groups(expann_graph* g) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (g->dev_outstanding) {  // (searches enqueued under the groups finish under them)
		HIP_TRY(g, hipSetDevice(g->device));
		HIP_TRY(g, graph_wait_outstanding(g));
	}
	g->forget<GraphRowGroups>();
	return EXPANN_OK;
}

int expann_graph_search_grouped_device(expann_graph* g, const float* d_queries, const uint32_t* d_query_groups, size_t m,
                                       size_t k, size_t ef_search, int mode, uint64_t* d_ids, float* d_dists,
                                       uint32_t* d_distcomps, void* stream) {
	bool empty = false;
	if (int rc = graph_search_args(g, d_queries, m, k, ef_search, mode, d_ids, d_dists, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	if (int rc = graph_grouped_args(g, d_query_groups))
		return rc;
	HIP_TRY(g, hipSetDevice(g->device));
	GraphDevSearch s;
	if (int rc = graph_dev_begin(g, stream, mode, true, d_queries, m, k, ef_search, d_ids, d_dists, d_distcomps, &s))
		return rc;
	hipEvent_t ev[3] = {g->ev_dev[0], g->ev_dev[1], g->ev_dev[2]};
	bool has_redo = false;
	if (int rc = graph_enqueue_grouped(g, s.p, d_query_groups, mode, s.ctr, s.st, ev, &has_redo))
		return rc;
	graph_dev_commit(g, s.st, true, has_redo);
	return EXPANN_OK;
}

// host buffers: the same launches on the handle's own stream with the host-buffer calls' counter slot, waited for here
int expann_graph_search_grouped(expann_graph* g, const float* queries, const uint32_t* query_groups, size_t m, size_t k,
                                size_t ef_search, int mode, uint64_t* ids, float* dists, uint32_t* distcomps) {
	bool empty = false;
	if (int rc = graph_search_args(g, queries, m, k, ef_search, mode, ids, dists, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	if (int rc = graph_grouped_args(g, query_groups))
		return rc;
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));  // (one set of visited arrays: device-buffer searches in flight go first)
	if (int rc = graph_dev_init(g))
		return rc;
	if (!g->ev2)
		HIP_TRY(g, hipEventCreate(&g->ev2));
	if (int rc = graph_ensure_bytes(g, mode))  // (before the parameters: they name the byte copy)
		return rc;
	GraphSearchParams p = graph_base_params(g, mode, k, ef_search);
	GraphHostStage stage;
	if (int rc = stage.begin(g, queries, query_groups, m, k, &p))
		return rc;
	hipEvent_t ev[3] = {g->ev0, g->ev1, g->ev2};
	bool has_redo = false;
	if (int rc = graph_enqueue_grouped(g, p, stage.b_qg.as<uint32_t>(), mode, stage.ctr, g->stream, ev, &has_redo))
		return rc;
	if (int rc = stage.read_slot(g))
		return rc;
	float ms = 0, ms_redo = 0;
	HIP_TRY(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
	if (has_redo)
		HIP_TRY(g, hipEventElapsedTime(&ms_redo, g->ev1, g->ev2));
	g->last_ms = (double)ms + (double)ms_redo;
	for (int j = 0; j < 3; ++j)
		g->stat_group[j] += stage.h_ctr[5 + j];
	return stage.finish(g, ids, dists, distcomps);
}

int expann_graph_range_search_device(expann_graph* g, const float* d_queries, const float* d_radii, size_t m,
                                     size_t max_results, size_t ef_search, uint64_t* d_ids, float* d_dists,
                                     uint32_t* d_counts, uint32_t* d_distcomps, void* stream) {
	bool empty = false;
	if (int rc = graph_range_args(g, d_queries, d_radii, m, max_results, ef_search, d_ids, d_counts, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	GraphDevSearch s;
	if (int rc = graph_dev_begin(g, stream, EXPANN_GRAPH_FP32, false, d_queries, m, max_results, ef_search, d_ids, d_dists,
	                             d_distcomps, &s))
		return rc;
	hipEvent_t ev[3] = {g->ev_dev[0], g->ev_dev[1], g->ev_dev[2]};
	bool has_redo = false;
	if (int rc = graph_enqueue_range(g, s.p, d_radii, d_counts, s.ctr, s.st, ev, &has_redo))
		return rc;
	graph_dev_commit(g, s.st, true, has_redo);
	return EXPANN_OK;
}

// host buffers: the same launches on the handle's own stream with the host-buffer calls' counter slot, waited for here
int expann_graph_range_search(expann_graph* g, const float* queries, const float* radii, size_t m, size_t max_results,
                              size_t ef_search, uint64_t* ids, float* dists, uint32_t* counts, uint32_t* distcomps) {
	bool empty = false;
	if (int rc = graph_range_args(g, queries, radii, m, max_results, ef_search, ids, counts, &empty))
		return rc;
	if (empty)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));  // (one set of visited arrays: device-buffer searches in flight go first)
	if (int rc = graph_dev_init(g))
		return rc;
	if (!g->ev2)
		HIP_TRY(g, hipEventCreate(&g->ev2));
	GraphSearchParams p = graph_base_params(g, EXPANN_GRAPH_FP32, max_results, ef_search);
	GraphHostStage stage;
	if (int rc = stage.begin(g, queries, nullptr, m, max_results, &p, radii))
		return rc;
	hipEvent_t ev[3] = {g->ev0, g->ev1, g->ev2};
	bool has_redo = false;
	if (int rc = graph_enqueue_range(g, p, stage.b_r.as<float>(), stage.b_cnt.as<uint32_t>(), stage.ctr, g->stream, ev, &has_redo))
		return rc;
	if (int rc = stage.read_slot(g))
		return rc;
	float ms = 0, ms_redo = 0;
	HIP_TRY(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
	if (has_redo)
		HIP_TRY(g, hipEventElapsedTime(&ms_redo, g->ev1, g->ev2));
	g->last_ms = (double)ms + (double)ms_redo;
	return stage.finish(g, ids, dists, distcomps, counts);
}

int expann_graph_get_stat(expann_graph* g, const char* name, uint64_t* out) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!name || !out)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	using G = const expann_graph*;
	struct StatRow {
		const char* name;
		uint64_t (*read)(G);
	};
	static const StatRow kGraphStatTable[] = {
	    {"redo_queries", [](G g) { return g->stat_redo_queries; }},
	    {"redo_overflows", [](G g) { return g->stat_redo_overflows; }},
	    {"deferred_searches", [](G g) { return g->stat_deferred; }},
	    {"distcomps", [](G g) { return g->stat_distcomps; }},
	    {"redo_kernel_ns", [](G g) { return (uint64_t)(g->stat_redo_ms * 1e6); }},
	    {"filter_active", [](G g) -> uint64_t { return g->filter_on ? 1 : 0; }},
	    {"filter_rows", [](G g) -> uint64_t { return g->filter_on ? g->n_allowed : g->n; }},
	    {"flat_searches", [](G g) { return g->stat_flat; }},
	    {"groups_active", [](G g) -> uint64_t { return g->groups_on ? 1 : 0; }},
	    {"group_count", [](G g) -> uint64_t { return g->groups_on ? g->n_groups : 0; }},  // distinct labels other than 0xFFFFFFFF
	    {"group_walk_queries", [](G g) { return g->stat_group[0]; }},
	    {"group_scan_queries", [](G g) { return g->stat_group[1]; }},
	    {"group_pad_queries", [](G g) { return g->stat_group[2]; }},
	    // the device bytes of the rows themselves
	    {"vector_bytes", [](G g) { return (uint64_t)g->n * (uint64_t)g->dim * (g->rows_f16 ? 2u : 4u); }},
	};
	// the range search's rows (tests/test_graph_options.py pins the names of the table above, one by one)
	static const StatRow kGraphRangeStatTable[] = {
	    {"range_searches", [](G g) { return g->stat_range; }},  // since create, from either entry point
	};
	// the append's rows (THE GRAPH APPEND RULE)
	static const StatRow kGraphAppendStatTable[] = {
	    {"append_calls", [](G g) { return g->stat_append.calls; }},
	    {"append_rows", [](G g) { return g->stat_append.rows; }},
	    {"append_batches", [](G g) { return g->stat_append.batches; }},
	    {"append_device", [](G g) { return g->stat_append.device; }},
	    {"append_host", [](G g) { return g->stat_append.host; }},
	    {"graph_reallocs", [](G g) { return g->stat_append.reallocs; }},
	    {"capacity_rows", [](G g) { return (uint64_t)g->cap_rows; }},
	    // the last rebuild of the walk's tables from the resident state: device time, edges of all layers
	    {"append_tables_ns", [](G g) { return g->tables_ns; }},
	    {"append_edges", [](G g) { return g->n_edges; }},
	};
	// the remove's rows (THE GRAPH REMOVE RULE)
	static const StatRow kGraphRemoveStatTable[] = {
	    {"remove_calls", [](G g) { return g->stat_remove.calls; }},
	    {"remove_rows", [](G g) { return g->stat_remove.rows; }},
	    {"remove_touched_rows", [](G g) { return g->stat_remove.touched; }},
	    // touched rows whose distinct candidates exceeded max(ef_construction, M0)
	    {"remove_truncated_rows", [](G g) { return g->stat_remove.truncated; }},
	    {"remove_device", [](G g) { return g->stat_remove.device; }},
	    {"remove_host", [](G g) { return g->stat_remove.host; }},
	    // device time of touch + gather + prune of the last call
	    {"remove_repair_ns", [](G g) { return g->remove_repair_ns; }},
	};
	auto read_from = [&](const StatRow* rows, size_t n_rows) {
		for (size_t i = 0; i < n_rows; ++i)
			if (!std::strcmp(name, rows[i].name)) {
				*out = rows[i].read(g);
				return true;
			}
		return false;
	};
	if (read_from(kGraphStatTable, sizeof(kGraphStatTable) / sizeof(StatRow)) ||
	    read_from(kGraphRangeStatTable, sizeof(kGraphRangeStatTable) / sizeof(StatRow)) ||
	    read_from(kGraphAppendStatTable, sizeof(kGraphAppendStatTable) / sizeof(StatRow)) ||
	    read_from(kGraphRemoveStatTable, sizeof(kGraphRemoveStatTable) / sizeof(StatRow)))
		return EXPANN_OK;
	return g->fail(EXPANN_ERR_INVALID_ARG, std::string("unknown stat: ") + name);
}

// test hook: a queue trace through the device's wave-cooperative heap code (tests/test_heap_pin.py);
// the signature of oracle_heap_trace / std_heap_trace, ids must fit 32 bits
size_t expann_device_heap_trace(int max_heap, size_t n_init, const float* init_d, const uint64_t* init_id, size_t n_ops,
                                const int* ops, const float* op_d, const uint64_t* op_id, uint64_t* out_size,
                                float* out_top_d, uint64_t* out_top_id, float* drain_d, uint64_t* drain_id) {
	const size_t cap = n_init + n_ops + 1;
	if (cap * sizeof(md_pair) > (60u << 10) || hipSetDevice(0) != hipSuccess)
		return (size_t)-1;
	std::vector<uint32_t> id32(n_init), opid32(n_ops);
	for (size_t i = 0; i < n_init; ++i)
		id32[i] = (uint32_t)init_id[i];
	for (size_t i = 0; i < n_ops; ++i)
		opid32[i] = (uint32_t)op_id[i];
	DevBuf b_id, b_ii, b_ops, b_od, b_oi, b_sz, b_td, b_ti, b_dd, b_di, b_n;
	if (b_id.alloc(4 * n_init) != hipSuccess || b_ii.alloc(4 * n_init) != hipSuccess || b_ops.alloc(4 * n_ops) != hipSuccess ||
	    b_od.alloc(4 * n_ops) != hipSuccess || b_oi.alloc(4 * n_ops) != hipSuccess || b_sz.alloc(4 * (n_ops + 1)) != hipSuccess ||
	    b_td.alloc(4 * (n_ops + 1)) != hipSuccess || b_ti.alloc(4 * (n_ops + 1)) != hipSuccess ||
	    b_dd.alloc(4 * cap) != hipSuccess || b_di.alloc(4 * cap) != hipSuccess || b_n.alloc(4) != hipSuccess)
		return (size_t)-1;
	hipMemcpy(b_id.p, init_d, 4 * n_init, hipMemcpyHostToDevice);
	hipMemcpy(b_ii.p, id32.data(), 4 * n_init, hipMemcpyHostToDevice);
	hipMemcpy(b_ops.p, ops, 4 * n_ops, hipMemcpyHostToDevice);
	hipMemcpy(b_od.p, op_d, 4 * n_ops, hipMemcpyHostToDevice);
	hipMemcpy(b_oi.p, opid32.data(), 4 * n_ops, hipMemcpyHostToDevice);
	HeapTraceParams p{max_heap, (uint32_t)n_init, (uint32_t)n_ops, b_id.as<float>(), b_ii.as<uint32_t>(), b_ops.as<int>(),
	                  b_od.as<float>(), b_oi.as<uint32_t>(), b_sz.as<uint32_t>(), b_td.as<float>(), b_ti.as<uint32_t>(),
	                  b_dd.as<float>(), b_di.as<uint32_t>(), b_n.as<uint32_t>(), 0u};
	if (const char* e = std::getenv("EXPANN_GRAPH_DEBUG"))
		p.serial = (uint32_t)std::atol(e) & 1u;
	hipLaunchKernelGGL(heap_trace_kernel, dim3(1), dim3(64), cap * sizeof(md_pair), nullptr, p);
	if (hipDeviceSynchronize() != hipSuccess)
		return (size_t)-1;
	std::vector<uint32_t> sz(n_ops + 1), ti(n_ops + 1), di(cap);
	uint32_t nd = 0;
	hipMemcpy(sz.data(), b_sz.p, 4 * (n_ops + 1), hipMemcpyDeviceToHost);
	hipMemcpy(out_top_d, b_td.p, 4 * (n_ops + 1), hipMemcpyDeviceToHost);
	hipMemcpy(ti.data(), b_ti.p, 4 * (n_ops + 1), hipMemcpyDeviceToHost);
	hipMemcpy(&nd, b_n.p, 4, hipMemcpyDeviceToHost);
	hipMemcpy(drain_d, b_dd.p, 4 * (size_t)nd, hipMemcpyDeviceToHost);
	hipMemcpy(di.data(), b_di.p, 4 * (size_t)nd, hipMemcpyDeviceToHost);
	for (size_t i = 0; i <= n_ops; ++i) {
		out_size[i] = sz[i];
		out_top_id[i] = ti[i];
	}
	for (uint32_t i = 0; i < nd; ++i)
		drain_id[i] = di[i];
	return nd;
}

// ---- GPU-assisted batched construction (graph_build.hpp) -------------------------------------
namespace {
using BuildSearchFn = void (*)(BuildSearchParams);
using BuildPruneFn = void (*)(BuildPruneParams);
struct BuildVariant {
	int d;
	BuildSearchFn search;
	BuildPruneFn prune;
};
#define BUILD_V(D) {D, build_search_kernel<D>, build_prune_kernel<D>}
const BuildVariant kBuild[] = {BUILD_V(64),  BUILD_V(128), BUILD_V(256), BUILD_V(512),
                               BUILD_V(768), BUILD_V(832), BUILD_V(960), BUILD_V(0)};
#undef BUILD_V
const BuildVariant* build_variant(int dim) {
	const BuildVariant* bv = &kBuild[sizeof(kBuild) / sizeof(kBuild[0]) - 1];  // (d = 0: run-time dim)
	for (const auto& v : kBuild)
		if (v.d == dim)
			bv = &v;
	return bv;
}

// The batch loop of THE BATCH RULE over device arrays: expann_graph_build_batched runs it over arrays it makes for
// the call, expann_graph_append over the handle's resident builder state.  build_batches fills what the two share;
// the caller sets the rest down to `resident`, and build_batches_geometry derives the launch geometry.
struct BuildBatches {
	const BuildVariant* bv;
	BuildGraph g;
	BuildConfig cfg;
	const BuildScratch* s;  // sized for max_batch + max_up_in_batch lists before build_run_batches
	hipStream_t st;
	int dim, cus;
	const uint8_t* levels;  // host: the level of vertex v is levels[v - level_base]
	size_t level_base;
	size_t b0, n;           // vertices [b0, n) are inserted; b0 ends behind the last batch that is in
	uint32_t max_layer, starting_vertex;  // in and out
	size_t max_batch;
	uint32_t* vis_bits;     // [slots][vis_words], all zero between searches
	uint32_t vis_words;
	// the resident form: the search's overflow counter is read before the batch's prune and reverse launches, so a
	// batch that overflows leaves the graph as it was; that wait is the batch's only one
	bool resident;
	// geometry
	size_t max_up_in_batch, search_lds, prune_lds;
	uint32_t list_cap, cand_cap;
	uint64_t slots;         // resident search workgroups
	// out
	uint64_t n_batches = 0, n_dirty_total = 0;
};
extern "C++" {  // (templates, a struct returned: this namespace sits inside the C ABI's linkage block)
BuildBatches build_batches(const BuildGraph& view, const BuildScratch& scratch, const BuildConfig& cfg, hipStream_t st, int dim,
                           int device) {
	return BuildBatches{build_variant(dim), view, cfg, &scratch, st, dim, num_cus(device)};  // (the rest zero)
}
template <typename F> int build_batches_geometry(F* fh, BuildBatches& r, bool upper_layers) {
	const size_t ef = r.cfg.ef_construction;
	if (r.max_batch == 0)
		r.max_batch = 32768;
	// search: one wave per new vertex; LDS = nearest heap + candidates heap + a hop's neighbour list
	r.list_cap = (uint32_t)std::max<size_t>(r.g.stride0, std::max<size_t>(r.g.strideu, ef));
	r.cand_cap = 8192;
	r.search_lds = sizeof(md_pair) * (ef + 1 + r.cand_cap + 1) + (sizeof(uint32_t) + sizeof(float)) * r.list_cap +
	               8 * sizeof(uint32_t) +
	               (r.bv->d == 0 ? (size_t)r.dim * sizeof(float) : 0);  // (run-time dim: the new row in LDS)
	// the prune kernel of the run-time-dim instance keeps the kept edge's row in dynamic LDS
	r.prune_lds = r.bv->d == 0 ? (size_t)r.dim * sizeof(float) : 0;
	HIP_TRY(fh, hipFuncSetAttribute((const void*)r.bv->search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.search_lds));
	r.slots = (uint64_t)r.cus * 2;  // resident search workgroups (two 72 KB workgroups per CU)
	r.max_up_in_batch = r.max_batch * (upper_layers ? 1 : 0) + 64;  // (bounded below per batch)
	return EXPANN_OK;
}
template <typename F> int build_run_batches(F* fh, BuildBatches& r) {
	const BuildVariant* bv = r.bv;
	const BuildGraph& g = r.g;
	const BuildScratch& s = *r.s;
	hipStream_t st = r.st;
	uint32_t* ctr = s.ctr;
	auto level_of = [&](size_t v) { return r.levels[v - r.level_base]; };
	const char* overflow = "construction search: candidates queue overflowed its LDS capacity";
	std::vector<PruneTask> tasks;
	std::vector<int32_t> up_slot;
	while (r.b0 < r.n) {
		const size_t b0 = r.b0;
		// a batch: at most 1/16 of the graph so far (its members do not see each other: measured
		// recall@10 at ef = 10, 12 k rows, M = 16: serial 0.384, batches of 1/8 0.354); a vertex that
		// opens a new layer goes alone
		size_t b1 = std::min(r.n, b0 + std::min(r.max_batch, std::max<size_t>(1, b0 / 16)));
		for (size_t v = b0; v < b1; ++v)
			if (level_of(v) >= r.max_layer) {
				b1 = v == b0 ? v + 1 : v;
				break;
			}
		const uint32_t B = (uint32_t)(b1 - b0);
		tasks.clear();
		up_slot.assign(B, -1);
		uint32_t n_up = 0;
		for (uint32_t i = 0; i < B; ++i)
			tasks.push_back(PruneTask{(uint32_t)(b0 + i), 0u, (int32_t)i});
		for (uint32_t i = 0; i < B; ++i) {
			const uint32_t lv = std::min<uint32_t>(level_of(b0 + i), r.max_layer - 1);
			if (lv >= 1) {
				up_slot[i] = (int32_t)n_up;
				for (uint32_t l = 1; l <= lv; ++l)
					tasks.push_back(PruneTask{(uint32_t)(b0 + i), l, (int32_t)(B + n_up + l - 1)});
				n_up += lv;
			}
		}
		if (n_up > r.max_up_in_batch)
			return fh->fail(EXPANN_ERR_UNSUPPORTED, "more upper-layer vertices in a batch than provisioned");
		const uint32_t n_tasks = (uint32_t)tasks.size();
		HIP_TRY(fh, hipMemcpyAsync(s.tasks, tasks.data(), sizeof(PruneTask) * n_tasks, hipMemcpyHostToDevice, st));
		HIP_TRY(fh, hipMemcpyAsync(s.up_slot, up_slot.data(), 4 * B, hipMemcpyHostToDevice, st));
		HIP_TRY(fh, hipMemcpyAsync(ctr + 3, &n_tasks, 4, hipMemcpyHostToDevice, st));
		HIP_TRY(fh, hipMemsetAsync(ctr, 0, 4, st));
		BuildSearchParams sp{};
		sp.g = g;
		sp.b0 = (uint32_t)b0;
		sp.b1 = (uint32_t)b1;
		sp.max_layer = r.max_layer;
		sp.starting_vertex = r.starting_vertex;
		sp.ef = (uint32_t)r.cfg.ef_construction;
		sp.cand_cap = r.cand_cap;
		sp.list_cap = r.list_cap;
		sp.vis_bits = r.vis_bits;
		sp.vis_words = r.vis_words;
		sp.up_slot = s.up_slot;
		sp.out = s.out;
		sp.out_cnt = s.out_cnt;
		sp.error = ctr + 2;
		sp.dim = (uint32_t)r.dim;
		hipLaunchKernelGGL(bv->search, dim3((uint32_t)std::min<uint64_t>(B, r.slots)), dim3(64), r.search_lds, st, sp);
		uint32_t h_ctr[4];
		if (r.resident) {
			HIP_TRY(fh, hipGetLastError());
			HIP_TRY(fh, hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
			HIP_TRY(fh, hipStreamSynchronize(st));
			if (h_ctr[2])
				return fh->fail(EXPANN_ERR_OVERFLOW, overflow);
		}
		BuildPruneParams pp{};
		pp.g = g;
		pp.tasks = s.tasks;
		pp.n_tasks = ctr + 3;
		pp.lists = s.out;
		pp.list_cnt = s.out_cnt;
		pp.ef = (uint32_t)r.cfg.ef_construction;
		pp.ortho_factor = r.cfg.ortho_factor;
		pp.ortho_bias = r.cfg.ortho_bias;
		pp.prune_overflow = (uint32_t)r.cfg.prune_overflow;
		pp.dim = (uint32_t)r.dim;
		hipLaunchKernelGGL(bv->prune, dim3(std::min<uint32_t>(n_tasks, (uint32_t)r.cus * 16)), dim3(kPruneThreads), r.prune_lds, st, pp);
		BuildReverseParams rp{};
		rp.g = g;
		rp.tasks = s.tasks;
		rp.n_tasks = n_tasks;
		rp.dirty = s.dirty;
		rp.n_dirty = ctr;
		rp.dirty_cap = (uint32_t)s.dirty_cap;
		rp.dropped = ctr + 1;
		hipLaunchKernelGGL(build_reverse_kernel, dim3((n_tasks + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, st, rp);
		// the rows that outgrew their cap: clamp to the slack, prune (grid-stride over the dirty list)
		hipLaunchKernelGGL(build_clamp_kernel, dim3((uint32_t)((s.dirty_cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, g,
		                   (const uint2*)s.dirty.get(), (const uint32_t*)ctr);
		BuildPruneParams dp = pp;
		dp.tasks = nullptr;
		dp.n_tasks = ctr;
		dp.dirty = s.dirty;
		hipLaunchKernelGGL(bv->prune, dim3((uint32_t)r.cus * 16), dim3(kPruneThreads), r.prune_lds, st, dp);
		HIP_TRY(fh, hipGetLastError());
		if (!r.resident) {
			HIP_TRY(fh, hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
			HIP_TRY(fh, hipStreamSynchronize(st));
			if (h_ctr[2])
				return fh->fail(EXPANN_ERR_OVERFLOW, overflow);
			r.n_dirty_total += h_ctr[0];
		}
		++r.n_batches;
		for (size_t v = b0; v < b1; ++v)  // :461-464
			while (level_of(v) >= r.max_layer) {
				++r.max_layer;
				r.starting_vertex = (uint32_t)v;
			}
		r.b0 = b1;
	}
	return EXPANN_OK;
}
}  // extern "C++"
}  // namespace

int expann_graph_build_batched(int dim, int device, const float* vectors, size_t n, const uint8_t* levels,
                               size_t n_built, uint32_t* max_layer_io, uint32_t* starting_vertex_io, size_t M,
                               size_t M0, size_t ef_construction, size_t prune_overflow, float ortho_factor,
                               float ortho_bias, size_t max_batch, uint32_t* ids0, float* d0, uint32_t* deg0,
                               size_t stride0, const int32_t* upper_idx, size_t U, size_t n_upper_layers,
                               uint32_t* idsu, float* du, uint32_t* degu, size_t strideu, uint64_t* stats) {
	if (int rc = graph_dim_error("expann_graph_build_batched", dim))
		return rc;
	if (!vectors || !levels || !max_layer_io || !starting_vertex_io || !ids0 || !d0 || !deg0 || !upper_idx ||
	    n == 0 || n_built == 0 || n_built > n || n >= (1ull << 32) - 64 || M < 2 || M0 < M || stride0 < M0 ||
	    (n_upper_layers && (!idsu || !du || !degu || strideu < M)) || ef_construction == 0 ||
	    ef_construction > (size_t)kPruneMaxCand || stride0 > (size_t)kPruneMaxCand ||
	    strideu > (size_t)kPruneMaxCand || *max_layer_io == 0 || *max_layer_io > n_upper_layers + 1 ||
	    *starting_vertex_io >= n_built) {
		g_create_error = "expann_graph_build_batched: bad arguments (ef_construction and row strides <= 1024)";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (expann_device_count() <= device || device < 0) {
		g_create_error = "no such HIP device: libexpann_hip has no CPU fallback";
		return EXPANN_ERR_NO_DEVICE;
	}
	struct Fail {
		int fail(int code, const std::string& m) const {
			g_create_error = "expann_graph_build_batched: " + m;
			return code;
		}
	} F;
	Fail* fh = &F;
	HIP_TRY(fh, hipSetDevice(device));
	struct StreamGuard {  // (every early return below leaves through this)
		hipStream_t s = nullptr;
		~StreamGuard() {
			if (s)
				(void)hipStreamDestroy(s);
		}
	} sg;
	HIP_TRY(fh, hipStreamCreate(&sg.s));
	hipStream_t st = sg.s;
	// the builder's arrays in the host's layout ([layer][U]: U_cap = U, L_cap = n_upper_layers), for this call
	DevBuf b_vec, b_vis;
	BuilderArrays arrays;
	BuildScratch scratch;
	HIP_TRY(fh, b_vec.alloc(n * (size_t)dim * 4));
	HIP_TRY(fh, hipMemcpyAsync(b_vec.p, vectors, n * (size_t)dim * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(fh, arrays.alloc(n, (uint32_t)stride0, (uint32_t)strideu, U, n_upper_layers, st));
	HIP_TRY(fh, arrays.copy_host<true>(n, levels, upper_idx, ids0, d0, deg0, U, n_upper_layers, U, idsu, du, degu, st));
	BuildBatches r = build_batches(arrays.view(b_vec.as<float>(), n, M0, M), scratch,
	                               BuildConfig{M, M0, ef_construction, prune_overflow, ortho_factor, ortho_bias}, st, dim, device);
	r.levels = levels;
	r.b0 = n_built;
	r.n = n;
	r.max_layer = *max_layer_io;
	r.starting_vertex = *starting_vertex_io;
	r.max_batch = max_batch;
	if (int rc = build_batches_geometry(fh, r, n_upper_layers != 0))
		return rc;
	// one visited bitset per resident workgroup, all zero between searches (graph_search.hpp)
	r.vis_words = (uint32_t)((n + 8191) / 8192 * 256);
	HIP_TRY(fh, b_vis.alloc(r.slots * r.vis_words * 4));
	HIP_TRY(fh, hipMemsetAsync(b_vis.p, 0, r.slots * r.vis_words * 4, st));
	r.vis_bits = b_vis.as<uint32_t>();
	HIP_TRY(fh, scratch.alloc(r.max_batch + r.max_up_in_batch, r.max_batch, ef_construction, n + arrays.upper_rows() + 1, st));
	if (int rc = build_run_batches(fh, r))
		return rc;
	HIP_TRY(fh, arrays.copy_host<false>(n, (uint8_t*)nullptr, (int32_t*)nullptr, ids0, d0, deg0, U, n_upper_layers, U, idsu, du, degu, st));
	uint32_t h_ctr[4];
	HIP_TRY(fh, hipMemcpy(h_ctr, scratch.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost));
	*max_layer_io = r.max_layer;
	*starting_vertex_io = r.starting_vertex;
	if (stats) {
		stats[0] = r.n_batches;
		stats[1] = h_ctr[1];
		stats[2] = r.n_dirty_total;
		stats[3] = h_ctr[2];
	}
	return EXPANN_OK;
}

}  // extern "C"

// ---- appends to a built graph: the builder's state resident in the handle (THE GRAPH APPEND RULE) ----------
namespace {
BuildGraph graph_build_view(const expann_graph* g) { return g->arrays.view(g->d_vectors.as<const float>(), g->n, g->cfg.M0, g->cfg.M); }

// what is sized by (cap_rows, U_cap, L_cap) and holds nothing between two rebuilds of the tables: the CSR, the dirty
// list, the scan's tile sums.  The CSR's CONTENT is lost when it grows: the caller rebuilds the tables.
int graph_size_derived(expann_graph* g) {
	const size_t up_rows = g->arrays.upper_rows(), L_cap = g->arrays.L_cap;
	const size_t off = (L_cap + 1) * (g->cap_rows + 1), edges = g->cap_rows * g->cfg.M0 + up_rows * g->cfg.M;
	if (off >= (1ull << 32) || edges >= (1ull << 32))
		return g->fail(EXPANN_ERR_UNSUPPORTED, "the capacity would take more than 2^32 edges or offsets");
	if (off > g->off_cap) {
		g->d_layer_off.reset();
		HIP_TRY(g, hipMalloc(&g->d_layer_off, off * sizeof(uint32_t)));
		g->off_cap = off;
		g->tiles_cap = (off + kScanTile - 1) / kScanTile;
		g->d_tile_sums.reset();
		HIP_TRY(g, hipMalloc(&g->d_tile_sums, g->tiles_cap * sizeof(uint32_t)));
	}
	if (edges > g->edge_cap) {
		g->d_neighbours.reset();
		HIP_TRY(g, hipMalloc(&g->d_neighbours, std::max<size_t>(edges, 1) * sizeof(uint32_t)));
		g->edge_cap = edges;
	}
	HIP_TRY(g, g->scratch.size_dirty(g->cap_rows + up_rows + 1));
	return EXPANN_OK;
}

// d_adj0 and the CSR remade from the resident state (graph_append.hpp) on the handle's stream, and waited for
int graph_rebuild_tables(expann_graph* g) {
	if (g->n > g->cap_rows || g->n_layers == 0 || g->n_layers > g->arrays.L_cap + 1 || g->stride0 % 4 != 0 || g->stride0 < g->cfg.M0)
		return g->fail(EXPANN_ERR_INVALID_ARG, "graph append: the builder state does not fit its capacity");
	AppendTables t{};
	t.g = graph_build_view(g);
	t.n_layers = g->n_layers;
	t.adj0 = g->d_adj0;
	t.stride0 = g->stride0;
	t.layer_off = g->d_layer_off;
	t.neighbours = g->d_neighbours;
	t.edge_cap = (uint32_t)g->edge_cap;
	t.tile_sums = g->d_tile_sums;
	const uint64_t entries = (uint64_t)g->n_layers * (g->n + 1), quads = (uint64_t)g->n * (g->stride0 / 4);
	const uint32_t n_tiles = (uint32_t)((entries + kScanTile - 1) / kScanTile);
	hipStream_t st = g->stream;
	for (OwnedEvent& ev : g->ev_tables)
		if (!ev)
			HIP_TRY(g, hipEventCreate(&ev));
	HIP_TRY(g, hipEventRecord(g->ev_tables[0], st));
	hipLaunchKernelGGL(append_adj0_kernel, dim3((uint32_t)((quads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, t);
	hipLaunchKernelGGL(append_degree_kernel, dim3((uint32_t)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, t);
	hipLaunchKernelGGL(append_scan_reduce_kernel, dim3(n_tiles), dim3(kBlock), 0, st, t);
	hipLaunchKernelGGL(append_scan_sums_kernel, dim3(1), dim3(kBlock), 0, st, t.tile_sums, n_tiles);
	hipLaunchKernelGGL(append_scan_tiles_kernel, dim3(n_tiles), dim3(kBlock), 0, st, t);
	hipLaunchKernelGGL(append_fill_kernel, dim3((uint32_t)((entries + kBlock / 16 - 1) / (kBlock / 16))), dim3(kBlock), 0, st, t);
	HIP_TRY(g, hipGetLastError());
	HIP_TRY(g, hipEventRecord(g->ev_tables[1], st));
	uint32_t last = 0;  // (the end entry of the top layer: every edge lies before it)
	HIP_TRY(g, hipMemcpyAsync(&last, g->d_layer_off.get() + entries - 1, sizeof(last), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipStreamSynchronize(st));
	float ms = 0;
	HIP_TRY(g, hipEventElapsedTime(&ms, g->ev_tables[0], g->ev_tables[1]));
	g->tables_ns = (uint64_t)((double)ms * 1e6);
	g->n_edges = last;
	return EXPANN_OK;
}

// room for `rows` rows in everything that is sized by the row count.  The caller has waited for the searches in
// flight.  A resident handle's CSR is left without content: the caller rebuilds the tables.
int graph_grow_rows(expann_graph* g, size_t rows) {
	if (rows <= g->cap_rows)
		return EXPANN_OK;
	if (g->vis_words == 0 || rows > (8u << 20))
		return g->fail(EXPANN_ERR_UNSUPPORTED, "a graph handle grows up to 8 Mi rows (visited bitsets)");
	const size_t n = g->n, row_bytes = (size_t)g->dim * (g->rows_f16 ? 2 : 4);
	hipStream_t st = g->stream;
	HIP_TRY(g, dev_regrow(g->d_vectors, n * row_bytes, rows * row_bytes, st));
	HIP_TRY(g, dev_regrow(g->d_adj0, n * g->stride0 * sizeof(uint32_t), rows * g->stride0 * sizeof(uint32_t), st));
	const uint32_t words = (uint32_t)((rows + 8191) / 8192 * 256);
	if (words != g->vis_words) {  // (all zero between searches: nothing to keep)
		HIP_TRY(g, dev_regrow(g->d_visited, 0, (size_t)g->slots * words * sizeof(uint32_t), st, true));
		g->vis_words = words;
	}
	if (g->resident)
		HIP_TRY(g, g->arrays.grow_rows(n, rows, st));
	g->cap_rows = rows;
	return g->resident ? graph_size_derived(g) : EXPANN_OK;
}

// the upper-layer arrays laid out again for at least U_need vertices and L_need layers
int graph_grow_upper(expann_graph* g, size_t U_need, size_t L_need) {
	const BuilderArrays& a = g->arrays;
	if (U_need <= a.U_cap && L_need <= a.L_cap)
		return EXPANN_OK;
	const size_t U_cap = U_need > a.U_cap ? std::max(U_need, a.U_cap + a.U_cap / 2) + 64 : a.U_cap;
	HIP_TRY(g, g->arrays.relayout_upper(g->U, U_cap, L_need > a.L_cap ? L_need + 1 : a.L_cap, g->stream));
	return graph_size_derived(g);
}
}  // namespace

extern "C" {

int expann_graph_reserve(expann_graph* g, size_t n_rows) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (n_rows <= g->cap_rows)
		return EXPANN_OK;
	if (n_rows >= (1ull << 32) - 64)
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_reserve: too many rows");
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));
	if (int rc = graph_grow_rows(g, n_rows))
		return rc;
	if (g->resident) {
		if (int rc = graph_rebuild_tables(g))
			return rc;
	}
	return EXPANN_OK;
}

int expann_graph_adopt_build_state(expann_graph* g, size_t M, size_t M0, size_t ef_construction, size_t prune_overflow,
                                   float ortho_factor, float ortho_bias, const uint8_t* levels, const int32_t* upper_idx,
                                   const uint32_t* ids0, const float* d0, const uint32_t* deg0, size_t stride0, size_t U,
                                   size_t n_upper_layers, const uint32_t* idsu, const float* du, const uint32_t* degu,
                                   size_t strideu) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	const char* fn = "expann_graph_adopt_build_state: ";
	if (g->rows_f16)
		return g->fail(EXPANN_ERR_UNSUPPORTED, std::string(fn) + "the builder works on fp32 rows, the handle holds binary16");
	if (g->vis_words == 0)
		return g->fail(EXPANN_ERR_UNSUPPORTED, std::string(fn) + "needs the visited bitsets (at most 8 Mi rows)");
	const size_t n = g->n;
	if (!levels || !upper_idx || !ids0 || !d0 || !deg0 || M < 2 || M0 < M || stride0 < M0 || strideu < M ||
	    (U && n_upper_layers && (!idsu || !du || !degu)) || ef_construction == 0 || ef_construction > (size_t)kPruneMaxCand ||
	    stride0 > (size_t)kPruneMaxCand || strideu > (size_t)kPruneMaxCand || n_upper_layers + 1 < g->n_layers)
		return g->fail(EXPANN_ERR_INVALID_ARG, std::string(fn) + "bad arguments (ef_construction and row strides <= 1024)");
	// (what graph_size_derived would refuse, refused before anything of the handle changes)
	if (g->cap_rows * M0 + (U + U / 2 + 128) * (g->n_layers + 1) * M >= (1ull << 32))
		return g->fail(EXPANN_ERR_UNSUPPORTED, std::string(fn) + "the capacity would take more than 2^32 edges");
	// what the kernels index by: every id, level, upper row and degree, checked once here as expann_graph_create
	// checks its CSR -- a row holds at most M0 / M edges, which is also what the tables' capacities count on
	for (size_t v = 0; v < n; ++v) {
		bool ok = deg0[v] <= M0 && levels[v] < g->n_layers;
		for (uint32_t i = 0; ok && i < deg0[v]; ++i)
			ok = ids0[v * stride0 + i] < n;
		if (ok && levels[v] >= 1) {
			ok = upper_idx[v] >= 0 && (size_t)upper_idx[v] < U;
			for (size_t l = 1; ok && l <= levels[v]; ++l) {
				const size_t r = (l - 1) * U + (size_t)upper_idx[v];
				ok = degu[r] <= M;
				for (uint32_t i = 0; ok && i < degu[r]; ++i)
					ok = idsu[r * strideu + i] < n;
			}
		}
		if (!ok)
			return g->fail(EXPANN_ERR_INVALID_ARG, std::string(fn) + "row " + std::to_string(v) + " is not a row of a graph built with these M / M0");
	}
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));
	g->forget<GraphBuildState>();
	g->cfg = BuildConfig{M, M0, ef_construction, prune_overflow, ortho_factor, ortho_bias};
	const size_t cap = g->cap_rows, L_used = g->n_layers - 1;
	hipStream_t st = g->stream;
	HIP_TRY(g, g->arrays.alloc(cap, (uint32_t)stride0, (uint32_t)strideu, 0, 0, st));
	// the host's [layer][U] upper rows go into a first [L_cap][U_cap] layout with room for half again as many upper
	// vertices and one more layer (g->U is still 0: nothing to carry over).  It also sizes the CSR to the capacities
	// (graph_size_derived: the one expann_graph_create made holds n rows exactly).
	if (int rc = graph_grow_upper(g, U + U / 2 + 64, L_used + 1))
		return rc;
	HIP_TRY(g, g->arrays.copy_host<true>(n, levels, upper_idx, ids0, d0, deg0, U, L_used, U, idsu, du, degu, st));
	g->U = U;
	// a batch's scratch, at the largest batch of THE BATCH RULE
	const size_t max_batch = 32768;
	HIP_TRY(g, g->scratch.alloc(2 * max_batch + 64, max_batch, ef_construction, 0, st));
	// the walk's layer-0 table takes rows of up to M0 ids from now on (the stride it has, when that is larger)
	const uint32_t stride_adj = std::max<uint32_t>(g->stride0, (uint32_t)((M0 + 3) / 4 * 4));
	if (stride_adj != g->stride0) {
		DevPtr<uint32_t> adj;
		HIP_TRY(g, hipMalloc(&adj, cap * stride_adj * sizeof(uint32_t)));
		g->d_adj0 = std::move(adj);
		g->stride0 = stride_adj;
	}
	g->resident = true;
	return graph_rebuild_tables(g);
}

int expann_graph_append(expann_graph* g, const float* rows, size_t n, const uint8_t* levels, uint32_t* max_layer_out,
                        uint32_t* starting_vertex_out, size_t* n_appended) {
	if (n_appended)
		*n_appended = 0;
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (n && (!rows || !levels))
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_append: NULL pointer");
	if (!g->resident)
		return g->fail(EXPANN_ERR_NOT_BUILT, "expann_graph_append before expann_graph_adopt_build_state");
	if (g->n + n >= (1ull << 32) - 64)
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_append: too many rows");
	if (max_layer_out)
		*max_layer_out = g->n_layers;
	if (starting_vertex_out)
		*starting_vertex_out = g->starting_vertex;
	if (n == 0)
		return EXPANN_OK;
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));  // (searches in flight read the tables this call remakes)
	g->forget<GraphRowFilter>();
	g->forget<GraphRowGroups>();
	g->forget<GraphRowBytes>();
	const size_t n_old = g->n, need = n_old + n;
	if (need > g->cap_rows) {  // a full handle grows by half
		if (int rc = graph_grow_rows(g, std::max(need, g->cap_rows + g->cap_rows / 2)))
			return rc;
		++g->stat_append.reallocs;
	}
	std::vector<int32_t> up(n, -1);
	size_t U_new = g->U, L_need = g->n_layers - 1;
	for (size_t i = 0; i < n; ++i) {
		if (levels[i] >= 1)
			up[i] = (int32_t)U_new++;
		L_need = std::max<size_t>(L_need, levels[i]);
	}
	if (int rc = graph_grow_upper(g, U_new, L_need))
		return rc;
	hipStream_t st = g->stream;
	HIP_TRY(g, hipMemcpyAsync(g->d_vectors.as<float>() + n_old * (size_t)g->dim, rows, n * (size_t)g->dim * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(g, hipMemcpyAsync(g->arrays.level.get() + n_old, levels, n, hipMemcpyHostToDevice, st));
	HIP_TRY(g, hipMemcpyAsync(g->arrays.upper_idx.get() + n_old, up.data(), n * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(g, hipMemsetAsync(g->arrays.deg0.get() + n_old, 0, n * 4, st));
	HIP_TRY(g, hipMemsetAsync(g->scratch.ctr, 0, 8 * 4, st));
	BuildBatches r = build_batches(graph_build_view(g), g->scratch, g->cfg, st, g->dim, g->device);
	r.g.n = (uint32_t)need;
	r.levels = levels;
	r.level_base = n_old;
	r.b0 = n_old;
	r.n = need;
	r.max_layer = g->n_layers;
	r.starting_vertex = g->starting_vertex;
	r.vis_bits = g->d_visited.as<uint32_t>();  // (the walk's sets: all zero between searches, and none is in flight)
	r.vis_words = g->vis_words;
	r.resident = true;
	if (int rc = build_batches_geometry(g, r, true))
		return rc;
	r.slots = std::min<uint64_t>(r.slots, g->slots);
	const int brc = build_run_batches(g, r);
	if (brc != EXPANN_OK && brc != EXPANN_ERR_OVERFLOW)
		return brc;
	// the rows of the batches that are in (all of them, unless a construction search overflowed)
	const size_t done = r.b0 - n_old;
	for (size_t i = 0; i < done; ++i)
		g->U += levels[i] >= 1;
	g->n = r.b0;
	g->n_layers = r.max_layer;
	g->starting_vertex = r.starting_vertex;
	g->max_degree0 = std::max<uint32_t>(g->max_degree0, (uint32_t)g->cfg.M0);
	const std::string overflow = g->err;
	if (int rc = graph_rebuild_tables(g))
		return rc;
	++g->stat_append.calls;
	g->stat_append.rows += done;
	g->stat_append.batches += r.n_batches;
	++g->stat_append.device;
	if (n_appended)
		*n_appended = done;
	if (max_layer_out)
		*max_layer_out = g->n_layers;
	if (starting_vertex_out)
		*starting_vertex_out = g->starting_vertex;
	return brc == EXPANN_OK ? EXPANN_OK : g->fail(brc, overflow);
}

int expann_graph_build_state_shape(expann_graph* g, size_t* shape) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!shape)
		return g->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	if (!g->resident)
		return g->fail(EXPANN_ERR_NOT_BUILT, "no builder state: expann_graph_adopt_build_state first");
	shape[0] = g->n;
	shape[1] = g->arrays.U_cap;
	shape[2] = g->n_layers - 1;
	shape[3] = g->U;
	shape[4] = g->arrays.stride0;
	shape[5] = g->arrays.strideu;
	return EXPANN_OK;
}

int expann_graph_read_build_state(expann_graph* g, uint8_t* levels, int32_t* upper_idx, uint32_t* ids0, float* d0,
                                  uint32_t* deg0, uint32_t* idsu, float* du, uint32_t* degu) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!g->resident)
		return g->fail(EXPANN_ERR_NOT_BUILT, "no builder state: expann_graph_adopt_build_state first");
	const size_t L_used = g->n_layers - 1, U_cap = g->arrays.U_cap;
	if (!levels || !upper_idx || !ids0 || !d0 || !deg0 || (L_used * U_cap && (!idsu || !du || !degu)))
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_read_build_state: NULL pointer");
	HIP_TRY(g, hipSetDevice(g->device));
	// the device's layout as it is: whole layers of U_cap rows (expann_graph_build_state_shape reports U_cap as the stride)
	HIP_TRY(g, g->arrays.copy_host<false>(g->n, levels, upper_idx, ids0, d0, deg0, U_cap, L_used, U_cap, idsu, du, degu, g->stream));
	return EXPANN_OK;
}

// carried: the six append counters of the handle the host route replaced, in GraphStats::Appends' order
int expann_graph_note_host_append(expann_graph* g, const uint64_t* carried, size_t rows) {
	static_assert(sizeof(GraphStats::Appends) == 6 * sizeof(uint64_t), "carried[6]: one word per field of Appends");
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (carried)
		std::memcpy(&g->stat_append, carried, sizeof(g->stat_append));
	++g->stat_append.calls;
	g->stat_append.rows += rows;
	++g->stat_append.host;
	return EXPANN_OK;
}

// ---- rows taken out of a built graph (THE GRAPH REMOVE RULE, graph_remove.hpp) ----------------------------------
namespace {
// One expann_graph_remove: what its phases hand on.  Everything here is the call's own; the handle changes in
// graph_remove_repair (rows re-pruned in place) and graph_remove_compact_swap, and nowhere before.
struct GraphRemoval {
	size_t n = 0, keep_cap = 0, task_cap = 0;
	uint32_t chunk = 0;                // tasks per gather + prune launch: lists of at most 16384 x 1024 x 8 bytes
	KeepBitmap rows, upper;            // over the rows; over the upper rows (by upper_idx)
	DevPtr<uint32_t> ctr;              // {touched rows, truncated rows, the top key's two words}
	DevPtr<PruneTask> tasks;           // [task_cap] the touched rows
	DevBuf d_ids;
	OwnedEvent ev[4];                  // around the touch pass; around gather + prune
	RemoveView rv{};
	dim3 entry_grid;
	// read at the early wait
	size_t n_new = 0, U_new = 0, n_touched = 0;
	uint32_t top_level = 0, start_new = 0;
	// built aside
	DevPtr<void> vec;
	BuilderArrays arrays;
	DevPtr<md_pair> lists;             // [chunk][keep_cap]
	DevPtr<uint32_t> list_cnt, chunk_cnt;
	std::vector<uint32_t> h_chunk;     // tasks of every chunk
};

// both keep bitmaps with their ranks, the touched rows as tasks, the key of the new top: all enqueued, nothing read
int graph_remove_mark_rank(expann_graph* g, const uint64_t* ids, size_t n_ids, GraphRemoval& r) {
	hipStream_t st = g->stream;
	HIP_TRY(g, r.rows.alloc(r.n, st));
	HIP_TRY(g, r.upper.alloc(g->U, st));
	HIP_TRY(g, hipMalloc(&r.ctr, sizeof(uint32_t) * 4));
	HIP_TRY(g, hipMalloc(&r.tasks, sizeof(PruneTask) * r.task_cap));
	HIP_TRY(g, r.d_ids.alloc(sizeof(uint64_t) * n_ids));
	for (OwnedEvent& e : r.ev)
		HIP_TRY(g, hipEventCreate(&e));
	HIP_TRY(g, hipMemsetAsync(r.ctr, 0, sizeof(uint32_t) * 4, st));
	HIP_TRY(g, r.rows.all_ones(st));
	HIP_TRY(g, r.upper.all_ones(st));
	HIP_TRY(g, hipMemcpyAsync(r.d_ids.p, ids, sizeof(uint64_t) * n_ids, hipMemcpyHostToDevice, st));
	r.rows.mark_ids(r.d_ids.as<const uint64_t>(), n_ids, st);
	r.rows.count_rank(st);
	r.rv = RemoveView{graph_build_view(g), g->n_layers, r.rows.bits(), r.rows.word_rank(), r.upper.bits(), r.upper.word_rank()};
	const dim3 row_grid((uint32_t)((r.n + kBlock - 1) / kBlock));
	r.entry_grid = dim3((uint32_t)(((uint64_t)g->n_layers * r.n + kBlock / 16 - 1) / (kBlock / 16)));
	hipLaunchKernelGGL(graph_remove_mark_upper_kernel, row_grid, dim3(kBlock), 0, st, r.rv, r.upper.bits());
	r.upper.count_rank(st);
	HIP_TRY(g, hipEventRecord(r.ev[0], st));
	hipLaunchKernelGGL(graph_remove_touch_kernel, r.entry_grid, dim3(kBlock), 0, st, r.rv, r.tasks.get(), (uint32_t)r.task_cap,
	                   r.chunk, r.ctr.get());
	HIP_TRY(g, hipEventRecord(r.ev[1], st));
	hipLaunchKernelGGL(graph_remove_top_kernel, dim3(std::min<uint32_t>(row_grid.x, 1024)), dim3(kBlock), 0, st, r.rv,
	                   (unsigned long long*)(r.ctr.get() + 2));
	HIP_TRY(g, hipGetLastError());
	return EXPANN_OK;
}

// the call's one early host wait, and what it can refuse: nothing of the handle has changed yet.  Then everything built
// aside -- the rows, the builder's arrays at the handle's capacities, a chunk's lists -- is allocated, before the first
// row changes
int graph_remove_wait(expann_graph* g, GraphRemoval& r) {
	hipStream_t st = g->stream;
	uint32_t seen[4] = {0, 0, 0, 0}, useen[4] = {0, 0, 0, 0}, h_ctr[4] = {0, 0, 0, 0};
	HIP_TRY(g, hipMemcpyAsync(seen, r.rows.stat(), sizeof(seen), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipMemcpyAsync(useen, r.upper.stat(), sizeof(useen), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipMemcpyAsync(h_ctr, r.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipStreamSynchronize(st));
	if (seen[2])
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_remove: an id at or beyond the graph's size");
	r.n_new = seen[0], r.U_new = useen[0], r.n_touched = h_ctr[0];
	if (r.n_new == 0)
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_remove: would leave no row (a graph is never empty)");
	if (r.n_touched > r.task_cap)
		return g->fail(EXPANN_ERR_HIP, "expann_graph_remove: more touched rows than rows");
	r.top_level = h_ctr[3], r.start_new = 0xFFFFFFFFu - h_ctr[2];
	const size_t n_chunks = (r.n_touched + r.chunk - 1) / r.chunk;
	HIP_TRY(g, hipMalloc(&r.vec, g->cap_rows * (size_t)g->dim * 4));
	HIP_TRY(g, hipMalloc(&r.lists, std::max<size_t>((size_t)r.chunk * r.keep_cap, 1) * sizeof(md_pair)));
	HIP_TRY(g, hipMalloc(&r.list_cnt, std::max<size_t>(r.chunk, 1) * 4));
	r.h_chunk.assign(std::max<size_t>(n_chunks, 1), 0);
	for (size_t c = 0; c < n_chunks; ++c)
		r.h_chunk[c] = (uint32_t)std::min<size_t>(r.chunk, r.n_touched - c * r.chunk);
	HIP_TRY(g, hipMalloc(&r.chunk_cnt, r.h_chunk.size() * 4));
	HIP_TRY(g, hipMemcpyAsync(r.chunk_cnt, r.h_chunk.data(), r.h_chunk.size() * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(g, r.arrays.alloc(g->cap_rows, g->arrays.stride0, g->arrays.strideu, g->arrays.U_cap, g->arrays.L_cap, st));
	return EXPANN_OK;
}

// the touched rows gathered and pruned in place, a chunk of tasks at a time over one list buffer
int graph_remove_repair(expann_graph* g, GraphRemoval& r) {
	hipStream_t st = g->stream;
	const BuildVariant* bv = build_variant(g->dim);
	const uint32_t cus = (uint32_t)num_cus(g->device);
	const size_t n_chunks = (r.n_touched + r.chunk - 1) / r.chunk;
	HIP_TRY(g, hipEventRecord(r.ev[2], st));
	for (size_t c = 0; c < n_chunks; ++c) {
		RemoveGatherParams gp{};
		gp.r = r.rv;
		gp.tasks = r.tasks.get() + c * r.chunk;
		gp.n_tasks = r.h_chunk[c];
		gp.keep_cap = (uint32_t)r.keep_cap;
		gp.lists = r.lists;
		gp.list_cnt = r.list_cnt;
		gp.n_truncated = r.ctr.get() + 1;
		gp.dim = (uint32_t)g->dim;
		hipLaunchKernelGGL(graph_remove_gather_kernel, dim3(std::min<uint32_t>(r.h_chunk[c], cus * 8)), dim3(kBlock), 0, st, gp);
		BuildPruneParams pp{};
		pp.g = r.rv.g;
		pp.tasks = gp.tasks;
		pp.n_tasks = r.chunk_cnt.get() + c;
		pp.lists = r.lists;
		pp.list_cnt = r.list_cnt;
		pp.ef = (uint32_t)r.keep_cap;
		pp.ortho_factor = g->cfg.ortho_factor;
		pp.ortho_bias = g->cfg.ortho_bias;
		pp.prune_overflow = (uint32_t)g->cfg.prune_overflow;
		pp.dim = (uint32_t)g->dim;
		hipLaunchKernelGGL(bv->prune, dim3(std::min<uint32_t>(r.h_chunk[c], cus * 16)), dim3(kPruneThreads),
		                   bv->d == 0 ? (size_t)g->dim * sizeof(float) : 0, st, pp);
	}
	HIP_TRY(g, hipEventRecord(r.ev[3], st));
	return EXPANN_OK;
}

// the survivors' rows and graph rows written aside under their new ids, waited for, and moved into the handle; the
// walk's tables remade
int graph_remove_compact_swap(expann_graph* g, GraphRemoval& r) {
	hipStream_t st = g->stream;
	const CompactRowsParams cp{r.rows.bits(), r.rows.word_rank(), g->d_vectors.as<const uint4>(), r.vec.as<uint4>(),
	                           (uint32_t)((size_t)g->dim * 4 / 16)};  // (no row terms carried along)
	hipLaunchKernelGGL(compact_rows_kernel, dim3((uint32_t)(r.rows.words / 4)), dim3(kBlock), 0, st, cp);
	const BuilderArrays& to = r.arrays;
	const RemoveCompactParams rc{r.rv, to.level, to.upper_idx, to.id0, to.d0, to.deg0, to.idu, to.du, to.degu};
	hipLaunchKernelGGL(graph_remove_compact_kernel, r.entry_grid, dim3(kBlock), 0, st, rc);
	HIP_TRY(g, hipGetLastError());
	uint32_t h_ctr[4] = {0, 0, 0, 0};
	HIP_TRY(g, hipMemcpyAsync(h_ctr, r.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
	HIP_TRY(g, hipStreamSynchronize(st));
	float ms_touch = 0, ms_repair = 0;
	HIP_TRY(g, hipEventElapsedTime(&ms_touch, r.ev[0], r.ev[1]));
	HIP_TRY(g, hipEventElapsedTime(&ms_repair, r.ev[2], r.ev[3]));
	g->d_vectors = std::move(r.vec);
	g->arrays = std::move(r.arrays);
	g->n = r.n_new;
	g->U = r.U_new;
	g->n_layers = r.top_level + 1;
	g->starting_vertex = r.start_new;
	if (int rc2 = graph_rebuild_tables(g))
		return rc2;
	g->remove_repair_ns = (uint64_t)(((double)ms_touch + (double)ms_repair) * 1e6);
	g->stat_remove.truncated += h_ctr[1];
	return EXPANN_OK;
}
}  // namespace

int expann_graph_remove(expann_graph* g, const uint64_t* ids, size_t n_ids, uint32_t* max_layer_out,
                        uint32_t* starting_vertex_out, size_t* n_removed) {
	if (n_removed)
		*n_removed = 0;
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (n_ids && !ids)
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_remove: ids == NULL");
	if (!g->resident)
		return g->fail(EXPANN_ERR_NOT_BUILT, "expann_graph_remove before expann_graph_adopt_build_state");
	if (max_layer_out)
		*max_layer_out = g->n_layers;
	if (starting_vertex_out)
		*starting_vertex_out = g->starting_vertex;
	if (n_ids == 0)
		return EXPANN_OK;
	GraphRemoval r;
	r.keep_cap = std::max(g->cfg.ef_construction, g->cfg.M0);
	if (r.keep_cap > (size_t)kPruneMaxCand || g->n >= (1ull << 32) - 64)
		return g->fail(EXPANN_ERR_UNSUPPORTED, "expann_graph_remove: max(ef_construction, M0) <= 1024");
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, graph_wait_outstanding(g));  // (searches in flight read the tables this call remakes)
	r.n = g->n;
	r.task_cap = r.n + (g->n_layers - 1) * g->U;
	if ((uint64_t)g->n_layers * r.n >= (1ull << 32) * (kBlock / 16))
		return g->fail(EXPANN_ERR_UNSUPPORTED, "expann_graph_remove: too many rows");
	r.chunk = (uint32_t)std::min<size_t>(r.task_cap, 16384);
	if (int rc = graph_remove_mark_rank(g, ids, n_ids, r))
		return rc;
	if (int rc = graph_remove_wait(g, r))
		return rc;
	// from here on the handle changes
	g->forget<GraphRowFilter>();
	g->forget<GraphRowGroups>();
	g->forget<GraphRowBytes>();
	if (int rc = graph_remove_repair(g, r))
		return rc;
	if (int rc = graph_remove_compact_swap(g, r))
		return rc;
	++g->stat_remove.calls;
	g->stat_remove.rows += r.n - r.n_new;
	g->stat_remove.touched += r.n_touched;
	++g->stat_remove.device;
	if (n_removed)
		*n_removed = r.n - r.n_new;
	if (max_layer_out)
		*max_layer_out = g->n_layers;
	if (starting_vertex_out)
		*starting_vertex_out = g->starting_vertex;
	return EXPANN_OK;
}

// carried: the six remove counters in GraphStats::Removes' order, remove_repair_ns, then the six append counters
int expann_graph_note_host_remove(expann_graph* g, const uint64_t* carried, size_t rows) {
	static_assert(sizeof(GraphStats::Removes) == 6 * sizeof(uint64_t) && 6 + 1 + sizeof(GraphStats::Appends) / sizeof(uint64_t) == 13,
	              "carried[13]: one word per field of Removes, remove_repair_ns, one per field of Appends");
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (carried) {
		std::memcpy(&g->stat_remove, carried, sizeof(g->stat_remove));
		g->remove_repair_ns = carried[6];
		std::memcpy(&g->stat_append, carried + 7, sizeof(g->stat_append));
	}
	++g->stat_remove.calls;
	g->stat_remove.rows += rows;
	++g->stat_remove.host;
	return EXPANN_OK;
}

int expann_graph_read_row_filter(expann_graph* g, uint32_t* allow_bits, size_t n_words) {
	if (!g)
		return EXPANN_ERR_INVALID_ARG;
	if (!g->filter_on)
		return g->fail(EXPANN_ERR_INVALID_ARG, "no row filter in force");
	const size_t words = (g->n + 31) / 32;
	if (!allow_bits || n_words < words)
		return g->fail(EXPANN_ERR_INVALID_ARG, "expann_graph_read_row_filter: NULL pointer or too few words");
	HIP_TRY(g, hipSetDevice(g->device));
	HIP_TRY(g, hipMemcpy(allow_bits, g->d_allow, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return EXPANN_OK;
}

// ---- the graph engine behind one handle (host build + device queries) --------------------
}  // extern "C"

#include "expann/gpu_antitopo_engine.h"

struct expann_antitopo {
	gpu_antitopo_engine<float>* eng = nullptr;
	int dim = 0;
	mutable std::string err;
	int fail(int code, const std::string& msg) const {
		err = msg;
		return code;
	}
};

#define ANTITOPO_TRY(e, body)                                              \
	try {                                                                  \
		body;                                                              \
	} catch (const std::exception& ex) {                                   \
		return (e)->fail(EXPANN_ERR_INVALID_ARG, ex.what());               \
	}

extern "C" {

int expann_antitopo_create(int dim, int device, size_t M, size_t ef_construction,
                           size_t ortho_count, size_t prune_overflow, int use_compression,
                           expann_antitopo** out) {
	if (!out || dim <= 0 || dim % 16 != 0 || M < 2 || ef_construction == 0) {
		g_create_error = "expann_antitopo_create: bad arguments (dim % 16 == 0, M >= 2)";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (int rc = graph_dim_error("expann_antitopo_create", dim))
		return rc;
	if (use_compression && dim % 64 != 0) {  // (the uint8 walk works in 64-dim blocks)
		g_create_error = "expann_antitopo_create: use_compression needs dim % 64 == 0";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (expann_device_count() <= 0) {
		g_create_error = "no HIP device visible: libexpann_hip has no CPU fallback";
		return EXPANN_ERR_NO_DEVICE;
	}
	gpu_antitopo_engine_config cfg(M, 2 * M, 1, ef_construction, ortho_count, 0.5f, 0.0f,
	                               prune_overflow, use_compression != 0);
	cfg.device = device;
	expann_antitopo* e = new expann_antitopo();
	e->dim = dim;
	e->eng = new gpu_antitopo_engine<float>(cfg);
	e->eng->index.dim = (size_t)dim;
	*out = e;
	return EXPANN_OK;
}

void expann_antitopo_destroy(expann_antitopo* e) {
	if (!e)
		return;
	delete e->eng;
	delete e;
}

const char* expann_antitopo_last_error(const expann_antitopo* e) {
	return e ? e->err.c_str() : g_create_error.c_str();
}

int expann_antitopo_store(expann_antitopo* e, const float* rows, size_t n) {
	if (!e || (!rows && n))
		return EXPANN_ERR_INVALID_ARG;
	e->eng->clear_row_filter();
	e->eng->clear_row_groups();
	ANTITOPO_TRY(e, e->eng->store_rows(rows, n));
	return EXPANN_OK;
}

int expann_antitopo_store_batched(expann_antitopo* e, const float* rows, size_t n, size_t n_serial) {
	if (!e || (!rows && n))
		return EXPANN_ERR_INVALID_ARG;
	e->eng->clear_row_filter();
	e->eng->clear_row_groups();
	ANTITOPO_TRY(e, e->eng->store_rows_batched(rows, n, n_serial ? n_serial : 2048));
	return EXPANN_OK;
}

int expann_antitopo_set_rows_f16(expann_antitopo* e, int on) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (e->eng->index.size() != 0)
		return e->fail(EXPANN_ERR_INVALID_ARG, "expann_antitopo_set_rows_f16: the engine already holds rows");
	e->eng->conf.rows_f16 = on != 0;
	return EXPANN_OK;
}

int expann_antitopo_build(expann_antitopo* e) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	ANTITOPO_TRY(e, e->eng->_build());
	return EXPANN_OK;
}

int expann_antitopo_set_ef_search(expann_antitopo* e, size_t ef_search) {
	if (!e || ef_search == 0)
		return EXPANN_ERR_INVALID_ARG;
	e->eng->set_ef_search(ef_search);
	return EXPANN_OK;
}

int expann_antitopo_query(expann_antitopo* e, const float* queries, size_t m, size_t k,
                          uint64_t* ids, float* dists) {
	if (!e || !queries || !ids || !dists || k == 0)
		return e ? e->fail(EXPANN_ERR_INVALID_ARG, "bad arguments") : EXPANN_ERR_INVALID_ARG;
	ANTITOPO_TRY(e, e->eng->query_k_batch(queries, m, k, ids, dists));
	return EXPANN_OK;
}

int expann_antitopo_query_device(expann_antitopo* e, const float* d_queries, size_t m, size_t k, uint64_t* d_ids,
                                 float* d_dists, void* stream) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_query_device before build()");
	const int rc = e->eng->query_k_batch_device(d_queries, m, k, d_ids, d_dists, stream);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_sync(expann_antitopo* e) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_sync before build()");
	const int rc = e->eng->sync();
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_set_row_filter(expann_antitopo* e, const uint32_t* allow_bits_or_NULL, size_t n_words) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_set_row_filter before build()");
	const int rc = e->eng->set_row_filter(allow_bits_or_NULL, n_words);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_set_row_filter_device(expann_antitopo* e, const uint32_t* d_allow_bits, size_t n_words, void* stream) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_set_row_filter_device before build()");
	const int rc = e->eng->set_row_filter_device(d_allow_bits, n_words, stream);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_set_row_groups(expann_antitopo* e, const uint32_t* groups_or_NULL, size_t n) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_set_row_groups before build()");
	const int rc = e->eng->set_row_groups(groups_or_NULL, n);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_set_row_groups_device(expann_antitopo* e, const uint32_t* d_groups, size_t n, void* stream) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_set_row_groups_device before build()");
	const int rc = e->eng->set_row_groups_device(d_groups, n, stream);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_query_grouped(expann_antitopo* e, const float* queries, const uint32_t* query_groups, size_t m,
                                  size_t k, uint64_t* ids, float* dists) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_query_grouped before build()");
	const int rc = e->eng->query_k_batch_grouped(queries, query_groups, m, k, ids, dists);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_query_grouped_device(expann_antitopo* e, const float* d_queries, const uint32_t* d_query_groups,
                                         size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_query_grouped_device before build()");
	const int rc = e->eng->query_k_batch_grouped_device(d_queries, d_query_groups, m, k, d_ids, d_dists, stream);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_range_query(expann_antitopo* e, const float* queries, const float* radii, size_t m,
                                size_t max_results, uint64_t* ids, float* dists, uint32_t* counts) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_range_query before build()");
	const int rc = e->eng->range_query_batch(queries, radii, m, max_results, ids, dists, counts);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_range_query_device(expann_antitopo* e, const float* d_queries, const float* d_radii, size_t m,
                                       size_t max_results, uint64_t* d_ids, float* d_dists, uint32_t* d_counts,
                                       void* stream) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_range_query_device before build()");
	const int rc = e->eng->range_query_batch_device(d_queries, d_radii, m, max_results, d_ids, d_dists, d_counts, stream);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_save(expann_antitopo* e, const char* index_path) {
	if (!e || !index_path)
		return EXPANN_ERR_INVALID_ARG;
	ANTITOPO_TRY(e, e->eng->save_index(index_path));  // (after an append: the adjacency comes back from the device first)
	return EXPANN_OK;
}

int expann_antitopo_append(expann_antitopo* e, const float* rows, size_t n, size_t* n_appended) {
	if (n_appended)
		*n_appended = 0;
	if (!e || (!rows && n))
		return e ? e->fail(EXPANN_ERR_INVALID_ARG, "expann_antitopo_append: rows == NULL") : EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_append before build()");
	int rc = EXPANN_OK;
	ANTITOPO_TRY(e, rc = e->eng->append_rows(rows, n, n_appended));
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_remove(expann_antitopo* e, const uint64_t* ids, size_t n_ids, size_t* n_removed) {
	if (n_removed)
		*n_removed = 0;
	if (!e || (!ids && n_ids))
		return e ? e->fail(EXPANN_ERR_INVALID_ARG, "expann_antitopo_remove: ids == NULL") : EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_remove before build()");
	int rc = EXPANN_OK;
	ANTITOPO_TRY(e, rc = e->eng->remove_rows(ids, n_ids, n_removed));
	const std::string& why = e->eng->remove_error;
	return rc == EXPANN_OK ? rc : e->fail(rc, why.empty() ? expann_graph_last_error(e->eng->graph) : why);
}

int expann_antitopo_compact_row_filter(expann_antitopo* e, size_t* n_removed) {
	if (n_removed)
		*n_removed = 0;
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_compact_row_filter before build()");
	int rc = EXPANN_OK;
	ANTITOPO_TRY(e, rc = e->eng->compact_row_filter(n_removed));
	const std::string& why = e->eng->remove_error;
	return rc == EXPANN_OK ? rc : e->fail(rc, why.empty() ? expann_graph_last_error(e->eng->graph) : why);
}

int expann_antitopo_reserve(expann_antitopo* e, size_t n_rows) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_reserve before build()");
	const int rc = e->eng->reserve(n_rows);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_get_stat(expann_antitopo* e, const char* name, uint64_t* out) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (!name || !out)
		return e->fail(EXPANN_ERR_INVALID_ARG, "NULL pointer");
	if (!e->eng->graph)
		return e->fail(EXPANN_ERR_NOT_BUILT, "expann_antitopo_get_stat before build()");
	const int rc = expann_graph_get_stat(e->eng->graph, name, out);
	return rc == EXPANN_OK ? rc : e->fail(rc, expann_graph_last_error(e->eng->graph));
}

int expann_antitopo_load(expann_antitopo* e, const char* index_path) {
	if (!e || !index_path)
		return EXPANN_ERR_INVALID_ARG;
	ANTITOPO_TRY(e, {
		e->eng->index.read_index(index_path);
		if ((int)e->eng->index.dim != e->dim)
			throw std::runtime_error("index dimension differs from the engine's");
		e->eng->upload();
	});
	return EXPANN_OK;
}

int expann_antitopo_set_compression(expann_antitopo* e, int mode) {
	if (!e)
		return EXPANN_ERR_INVALID_ARG;
	if (mode < EXPANN_GRAPH_FP32 || mode > EXPANN_GRAPH_RANGED_Q8)
		return e->fail(EXPANN_ERR_INVALID_ARG, "mode must be 0 (fp32), 1 (uint8 cast) or 2 (ranged int8)");
	if (mode != EXPANN_GRAPH_FP32 && e->dim % 64 != 0)  // (both byte walks work in 64-dim blocks)
		return e->fail(EXPANN_ERR_INVALID_ARG, "a compressed bottom layer needs dim % 64 == 0");
	e->eng->conf.compression_mode = mode;
	return EXPANN_OK;
}

size_t expann_antitopo_size(const expann_antitopo* e) { return e ? e->eng->index.size() : 0; }
uint64_t expann_antitopo_num_distcomps(const expann_antitopo* e) {
	return e ? e->eng->num_distcomps : 0;
}

int expann_quantize_simple_u8_device(int device, const float* d_rows, size_t n_values,
                                     uint8_t* d_out, void* stream) {
	if (!d_rows || !d_out) {
		g_create_error = "expann_quantize_simple_u8_device: NULL pointer";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (n_values == 0)
		return EXPANN_OK;
	if (hipSetDevice(device) != hipSuccess) {
		g_create_error = "hipSetDevice failed";
		return EXPANN_ERR_HIP;
	}
	launch_quantize_simple_u8(d_rows, n_values, d_out, (hipStream_t)stream);
	if (hipGetLastError() != hipSuccess) {
		g_create_error = "quantize_simple_u8_kernel launch failed";
		return EXPANN_ERR_HIP;
	}
	return EXPANN_OK;
}

int expann_quantize_ranged_q8_device(int device, const float* d_rows, size_t n_values,
                                     int8_t* d_out, float* d_scale_offset, void* stream) {
	if (!d_rows || !d_out || !d_scale_offset || n_values == 0) {
		g_create_error = "expann_quantize_ranged_q8_device: bad arguments";
		return EXPANN_ERR_INVALID_ARG;
	}
	if (hipSetDevice(device) != hipSuccess) {
		g_create_error = "hipSetDevice failed";
		return EXPANN_ERR_HIP;
	}
	hipStream_t st = (hipStream_t)stream;
	uint32_t* d_mm = nullptr;
	if (hipMalloc(&d_mm, 2 * sizeof(uint32_t)) != hipSuccess) {
		g_create_error = "hipMalloc failed";
		return EXPANN_ERR_HIP;
	}
	const hipError_t e = launch_quantize_ranged_q8(d_rows, n_values, d_mm, d_out, d_scale_offset, st);
	hipFree(d_mm);
	if (e != hipSuccess) {
		g_create_error = std::string("expann_quantize_ranged_q8_device: ") + hipGetErrorString(e);
		return EXPANN_ERR_HIP;
	}
	return EXPANN_OK;
}

}  // extern "C"
