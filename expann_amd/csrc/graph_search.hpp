// graph_search.hpp -- query side of the reference's graph engine on the device:
//   antitopo_engine::_query_k            src/antitopo_engine.h:853-928
//   query_k_at_layer<true,false,false>   src/antitopo_engine.h:495-708   (fp32 bottom layer)
//   query_k_bottom_compressed            src/antitopo_engine.h:710-851   (uint8 bottom layer +
//                                        final fp32 re-score :845-848)
// and the same compressed walk over quantizer_ranged_q8 rows (src/quantizer.h:152-238, never instantiated by
// the reference): MODE kGraphRangedQ8, bytes in [0, 127] from the index's global scale / offset.
// One wavefront (= one 64-thread workgroup) walks one query; workgroups are persistent and pull
// queries round-robin.  The traversal is a dependent chain, so the parallelism inside a query is
// the neighbour batch of a hop: the "visited" tests of a vertex's <= M0 neighbours run one lane
// per neighbour, and their distances are evaluated 4 rows at a time with 16 lanes per row in the
// reference's exact FMA order (common.hpp) -- the same arithmetic as the brute-force scan, so
// every distance, and therefore every branch of the walk, is bit-identical to the CPU code.
// The two priority queues live in LDS and are updated with exactly libstdc++'s push_heap / pop_heap
// element movement (the reference's comparators look at .first only, so the order among equal
// distances is the heap's; integer-valued uint8 distances tie often) -- by the WHOLE WAVE (round 3):
// the path of a sift is known before anything moves (the ancestors of the hole for __push_heap; the
// chain of larger children for __adjust_heap, which libstdc++ walks to a leaf before it looks at the
// value), so one lane per level reads its element, a ballot finds where the value settles and the
// lanes shift their elements in one step: the same final array as the serial code, in ~3 LDS round
// trips instead of ~3 per level (coop_push / coop_pop below; round 2's lane-0 loops took 40-52 % of a
// hop, profiles/r03_c4_hop_breakdown.txt).
// A neighbour that cannot beat the current worst kept distance is dropped before the queue update
// (all lanes test, ballot-compacted in list order): `nearest.top()` only decreases while the queue is
// full, so the sequential test of :666 / :823 would reject it too.
// Visited set (the reference keeps a byte array and a reset list, :208-209, :692-694): a BITSET per
// resident workgroup -- test-and-set by one returning atomicOr, cleared by streaming stores when the
// query ends (cheaper than a reset list's scattered stores up to a few million vertices); beyond 8 M
// vertices one epoch-stamped byte per vertex and workgroup, never cleared (round 2's only form).
#pragma once
#include <type_traits>

#include "common.hpp"
#include "quantize.hpp"
#include "scan_int8.hpp"

namespace expann {

// bottom-layer scoring of the walk (expann_graph_compression): fp32 rows; quantizer_simple<uint8_t> bytes
// (a plain cast); quantizer_ranged_q8 bytes (global affine, [0, 127]).  The last two share everything
// but the conversion of the query.
constexpr int kGraphF32 = 0, kGraphU8Cast = 1, kGraphRangedQ8 = 2;

struct GraphSearchParams {
	const float* vectors;         // [n][D]; TR = _Float16 instances: the same address holds [n][D] binary16 rows
	const uint8_t* compressed;    // [n][D] (quantizer_simple<uint8_t>, or quantizer_ranged_q8 in the ranged mode) or nullptr
	const uint32_t* layer_off;    // [n_layers][n+1] (CSR; the walk uses it for the layers above 0)
	const uint32_t* neighbours;
	const uint32_t* adj0;         // [n][stride0] layer-0 lists at a fixed stride, padded with UINT32_MAX: a
	uint32_t stride0;             // hop reads its list without the dependent round trip for the offsets
	uint32_t n, n_layers, starting_vertex;
	const float* queries;         // [m][D]
	uint32_t m;
	uint32_t k, ef;
	uint32_t cand_cap;            // capacity of the candidates heap (LDS)
	uint32_t max_degree;          // longest neighbour list of layer 0 (<= list_cap)
	uint32_t list_cap;
	uint8_t* visited;             // [gridDim.x][n] epoch bytes, zero-initialised (vis_words == 0)
	uint32_t* epochs;             // [gridDim.x] last epoch used by that workgroup
	// vis_words != 0: the visited set is a BITSET per workgroup, vis_bits[gridDim.x][vis_words] (vis_words a
	// multiple of 256, all zero between queries): test-and-set is one returning atomicOr, the set is
	// cleared with streaming stores when the query ends.  An eighth of the bytes' footprint: at 1 M rows
	// the resident workgroups' sets are 0.4 GB instead of 3-4 GB and mostly live in the Infinity Cache.
	uint32_t* vis_bits;
	uint32_t vis_words;
	uint64_t* out_ids;            // [m][k]
	float* out_dists;             // [m][k]
	uint32_t* out_distcomps;      // [m] or nullptr
	uint32_t* error;              // [1] != 0: a candidates heap overflowed cand_cap
	uint32_t* next_query;         // [1] zero at launch: the workgroups of the (resident) grid pull queries from it
	uint32_t debug;               // bisection switch (EXPANN_GRAPH_DEBUG): 1 = lane 0 runs the serial queue code
	// DBG instance only (profiles/r03_c4_hop_breakdown.txt): stamps[blockIdx.x][8] = shader clocks this
	// workgroup spent in {0 per-query setup + descent, 1 pop + broadcast, 2 adjacency + visited tests,
	// 3 row gathers + scoring, 4 serial queue update, 5 output}, 6 = hops, 7 = queue insertions
	unsigned long long* stamps;
	uint32_t dim;                 // run-time-dim instance (D = 0) only: the row length (the others have it as D)
	float q_scale, q_offset;      // kGraphRangedQ8 only: the rows' quantiser, applied to the query as it is staged
	// Overflow per query, for the redo launch; all inert when nullptr.
	// redo_list != nullptr: a walk that met a full candidates heap appends its query number to
	// redo_list[atomicAdd(redo_count, 1)] instead of raising `error` (its output row is still written).
	uint32_t* redo_list;          // [m]
	uint32_t* redo_count;         // [1] zero at launch
	// query_map != nullptr: the number pulled from next_query indexes query_map, and the bound is *m_dev (at most m).
	// A second launch with query_map = the first one's redo_list and m_dev = its redo_count walks the overflowed
	// queries again at this launch's cand_cap and overwrites their rows; workgroups that find nothing leave after
	// one atomic.
	const uint32_t* query_map;
	const uint32_t* m_dev;
	// != nullptr: every query adds its distcomps (one atomic from one lane); a query put on the redo list does
	// not, the launch that walks it again does
	unsigned long long* distcomps_total;
	// FILTERED instances only (nullptr in unfiltered launches): the row filter, bit v & 31 of word v >> 5 says
	// whether vertex v may appear in a result; the handle's own copy, zero from n on (THE FILTER RULE below)
	const uint32_t* allow_bits;
	// group instances only (THE GROUP RULE below): the label of every row, the group each query names, and the
	// directory made at set time -- the distinct labels ascending (0xFFFFFFFF left out) with their row counts as
	// offsets; flat_rows is "filter_flat_rows" resolved; group_walked counts the queries the first launch walks
	const uint32_t* row_groups;    // [n]
	const uint32_t* query_groups;  // [m]
	const uint32_t* group_keys;    // [n_groups]
	const uint32_t* group_off;     // [n_groups + 1]
	uint32_t n_groups, flat_rows;
	uint32_t* group_walked;        // [1] or nullptr
	// capacity of `nearest` (LDS): ef in every walk but the range walk, whose queue grows to max(ef, max_results)
	uint32_t near_cap;
	// range instances only (THE RANGE WALK RULE below): the radius of every query, the rows a query may return (the
	// stride of out_ids / out_dists; k holds the same number) and the in-range rows each walk scored
	const float* radii;            // [m]
	uint32_t max_results;
	uint32_t* out_counts;          // [m]
};

// what a walk instance is filtered by: nothing, the handle's bitmap (THE FILTER RULE), or row groups (THE GROUP RULE);
// kFilterRange is no filter but the fourth kind of walk: the unfiltered one that keeps what lies within a radius (THE
// RANGE WALK RULE)
constexpr int kFilterNone = 0, kFilterBitmap = 1, kFilterGroups = 2, kFilterRange = 3;
// the group a query names to search every row
constexpr uint32_t kGroupAny = 0xFFFFFFFFu;
// min(k, allowed) the exact scan keeps in LDS; beyond it the search walks.  Not measured: the scan's final ranking reads
// keys^2 / 64 LDS words per lane and each replacement scans keys / 64, so the bound is held where that work (16 k
// reads per lane and query) stays small next to scoring the rows.
constexpr uint32_t kGraphFlatMaxKeys = 1024;

// How a query that names group `qg` (not kGroupAny) is served, decided the same way by the walk and by the scan:
// *gi = the group's place in the directory, *s = its row count (0: no row carries the label).  Wave-uniform: a
// binary search of the ascending keys.
// (The bitmap path's graph_serve has a third clause: a scan whose LDS -- 8 bytes x min(k, rows) keys plus 4 x dim for
// the query -- exceeds the 160 KB a search may take walks instead.  With min(k, rows) <= kGraphFlatMaxKeys and dim <=
// 4096, the graph path's limit, that is at most 24 KB, so the clause can never hold and is not restated here; "bit for
// bit the bitmap path" rests on those two limits.)
constexpr int kGroupServeWalk = 0, kGroupServeScan = 1, kGroupServePad = 2;
__device__ inline int group_serve(const uint32_t* keys, const uint32_t* off, uint32_t n_groups, uint32_t qg, uint32_t k,
                                  uint32_t flat_rows, uint32_t* gi, uint32_t* s) {
	uint32_t lo = 0, hi = n_groups;  // the first key >= qg
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (keys[mid] < qg)
			lo = mid + 1;
		else
			hi = mid;
	}
	*gi = lo;
	*s = 0;
	if (lo == n_groups || keys[lo] != qg)
		return kGroupServePad;
	const uint32_t rows = off[lo + 1] - off[lo];
	*s = rows;
	const uint32_t kk = k < rows ? k : rows;
	return rows <= flat_rows && kk <= kGraphFlatMaxKeys ? kGroupServeScan : kGroupServeWalk;
}

struct md_pair {
	float d;
	uint32_t id;
};

// libstdc++ heap primitives on an LDS array; MAXH: top = largest .d (worst_elem), else smallest
template <bool MAXH> __device__ inline bool md_less(md_pair a, md_pair b) {
	return MAXH ? (a.d < b.d) : (a.d > b.d);
}
template <bool MAXH>
__device__ inline void heap_push_up(md_pair* v, uint32_t hole, uint32_t top, md_pair value) {
	while (hole > top) {
		const uint32_t parent = (hole - 1) / 2;
		if (!md_less<MAXH>(v[parent], value))
			break;
		v[hole] = v[parent];
		hole = parent;
	}
	v[hole] = value;
}
template <bool MAXH>
__device__ inline void heap_adjust(md_pair* v, uint32_t hole, uint32_t len, md_pair value) {
	const uint32_t top = hole;
	uint32_t child = hole;
	while (len > 1 && child < (len - 1) / 2) {
		child = 2 * (child + 1);
		if (md_less<MAXH>(v[child], v[child - 1]))
			--child;
		v[hole] = v[child];
		hole = child;
	}
	if ((len & 1) == 0 && len >= 2 && child == (len - 2) / 2) {
		child = 2 * (child + 1);
		v[hole] = v[child - 1];
		hole = child - 1;
	}
	heap_push_up<MAXH>(v, hole, top, value);
}
template <bool MAXH> __device__ inline void heap_push(md_pair* v, uint32_t& n, md_pair e) {
	v[n] = e;
	heap_push_up<MAXH>(v, n, 0, e);
	++n;
}
template <bool MAXH> __device__ inline void heap_pop(md_pair* v, uint32_t& n) {
	if (n > 1) {
		const md_pair value = v[n - 1];
		v[n - 1] = v[0];
		heap_adjust<MAXH>(v, 0, n - 1, value);
	}
	--n;
}

// min of a 64-bit key over the wave (all lanes get it)
__device__ inline uint64_t wave_min_key64(uint64_t v) {
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
		const uint64_t o = ((uint64_t)hi << 32) | lo;
		v = o < v ? o : v;
	}
	return v;
}

// ---- the queues, updated by the whole wave --------------------------------------------------------
// (every lane calls with the same arguments; n and the results are wave-uniform)
__device__ inline void wave_lds_sync() {  // lanes exchange data through LDS: keep the compiler's order
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// std::__push_heap(first, hole, top = 0, value): lane j reads the j-th ancestor of the hole; the value
// stops in front of the first ancestor that is not "less" than it; the ancestors below move down one.
template <bool MAXH> __device__ inline void coop_push_up(md_pair* v, uint32_t hole, md_pair value, int lane) {
	asm volatile("" : "+v"(lane));  // (opaque: the lanes' heap addresses are formed here -- hoisted out of the hop loop they
	                                // spilled in the 128-register uint8 instance, a scratch round trip per queue update)
	const uint32_t h1 = hole + 1;
	const int levels = 31 - __builtin_clz(h1);  // ancestors of the hole
	const bool act = lane < levels;
	const md_pair x = v[act ? (h1 >> ((lane + 1) & 31)) - 1 : 0];
	// (every lane's element is in its registers before any lane stores: without the fence the compiler
	// sinks the load of x.id -- the ballot only needs x.d -- into the branch that uses it, behind another
	// lane's store to the same slot)
	wave_lds_sync();
	const unsigned long long stops = __builtin_amdgcn_ballot_w64(act && !md_less<MAXH>(x, value));
	const int stop = stops ? __builtin_ctzll(stops) : levels;
	const uint32_t pos = (h1 >> (lane & 31)) - 1;  // lane 0: the hole; lane j: ancestor j - 1 (lanes <= stop <= 31 write)
	if (lane < stop)
		v[pos] = x;
	else if (lane == stop)
		v[pos] = value;
}
template <bool MAXH> __device__ inline void coop_push(md_pair* v, uint32_t& n, md_pair e, int lane, uint32_t serial = 0) {
	if (serial) {
		wave_lds_sync();
		if (lane == 0) {
			v[n] = e;
			heap_push_up<MAXH>(v, n, 0, e);
		}
		wave_lds_sync();
	} else {
		coop_push_up<MAXH>(v, n, e, lane);
	}
	++n;
}

// std::__adjust_heap(first, hole = 0, len, value) for len <= 128 * NPL + 1: lane i (+ 64 s) compares the
// two children of node i, the chain of larger children is followed with readlanes (one per level),
// then -- as libstdc++ does -- the value is pushed up from the leaf along that very chain: lane t holds
// the chain's element t + 1, a ballot finds where the value settles.
template <bool MAXH, int NPL>
__device__ inline void coop_adjust(md_pair* v, uint32_t len, md_pair value, int lane) {
	asm volatile("" : "+v"(lane));  // (opaque, as in coop_push_up)
	const uint32_t half = (len - 1) / 2;  // nodes < half have two children
	uint32_t big[NPL];
#pragma unroll
	for (int s = 0; s < NPL; ++s) {
		const uint32_t i = (uint32_t)lane + 64u * s;
		big[s] = 0;
		if (i < half) {
			const uint32_t c2 = 2 * i + 2;
			const md_pair a = v[c2 - 1], b = v[c2];
			big[s] = md_less<MAXH>(b, a) ? c2 - 1 : c2;
		}
	}
	uint32_t cur = 0, depth = 0, my_c = 0, my_cn = 0;
	auto step_to = [&](uint32_t nxt) {
		++depth;
		if ((uint32_t)lane == depth)
			my_c = nxt;
		if ((uint32_t)lane + 1 == depth)
			my_cn = nxt;
		cur = nxt;
	};
	while (cur < half) {
		const uint32_t ln = cur & 63u, sl = cur >> 6;
		uint32_t nxt = (uint32_t)__builtin_amdgcn_readlane((int)big[0], (int)ln);
#pragma unroll
		for (int s = 1; s < NPL; ++s)
			if (sl == (uint32_t)s)
				nxt = (uint32_t)__builtin_amdgcn_readlane((int)big[s], (int)ln);
		step_to(nxt);
	}
	if ((len & 1) == 0 && cur == (len - 2) / 2)
		step_to(2 * cur + 1);  // the last node has a left child only
	const bool on_chain = (uint32_t)lane < depth;
	const md_pair z = v[on_chain ? my_cn : 0];
	wave_lds_sync();  // (as in coop_push_up: all loads before any lane's store)
	const unsigned long long rises = __builtin_amdgcn_ballot_w64(on_chain && md_less<MAXH>(z, value));
	const unsigned long long stay = ~rises & ((depth >= 64 ? 0ull : (1ull << depth)) - 1ull);
	const uint32_t settle = stay ? 64u - (uint32_t)__builtin_clzll(stay) : 0u;
	if ((uint32_t)lane < settle)
		v[my_c] = z;
	else if ((uint32_t)lane == settle)
		v[my_c] = value;
}
// the same for any length: the chain of larger children is walked one level at a time (every lane reads
// the same two children: LDS broadcasts), the tail is coop_adjust's
template <bool MAXH> __device__ inline void coop_adjust_deep(md_pair* v, uint32_t len, md_pair value, int lane) {
	const uint32_t half = (len - 1) / 2;
	uint32_t cur = 0, depth = 0, my_c = 0, my_cn = 0;
	auto step_to = [&](uint32_t nxt) {
		++depth;
		if ((uint32_t)lane == depth)
			my_c = nxt;
		if ((uint32_t)lane + 1 == depth)
			my_cn = nxt;
		cur = nxt;
	};
	while (cur < half) {
		const uint32_t c2 = 2 * cur + 2;
		const float a = v[c2 - 1].d, b = v[c2].d;
		step_to((MAXH ? (b < a) : (b > a)) ? c2 - 1 : c2);
	}
	if ((len & 1) == 0 && cur == (len - 2) / 2)
		step_to(2 * cur + 1);
	const bool on_chain = (uint32_t)lane < depth;
	const md_pair z = v[on_chain ? my_cn : 0];
	wave_lds_sync();
	const unsigned long long rises = __builtin_amdgcn_ballot_w64(on_chain && md_less<MAXH>(z, value));
	const unsigned long long stay = ~rises & ((depth >= 64 ? 0ull : (1ull << depth)) - 1ull);
	const uint32_t settle = stay ? 64u - (uint32_t)__builtin_clzll(stay) : 0u;
	if ((uint32_t)lane < settle)
		v[my_c] = z;
	else if ((uint32_t)lane == settle)
		v[my_c] = value;
}
// std::pop_heap + pop_back
template <bool MAXH> __device__ inline void coop_pop(md_pair* v, uint32_t& n, int lane, uint32_t serial = 0) {
	if (n > 1) {
		// (libstdc++ also parks the old top in slot n - 1; nothing ever reads a slot beyond the queue's
		// size, so that store -- and the two fences it would need around it -- is left out)
		const md_pair value = v[n - 1];
		const uint32_t len = n - 1;
		if (serial) {
			wave_lds_sync();
			if (lane == 0)
				heap_adjust<MAXH>(v, 0, len, value);
		} else if (len <= 129) {
			coop_adjust<MAXH, 1>(v, len, value, lane);
		} else if (len <= 513) {
			coop_adjust<MAXH, 4>(v, len, value, lane);
		} else {  // long queues (the builder's candidates at ef_construction = 480): walk the chain level by level
			coop_adjust_deep<MAXH>(v, len, value, lane);
		}
		wave_lds_sync();
	}
	--n;
}

// Test hook (expann_device_heap_trace): one wave replays a trace of queue operations through the very
// coop_push / coop_pop the walk uses, so that tests/golden/heap_ref.json -- answered by the image's real
// std::priority_queue -- pins the device queues directly.  The range constructor's make_heap runs the
// serial __adjust_heap (the walk only ever constructs one-element queues).
struct HeapTraceParams {
	int max_heap;
	uint32_t n_init, n_ops;
	const float* init_d;
	const uint32_t* init_id;
	const int* ops;       // 1 = push (op_d, op_id), 0 = pop
	const float* op_d;
	const uint32_t* op_id;
	uint32_t* out_size;   // [n_ops + 1]
	float* out_top_d;
	uint32_t* out_top_id;
	float* drain_d;       // [n_init + n_ops]
	uint32_t* drain_id;
	uint32_t* n_drain;
	uint32_t serial;
};
template <bool MAXH> __device__ inline void heap_trace_body(const HeapTraceParams& p, md_pair* v, int lane) {
	uint32_t n = p.n_init;
	for (uint32_t i = lane; i < n; i += 64)
		v[i] = md_pair{p.init_d[i], p.init_id[i]};
	wave_lds_sync();
	if (lane == 0 && n >= 2)  // std::__make_heap
		for (uint32_t parent = (n - 2) / 2;; --parent) {
			const md_pair value = v[parent];
			heap_adjust<MAXH>(v, parent, n, value);
			if (parent == 0)
				break;
		}
	wave_lds_sync();
	for (uint32_t i = 0;; ++i) {
		const md_pair top = v[0];
		if (lane == 0) {
			p.out_size[i] = n;
			p.out_top_d[i] = n ? top.d : 0.0f;
			p.out_top_id[i] = n ? top.id : 0u;
		}
		if (i == p.n_ops)
			break;
		if (p.ops[i] == 1)
			coop_push<MAXH>(v, n, md_pair{p.op_d[i], p.op_id[i]}, lane, p.serial);
		else if (n)
			coop_pop<MAXH>(v, n, lane, p.serial);
		wave_lds_sync();
	}
	uint32_t nd = 0;
	while (n) {
		const md_pair top = v[0];
		if (lane == 0) {
			p.drain_d[nd] = top.d;
			p.drain_id[nd] = top.id;
		}
		++nd;
		coop_pop<MAXH>(v, n, lane, p.serial);
		wave_lds_sync();
	}
	if (lane == 0)
		*p.n_drain = nd;
}
static __global__ __launch_bounds__(64) void heap_trace_kernel(HeapTraceParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char heap_trace_smem[];
	md_pair* v = reinterpret_cast<md_pair*>(heap_trace_smem);
	if (p.max_heap)
		heap_trace_body<true>(p, v, (int)threadIdx.x);
	else
		heap_trace_body<false>(p, v, (int)threadIdx.x);
}

// ---- run-time dim (D = 0 instances of the walk and of the builder's search) ----------------------
// Any dim that is a multiple of 16 up to kGraphMaxAnyDim (uint8: of 64).  The query sits in LDS (a
// register copy would be dim / 16 floats per lane); a row is read in chunks of kGraphAnyChunk dims per
// lane with kGraphAnyRows rows in flight per 16-lane group, and every row's accumulator is carried from
// chunk to chunk: lane l still runs fma(diff, diff, acc) over t = 0 ... dim/16 - 1 in ascending order,
// then reduce16_ref_order -- the compiled instances' (and the reference's) arithmetic, bit for bit.
constexpr uint32_t kGraphMaxAnyDim = 4096;
constexpr int kGraphAnyRows = 4;
constexpr int kGraphAnyChunk = 16;   // fp32: dims per lane and chunk (256 per row)
constexpr int kGraphAnyChunkU8 = 8;  // uint8: dwords per lane and chunk (512 B per row)

// _Float16 rows: every load of a batch is issued before the first value is consumed.  Left to itself the scheduler
// sinks each 2-byte load next to the v_fma_mix that uses it (fewer registers) and the batch becomes one dependent
// memory round trip per dim.  Nothing for float rows: their instances stay as they are.
template <typename TR> __device__ __attribute__((always_inline)) inline void rows_requested() {
	if constexpr (!std::is_same<TR, float>::value)
		__builtin_amdgcn_sched_barrier(0);
}

// fp32 squared L2 of the query qs[dim] (LDS) against U rows per 16-lane group; TR: the rows' element type (float, or
// _Float16: lane l reads its dims as 2-byte loads, the per-dim step is ref_diff<_Float16>, common.hpp)
template <int U, typename TR = float>
__device__ inline void dist_f32_rows_any(const TR* vectors, uint32_t dim, const float* qs, const uint32_t* rows,
                                         float* d, int l) {
	const uint32_t dpl = dim / 16;
	const TR* src[U];
	float acc[U];
#pragma unroll
	for (int u = 0; u < U; ++u) {
		src[u] = vectors + (size_t)rows[u] * dim + l;
		acc[u] = 0.0f;
	}
	uint32_t t0 = 0;
	for (; t0 + kGraphAnyChunk <= dpl; t0 += kGraphAnyChunk) {
		TR r[U][kGraphAnyChunk];
#pragma unroll
		for (int u = 0; u < U; ++u)
#pragma unroll
			for (int t = 0; t < kGraphAnyChunk; ++t)
				r[u][t] = src[u][16 * (t0 + t)];
		rows_requested<TR>();
#pragma unroll
		for (int t = 0; t < kGraphAnyChunk; ++t) {
			const float qv = qs[l + 16 * (t0 + t)];
#pragma unroll
			for (int u = 0; u < U; ++u) {
				const float diff = ref_diff<TR>(qv, r[u][t]);
				acc[u] = __builtin_fmaf(diff, diff, acc[u]);
			}
		}
	}
	if (t0 < dpl) {  // the last, partial chunk (wave-uniform tests: nothing is read past the row)
		TR r[U][kGraphAnyChunk];
#pragma unroll
		for (int t = 0; t < kGraphAnyChunk; ++t)
			if (t0 + t < dpl)
#pragma unroll
				for (int u = 0; u < U; ++u)
					r[u][t] = src[u][16 * (t0 + t)];
		rows_requested<TR>();
#pragma unroll
		for (int t = 0; t < kGraphAnyChunk; ++t) {
			if (t0 + t < dpl) {
				const float qv = qs[l + 16 * (t0 + t)];
#pragma unroll
				for (int u = 0; u < U; ++u) {
					const float diff = ref_diff<TR>(qv, r[u][t]);
					acc[u] = __builtin_fmaf(diff, diff, acc[u]);
				}
			}
		}
	}
#pragma unroll
	for (int u = 0; u < U; ++u)
		d[u] = reduce16_ref_order(acc[u]);
}

// uint8 squared L2 (kU8L2, exact integers: any lane split gives the same sum) of the query's truncated
// bytes q8s[dim / 4] (LDS, packed) against U rows per 16-lane group; lane l takes dwords l, l + 16, ...
// of a row (dim % 64 == 0).  q8self = the query's sum of squares.
template <int U>
__device__ inline void dist_u8_rows_any(const uint8_t* compressed, uint32_t dim, const int* q8s, int q8self,
                                        const uint32_t* rows, float* d, int l) {
	const uint32_t nw = dim / 64;
	const int* src[U];
	int acc[U], bself[U];
#pragma unroll
	for (int u = 0; u < U; ++u) {
		src[u] = reinterpret_cast<const int*>(compressed + (size_t)rows[u] * dim) + l;
		acc[u] = 0;
		bself[u] = 0;
	}
	uint32_t w0 = 0;
	for (; w0 + kGraphAnyChunkU8 <= nw; w0 += kGraphAnyChunkU8) {
		int b[U][kGraphAnyChunkU8];
#pragma unroll
		for (int u = 0; u < U; ++u)
#pragma unroll
			for (int w = 0; w < kGraphAnyChunkU8; ++w)
				b[u][w] = src[u][16 * (w0 + w)];
#pragma unroll
		for (int w = 0; w < kGraphAnyChunkU8; ++w) {
			const int qv = q8s[l + 16 * (w0 + w)];
#pragma unroll
			for (int u = 0; u < U; ++u) {
				bself[u] = dot4<kU8L2>(b[u][w], b[u][w], bself[u]);
				acc[u] = dot4<kU8L2>(qv, b[u][w], acc[u]);
			}
		}
	}
	if (w0 < nw) {
		int b[U][kGraphAnyChunkU8];
#pragma unroll
		for (int w = 0; w < kGraphAnyChunkU8; ++w)
			if (w0 + w < nw)
#pragma unroll
				for (int u = 0; u < U; ++u)
					b[u][w] = src[u][16 * (w0 + w)];
#pragma unroll
		for (int w = 0; w < kGraphAnyChunkU8; ++w) {
			if (w0 + w < nw) {
				const int qv = q8s[l + 16 * (w0 + w)];
#pragma unroll
				for (int u = 0; u < U; ++u) {
					bself[u] = dot4<kU8L2>(b[u][w], b[u][w], bself[u]);
					acc[u] = dot4<kU8L2>(qv, b[u][w], acc[u]);
				}
			}
		}
	}
#pragma unroll
	for (int u = 0; u < U; ++u)
		d[u] = (float)(reduce16_i32(bself[u] - 2 * acc[u]) + q8self);
}

// row `row` of `src` (fp32, dim floats) -> qs; for the uint8 walk also its truncated bytes -> q8s
// (packed as the rows are) and their sum of squares; RANGED: the bytes are the rows' affine conversion
// (ranged_q8_convert with the index's scale / offset) instead.  Called by the whole wave; ends with the LDS in place.
template <bool RANGED = false>
__device__ inline int stage_query_any(const float* src, uint32_t dim, float* qs, int* q8s, bool bytes, int lane,
                                      float scale = 0.0f, float offset = 0.0f) {
	for (uint32_t i = lane; i < dim; i += 64)
		qs[i] = src[i];
	if (bytes)
		for (uint32_t w = lane; w < dim / 4; w += 64) {
			unsigned packed = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				if constexpr (RANGED)
					packed |= (unsigned)ranged_q8_convert(src[4 * w + b], scale, offset) << (8 * b);
				else
					packed |= ((unsigned)(uint8_t)(uint32_t)src[4 * w + b]) << (8 * b);
			}
			q8s[w] = (int)packed;
		}
	wave_lds_sync();
	int self = 0;
	if (bytes) {
		for (uint32_t w = lane & 15; w < dim / 4; w += 16)
			self = dot4<kU8L2>(q8s[w], q8s[w], self);
		self = reduce16_i32(self);
	}
	return self;
}

// rows in flight per 16-lane group while a hop's neighbours are scored
template <int D> constexpr int graph_rows_f32() { return D == 0 ? kGraphAnyRows : (D <= 128 ? 8 : (D <= 256 ? 4 : 2)); }
// (binary16 rows keep the float instances' rows in flight)
template <int D> constexpr int graph_rows_u8() { return D == 0 ? kGraphAnyRows : (D <= 128 ? 16 : (D <= 256 ? 8 : 4)); }

// (the uint8 walk waits on latency, not bandwidth: 128 registers = 16 waves per CU instead of 12)
// D = 0: the run-time-dim instance (p.dim); the query and its bytes sit in LDS behind ndist
// MODE: kGraphF32 / kGraphU8Cast / kGraphRangedQ8; the two byte modes are one walk (COMPRESSED), the ranged
// one differs where the query's bytes are made
// waves per SIMD the run-time-dim instances are held to: fp32 3, the byte walks 4 (128 registers; left to itself the
// compiler takes one or two more and loses the fourth wave)
// (GROUPS: the group instances carry the query's group and the directory's pointers; at the same bound they spill
// 8-12 bytes per lane to scratch, so they are held to one wave less)
template <int MODE, bool GROUPS = false> constexpr int graph_any_dim_waves() { return (MODE != kGraphF32 ? 4 : 3) - (GROUPS ? 1 : 0); }

// THE FILTER RULE (FILTERED instances; p.allow_bits is a bitmap over vertex numbers, bit v & 31 of word v >> 5,
// least significant bit first; bits at and beyond n are ignored: the library keeps its own copy, zero from n on).
//   Descent: the entry evaluation and the greedy descent through the upper layers are unchanged and never look at
//   the filter.
//   Bottom-layer entry: the entry vertex is scored, marked visited and pushed on `candidates`; it is pushed on
//   `nearest` only if it is allowed.
//   Stop rule: stop when `candidates` is empty, or when nearest.size() == ef && cur.d > nearest.top().d.  While
//   `nearest` holds fewer than ef entries -- none included: nearest[0] means nothing then -- only an empty
//   `candidates` stops the walk.
//   Neighbour update: for each unvisited neighbour in adjacency order with distance dn: if nearest.size() < ef ||
//   dn < nearest.top().d, push it on `candidates`; if it is also allowed, push it on `nearest` and pop `nearest`
//   when it exceeds ef.  A disallowed vertex is traversed but never kept.
//   Pre-drop: a full `nearest` and !(dn < worst0) still drops a neighbour before the queue update (worst0 only
//   falls while the queue is full).
//   distcomps count every scored vertex, allowed or not.  Output as without a filter: drain `nearest`, reverse,
//   re-score in fp32 in the byte modes, truncate to k, pad with UINT64_MAX / +inf.
// With every bit set this is the unfiltered walk exactly (ids, distance bits, distcomps, all modes).
// How the flag travels: the lane that holds a neighbour for the visited test also reads its allow word (both
// requests are in flight together: no round trip is added to a hop) and leaves the flag in the SIGN BIT of the
// neighbour's ndist slot -- distances are >= 0 --, the lane that stores the score keeps that bit, and every reader
// strips it before it compares or stores.  No LDS, scratch or serial read is added.
// THE GROUP RULE (kFilterGroups instances; the header states it in full).  p.row_groups[v] is the label of vertex v,
// p.query_groups[qi] the group query qi names.  A query that names kGroupAny walks as if unfiltered: no label is
// loaded.  Any other query is walked here only when group_serve says so (the scan kernel serves the rest: a pulled
// query that is not walk-served is skipped); for it "allowed" means row_groups[v] == its group, and everything else
// is THE FILTER RULE word for word.  The label request stands where the allow word's does, beside the visited test;
// a list's padding reads the last row's label.
// THE RANGE WALK RULE (kFilterRange instances, MODE kGraphF32 only; the header states it in full).  r = p.radii[qi] in
// squared-L2 units, ef = p.ef, R = p.max_results, cap = p.near_cap = max(ef, R).  "d > r" below means !(d <= r): a NaN
// radius is in range of nothing.
//   Descent: unchanged, never looks at r.
//   Bottom layer: the plain walk's two queues.  Every scored bottom-layer vertex with d <= r adds 1 to `count`, kept or
//   not, the entry vertex included.
//   Stop rule: `candidates` empty, or nearest.size() >= ef && cur.d > nearest.top().d && (cur.d > r || nearest.size()
//   >= cap).
//   Neighbour update, unvisited neighbours in adjacency order: accept when nearest.size() < ef || dn < nearest.top().d
//   || (dn <= r && nearest.size() < cap); an accepted one is pushed on both queues, then `nearest` is popped once if
//   nearest.size() > ef && (nearest.top().d > r || nearest.size() > cap).  So either nearest.size() <= ef, or every
//   entry is in range and nearest.size() <= cap.
//   Pre-drop: with full0 = nearest.size() >= ef, worst0 and n0 taken at the start of the hop, a neighbour is dropped
//   before the queue update iff full0 && !(dn < worst0) && !(dn <= r && n0 < cap) -- it changes nothing: while the top is
//   above r it only falls, once every entry is in range it rises only up to r, and at cap it only falls again.  Counted
//   before it is dropped.
//   Output: drain `nearest`, reverse; the leading entries with d <= r, at most R of them, padded with UINT64_MAX /
//   +inf; out_counts = count; distcomps as the plain walk.
// With R <= ef, or r < 0 or NaN, this is the plain walk at that ef (equal distcomps) cut at r and R.
// `count` is wave-uniform: the compaction loop's lanes already hold every dn, one ballot per 64 neighbours feeds it, one
// lane stores it with the distcomps.  Nothing serial and no atomic is added to the hop loop.
// TR: the element type of p.vectors -- float, or _Float16 for a handle made by expann_graph_create_f16.  It covers
// every read of the rows (entry evaluation, descent, fp32 bottom layer, final re-score of the byte modes); the
// arithmetic is the float instance's over (float)row, bit for bit (ref_diff, common.hpp).
template <int D, int MODE, int DBG = 0, int KIND = kFilterNone, typename TR = float>
__global__ __launch_bounds__(64, (D == 0 ? graph_any_dim_waves<MODE, (KIND == kFilterGroups)>() : ((MODE != kGraphF32 && D <= 128) ? 4 : 1))) void graph_search_kernel(GraphSearchParams p) {
	constexpr bool COMPRESSED = MODE != kGraphF32, RANGED = MODE == kGraphRangedQ8;
	constexpr bool FILTERED = KIND == kFilterBitmap || KIND == kFilterGroups, GROUPS = KIND == kFilterGroups;
	constexpr bool RANGE = KIND == kFilterRange;
	static_assert(!RANGE || MODE == kGraphF32, "the range walk scores fp32 distances: the byte modes walk on integers");
	constexpr int DPL = D ? D / 16 : 1;
	constexpr int NW = D ? D / 64 : 1;
	unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ts = DBG ? clock64() : 0;
	auto stamp = [&](int i) {
		if (DBG) {
			const unsigned long long now = clock64();
			seg[i] += now - ts;
			ts = now;
		}
	};
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	md_pair* nearest = reinterpret_cast<md_pair*>(smem_raw);             // [near_cap + 1]
	md_pair* candidates = nearest + (p.near_cap + 1);                    // [cand_cap + 1]
	uint32_t* nlist = reinterpret_cast<uint32_t*>(candidates + (p.cand_cap + 1));  // [list_cap]
	float* ndist = reinterpret_cast<float*>(nlist + p.list_cap);          // [list_cap]
	float* qs = ndist + p.list_cap;                                       // D = 0: [dim] the query
	int* q8s = reinterpret_cast<int*>(qs + p.dim);                        // D = 0, COMPRESSED: [dim / 4] its bytes

	const int lane = threadIdx.x;
	const int l = lane & 15, rg = lane >> 4;
	const TR* vectors = reinterpret_cast<const TR*>(p.vectors);
	const bool bits = p.vis_words != 0;
	uint8_t* visited = bits ? nullptr : p.visited + (size_t)blockIdx.x * p.n;
	uint32_t* vbits = bits ? p.vis_bits + (size_t)blockIdx.x * p.vis_words : nullptr;
	uint32_t epoch = bits ? 0u : p.epochs[blockIdx.x];
	// is vertex nb new to this query?  (marks it)
	auto test_and_set = [&](uint32_t nb, uint8_t ep8) -> bool {
		if (bits)
			return (atomicOr(&vbits[nb >> 5], 1u << (nb & 31)) & (1u << (nb & 31))) == 0;
		const bool fresh = visited[nb] != ep8;
		if (fresh)
			visited[nb] = ep8;
		return fresh;
	};
	uint32_t overflowed = 0;
	uint32_t n_walked = 0;  // GROUPS: queries this workgroup walked (wave-uniform; one atomic when it leaves)

	for (;;) {
		// queries are pulled, not dealt: walks differ in length, and a grid sized to what is resident
		// ends evenly
		uint32_t qi = 0;
		if (lane == 0)
			qi = atomicAdd(p.next_query, 1u);
		qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)qi);
		if (p.query_map) {  // a redo launch: the queries the list names, as many as the device counted
			const uint32_t m_redo = *p.m_dev;
			if (qi >= (m_redo < p.m ? m_redo : p.m))
				break;
			qi = p.query_map[qi];
		} else if (qi >= p.m)
			break;
		uint32_t qgroup = kGroupAny;  // GROUPS: the group this query names; wave-uniform
		if constexpr (GROUPS) {
			qgroup = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.query_groups[qi]);
			if (qgroup != kGroupAny) {
				uint32_t gi, s;
				if (group_serve(p.group_keys, p.group_off, p.n_groups, qgroup, p.k, p.flat_rows, &gi, &s) != kGroupServeWalk) {
					wave_lds_sync();  // (every iteration ends in the wave barrier, as a walked one does)
					continue;         // the scan kernel's
				}
			}
			++n_walked;
		}
		const bool any_group = qgroup == kGroupAny;
		// RANGE: the query's radius and the in-range vertices its bottom layer scored; wave-uniform
		float radius = 0.0f;
		uint32_t in_range = 0;
		if constexpr (RANGE)
			radius = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.radii[qi])));
		bool q_overflowed = false;  // wave-uniform: this walk met a full candidates heap
		// ---- per-query setup ----------------------------------------------------------
		if (!bits && ++epoch > 255) {  // epoch bytes wrapped: clear this workgroup's visited array
			for (uint32_t i = lane; i < p.n; i += 64)
				visited[i] = 0;
			epoch = 1;
		}
		const uint8_t ep8 = (uint8_t)epoch;
		float q[DPL];
		int q8[NW];  // trunc(query) bytes of this lane (compressed path)
		int q8self = 0;
		if constexpr (D == 0) {
			if constexpr (RANGED)
				q8self = stage_query_any<true>(p.queries + (size_t)qi * p.dim, p.dim, qs, q8s, true, lane, p.q_scale, p.q_offset);
			else
				q8self = stage_query_any(p.queries + (size_t)qi * p.dim, p.dim, qs, q8s, COMPRESSED, lane);
		} else {
#pragma unroll
			for (int t = 0; t < DPL; ++t)
				q[t] = p.queries[(size_t)qi * D + l + 16 * t];
			if (COMPRESSED) {
#pragma unroll
				for (int w = 0; w < NW; ++w) {
					unsigned packed = 0;
#pragma unroll
					for (int b = 0; b < 4; ++b) {
						const float v = p.queries[(size_t)qi * D + l * (D / 16) + 4 * w + b];
						if constexpr (RANGED)
							packed |= (unsigned)ranged_q8_convert(v, p.q_scale, p.q_offset) << (8 * b);
						else
							packed |= ((unsigned)(uint8_t)(uint32_t)v) << (8 * b);
					}
					q8[w] = (int)packed;
					q8self = dot4<kU8L2>(q8[w], q8[w], q8self);
				}
				q8self = reduce16_i32(q8self);
			}
		}
		// exact fp32 squared L2 of the query against U rows per 16-lane group (reference order), all
		// rows requested before the first is consumed
		auto dist_f32_rows = [&](auto u_tag, const uint32_t* rows, float* d) {
			constexpr int U = decltype(u_tag)::value;
			if constexpr (D == 0) {
				dist_f32_rows_any<U, TR>(vectors, p.dim, qs, rows, d, l);
				return;
			}
			TR r[U][DPL];
#pragma unroll
			for (int u = 0; u < U; ++u) {
				const TR* src = vectors + (size_t)rows[u] * D + l;
#pragma unroll
				for (int t = 0; t < DPL; ++t)
					r[u][t] = src[16 * t];
			}
			rows_requested<TR>();
#pragma unroll
			for (int u = 0; u < U; ++u) {
				float acc = 0.0f;
#pragma unroll
				for (int t = 0; t < DPL; ++t) {
					const float diff = ref_diff<TR>(q[t], r[u][t]);
					acc = __builtin_fmaf(diff, diff, acc);
				}
				d[u] = reduce16_ref_order(acc);
			}
		};
		auto dist_u8_rows = [&](auto u_tag, const uint32_t* rows, float* d) {
			constexpr int U = decltype(u_tag)::value;
			if constexpr (D == 0) {
				dist_u8_rows_any<U>(p.compressed, p.dim, q8s, q8self, rows, d, l);
				return;
			}
			int b[U][NW];
#pragma unroll
			for (int u = 0; u < U; ++u) {
				const int* r = reinterpret_cast<const int*>(p.compressed + (size_t)rows[u] * D) + l * NW;
#pragma unroll
				for (int w = 0; w < NW; ++w)
					b[u][w] = r[w];
			}
#pragma unroll
			for (int u = 0; u < U; ++u) {
				int bself = 0;
#pragma unroll
				for (int w = 0; w < NW; ++w)
					bself = dot4<kU8L2>(b[u][w], b[u][w], bself);
				const int part = partial_score<kU8L2, NW>(q8, b[u], bself);
				d[u] = (float)(reduce16_i32(part) + q8self);
			}
		};
		auto dist_f32 = [&](uint32_t row) -> float {
			float d1[1];
			dist_f32_rows(std::integral_constant<int, 1>{}, &row, d1);
			return d1[0];
		};
		uint32_t distcomps = 0;

		// ---- upper layers: greedy descent (:863-902) -----------------------------------
		uint32_t entry = p.starting_vertex;
		float ep_dist = dist_f32(entry);  // every 16-lane row computes the same value
		++distcomps;
		for (uint32_t layer = p.n_layers - 1; layer > 0; --layer) {
			const uint32_t* off = p.layer_off + (size_t)layer * (p.n + 1);
			bool changed = true;
			while (changed) {
				changed = false;
				const uint32_t e0 = off[entry], deg = off[entry + 1] - e0;
				// first-improvement chain == first occurrence of the minimum, if it improves: the smallest
				// (distance bits, list position) key of the list (distances are >= 0: their bits order them)
				// (run-time dim, uint8 walk: 2 rows, so that both row scorers fit the 168 registers without spilling)
				constexpr int UD = COMPRESSED ? (D == 0 ? 2 : (graph_rows_f32<D>() > 4 ? 4 : graph_rows_f32<D>())) : graph_rows_f32<D>();
				uint64_t best_key = ~0ull;
				uint32_t best_nb = 0;
				for (uint32_t i0 = 0; i0 < deg; i0 += 4 * UD) {
					uint32_t nb[UD];
					float d[UD];
#pragma unroll
					for (int u = 0; u < UD; ++u) {
						const uint32_t i = i0 + 4 * u + rg;
						nb[u] = p.neighbours[e0 + (i < deg ? i : deg - 1)];
					}
					dist_f32_rows(std::integral_constant<int, UD>{}, nb, d);
#pragma unroll
					for (int u = 0; u < UD; ++u) {
						const uint32_t i = i0 + 4 * u + rg;
						const uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, d[u]) << 32) | i;
						if (i < deg && key < best_key) {
							best_key = key;
							best_nb = nb[u];
						}
					}
				}
				const uint64_t wmin = wave_min_key64(best_key);
				distcomps += deg;
				const float dmin = __builtin_bit_cast(float, (uint32_t)(wmin >> 32));
				if (wmin != ~0ull && dmin < ep_dist) {
					// the lane(s) that hold the winning key broadcast its vertex
					const unsigned long long who = __builtin_amdgcn_ballot_w64(best_key == wmin);
					entry = (uint32_t)__builtin_amdgcn_readlane((int)best_nb, __builtin_ctzll(who));
					ep_dist = dmin;
					changed = true;
				}
			}
		}
		stamp(0);

		// ---- bottom layer: best-first search --------------------------------------------
		uint32_t n_near = 0, n_cand = 0;  // wave-uniform
		float d_entry;
		{
			float d1[1];
			if (COMPRESSED)
				dist_u8_rows(std::integral_constant<int, 1>{}, &entry, d1);
			else
				dist_f32_rows(std::integral_constant<int, 1>{}, &entry, d1);
			d_entry = d1[0];
		}
		++distcomps;
		if constexpr (RANGE)
			in_range += d_entry <= radius ? 1u : 0u;
		{
			const md_pair e{d_entry, entry};
			coop_push<false>(candidates, n_cand, e, lane, p.debug & 1);
			bool keep_entry = true;  // wave-uniform
			if constexpr (GROUPS)
				keep_entry = any_group || p.row_groups[entry] == qgroup;
			else if constexpr (FILTERED)
				keep_entry = (p.allow_bits[entry >> 5] >> (entry & 31)) & 1u;
			if (keep_entry)
				coop_push<true>(nearest, n_near, e, lane, p.debug & 1);
			if (lane == 0)
				(void)test_and_set(entry, ep8);
		}
		wave_lds_sync();
		for (;;) {
			// pop the best candidate (:588-594)
			if (n_cand == 0)
				break;
			const md_pair cur = candidates[0];
			coop_pop<false>(candidates, n_cand, lane, p.debug & 1);
			const bool full0 = RANGE ? n_near >= p.ef : n_near == p.ef;
			const uint32_t n0 = n_near;  // RANGE: room for in-range neighbours while n0 < near_cap
			// (FILTERED: `nearest` may be empty, its slot 0 never written; worst0 only counts when the queue is full)
			const float worst0 = FILTERED ? (full0 ? nearest[0].d : __builtin_inff()) : nearest[0].d;
			stamp(1);
			if constexpr (RANGE) {
				if (full0 && cur.d > worst0 && (!(cur.d <= radius) || n0 >= p.near_cap))
					break;
			} else if (cur.d > worst0 && full0)
				break;
			if (DBG)
				seg[6]++;
			// unvisited neighbours, in adjacency order (:595-607): the list sits at a fixed stride, both
			// halves of a list longer than a wavefront are requested before either is consumed
			const uint32_t* adj = p.adj0 + (size_t)cur.id * p.stride0;
			uint32_t nbv[2];
			bool fresh[2];
			// FILTERED: 0x80000000 when the neighbour is disallowed, else 0 -- the sign bit of its ndist slot
			uint32_t* nflag = reinterpret_cast<uint32_t*>(ndist);
			// (a list's padding, UINT32_MAX, reads the last word: it is never fresh, its flag goes nowhere)
			auto disallowed = [&](uint32_t nb) -> uint32_t {
				if constexpr (GROUPS)
					return any_group ? 0u : (p.row_groups[nb < p.n ? nb : p.n - 1] != qgroup ? 0x80000000u : 0u);
				const uint32_t w = nb >> 5, w_last = (p.n - 1) >> 5;
				return (~(p.allow_bits[w < w_last ? w : w_last] >> (nb & 31)) & 1u) << 31;
			};
			uint32_t dis[2] = {0u, 0u};
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const uint32_t i = 64u * h + lane;
				nbv[h] = i < p.stride0 ? adj[i] : 0xFFFFFFFFu;
			}
			if constexpr (FILTERED) {
#pragma unroll
				for (int h = 0; h < 2; ++h)
					dis[h] = disallowed(nbv[h]);
			}
#pragma unroll
			for (int h = 0; h < 2; ++h)
				fresh[h] = nbv[h] != 0xFFFFFFFFu && test_and_set(nbv[h], ep8);
			uint32_t n_list = 0;
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(fresh[h]);
				if (fresh[h]) {
					const uint32_t pos = n_list + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
					nlist[pos] = nbv[h];
					if constexpr (FILTERED)
						nflag[pos] = dis[h];
				}
				n_list += (uint32_t)__builtin_popcountll(mask);
			}
			for (uint32_t i0 = 128; i0 < p.stride0; i0 += 64) {  // (lists beyond 128: M0 > 128)
				const uint32_t i = i0 + lane;
				const uint32_t nb = i < p.stride0 ? adj[i] : 0xFFFFFFFFu;
				uint32_t ds = 0u;
				if constexpr (FILTERED)
					ds = disallowed(nb);
				const bool fr = nb != 0xFFFFFFFFu && test_and_set(nb, ep8);
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(fr);
				if (fr) {
					const uint32_t pos = n_list + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
					nlist[pos] = nb;
					if constexpr (FILTERED)
						nflag[pos] = ds;
				}
				n_list += (uint32_t)__builtin_popcountll(mask);
			}
			wave_lds_sync();
			stamp(2);
			// score them (:636-689 / :795-835): 4 rows per step (16 lanes each), U steps' rows requested
			// before the first is consumed -- a hop is a dependent chain of HBM round trips otherwise
			constexpr int U = COMPRESSED ? graph_rows_u8<D>() : graph_rows_f32<D>();
			for (uint32_t i0 = 0; i0 < n_list; i0 += 4 * U) {
				uint32_t nb[U];
#pragma unroll
				for (int u = 0; u < U; ++u) {
					const uint32_t i = i0 + 4 * u + rg;
					nb[u] = nlist[i < n_list ? i : n_list - 1];
				}
				float d[U];
				if (COMPRESSED)
					dist_u8_rows(std::integral_constant<int, U>{}, nb, d);
				else
					dist_f32_rows(std::integral_constant<int, U>{}, nb, d);
#pragma unroll
				for (int u = 0; u < U; ++u) {
					const uint32_t i = i0 + 4 * u + rg;
					if (l == 0 && i < n_list) {
						if constexpr (FILTERED)  // (the slot holds the neighbour's flag, its sign bit, and nothing else: one LDS or)
							(void)__hip_atomic_fetch_or(&nflag[i], __builtin_bit_cast(uint32_t, d[u]), __ATOMIC_RELAXED,
							                            __HIP_MEMORY_SCOPE_WAVEFRONT);
						else
							ndist[i] = d[u];
					}
				}
			}
			distcomps += n_list;
			wave_lds_sync();
			stamp(3);
			// queue update in list order (:666-670): first every lane drops what cannot pass `d_next <
			// nearest.top().first` any more (the top only falls while the queue is full), the survivors are
			// compacted in place, in order; then one wave-wide queue operation per survivor
			uint32_t n_s = 0;
			for (uint32_t i0 = 0; i0 < n_list; i0 += 64) {  // (a chunk only writes slots it has already read)
				const uint32_t i = i0 + lane;
				const uint32_t id = i < n_list ? nlist[i] : 0u;
				const float dn_raw = i < n_list ? ndist[i] : 0.0f;  // FILTERED: with the flag in its sign bit
				const float dn = FILTERED ? __builtin_fabsf(dn_raw) : dn_raw;
				bool keep = i < n_list && !(full0 && !(dn < worst0));
				if constexpr (RANGE) {  // counted before anything is dropped; an in-range neighbour stays while there is room
					const bool within = i < n_list && dn <= radius;
					in_range += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(within));
					keep = keep || (within && n0 < p.near_cap);
				}
				wave_lds_sync();
				const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
				const uint32_t pos = n_s + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
				if (keep) {
					nlist[pos] = id;
					ndist[pos] = dn_raw;
				}
				n_s += (uint32_t)__builtin_popcountll(mask);
			}
			wave_lds_sync();
			for (uint32_t j = 0; j < n_s; ++j) {
				const float dn_raw = ndist[j];
				const float dn = FILTERED ? __builtin_fabsf(dn_raw) : dn_raw;
				const bool allowed = !FILTERED || !(__builtin_bit_cast(uint32_t, dn_raw) & 0x80000000u);  // wave-uniform
				if constexpr (RANGE) {
					if (n_near < p.ef || dn < nearest[0].d || (dn <= radius && n_near < p.near_cap)) {
						const md_pair e{dn, nlist[j]};
						if (n_cand >= p.cand_cap)
							q_overflowed = true;
						else
							coop_push<false>(candidates, n_cand, e, lane, p.debug & 1);
						coop_push<true>(nearest, n_near, e, lane, p.debug & 1);
						wave_lds_sync();
						if (n_near > p.ef && (!(nearest[0].d <= radius) || n_near > p.near_cap))
							coop_pop<true>(nearest, n_near, lane, p.debug & 1);
					}
				} else if (n_near < p.ef || dn < nearest[0].d) {
					const md_pair e{dn, nlist[j]};
					if (n_cand >= p.cand_cap)
						q_overflowed = true;
					else
						coop_push<false>(candidates, n_cand, e, lane, p.debug & 1);
					if (allowed) {
						coop_push<true>(nearest, n_near, e, lane, p.debug & 1);
						wave_lds_sync();
						if (n_near > p.ef)
							coop_pop<true>(nearest, n_near, lane, p.debug & 1);
					} else if (FILTERED)
						wave_lds_sync();
					if (DBG)
						seg[7]++;
				}
			}
			wave_lds_sync();
			stamp(4);
		}
		// ---- output: drain nearest, reverse, (re-score), truncate to k (:695-707, :845-848) -
		const uint32_t cnt = n_near;
		for (uint32_t i = cnt; i-- > 0;) {
			const md_pair t = nearest[0];
			coop_pop<true>(nearest, n_near, lane, p.debug & 1);
			if (lane == 0) {
				nlist[i] = t.id;
				ndist[i] = t.d;
			}
		}
		wave_lds_sync();
		uint32_t n_out = cnt < p.k ? cnt : p.k;
		if constexpr (RANGE) {  // the leading entries within the radius (ascending: they are all of them), at most k = R
			uint32_t n_in = 0;
			for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
				const uint32_t i = i0 + lane;
				n_in += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(i < cnt && ndist[i] <= radius));
			}
			n_out = n_in < p.k ? n_in : p.k;
		}
		if (COMPRESSED) {
			for (uint32_t i0 = 0; i0 < n_out; i0 += 4) {
				const uint32_t i = i0 + rg;
				const float d = dist_f32(nlist[i < n_out ? i : n_out - 1]);
				if (l == 0 && i < n_out)
					ndist[i] = d;
			}
			wave_lds_sync();
		}
		for (uint32_t i = lane; i < p.k; i += 64) {
			p.out_ids[(size_t)qi * p.k + i] = i < n_out ? (uint64_t)nlist[i] : ~0ull;
			if (!RANGE || p.out_dists)
				p.out_dists[(size_t)qi * p.k + i] = i < n_out ? ndist[i] : __builtin_inff();
		}
		if (lane == 0 && p.out_distcomps)
			p.out_distcomps[qi] = distcomps;
		if constexpr (RANGE) {
			if (lane == 0)
				p.out_counts[qi] = in_range;
		}
		// an overflowed walk goes on the redo list when there is one (its row is rewritten by the redo launch, which
		// also counts its distcomps), else it raises the launch's error flag
		const bool to_redo = q_overflowed && p.redo_list;
		if (q_overflowed && !to_redo)
			overflowed = 1;
		if (lane == 0) {
			if (to_redo)
				p.redo_list[atomicAdd(p.redo_count, 1u)] = qi;
			else if (p.distcomps_total)
				atomicAdd(p.distcomps_total, (unsigned long long)distcomps);
		}
		if (bits) {  // the set goes back to all-zero: 16 bytes per lane and store, nothing waits for them
			uint4* w = reinterpret_cast<uint4*>(vbits);
			for (uint32_t i = lane; i < p.vis_words / 4; i += 64)
				w[i] = make_uint4(0u, 0u, 0u, 0u);
		}
		wave_lds_sync();
		stamp(5);
	}
	if (DBG && lane == 0 && p.stamps)
		for (int i = 0; i < 8; ++i)
			p.stamps[(size_t)blockIdx.x * 8 + i] = seg[i];
	if (lane == 0) {
		if (!bits)
			p.epochs[blockIdx.x] = epoch;
		if (overflowed)
			atomicAdd(p.error, 1u);
		if (GROUPS && n_walked && !p.query_map && p.group_walked)
			atomicAdd(p.group_walked, n_walked);
	}
}

}  // namespace expann
