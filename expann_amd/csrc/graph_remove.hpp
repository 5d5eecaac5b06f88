// graph_remove.hpp -- rows taken out of a built graph on the device (expann_graph_remove, THE GRAPH REMOVE RULE in
// include/expann_hip.h), over the builder's resident state (BuildGraph, graph_build.hpp).
//
// The keep bitmap and its word ranks are keep_bitmap.hpp's; a second bitmap of the same kind over the upper-layer
// rows (graph_remove_mark_upper_kernel) gives the survivors' new upper_idx, which is a rank in id order as well.
//   graph_remove_touch_kernel    16 lanes per (layer, vertex) row of a survivor: a row that holds a removed
//                                neighbour becomes a PruneTask, in no particular order
//   graph_remove_top_kernel      max over the survivors of (level, lowest new id): max_layer and starting_vertex
//   graph_remove_gather_kernel   one workgroup per task: the row's surviving entries with their stored lengths, and
//                                the surviving neighbours of every removed neighbour (one hop) with dist2 in the
//                                reference's lane order, distinct by id, the `keep_cap` smallest (length, id) kept --
//                                streamed: up to 1024 new keys at a time are sorted together with the best so far,
//                                equal keys dropped, the first keep_cap kept, which gives that set whatever the
//                                chunking.  Output: build_prune_kernel's candidate list (PruneTask::src_slot).
//   build_prune_kernel           graph_build.hpp's, unchanged, writes the touched row in place
//   graph_remove_compact_kernel  16 lanes per surviving row: level, upper_idx, degree, ids through the id map and
//                                lengths into arrays built aside under the new ids
// A gather reads the task's own row and rows of REMOVED vertices only, and no prune writes either before the task's
// own: the tasks go through gather + prune in chunks over one bounded list buffer, and every touched row is still
// computed from the graph as it was.  The degree of a row is read through remove_degree alone (min(deg, cap), the
// tables' rule: graph_append.hpp), so the passes cannot disagree on what a row holds.  Nothing here is on the path of a
// search.
#pragma once
#include "graph_build.hpp"
#include "keep_bitmap.hpp"

namespace expann {

constexpr uint32_t kRemoveChunk = 1024;  // new candidates per sort of the gather (= kPruneMaxCand, the list's bound)

struct RemoveView {
	BuildGraph g;               // the state before the call: g.n rows, g.U the stride of the upper arrays
	uint32_t n_layers;
	const uint32_t* bits;       // keep bitmap over the rows
	const uint32_t* word_rank;
	const uint32_t* ubits;      // keep bitmap over the upper rows (by upper_idx)
	const uint32_t* uword_rank;
};

__device__ inline bool remove_kept(const uint32_t* bits, uint32_t v) { return (bits[v >> 5] >> (v & 31)) & 1u; }
__device__ inline uint32_t remove_rank(const uint32_t* bits, const uint32_t* word_rank, uint32_t v) {
	return word_rank[v >> 5] + (uint32_t)__builtin_popcount(bits[v >> 5] & ((1u << (v & 31)) - 1u));
}
__device__ inline uint32_t remove_degree(const BuildGraph& g, uint32_t l, uint32_t v) { return min(*g.deg(l, v), g.cap(l)); }

// the upper rows of the removed vertices leave the upper bitmap (all ones on entry)
static __global__ __launch_bounds__(kBlock) void graph_remove_mark_upper_kernel(RemoveView r, uint32_t* __restrict__ ubits) {
	const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
	if (v >= r.g.n || remove_kept(r.bits, v) || r.g.level[v] == 0)
		return;
	const uint32_t u = (uint32_t)r.g.upper_idx[v];
	atomicAnd(&ubits[u >> 5], ~(1u << (u & 31)));
}

// ctr[0] += touched rows; tasks[t] = (vertex, layer, t % chunk).  Entry i of the layer-major sequence is
// (layer, vertex) = (i / n, i % n), 16 lanes each.
static __global__ __launch_bounds__(kBlock) void graph_remove_touch_kernel(RemoveView r, PruneTask* __restrict__ tasks,
                                                                      uint32_t task_cap, uint32_t chunk,
                                                                      uint32_t* __restrict__ ctr) {
	const uint64_t i = (uint64_t)blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);
	const uint32_t lane = threadIdx.x & 63, sub = threadIdx.x & 15;
	bool hit = false;
	uint32_t l = 0, v = 0;
	if (i < (uint64_t)r.n_layers * r.g.n) {
		l = (uint32_t)(i / r.g.n);
		v = (uint32_t)(i % r.g.n);
		if (remove_kept(r.bits, v) && r.g.level[v] >= l) {
			const uint32_t deg = remove_degree(r.g, l, v);
			const uint32_t* ids = r.g.ids(l, v);
			for (uint32_t j = sub; j < deg; j += 16)
				hit = hit || !remove_kept(r.bits, ids[j]);
		}
	}
	const unsigned long long any = __builtin_amdgcn_ballot_w64(hit) & (0xFFFFull << (lane & 48));
	if (sub == 0 && any) {
		const uint32_t t = atomicAdd(&ctr[0], 1u);
		if (t < task_cap)
			tasks[t] = PruneTask{v, l, (int32_t)(t % chunk)};
	}
}

// *top = max over the survivors of (level << 32 | ~new id): the highest level, the lowest new id of that level
static __global__ __launch_bounds__(kBlock) void graph_remove_top_kernel(RemoveView r, unsigned long long* __restrict__ top) {
	unsigned long long best = 0;
	for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < r.g.n; v += gridDim.x * kBlock)
		if (remove_kept(r.bits, v)) {
			const unsigned long long key =
			    ((unsigned long long)r.g.level[v] << 32) | (0xFFFFFFFFu - remove_rank(r.bits, r.word_rank, v));
			best = key > best ? key : best;
		}
	for (int off = 32; off > 0; off >>= 1) {
		const unsigned long long o = __shfl_xor(best, off);
		best = o > best ? o : best;
	}
	if ((threadIdx.x & 63) == 0 && best)
		atomicMax(top, best);
}

struct RemoveGatherParams {
	RemoveView r;
	const PruneTask* tasks;   // the chunk's tasks
	uint32_t n_tasks;
	uint32_t keep_cap;        // max(ef_construction, M0) <= kPruneMaxCand: entries per list
	md_pair* lists;           // [chunk][keep_cap]
	uint32_t* list_cnt;       // [chunk]
	uint32_t* n_truncated;    // += rows with more than keep_cap distinct candidates
	uint32_t dim;
};

// keys[0, 2 * kRemoveChunk) sorted ascending, all threads of the workgroup
__device__ inline void remove_sort_keys(uint64_t* keys) {
	constexpr uint32_t N = 2 * kRemoveChunk;
	for (uint32_t size = 2; size <= N; size <<= 1)
		for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
			for (uint32_t i = threadIdx.x; i < N / 2; i += kBlock) {
				const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
				const bool up = (lo & size) == 0;
				const uint64_t a = keys[lo], b = keys[hi];
				if ((a > b) == up) {
					keys[lo] = b;
					keys[hi] = a;
				}
			}
			__syncthreads();
		}
}

static __global__ __launch_bounds__(kBlock) void graph_remove_gather_kernel(RemoveGatherParams p) {
	constexpr uint32_t N = 2 * kRemoveChunk;
	__shared__ uint64_t keys[N];            // [0, kRemoveChunk): the best so far; behind them the new candidates
	__shared__ uint32_t own_id[kPruneMaxCand];
	__shared__ uint32_t pend_id[kRemoveChunk];
	__shared__ uint32_t n_pend, n_out, truncated;
	const BuildGraph& g = p.r.g;
	const uint32_t tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;

	for (uint32_t t = blockIdx.x; t < p.n_tasks; t += gridDim.x) {
		const uint32_t v = p.tasks[t].vertex, layer = p.tasks[t].layer;
		const uint32_t slot = (uint32_t)p.tasks[t].src_slot;
		const uint32_t deg_v = remove_degree(g, layer, v);
		const uint32_t* ids_v = g.ids(layer, v);
		const float* d_v = g.dists(layer, v);
		const float* vec_v = g.vec + (size_t)v * p.dim;
		for (uint32_t i = tid; i < kRemoveChunk; i += kBlock) {
			uint64_t k = kSentinelKey;
			uint32_t id = 0xFFFFFFFFu;
			if (i < deg_v) {
				id = ids_v[i];
				if (remove_kept(p.r.bits, id))
					k = make_key(d_v[i], id);
			}
			own_id[i] = id;
			keys[i] = k;
			keys[kRemoveChunk + i] = kSentinelKey;
		}
		if (tid == 0)
			n_pend = 0, n_out = 0, truncated = 0;
		__syncthreads();

		// the pending candidates get their lengths, join the best so far, and the keep_cap smallest distinct keys stay
		auto flush = [&]() {
			const uint32_t np = n_pend;
			for (uint32_t i0 = 0; i0 < np; i0 += kBlock / 16) {  // 16 lanes per candidate, every lane in the reduction
				const uint32_t i = i0 + grp;
				const uint32_t c = pend_id[i < np ? i : np - 1];
				const float* vec_c = g.vec + (size_t)c * p.dim;
				float acc = 0.0f;
				for (uint32_t k = sub; k < p.dim; k += 16) {
					const float diff = vec_v[k] - vec_c[k];
					acc = __builtin_fmaf(diff, diff, acc);
				}
				const float d = reduce16_ref_order(acc);
				if (sub == 0 && i < np)
					keys[kRemoveChunk + i] = make_key(d, c);
			}
			__syncthreads();
			remove_sort_keys(keys);
			// a vertex adopted twice has the same length both times: equal keys stand side by side
			bool dup[N / kBlock];
			int any = 0;
#pragma unroll
			for (uint32_t j = 0; j < N / kBlock; ++j) {
				const uint32_t i = tid + j * kBlock;
				dup[j] = i > 0 && keys[i] != kSentinelKey && keys[i] == keys[i - 1];
				any |= dup[j];
			}
			__syncthreads();
#pragma unroll
			for (uint32_t j = 0; j < N / kBlock; ++j)
				if (dup[j])
					keys[tid + j * kBlock] = kSentinelKey;
			if (__syncthreads_or(any))
				remove_sort_keys(keys);
			if (tid == 0) {
				if (keys[p.keep_cap] != kSentinelKey)
					truncated = 1;
				n_pend = 0;
			}
			__syncthreads();
			for (uint32_t i = p.keep_cap + tid; i < N; i += kBlock)
				keys[i] = kSentinelKey;
			__syncthreads();
		};

		uint32_t pend_bound = 0;  // (what n_pend cannot exceed: the same in every thread, no read of the counter)
		for (uint32_t j = 0; j < deg_v; ++j) {
			const uint32_t r = own_id[j];
			if (remove_kept(p.r.bits, r))
				continue;
			const uint32_t deg_r = remove_degree(g, layer, r);
			const uint32_t* ids_r = g.ids(layer, r);
			if (pend_bound + deg_r > kRemoveChunk) {
				flush();
				pend_bound = 0;
			}
			pend_bound += deg_r;
			for (uint32_t i = tid; i < deg_r; i += kBlock) {
				const uint32_t c = ids_r[i];
				bool take = c != v && remove_kept(p.r.bits, c);
				for (uint32_t k = 0; take && k < deg_v; ++k)  // an own entry wins over an adopted duplicate
					take = own_id[k] != c;
				if (take)
					pend_id[atomicAdd(&n_pend, 1u)] = c;
			}
			__syncthreads();
		}
		flush();

		md_pair* out = p.lists + (size_t)slot * p.keep_cap;
		uint32_t mine = 0;
		for (uint32_t i = tid; i < p.keep_cap; i += kBlock) {
			const uint64_t k = keys[i];
			if (k != kSentinelKey) {
				out[i] = md_pair{key_score(k), key_idx(k)};
				++mine;
			}
		}
		if (mine)
			atomicAdd(&n_out, mine);
		__syncthreads();
		if (tid == 0) {
			p.list_cnt[slot] = n_out;
			if (truncated)
				atomicAdd(p.n_truncated, 1u);
		}
		__syncthreads();
	}
}

struct RemoveCompactParams {
	RemoveView r;
	uint8_t* level;       // the arrays under the new ids, at the handle's capacities and strides
	int32_t* upper_idx;
	uint32_t* id0;
	float* d0;
	uint32_t* deg0;       // zero on entry
	uint32_t* idu;
	float* du;
	uint32_t* degu;       // zero on entry
};

// Entry i of the layer-major sequence, 16 lanes each, as graph_remove_touch_kernel.  Every id in a surviving row is a
// survivor's by now: an untouched row held no other, a touched row was pruned from survivors.
static __global__ __launch_bounds__(kBlock) void graph_remove_compact_kernel(RemoveCompactParams p) {
	const BuildGraph& g = p.r.g;
	const uint64_t i = (uint64_t)blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);
	if (i >= (uint64_t)p.r.n_layers * g.n)
		return;
	const uint32_t l = (uint32_t)(i / g.n), v = (uint32_t)(i % g.n), sub = threadIdx.x & 15;
	if (!remove_kept(p.r.bits, v) || g.level[v] < l)
		return;
	const uint32_t nv = remove_rank(p.r.bits, p.r.word_rank, v);
	const uint32_t nu = g.level[v] >= 1 ? remove_rank(p.r.ubits, p.r.uword_rank, (uint32_t)g.upper_idx[v]) : 0u;
	const uint32_t deg = remove_degree(g, l, v);
	const uint32_t* src_id = g.ids(l, v);
	const float* src_d = g.dists(l, v);
	uint32_t* dst_id;
	float* dst_d;
	if (l == 0) {
		dst_id = p.id0 + (size_t)nv * g.stride0;
		dst_d = p.d0 + (size_t)nv * g.stride0;
		if (sub == 0) {
			p.level[nv] = g.level[v];
			p.upper_idx[nv] = g.level[v] >= 1 ? (int32_t)nu : -1;
			p.deg0[nv] = deg;
		}
	} else {
		const size_t row = (size_t)(l - 1) * g.U + nu;
		dst_id = p.idu + row * g.strideu;
		dst_d = p.du + row * g.strideu;
		if (sub == 0)
			p.degu[row] = deg;
	}
	for (uint32_t j = sub; j < deg; j += 16) {
		dst_id[j] = remove_rank(p.r.bits, p.r.word_rank, src_id[j]);
		dst_d[j] = src_d[j];
	}
}

}  // namespace expann
