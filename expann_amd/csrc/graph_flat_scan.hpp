// graph_flat_scan.hpp -- what a graph search does under a SPARSE row filter: an exact scan of the allowed rows.
//
// A walk under a filter that allows few rows visits most of the graph with `nearest` never full; its candidates
// heap grows with the frontier.  So when a filter allows at most "filter_flat_rows" rows the search does not walk:
// every query is scored against exactly the allowed rows -- fp32, the reference's FMA order (dist_f32_rows_any,
// the query in LDS, whatever the handle's mode) -- and the min(k, allowed) smallest (distance, id) are returned
// ascending, padded with UINT64_MAX / +inf: what the brute-force index returns over those rows.  distcomps per
// query = the allowed count.
//
// One wavefront (= one 64-thread workgroup) per query; workgroups pull queries from a counter as the walk's do.
// The allowed rows come as the compacted ascending list made at set time (filter_compact_kernel).  The k best so
// far are (distance bits << 32 | id) keys in LDS, unordered, with the largest of them (`worst`) and its slot in
// registers: a scored row that does not beat `worst` while the set is full is dropped by its own lane before
// anything serial happens; a survivor replaces the worst key and the wave finds the new worst.  Distances are
// >= 0, so their bits order them, and ids make every key distinct.  The keys are ranked at the end (rank = number
// of smaller keys) and written in order.
#pragma once
#include "graph_search.hpp"

namespace expann {

struct GraphFlatParams {
	const float* vectors;       // [n][dim]; TR = _Float16: the same address holds [n][dim] binary16 rows
	uint32_t dim;               // a multiple of 16
	const uint32_t* list;       // [n_list] the allowed vertices, ascending
	uint32_t n_list;            // >= 1
	const float* queries;       // [m][dim]
	uint32_t m, k;
	uint32_t kk;                // min(k, n_list): keys kept in LDS
	uint64_t* out_ids;          // [m][k]
	float* out_dists;           // [m][k]
	uint32_t* out_distcomps;    // [m] or nullptr
	uint32_t* next_query;       // [1] zero at launch
	unsigned long long* distcomps_total;  // as GraphSearchParams::distcomps_total, or nullptr
};

// dynamic LDS of a launch: the keys and the query
inline size_t graph_flat_lds_bytes(uint32_t kk, uint32_t dim) { return sizeof(uint64_t) * kk + sizeof(float) * dim; }

// max of a 64-bit key over the wave (all lanes get it)
__device__ inline uint64_t wave_max_key64(uint64_t v) {
	for (int off = 32; off > 0; off >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
		const uint64_t o = ((uint64_t)hi << 32) | lo;
		v = o > v ? o : v;
	}
	return v;
}

// One query of the scan, by one wave: the kk = p.kk smallest (distance, id) of p.list[0 .. p.n_list) for query qi,
// ascending and padded to p.k, distcomps = p.n_list.  keys: [kk] in LDS, qs: [dim] in LDS (staged here).  Both scan
// kernels call it; p.m and p.next_query are not read.
// TR: the rows' element type, as in graph_search_kernel
template <typename TR>
__device__ __attribute__((always_inline)) inline void flat_scan_query(const GraphFlatParams p, uint32_t qi, uint64_t* keys,
                                                                      float* qs, int lane, int l, int rg) {
	constexpr int U = kGraphAnyRows;
	for (uint32_t i = lane; i < p.dim; i += 64)
		qs[i] = p.queries[(size_t)qi * p.dim + i];
	wave_lds_sync();
	uint32_t n_kept = 0, worst_pos = 0;  // wave-uniform
	uint64_t worst = ~0ull;              // the largest kept key once n_kept == kk
	// the largest key and its slot, by the whole wave (the keys are distinct)
	auto find_worst = [&]() {
		wave_lds_sync();
		uint64_t mine = 0;
		uint32_t mine_pos = 0;
		for (uint32_t i = lane; i < p.kk; i += 64) {
			const uint64_t v = keys[i];
			if (v >= mine) {
				mine = v;
				mine_pos = i;
			}
		}
		worst = wave_max_key64(mine);
		const unsigned long long who = __builtin_amdgcn_ballot_w64(mine == worst && (uint32_t)lane < p.kk);
		worst_pos = (uint32_t)__builtin_amdgcn_readlane((int)mine_pos, __builtin_ctzll(who));
	};
	for (uint32_t i0 = 0; i0 < p.n_list; i0 += 4 * U) {
		uint32_t rows[U];
		float d[U];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t i = i0 + 4 * u + rg;
			rows[u] = p.list[i < p.n_list ? i : p.n_list - 1];
		}
		dist_f32_rows_any<U, TR>(reinterpret_cast<const TR*>(p.vectors), p.dim, qs, rows, d, l);
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const uint32_t i = i0 + 4 * u + rg;
			const uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, d[u]) << 32) | rows[u];
			// the pre-drop: `worst` only falls while the set is full
			const bool pass = l == 0 && i < p.n_list && (n_kept < p.kk || key < worst);
			unsigned long long mask = __builtin_amdgcn_ballot_w64(pass);
			while (mask) {
				const int src = __builtin_ctzll(mask);
				mask &= mask - 1;
				const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, src);
				const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), src);
				const uint64_t kb = ((uint64_t)hi << 32) | lo;
				if (n_kept < p.kk) {
					if (lane == 0)
						keys[n_kept] = kb;
					if (++n_kept == p.kk)
						find_worst();
				} else if (kb < worst) {
					if (lane == 0)
						keys[worst_pos] = kb;
					find_worst();
				}
			}
		}
	}
	// n_kept == kk here (kk <= n_list and the keys of distinct rows are distinct); rank and write
	wave_lds_sync();
	for (uint32_t i = lane; i < p.kk; i += 64) {
		const uint64_t mine = keys[i];
		uint32_t rank = 0;
		for (uint32_t j = 0; j < p.kk; ++j)
			rank += keys[j] < mine ? 1u : 0u;
		p.out_ids[(size_t)qi * p.k + rank] = (uint64_t)(uint32_t)mine;
		p.out_dists[(size_t)qi * p.k + rank] = __builtin_bit_cast(float, (uint32_t)(mine >> 32));
	}
	for (uint32_t i = p.kk + lane; i < p.k; i += 64) {
		p.out_ids[(size_t)qi * p.k + i] = ~0ull;
		p.out_dists[(size_t)qi * p.k + i] = __builtin_inff();
	}
	if (lane == 0) {
		if (p.out_distcomps)
			p.out_distcomps[qi] = p.n_list;
		if (p.distcomps_total)
			atomicAdd(p.distcomps_total, (unsigned long long)p.n_list);
	}
	wave_lds_sync();  // (the next query overwrites qs and the keys)
}

template <typename TR = float> __global__ __launch_bounds__(64) void graph_flat_scan_kernel(GraphFlatParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char flat_smem[];
	uint64_t* keys = reinterpret_cast<uint64_t*>(flat_smem);  // [kk]
	float* qs = reinterpret_cast<float*>(keys + p.kk);        // [dim]
	const int lane = threadIdx.x;
	const int l = lane & 15, rg = lane >> 4;
	for (;;) {
		uint32_t qi = 0;
		if (lane == 0)
			qi = atomicAdd(p.next_query, 1u);
		qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)qi);
		if (qi >= p.m)
			break;
		flat_scan_query<TR>(p, qi, keys, qs, lane, l, rg);
	}
}

// ---- row groups (THE GROUP RULE): the scan's share of a grouped search ----------------------------------------
// Every query names a group; the directory made at set time gives the group's rows as an ascending list.  A query
// that group_serve sends to the walk (or that names kGroupAny) is skipped here; one whose group no row carries
// gets padding and distcomps 0; any other is flat_scan_query over its group's rows with kk = min(k, rows).
struct GraphGroupScanParams {
	GraphFlatParams f;             // vectors, dim, queries, m, k, outputs, next_query, distcomps_total; kk = min(k,
	                               // kGraphFlatMaxKeys): the LDS keys of a launch; list / n_list are set per query
	const uint32_t* query_groups;  // [m]
	const uint32_t* group_keys;    // [n_groups]
	const uint32_t* group_off;     // [n_groups + 1]
	const uint32_t* group_rows;    // the rows of group g at [off[g], off[g + 1]), ascending
	uint32_t n_groups, flat_rows;
	uint32_t* scanned;             // [1] queries served by the scan
	uint32_t* padded;              // [1] queries whose group is empty
};

// Every path of an iteration ends in wave_lds_sync(), and the served queries are counted in wave-uniform registers
// with one atomic each when the workgroup leaves.  A first form had `if (lane == 0) atomicAdd(...)` directly before
// the loop's back edge and never ended on the GPU: in its code (profiles/graph_groups_scan_hang_isa.txt) only lane 0
// leaves the iteration there, and lanes 1..63 pass the readfirstlane of the next query without it and read query 0.
template <typename TR = float> __global__ __launch_bounds__(64) void graph_group_scan_kernel(GraphGroupScanParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char flat_smem[];
	uint64_t* keys = reinterpret_cast<uint64_t*>(flat_smem);  // [p.f.kk]
	float* qs = reinterpret_cast<float*>(keys + p.f.kk);      // [dim]
	const int lane = threadIdx.x;
	const int l = lane & 15, rg = lane >> 4;
	uint32_t n_scanned = 0, n_padded = 0;  // wave-uniform
	for (;;) {
		uint32_t qi = 0;
		if (lane == 0)
			qi = atomicAdd(p.f.next_query, 1u);
		qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)qi);
		if (qi >= p.f.m)
			break;
		const uint32_t qg = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.query_groups[qi]);
		uint32_t gi = 0, s = 0;
		const int serve = qg == kGroupAny ? kGroupServeWalk
		                                  : group_serve(p.group_keys, p.group_off, p.n_groups, qg, p.f.k, p.flat_rows, &gi, &s);
		if (serve == kGroupServeScan) {
			GraphFlatParams q = p.f;
			q.list = p.group_rows + p.group_off[gi];
			q.n_list = s;
			q.kk = p.f.k < s ? p.f.k : s;  // (<= p.f.kk: group_serve keeps it within kGraphFlatMaxKeys)
			flat_scan_query<TR>(q, qi, keys, qs, lane, l, rg);
			++n_scanned;
		} else if (serve == kGroupServePad) {
			for (uint32_t i = lane; i < p.f.k; i += 64) {
				p.f.out_ids[(size_t)qi * p.f.k + i] = ~0ull;
				p.f.out_dists[(size_t)qi * p.f.k + i] = __builtin_inff();
				if (i == 0 && p.f.out_distcomps)
					p.f.out_distcomps[qi] = 0;
			}
			++n_padded;
		}
		wave_lds_sync();
	}
	if (lane == 0) {
		if (n_scanned)
			atomicAdd(p.scanned, n_scanned);
		if (n_padded)
			atomicAdd(p.padded, n_padded);
	}
}

}  // namespace expann
