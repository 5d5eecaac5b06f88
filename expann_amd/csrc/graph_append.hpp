// graph_append.hpp -- the walk's tables remade on the device from the builder's resident state
// (expann_graph_append, THE GRAPH APPEND RULE in include/expann_hip.h).
//
// After the batches of an append the handle's builder state (BuildGraph, graph_build.hpp: fixed-stride rows of
// (id, distance) with a degree per row) is the graph; what the walk reads is derived from it here, whole, in the
// order antitopo_index::flatten() and expann_graph_create would give it:
//   append_adj0_kernel      layer 0 at the walk's fixed stride: row v = its first deg0[v] ids, then UINT32_MAX
//   append_degree_kernel    the layer-major sequence of degrees, one entry per (layer, vertex) and one more per layer
//                           for the layer's end entry (degree 0), written where the offsets will stand
//   append_scan_*           exclusive scan of that sequence in place, reduce-then-scan over workgroups: tile sums,
//                           one workgroup scans the sums, every tile is scanned again from its sum
//   append_fill_kernel      the ids of every row copied behind its offset
// A row's degree is read through append_degree alone, so the three passes cannot disagree.  Nothing here is on the
// path of a search.
#pragma once
#include "graph_build.hpp"

namespace expann {

struct AppendTables {
	BuildGraph g;           // g.n rows; g.U is the stride of the upper-layer arrays (a capacity)
	uint32_t n_layers;
	uint32_t* adj0;         // [n][stride0]
	uint32_t stride0;       // a multiple of 4, >= g.cap0
	uint32_t* layer_off;    // [n_layers][n + 1]
	uint32_t* neighbours;   // [edge_cap]
	uint32_t edge_cap;
	uint32_t* tile_sums;    // [ceil(n_layers * (n + 1) / kScanTile)]
};

constexpr int kScanPer = 8;                       // entries per thread
constexpr int kScanTile = kBlock * kScanPer;      // entries per workgroup

__device__ inline uint64_t append_entries(const AppendTables& t) { return (uint64_t)t.n_layers * (t.g.n + 1ull); }

// the degree of entry i of the layer-major sequence: (layer, vertex) = (i / (n + 1), i % (n + 1)); the end entry of
// a layer and a vertex below the layer have none.  A row never holds more than its cap once a batch is in.
__device__ inline uint32_t append_degree(const AppendTables& t, uint64_t i, uint32_t* layer, uint32_t* vertex) {
	const uint32_t l = (uint32_t)(i / (t.g.n + 1ull)), v = (uint32_t)(i % (t.g.n + 1ull));
	*layer = l;
	*vertex = v;
	if (v == t.g.n)
		return 0;
	if (l == 0)
		return min(t.g.deg0[v], t.g.cap0);
	if (t.g.level[v] < l)
		return 0;
	return min(*t.g.deg(l, v), t.g.capu);
}

// 16 bytes per lane: four ids of one row
__global__ __launch_bounds__(kBlock) void append_adj0_kernel(AppendTables t) {
	const uint32_t quads = t.stride0 / 4;
	const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	if (i >= (uint64_t)t.g.n * quads)
		return;
	const uint32_t v = (uint32_t)(i / quads), c = (uint32_t)(i % quads) * 4;
	const uint32_t deg = min(t.g.deg0[v], t.g.cap0);
	const uint32_t* src = t.g.id0 + (size_t)v * t.g.stride0 + c;
	uint4 o = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
	if (c + 4 <= deg && t.g.stride0 % 4 == 0) {
		o = *reinterpret_cast<const uint4*>(src);
	} else {
		if (c + 0 < deg) o.x = src[0];
		if (c + 1 < deg) o.y = src[1];
		if (c + 2 < deg) o.z = src[2];
		if (c + 3 < deg) o.w = src[3];
	}
	*reinterpret_cast<uint4*>(t.adj0 + (size_t)v * t.stride0 + c) = o;
}

__global__ __launch_bounds__(kBlock) void append_degree_kernel(AppendTables t) {
	const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	if (i >= append_entries(t))
		return;
	uint32_t l, v;
	t.layer_off[i] = append_degree(t, i, &l, &v);
}

// exclusive scan of one value per thread over the workgroup; *total = the workgroup's sum.  wave_sums: LDS [kBlock / 64]
__device__ inline uint32_t block_exclusive_scan(uint32_t x, uint32_t* wave_sums, uint32_t* total) {
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t incl = x;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
		if (lane >= (uint32_t)off)
			incl += y;
	}
	__syncthreads();  // (wave_sums of the call before are read by now)
	if (lane == 63)
		wave_sums[wave] = incl;
	__syncthreads();
	uint32_t base = 0, sum = 0;
#pragma unroll
	for (uint32_t w = 0; w < kBlock / 64; ++w) {
		if (w < wave)
			base += wave_sums[w];
		sum += wave_sums[w];
	}
	*total = sum;
	return base + incl - x;
}

// the kScanPer entries of thread `threadIdx.x` in tile `blockIdx.x` (0 beyond the end)
__device__ inline void append_load_entries(const AppendTables& t, uint64_t n_entries, uint32_t (&e)[kScanPer]) {
	const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
	if (i0 + kScanPer <= n_entries) {  // (a tile starts at a multiple of 8 entries: 16-byte aligned)
		const uint4 a = *reinterpret_cast<const uint4*>(t.layer_off + i0);
		const uint4 b = *reinterpret_cast<const uint4*>(t.layer_off + i0 + 4);
		e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
		e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
	} else {
#pragma unroll
		for (int j = 0; j < kScanPer; ++j)
			e[j] = i0 + j < n_entries ? t.layer_off[i0 + j] : 0u;
	}
}

__global__ __launch_bounds__(kBlock) void append_scan_reduce_kernel(AppendTables t) {
	__shared__ uint32_t wave_sums[kBlock / 64];
	uint32_t e[kScanPer];
	append_load_entries(t, append_entries(t), e);
	uint32_t s = 0;
#pragma unroll
	for (int j = 0; j < kScanPer; ++j)
		s += e[j];
	uint32_t total;
	(void)block_exclusive_scan(s, wave_sums, &total);
	if (threadIdx.x == 0)
		t.tile_sums[blockIdx.x] = total;
}

// one workgroup: the tile sums become their exclusive scan, kBlock at a time with the carry in a register
__global__ __launch_bounds__(kBlock) void append_scan_sums_kernel(uint32_t* tile_sums, uint32_t n_tiles) {
	__shared__ uint32_t wave_sums[kBlock / 64];
	uint32_t carry = 0;
	for (uint32_t i0 = 0; i0 < n_tiles; i0 += kBlock) {
		const uint32_t i = i0 + threadIdx.x;
		const uint32_t x = i < n_tiles ? tile_sums[i] : 0u;
		uint32_t total;
		const uint32_t ex = block_exclusive_scan(x, wave_sums, &total);
		if (i < n_tiles)
			tile_sums[i] = carry + ex;
		carry += total;
	}
}

__global__ __launch_bounds__(kBlock) void append_scan_tiles_kernel(AppendTables t) {
	__shared__ uint32_t wave_sums[kBlock / 64];
	const uint64_t n_entries = append_entries(t);
	uint32_t e[kScanPer];
	append_load_entries(t, n_entries, e);
	uint32_t s = 0;
#pragma unroll
	for (int j = 0; j < kScanPer; ++j)
		s += e[j];
	uint32_t total;
	uint32_t run = t.tile_sums[blockIdx.x] + block_exclusive_scan(s, wave_sums, &total);
	const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
	uint32_t o[kScanPer];
#pragma unroll
	for (int j = 0; j < kScanPer; ++j) {
		o[j] = run;
		run += e[j];
	}
	if (i0 + kScanPer <= n_entries) {
		*reinterpret_cast<uint4*>(t.layer_off + i0) = make_uint4(o[0], o[1], o[2], o[3]);
		*reinterpret_cast<uint4*>(t.layer_off + i0 + 4) = make_uint4(o[4], o[5], o[6], o[7]);
	} else {
#pragma unroll
		for (int j = 0; j < kScanPer; ++j)
			if (i0 + j < n_entries)
				t.layer_off[i0 + j] = o[j];
	}
}

// 16 lanes per entry: the row's ids behind its offset (an edge past edge_cap is never written: the capacity is
// cap0 / capu edges per row, which append_degree does not exceed)
__global__ __launch_bounds__(kBlock) void append_fill_kernel(AppendTables t) {
	const uint64_t i = (uint64_t)blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);
	if (i >= append_entries(t))
		return;
	uint32_t l, v;
	const uint32_t deg = append_degree(t, i, &l, &v);
	if (deg == 0)
		return;
	const uint32_t off = t.layer_off[i];
	const uint32_t* src = t.g.ids(l, v);
	for (uint32_t j = threadIdx.x & 15; j < deg; j += 16)
		if (off + j < t.edge_cap)
			t.neighbours[off + j] = src[j];
}

}  // namespace expann
