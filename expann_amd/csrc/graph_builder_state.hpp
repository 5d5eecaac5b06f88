// graph_builder_state.hpp -- what the batched builder (graph_build.hpp) works on, owned on the host side: the eight
// arrays of a BuildGraph with their geometry, a batch's scratch, and the build's parameters.  expann_graph_build_batched
// makes them for one call; a graph handle keeps them from its first append or remove on (expann_graph.hip:
// GraphBuildState), and expann_graph_remove builds a second set of arrays aside and moves it in.
//
// THE TWO UPPER LAYOUTS.  The host (antitopo_index's strided form, the one-shot builder's arguments) keeps the upper
// rows as [layer][U]: row (l - 1) * U + upper_idx[v], U the upper vertices there are.  A handle keeps them as
// [L_cap][U_cap] with room to grow: row (l - 1) * U_cap + upper_idx[v].  copy_host() takes the HOST's row stride per
// layer and converts; BuildGraph::U is always the DEVICE's, U_cap.  The one-shot builder has U_cap = U.
//
// Every call enqueues on the stream it is given and returns the first HIP error; copy_host() also waits for the
// stream (the host's arrays are pageable, and the caller reads or frees them next).
#pragma once
#include "graph_build.hpp"
#include "host_common.hpp"

namespace expann {

// `a` becomes an array of cap_bytes that starts with its first keep_bytes (zero behind them when `zero`); the old
// block goes once the copy is done, so the old and the new of ONE array are live together, never of several
template <typename T> hipError_t dev_regrow(DevPtr<T>& a, size_t keep_bytes, size_t cap_bytes, hipStream_t st, bool zero = false) {
	DevPtr<T> b;
	HIP_OK(hipMalloc(&b, std::max<size_t>(cap_bytes, 1)));
	if (zero)
		HIP_OK(hipMemsetAsync(b, 0, cap_bytes, st));
	if (keep_bytes)
		HIP_OK(hipMemcpyAsync(b, a, keep_bytes, hipMemcpyDeviceToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
	a = std::move(b);
	return hipSuccess;
}

struct BuilderArrays {
	uint32_t stride0 = 0, strideu = 0;  // row strides: M0 / M plus the slack for reverse edges
	size_t U_cap = 0, L_cap = 0;        // the upper arrays hold [L_cap][U_cap] rows
	DevPtr<uint8_t> level;              // [rows]: the row capacity is the owner's (GraphRows::cap_rows, or n)
	DevPtr<int32_t> upper_idx;          // [rows]
	DevPtr<uint32_t> id0;               // [rows][stride0]
	DevPtr<float> d0;
	DevPtr<uint32_t> deg0;              // [rows]
	DevPtr<uint32_t> idu;               // [L_cap * U_cap][strideu]
	DevPtr<float> du;
	DevPtr<uint32_t> degu;              // [L_cap * U_cap]

	size_t upper_rows() const { return L_cap * U_cap; }

	// arrays of this geometry in place of what was held, every degree zero
	hipError_t alloc(size_t rows, uint32_t s0, uint32_t su, size_t U_cap_, size_t L_cap_, hipStream_t st) {
		*this = BuilderArrays{};
		stride0 = s0, strideu = su, U_cap = U_cap_, L_cap = L_cap_;
		const size_t up = upper_rows();
		HIP_OK(hipMalloc(&level, std::max<size_t>(rows, 1)));
		HIP_OK(hipMalloc(&upper_idx, std::max<size_t>(rows, 1) * 4));
		HIP_OK(hipMalloc(&id0, std::max<size_t>(rows * s0, 1) * 4));
		HIP_OK(hipMalloc(&d0, std::max<size_t>(rows * s0, 1) * 4));
		HIP_OK(hipMalloc(&deg0, std::max<size_t>(rows, 1) * 4));
		HIP_OK(hipMalloc(&idu, std::max<size_t>(up * su, 1) * 4));
		HIP_OK(hipMalloc(&du, std::max<size_t>(up * su, 1) * 4));
		HIP_OK(hipMalloc(&degu, std::max<size_t>(up, 1) * 4));
		HIP_OK(hipMemsetAsync(deg0, 0, rows * 4, st));
		return hipMemsetAsync(degu, 0, up * 4, st);
	}

	// The first n rows, and the first `rows` rows of `layers` upper layers, from (UP) or to the host's arrays, whose
	// upper layers are host_U rows apart; where both sides keep their layers `rows` apart, the layers are one run.  A
	// null host array is left out.  Waited for.  (A download into const arrays does not compile.)
	template <bool UP, typename B, typename I, typename W, typename D>
	hipError_t copy_host(size_t n, B* h_level, I* h_upper_idx, W* h_id0, D* h_d0, W* h_deg0, size_t rows, size_t layers,
	                     size_t host_U, W* h_idu, D* h_du, W* h_degu, hipStream_t st) const {
		auto copy = [&](auto* dev, auto* host, size_t count) {
			if (!host || !count)
				return hipSuccess;
			if constexpr (UP)
				return hipMemcpyAsync(dev, host, count * sizeof(*dev), hipMemcpyHostToDevice, st);
			else
				return hipMemcpyAsync(host, dev, count * sizeof(*dev), hipMemcpyDeviceToHost, st);
		};
		HIP_OK(copy(level.get(), h_level, n));
		HIP_OK(copy(upper_idx.get(), h_upper_idx, n));
		HIP_OK(copy(id0.get(), h_id0, n * stride0));
		HIP_OK(copy(d0.get(), h_d0, n * stride0));
		HIP_OK(copy(deg0.get(), h_deg0, n));
		const size_t su = strideu, runs = (rows == U_cap && rows == host_U) ? 1 : layers, run = runs == 1 ? rows * layers : rows;
		for (size_t l = 0; l < runs && h_idu; ++l) {
			HIP_OK(copy(idu.get() + l * U_cap * su, h_idu + l * host_U * su, run * su));
			HIP_OK(copy(du.get() + l * U_cap * su, h_du + l * host_U * su, run * su));
			HIP_OK(copy(degu.get() + l * U_cap, h_degu + l * host_U, run));
		}
		return hipStreamSynchronize(st);
	}

	// the kernels' view: n rows at `vec`, rows cut at M0 / M
	BuildGraph view(const float* vec, size_t n, size_t M0, size_t M) const {
		return BuildGraph{vec,     (uint32_t)n, level, upper_idx, id0,           d0,      deg0,           (uint32_t)M0,
		                  stride0, idu,         du,    degu,      (uint32_t)M, strideu, (uint32_t)U_cap};
	}

	// room for `rows` rows, the first n kept, the degrees behind them zero; one array at a time
	hipError_t grow_rows(size_t n, size_t rows, hipStream_t st) {
		HIP_OK(dev_regrow(level, n, rows, st));
		HIP_OK(dev_regrow(upper_idx, n * 4, rows * 4, st));
		HIP_OK(dev_regrow(id0, n * stride0 * 4, rows * stride0 * 4, st));
		HIP_OK(dev_regrow(d0, n * stride0 * 4, rows * stride0 * 4, st));
		return dev_regrow(deg0, n * 4, rows * 4, st, true);
	}

	// the upper arrays laid out again as [new_L][new_U] (neither smaller than before): the first U rows of every
	// layer kept, every other degree zero; waited for, the old arrays go
	hipError_t relayout_upper(size_t U, size_t new_U, size_t new_L, hipStream_t st) {
		const size_t rows = new_U * new_L, su = strideu;
		DevPtr<uint32_t> idu2, degu2;
		DevPtr<float> du2;
		HIP_OK(hipMalloc(&idu2, std::max<size_t>(rows * su, 1) * 4));
		HIP_OK(hipMalloc(&du2, std::max<size_t>(rows * su, 1) * 4));
		HIP_OK(hipMalloc(&degu2, std::max<size_t>(rows, 1) * 4));
		HIP_OK(hipMemsetAsync(degu2, 0, rows * 4, st));
		for (size_t l = 0; l < L_cap && U; ++l) {
			HIP_OK(hipMemcpyAsync(idu2.get() + l * new_U * su, idu.get() + l * U_cap * su, U * su * 4, hipMemcpyDeviceToDevice, st));
			HIP_OK(hipMemcpyAsync(du2.get() + l * new_U * su, du.get() + l * U_cap * su, U * su * 4, hipMemcpyDeviceToDevice, st));
			HIP_OK(hipMemcpyAsync(degu2.get() + l * new_U, degu.get() + l * U_cap, U * 4, hipMemcpyDeviceToDevice, st));
		}
		HIP_OK(hipStreamSynchronize(st));
		idu = std::move(idu2);
		du = std::move(du2);
		degu = std::move(degu2);
		U_cap = new_U;
		L_cap = new_L;
		return hipSuccess;
	}
};

// the parameters of a build, the same for every batch
struct BuildConfig {
	size_t M = 0, M0 = 0, ef_construction = 0, prune_overflow = 0;
	float ortho_factor = 0, ortho_bias = 0;
};

// a batch's search lists, prune tasks and counters
struct BuildScratch {
	DevPtr<md_pair> out;        // [lists][ef_construction]
	DevPtr<uint32_t> out_cnt;   // [lists]
	DevPtr<PruneTask> tasks;    // [lists]
	DevPtr<int32_t> up_slot;    // [max_batch]
	DevPtr<uint2> dirty;        // [dirty_cap]
	size_t dirty_cap = 0;
	DevPtr<uint32_t> ctr;       // [8], zero: [0] n_dirty, [1] dropped, [2] search overflow, [3] n_tasks

	// a dirty list of at least `cap` entries (its content is a batch's: nothing is kept)
	hipError_t size_dirty(size_t cap) {
		if (cap <= dirty_cap)
			return hipSuccess;
		dirty.reset();
		HIP_OK(hipMalloc(&dirty, cap * sizeof(uint2)));
		dirty_cap = cap;
		return hipSuccess;
	}
	// `lists` = the vertices of the largest batch + the upper-layer lists it may bring
	hipError_t alloc(size_t lists, size_t max_batch, size_t ef_construction, size_t dirty_entries, hipStream_t st) {
		HIP_OK(hipMalloc(&out, lists * ef_construction * sizeof(md_pair)));
		HIP_OK(hipMalloc(&out_cnt, lists * 4));
		HIP_OK(hipMalloc(&tasks, lists * sizeof(PruneTask)));
		HIP_OK(hipMalloc(&up_slot, max_batch * 4));
		HIP_OK(hipMalloc(&ctr, 8 * 4));
		HIP_OK(hipMemsetAsync(ctr, 0, 8 * 4, st));
		return size_dirty(dirty_entries);
	}
};

}  // namespace expann
