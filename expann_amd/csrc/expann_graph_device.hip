// expann_graph_device.hip -- the graph_search_kernel instances behind expann_graph_search_device (DEV = true:
// overflow list per query, query indirection for the redo launch, distcomps total).  A translation unit of
// their own: the host-buffer instances in expann_graph.hip stay byte for byte what they were, and the two
// sets compile side by side.  The host code of the path is in expann_graph.hip.
#include <hip/hip_runtime.h>

#include "graph_search.hpp"

namespace expann {
namespace {
struct DeviceVariant {
	int d;
	int mode;  // expann_graph_compression
	GraphSearchFn fn;
};
#define GRAPH_DEV_V(D)                                                     \
	{D, kGraphF32, graph_search_kernel<D, kGraphF32, 0, true>},            \
	    {D, kGraphU8Cast, graph_search_kernel<D, kGraphU8Cast, 0, true>},  \
	    {D, kGraphRangedQ8, graph_search_kernel<D, kGraphRangedQ8, 0, true>}
const DeviceVariant kGraphDev[] = {GRAPH_DEV_V(64),  GRAPH_DEV_V(128), GRAPH_DEV_V(256), GRAPH_DEV_V(512),
                                   GRAPH_DEV_V(768), GRAPH_DEV_V(832), GRAPH_DEV_V(960), GRAPH_DEV_V(0)};
#undef GRAPH_DEV_V
}  // namespace

GraphSearchFn graph_search_device_instance(int dim, int mode, bool* run_time_dim) {
	const DeviceVariant* any = nullptr;
	for (const auto& v : kGraphDev)
		if (v.mode == mode) {
			if (v.d == dim) {
				*run_time_dim = false;
				return v.fn;
			}
			if (v.d == 0)
				any = &v;
		}
	*run_time_dim = true;
	return any ? any->fn : nullptr;
}
}  // namespace expann
