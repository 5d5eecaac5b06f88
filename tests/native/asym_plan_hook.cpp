// asym_plan_hook.cpp -- plan_asym / plan_asym_tiles of bf_plan.hpp for tests/test_asym_abi.py.  Each input line
// "int_mode k cap n sel_rows first last" prints "status family n_tiles_sel tile_stride fixed".
#include <cstdio>

#include "bf_plan.hpp"

int main() {
	int int_mode, first, last;
	unsigned long k, n;
	unsigned cap, sel_rows;
	while (std::scanf("%d %lu %u %lu %u %d %d", &int_mode, &k, &cap, &n, &sel_rows, &first, &last) == 7) {
		expann::PlanIndex x;
		x.int_mode = int_mode;
		x.dtype = int_mode == expann::kPlanB1Ham ? EXPANN_DTYPE_B1 : EXPANN_DTYPE_I8;
		const expann::ScanPlan p = expann::plan_asym(x, expann::PlanCall{1, k, cap});
		const expann::AsymTiles t = expann::plan_asym_tiles(n, sel_rows, first != 0, last != 0, cap);
		std::printf("%d %d %u %u %u\n", p.status, (int)p.family, t.n_tiles_sel, t.tile_stride, t.fixed);
	}
	return 0;
}
