// pq4_plan_hook.cpp -- plan_pq4 (through plan_scan) of bf_plan.hpp for tests/test_pq4_abi.py.  Each input line
// "metric dim M m k cap" prints "status family direct_tq sampled".
#include <cstdio>

#include "bf_plan.hpp"

int main() {
	int metric, dim, M;
	unsigned long m, k;
	unsigned cap;
	while (std::scanf("%d %d %d %lu %lu %u", &metric, &dim, &M, &m, &k, &cap) == 6) {
		expann::PlanIndex x;
		x.dtype = EXPANN_DTYPE_PQ4;
		x.int_mode = expann::kPlanPQ4;
		x.metric = metric;
		x.dim = dim;
		x.pq_m = M;
		const expann::ScanPlan p = expann::plan_scan(x, expann::PlanCall{m, k, cap}, expann::PlanAttempt{});
		std::printf("%d %d %d %d\n", p.status, (int)p.family, p.direct_tq, (int)p.sampled);
	}
	return 0;
}
