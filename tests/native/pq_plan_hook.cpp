// pq_plan_hook.cpp -- plan_pq (through plan_scan) and plan_pq_chunks of bf_plan.hpp for tests/test_pq_abi.py.  Each
// input line "metric dim M m k cap query_tile n_groups n_qtiles slots" prints "status family direct_tq sampled chunks".
#include <cstdio>

#include "bf_plan.hpp"

int main() {
	int metric, dim, M;
	unsigned long m, k;
	unsigned cap, n_groups, n_qtiles, slots;
	long query_tile;
	while (std::scanf("%d %d %d %lu %lu %u %ld %u %u %u", &metric, &dim, &M, &m, &k, &cap, &query_tile, &n_groups, &n_qtiles,
	                  &slots) == 10) {
		expann::PlanIndex x;
		x.dtype = EXPANN_DTYPE_PQ8;
		x.int_mode = expann::kPlanPQ;
		x.metric = metric;
		x.dim = dim;
		x.pq_m = M;
		x.query_tile = query_tile;
		const expann::ScanPlan p = expann::plan_scan(x, expann::PlanCall{m, k, cap}, expann::PlanAttempt{});
		std::printf("%d %d %d %d %u\n", p.status, (int)p.family, p.direct_tq, (int)p.sampled,
		            expann::plan_pq_chunks(n_groups, n_qtiles, slots, dim, M));
	}
	return 0;
}
