/*
 * expann_oracle_graph.c -- CPU restatement of the query side of the reference's graph engine, and of
 * the batched builder of include/expann_hip.h (expann_graph_build_batched) at the end of the file.
 * TEST INFRASTRUCTURE ONLY (see expann_oracle.h).  Each function cites src/antitopo_engine.h.
 */
#include "expann_oracle.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct oracle_graph {
	size_t n, dim, starting_vertex, max_layer;
	float* vectors;        /* all_entries */
	uint8_t* compressed;   /* quantizer_simple<uint8_t>::stored, built lazily (:485-486) */
	size_t* n_layers;      /* per vertex */
	size_t** n_edges;      /* [v][layer] */
	uint64_t*** adj;       /* [v][layer][edge] = hadj_flat */
	char* visited;
	size_t* visited_recent;
	size_t n_recent;
};

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

/* src/antitopo_engine.h:994-1074 */
oracle_graph* oracle_graph_load(const char* path) {
	FILE* f = fopen(path, "rb");
	if (!f)
		return NULL;
	oracle_graph* g = (oracle_graph*)calloc(1, sizeof(*g));
	uint64_t sv, M, M0, efm, tmp, efc, oc, po, ml, n;
	uint8_t has_ef, uc, ul;
	float of, ob;
	int ok = rd(f, &sv, 8) && rd(f, &M, 8) && rd(f, &M0, 8) && rd(f, &efm, 8) && rd(f, &has_ef, 1);
	if (ok && has_ef)
		ok = rd(f, &tmp, 8);
	ok = ok && rd(f, &efc, 8) && rd(f, &oc, 8) && rd(f, &of, 4) && rd(f, &ob, 4) && rd(f, &po, 8) &&
	     rd(f, &uc, 1) && rd(f, &ul, 1) && rd(f, &ml, 8) && rd(f, &n, 8);
	if (!ok)
		goto fail;
	g->starting_vertex = sv;
	g->max_layer = ml;
	g->n = n;
	for (uint64_t i = 0; i < n; ++i) {
		uint64_t len;
		if (!rd(f, &len, 8))
			goto fail;
		if (i == 0) {
			g->dim = len;
			g->vectors = (float*)malloc(sizeof(float) * n * len);
		}
		if (len != g->dim || !rd(f, g->vectors + i * g->dim, 4 * len))
			goto fail;
	}
	uint64_t nv;
	if (!rd(f, &nv, 8) || nv != n)
		goto fail;
	g->n_layers = (size_t*)calloc(n, sizeof(size_t));
	g->n_edges = (size_t**)calloc(n, sizeof(size_t*));
	g->adj = (uint64_t***)calloc(n, sizeof(uint64_t**));
	for (uint64_t v = 0; v < n; ++v) {
		uint64_t nl;
		if (!rd(f, &nl, 8))
			goto fail;
		g->n_layers[v] = nl;
		g->n_edges[v] = (size_t*)calloc(nl ? nl : 1, sizeof(size_t));
		g->adj[v] = (uint64_t**)calloc(nl ? nl : 1, sizeof(uint64_t*));
		for (uint64_t l = 0; l < nl; ++l) {
			uint64_t ne;
			if (!rd(f, &ne, 8))
				goto fail;
			g->n_edges[v][l] = ne;
			g->adj[v][l] = (uint64_t*)malloc(sizeof(uint64_t) * (ne ? ne : 1));
			for (uint64_t e = 0; e < ne; ++e) {
				float len;
				if (!rd(f, &len, 4) || !rd(f, &g->adj[v][l][e], 8))
					goto fail;
			}
		}
	}
	fclose(f);
	g->visited = (char*)calloc(n, 1);
	g->visited_recent = (size_t*)malloc(sizeof(size_t) * (n + 1));
	return g;
fail:
	fclose(f);
	oracle_graph_destroy(g);
	return NULL;
}

void oracle_graph_destroy(oracle_graph* g) {
	if (!g)
		return;
	if (g->adj)
		for (size_t v = 0; v < g->n; ++v) {
			if (g->adj[v])
				for (size_t l = 0; l < g->n_layers[v]; ++l)
					free(g->adj[v][l]);
			free(g->adj[v]);
			if (g->n_edges)
				free(g->n_edges[v]);
		}
	free(g->adj);
	free(g->n_edges);
	free(g->n_layers);
	free(g->vectors);
	free(g->compressed);
	free(g->visited);
	free(g->visited_recent);
	free(g);
}
size_t oracle_graph_size(const oracle_graph* g) { return g->n; }
size_t oracle_graph_dim(const oracle_graph* g) { return g->dim; }
const float* oracle_graph_vectors(const oracle_graph* g) { return g->vectors; }

/* ---- libstdc++ heap algorithms on (dist, id) pairs, comparator on .first only ------------- */
typedef struct {
	float d;
	uint64_t id;
} md_t;
typedef struct {
	md_t* v;
	size_t n, cap;
	int max_heap; /* 1: worst_elem (a.first < b.first), top = largest; 0: best_elem, top = smallest */
} pq_t;
static inline int pq_less(const pq_t* h, md_t a, md_t b) {
	return h->max_heap ? (a.d < b.d) : (a.d > b.d);
}
static void pq_init(pq_t* h, int max_heap) {
	h->cap = 64;
	h->v = (md_t*)malloc(sizeof(md_t) * h->cap);
	h->n = 0;
	h->max_heap = max_heap;
}
static void pq_push_up(pq_t* h, size_t hole, size_t top, md_t value) { /* std::__push_heap */
	while (hole > top) {
		size_t parent = (hole - 1) / 2;
		if (!pq_less(h, h->v[parent], value))
			break;
		h->v[hole] = h->v[parent];
		hole = parent;
	}
	h->v[hole] = value;
}
static void pq_adjust(pq_t* h, size_t hole, size_t len, md_t value) { /* std::__adjust_heap */
	const size_t top = hole;
	size_t child = hole;
	while (len > 1 && child < (len - 1) / 2) {
		child = 2 * (child + 1);
		if (pq_less(h, h->v[child], h->v[child - 1]))
			--child;
		h->v[hole] = h->v[child];
		hole = child;
	}
	if ((len & 1) == 0 && len >= 2 && child == (len - 2) / 2) {
		child = 2 * (child + 1);
		h->v[hole] = h->v[child - 1];
		hole = child - 1;
	}
	pq_push_up(h, hole, top, value);
}
static void pq_push(pq_t* h, md_t e) {
	if (h->n == h->cap) {
		h->cap *= 2;
		h->v = (md_t*)realloc(h->v, sizeof(md_t) * h->cap);
	}
	h->v[h->n++] = e;
	pq_push_up(h, h->n - 1, 0, e);
}
static void pq_pop(pq_t* h) {
	if (h->n > 1) {
		md_t value = h->v[h->n - 1];
		h->v[h->n - 1] = h->v[0];
		pq_adjust(h, 0, h->n - 1, value);
	}
	h->n--;
}

static void pq_make(pq_t* h) { /* std::__make_heap (priority_queue's range constructor, :551-558) */
	const size_t len = h->n;
	if (len < 2)
		return;
	for (size_t parent = (len - 2) / 2;; --parent) {
		md_t value = h->v[parent];
		pq_adjust(h, parent, len, value);
		if (parent == 0)
			break;
	}
}

/* Test hook: run a trace of queue operations through pq_* (the heap code search_bottom uses) so
 * that tests/test_oracle.py can compare it with the same trace run through the image's real
 * libstdc++ (tests/golden/heap_ref.json, oracle/ref/heap_ref.cpp).  ops[i] 1 = push (op_d[i],
 * op_id[i]), 0 = pop.  Entry 0 of the out_* arrays is the state after construction from the
 * init range, entry i + 1 the state after op i (size 0: top fields 0).  Returns the drain length. */
size_t oracle_heap_trace(int max_heap, size_t n_init, const float* init_d, const uint64_t* init_id,
                         size_t n_ops, const int* ops, const float* op_d, const uint64_t* op_id,
                         uint64_t* out_size, float* out_top_d, uint64_t* out_top_id, float* drain_d,
                         uint64_t* drain_id) {
	pq_t h;
	pq_init(&h, max_heap);
	for (size_t i = 0; i < n_init; ++i) {
		if (h.n == h.cap) {
			h.cap *= 2;
			h.v = (md_t*)realloc(h.v, sizeof(md_t) * h.cap);
		}
		h.v[h.n].d = init_d[i];
		h.v[h.n].id = init_id[i];
		h.n++;
	}
	pq_make(&h);
	for (size_t i = 0;; ++i) {
		out_size[i] = h.n;
		out_top_d[i] = h.n ? h.v[0].d : 0.0f;
		out_top_id[i] = h.n ? h.v[0].id : 0;
		if (i == n_ops)
			break;
		if (ops[i] == 1) {
			md_t e = {op_d[i], op_id[i]};
			pq_push(&h, e);
		} else if (h.n) {
			pq_pop(&h);
		}
	}
	size_t nd = 0;
	while (h.n) {
		drain_d[nd] = h.v[0].d;
		drain_id[nd] = h.v[0].id;
		++nd;
		pq_pop(&h);
	}
	free(h.v);
	return nd;
}

/* src/antitopo_engine.h:25-37 (DIM % 128 == 0 -> src/distance.h:86-111) */
static inline float g_dist2(const oracle_graph* g, const float* a, const float* b) {
	return oracle_l2_f32(a, b, g->dim);
}

/* Bottom-layer best-first search shared by :495-708 (fp32) and :710-851 (uint8). */
static size_t search_bottom(oracle_graph* g, const float* q, uint64_t entry_point, size_t k,
                            int compressed, md_t* out, uint64_t* n_distcomps) {
	pq_t candidates, nearest;
	pq_init(&candidates, 0);
	pq_init(&nearest, 1);
#define SCORE(idx)                                                                               \
	(++*n_distcomps, compressed ? (float)oracle_l2_u8_compressed(q, g->compressed + (idx)*g->dim, g->dim) \
	                            : g_dist2(g, q, g->vectors + (idx)*g->dim))
	md_t e0 = {SCORE(entry_point), entry_point};
	pq_push(&candidates, e0); /* one entry point: make_heap of one element */
	pq_push(&nearest, e0);
	while (nearest.n > k)
		pq_pop(&nearest);
	g->visited[entry_point] = 1;
	g->n_recent = 0;
	g->visited_recent[g->n_recent++] = entry_point;
	size_t nl_cap = 256, nl_n;
	uint64_t* neighbour_list = (uint64_t*)malloc(sizeof(uint64_t) * nl_cap);
	while (candidates.n) {
		md_t cur = candidates.v[0];
		pq_pop(&candidates);
		if (cur.d > nearest.v[0].d && nearest.n == k) /* :588-590 / :774-776 */
			break;
		nl_n = 0;
		const size_t ne = g->n_layers[cur.id] ? g->n_edges[cur.id][0] : 0;
		for (size_t i = 0; i < ne; ++i) {
			uint64_t nb = g->adj[cur.id][0][i];
			if (!g->visited[nb]) {
				if (nl_n == nl_cap) {
					nl_cap *= 2;
					neighbour_list = (uint64_t*)realloc(neighbour_list, sizeof(uint64_t) * nl_cap);
				}
				neighbour_list[nl_n++] = nb;
				g->visited[nb] = 1;
				g->visited_recent[g->n_recent++] = nb;
			}
		}
		for (size_t i = 0; i < nl_n; ++i) { /* :636-689 / :795-835 */
			uint64_t next = neighbour_list[i];
			float dn = SCORE(next);
			if (nearest.n < k || dn < nearest.v[0].d) {
				md_t e = {dn, next};
				pq_push(&candidates, e);
				pq_push(&nearest, e);
				if (nearest.n > k)
					pq_pop(&nearest);
			}
		}
	}
#undef SCORE
	for (size_t i = 0; i < g->n_recent; ++i)
		g->visited[g->visited_recent[i]] = 0;
	g->n_recent = 0;
	size_t cnt = nearest.n;
	for (size_t i = cnt; i-- > 0;) { /* drain (worst first) then reverse */
		out[i] = nearest.v[0];
		pq_pop(&nearest);
	}
	free(neighbour_list);
	free(candidates.v);
	free(nearest.v);
	return cnt;
}

/* src/antitopo_engine.h:853-928 */
size_t oracle_graph_query_k(oracle_graph* g, const float* q, size_t k, size_t ef_search,
                            int use_compression, uint64_t* ids, float* dists,
                            uint64_t* n_distcomps) {
	uint64_t dc = 0;
	if (use_compression && !g->compressed) { /* :485-486 -> src/quantizer.h:132-141 */
		g->compressed = (uint8_t*)malloc(g->n * g->dim);
		oracle_quantize_simple_u8(g->vectors, g->n * g->dim, g->compressed);
	}
	uint64_t entry_point = g->starting_vertex;
	++dc;
	float ep_dist = g_dist2(g, g->vectors + entry_point * g->dim, q); /* :866-869 */
	for (size_t layer = g->max_layer - 1; layer > 0; --layer) {       /* :879-893 */
		int changed = 1;
		while (changed) {
			changed = 0;
			const uint64_t* nbrs = g->adj[entry_point][layer]; /* list bound at loop start */
			const size_t ne = g->n_edges[entry_point][layer];
			for (size_t i = 0; i < ne; ++i) {
				++dc;
				float nd = g_dist2(g, g->vectors + nbrs[i] * g->dim, q);
				if (nd < ep_dist) {
					entry_point = nbrs[i];
					ep_dist = nd;
					changed = 1;
				}
			}
		}
	}
	md_t* ret = (md_t*)malloc(sizeof(md_t) * (ef_search + 1));
	size_t cnt = search_bottom(g, q, entry_point, ef_search, use_compression, ret, &dc);
	if (use_compression) /* :845-848 final re-score, order kept */
		for (size_t i = 0; i < cnt; ++i)
			ret[i].d = g_dist2(g, g->vectors + ret[i].id * g->dim, q);
	if (cnt > k)
		cnt = k; /* :914-919 */
	for (size_t i = 0; i < cnt; ++i) {
		ids[i] = ret[i].id;
		if (dists)
			dists[i] = ret[i].d;
	}
	free(ret);
	if (n_distcomps)
		*n_distcomps = dc;
	return cnt;
}

/* ---- the batched builder (include/expann_hip.h: expann_graph_build_batched) ---------------------
 * Written from the reference's _store_vector / prune_edges / query_k_at_layer
 * (src/antitopo_engine.h:263-465, :495-708, ortho_count = 1) and the contract in the header, on the
 * ABI's own strided arrays.  A batch [b0, b1) is inserted against the graph as it stood before the
 * batch: all searches first, then prune_edges on every new row, then the reverse edges in ascending
 * new-vertex order, then prune_edges once on every row whose length passed its cap. */
typedef struct {
	size_t dim, n, M, M0, ef, prune_overflow, stride0, strideu, U;
	float ortho_factor, ortho_bias;
	const float* vec;
	const int32_t* upper_idx;
	uint32_t *ids0, *deg0, *idsu, *degu;
	float *d0, *du;
	uint8_t *ordered0, *orderedu;
	float* pair; /* [n][n] memo of g_dist2 between rows (small n only), bits 0xFFFFFFFF = not yet */
	char* visited;
	size_t* recent;
	uint64_t hazards, dropped, repruned;
} bb_t;

static inline size_t bb_urow(const bb_t* b, size_t l, size_t v) {
	return (l - 1) * b->U + (size_t)b->upper_idx[v];
}
static inline uint32_t* bb_ids(const bb_t* b, size_t l, size_t v) {
	return l == 0 ? b->ids0 + v * b->stride0 : b->idsu + bb_urow(b, l, v) * b->strideu;
}
static inline float* bb_d(const bb_t* b, size_t l, size_t v) {
	return l == 0 ? b->d0 + v * b->stride0 : b->du + bb_urow(b, l, v) * b->strideu;
}
static inline uint32_t* bb_deg(const bb_t* b, size_t l, size_t v) {
	return l == 0 ? b->deg0 + v : b->degu + bb_urow(b, l, v);
}
static inline void bb_set_ordered(const bb_t* b, size_t l, size_t v, uint8_t x) {
	if (l == 0 ? b->ordered0 != NULL : b->orderedu != NULL)
		*(l == 0 ? b->ordered0 + v : b->orderedu + bb_urow(b, l, v)) = x;
}
static inline size_t bb_cap(const bb_t* b, size_t l) { return l == 0 ? b->M0 : b->M; }
static inline size_t bb_stride(const bb_t* b, size_t l) { return l == 0 ? b->stride0 : b->strideu; }
/* the entries of a row a reader may look at: the counter can stand past the stride */
static inline size_t bb_len(const bb_t* b, size_t l, size_t v) {
	const size_t deg = *bb_deg(b, l, v), st = bb_stride(b, l);
	return deg < st ? deg : st;
}
/* dist2(all_entries[x], all_entries[y]), src/antitopo_engine.h:25-37: the same bits in either order */
static float bb_dist(bb_t* b, size_t x, size_t y) {
	if (!b->pair)
		return oracle_l2_f32(b->vec + x * b->dim, b->vec + y * b->dim, b->dim);
	float* p = b->pair + x * b->n + y;
	uint32_t bits;
	memcpy(&bits, p, 4);
	if (bits == 0xFFFFFFFFu) {
		*p = oracle_l2_f32(b->vec + x * b->dim, b->vec + y * b->dim, b->dim);
		b->pair[y * b->n + x] = *p;
	}
	return *p;
}

static int bb_cmp_bits(const void* x, const void* y) {
	uint32_t a, c;
	memcpy(&a, x, 4);
	memcpy(&c, y, 4);
	return a < c ? -1 : a > c;
}
/* pairs of entries with bit-equal values */
static uint64_t bb_tie_pairs(float* d, size_t n) {
	uint64_t pairs = 0;
	qsort(d, n, sizeof(float), bb_cmp_bits);
	for (size_t i = 0; i < n;) {
		size_t j = i + 1;
		while (j < n && memcmp(d + i, d + j, 4) == 0)
			++j;
		pairs += (uint64_t)(j - i) * (j - i - 1) / 2;
		i = j;
	}
	return pairs;
}

typedef struct {
	float* v;
	size_t n, cap;
} fvec_t;
static void fvec_push(fvec_t* f, float x) {
	if (f->n == f->cap) {
		f->cap = f->cap ? 2 * f->cap : 256;
		f->v = (float*)realloc(f->v, sizeof(float) * f->cap);
	}
	f->v[f->n++] = x;
}

/* query_k_at_layer (:495-708) for one entry point, plain distances, on layer `layer` of the strided
 * rows; out receives at most ef pairs, nearest first */
static size_t bb_search_layer(bb_t* b, size_t q, size_t layer, uint64_t entry_point, md_t* out, fvec_t* pushed) {
	const size_t k = b->ef;
	pq_t candidates, nearest;
	pq_init(&candidates, 0);
	pq_init(&nearest, 1);
	size_t n_recent = 0;
	pushed->n = 0;
	md_t e0 = {bb_dist(b, entry_point, q), entry_point};
	pq_push(&candidates, e0);
	pq_push(&nearest, e0);
	fvec_push(pushed, e0.d);
	b->visited[entry_point] = 1;
	b->recent[n_recent++] = entry_point;
	uint64_t* neighbour_list = (uint64_t*)malloc(sizeof(uint64_t) * (bb_stride(b, layer) + 1));
	while (candidates.n) {
		md_t cur = candidates.v[0];
		pq_pop(&candidates);
		if (cur.d > nearest.v[0].d && nearest.n == k) /* :588-590 */
			break;
		size_t nl_n = 0;
		const uint32_t* row = bb_ids(b, layer, cur.id);
		const size_t ne = bb_len(b, layer, cur.id);
		for (size_t i = 0; i < ne; ++i) {
			const uint64_t nb = row[i];
			if (!b->visited[nb]) {
				neighbour_list[nl_n++] = nb;
				b->visited[nb] = 1;
				b->recent[n_recent++] = nb;
			}
		}
		for (size_t i = 0; i < nl_n; ++i) { /* :636-689 */
			const uint64_t next = neighbour_list[i];
			const float dn = bb_dist(b, next, q);
			if (nearest.n < k || dn < nearest.v[0].d) {
				md_t e = {dn, next};
				pq_push(&candidates, e);
				pq_push(&nearest, e);
				fvec_push(pushed, dn);
				if (nearest.n > k)
					pq_pop(&nearest);
			}
		}
	}
	for (size_t i = 0; i < n_recent; ++i)
		b->visited[b->recent[i]] = 0;
	const size_t cnt = nearest.n;
	for (size_t i = cnt; i-- > 0;) { /* drain (worst first) then reverse */
		out[i] = nearest.v[0];
		pq_pop(&nearest);
	}
	b->hazards += bb_tie_pairs(pushed->v, pushed->n);
	free(neighbour_list);
	free(candidates.v);
	free(nearest.v);
	return cnt;
}

static int bb_cmp_md(const void* x, const void* y) { /* std::pair<float, size_t> operator< */
	const md_t* a = (const md_t*)x;
	const md_t* c = (const md_t*)y;
	if (a->d != c->d)
		return a->d < c->d ? -1 : 1;
	return a->id < c->id ? -1 : a->id > c->id;
}

/* prune_edges (:263-308) over `C` candidates; the survivors become row (layer, from).  The
 * reference evaluates score() of every candidate from scratch in every round; here a candidate
 * keeps where that loop stood (res, leniency, how many of `ret` it has seen) and resumes it when
 * `ret` has grown: the same operations on the same values in the same order. */
static void bb_prune(bb_t* b, size_t layer, size_t from, md_t* cand, size_t C) {
	const size_t cap = bb_cap(b, layer);
	const float prune_score = 3.402823466e+38f; /* std::numeric_limits<float>::max() */
	qsort(cand, C, sizeof(md_t), bb_cmp_md);     /* sort + std::set: (distance, id) order */
	float* res = (float*)malloc(sizeof(float) * (C + 1));
	size_t* leniency = (size_t*)malloc(sizeof(size_t) * (C + 1));
	size_t* seen = (size_t*)malloc(sizeof(size_t) * (C + 1));
	char* gone = (char*)calloc(C + 1, 1);
	size_t* ret = (size_t*)malloc(sizeof(size_t) * (cap + 1));
	size_t n_ret = 0, n_left = C;
	for (size_t c = 0; c < C; ++c) {
		res[c] = cand[c].d;
		leniency[c] = b->prune_overflow + 1;
		seen[c] = 0;
	}
	while (n_ret < cap && n_left) {
		size_t best = C;
		float best_s = 0.0f;
		for (size_t c = 0; c < C; ++c) {
			if (gone[c])
				continue;
			const float basic_dist = cand[c].d;
			while (res[c] != prune_score && seen[c] < n_ret) {
				const float co_dist = bb_dist(b, cand[ret[seen[c]]].id, cand[c].id);
				++seen[c];
				if (co_dist < basic_dist) {
					res[c] += b->ortho_factor * (basic_dist - co_dist) + b->ortho_bias;
					if (--leniency[c] == 0)
						res[c] = prune_score;
				}
			}
			if (best == C || res[c] < best_s) { /* std::ranges::min_element: the first minimum */
				best = c;
				best_s = res[c];
			}
		}
		if (best_s == prune_score)
			break;
		ret[n_ret++] = best;
		gone[best] = 1;
		--n_left;
	}
	uint32_t* ids = bb_ids(b, layer, from);
	float* ds = bb_d(b, layer, from);
	/* (cand may alias nothing of the row: callers hand in a copy) */
	for (size_t i = 0; i < n_ret; ++i) {
		ids[i] = (uint32_t)cand[ret[i]].id;
		ds[i] = cand[ret[i]].d;
	}
	*bb_deg(b, layer, from) = (uint32_t)n_ret;
	bb_set_ordered(b, layer, from, 1);
	free(res);
	free(leniency);
	free(seen);
	free(gone);
	free(ret);
}

size_t oracle_graph_batch_end(const uint8_t* levels, size_t n, size_t b0, uint32_t max_layer, size_t max_batch) {
	if (max_batch == 0)
		max_batch = 32768;
	size_t step = b0 / 16 ? b0 / 16 : 1;
	if (step > max_batch)
		step = max_batch;
	size_t b1 = b0 + step < n ? b0 + step : n;
	for (size_t v = b0; v < b1; ++v)
		if (levels[v] >= max_layer) { /* a vertex that opens a layer goes alone */
			b1 = v == b0 ? v + 1 : v;
			break;
		}
	return b1;
}

int oracle_graph_build_batched(size_t dim, const float* vectors, size_t n, const uint8_t* levels, size_t n_built,
                               uint32_t* max_layer_io, uint32_t* starting_vertex_io, size_t M, size_t M0,
                               size_t ef_construction, size_t prune_overflow, float ortho_factor, float ortho_bias,
                               size_t max_batch, uint32_t* ids0, float* d0, uint32_t* deg0, size_t stride0,
                               const int32_t* upper_idx, size_t U, size_t n_upper_layers, uint32_t* idsu, float* du,
                               uint32_t* degu, size_t strideu, uint64_t* stats, uint64_t* tie_hazards,
                               uint8_t* ordered0, uint8_t* orderedu) {
	if (!vectors || !levels || !max_layer_io || !starting_vertex_io || !ids0 || !d0 || !deg0 || !upper_idx ||
	    dim == 0 || dim % 16 != 0 || n == 0 || n_built == 0 || n_built > n || M < 2 || M0 < M || stride0 < M0 ||
	    (n_upper_layers && (!idsu || !du || !degu || strideu < M)) || ef_construction == 0 ||
	    *max_layer_io == 0 || *max_layer_io > n_upper_layers + 1 || *starting_vertex_io >= n_built)
		return -1;
	for (size_t v = 0; v < n; ++v)
		if (levels[v] > n_upper_layers || (levels[v] >= 1) != (upper_idx[v] >= 0) ||
		    (upper_idx[v] >= 0 && (size_t)upper_idx[v] >= U))
			return -1;
	bb_t b;
	memset(&b, 0, sizeof(b));
	b.dim = dim; b.n = n; b.M = M; b.M0 = M0; b.ef = ef_construction; b.prune_overflow = prune_overflow;
	b.stride0 = stride0; b.strideu = strideu; b.U = U;
	b.ortho_factor = ortho_factor; b.ortho_bias = ortho_bias;
	b.vec = vectors; b.upper_idx = upper_idx;
	b.ids0 = ids0; b.d0 = d0; b.deg0 = deg0; b.idsu = idsu; b.du = du; b.degu = degu;
	b.ordered0 = ordered0; b.orderedu = orderedu;
	if (ordered0)
		memset(ordered0, 0, n);
	if (orderedu)
		memset(orderedu, 0, U * n_upper_layers);
	if (n <= 4096) {
		b.pair = (float*)malloc(sizeof(float) * n * n);
		memset(b.pair, 0xFF, sizeof(float) * n * n);
	}
	b.visited = (char*)calloc(n, 1);
	b.recent = (size_t*)malloc(sizeof(size_t) * (n + 1));
	size_t max_layer = *max_layer_io, starting_vertex = *starting_vertex_io;
	uint64_t n_batches = 0;
	fvec_t tmp = {NULL, 0, 0};
	size_t n_dirty_cap = 256, n_dirty;
	size_t(*dirty)[2] = malloc(sizeof(size_t[2]) * n_dirty_cap);
	const size_t max_stride = stride0 > strideu ? stride0 : strideu;
	md_t* rowcopy = (md_t*)malloc(sizeof(md_t) * (max_stride + 1));
	size_t b0 = n_built;
	while (b0 < n) {
		const size_t b1 = oracle_graph_batch_end(levels, n, b0, (uint32_t)max_layer, max_batch);
		const size_t B = b1 - b0;
		/* searches (:333-428): every new vertex against the graph before the batch */
		md_t*** lists = (md_t***)calloc(B, sizeof(md_t**));
		size_t** counts = (size_t**)calloc(B, sizeof(size_t*));
		for (size_t v = b0; v < b1; ++v) {
			const size_t new_max_layer = levels[v];
			uint64_t entry_point = starting_vertex;
			float ep_dist = bb_dist(&b, entry_point, v);
			for (size_t layer = max_layer - 1; layer > new_max_layer; --layer) { /* :353-370 */
				int changed = 1;
				while (changed) {
					changed = 0;
					const uint32_t* row = bb_ids(&b, layer, entry_point); /* the list the loop started on */
					const size_t ne = bb_len(&b, layer, entry_point);
					tmp.n = 0;
					fvec_push(&tmp, ep_dist);
					for (size_t i = 0; i < ne; ++i) {
						const float neighbour_dist = bb_dist(&b, row[i], v);
						fvec_push(&tmp, neighbour_dist);
						if (neighbour_dist < ep_dist) {
							entry_point = row[i];
							ep_dist = neighbour_dist;
							changed = 1;
						}
					}
					b.hazards += bb_tie_pairs(tmp.v, tmp.n);
				}
			}
			const size_t top = new_max_layer < max_layer - 1 ? new_max_layer : max_layer - 1;
			lists[v - b0] = (md_t**)calloc(top + 1, sizeof(md_t*));
			counts[v - b0] = (size_t*)calloc(top + 1, sizeof(size_t));
			for (size_t layer = top + 1; layer-- > 0;) { /* :382-425 */
				md_t* out = (md_t*)malloc(sizeof(md_t) * (ef_construction + 1));
				counts[v - b0][layer] = bb_search_layer(&b, v, layer, entry_point, out, &tmp);
				lists[v - b0][layer] = out;
				entry_point = out[0].id;
			}
		}
		/* the new rows (:437-440) */
		for (size_t v = b0; v < b1; ++v) {
			const size_t top = (size_t)levels[v] < max_layer - 1 ? (size_t)levels[v] : max_layer - 1;
			for (size_t layer = 0; layer <= top; ++layer)
				bb_prune(&b, layer, v, lists[v - b0][layer], counts[v - b0][layer]);
		}
		/* reverse edges (:442-455), ascending new vertex; a row takes `stride` entries and counts on */
		n_dirty = 0;
		for (size_t v = b0; v < b1; ++v) {
			const size_t top = (size_t)levels[v] < max_layer - 1 ? (size_t)levels[v] : max_layer - 1;
			for (size_t layer = 0; layer <= top; ++layer) {
				const size_t deg = *bb_deg(&b, layer, v);
				const uint32_t* ids = bb_ids(&b, layer, v);
				const float* ds = bb_d(&b, layer, v);
				for (size_t i = 0; i < deg; ++i) {
					const size_t nb = ids[i];
					const size_t slot = (*bb_deg(&b, layer, nb))++;
					if (slot < bb_stride(&b, layer)) {
						bb_ids(&b, layer, nb)[slot] = (uint32_t)v;
						bb_d(&b, layer, nb)[slot] = ds[i];
					} else {
						++b.dropped;
					}
					bb_set_ordered(&b, layer, nb, 0);
					if (slot == bb_cap(&b, layer)) { /* the row has passed its cap (:270) */
						if (n_dirty == n_dirty_cap) {
							n_dirty_cap *= 2;
							dirty = realloc(dirty, sizeof(size_t[2]) * n_dirty_cap);
						}
						dirty[n_dirty][0] = nb;
						dirty[n_dirty][1] = layer;
						++n_dirty;
					}
				}
			}
		}
		/* one prune_edges for every such row */
		for (size_t t = 0; t < n_dirty; ++t) {
			const size_t v = dirty[t][0], layer = dirty[t][1];
			const size_t len = bb_len(&b, layer, v);
			const uint32_t* ids = bb_ids(&b, layer, v);
			const float* ds = bb_d(&b, layer, v);
			for (size_t i = 0; i < len; ++i) {
				rowcopy[i].d = ds[i];
				rowcopy[i].id = ids[i];
			}
			bb_prune(&b, layer, v, rowcopy, len);
		}
		b.repruned += n_dirty;
		for (size_t v = b0; v < b1; ++v) {
			const size_t top = (size_t)levels[v] < max_layer - 1 ? (size_t)levels[v] : max_layer - 1;
			for (size_t layer = 0; layer <= top; ++layer)
				free(lists[v - b0][layer]);
			free(lists[v - b0]);
			free(counts[v - b0]);
		}
		free(lists);
		free(counts);
		for (size_t v = b0; v < b1; ++v) /* :459-462 */
			while (levels[v] >= max_layer) {
				++max_layer;
				starting_vertex = v;
			}
		++n_batches;
		b0 = b1;
	}
	*max_layer_io = (uint32_t)max_layer;
	*starting_vertex_io = (uint32_t)starting_vertex;
	if (stats) {
		stats[0] = n_batches;
		stats[1] = b.dropped;
		stats[2] = b.repruned;
		stats[3] = 0;
	}
	if (tie_hazards)
		*tie_hazards = b.hazards;
	free(rowcopy);
	free(dirty);
	free(tmp.v);
	free(b.recent);
	free(b.visited);
	free(b.pair);
	return 0;
}
