/*
 * expann_hip.h -- C ABI of the MI355X-native distance + top-k engine (libexpann_hip.so).
 *
 * This is the drop-in boundary for expANN's hot path: the entry points are what a C++
 * engine class satisfying the reference's CRTP `ann_engine<T, Derived>` interface
 * (upstream src/ann_engine.h:16-29) binds to.  Plain pointers and sizes only; no C++
 * types, no exceptions, no torch types cross this boundary.  Every call returns an int
 * status (EXPANN_OK == 0); the message of the last failure on a handle is available from
 * expann_last_error().  A handle is single-caller; distinct handles may be used from
 * different host threads concurrently (the reference runs one private engine per job
 * thread, src/bench_runner.h:30-57,78-87).
 *
 * There is no CPU fallback behind this ABI: without a usable HIP device every compute
 * entry point fails with EXPANN_ERR_NO_DEVICE.
 */
#ifndef EXPANN_HIP_H
#define EXPANN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: expann_profile grew (deferred_searches); expann_sharded_* gained the device-resident in-process
 * search, the all-to-all exchange pattern and its caller-transport hook */
#define EXPANN_ABI_VERSION 2

enum expann_status {
	EXPANN_OK = 0,
	EXPANN_ERR_INVALID_ARG = 1,
	EXPANN_ERR_NO_DEVICE = 2,
	EXPANN_ERR_HIP = 3,
	EXPANN_ERR_NOT_BUILT = 4,
	EXPANN_ERR_UNSUPPORTED = 5,
	EXPANN_ERR_OVERFLOW = 6 /* internal candidate buffers exhausted even after retries */
};

/* element type of the stored rows */
enum expann_dtype {
	EXPANN_DTYPE_F32 = 0, /* vec<float> rows, src/vec.h:17-23                         */
	EXPANN_DTYPE_U8 = 1,  /* quantizer_simple<uint8_t> rows, src/quantizer.h:127      */
	EXPANN_DTYPE_I8 = 2,  /* quantizer_ranged_q8 rows, src/quantizer.h:152-238        */
	EXPANN_DTYPE_I16 = 3, /* int16 rows scored by src/distance.h:14-27 bit for bit
	                       * (distance_compare_avx512f_i32: 16-bit wrapping arithmetic,
	                       * exact only while |a_i - b_i| <= 181); EXPANN_METRIC_L2 only,
	                       * dim 64 or 128; queries int16                            */
	EXPANN_DTYPE_F16 = 4  /* IEEE binary16 rows, see below (appended; EXPANN_ABI_VERSION stays 2:
	                       * nothing that existed changed)                            */
};
/* EXPANN_DTYPE_F16: rows are IEEE binary16, [n][dim], 2 bytes per element -- in expann_add's staging, on the
 * device and for expann_set_base_device -- and stay binary16 on the device (expann_get_stat "base_bytes").  Queries
 * are fp32 [m][dim], as for F32 and U8 rows.  Metrics EXPANN_METRIC_L2 and EXPANN_METRIC_IP (anything else
 * EXPANN_ERR_INVALID_ARG); dim: the f32 rule (any multiple of 16 up to 4096).
 * THE RULE: every entry point returns, bit for bit (ids and fp32 distance bits, ties by lower id, padding as
 * everywhere), what an EXPANN_DTYPE_F32 index holding (float)row would return -- the reference's FMA lane order on
 * the exactly converted values.  binary16 subnormals convert exactly, nothing is flushed; rows with +-inf or NaN
 * behave as the same values do in an F32 index.  Covered: expann_search and expann_search_device (latency mode,
 * "async_search" with expann_sync, k up to 8192), expann_score_ids, expann_set_base_device with id_offset, the
 * row filter, and the expann_sharded_* handles created with this dtype.
 * How: the fp16 filter copy, its row terms and max ||b||^2 are built from the converted values and are the bits
 * the F32 index of the same values builds, so the matrix-core filters, their candidate lists and the speculative
 * thresholds ("spec_rank") run unchanged; the exact side -- the direct scan, the re-rank inside the select
 * kernels, expann_score_ids -- reads the binary16 rows and converts on load (at every dim through the run-time-dim
 * instances).  An F16 index never takes the uint8 shadow ("u8_exact"), the int8 filter ("i8_filter") or the
 * bf16x3 form, which build their operands from fp32 storage: the options are accepted and ignored, "scan_kernel" 3
 * runs the exact direct scan (as do queries outside the fp16 range), as under a row filter. */

/* how a (query, row) pair is scored; smaller score = nearer */
enum expann_metric {
	EXPANN_METRIC_L2 = 0, /* f32: squared L2 in the lane order of src/distance.h:136-147;
	                         u8: src/antitopo_engine.h:38-61 (dist2_compressed);
	                         i8: true sum (a-b)^2                                      */
	EXPANN_METRIC_IP = 1, /* score = -dot (src/distance.h:181-190 for f32); largest
	                         inner product first, ties by lower id                      */
	EXPANN_METRIC_L2_I8_REFCOMPAT = 2 /* i8 only: src/distance.h:29-53 bit for bit,
	                         including its zero-extension of the wrapped difference     */
};

typedef struct expann_index expann_index;

/* library / device ------------------------------------------------------------------ */
int expann_abi_version(void);
/* number of visible HIP devices (0 when there is none or the runtime is unusable). */
int expann_device_count(void);

/* lifecycle (replaces: engine construction, src/bench_runner.h:33) -------------------- */
/* dim: a multiple of 16 (else EXPANN_ERR_INVALID_ARG).  f32 and f16 rows: any such dim up to 4096 (over it:
 * EXPANN_ERR_UNSUPPORTED, checked before the device); 8-bit rows (U8, I8): any multiple of 64 up to 4096
 * (not a multiple of 64: EXPANN_ERR_INVALID_ARG; over 4096: EXPANN_ERR_UNSUPPORTED, checked before the device;
 * 64, 128, 256, 768, 832, 960 have kernels compiled for them, the others run with the dim known at run time --
 * d = 896 on the matrix cores through the 1024-byte-slot form of 832 / 960);
 * int16 rows: 64, 128. */
int expann_create(int dim, int dtype, int metric, int device, expann_index** out);
void expann_destroy(expann_index* h);
/* message of the last error on h (or of the last failed expann_create when h == NULL). */
const char* expann_last_error(const expann_index* h);

/* store_vector x n (src/ann_engine.h:23-25, src/brute_force_engine.h:20-22): rows are
 * COPIED into host staging; the caller keeps ownership.  Row i of the j-th call gets id
 * (rows stored so far) + i, i.e. insertion order, like all_entries.push_back. */
int expann_add(expann_index* h, const void* rows, size_t n);

/* build() (src/ann_engine.h:26, src/brute_force_engine.h:24-26): upload the staged rows
 * to HBM.  Fails with EXPANN_ERR_INVALID_ARG on an empty index (the reference asserts). */
int expann_build(expann_index* h);

/* Adopt rows that already live in device memory (no copy; the caller keeps them alive
 * until expann_destroy).  id_offset is added to every returned id: rank r of a sharded
 * job passes the global number of its first row.  Replaces add+build. */
int expann_set_base_device(expann_index* h, const void* d_rows, size_t n, uint64_t id_offset);

size_t expann_size(const expann_index* h);

/* query_k for a batch (src/ann_engine.h:27-29, src/brute_force_engine.h:28-46; the
 * reference has no batch API -- m = 1 is query_k).  Host buffers.  For each query the k
 * rows with the smallest (score, id), ascending; ids[m][k], dists[m][k] (dists may be
 * NULL).  When fewer than k rows exist the tail is padded with UINT64_MAX / +inf.
 * 1 <= k <= 8192 (half the longest candidate list): a larger k is refused by value with
 * EXPANN_ERR_UNSUPPORTED before any GPU work, whatever the index holds. */
int expann_search(expann_index* h, const void* queries, size_t m, size_t k, uint64_t* ids,
                  float* dists);

/* same with device-resident queries and outputs, enqueued on `stream` (a hipStream_t;
 * NULL = the index's own stream).  The call returns after the stream has drained: the one host
 * synchronisation of a search is the check that no internal candidate list overflowed (the
 * search is re-run with larger lists / the tie-exact kernel if one did). */
int expann_search_device(expann_index* h, const void* d_queries, size_t m, size_t k,
                         uint64_t* d_ids, float* d_dists, void* stream);

/* Deferred check (option "async_search" = 1, device-pointer searches only): expann_search_device
 * enqueues the whole search and returns WITHOUT waiting, so the caller can enqueue what follows
 * (the next batch, the RCCL exchange of a sharded job) while the GPU still scans.  expann_sync
 * waits for the stream of the last such search and reports on all searches since the previous
 * sync: EXPANN_OK, or EXPANN_ERR_OVERFLOW when one of them would have needed the synchronous
 * retry (overflowed candidate lists, queries outside the fp16 range of the index): its results
 * are then invalid and the caller repeats it with "async_search" = 0.  At most 256 searches may
 * be outstanding (further ones wait by themselves).
 * ONE stream at a time: all searches of a handle share one workspace, so a search enqueued on a
 * different stream than the outstanding deferred ones first waits (on the host) until those have
 * drained; deferred searches overlap with each other only in stream order. */
int expann_sync(expann_index* h);

/* k-way merge of per-shard results after an all-gather (RCCL): in_ids/in_dists are
 * [n_lists][m][k], each row ascending by (score, id) and padded as above; out is [m][k].
 * 1 <= n_lists <= 64 and k >= 1, else EXPANN_ERR_INVALID_ARG; m = 0 is EXPANN_OK. */
int expann_merge_topk_device(int device, const uint64_t* d_in_ids, const float* d_in_dists,
                             size_t n_lists, size_t m, size_t k, uint64_t* d_out_ids,
                             float* d_out_dists, void* stream);

/* the same with explicit distances (in elements) between the lists: list g is at
 * d_in_ids + g*ids_stride and d_in_dists + g*dists_stride.  For all-gathered chunks that hold
 * [ids | dists] of one rank each (one collective per exchange instead of two). */
int expann_merge_topk_strided_device(int device, const uint64_t* d_in_ids, const float* d_in_dists,
                                     size_t ids_stride, size_t dists_stride, size_t n_lists, size_t m,
                                     size_t k, uint64_t* d_out_ids, float* d_out_dists, void* stream);

/* row-sharded brute force over the GPUs of one node (SURVEY 8b "create(..., devices, n_dev, ...)",
 * 8e; csrc/expann_sharded.hip) -------------------------------------------------------------------
 * Shard r holds the contiguous rows [r * ceil(N/G), min(N, (r+1) * ceil(N/G))) and searches ALL
 * queries on its own device; the per-shard results [m][k] of (score, global id) are exchanged over
 * RCCL (xGMI) and merged in the reference's (score, id) order, so ids and distances are bit-identical
 * to the single-device index (contiguous ranges + global ids).  Two exchange patterns (option
 * "exchange_pattern"): 2 (default) = an all-to-all of QUERY SLICES -- rank j receives, from every
 * shard, the results of the queries [j * ceil(m/G), ...) and merges those (m/G queries, G lists);
 * the rank form then all-gathers the merged slices; 1 = ONE ncclAllGather of every shard's whole
 * [ids m*k u64 | dists m*k f32] chunk, every rank merges all m queries.  The reference has no
 * counterpart (one engine, one thread: src/basic_bench.h:83-84); the calls mirror the
 * single-device ones above (engine construction src/bench_runner.h:33, store_vector / build /
 * query_k src/ann_engine.h:23-29). */
typedef struct expann_sharded expann_sharded;
/* In-process form: ONE handle drives n_dev devices of this node (one stream and one enqueue thread
 * per device, ncclCommInitAll at build).  devices[] may name a device more than once (several shards
 * on one GPU; the exchange then runs as device copies, RCCL refuses duplicate devices). */
int expann_sharded_create(int dim, int dtype, int metric, const int* devices, int n_dev,
                          expann_sharded** out);
/* One-process-per-GPU form: rank `rank` of `world` ranks on `device`; id128 = the 128 bytes rank 0
 * got from expann_sharded_unique_id (ncclGetUniqueId), distributed by the launcher.  Collective:
 * every rank calls it (ncclCommInitRank).  id128 == NULL: no RCCL communicator -- one rank needs
 * none, more ranks exchange through expann_sharded_set_exchange_fn / _set_alltoallv_fn. */
int expann_sharded_unique_id(void* id128);
int expann_sharded_create_rank(int dim, int dtype, int metric, int device, int rank, int world,
                               const void* id128, expann_sharded** out);
void expann_sharded_destroy(expann_sharded* h);
const char* expann_sharded_last_error(const expann_sharded* h);
/* in-process form: store_vector x n into host staging, then build() cuts the rows into the ranges
 * above and uploads each to its device (as expann_add / expann_build). */
int expann_sharded_add(expann_sharded* h, const void* rows, size_t n);
int expann_sharded_build(expann_sharded* h);
/* Adopt rows already in the shard's device memory (as expann_set_base_device): the rank form's
 * only way to receive rows (shard = 0, id_offset = global number of the rank's first row; n = 0
 * with d_rows = NULL declares the rank's range empty -- the ceil partition leaves trailing ranks
 * without rows when N < G * (G-1) -- and the rank still takes part in every exchange);
 * in-process form: shards in order 0, 1, ... instead of add + build. */
int expann_sharded_set_shard_device(expann_sharded* h, int shard, const void* d_rows, size_t n,
                                    uint64_t id_offset);
size_t expann_sharded_size(const expann_sharded* h);  /* rows over all local shards */
int expann_sharded_shards(const expann_sharded* h);   /* shards in use (rank form: world) */
int expann_sharded_exchange(const expann_sharded* h); /* transport: 0 none (one shard), 1 RCCL, 2 device
                                                         copies, 3 the caller's function */
int expann_sharded_exchange_pattern(const expann_sharded* h); /* 0 none, 1 all-gather of chunks, 2 all-to-all
                                                                 of query slices */
/* ranks of the RCCL communicator as RCCL reports them (ncclCommCount); 0 = no communicator */
int expann_sharded_comm_ranks(const expann_sharded* h);
/* host time the last in-process search spent enqueuing (scan + exchange + merge of all shards, up to
 * the point where the host starts waiting), milliseconds */
double expann_sharded_last_enqueue_ms(const expann_sharded* h);
/* Rank form: the exchange through the caller's transport instead of RCCL (another fabric; ranks
 * that share one GPU, which RCCL refuses; tests).  expann_exchange_fn (pattern 1) gathers `bytes`
 * bytes of device memory d_send from every rank into d_recv (rank r's chunk at r * bytes);
 * expann_alltoallv_fn (pattern 2) sends send_bytes[j] bytes at d_send + send_off[j] to rank j and
 * receives recv_bytes[j] bytes from rank j at d_recv + recv_off[j] (arrays of `world` entries; entry
 * [rank] is always 0 bytes: the library copies what stays).  Both: ordered after the work already
 * on `stream`, complete -- as far as `stream` is concerned -- on return or in stream order; 0 = ok.
 * NULL goes back to the communicator.  With both set, "exchange_pattern" chooses. */
typedef int (*expann_exchange_fn)(void* ctx, const void* d_send, void* d_recv, size_t bytes, int rank,
                                  int world, void* stream);
typedef int (*expann_alltoallv_fn)(void* ctx, const void* d_send, const size_t* send_off,
                                   const size_t* send_bytes, void* d_recv, const size_t* recv_off,
                                   const size_t* recv_bytes, int rank, int world, void* stream);
int expann_sharded_set_exchange_fn(expann_sharded* h, expann_exchange_fn fn, void* ctx);
int expann_sharded_set_alltoallv_fn(expann_sharded* h, expann_alltoallv_fn fn, void* ctx);
/* in-process form, host buffers: as expann_search. */
int expann_sharded_search(expann_sharded* h, const void* queries, size_t m, size_t k, uint64_t* ids,
                          float* dists);
/* in-process form, everything resident: d_queries[r] = the m queries in the memory of shard r's
 * device; shard r merges the query slice expann_sharded_slice(h, m, r, &lo, &hi) and leaves it in
 * d_ids[r][(hi-lo)][k] / d_dists[r] on its device (ordered on the shard's own stream).  With
 * "async_search" = 1 (default) the call returns once everything is enqueued on every device;
 * expann_sharded_sync waits for all shards and validates the searches since the last sync
 * (EXPANN_ERR_OVERFLOW: repeat them with "async_search" = 0). */
int expann_sharded_search_devices(expann_sharded* h, const void* const* d_queries, size_t m, size_t k,
                                  uint64_t* const* d_ids, float* const* d_dists);
/* query slice [*q_lo, *q_hi) that shard (rank) `shard` merges under pattern 2 and in
 * expann_sharded_search_devices: [min(m, shard * ceil(m/G)), min(m, (shard+1) * ceil(m/G))) */
int expann_sharded_slice(const expann_sharded* h, size_t m, int shard, size_t* q_lo, size_t* q_hi);
/* rank form, device buffers on `stream` (NULL = the handle's own): local search, exchange, merge;
 * every rank ends with the full ids[m][k] / dists[m][k].  Collective.  With the option
 * "async_search" = 1 the call returns without a host wait (expann_sharded_sync, as expann_sync). */
int expann_sharded_search_device(expann_sharded* h, const void* d_queries, size_t m, size_t k,
                                 uint64_t* d_ids, float* d_dists, void* stream);
int expann_sharded_sync(expann_sharded* h);
/* "exchange" (in-process form, transport: 0 auto, 1 RCCL, 2 device copies), "exchange_pattern" (0 auto
 * = 2, 1 all-gather of whole chunks, 2 all-to-all of query slices), "threads" (in-process form: 1
 * (default) = one enqueue thread per shard, 0 = the calling thread enqueues every device in turn),
 * "async_search" (in-process form: 1 (default) = the shards' searches are enqueued on all devices
 * before the host waits for any); every other option goes to the shards' indexes (expann_set_option). */
int expann_sharded_set_option(expann_sharded* h, const char* name, long value);

/* batched candidate scoring (quantized_scorer::filter_by_score, src/quantizer.h:20-59):
 * for each of n_ids row ids (order kept) score against ONE query; keep (id, score) with
 * score < cutoff.  Host buffers; *n_kept receives the count. */
int expann_score_ids(expann_index* h, const void* query, const uint64_t* ids, size_t n_ids,
                     float cutoff, uint64_t* kept_ids, float* kept_scores, size_t* n_kept);

/* graph search (antitopo_engine, query side) --------------------------------------------- */
typedef struct expann_graph expann_graph;
/* Upload a built graph (replaces the tail of antitopo_engine::_build, src/antitopo_engine.h:
 * 467-493, after deserialize :994-1074): `vectors` [n][dim] fp32 (all_entries), CSR adjacency
 * per layer as flattened by include/expann/antitopo_index.h (hadj_flat): layer_offsets is
 * [n_layers][n+1] into `neighbours`; layer 0 is hadj_bottom.  Host arrays, copied.
 * dim: any multiple of 16 up to 4096 (64, 128, 256, 512, 768, 832, 960 compiled, the others
 * run-time-dim kernels); not a multiple of 16 -> EXPANN_ERR_INVALID_ARG, over 4096 ->
 * EXPANN_ERR_UNSUPPORTED, both before any device lookup. */
int expann_graph_create(int dim, int device, const float* vectors, size_t n, uint32_t n_layers,
                        uint32_t starting_vertex, const uint64_t* layer_offsets,
                        const uint32_t* neighbours, expann_graph** out);
void expann_graph_destroy(expann_graph* g);
const char* expann_graph_last_error(const expann_graph* g);
/* antitopo_engine::_query_k for a batch (src/antitopo_engine.h:853-928): greedy descent, then
 * the bottom-layer best-first search with queue size ef_search (:495-708), or with
 * use_compression != 0 over uint8 rows + final fp32 re-score (:710-851).  Host buffers:
 * ids[m][k] / dists[m][k] padded with UINT64_MAX / +inf; distcomps[m] (RECORD_STATS'
 * num_distcomps per query, :125-129) may be NULL.  use_compression != 0 needs dim % 64 == 0
 * (EXPANN_ERR_UNSUPPORTED otherwise, checked before the device is touched). */
int expann_graph_search(expann_graph* g, const float* queries, size_t m, size_t k,
                        size_t ef_search, int use_compression, uint64_t* ids, float* dists,
                        uint32_t* distcomps);
/* device time of the last search's traversal kernel, milliseconds: its first launch plus its redo launch when
 * there was one (below), after a host-buffer call as after an expann_graph_sync */
double expann_graph_last_kernel_ms(const expann_graph* g);

/* how the bottom layer of the walk scores a row */
enum expann_graph_compression {
	EXPANN_GRAPH_FP32 = 0,     /* fp32 rows (:495-708)                                                    */
	EXPANN_GRAPH_U8_CAST = 1,  /* quantizer_simple<uint8_t> bytes, a plain cast: rows that already hold
	                            * integers in [0, 255] (:710-851) -- what use_compression means            */
	EXPANN_GRAPH_RANGED_Q8 = 2 /* quantizer_ranged_q8 bytes (src/quantizer.h:152-238, which the reference
	                            * never instantiates): one global scale_factor / offset from the rows' min
	                            * and max, bytes in [0, 127] -- any fp32 rows                             */
};
/* expann_graph_search with the bottom-layer scoring as a mode (expann_graph_search(..., use_compression, ...)
 * is this call with use_compression ? 1 : 0).  Mode 2 is the uint8 walk in every respect -- fp32 entry
 * evaluation and descent, exact integer sum (q8_i - r8_i)^2 on the bottom layer, same queues, stop rule and
 * distcomps, results in the order of the integer distances, re-scored in fp32 on the original rows -- over an
 * int8 copy of the rows made at the first use (n * dim bytes of device memory, next to the uint8 copy), with
 * the queries converted by the same scale_factor / offset inside the walk kernel (components outside the
 * rows' range clamp).  Errors, all before the device is touched: mode outside 0..2 EXPANN_ERR_INVALID_ARG;
 * modes 1 and 2 need dim % 64 == 0 (EXPANN_ERR_UNSUPPORTED).  Mode 2 on rows whose scale_factor is not
 * finite and positive (all components equal): EXPANN_ERR_INVALID_ARG, nothing is walked.
 * A walk whose candidates heap overflows is walked again by the redo launch of expann_graph_search_device (below),
 * which this call enqueues only when there are such queries; EXPANN_ERR_OVERFLOW when one overflows there too or
 * there is no larger capacity to go to (the rows of those queries are what the last walk left).  A larger capacity
 * whose working set exceeds the LDS is never tried: the redo launch runs at the largest that fits. */
int expann_graph_search_mode(expann_graph* g, const float* queries, size_t m, size_t k, size_t ef_search,
                             int mode, uint64_t* ids, float* dists, uint32_t* distcomps);
/* scale_factor / offset of the handle's affine quantiser; builds the int8 copy if it does not exist yet
 * (errors as mode 2 of expann_graph_search_mode) */
int expann_graph_ranged_params(expann_graph* g, float* scale_factor, float* offset);

/* Graph search on device buffers (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed).
 * expann_graph_search_device is expann_graph_search_mode with the queries [m][dim], ids [m][k], dists [m][k] and
 * distcomps [m] (may be NULL) in device memory: same arguments, same checks in the same order, same error codes,
 * all before the device is touched; m == 0 is EXPANN_OK and enqueues nothing.  The call ENQUEUES on `stream` (a
 * hipStream_t; NULL = the handle's own) and returns without waiting for it: the resets of its counters, the walk
 * at the first heap capacity, and a REDO launch that walks only the queries whose
 * candidates heap overflowed again, at the largest power-of-two capacity up to 8192 whose working set fits the
 * LDS, and overwrites their rows (sized without knowing their number: with none, its workgroups leave after one
 * atomic).  A walk that does not overflow never looks at the capacity, so ids, distances and distcomps do not
 * depend on which launch served a query; the host-buffer call plans and launches the same way.  When the redo
 * capacity is not larger than the first launch's there is no redo launch and an overflow is final.  In steady state -- the same
 * kernel instance, a working set and an m no larger than seen before -- a call makes no allocation, no copy
 * between host and device, no attribute or occupancy query and no synchronisation.
 * expann_graph_sync waits for the stream of the last such search and reports on all of them since the previous
 * sync: EXPANN_OK, or EXPANN_ERR_OVERFLOW when a walk overflowed the redo capacity too (that search's rows of those
 * queries are what the last walk left, as the host-buffer call returns them).  After it
 * expann_graph_last_kernel_ms is the last search's first launch plus redo launch.
 * ONE set of visited arrays per handle, so the rule is expann_sync's: searches of a handle overlap only in stream
 * order; one enqueued on a different stream than the outstanding ones first waits for those on the host, and so do
 * expann_graph_search / expann_graph_search_mode; at most 256 searches may be outstanding (further ones wait by
 * themselves).  The first use of mode 1 or 2 on a handle builds its byte copy of the rows on the handle's own
 * stream and waits for it on the host, so the copy is complete before the walk starts on whichever stream. */
int expann_graph_search_device(expann_graph* g, const float* d_queries, size_t m, size_t k, size_t ef_search,
                               int mode, uint64_t* d_ids, float* d_dists, uint32_t* d_distcomps, void* stream);
int expann_graph_sync(expann_graph* g);
/* options of both entry points (0 = auto): "cand_capacity" = the first launch's heap, "redo_capacity" = the redo
 * launch's (at most 8192); a power of two >= 8, anything else -- and an unknown name -- is EXPANN_ERR_INVALID_ARG.
 * "filter_flat_rows" (a row count >= 0, no power-of-two rule): see expann_graph_set_row_filter. */
int expann_graph_set_option(expann_graph* g, const char* name, long value);
/* Device-buffer searches only (a host-buffer call changes none of them): "redo_queries" = queries the redo
 * launches served, over the searches the last expann_graph_sync checked;
 * "redo_overflows" = searches since create that ended in EXPANN_ERR_OVERFLOW; "deferred_searches" = device-buffer
 * searches since create; "distcomps" = distance evaluations of all device-buffer searches since create, as of the
 * last sync; "redo_kernel_ns" = device time of the last search's redo launch, as of the last sync;
 * "filter_active", "filter_rows", "flat_searches": see expann_graph_set_row_filter; "groups_active", "group_count",
 * "group_walk_queries", "group_scan_queries", "group_pad_queries": see expann_graph_set_row_groups; "vector_bytes": see
 * expann_graph_create_f16; "range_searches": see expann_graph_range_search.  An unknown name is
 * EXPANN_ERR_INVALID_ARG. */
int expann_graph_get_stat(expann_graph* g, const char* name, uint64_t* out);

/* GPU-assisted batched construction of the graph (csrc/graph_build.hpp; replaces the inner loop of
 * antitopo_engine::_store_vector / prune_edges, src/antitopo_engine.h:263-465, for the vectors
 * [n_built, n) -- the first n_built come with their rows already built, by the serial host builder
 * of include/expann/antitopo_index.h).  Vectors are inserted in BATCHES against the graph of the
 * vectors before them: ef_construction searches per layer, prune_edges' rule on the candidate lists,
 * reverse edges, and one more prune of every row that outgrew M / M0.  `levels[v]` = the level the
 * reference's draw gives vertex v (:323).  Adjacency arrays are host memory, fixed row strides:
 * layer 0 ids0 / d0 [n][stride0] + deg0[n]; layers 1.. idsu / du [(l-1) * U + upper_idx[v]][strideu] +
 * degu, upper_idx[v] = -1 for level-0 vertices.  On return rows hold at most M0 / M edges (id,
 * reference-order distance).  stats[4] (optional): batches, reverse edges dropped for want of slack,
 * rows re-pruned, 0.  ortho_count = 1 only (the reference's sweep, src/bench_runner.h:138).  dim: as
 * expann_graph_create (multiple of 16 up to 4096, checked before any device lookup).
 * THE BATCH RULE.  The first batch is [b0, b1) with b0 = n_built and b1 = min(n, b0 + min(max_batch, max(1,
 * b0 / 16))) (max_batch = 0: 32768): at most 1/16 of the graph so far.  It is cut short before the first vertex
 * whose level is >= max_layer; such a vertex, when it comes first, is a batch of its own.  After a batch,
 * max_layer and starting_vertex advance as in :459-462, once per layer a vertex of the batch opens (a level may
 * skip layers); the next batch starts at b1.  Within a batch: every search runs on the graph as it stood before
 * the batch (greedy descent from starting_vertex through the layers above the vertex's level -- per pass the
 * first occurrence of the row's minimum, taken only if strictly better -- then the ef_construction search of
 * every layer <= min(level, max_layer - 1), top down, each seeded with the nearest of the layer above; a row is
 * read up to min(degree, stride)); prune_edges on every candidate list in (distance, id) order, the score
 * res += ortho_factor * (basic - co) + ortho_bias with every operation rounded (no fused multiply-add), the
 * first of equal scores wins; the reverse edge (distance, new vertex) goes to every kept neighbour's row -- a
 * row takes `stride` entries, further ones are dropped and counted in stats[1]; every row whose length passed
 * M0 / M is sorted and pruned once.  Everything but the order of the appended entries in a row that was not
 * re-pruned is determined (tests/test_gpu_graph_build_exact.py compares it batch by batch, bit for bit, with a
 * CPU restatement of this paragraph). */
int expann_graph_build_batched(int dim, int device, const float* vectors, size_t n, const uint8_t* levels,
                               size_t n_built, uint32_t* max_layer_io, uint32_t* starting_vertex_io, size_t M,
                               size_t M0, size_t ef_construction, size_t prune_overflow, float ortho_factor,
                               float ortho_bias, size_t max_batch, uint32_t* ids0, float* d0, uint32_t* deg0,
                               size_t stride0, const int32_t* upper_idx, size_t U, size_t n_upper_layers,
                               uint32_t* idsu, float* du, uint32_t* degu, size_t strideu, uint64_t* stats);

/* the whole graph engine behind one handle (what src/pyrunner.cpp:56-90 binds: ctor,
 * store_vector / store_many_vectors, build, query_k, set_ef_search).  Construction runs on the
 * host (include/expann/antitopo_index.h), queries on the GPU (expann_graph_search). */
typedef struct expann_antitopo expann_antitopo;
/* antitopo_engine(M, ef_construction, ortho_count, prune_overflow, use_compression),
 * src/antitopo_engine.h:157-166: M0 = 2M, ortho_factor = 0.5, ortho_bias = 0, ef_search_mult = 1.
 * dim: any multiple of 16 up to 4096 (EXPANN_ERR_INVALID_ARG / EXPANN_ERR_UNSUPPORTED otherwise);
 * use_compression != 0 needs dim % 64 == 0 (EXPANN_ERR_INVALID_ARG); all checked before the device. */
int expann_antitopo_create(int dim, int device, size_t M, size_t ef_construction,
                           size_t ortho_count, size_t prune_overflow, int use_compression,
                           expann_antitopo** out);
void expann_antitopo_destroy(expann_antitopo* e);
const char* expann_antitopo_last_error(const expann_antitopo* e);
int expann_antitopo_store(expann_antitopo* e, const float* rows, size_t n);  /* _store_vector x n */
/* the same rows through the batched GPU builder (expann_graph_build_batched); the first
 * min(n_serial, n) of an empty engine are still inserted serially and seed the batches */
int expann_antitopo_store_batched(expann_antitopo* e, const float* rows, size_t n, size_t n_serial);
int expann_antitopo_build(expann_antitopo* e);                               /* _build (:467-493) */
int expann_antitopo_set_ef_search(expann_antitopo* e, size_t ef_search);     /* :189-195 */
/* query_k for a batch; ef_search defaults to k * ef_search_mult and is sticky (:858-859) */
int expann_antitopo_query(expann_antitopo* e, const float* queries, size_t m, size_t k,
                          uint64_t* ids, float* dists);
/* (appended with expann_graph_search_device) expann_antitopo_query on device buffers: the same sticky ef_search
 * and the same mode, enqueued on `stream` (NULL = the graph handle's) without waiting; expann_antitopo_sync is
 * expann_graph_sync and adds the distance evaluations the device counted to num_distcomps.  Before build() both
 * return EXPANN_ERR_NOT_BUILT. */
int expann_antitopo_query_device(expann_antitopo* e, const float* d_queries, size_t m, size_t k,
                                 uint64_t* d_ids, float* d_dists, void* stream);
int expann_antitopo_sync(expann_antitopo* e);
int expann_antitopo_save(expann_antitopo* e, const char* index_path);  /* serialize, :932-991 */
int expann_antitopo_load(expann_antitopo* e, const char* index_path);  /* deserialize + upload */
/* mode (expann_graph_compression) of expann_antitopo_query's bottom layer; default: what use_compression at
 * create says (0 or 1).  A run-time property: the index file does not record it.  A mode outside 0..2, or
 * mode 1 / 2 on an engine whose dim is not a multiple of 64: EXPANN_ERR_INVALID_ARG (no device call). */
int expann_antitopo_set_compression(expann_antitopo* e, int mode);
size_t expann_antitopo_size(const expann_antitopo* e);
uint64_t expann_antitopo_num_distcomps(const expann_antitopo* e);

/* test hook: replays a trace of priority-queue operations through the device's wave-cooperative heap code
 * (csrc/graph_search.hpp coop_push / coop_pop, the walk's queues) on device 0.  Trace format of
 * tests/golden/heap_ref.json: ops[i] 1 = push (op_d[i], op_id[i]), 0 = pop; entry 0 of the
 * out_* arrays is the state after the range constructor, entry i + 1 the state after op i; returns the
 * drain length, (size_t)-1 on failure.  tests/test_heap_pin.py checks it against the traces the image's
 * real std::priority_queue answered (tests/golden/heap_ref.json). */
size_t expann_device_heap_trace(int max_heap, size_t n_init, const float* init_d, const uint64_t* init_id,
                                size_t n_ops, const int* ops, const float* op_d, const uint64_t* op_id,
                                uint64_t* out_size, float* out_top_d, uint64_t* out_top_id, float* drain_d,
                                uint64_t* drain_id);

/* quantiser builds on device buffers (src/quantizer.h) -------------------------------- */
/* quantizer_simple<uint8_t>::build (src/quantizer.h:132-141): out[i] = uint8_t(in[i]), no
 * scaling; defined for 0 <= in[i] < 256.  Asynchronous on `stream`. */
int expann_quantize_simple_u8_device(int device, const float* d_rows, size_t n_values,
                                     uint8_t* d_out, void* stream);
/* quantizer_ranged_q8::build (src/quantizer.h:213-232, :196-200): global affine int8 in
 * [0,127]; d_scale_offset[0..1] receive scale_factor and offset.  Synchronises `stream`. */
int expann_quantize_ranged_q8_device(int device, const float* d_rows, size_t n_values,
                                     int8_t* d_out, float* d_scale_offset, void* stream);

/* profiling ------------------------------------------------------------------------- */
typedef struct expann_profile {
	uint64_t scan_launches;   /* launches of the full-base scan kernel since reset      */
	double scan_ms;           /* their summed device time (HIP events on their stream)  */
	uint64_t scan_rows;       /* rows streamed by those launches (per launch: n)        */
	uint64_t scan_query_tiles;/* query tiles (passes over the base) by those launches   */
	uint32_t query_tile;      /* Q_t: queries per pass of the last launch               */
	uint32_t levels;          /* threshold levels of the last search                    */
	uint64_t candidates;      /* candidates kept by the last full scan (all queries)    */
	uint64_t retries;         /* overflow retries since reset                           */
	char scan_kernel[64];     /* name of the full-scan kernel last launched             */
	uint64_t deferred_searches; /* searches since reset whose flag check was deferred to
	                             * expann_sync ("async_search"); the others waited on the host */
} expann_profile;
/* enable != 0 brackets every full-scan launch with HIP events. */
int expann_set_profiling(expann_index* h, int enable);
/* synchronises the recorded events, fills *out and resets the accumulators. */
int expann_get_profile(expann_index* h, expann_profile* out);
/* the same for every shard / for one shard of a sharded handle */
int expann_sharded_set_profiling(expann_sharded* h, int enable);
int expann_sharded_get_profile(expann_sharded* h, int shard, expann_profile* out);

/* integer options (expann_amd/csrc/bf_options.hpp is the one list of them: names, defaults, environment variables
 * and the rule each value passes through): "query_tile" (0 = auto), "cand_capacity" (0 = auto),
 * "scan_kernel" (0 = auto, 1 = direct VALU scan, 2 = GEMM form on the fp32 / int8 matrix
 * cores, 3 = GEMM form on the bf16 matrix cores with the 3-term split, 4 = GEMM form with one
 * scaled fp16 product, 5 = 8-bit rows: int8 MFMA form with per-wave hit queues (d = 128,
 * 256, 768, 832, 896, 960 compiled; every other multiple of 64 up to 4096 with the dim known at
 * run time); the final ids and distances are identical for every choice),
 * "sample_ratio" (rows ratio between the levels of the threshold ladder, default 32),
 * "sample_pass" (fp16 form: 1 = one sampled pass gives the threshold (default), 0 = ladder),
 * "sample_frac" (the sampled pass reads 1/frac of the rows; 0 = chosen from k (default)),
 * "u8_exact" (1 (default): an fp32 L2 index of dim 128 / 256 whose values are all integers in
 * [0, 255] keeps a uint8 copy, and batches of 8-bit integer queries are searched through the
 * exact 8-bit kernels -- same ids and fp32 distances; 0: never),
 * "latency_mode" (1 (default): expann_search with few queries (m*k <= 16384) stages them in
 * pinned memory and lets the select kernels store the results there -- one host sync per
 * search and no pageable copies; 0: always the plain copy path),
 * "async_search" (1: expann_search_device returns without the final host wait, see expann_sync),
 * "xcd_tolerance" (percent of modelled launch cost given up for an XCD-aligned row-chunk count,
 * default 3), "scan_chunks" (experiments: force the row-chunk count of the fp16 scan; 0 = model),
 * "sample_run", "debug" (bench / ablation switches),
 * "persist" (1 (default): the d = 128 fp16 scan runs as resident workgroups pulling work per XCD; 0: plain launch;
 * EXPANN_PERSIST sets the starting value),
 * "tail_chunks" (1 (default): that scan cuts the row chunks of its last round three times finer; 0: one size;
 * EXPANN_TAIL_CHUNKS sets the starting value),
 * "group_list_rows" (row groups: the longest group the list kernel serves, see expann_set_row_groups),
 * "f16x", "i8x", "i8w" (A/B switches whose 0 side was removed: 0 is EXPANN_ERR_UNSUPPORTED, any other value is
 * accepted and changes nothing),
 * "ip_rescale" (1 (default): inner product, fp16 form: the filter sees each query times a power of two that brings
 * its norm to the largest row's -- ranks unchanged, results exact; 0: rounds 1-2's unscaled filter),
 * "i8_filter" (fp32 L2, d = 128, scan_kernel on auto: the full scan on the int8 matrix cores with a rigorous
 * slack and the exact re-rank, thresholds from the fp16 sampled pass; 1 (default): from the planner's crossover
 * on, 2: wherever supported, 0: never; the environment variable EXPANN_I8_FILTER sets the starting value),
 * "i8_sample" (int8 filter with speculative thresholds: the sampled pass runs on the int8 matrix cores too, over the
 * index's int8 copy with a centre row term of 4 bytes per row kept beside it -- the speculative threshold is then an
 * estimate from the int8 products, which the select's check covers as it covers any other, and the proven threshold
 * of the redo pass comes from the same pass; ids and distances do not change.  1 (default): where the int8 filter
 * speculates at its auto rank ("spec_rank" 0) and no row filter is set; 2: wherever it speculates, forced ranks
 * included; 0: never -- the fp16 sampled pass, as every proven-threshold, fp16-form, filtered or repeated search
 * takes.  EXPANN_I8_SAMPLE sets the starting value),
 * "spec_rank" (fp32 rows, d = 64 / 128, batches of more than 64 queries: the full scan filters with a SPECULATIVE
 * threshold, the j-th largest class maximum of the sampled pass instead of the k-th; the select checks every
 * query's result against it and the few failing queries are searched again on the device with the proven
 * threshold -- ids and distances do not change.  0 (default): j from k, the sampled share of the rows and a share
 * of failing queries of at most 1 %, where the planner found a gain; j >= 1: that rank wherever the check exists;
 * j >= k: off.  The environment variable EXPANN_SPEC_RANK sets the starting value),
 * and two debug switches of a speculating search's tail, for tests and A/B runs (results are the same either way;
 * EXPANN_REDO_BOUND / EXPANN_SELECT_OVERLAP set the starting values): "redo_bound" (1, default: the redo pass filters
 * with the smaller of the proven threshold and the k-th exact score of the failed list; 0: the proven threshold
 * alone) and "select_overlap" (1, default: the select stages of lists beyond 512 keys run on an internal side
 * stream beside the short lists' stage, joined before anything that follows; 0: one stream),
 * "rerank_rounds" (int8 filter: how the select re-ranks a candidate list exactly.  2 (default): the rows of the 16
 * (k rounded up to 16) smallest filter keys first, then only the rows whose proven lower bound does not exceed the
 * k-th exact score of that first round; 1: every row the filter's interval bounds cannot rule out, in one round.
 * Ids and distances are the same either way; EXPANN_RERANK_ROUNDS sets the starting value),
 * "rerank_stats" (0 (default); 1: the selects count the rows they re-score exactly, read as the statistic
 * "rerank_rows" -- adds a counter store per query, two small launches and a host wait to every search, deferred
 * ones included: for tests and measurements, not for timed runs). */
int expann_set_option(expann_index* h, const char* name, long value);

/* counters outside expann_profile (whose layout is fixed): "redo_queries" = queries of the last search that the
 * redo pass of the speculative thresholds served (deferred searches: of the searches the last expann_sync
 * checked), "redo_candidates" = the keys the redo lists of those queries held, "redo_overflows" = searches since the handle was made whose failing queries did not fit the redo
 * pass (repeated with proven thresholds: a retry), "spec_rank" = the rank j of the last search's thresholds
 * (= k: proven thresholds), "i8_sample" = 1 when the last search's sampled pass ran on the int8 matrix cores (option
 * "i8_sample"; 0 after a search whose last attempt took the fp16 pass or none), "rerank_rows" = rows of the index the last search's selects (the redo pass's included)
 * re-scored exactly, counted only under the option "rerank_stats" (else 0), "base_bytes" = bytes of device memory that hold the rows themselves (n * dim * bytes
 * per element, every dtype; 0 before the rows are on the device). */
int expann_get_stat(expann_index* h, const char* name, uint64_t* out);
/* the auto rank for k neighbours when the sampled pass reads 1/sample_frac of the rows: the smallest j with
 * P(Bin(k - 1, 1/sample_frac) >= j) <= 1 %; k = no speculation.  Host arithmetic only. */
uint32_t expann_spec_rank_auto(size_t k, uint32_t sample_frac);

/* Row filter of the brute-force index (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed).
 * Bit r & 31 of word r >> 5 (least significant bit first) says whether LOCAL row r -- the row number before
 * id_offset -- is allowed; bits at and beyond expann_size(h) are ignored.  The library copies the bits, the
 * caller may free them on return; its own copy covers the padded row count of the fp16 copy, is zero from row n
 * on, and no kernel reads a bit word outside it.
 * While a filter is set, expann_search, expann_search_device (also under "async_search") and the latency mode
 * return the min(k, allowed) smallest (score, id) among the allowed rows, ascending, padded with UINT64_MAX /
 * +inf: exactly what an index holding only the allowed rows, in the same order, would return, with its ids
 * mapped back.  Ids and distance bits are those of the reference's arithmetic, as everywhere else.
 * expann_score_ids takes explicit ids and is not affected.
 * Both set calls and the clear call first wait on the host for outstanding deferred searches (the rule of a
 * search on another stream), so every search runs under the filter that was in force when it was enqueued.
 * expann_set_row_filter_device reads d_allow_bits in the order of `stream` (a hipStream_t; NULL = the handle's
 * own) and returns after that stream and the handle's own have drained: the allowed-row count is needed on the
 * host for planning -- one host wait per filter change, none per search.  expann_build and
 * expann_set_base_device clear the filter.
 * Errors, in this order: h == NULL or bits == NULL EXPANN_ERR_INVALID_ARG; a dtype other than EXPANN_DTYPE_F32 /
 * EXPANN_DTYPE_F16 EXPANN_ERR_UNSUPPORTED (8-bit and int16 rows have integer row terms without a NaN: not offered) -- both before
 * the device is touched --; no rows on the device yet EXPANN_ERR_NOT_BUILT; n_words < ceil(n / 32)
 * EXPANN_ERR_INVALID_ARG.  A failed call leaves the filter as it was.
 * A filtered search never takes the uint8 shadow index ("u8_exact"), the int8 filter ("i8_filter") or
 * speculative thresholds ("spec_rank"), whatever those options say, and never the bf16x3 form ("scan_kernel" 3
 * runs the exact direct scan, as do queries outside the fp16 range).
 * expann_sharded_* does not offer the filter (its set_option pass-through is unchanged and there is no
 * sharded entry point for it).  Per query: row groups, expann_set_row_groups at the end of this header.  The graph
 * engine has a row filter of its own: expann_graph_set_row_filter, below, and a per-query form of it:
 * expann_graph_set_row_groups.
 * expann_get_stat: "filter_active" (0 / 1), "filter_rows" (allowed rows; n when no filter is set). */
int expann_set_row_filter(expann_index* h, const uint32_t* allow_bits, size_t n_words);        /* host bits   */
int expann_set_row_filter_device(expann_index* h, const uint32_t* d_allow_bits, size_t n_words, void* stream);
int expann_clear_row_filter(expann_index* h);

/* Row filter of the graph engine (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed; with no
 * filter set every launch uses the kernel instances it used before).
 * THE FILTER RULE.  A filter is a bitmap over vertex numbers: bit v & 31 of word v >> 5, least significant bit
 * first, says whether vertex v may appear in a result.  Bits at and beyond n are ignored; the library keeps its own
 * copy, which is zero from n on (the caller may free its bits on return).  Under a filter the walk runs as follows.
 *   Descent: the entry evaluation and the greedy descent through the upper layers are unchanged; they never look
 *   at the filter.
 *   Bottom-layer entry: the entry vertex is scored and marked visited; it is pushed on `candidates`; it is pushed
 *   on `nearest` only if it is allowed.
 *   Stop rule: stop when `candidates` is empty; also stop when nearest.size() == ef && cur.d > nearest.top().d.
 *   While `nearest` holds fewer than ef entries -- none included -- nothing stops the walk but an empty
 *   `candidates`.
 *   Neighbour update: for each unvisited neighbour in adjacency order, with distance dn: if nearest.size() < ef ||
 *   dn < nearest.top().d, push it on `candidates`; if it is also allowed, push it on `nearest` and pop `nearest`
 *   when it exceeds ef.  A disallowed vertex is traversed but never kept.
 *   The pre-drop of a neighbour (a full `nearest` and !(dn < its top at the start of the hop)) stays valid: the
 *   top only falls while the queue is full.  distcomps count every scored vertex, allowed or not.
 *   Output as without a filter: drain `nearest`, reverse, re-score in fp32 in modes 1 and 2, truncate to k, pad
 *   with UINT64_MAX / +inf.
 * With every bit set this is the unfiltered walk exactly: ids, distance bits and distcomps equal it in all three
 * modes.  The redo launch, the counters and EXPANN_ERR_OVERFLOW work as without a filter.
 * SPARSE FILTERS ARE SCANNED.  A walk under a filter that allows few rows visits most of the graph with `nearest`
 * never full, and `candidates` grows with the frontier.  So when the filter allows at most "filter_flat_rows" rows
 * (expann_graph_set_option: v >= 0, anything else EXPANN_ERR_INVALID_ARG; 0 = auto: 128 000, measured on
 * a 1 M x d128 graph at ef_search = 60, k = 10 (profiles/graph_filter_ab.txt); v > 0: filters allowing
 * at most v rows are scanned, so 1 is in effect "always walk") a search does not walk: it scores exactly the
 * allowed rows in fp32, in the reference's FMA order, whatever the mode, and returns the min(k, allowed) smallest by
 * (distance, id), ascending, padded -- what the brute-force index returns over those rows -- with distcomps per
 * query = the allowed count.  (A search with min(k, allowed) > 1024 walks whatever the option says: the scan keeps
 * its k best in LDS.)  A filter that allows no row returns padding and distcomps 0, with no walk and no scan.
 * expann_graph_search, _mode, _device and the expann_antitopo_query calls all honour the filter, the device-buffer
 * call in stream order and with its steady-state promise (no allocation, copy, query or synchronisation).
 * Both set calls and the clear call first wait on the host for outstanding device-buffer searches (their counters
 * stay for the next expann_graph_sync), so every search runs under the filter that was in force when it was
 * enqueued.  expann_graph_set_row_filter_device reads d_allow_bits in the order of `stream` (a hipStream_t; NULL =
 * the handle's own) and returns after that stream and the handle's own have drained: the allowed count is needed on
 * the host to choose between walk and scan -- one host wait per filter change, none per search.
 * Errors, in this order, both before the device is touched: handle or bits NULL EXPANN_ERR_INVALID_ARG; n_words <
 * ceil(n / 32) EXPANN_ERR_INVALID_ARG.  A failed call leaves the filter as it was.
 * expann_graph_get_stat: "filter_active" (0 / 1), "filter_rows" (allowed rows; n when no filter is set),
 * "flat_searches" (searches since create, of either entry point, that were answered without a walk: by the scan, or
 * by padding alone under a filter that allows no row).
 * expann_antitopo_set_row_filter is the same on the engine's graph (NULL bits clear the filter); before build()
 * EXPANN_ERR_NOT_BUILT.  expann_antitopo_store*, _build and _load clear the filter: it is a run-time property and is
 * not written to the index file.  expann_antitopo_set_row_filter_device takes device bits as
 * expann_graph_set_row_filter_device does.
 * Not offered: a filter for expann_graph_build_batched's searches.  (Per query: row groups; deleting the rows a
 * filter disallows: expann_antitopo_compact_row_filter, both at the end of this header.) */
int expann_graph_set_row_filter(expann_graph* g, const uint32_t* allow_bits, size_t n_words);
int expann_graph_set_row_filter_device(expann_graph* g, const uint32_t* d_allow_bits, size_t n_words, void* stream);
int expann_graph_clear_row_filter(expann_graph* g);
int expann_antitopo_set_row_filter(expann_antitopo* e, const uint32_t* allow_bits_or_NULL, size_t n_words);
int expann_antitopo_set_row_filter_device(expann_antitopo* e, const uint32_t* d_allow_bits, size_t n_words, void* stream);

/* Graph engine over IEEE binary16 rows (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed; a handle
 * made by expann_graph_create launches exactly the kernel instances it launched before).
 * THE F16 ROW RULE.  A graph handle whose rows are binary16 returns what the handle made by expann_graph_create from
 * (float)row returns, from every entry point and in every mode, bit for bit: ids, fp32 distance bits, distcomps,
 * padding, the redo launch's behaviour and the EXPANN_ERR_OVERFLOW cases -- expann_graph_search, _search_mode (modes
 * 0, 1, 2), _search_device + _sync, the row filter (walk and scan) and expann_graph_ranged_params.  binary16 -> fp32
 * is exact, subnormals included: nothing is flushed.  The byte copies of modes 1 and 2 are made from the halves
 * converted on load, so bytes, scale_factor and offset are the fp32 handle's bits.  Queries stay fp32.
 * expann_graph_create_f16 is expann_graph_create with rows [n][dim] of 2 bytes each (host memory): the same checks
 * in the same order, all before the device is touched; the rows stay binary16 on the device (half the bytes a hop
 * gathers, half the device copy).  expann_graph_get_stat "vector_bytes" = the device bytes of the rows themselves,
 * n * dim * 2 or n * dim * 4.
 * expann_antitopo_set_rows_f16(e, on): allowed only while the engine holds no rows, else EXPANN_ERR_INVALID_ARG (a
 * NULL handle too; no device call is made).  With it on, expann_antitopo_store / _store_batched round every incoming
 * float to the nearest-even binary16 (expann::f32_to_f16_bits, include/expann/half.h) and keep (float) of that on
 * the host, so the serial builder, the batched builder and the index file see exactly the values the device will
 * hold; a call whose rows hold a NaN, or a value that rounds to +-inf, is refused with EXPANN_ERR_INVALID_ARG before
 * any of its rows is inserted.  _build / _load upload through expann_graph_create_f16.  _save writes the usual
 * file (fp32 values, the reference's layout).  _load into such an engine fails with EXPANN_ERR_INVALID_ARG, and
 * uploads nothing, when any stored value is not exactly a binary16 value: no rounding is ever silent after the
 * edges were chosen.
 * Not offered: binary16 device rows for expann_graph_build_batched (it receives the upcast fp32 rows), fp16
 * queries, bf16 rows. */
int expann_graph_create_f16(int dim, int device, const void* rows_f16, size_t n, uint32_t n_layers,
                            uint32_t starting_vertex, const uint64_t* layer_offsets, const uint32_t* neighbours,
                            expann_graph** out);
int expann_antitopo_set_rows_f16(expann_antitopo* e, int on);

/* Row groups of the graph engine: every query of a batch names the rows it may return (appended; EXPANN_ABI_VERSION
 * stays 2: nothing that existed changed).
 * THE GROUP RULE.  groups[v] is the group of vertex v and may be any uint32.  Query i of a grouped search may return
 * exactly the vertices with groups[v] == query_groups[i].  A query that names EXPANN_GROUP_ANY may return every
 * vertex: for it the search is the unfiltered search bit for bit -- ids, distance bits and distcomps, in all three
 * modes.  A row labelled 0xFFFFFFFF therefore belongs to no group: only ANY queries return it.
 * Let s_i be the number of rows in query i's group and F the option "filter_flat_rows" (0 = auto = 128 000: the row
 * filter's option, with the same meaning).  Each query is served on its own:
 *   s_i == 0 (a group that no row carries): padding with UINT64_MAX / +inf, distcomps 0.
 *   s_i <= F and min(k, s_i) <= 1024 (scan): the exact fp32 scan of the group's rows -- what SPARSE FILTERS ARE
 *   SCANNED above returns for a bitmap of the same rows, in every mode: the min(k, s_i) smallest by (distance, id),
 *   ascending and padded, distcomps = s_i.
 *   otherwise (walk): THE FILTER RULE's walk with "allowed" meaning groups[v] == query_groups[i].  Descent, stop rule,
 *   neighbour update, pre-drop, distcomps and output are word for word the same; the redo launch and
 *   EXPANN_ERR_OVERFLOW behave as under a bitmap.
 * So for a fixed group X the grouped answer is what expann_graph_set_row_filter(bits of groups == X) plus the plain
 * search give at the same "filter_flat_rows", bit for bit, distcomps included.
 * The plain searches (expann_graph_search, _mode, _device, expann_antitopo_query*) ignore the groups entirely and
 * launch the kernel instances they launch without them.
 * Set calls.  They first wait on the host for outstanding device-buffer searches (their counters stay for the next
 * expann_graph_sync), so every search runs under the groups that were in force when it was enqueued.  The library
 * keeps its own copy -- the labels, and a directory of the distinct labels with each group's rows, made on the host --
 * so the caller may free its array on return.  expann_graph_set_row_groups_device reads d_groups in the order of
 * `stream` (a hipStream_t; NULL = the handle's own) and returns after that stream and the handle's own have drained.
 * Errors, before the device is touched: handle or array NULL EXPANN_ERR_INVALID_ARG; n != the handle's row count
 * EXPANN_ERR_INVALID_ARG.  A failed call leaves the groups as they were.  expann_graph_clear_row_groups drops them.
 * Grouped searches.  The checks are expann_graph_search_mode's, in its order (m == 0 is EXPANN_OK); then query_groups
 * NULL EXPANN_ERR_INVALID_ARG; then no groups set EXPANN_ERR_NOT_BUILT; then a row filter in force
 * EXPANN_ERR_UNSUPPORTED -- all before the device is touched.  expann_graph_search_grouped_device keeps
 * expann_graph_search_device's promises: it enqueues on `stream` -- the counter reset, the scan of the scan-served
 * queries, the walk of the others and its redo launch -- and returns without waiting; in steady state it makes no
 * allocation, host/device copy, attribute query or synchronisation; expann_graph_sync reports.
 * expann_graph_search_grouped (host buffers) enqueues the same launches and waits.  expann_graph_last_kernel_ms is
 * the sum of the grouped search's launches.
 * expann_graph_get_stat: "groups_active" (0 / 1); "group_count" (distinct labels other than 0xFFFFFFFF);
 * "group_walk_queries", "group_scan_queries", "group_pad_queries" (queries of grouped searches since create, by how
 * they were served; counted on the device and folded in when a search is checked: on return of the host-buffer call,
 * or at expann_graph_sync).
 * expann_antitopo_set_row_groups is the same on the engine's graph (a NULL array clears the groups; before build()
 * EXPANN_ERR_NOT_BUILT; _set_row_groups_device takes device labels as expann_graph_set_row_groups_device does);
 * expann_antitopo_query_grouped / _device search with the engine's ef_search and compression.
 * expann_antitopo_store*, _build and _load clear the groups: they are a run-time property and are not written to
 * the index file.
 * Not offered: a grouped search while a row filter is in force (bitmap x groups), several groups per row or a set
 * of groups per query, groups for expann_graph_build_batched's searches, groups on the sharded handles.  (The
 * brute-force index has row groups of its own: expann_set_row_groups, at the end of this header.) */
#define EXPANN_GROUP_ANY 0xFFFFFFFFu
int expann_graph_set_row_groups(expann_graph* g, const uint32_t* groups, size_t n);            /* host [n] */
int expann_graph_set_row_groups_device(expann_graph* g, const uint32_t* d_groups, size_t n, void* stream);
int expann_graph_clear_row_groups(expann_graph* g);
int expann_graph_search_grouped(expann_graph* g, const float* queries, const uint32_t* query_groups, size_t m,
                                size_t k, size_t ef_search, int mode, uint64_t* ids, float* dists, uint32_t* distcomps);
int expann_graph_search_grouped_device(expann_graph* g, const float* d_queries, const uint32_t* d_query_groups,
                                       size_t m, size_t k, size_t ef_search, int mode, uint64_t* d_ids,
                                       float* d_dists, uint32_t* d_distcomps, void* stream);
int expann_antitopo_set_row_groups(expann_antitopo* e, const uint32_t* groups_or_NULL, size_t n);
int expann_antitopo_set_row_groups_device(expann_antitopo* e, const uint32_t* d_groups, size_t n, void* stream);
int expann_antitopo_query_grouped(expann_antitopo* e, const float* queries, const uint32_t* query_groups,
                                  size_t m, size_t k, uint64_t* ids, float* dists);
int expann_antitopo_query_grouped_device(expann_antitopo* e, const float* d_queries, const uint32_t* d_query_groups,
                                         size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream);

/* Row groups of the brute-force index: every query of a batch names the rows it may return (appended;
 * EXPANN_ABI_VERSION stays 2: nothing that existed changed).
 * THE GROUP RULE.  groups[r] is the group of LOCAL row r -- the row number before id_offset -- and may be any
 * uint32.  Query i of a grouped search may return exactly the rows with groups[r] == query_groups[i].  For a fixed
 * label X the answer is, bit for bit (ids with id_offset applied, fp32 distance bits, ties by lower id, padding with
 * UINT64_MAX / +inf), what expann_set_row_filter(bits of groups == X) followed by expann_search returns on the same
 * handle: what an index of only those rows returns, with its ids mapped back.  A query that names EXPANN_GROUP_ANY
 * gets the unfiltered search, bit for bit.  A row labelled 0xFFFFFFFF therefore belongs to no group: only ANY queries
 * return it.  The exact top-k by (score, id) in the reference's arithmetic is unique, so how a query is served never
 * shows in its answer.
 * query_groups IS HOST MEMORY in both search calls, on purpose: the queries of a batch are bucketed by group on the
 * host before anything is launched, a serving process knows its requests' tenants on the host, and a device array
 * would put a copy and a host wait in front of every search.  (The graph engine takes device labels because its
 * kernels serve each query on its own.)
 * How a batch is served.  Let s be the number of rows that carry a query's label and L the option "group_list_rows"
 * (expann_set_option: 0 = auto; v > 0: groups of at most v rows take the list kernel, so 1 is in effect "always a
 * filter pass"; v > 16384 -- the longest list the select sorts in LDS -- EXPANN_ERR_INVALID_ARG).  Auto = 16384,
 * measured on 1 M x d128 fp32 rows at k = 10 (profiles/bf_groups_ab.txt): with groups of 1 024 .. 16 384 rows tiling
 * the index, at 10 and at 100 queries per group, the list kernel was never the slower way (x 0.005 of the filter
 * passes' time at 1 024 rows and 10 queries per group, x 0.82 at 16 384 rows and 100).
 *   s == 0: padding only.
 *   ANY: the plain search over these queries (gathered into contiguous staging, scattered back; a batch that is
 *   all ANY runs in place), exactly the launches expann_search_device makes.
 *   s <= L (list): ONE launch of the list kernel (csrc/scan_groups.hpp) serves every such group of the batch -- a
 *   workgroup per (tile of queries that share a group, chunk of that group's rows), exact keys of every row of the
 *   group -- and one select launch writes the callers' rows.  No host wait.
 *   s > L (filter): at most n / L distinct labels are this large.  For each one present in the batch, in turn: the
 *   group's bitmap is made from the labels on the device and installed through the row filter's own path, the
 *   filtered search (all of its regimes and retries) serves the group's gathered queries, the rows are scattered
 *   back.  ONE HOST WAIT PER DISTINCT SUCH GROUP IN THE BATCH.  Afterwards the handle has no filter, also when a step
 *   failed.
 * A grouped search returns after its stream has drained: it ignores "async_search" and first waits for outstanding
 * deferred searches (as expann_search does).  The plain searches ignore the groups entirely and launch exactly what
 * they launch without them.
 * Set calls.  They first wait on the host for outstanding deferred searches.  The library keeps its own copy -- the
 * labels on the device, and a directory made on the host: the distinct labels ascending, their offsets, each group's
 * rows ascending -- so the caller may free its array on return.  Everything is built aside and swapped in when
 * complete: a failed call leaves the groups as they were.  expann_set_row_groups_device reads d_groups in the order
 * of `stream` (a hipStream_t; NULL = the handle's own) and returns after that stream and the handle's own have
 * drained.  expann_build and expann_set_base_device clear the groups, as they clear the filter;
 * expann_clear_row_groups drops them.
 * Errors of the set calls, in this order, the first three before the device is touched: handle or array NULL
 * EXPANN_ERR_INVALID_ARG; a dtype other than EXPANN_DTYPE_F32 / EXPANN_DTYPE_F16 EXPANN_ERR_UNSUPPORTED (the row
 * filter's rule, for its reason); n != expann_size(h) EXPANN_ERR_INVALID_ARG; no rows on the device yet
 * EXPANN_ERR_NOT_BUILT.
 * Grouped searches run expann_search's checks in its order (k in 1..8192; m == 0 is EXPANN_OK); then query_groups
 * NULL EXPANN_ERR_INVALID_ARG; then no groups set EXPANN_ERR_NOT_BUILT; then a row filter in force
 * EXPANN_ERR_UNSUPPORTED.
 * expann_get_stat: "groups_active" (0 / 1); "group_count" (distinct labels other than 0xFFFFFFFF); of the last
 * grouped search: "group_list_queries", "group_filter_queries", "group_any_queries", "group_pad_queries" (they add
 * up to m) and "group_filter_passes" (distinct filter groups it served).  "filter_active" reads 0 after a grouped
 * search.
 * Not offered: groups on the sharded handles, on 8-bit / int16 rows, groups together with the bitmap, several groups
 * per row or a set of groups per query, deferred grouped searches. */
int expann_set_row_groups(expann_index* h, const uint32_t* groups, size_t n);                 /* host [n] */
int expann_set_row_groups_device(expann_index* h, const uint32_t* d_groups, size_t n, void* stream);
int expann_clear_row_groups(expann_index* h);
int expann_search_grouped(expann_index* h, const void* queries, const uint32_t* query_groups, size_t m,
                          size_t k, uint64_t* ids, float* dists);                              /* host buffers */
int expann_search_grouped_device(expann_index* h, const void* d_queries, const uint32_t* query_groups /* HOST [m] */,
                                 size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream);

/* Range search of the brute-force index: every row within a per-query radius, exact (appended; EXPANN_ABI_VERSION
 * stays 2: nothing that existed changed).
 * THE RANGE RULE.  score is what expann_search reports: for EXPANN_METRIC_L2 the squared L2 in the reference's FMA
 * lane order, for EXPANN_METRIC_IP -dot (so "dot >= 0.8" is radii[i] = -0.8f).  Row b is in range of query i iff
 * score(q_i, b) <= radii[i] -- inclusive, the comparison every threshold of this engine makes.  A NaN radius is in
 * range of nothing.
 *   counts[i] is the exact number of rows in range, whatever it is, up to n: never an estimate, never saturated.
 *   ids[i][0 .. max_results) and dists[i][...] hold the min(counts[i], max_results) in-range rows with the smallest
 *   (score, id), ascending: ids with id_offset applied, the fp32 distance bits expann_search returns, ties by lower
 *   id, the tail padded with UINT64_MAX / +inf.  dists may be NULL.  counts[i] > max_results tells the caller that
 *   the row was truncated and that what it holds are the nearest rows.
 *   0 <= max_results <= 8192.  With max_results == 0 the call only counts, and ids / dists may be NULL.
 * Served: EXPANN_DTYPE_F32 and EXPANN_DTYPE_F16 rows (an F16 index returns bit for bit what the F32 index of the
 * upcast rows returns: THE RULE of that dtype), both metrics, every dim the index takes, expann_set_base_device rows
 * with their id_offset, m beyond one pass (32 768 queries).
 * Errors, in this order, all before the device is touched: handle NULL EXPANN_ERR_INVALID_ARG; queries, radii or
 * counts NULL, or ids NULL with max_results > 0, EXPANN_ERR_INVALID_ARG; max_results > 8192 EXPANN_ERR_UNSUPPORTED
 * (by value, as k is); a dtype other than F32 / F16 EXPANN_ERR_UNSUPPORTED; no rows on the device
 * EXPANN_ERR_NOT_BUILT; a row filter in force EXPANN_ERR_UNSUPPORTED.  Row groups that are merely set are ignored, as
 * the plain searches ignore them.  m == 0 is EXPANN_OK.  A failed call leaves the handle usable.
 * Both calls return after their stream has drained: they ignore "async_search" and first wait for outstanding
 * deferred searches (expann_search_grouped's rule).  The device call reads d_radii and writes its outputs in the
 * order of `stream` (a hipStream_t; NULL = the handle's own).
 * How a batch is served (csrc/select_range.hpp).  The engine's filters keep every row with
 * score <= tau for ANY tau, so the caller's radii are the thresholds: no sampled pass, no estimate.  Stage 1: every
 * query, candidate lists of "cand_capacity" keys (expann_set_option; unset: room for twice max_results, at least
 * 1 024) -- the fp16 single-product form where the plain search would use a matrix-core form and the queries fit the
 * index's fp16 range, every candidate re-scored exactly and cut at the radius; else the exact direct scan.  Stage 2:
 * the queries whose list did not fit, at 16 384 keys: the fp16 form again where stage 1 ran it with shorter lists,
 * then the exact direct scan, whose counter is the exact count.  Stage 3: queries with more than 16 384
 * rows in range -- their max_results nearest rows are all in range, so the plain pipeline at k = max_results writes
 * them.  One host wait per stage that runs.  Never the uint8 shadow, the int8 filter, speculative thresholds, the
 * bf16x3 form or the latency mode in stages 1 and 2, whatever the options say.
 * expann_get_stat, of the last range search: "range_list_queries" (answered from a candidate list, stages 1 and 2),
 * "range_topk_queries" (more than 16 384 rows in range; the two add up to m), "range_retries" (queries that stage
 * 1's lists could not hold).  expann_get_profile's scan_kernel names the scan of stage 1.
 * Not offered: range search under a row filter or per row group, on 8-bit / int16 rows, on the sharded handles;
 * deferred ("async_search") range searches; a CSR-packed output (lims are the running sum of min(counts,
 * max_results)); more than 8192 rows per query.  (The graph engine has a range search of its own, approximate as its
 * walk is: expann_graph_range_search, at the end of this header.) */
int expann_range_search(expann_index* h, const void* queries, const float* radii, size_t m,
                        size_t max_results, uint64_t* ids, float* dists, uint32_t* counts);      /* host buffers */
int expann_range_search_device(expann_index* h, const void* d_queries, const float* d_radii, size_t m,
                               size_t max_results, uint64_t* d_ids, float* d_dists, uint32_t* d_counts,
                               void* stream);

/* Append rows to a built brute-force index (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed --
 * expann_add on a built handle still fails with "index already built").  The reference's brute_force_engine has no
 * frozen state (src/brute_force_engine.h:20-46: store, build, query, store, query works); these calls give a built
 * handle the same, without destroying it and staging, uploading and deriving every row again.
 * THE APPEND RULE.  After expann_append(h, R, r) on a handle that held the rows B -- R in the index's dtype and
 * layout, [r][dim] -- the new rows have the ids expann_size(h) + i (before the call), in insertion order, and EVERY
 * entry point returns, bit for bit, what a fresh handle made by expann_add(B), expann_add(R), expann_build with the
 * same options returns: ids, fp32 distance bits, ties by lower id, padding and counts -- expann_search and
 * expann_search_device (latency mode, "async_search" with expann_sync, k up to 8192), expann_score_ids (ids of
 * appended rows are valid), expann_range_search*, and the filter and group calls issued afterwards.  The exact top-k
 * by (score, id) is unique, so how the derived copies were brought up to date never shows in an answer.
 * What survives: the options, the profiling state, the statistics and the workspace.  What does not: a row filter
 * and row groups are CLEARED, as expann_build clears them -- they describe the rows they were set for; the caller
 * sets them again for the longer index.
 * All three calls first wait on the host for outstanding deferred searches (the row filter's rule), so every
 * search runs over the rows that were there when it was enqueued.  Both append calls return after the rows and the
 * copies are complete: one host wait per append, none per search.  expann_append_device reads d_rows in the order
 * of `stream` (a hipStream_t; NULL = the handle's own) and copies them: the caller may free them on return.
 * Errors, in this order, all before the device is touched: h == NULL EXPANN_ERR_INVALID_ARG; rows == NULL with
 * n > 0 EXPANN_ERR_INVALID_ARG; no rows on the device yet EXPANN_ERR_NOT_BUILT (before build() the call is
 * expann_add's job); rows adopted by expann_set_base_device EXPANN_ERR_UNSUPPORTED (they are the caller's memory);
 * n + expann_size(h) >= 2^32 - 32 EXPANN_ERR_UNSUPPORTED.  n == 0 is EXPANN_OK and does nothing.  A failed call
 * leaves the handle as it was and usable -- a failed allocation too: the larger base is built aside and swapped in.
 * CAPACITY.  expann_reserve(h, n_rows) makes room for at least n_rows rows: on a built handle that owns its rows it
 * reallocates now; before expann_build it is remembered and expann_build allocates max(staged, reserved) rows; a
 * value at or below the current capacity is EXPANN_OK and does nothing; on adopted rows EXPANN_ERR_UNSUPPORTED.
 * A reserve adds no rows, so it clears nothing: the filter, the groups and every derived copy stay (the fp16 copy
 * moves to a larger allocation with the base; what reads the base itself follows it to the new one).
 * Without a reserve, an append that does not fit grows the capacity by HALF (x 1.5, at least to what is needed), so a
 * run of appends copies O(total rows), at most three times the final size.  While a base is being grown the old
 * and the new allocation are both live (up to 2.5 x the old base, and the same for the fp16 copy beside it).  An
 * index that is never reserved or appended to allocates exactly what it allocated before these calls existed.
 * THE COPIES (csrc/bf_append.hpp is the one list of the rules, csrc/append_rows.hpp the device side).  The scaled
 * fp16 copy that every fp32 / fp16 search filters through, its two row-term arrays and max ||b||^2 are EXTENDED IN
 * PLACE by one kernel launch over the new rows when the scale of the longer index -- 2^floor(log2(32768 / max |v|)) --
 * is the current one; the extended arrays hold the bits a fresh build writes.  When the new rows raise max |v| past
 * a power of two, the copy is dropped and made again (at once where expann_build would make it, else by the next
 * search; the rows are in by then, so the append is EXPANN_OK even if that rebuild cannot be done now -- the next
 * search tries again and reports it).  Every other derived copy -- the uint8 shadow, the bf16x3 planes, the int8 filter's set, the 8-bit
 * indexes' row terms -- is dropped by every append and rebuilt by its next use.
 * expann_get_stat: "append_calls" and "append_rows" (accepted calls and their rows since create), "append_extends"
 * (appends that extended the fp16 copy in place), "append_rebuilds" (appends that had to drop it: the scale
 * changed), "base_capacity_rows" (rows the handle's own base allocation holds; before build() the reserved value;
 * 0 for adopted rows), "base_reallocs" (reallocations of the base since create, expann_reserve's included),
 * "copies_digest" (a 64-bit digest, independent of summation order, of the fp16 copy's rows and row terms over the
 * whole tiles the scans read, max ||b||^2 and the scale; 0 when there is no copy; computed on demand with a host wait,
 * never on a search path.  Results are exact whatever the copy holds, so only the digest shows that an extended copy
 * IS the fresh one: equal digests on an appended and on a freshly built handle of the same rows).
 * Not offered: appending to rows adopted by expann_set_base_device or to the sharded handles (expann_sharded_add
 * after build still fails); keeping a filter or groups across
 * an append; a deferred append; in-place extension of the int8 filter's, the uint8 shadow's, the bf16x3 and the
 * 8-bit copies -- they are rebuilt whole at the next search that uses them.  What that costs, measured on a
 * 1 M x d128 fp32 index at default options, where 10 000-query batches run the int8 filter
 * (profiles/bf_append_ab.txt): the first search after an append takes 2.6 .. 2.8 ms against 1.64 ms in steady state,
 * about 1.0 ms once per append -- more than the append itself (0.84 ms for 1 000 rows, against 139 ms for destroy +
 * add + build).  Extending that copy in place would be worth building for a caller that alternates single appends
 * with single batches; at one append per hundred batches it is 0.6 % of the search time.  (Removing rows:
 * expann_remove, at the end of this header.) */
int expann_append(expann_index* h, const void* rows, size_t n);                          /* host rows   */
int expann_append_device(expann_index* h, const void* d_rows, size_t n, void* stream);   /* device rows */
int expann_reserve(expann_index* h, size_t n_rows);

/* Range search of the graph engine: the rows within a per-query radius, found by the walk (appended;
 * EXPANN_ABI_VERSION stays 2: nothing that existed changed).  The reference has no range query: the rule is this
 * project's, stated so that a CPU restatement pins it bit for bit (tests/graph_range_helpers.py).
 * THE RANGE WALK RULE.
 * Inputs.  Per query a radius r = radii[i] in squared-L2 units, the units expann_graph_search reports.  Per call
 * ef = ef_search >= 1 and R = max_results >= 0; cap = max(ef, R).  Mode 0 only: fp32 bottom layer, over fp32 or
 * binary16 rows.  Below, "d > r" means "not d <= r": the comparison with the radius is inclusive, and a NaN radius is
 * in range of nothing.
 * Descent.  Entry evaluation and greedy descent are unchanged and never look at r.
 * Bottom layer.  The queues `candidates` (min) and `nearest` (max) are the plain walk's, with the libstdc++ heap
 * behaviour it reproduces.  `count` starts at 0.
 *   The entry vertex is scored, marked visited, and pushed on both queues.
 *   Every scored bottom-layer vertex with d <= r adds 1 to `count`, whether or not it is kept.  The entry vertex counts.
 *   Stop when `candidates` is empty, or when nearest.size() >= ef && cur.d > nearest.top().d && (cur.d > r ||
 *   nearest.size() >= cap), cur being the best candidate.
 *   Neighbour update.  For each unvisited neighbour in adjacency order, with distance dn: accept when nearest.size() <
 *   ef || dn < nearest.top().d || (dn <= r && nearest.size() < cap).  An accepted neighbour is pushed on `candidates`
 *   and on `nearest`.  Then `nearest` is popped once if nearest.size() > ef && (nearest.top().d > r || nearest.size() >
 *   cap).
 *   Invariant, which follows: either nearest.size() <= ef, or every entry of `nearest` is in range and nearest.size()
 *   <= cap.
 * Output.  Drain `nearest` and reverse it: ascending distance, equal distances in the heap's order, as
 * expann_graph_search returns them, and not by id.  The leading entries with d <= r are the result.
 *   ids[i][0 .. R) and dists[i][...] hold the first min(that number, R) of them, padded with UINT64_MAX / +inf.
 *   counts[i] = count.
 *   distcomps[i] is as for the plain walk: descent plus every scored vertex.
 * What counts means.  It is the number of distinct in-range rows the walk scored.  It is never more than the true
 * number.  counts[i] > R tells the caller that the row was truncated; what it holds are the nearest rows the walk
 * kept.  counts[i] may be smaller than the true number: this is an approximate search.  Every returned row is truly in
 * range, because the distances are the exact fp32 ones.
 * Consequences.  With R <= ef, cap equals ef: the walk is the plain walk at that ef, with equal distcomps, and the
 * output is its result cut at r and at R; so r = +inf gives expann_graph_search(k = R, ef) bit for bit.  With r < 0 or
 * NaN, at any R, the walk is the plain walk: distcomps equal the plain walk's, counts is 0, the rows are padding.
 * Pre-drop (the kernel's; it changes nothing).  With full0 = nearest.size() >= ef, worst0 = nearest.top().d and n0 =
 * nearest.size() at the start of the hop, a neighbour is dropped before the queue update iff full0 && !(dn < worst0)
 * && !(dn <= r && n0 < cap): while the top is above r it only falls; once every entry is in range it rises only up to
 * r; at cap it only falls again.  A neighbour is counted before it is dropped.
 * Binary16 handles return what the fp32 handle of the upcast rows returns, bit for bit (THE F16 ROW RULE).
 * Arguments.  dists and distcomps may be NULL.  With max_results == 0 the call only counts, and ids may be NULL.
 * Checks, in this order, all before the device is touched: handle NULL EXPANN_ERR_INVALID_ARG; ef_search == 0
 * EXPANN_ERR_INVALID_ARG; m == 0 EXPANN_OK, nothing enqueued; queries, radii or counts NULL, or ids NULL with
 * max_results > 0, EXPANN_ERR_INVALID_ARG; ef_search > 4096 or max_results > 4096 EXPANN_ERR_UNSUPPORTED (by value);
 * a row filter in force EXPANN_ERR_UNSUPPORTED.  Row groups that are merely set are ignored.  A working set beyond
 * the LDS is EXPANN_ERR_UNSUPPORTED, as for the plain searches.
 * The redo launch, "cand_capacity" / "redo_capacity" and EXPANN_ERR_OVERFLOW work as for expann_graph_search_device;
 * in-range neighbours are pushed on `candidates` while `nearest` is full, so a range walk overflows a capacity sooner
 * than a plain one.  expann_graph_range_search_device keeps expann_graph_search_device's promises: it enqueues on
 * `stream` and returns without waiting; in steady state it makes no allocation, copy, query or synchronisation; it
 * counts towards the 256 outstanding searches; expann_graph_sync reports EXPANN_ERR_OVERFLOW.
 * expann_graph_range_search (host buffers) enqueues the same launches and waits.  expann_graph_last_kernel_ms covers
 * the range launches.  expann_graph_get_stat "range_searches" = range searches since create, from either entry point.
 * The expann_antitopo_* calls search the engine's graph with its sticky ef_search; when that is unset it is set as
 * expann_antitopo_query sets it, with k = max(1, max_results).  The engine's compression mode is not consulted: the
 * range walk is fp32.  Before build() they return EXPANN_ERR_NOT_BUILT.
 * Not offered: the byte modes 1 and 2 -- they walk on integer distances, which a squared-L2 radius does not cut; the
 * calls have no `mode` argument for that reason; range search under a row filter or per row group; an order by id
 * among equal distances; more than 4096 rows per query; the sharded handles.  (Exact range search: expann_range_search
 * on a brute-force index of the same rows.) */
int expann_graph_range_search(expann_graph* g, const float* queries, const float* radii, size_t m,
                              size_t max_results, size_t ef_search, uint64_t* ids, float* dists,
                              uint32_t* counts, uint32_t* distcomps);             /* host buffers */
int expann_graph_range_search_device(expann_graph* g, const float* d_queries, const float* d_radii, size_t m,
                                     size_t max_results, size_t ef_search, uint64_t* d_ids, float* d_dists,
                                     uint32_t* d_counts, uint32_t* d_distcomps, void* stream);
int expann_antitopo_range_query(expann_antitopo* e, const float* queries, const float* radii, size_t m,
                                size_t max_results, uint64_t* ids, float* dists, uint32_t* counts);
int expann_antitopo_range_query_device(expann_antitopo* e, const float* d_queries, const float* d_radii, size_t m,
                                       size_t max_results, uint64_t* d_ids, float* d_dists, uint32_t* d_counts,
                                       void* stream);

/* Remove rows from a built brute-force index (appended; EXPANN_ABI_VERSION stays 2: nothing that existed changed,
 * and a handle that never calls these allocates and launches exactly what it did).  With expann_append this
 * completes the life of a handle: store, build, query, append, remove, query; an upsert is a remove followed by an
 * append; tombstones set through the row filter become reclaimed space with one call.
 * THE REMOVE RULE.
 * What an id is.  `ids` are the ids a search returns: row numbers.  Only a handle that owns its rows can remove,
 * and such a handle has id_offset 0.  The ids may come in any order and may repeat; a repeated id counts once.
 * What the handle holds afterwards.  Let S be the set of distinct ids.  The handle holds the rows not in S, in their
 * old order; expann_size drops by |S|; the survivor that had id i now has id i - |{s in S : s < i}| -- the
 * order-preserving shift of a flat index: the caller keeps any external id map, and the next append gets ids
 * starting at the new size.
 * Exactness.  EVERY entry point then returns, bit for bit, what a fresh handle made by expann_add of the survivors
 * in that order, expann_build and the same options returns: ids, fp32 distance bits, ties by lower id, padding and
 * counts -- expann_search and expann_search_device (latency mode, "async_search" with expann_sync, k up to 8192),
 * expann_score_ids, expann_range_search*, and the filter, group and append calls issued afterwards.
 * *n_removed may be NULL; when given it receives |S|.
 * expann_compact_row_filter removes every row the row filter in force disallows -- the same rule with S = the
 * disallowed rows -- and clears the filter: it makes the tombstones permanent.
 * What survives: the options, the profiling state, the statistics, the workspace and the base's CAPACITY --
 * "base_capacity_rows" is unchanged, so the freed room serves later appends without a reallocation, and a remove
 * does not count in "base_reallocs" (the base did not grow).  What does not: a row filter and row groups are
 * CLEARED, as an append clears them; every derived copy except the fp16 copy is forgotten and rebuilt by its next
 * use, as after an append.
 * All dtypes: F32, F16, U8, I8 and I16 rows can be removed; the base compaction moves bytes.  Only float rows have
 * an fp16 copy to carry over.
 * All three calls first wait on the host for outstanding deferred searches (the append's rule), so every search
 * runs over the rows that were there when it was enqueued.  One host wait per call, none per search.
 * expann_remove_device reads d_ids in the order of `stream` (a hipStream_t; NULL = the handle's own); the caller may
 * free them on return.
 * THE COPIES (csrc/bf_remove.hpp is the one list of the rules, csrc/remove_rows.hpp the device side).  The scaled
 * fp16 copy, its two row-term arrays, max ||b||^2 and max |v| describe the rows they were made from, and a row's
 * fp16 row and terms depend on that row, the dim, the metric and the scale alone.  When the survivors' scale --
 * 2^floor(log2(32768 / max |v| over the survivors)) -- is the current one, the copy is COMPACTED: the survivors'
 * fp16 rows and terms are gathered to their new positions, both maxima are recomputed over the survivors with the
 * bits a fresh build computes, the tiles the scans read shrink to the survivors in whole tiles, and everything
 * behind the new size is what a build initialises (zero rows, NaN terms: later in-place appends rely on it);
 * "copies_digest" then equals a fresh handle's.  When the removed rows carried max |v| across a power of two, the
 * copy is dropped and made again (at once where expann_build would make it, else by the next search; the remove has
 * succeeded by then whatever becomes of the copy).  When the rows were marked unusable for fp16 (a NaN, an inf, an
 * astronomically large value) the mark is forgotten -- the survivors may fit -- and the copy is treated as dropped.
 * BUILT ASIDE.  A base of the same capacity and, where the copy is kept, fp16 arrays of the same size are built
 * aside, the survivors are compacted into them, and the handle swaps them in only after the one host wait has
 * shown that everything succeeded.  So a call that fails -- a bad id, a failed allocation -- leaves the handle as
 * it was and usable; and DURING a call the old and the new base, and the two fp16 copies, are both live: the rows
 * briefly take twice their memory.
 * Errors, in this order, all before the device is touched: h == NULL EXPANN_ERR_INVALID_ARG; ids == NULL with
 * n_ids > 0 EXPANN_ERR_INVALID_ARG; no rows on the device EXPANN_ERR_NOT_BUILT; rows adopted by
 * expann_set_base_device EXPANN_ERR_UNSUPPORTED.  n_ids == 0 is EXPANN_OK and does nothing.  Then, decided before
 * any row of the handle changes and learnt at the call's one host wait: an id at or beyond expann_size(h), and a
 * removal that would leave no row (an index is never empty, as expann_build refuses an empty one), both
 * EXPANN_ERR_INVALID_ARG.  An id out of range is refused by a comparison made before the bitmap is touched.
 * expann_compact_row_filter with no filter in force is EXPANN_ERR_INVALID_ARG; with a filter that allows no row
 * EXPANN_ERR_INVALID_ARG, and the filter stays; a filter that allows every row removes nothing, clears the filter
 * and keeps every copy.
 * expann_get_stat: "remove_calls" (accepted calls since create), "remove_rows" (rows removed), "remove_compacts"
 * (removes that carried the fp16 copy over), "remove_rebuilds" (removes that dropped it or forgot an unusable mark).
 * Not offered: compaction in place (the rows take twice their memory during a call); shrinking the capacity;
 * the sharded handles; rows adopted by expann_set_base_device; keeping a filter or groups across a remove; a
 * deferred remove; stable external ids -- they stay the caller's map. */
int expann_remove(expann_index* h, const uint64_t* ids, size_t n_ids, size_t* n_removed);             /* host ids   */
int expann_remove_device(expann_index* h, const uint64_t* d_ids, size_t n_ids, void* stream,
                         size_t* n_removed);                                                          /* device ids */
int expann_compact_row_filter(expann_index* h, size_t* n_removed);

/* Append rows to a built graph engine without uploading the graph again (appended; EXPANN_ABI_VERSION stays 2:
 * nothing that existed changed, and a handle that never calls these allocates and launches exactly what it did).
 * THE GRAPH APPEND RULE.  After expann_antitopo_append(e, R, r) on a built engine of n rows the new rows have the ids
 * n .. n + r - 1, and the engine is in the state that expann_antitopo_store_batched(e, R, r, 0) followed by
 * expann_antitopo_build(e) leaves: the index expann_antitopo_save writes, max_layer and starting_vertex, the state
 * of the level generator, and the graph the walk sees.  The batches are THE BATCH RULE's with max_batch = 0, the
 * levels are the same draws, the kernels are the same; "the same" has the freedom THE BATCH RULE leaves -- the order
 * of the reverse edges within a row that was not re-pruned.
 *   The device graph is always exactly flatten() of the host graph the engine would save, neighbour for neighbour in
 * the same order: every search entry point answers, bit for bit, as a fresh engine that loads the saved index.
 *   An append first waits, on the host, for the handle's outstanding device-buffer searches, as expann_graph_search
 * does: a search enqueued before the append runs on the graph as it was.
 *   A row filter and row groups are CLEARED, as expann_antitopo_store clears them; the uint8 and the ranged-int8 copy
 * of the rows are dropped and made again by their next use (the ranged scale is global: it may change with the rows).
 * THE DEVICE ROUTE serves engines with fp32 rows, ortho_count == 1 and at least 2048 rows.  The handle's FIRST append
 * uploads the builder's view of the graph once -- the fixed-stride rows of (id, distance) that
 * expann_graph_build_batched works on, (M0 + 64) x 8 bytes per row: 1.47 GB at 1 M rows and M = 60 -- and keeps it,
 * sized to a CAPACITY in rows, beside the walk's tables; the rows themselves are not kept twice.  Every later append
 * uploads the new rows and their levels, runs the batches on the resident state, and remakes the walk's tables --
 * the fixed-stride layer-0 table and the CSR -- from it on the device (csrc/graph_append.hpp: a degree pass, an
 * exclusive scan, a fill); no transfer and no host work is proportional to the rows already in the graph.  The
 * capacity covers everything that is sized by the row count (rows, tables, builder state, visited sets);
 * expann_antitopo_reserve sets it, a full handle grows by half, and the upper-layer arrays have a capacity of their
 * own.  The capacity belongs to the device graph: expann_antitopo_build and expann_antitopo_load make a new one.
 *   The host index goes stale: an append adds the new rows to the host's vectors and marks the adjacency stale; what
 * reads the host graph -- expann_antitopo_save, _store, _store_batched, _build -- first downloads the builder's state.
 * expann_antitopo_size is right at all times.
 *   A batch whose construction search overflows its candidates queue leaves the graph as it was after the batch
 * before: the call returns EXPANN_ERR_OVERFLOW, *n_appended says how many rows are in, and the engine answers as if
 * only those had been given (the level generator stands after that many draws).
 * THE HOST ROUTE, inside the same call: engines with binary16 rows (the builder works on fp32 rows, the handle holds
 * halves), with ortho_count != 1, or smaller than 2048 rows take expann_antitopo_store_batched +
 * expann_antitopo_build as they are -- correct, and no faster.
 * Errors, all before the device is touched: e == NULL, or rows == NULL with n > 0, EXPANN_ERR_INVALID_ARG; before
 * expann_antitopo_build EXPANN_ERR_NOT_BUILT; n == 0 is EXPANN_OK and does nothing.  n_appended may be NULL.
 * expann_antitopo_reserve below the current capacity does nothing; before expann_antitopo_build it is
 * EXPANN_ERR_NOT_BUILT; on an engine of the host route it is EXPANN_OK and does nothing.
 * expann_graph_get_stat (expann_antitopo_get_stat reads the engine's graph handle by the same names; before
 * expann_antitopo_build EXPANN_ERR_NOT_BUILT): "append_calls", "append_rows", "append_batches", "append_device" =
 * appends served on the device, "append_host" = appends that took the host route, "capacity_rows", "graph_reallocs" =
 * appends that had to grow the capacity; "append_tables_ns" = device time of the last remake of the walk's tables,
 * "append_edges" = the edges of all layers it counted.  The host route makes a new graph handle; the counts are
 * carried over.
 * Not offered: rows already on the device; a deferred append; the sharded handles (rows are taken OUT of a graph by
 * THE GRAPH REMOVE RULE, at the end of this header); making the
 * builder's state from the device CSR instead of the one-time upload; giving the resident state's memory back short
 * of destroying the engine; more than 8 Mi rows (the host route serves them). */
int expann_antitopo_append(expann_antitopo* e, const float* rows, size_t n, size_t* n_appended);
int expann_antitopo_reserve(expann_antitopo* e, size_t n_rows);
int expann_antitopo_get_stat(expann_antitopo* e, const char* name, uint64_t* out);
/* The library calls under the device route, for callers that keep their own host graph (gpu_antitopo_engine.h is
 * one).  expann_graph_adopt_build_state makes the builder's state resident: the arrays of
 * expann_graph_build_batched for the handle's n rows (levels[n], upper_idx[n], ids0 / d0 [n][stride0], deg0[n], idsu
 * / du [(l - 1) * U + upper_idx[v]][strideu], degu), which must describe the graph the handle was created from, and
 * the builder's parameters; every id, level and degree is checked (a row holds at most M0 / M edges).  Binary16
 * handles and handles beyond 8 Mi rows are EXPANN_ERR_UNSUPPORTED.  expann_graph_append inserts rows[n][dim] with
 * levels[n] by THE BATCH RULE (max_batch = 0) and remakes the walk's tables; *max_layer_out / *starting_vertex_out /
 * *n_appended (each may be NULL) receive the graph's after the call, also with EXPANN_ERR_OVERFLOW (above); before
 * expann_graph_adopt_build_state it is EXPANN_ERR_NOT_BUILT.  expann_graph_build_state_shape fills shape[6] = {rows,
 * U_stride, n_upper_layers, U, stride0, strideu} and expann_graph_read_build_state downloads the arrays in that
 * shape: the upper arrays are [n_upper_layers][U_stride] rows, of which the first U per layer are in use.
 * expann_graph_reserve grows the capacity of any graph handle (EXPANN_ERR_UNSUPPORTED beyond 8 Mi rows).
 * expann_graph_note_host_append counts one append of `rows` rows served by the host route, on top of carried[6] =
 * {"append_calls", "append_rows", "append_batches", "append_device", "append_host", "graph_reallocs"} of the handle
 * it replaces (NULL: on top of its own). */
int expann_graph_reserve(expann_graph* g, size_t n_rows);
int expann_graph_adopt_build_state(expann_graph* g, size_t M, size_t M0, size_t ef_construction, size_t prune_overflow,
                                   float ortho_factor, float ortho_bias, const uint8_t* levels, const int32_t* upper_idx,
                                   const uint32_t* ids0, const float* d0, const uint32_t* deg0, size_t stride0, size_t U,
                                   size_t n_upper_layers, const uint32_t* idsu, const float* du, const uint32_t* degu,
                                   size_t strideu);
int expann_graph_append(expann_graph* g, const float* rows, size_t n, const uint8_t* levels, uint32_t* max_layer_out,
                        uint32_t* starting_vertex_out, size_t* n_appended);
int expann_graph_build_state_shape(expann_graph* g, size_t* shape);
int expann_graph_read_build_state(expann_graph* g, uint8_t* levels, int32_t* upper_idx, uint32_t* ids0, float* d0,
                                  uint32_t* deg0, uint32_t* idsu, float* du, uint32_t* degu);
int expann_graph_note_host_append(expann_graph* g, const uint64_t* carried, size_t rows);

/* Remove rows from a built graph engine: the neighbours of the removed rows are repaired on the device (appended;
 * EXPANN_ABI_VERSION stays 2: nothing that existed changed, and a handle that never calls these allocates and
 * launches exactly what it did).  The reference has no deletion: the rule is this project's own, exact, restated on
 * the CPU (antitopo_index::remove_rows, include/expann/antitopo_index.h) and in NumPy (tests/graph_remove_helpers.py).
 * THE GRAPH REMOVE RULE.  Let S be the distinct ids given to expann_antitopo_remove(e, ids, n_ids, &n_removed) -- any
 * order, repeats allowed, as for expann_remove -- and n the size before the call.
 *   IDS.  Survivors keep their order: the survivor with id i gets id i - |{s in S : s < i}|.  expann_antitopo_size
 * drops by |S| = *n_removed, the next append gets ids from the new size on, and the level generator is not touched:
 * it stands after as many draws as rows were ever inserted.
 *   LEVELS.  A survivor keeps its level.  max_layer = 1 + the highest level among the survivors; starting_vertex =
 * the lowest new id among the survivors of that level (what insert_with_level's `while (new_max_layer >= max_layer)`
 * leaves for those rows in that order: the old starting vertex when nothing at the top is removed).  upper_idx is the
 * rank among the survivors with level >= 1 in id order (to_strided's rule).
 *   ROWS, per layer l and surviving vertex v of level >= l, everything read from the graph as it was BEFORE the call.
 * An UNTOUCHED row -- no neighbour in S -- keeps its entries, their order and their lengths; only the ids are
 * renumbered.  A TOUCHED row -- at least one neighbour in S -- is made again from these candidates: (1) its surviving
 * neighbours with their stored lengths; (2) for every removed neighbour r, in row order, r's surviving layer-l
 * neighbours c != v that are not candidates already, with length dist2(v, c) in the reference's 16-lane FMA order
 * (the bits of dist2_ref_order, antitopo_index.h).  One hop only: the removed neighbours of a removed neighbour are
 * not followed.  A candidate is identified by its id; an own entry wins over an adopted duplicate.  Of the distinct
 * candidates the `cap` smallest in (length, id) order are kept, cap = max(ef_construction, M0) -- at most 1024, which
 * expann_graph_adopt_build_state enforces: a touched row is pruned from no more candidates than an inserted row is --
 * and that list goes through prune_edges(l, v, lazy = false) to at most M0 (layer 0) or M (above) edges: the
 * builder's rule with the builder's arithmetic (ortho_term unfused, first of equals).  A touched row may end up
 * empty.  No reverse edges are added; all touched rows are computed from the old graph, so the result does not depend
 * on any order of processing.
 *   The device graph is always exactly flatten() of the host graph the engine would save, neighbour for neighbour in
 * the same order: every search entry point answers, bit for bit, as a fresh engine that loads the saved index.
 *   A remove first waits, on the host, for the handle's outstanding device-buffer searches: a search enqueued before
 * the remove runs on the graph as it was.  A row filter and row groups are CLEARED; the uint8 and the ranged-int8
 * copy of the rows are dropped and made again by their next use.  The capacity stays: the freed room serves later
 * appends.  The host adjacency goes stale exactly as after an append, and the host's copy of the vectors is compacted
 * on the host -- the one piece of work proportional to n.
 * THE DEVICE ROUTE serves engines with fp32 rows, ortho_count == 1, at least 2048 and at most 8 Mi rows at the time
 * of the call; when the builder's state is not resident yet the call uploads it once, as a first append does.  On the
 * handle's stream (csrc/graph_remove.hpp): the keep bitmap and the id map of expann_remove (csrc/keep_bitmap.hpp), a
 * touch pass that lists the touched rows, a gather kernel -- one workgroup per touched row: candidates collected,
 * deduplicated and cut to `cap` in LDS, adopted lengths by 16 lanes per row -- the builder's own build_prune_kernel
 * over those lists, the compaction of rows, levels and adjacency arrays under the new ids into arrays built aside at
 * the same capacity, and the append's remake of the walk's tables.  The out-of-range flag, the survivor count and the
 * touched-row count are read at the call's one early host wait, and everything built aside is allocated before the
 * first row changes.
 * THE HOST ROUTE, inside the same call: every other engine takes antitopo_index::remove_rows followed by
 * expann_antitopo_build -- correct, and no faster than a re-upload.
 * Refusals, all decided before anything in the engine changes: e == NULL, or ids == NULL with n_ids > 0,
 * EXPANN_ERR_INVALID_ARG; before expann_antitopo_build EXPANN_ERR_NOT_BUILT; an id >= size EXPANN_ERR_INVALID_ARG; a
 * removal that would leave no row EXPANN_ERR_INVALID_ARG; n_ids == 0 is EXPANN_OK and nothing happens.  A refused
 * call leaves the engine as it was and usable.  n_removed may be NULL.
 * expann_antitopo_compact_row_filter applies the same rule with S = the rows the bitmap filter in force disallows: it
 * makes tombstones permanent.  No filter in force, or a filter that allows no row: EXPANN_ERR_INVALID_ARG; a filter
 * that allows every row removes nothing and is cleared.
 * expann_graph_get_stat / expann_antitopo_get_stat: "remove_calls", "remove_rows", "remove_touched_rows",
 * "remove_truncated_rows" = touched rows whose distinct candidates exceeded cap, "remove_device" / "remove_host" =
 * removes by route, "remove_repair_ns" = device time of touch + gather + prune of the last call.  The host route
 * makes a new graph handle; the counts are carried over.
 * Not offered: ids already on the device; reverse edges for adopted neighbours; following more than one hop;
 * shrinking the capacity; a deferred remove; the sharded handles; stable external ids. */
int expann_antitopo_remove(expann_antitopo* e, const uint64_t* ids, size_t n_ids, size_t* n_removed);
int expann_antitopo_compact_row_filter(expann_antitopo* e, size_t* n_removed);
/* The library calls underneath.  expann_graph_remove applies the rule to a handle whose builder state is resident
 * (before expann_graph_adopt_build_state EXPANN_ERR_NOT_BUILT); *max_layer_out / *starting_vertex_out / *n_removed
 * (each may be NULL) receive the graph's after the call; the caller compacts its own host rows.
 * expann_graph_note_host_remove counts one remove of `rows` rows served by the host route, on top of carried[13] = the
 * seven remove counters above followed by the six append counters of expann_graph_note_host_append, both of the handle
 * it replaces (NULL: on top of its own).  expann_graph_read_row_filter copies the bitmap filter in force to
 * allow_bits[ceil(n / 32)] (no filter in force: EXPANN_ERR_INVALID_ARG). */
int expann_graph_remove(expann_graph* g, const uint64_t* ids, size_t n_ids, uint32_t* max_layer_out,
                        uint32_t* starting_vertex_out, size_t* n_removed);
int expann_graph_note_host_remove(expann_graph* g, const uint64_t* carried, size_t rows);
int expann_graph_read_row_filter(expann_graph* g, uint32_t* allow_bits, size_t n_words);

#ifdef __cplusplus
}
#endif
#endif
