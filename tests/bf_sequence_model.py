"""Model-based operation sequences for the mutable brute-force handle.

Three parts, none of which touches a GPU or the HIP library:
  Model      -- the truth about a handle in plain NumPy: its rows (an id is a position), its row filter, its row labels,
                its capacity and options, and the documented refusals by status code.  The arithmetic of every expected
                answer is the unchanged CPU oracle.
  generate() -- a pure function (config, seed) -> about 40 operations, reads and mutations interleaved, every mutation
                QUERY-RELEVANT: an append carries near copies of a third of the queries, a remove takes the current
                nearest row of a third of them, a filter or a labelling has a random density between 1 % and 60 %.
  run()      -- the driver: after every mutation it checks size(), a search at the step's (m, k) and one more entry
                point in turn, exactly (ids, distance bit patterns, counts, status codes), and the stat facts the design
                states.  A failure names the config, the seed, the step and the operations up to it; replay() rebuilds
                that prefix.
FakeEngine is the engine's interface over a second Model; its stale subclasses are how tests/test_bf_sequence_model.py
shows that the driver notices staleness without a broken library."""
import collections
import functools

import numpy as np

import row_groups_helpers as rgh

PAD = np.uint64(2 ** 64 - 1)
ANY = 0xFFFFFFFF
OK, INVALID_ARG, NOT_BUILT, UNSUPPORTED = 0, 1, 4, 5
M = 130                      # queries of a sequence
MS, KS = (1, 7, 130), (1, 10, 100)
TILE = 128                   # rows of the widest scan tile
DIRECT_BELOW = 4096          # under this many rows the direct scan serves and a build makes no fp16 copy
GROUP_LIST_ROWS_AUTO = 16384
RANGE_MAX_RESULTS = 128
N0 = 3900
SEEDS = (0, 1, 2)
# The sequences live between 1 500 and 10 000 rows.  Three derived copies exist only from a row count on that the
# planner sets (csrc/bf_plan.hpp): the int8 filter's set and the 8-bit hit-queue operand from 32 768 rows, the uint8
# shadow from 65 536.  The configs that are about them (B, F, C) end with an excursion past that size.
I8_MIN_ROWS, U8_SHADOW_ROWS = 32768, 65536
MAX_ROWS = {"A": 10000, "B": 40000, "C": 75000, "D": 10000, "E": 10000, "F": 42000}

Config = collections.namedtuple("Config", "name dtype metric d data options async_seed")
# options: B changes them mid-sequence; async_seed: the seed that runs the deferred pattern on device buffers
CONFIGS = {
    "A": Config("A", "f32", "l2", 128, "gauss", False, 2),
    "B": Config("B", "f32", "l2", 128, "gauss", True, None),
    "C": Config("C", "f32", "l2", 128, "int255", False, None),
    "D": Config("D", "f32", "ip", 144, "gauss", False, None),
    "E": Config("E", "f16", "l2", 256, "gauss", False, 1),
    "F": Config("F", "8bit", None, 128, "8bit", False, None),   # seed 0: u8 L2; seeds 1, 2: i8 inner product
}


def resolve(cfg, seed):
    """config F names two engines: the seed picks one"""
    if isinstance(cfg, str):
        cfg = CONFIGS[cfg]
    if cfg.dtype != "8bit":
        return cfg
    return cfg._replace(dtype="u8", metric="l2", data="u8") if seed % 3 == 0 else \
        cfg._replace(dtype="i8", metric="ip", data="i8")


def float_rows(cfg):
    return cfg.dtype in ("f32", "f16")


class Refused(Exception):
    """what a FakeEngine raises: the status code a refused call returns"""

    def __init__(self, code):
        super().__init__("refused with status %d" % code)
        self.code = code


def _oracle_metric(oracle, cfg):
    if cfg.dtype == "u8":
        return oracle.METRIC_L2_U8
    if cfg.dtype == "i8":
        return oracle.METRIC_IP_I8
    return oracle.METRIC_IP_F32 if cfg.metric == "ip" else oracle.METRIC_L2_F32


def grown_capacity(capacity, need):
    """csrc/bf_append.hpp: an append that does not fit grows the capacity by half, at least to what is needed"""
    return max(capacity + capacity // 2, need)


def range_expected(ref, radii, max_results):
    """the rule of test_gpu_range_search.expected with full=True: ref is the oracle's sorted prefix at k = all rows, so
    every count is proven"""
    from test_gpu_range_search import expected
    return expected(ref, radii, max_results, full=True)


class Model:
    """What a brute-force handle must contain, and what each entry point must therefore answer."""

    def __init__(self, oracle, cfg, rows, owned=True):
        self.oracle, self.cfg = oracle, cfg
        self.metric = _oracle_metric(oracle, cfg)
        self.rows = self._stored(rows)
        self.owned = owned
        self.allow = None        # the row filter in force (bool [n]) or None
        self.labels = None       # the row labels (uint32 [n]) or None
        self.capacity = self.rows.shape[0]
        self.reallocs = 0
        self.reserved = False    # the capacity in force was set by a reserve
        self.options = {}
        self.filter_used = False  # a search ran under the filter in force
        self.last_tiers = None   # tiers of the last grouped search
        self.tags = []           # what the last call was, for the coverage conditions

    # ---- the rows ------------------------------------------------------------------------------------------
    def _stored(self, rows):
        """rows as the handle keeps them, in the oracle's type (binary16 rows: what the cast leaves, as fp32)"""
        rows = np.asarray(rows)
        if self.cfg.dtype == "f16":
            return np.ascontiguousarray(rows.astype(np.float16).astype(np.float32))
        return np.ascontiguousarray(rows, dtype={"f32": np.float32, "u8": np.uint8, "i8": np.int8}[self.cfg.dtype])

    @property
    def n(self):
        return self.rows.shape[0]

    def maxabs(self):
        return float(np.abs(self.rows.astype(np.float64)).max())

    @staticmethod
    def _scale_exp(maxabs):
        return int(np.floor(np.log2(32768.0 / maxabs))) if maxabs > 0 else 0

    # ---- mutations: each returns the status code the handle returns -------------------------------------------------
    def append(self, rows):
        self.tags = []
        rows = self._stored(rows)
        if not self.owned:
            return UNSUPPORTED
        if rows.shape[0] == 0:
            return OK
        n0, n1 = self.n, self.n + rows.shape[0]
        old_max, new_max = self.maxabs(), float(np.abs(rows.astype(np.float64)).max())
        if n1 > self.capacity:
            self.capacity = grown_capacity(self.capacity, n1)
            self.reallocs += 1
            self.reserved = False
            self.tags.append("cap_growth")
        elif self.reserved:
            self.tags.append("within_reserve")
        self.rows = np.concatenate([self.rows, rows])
        self.allow = self.labels = None
        self.filter_used = False
        self.tags.append("tile_exact" if n1 % TILE == 0 else "tile_inside")
        if n0 < DIRECT_BELOW <= n1:
            self.tags.append("cross_up")
        if new_max >= 2 * old_max:
            self.tags.append("scale_append")
            assert self._scale_exp(max(new_max, old_max)) != self._scale_exp(old_max)
        return OK

    def reserve(self, n):
        self.tags = []
        if not self.owned:
            return UNSUPPORTED
        if n > self.capacity:
            self.capacity = int(n)
            self.reallocs += 1
            self.reserved = True
            self.tags.append("reserve_grows")
        return OK

    def remove(self, ids):
        self.tags = []
        if not self.owned:
            return UNSUPPORTED
        ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        if ids.size == 0:
            return OK
        gone = np.unique(ids)
        if gone[-1] >= self.n:
            self.tags.append("refuse_remove_id")
            return INVALID_ARG
        if gone.size == self.n:
            self.tags.append("refuse_remove_all")
            return INVALID_ARG
        if self.allow is not None and self.filter_used:
            self.tags.append("remove_after_filter_used")
        self._take_out(gone.astype(np.int64))
        return OK

    def _take_out(self, gone):
        n0, old_max = self.n, self.maxabs()
        carried = np.abs(self.rows[gone].astype(np.float64)).max() == old_max if gone.size else False
        self.rows = np.ascontiguousarray(np.delete(self.rows, gone, axis=0))
        self.allow = self.labels = None
        self.filter_used = False
        if self.n < DIRECT_BELOW <= n0:
            self.tags.append("cross_down")
        if carried and self._scale_exp(self.maxabs()) != self._scale_exp(old_max):
            self.tags.append("max_row_removed")

    def compact_row_filter(self):
        self.tags = []
        if not self.owned:
            return UNSUPPORTED
        if self.allow is None:
            self.tags.append("refuse_compact_nofilter")
            return INVALID_ARG
        if not self.allow.any():
            self.tags.append("refuse_compact_zero")
            return INVALID_ARG
        self.tags.append("compact")
        self._take_out(np.flatnonzero(~self.allow))
        return OK

    def set_row_filter(self, allow):
        self.tags = []
        if allow is None:
            self.allow = None
            self.filter_used = False
            return OK
        if not float_rows(self.cfg):
            self.tags.append("refuse_filter_8bit")
            return UNSUPPORTED
        allow = np.asarray(allow).astype(bool).reshape(-1)
        if allow.size < self.n:
            return INVALID_ARG
        self.allow = allow[:self.n].copy()
        self.filter_used = False
        return OK

    def set_row_groups(self, labels):
        self.tags = []
        if labels is None:
            self.labels = None
            return OK
        if not float_rows(self.cfg):
            self.tags.append("refuse_groups_8bit")
            return UNSUPPORTED
        labels = np.asarray(labels, dtype=np.uint32).reshape(-1)
        if labels.size != self.n:
            return INVALID_ARG
        self.labels = labels.copy()
        return OK

    def set_option(self, name, value):
        self.tags = []
        self.options[name] = int(value)
        return OK

    # ---- reads: (status, answer) ----------------------------------------------------------------------------------
    def _ip(self):
        return self.cfg.metric == "ip"

    def search_refused(self):
        """ "scan_kernel" 2 names the 8-bit matrix-core form: float rows have none and the search says so"""
        return float_rows(self.cfg) and self.options.get("scan_kernel", 0) == 2

    def plain(self, queries, k, rows=None):
        """the oracle over `rows` (default: all of the handle's), no filter"""
        rows = self.rows if rows is None else rows
        return self.oracle.brute_force(rows, queries, k, self.metric, n_threads=8)

    def expect_search(self, queries, k, note_use=True):
        if self.search_refused():
            return UNSUPPORTED, None
        if self.allow is None:
            return OK, self.plain(queries, k)
        if note_use:
            self.filter_used = True
        return OK, rgh.expected(self.oracle, self.rows, queries, k, self.allow, ip=self._ip())

    def tiers(self, query_groups):
        """how the header says a grouped batch is served: (list, filter, any, pad) queries"""
        limit = self.options.get("group_list_rows", 0) or GROUP_LIST_ROWS_AUTO
        out = dict(list=0, filter=0, any=0, pad=0)
        for x in np.asarray(query_groups, dtype=np.uint32):
            s = 0 if x == ANY else int((self.labels == x).sum())
            out["any" if x == ANY else "pad" if s == 0 else "list" if s <= limit else "filter"] += 1
        return out

    def expect_grouped(self, queries, query_groups, k):
        if self.search_refused():
            return None, None     # (not specified: the driver does not ask)
        if self.labels is None:
            return NOT_BUILT, None
        if self.allow is not None:
            self.tags.append("refuse_grouped_filter")
            return UNSUPPORTED, None
        self.last_tiers = self.tiers(query_groups)
        return OK, rgh.expected_grouped(self.oracle, self.rows, self.labels, queries, query_groups, k, ip=self._ip())

    def range_radii(self, queries):
        """query i: the exact bits of its t-th distance, t cycling over 1, 10, 100; every sixth: just below its nearest"""
        ref = self.plain(queries, self.n)
        ts = (1, 10, 100)
        r = np.array([ref[1][i, min(ts[i % 3], self.n) - 1] for i in range(queries.shape[0])], np.float32)
        r[::6] = np.nextafter(ref[1][::6, 0], np.float32(-np.inf))
        return r

    def expect_range(self, queries, radii, max_results, rows_mask=None):
        if not float_rows(self.cfg):
            self.tags.append("refuse_range_8bit")
            return UNSUPPORTED, None
        if self.allow is not None:
            self.tags.append("refuse_range_filter")
            return UNSUPPORTED, None
        if self.search_refused():
            return None, None
        if rows_mask is None:
            return OK, range_expected(self.plain(queries, self.n), radii, max_results)
        idx = np.flatnonzero(rows_mask)
        rids, rd = self.plain(queries, idx.size, np.ascontiguousarray(self.rows[idx]))
        return OK, range_expected((idx.astype(np.uint64)[rids.astype(np.int64)], rd), radii, max_results)

    def score_case(self, j):
        """the ids a score_ids check asks for, descending: the newest rows, two old ones and a stride through the index"""
        n = self.n
        return np.unique(np.concatenate([np.arange(max(0, n - 45), n), [0, min(5, n - 1)],
                                         np.arange(j % 37, n, 37)])).astype(np.uint64)[::-1].copy()

    def expect_score(self, query, ids, cutoff=None, rows=None):
        """(cutoff, (kept ids, kept scores)); without a cutoff: the median score, so that about half are kept"""
        rows = self.rows if rows is None else rows
        if cutoff is None:
            _, sc = self.oracle.filter_by_score(rows, query, ids, float("inf"), self.metric)
            cutoff = float(np.median(sc))
        return cutoff, self.oracle.filter_by_score(rows, query, ids, cutoff, self.metric)


# ---- the generator -----------------------------------------------------------------------------------------------
def _data(cfg, rng, n):
    """n rows of the config's kind, as the engine's store calls take them"""
    if cfg.data == "gauss":
        return np.clip(rng.standard_normal((n, cfg.d)) * 0.4, -1.4, 1.4).astype(np.float32)
    if cfg.data in ("int255", "u8"):
        return rng.randint(0, 256, size=(n, cfg.d)).astype(np.float32 if cfg.data == "int255" else np.uint8)
    return rng.randint(-127, 128, size=(n, cfg.d)).astype(np.int8)


def _queries(cfg, rng):
    if cfg.data == "gauss":
        return (rng.standard_normal((M, cfg.d)) * 0.4).astype(np.float32)
    if cfg.data in ("int255", "u8"):
        return rng.randint(0, 256, size=(M, cfg.d)).astype(np.float32)
    return rng.randint(-127, 128, size=(M, cfg.d)).astype(np.int8)


def _near(cfg, rng, queries, which):
    """a near copy of each query in `which`: the query plus small noise, in the rows' type"""
    q = queries[which].astype(np.float64)
    if cfg.data == "gauss":
        return np.clip(q + 0.01 * rng.standard_normal(q.shape), -1.4, 1.4).astype(np.float32)
    lo, hi = (0, 255) if cfg.data in ("int255", "u8") else (-127, 127)
    out = np.clip(q + rng.randint(-2, 3, size=q.shape), lo, hi)
    return out.astype({"int255": np.float32, "u8": np.uint8, "i8": np.int8}[cfg.data])


BIG = {"gauss": 3.3, "int255": 600.5}   # a value at least twice the index's max |v| (1.5, 255): the fp16 scale changes


def initial(cfg, seed):
    """(rows, queries) a sequence starts from; gauss rows: max |v| = 1.5 sits in row 10 alone"""
    cfg = resolve(cfg, seed)
    rng = np.random.RandomState(1000 * (ord(cfg.name) - 64) + seed)
    rows, queries = _data(cfg, rng, N0), _queries(cfg, rng)
    if cfg.data == "gauss":
        rows[10, 5] = 1.5
    for a in (rows, queries):
        a.setflags(write=False)
    return rows, queries


def describe(op):
    o = op["op"]
    if o == "append":
        return "append(%d rows%s)" % (op["rows"].shape[0], ", device" if op.get("device") else "")
    if o == "remove":
        return "remove(%d ids%s)" % (op["ids"].size, ", device" if op.get("device") else "")
    if o == "reserve":
        return "reserve(%d)" % op["n"]
    if o == "set_filter":
        return "set_filter(%d allowed)" % int(op["allow"].sum()) if op["allow"] is not None else "clear_filter"
    if o == "set_groups":
        return "set_groups" if op["labels"] is not None else "clear_groups"
    if o == "option":
        return "option(%s=%d)" % (op["name"], op["value"])
    if o in ("search", "grouped", "range", "score"):
        return "%s(m=%d, k=%d)" % (o, op["m"], op["k"])
    return o


MUTATIONS = ("append", "remove", "reserve", "compact", "set_filter", "set_groups", "option")


@functools.lru_cache(maxsize=None)
def _generate(name, seed):
    import oracle_ctypes as oracle
    cfg = resolve(name, seed)
    rows0, queries = initial(name, seed)
    rng = np.random.RandomState(7919 * (ord(cfg.name) - 64) + 31 * seed + 5)
    model = Model(oracle, cfg, rows0)
    flt = float_rows(cfg)
    deferred = CONFIGS[name].async_seed == seed
    ops = []

    def mk():
        return dict(m=MS[rng.randint(3)], k=KS[rng.randint(3)])

    def push(op):
        """add the operation and carry it out on the model, so that the next one is drawn from the state it leaves"""
        op = dict(mk(), **op)
        ops.append(op)
        o = op["op"]
        if o == "append":
            model.append(op["rows"])
        elif o == "remove":
            model.remove(op["ids"])
        elif o == "reserve":
            model.reserve(op["n"])
        elif o == "compact":
            model.compact_row_filter()
        elif o == "set_filter":
            model.set_row_filter(op["allow"])
        elif o == "set_groups":
            model.set_row_groups(op["labels"])
        elif o == "option":
            model.set_option(op["name"], op["value"])
        if o in MUTATIONS or o == "search":
            model.expect_search(queries[:1], 1)    # (the driver searches after every mutation: a filter counts as used)

    def third():
        return rng.choice(M, 50, replace=False)    # (a third is 44: a few to spare for near copies that coincide)

    def append(n_total, big=False, to_tile=None, fraction=False):
        """n_total rows, 50 of them near copies of queries; to_tile: True ends on a 128-row tile, False inside one;
        big: one row carries a value twice the index's max |v|; fraction: one row is no integer"""
        if to_tile is True:
            n_total += (-(model.n + n_total)) % TILE
        elif to_tile is False and (model.n + n_total) % 64 == 0:   # (inside a 64-row tile too: the 8-bit forms' tile)
            n_total += 37
        new = _data(cfg, rng, n_total)
        at = rng.choice(n_total, 50, replace=False)
        new[at] = _near(cfg, rng, queries, third())
        if big:
            spare = np.setdiff1d(np.arange(n_total), at)
            new[spare[0], 7] = BIG[cfg.data]
        if fraction:
            new[np.setdiff1d(np.arange(n_total), at)[1], 3] = 17.5
        new.setflags(write=False)
        push(dict(op="append", rows=new, device=deferred, deferred=deferred))

    def nearest_ids(extra):
        """the current nearest row of a third of the queries, `extra` random rows, a few of them twice"""
        top = model.plain(np.ascontiguousarray(queries[third()]), 1)[0][:, 0]
        more = rng.choice(model.n, extra, replace=False).astype(np.uint64)
        ids = np.concatenate([top, more, more[:7]])
        return ids[rng.permutation(ids.size)]

    def remove(extra, also=None, keep_max=True):
        ids = nearest_ids(extra)
        if flt and keep_max:   # (the row that carries max |v| stays unless the step is about it)
            ids = ids[~np.isin(ids, carriers().astype(np.uint64))]
        if also is not None:
            ids = np.concatenate([ids, np.asarray(also, dtype=np.uint64)])
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        ids.setflags(write=False)
        push(dict(op="remove", ids=ids, device=deferred, deferred=deferred))

    def density():
        return float(np.exp(rng.uniform(np.log(0.01), np.log(0.6))))

    def carriers():
        """the rows that carry the index's max |v| -- none where many rows share it (integer rows at 255)"""
        at = np.flatnonzero(np.abs(model.rows).max(axis=1) == np.abs(model.rows).max())
        return at if at.size <= 4 else at[:0]

    def set_filter(p=None, allow=None, clear=False):
        if clear:
            push(dict(op="set_filter", allow=None))
            return
        if allow is None:
            allow = rng.rand(model.n) < (density() if p is None else p)
            allow[carriers()] = True   # (the row that carries max |v| goes in the step that is about it)
        allow.setflags(write=False)
        push(dict(op="set_filter", allow=allow))

    def set_groups(p=None):
        """label 3 on a share p of the rows, 2 % of the rows in no group, the rest spread over three labels"""
        p = density() if p is None else p
        u = rng.rand(model.n)
        labels = np.asarray([7, 100, 2 ** 31 + 5], np.uint32)[rng.randint(0, 3, model.n)]
        labels[u < p] = 3
        labels[u > 0.98] = ANY
        labels.setflags(write=False)
        push(dict(op="set_groups", labels=labels))

    def read(kind, **mk_):
        push(dict(op=kind, **mk_))

    def batch():
        read("search", m=M, k=10)   # (a batch of 130 queries: the shape the matrix-core forms and their copies serve)

    def option(name, value):
        push(dict(op="option", name=name, value=value))

    B = CONFIGS[name].options
    read("search")
    if B:
        option("i8_filter", 2)
        option("i8_sample", 2)
        read("search")
    if not flt:
        # 8-bit rows: the filter, the groups and the range search are refused, and the handle answers as before
        set_filter()
        set_groups()
        read("range")
    append(300 + rng.randint(0, 100), to_tile=True)        # crosses 4 096 rows upward, ends on a tile, grows the capacity
    read("score")
    if flt:
        set_filter()
        read("search")
        read("range")                                       # refused under the filter
        set_groups()
        read("grouped")                                     # refused under the filter
    if B:
        option("scan_kernel", 1)
    remove(40 + rng.randint(0, 60))                         # follows a filter that was set and used
    if flt:
        set_groups()
        read("grouped")
    if B:
        option("group_list_rows", 64)                       # the larger groups take the filter tier
        read("grouped")
        option("scan_kernel", 2)                            # float rows have no such form: the search is refused
        option("scan_kernel", 3)
    append(200 + rng.randint(0, 200), to_tile=False)        # ends inside a tile
    read("range")
    push(dict(op="reserve", n=7000 + rng.randint(0, 500)))
    if B:
        option("scan_kernel", 4)
        option("sample_pass", 0)
    append(300 + rng.randint(0, 300), big=flt, to_tile=False)   # within the reserve; float rows: the scale changes
    read("search")
    read("score")
    push(dict(op="compact"))                                # no filter in force: refused
    if flt:
        set_filter(allow=np.zeros(model.n, dtype=bool))
        push(dict(op="compact"))                            # allows no row: refused, the filter stays
        set_filter(p=rng.uniform(0.3, 0.6))
        read("search")
        push(dict(op="compact"))                            # crosses 4 096 rows downward
        set_groups()
        read("grouped")
    else:
        remove(model.n - DIRECT_BELOW + 150 + rng.randint(0, 300))   # crosses 4 096 rows downward
    if B:
        option("scan_kernel", 0)
        option("sample_pass", 1)
    bad = np.array([3, model.n, 9], dtype=np.uint64)
    push(dict(op="remove", ids=bad))                        # an id at the size: refused
    push(dict(op="remove", ids=np.arange(model.n, dtype=np.uint64)))   # every row: refused
    append(2500 + rng.randint(0, 500), to_tile=False)       # back above 4 096 rows, within the capacity or past it
    read("range")
    if flt:
        carrier = carriers()
        set_filter()
        read("search")
        remove(30 + rng.randint(0, 40), also=carrier, keep_max=False)   # the row that carries max |v| goes
        read("score")
        set_groups()
        read("grouped")
    if B:
        option("group_list_rows", 0)
    append(2500 + rng.randint(0, 1000), to_tile=False)      # a second growth of the capacity
    read("search")
    remove(200 + rng.randint(0, 200))
    read("range")
    read("score")
    if B:
        # past 32 768 rows "i8_filter" 2 builds the int8 filter's set; every change of rows forgets it
        append(I8_MIN_ROWS - model.n + 600 + rng.randint(0, 800), to_tile=False)
        batch()
        option("sample_pass", 0)
        batch()
        option("sample_pass", 1)
        remove(250 + rng.randint(0, 100))
        batch()
        append(150 + rng.randint(0, 100), to_tile=True)
        read("search", m=M, k=100)
        set_filter()                                        # a filtered search never takes the int8 filter
        batch()
        set_filter(allow=None, clear=True)
        batch()
    if cfg.data == "int255":
        # past 65 536 integer rows the uint8 shadow serves batches of integer queries; a fractional row ends that,
        # its removal allows it again
        append(U8_SHADOW_ROWS - model.n + 700 + rng.randint(0, 800), to_tile=False)
        batch()
        append(100 + rng.randint(0, 100), fraction=True)
        batch()
        odd = np.flatnonzero((model.rows != np.floor(model.rows)).any(axis=1))
        remove(100 + rng.randint(0, 100), also=odd)
        batch()
        read("range", m=7)
    if not flt:
        # past 32 768 rows "scan_kernel" 5 serves 8-bit rows from per-wave hit queues over an int8 operand: a copy for
        # uint8 rows and for a row count inside a 64-row tile, else the base itself (seed 2 keeps whole tiles)
        whole = seed == 2
        option("scan_kernel", 5)
        append(I8_MIN_ROWS - model.n + 500 + rng.randint(0, 500), to_tile=whole)   # the capacity becomes the row count
        batch()
        append(256 + 128 * rng.randint(0, 3), to_tile=whole)                       # so this append reallocates
        batch()
        push(dict(op="reserve", n=model.n + 4000))                                 # moves the base, forgets nothing
        batch()
        remove(250 + rng.randint(0, 100))
        batch()
    return tuple(ops)


def generate(config, seed):
    """the operations of (config, seed): a list of dicts, each with "op", the (m, k) of the step's search check and the
    operation's own arguments (read-only arrays).  Deterministic: the same list for the same arguments."""
    name = config if isinstance(config, str) else config.name
    return list(_generate(name, int(seed)))


def replay(config, seed, upto):
    """the operations up to and including step `upto`: what a failure message names"""
    return generate(config, seed)[:upto + 1]


# ---- the driver --------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _call(fn, *args, **kw):
    """(status, result) of an engine call: a refusal is an exception that carries the status code"""
    try:
        return OK, fn(*args, **kw)
    except Exception as e:  # noqa: BLE001 (ExpannError and Refused both carry .code)
        if not hasattr(e, "code"):
            raise
        return e.code, None


def _same_topk(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: ids differ in rows %s" % (
        what, np.flatnonzero((got[0] != want[0]).any(axis=1))[:8])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "%s: distance bits differ" % what


QUERY_GROUPS = np.asarray([3, 7, 100, 2 ** 31 + 5, ANY, 999], np.uint32)[np.arange(M) % 6]


class Driver:
    def __init__(self, engine, model, queries, device=None, log=None):
        self.e, self.model, self.q = engine, model, queries
        self.device = device      # the GPU tests' adapter for device buffers and streams, or None
        self.turn = 0
        self.status, self.own_tags = OK, ()   # of the last mutation
        self.log = log if log is not None else []

    # ---- reads ------------------------------------------------------------------------------------------------
    def check_search(self, m, k):
        q = np.ascontiguousarray(self.q[:m])
        want_rc, want = self.model.expect_search(q, k)
        rc, got = _call(self.e.query_k_batch, q, k)
        assert rc == want_rc, "search(m=%d, k=%d): status %d, expected %d" % (m, k, rc, want_rc)
        if rc == OK:
            _same_topk(got, want, "search(m=%d, k=%d)" % (m, k))

    def check_grouped(self, m, k):
        q, qg = np.ascontiguousarray(self.q[:m]), np.ascontiguousarray(QUERY_GROUPS[:m])
        want_rc, want = self.model.expect_grouped(q, qg, k)
        if want_rc is None:
            return
        rc, got = _call(self.e.query_k_batch, q, k, groups=qg)
        assert rc == want_rc, "grouped search(m=%d, k=%d): status %d, expected %d" % (m, k, rc, want_rc)
        if rc == OK:
            _same_topk(got, want, "grouped search(m=%d, k=%d)" % (m, k))
            tiers = {t: self.e.get_stat("group_%s_queries" % t) for t in ("list", "filter", "any", "pad")}
            assert tiers == self.model.last_tiers, "grouped search: tiers %s, expected %s" % (tiers, self.model.last_tiers)

    def check_range(self, m, k):
        q = np.ascontiguousarray(self.q[:m]).astype(np.float32)
        radii = self.model.range_radii(self.q[:m]) if float_rows(self.model.cfg) else np.ones(m, np.float32)
        want_rc, want = self.model.expect_range(self.q[:m], radii, RANGE_MAX_RESULTS)
        if want_rc is None:
            return
        rc, got = _call(self.e.range_search, q, radii, RANGE_MAX_RESULTS)
        assert rc == want_rc, "range search(m=%d): status %d, expected %d" % (m, rc, want_rc)
        if rc == OK:
            assert np.array_equal(got[2], want[2]), "range search(m=%d): counts differ at %s" % (
                m, np.flatnonzero(got[2] != want[2])[:8])
            _same_topk(got[:2], want[:2], "range search(m=%d)" % m)

    def check_score(self, m, k):
        j = (m * 31 + k) % M
        ids = self.model.score_case(j)
        cutoff, (wkept, wsc) = self.model.expect_score(self.q[j], ids)
        rc, got = _call(self.e.score_ids, self.q[j], ids, cutoff)
        assert rc == OK, "score_ids: status %d" % rc
        assert np.array_equal(got[0], wkept), "score_ids(query %d): kept ids differ" % j
        assert np.array_equal(_bits(got[1]), _bits(wsc)), "score_ids(query %d): score bits differ" % j

    def check_other(self, m, k):
        """one more entry point, taken in turn"""
        kinds = ("grouped", "range", "score") if float_rows(self.model.cfg) else ("range", "score")
        kind = kinds[self.turn % len(kinds)]
        self.turn += 1
        getattr(self, "check_" + kind)(m, k)

    def check_stats(self, before, op):
        cap, re = self.e.get_stat("base_capacity_rows"), self.e.get_stat("base_reallocs")
        assert cap >= before[0], "base_capacity_rows fell from %d to %d" % (before[0], cap)
        if op["op"] in ("remove", "compact"):
            assert (cap, re) == before[:2], "a remove changed (base_capacity_rows, base_reallocs) %s -> %s" % (
                before[:2], (cap, re))
        if op["op"] == "append" and before[2] + op["rows"].shape[0] <= before[0]:
            assert (cap, re) == before[:2], "an append within the capacity reallocated: %s -> %s" % (before[:2], (cap, re))
        assert (cap, re) == (self.model.capacity, self.model.reallocs), \
            "(base_capacity_rows, base_reallocs) = %s, the rules give %s" % ((cap, re), (self.model.capacity,
                                                                                          self.model.reallocs))

    # ---- one operation ---------------------------------------------------------------------------------------------
    def mutate(self, op):
        """carry the mutation out on the engine and on the model; their status codes must agree"""
        o, e, mod = op["op"], self.e, self.model
        dev = self.device if op.get("device") else None
        if o == "append":
            rc, _ = _call(dev.append if dev else e.append, *((e, op["rows"]) if dev else (op["rows"],)))
            want = mod.append(op["rows"])
        elif o == "remove":
            rc, removed = _call(dev.remove if dev else e.remove, *((e, op["ids"]) if dev else (op["ids"],)))
            want = mod.remove(op["ids"])
            if rc == OK == want:
                assert removed == np.unique(op["ids"]).size, "remove: %d rows reported" % removed
        elif o == "reserve":
            rc, _ = _call(e.reserve, op["n"])
            want = mod.reserve(op["n"])
        elif o == "compact":
            n0 = mod.n
            rc, removed = _call(e.compact_row_filter)
            want = mod.compact_row_filter()
            if rc == OK == want:
                assert removed == n0 - mod.n, "compact_row_filter: %d rows reported, %d expected" % (removed, n0 - mod.n)
        elif o == "set_filter":
            rc, _ = _call(e.set_row_filter, op["allow"])
            want = mod.set_row_filter(op["allow"])
        elif o == "set_groups":
            rc, _ = _call(e.set_row_groups, op["labels"])
            want = mod.set_row_groups(op["labels"])
        else:
            rc, _ = _call(e.set_option, op["name"], op["value"])
            want = mod.set_option(op["name"], op["value"])
        assert rc == want, "%s: status %d, expected %d" % (describe(op), rc, want)
        # what the mutation itself returned and was, before any check reads through the model
        self.status, self.own_tags = want, tuple(mod.tags)

    def step(self, op):
        o, m, k = op["op"], op["m"], op["k"]
        if o in ("search", "grouped", "range", "score"):
            getattr(self, "check_" + o)(m, k)
            return
        before = (self.e.get_stat("base_capacity_rows"), self.e.get_stat("base_reallocs"), self.model.n)
        pending = None
        if op.get("deferred") and self.device is not None and not self.model.search_refused():
            # searches enqueued, then the mutation, then sync: they answer over the rows before the mutation
            q = np.ascontiguousarray(self.q[:m])
            want = [self.model.expect_search(q, kk)[1] for kk in (k, 10)]
            pending = self.device.enqueue(self.e, q, (k, 10))
        self.mutate(op)
        if pending is not None:
            for kk, got, w in zip((k, 10), self.device.collect(self.e, pending), want):
                _same_topk(got, w, "deferred search(m=%d, k=%d) enqueued before %s" % (m, kk, describe(op)))
        assert self.e.size() == self.model.n, "size() = %d, expected %d" % (self.e.size(), self.model.n)
        self.check_stats(before, op)
        self.check_search(m, k)
        self.check_other(m, k)


def run(engine, model, ops, oracle=None, queries=None, device=None, config="?", seed=-1, log=None, after_step=None):
    """Drive `engine` and `model` through `ops`, checking after every step.  `queries`: the sequence's 130 queries;
    `device`: an adapter with append / remove / enqueue / collect for the steps marked for device buffers (None: the
    host calls serve them and nothing is deferred); `log`: a list that receives (step, description) as steps pass;
    `after_step(i, op, driver)` is called after each step that passed.  `oracle` is the model's (kept in the
    signature so that a caller names the arithmetic it trusts)."""
    assert oracle is None or oracle is model.oracle
    drv = Driver(engine, model, queries, device, log)
    for i, op in enumerate(ops):
        model.tags = []
        try:
            drv.step(op)
        except AssertionError as err:
            prefix = "\n".join("  %2d %s" % (j, describe(p)) for j, p in enumerate(ops[:i + 1]))
            raise AssertionError("config %s seed %d step %d, %s: %s\nthe operations up to it, "
                                 "bf_sequence_model.replay(%r, %d, %d):\n%s" % (config, seed, i, describe(op), err, config,
                                                                                seed, i, prefix)) from None
        drv.log.append((i, describe(op)))
        if after_step:
            after_step(i, op, drv)
    return drv


def _top10(model, q, kind):
    """(status, distance bits) of the model's expected top-10 over all 130 queries, without a trace in the model"""
    saved = (list(model.tags), model.last_tiers, model.filter_used)
    if kind == "rows":
        out = OK, model.plain(q, 10)
    elif kind == "filter":
        out = model.expect_search(q, 10, note_use=False)
    elif model.labels is None:
        out = OK, model.plain(q, 10)
    else:   # (the labelling itself: whether a filter in force makes the grouped search a refusal is not the point)
        out = OK, rgh.expected_grouped(model.oracle, model.rows, model.labels, q, QUERY_GROUPS, 10, ip=model._ip())
    model.tags, model.last_tiers, model.filter_used = saved
    return out[0], None if out[1] is None else _bits(out[1][1])


SENSITIVE = {"append": "rows", "remove": "rows", "compact": "rows", "set_filter": "filter", "set_groups": "groups"}


@functools.lru_cache(maxsize=None)
def simulate(name, seed):
    """The sequence driven against a FakeEngine (which must pass), with what the CPU conditions read: per step a dict
    of the operation, the tags of what happened (the coverage conditions) and, for an ACCEPTED mutation of the rows, the
    filter or the labels, `changed`: for how many of the 130 queries the expected top-10 distances differ from those
    before it.  Rows are compared without the filter (an append and a remove clear it: that alone would change every
    answer), a filter change under the filter, a labelling as the grouped answers over the new labels against those
    over the labels before it (none: the ungrouped answers), so that it is the labelling that is judged and not the
    status code.  `status` is what the mutation itself returned and `own_tags` what it was, both taken before the
    driver's checks read through the model.  A reserve, an option and a refused call must change no answer, which the
    driver checks; they have no `changed`."""
    import oracle_ctypes as oracle
    cfg = resolve(name, seed)
    rows, queries = initial(name, seed)
    model = Model(oracle, cfg, rows)
    fake = FakeEngine(oracle, cfg, rows)
    drv = Driver(fake, model, queries)
    out = []
    for i, op in enumerate(generate(name, seed)):
        kind = SENSITIVE.get(op["op"])
        before = _top10(model, queries, kind) if kind else None
        n0 = model.n
        model.tags = []
        drv.step(op)
        mutation = op["op"] in MUTATIONS
        rec = dict(i=i, op=op["op"], what=describe(op), tags=tuple(model.tags), n0=n0, n1=model.n, changed=None,
                   status=drv.status if mutation else None, own_tags=drv.own_tags if mutation else ())
        if kind and rec["status"] == OK:
            after = _top10(model, queries, kind)
            if before[1] is None or after[1] is None:
                rec["changed"] = M if before != after else 0
            else:
                rec["changed"] = int((before[1] != after[1]).any(axis=1).sum())
        out.append(rec)
    return tuple(out)


# ---- the engine's interface over a Model, and its stale variants ------------------------------------------------------
class FakeEngine:
    def __init__(self, oracle, cfg, rows):
        self.m = Model(oracle, cfg, rows)
        self.appended = np.zeros(self.m.n, dtype=bool)

    def _do(self, rc, value=None):
        if rc != OK:
            raise Refused(rc)
        return value

    def size(self):
        return self.m.n

    def append(self, rows):
        rc = self.m.append(rows)
        if rc == OK:
            self.appended = np.concatenate([self.appended, np.ones(len(rows), dtype=bool)])
        self._do(rc)

    def reserve(self, n):
        self._do(self.m.reserve(n))

    def _removed(self, gone):
        self.appended = np.delete(self.appended, gone)

    def remove(self, ids):
        rc = self.m.remove(ids)
        if rc == OK:
            self._removed(np.unique(np.asarray(ids, dtype=np.uint64)).astype(np.int64))
        return self._do(rc, np.unique(ids).size)

    def compact_row_filter(self):
        n0, allow = self.m.n, self.m.allow
        rc = self.m.compact_row_filter()
        if rc == OK:
            self._removed(np.flatnonzero(~allow))
        return self._do(rc, n0 - self.m.n)

    def set_row_filter(self, allow):
        self._do(self.m.set_row_filter(allow))

    def set_row_groups(self, labels):
        self._do(self.m.set_row_groups(labels))

    def set_option(self, name, value):
        self._do(self.m.set_option(name, value))

    def query_k_batch(self, queries, k, groups=None):
        if groups is None:
            rc, out = self.m.expect_search(queries, k)
        else:
            rc, out = self.m.expect_grouped(queries, groups, k)
        return self._do(rc, out)

    def range_search(self, queries, radius, max_results):
        rc, out = self.m.expect_range(queries, radius, max_results)
        return self._do(rc, out)

    def score_ids(self, query, ids, cutoff=float("inf")):
        return self.m.expect_score(query, ids, cutoff)[1]

    def get_stat(self, name):
        if name == "base_capacity_rows":
            return self.m.capacity
        if name == "base_reallocs":
            return self.m.reallocs
        if name.startswith("group_") and name.endswith("_queries"):
            return self.m.last_tiers[name[6:-8]]
        raise KeyError(name)


class StaleRange(FakeEngine):
    """range_search answers from the rows that were there at build: it ignores every append"""

    def range_search(self, queries, radius, max_results):
        rc, out = self.m.expect_range(queries, radius, max_results, rows_mask=~self.appended)
        return self._do(rc, out)


class StaleFilter(FakeEngine):
    """a remove keeps the filter (compacted with the rows) instead of clearing it"""

    def remove(self, ids):
        allow = self.m.allow
        removed = super().remove(ids)
        if allow is not None:
            self.m.allow = np.delete(allow, np.unique(np.asarray(ids, dtype=np.uint64)).astype(np.int64))
        return removed


class StaleScore(FakeEngine):
    """score_ids reads the rows in the numbering from before the last remove"""
    before = None

    def remove(self, ids):
        rows = self.m.rows
        removed = super().remove(ids)
        self.before = rows
        return removed

    def append(self, rows):
        super().append(rows)
        self.before = None

    def score_ids(self, query, ids, cutoff=float("inf")):
        return self.m.expect_score(query, ids, cutoff, rows=self.before)[1]


class StaleOption(FakeEngine):
    """ "group_list_rows" is accepted and forgotten: the tiers stay those of the default"""

    def set_option(self, name, value):
        if name != "group_list_rows":
            super().set_option(name, value)


STALE_FAKES = (StaleRange, StaleFilter, StaleScore, StaleOption)
