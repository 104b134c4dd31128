"""Hand-laid column batches for the groupbytrace store (tests/test_gbt_layouts.py).

Three things, all numpy / Python and none of them the C++:

* Batch / lay(): one add's `native.Columns` built from numpy arrays (host
  pointers; DeviceBatch uploads it): ids as (hi, lo) pairs, a free scope[i],
  an arena with route, path, string attribute values and queries of chosen
  lengths, every optional column switchable to NULL.
* Store: a column-level restatement of the store's documented semantics
  (the header comment of gbt_kernel.hip) with dicts and lists:
  what a release holds, in which order, with which refs and arena bytes, the
  refusals and the eight stats() values.  tests/gbt_ref.py stays the Go-level
  restatement; test_gbt_layouts.py checks the two against each other.
* Census: the host's bookkeeping restated (ring positions, the id table's
  slots / epoch / claimed slots, the release's seq range and sort bits), so
  that a layout can say which seam each step hits.  On the GPU every step
  compares it with osehost_gbt_state, so the policy restated here is not
  trusted either.

The constants a layout is laid against are parsed from the sources at import
(K); DESIGNED pins the values the layouts were drawn for.  Test
infrastructure only.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from odigos_amd import native

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
M64 = (1 << 64) - 1
SEC = 1_000_000_000
T0 = 1_700_000_000_000_000_000
STATS = ("waiting_traces", "held_spans", "created", "released", "evicted", "released_spans", "added_spans",
         "held_bytes")
STATE = ("table_slots", "epoch", "slots_used", "pool_begin", "pool_end", "scope_begin", "scope_end", "arena_begin",
         "arena_end", "next_seq", "rel_end", "epochs", "n_attrsets")


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    hpp = (CSRC / "kernels.hpp").read_text()
    hip = (CSRC / "gbt_kernel.hip").read_text()
    host = (CSRC / "gbt_host.cpp").read_text()

    def const(text, name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name}: definition not found"
        return int(m.group(1))

    def one(pattern, what):
        m = re.search(pattern, host)
        assert m, f"gbt_host.cpp: {what} changed; tests/gbt_layouts.py must follow it"
        return [int(x) for x in m.groups()]

    k = SimpleNamespace()
    k.kGbtThreads = const(hip, "kGbtThreads")
    k.kScanTileItems = const(hpp, "kScanTileItems")
    k.kSortTile = const(hpp, "kSortTile")
    k.pool_floor, = one(r"g->pool_cap = std::max<uint64_t>\(span_capacity, (\d+)\);", "the span capacity floor")
    shift, = one(r"g->arena_cap = std::max<uint64_t>\(arena_capacity, 1 << (\d+)\);", "the arena capacity floor")
    k.arena_floor = 1 << shift
    one(r"g->scope_cap = g->pool_cap;", "the scope ring's capacity")
    k.table_floor, k.table_factor = one(r"uint64_t slots = (\d+);\s*while \(slots < (\d+) \* \(live \+ n\)\) slots <<= 1;",
                                        "the id table's sizing")
    k.rebuild_div, = one(r"g->slots_used \+ n > g->table_slots / (\d+);", "the id table's rebuild rule")
    return k


K = _parse_constants()
DESIGNED = dict(kGbtThreads=256, kScanTileItems=1024, kSortTile=4096, pool_floor=1024, arena_floor=1 << 16,
                table_floor=1024, table_factor=4, rebuild_div=2)


# ---------------------------------------------------------------------------
# hashes (trace_device.hpp tid_hash; contrib's workerIndexForTraceID)

def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tid_hash(hi: int, lo: int) -> int:
    return splitmix64(hi ^ splitmix64(lo))


def _splitmix64_np(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def ids_for_slot(slot: int, mask: int, count: int, seed: int, hi: int = 0x51D) -> list:
    """`count` ids (hi, lo) with tid_hash & mask == slot: a search over lo from seed << 32."""
    out, base = [], seed << 32
    while len(out) < count:
        lo = np.arange(base, base + (1 << 16), dtype=np.uint64)
        h = _splitmix64_np(np.uint64(hi) ^ _splitmix64_np(lo)) & np.uint64(mask)
        out += [(hi, int(x)) for x in lo[h == np.uint64(slot)]]
        base += 1 << 16
    out = out[:count]
    assert all(tid_hash(h, l) & mask == slot for h, l in out)
    return out


def worker_of(hi: int, lo: int, W: int) -> int:
    """FNV-1 (64-bit) over the id's 16 big-endian bytes, modulo the workers"""
    h = 0xCBF29CE484222325
    for b in hi.to_bytes(8, "big") + lo.to_bytes(8, "big"):
        h = (h * 0x100000001B3) & M64
        h ^= b
    return h % W


def tid(k: int) -> tuple:
    """the suite's id number k (never zero, hi and lo both varied)"""
    return (splitmix64(k) | 1, k + 1)


def ids_for_worker(w: int, W: int, count: int, start: int = 1 << 20) -> list:
    out, k = [], start
    while len(out) < count:
        if worker_of(*tid(k), W) == w:
            out.append(tid(k))
        k += 1
    return out


# ---------------------------------------------------------------------------
# one add's columns

SPAN_OPTIONAL = ("url_flags", "span_size", "name_len", "attr_match", "route", "path")
RES_OPTIONAL = ("res_svc_str", "res_url_ok", "res_size", "scope_size")
ALL_OPTIONAL = SPAN_OPTIONAL + RES_OPTIONAL
_FIELDS = ("arena", "trace_id", "start_ns", "end_ns", "status", "kind", "resource", "scope", "url_flags", "path", "route",
           "span_size", "name_len", "attr_match", "res_svc", "res_svc_str", "res_url_ok", "res_attrset", "res_size",
           "scope_size", "scope_resource", "attr_type", "attr_val", "db_flags", "db_query", "res_sql_ok")


class Batch:
    """Columns of one add as numpy arrays named like ose_columns (None = NULL)."""

    def __init__(self, **kw):
        for f in _FIELDS:
            setattr(self, f, None)
        self.attrset_map = None
        self.__dict__.update(kw)
        self._keep = None
        self._lay = {}

    def columns(self) -> native.Columns:
        c = native.Columns()
        c.n_spans, c.n_resources, c.n_scopes, c.n_attrsets = self.n, self.R, self.S, self.A
        c.n_attr_keys, c.attr_match_words, c.arena_bytes = self.K, self.words, self.arena_bytes
        self._keep = {}
        for f in _FIELDS:
            a = getattr(self, f)
            if a is not None:
                a = np.ascontiguousarray(a)
                self._keep[f] = a
                setattr(c, f, a.ctypes.data)
        return c

    @staticmethod
    def from_columns(c: native.Columns) -> "Batch":
        """a copy of host columns (the host columniser's)"""
        n, R, S, Kk = c.n_spans, c.n_resources, c.n_scopes, c.n_attr_keys
        words = max(1, c.attr_match_words)

        def arr(name, cnt, dt):
            p = getattr(c, name)
            if not p:
                return None
            nb = cnt * np.dtype(dt).itemsize
            if nb == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array((C.c_uint8 * nb).from_address(p)).view(dt).copy()

        b = Batch(n=n, R=R, S=S, A=c.n_attrsets, K=Kk, words=words, arena_bytes=c.arena_bytes)
        arena = arr("arena", c.arena_bytes, np.uint8)
        b.arena = np.concatenate([arena if arena is not None else np.zeros(0, np.uint8), np.zeros(48, np.uint8)])
        b.trace_id = arr("trace_id", 2 * n, np.uint64).reshape(n, 2)
        for name, cnt, dt in (("start_ns", n, np.uint64), ("end_ns", n, np.uint64), ("status", n, np.uint8),
                              ("kind", n, np.uint8), ("resource", n, np.uint32), ("scope", n, np.uint32),
                              ("url_flags", n, np.uint8), ("span_size", n, np.uint32), ("name_len", n, np.uint32),
                              ("attr_match", words * n, np.uint64), ("res_svc", R, np.uint32),
                              ("res_svc_str", R, np.uint32), ("res_url_ok", R, np.uint8), ("res_attrset", R, np.uint32),
                              ("res_size", R, np.uint32), ("scope_size", S, np.uint32), ("scope_resource", S, np.uint32),
                              ("attr_type", Kk * n, np.uint8), ("attr_val", Kk * n, np.uint64), ("db_flags", n, np.uint8),
                              ("res_sql_ok", R, np.uint8)):
            setattr(b, name, arr(name, cnt, dt))
        for name in ("route", "path", "db_query"):
            a = arr(name, 2 * n, np.uint32)
            setattr(b, name, None if a is None else a.reshape(n, 2))
        return b

    def layout(self, sql: bool) -> SimpleNamespace:
        """Each span's string block as the store lays it: route, path, the
        string attribute values in key order, then (sql) the query.  Offsets
        are relative to the block."""
        if sql in self._lay:
            return self._lay[sql]
        n = self.n
        z = np.zeros(n, np.int64)
        L = SimpleNamespace()
        L.route_len = self.route[:, 1].astype(np.int64) if self.route is not None else z
        L.path_len = self.path[:, 1].astype(np.int64) if self.path is not None else z
        L.route_off = z
        L.path_off = L.route_len if self.path is not None else z   # a NULL column's ref is the block's start
        rel = L.route_len + L.path_len
        L.attr_str, L.attr_off, L.attr_len = [], [], []
        for k in range(self.K):
            s = self.attr_type[k * n:(k + 1) * n] == native.ATTR_STR
            ln = np.where(s, (self.attr_val[k * n:(k + 1) * n] >> np.uint64(32)).astype(np.int64), 0)
            L.attr_str.append(s)
            L.attr_off.append(rel)
            L.attr_len.append(ln)
            rel = rel + ln
        L.has_q = (self.db_flags & native.DB_HAS_QUERY) != 0 if (sql and self.db_flags is not None) else np.zeros(n, bool)
        L.q_len = np.where(L.has_q, self.db_query[:, 1].astype(np.int64), 0) if L.has_q.any() else z
        L.q_off = rel
        L.blen = rel + L.q_len
        self._lay[sql] = L
        return L

    def block(self, i: int, sql: bool) -> bytes:
        L = self.layout(sql)
        if not L.blen[i]:
            return b""
        a = self.arena
        parts = []
        if self.route is not None:
            o, ln = self.route[i]
            parts.append(a[o:o + ln])
        if self.path is not None:
            o, ln = self.path[i]
            parts.append(a[o:o + ln])
        for k in range(self.K):
            if L.attr_str[k][i]:
                v = int(self.attr_val[k * self.n + i])
                parts.append(a[v & 0xFFFFFFFF:(v & 0xFFFFFFFF) + (v >> 32)])
        if L.has_q[i]:
            o, ln = self.db_query[i]
            parts.append(a[o:o + ln])
        return b"".join(p.tobytes() for p in parts)


def _text(uid: int, which: int, n: int) -> np.ndarray:
    """n bytes that name their span, their string and their place in it"""
    return ((np.arange(n, dtype=np.int64) * 7 + uid * 131 + which * 17 + 1) & 0xFF).astype(np.uint8)


def lay(ids, uid0=0, scope=None, n_scopes=None, scope_resource=None, n_resources=None, Kk=2, words=1, route=None,
        path=None, attr=None, query=None, sql=False, null=(), attrset_map=None, n_attrsets=None, opname=True) -> Batch:
    """A batch of len(ids) spans.  route / path: a length per span (an int =
    every span; None = a short pattern, some of them zero); attr: per key a
    list of lengths, None in it = not a string (None = a pattern); query
    (sql): a length per span, None in it = no db.query.text (None = a
    pattern); null: names of optional columns to leave NULL ("db_flags" and
    "res_sql_ok" too).  Every fixed value derives from the span's uid (uid0 +
    i), the resource's and the scope's, so no two spans of a layout agree."""
    n = len(ids)
    u = np.arange(uid0, uid0 + n, dtype=np.int64)
    scope = np.zeros(n, np.uint32) if scope is None else np.asarray(scope, np.uint32)
    S = int(scope.max()) + 1 if n_scopes is None else n_scopes
    R = S if n_resources is None else n_resources
    sr = np.arange(S, dtype=np.uint32) % R if scope_resource is None else np.asarray(scope_resource, np.uint32)
    A = R if n_attrsets is None else n_attrsets
    b = Batch(n=n, R=R, S=S, A=A, K=Kk, words=words, attrset_map=attrset_map)
    b.trace_id = np.array([[h, l] for h, l in ids], np.uint64).reshape(n, 2)
    b.start_ns = (T0 + u).astype(np.uint64)
    b.end_ns = (T0 + u + 1 + u % 7).astype(np.uint64)
    b.status = (u % 3).astype(np.uint8)
    b.kind = (u % 6).astype(np.uint8)
    b.scope = scope
    b.scope_resource = sr
    b.resource = sr[scope]
    b.url_flags = ((u * 5) & 0x3F).astype(np.uint8)
    b.span_size = (100 + u % 900).astype(np.uint32)
    b.name_len = (u % 50).astype(np.uint32)
    b.attr_match = _splitmix64_np(np.tile(u.astype(np.uint64), words) + np.repeat(np.arange(words, dtype=np.uint64), n))
    ru = uid0 + np.arange(R, dtype=np.int64)
    su = uid0 + np.arange(S, dtype=np.int64)
    b.res_svc = (10 + ru % 7).astype(np.uint32)
    b.res_svc_str = (20 + ru % 11).astype(np.uint32)
    b.res_url_ok = (ru & 1).astype(np.uint8)
    b.res_attrset = (np.arange(R) % max(A, 1)).astype(np.uint32)
    b.res_size = (1000 + ru).astype(np.uint32)
    b.scope_size = (30 + su).astype(np.uint32)

    def lens(x, default):
        if x is None:
            x = default
        return [x] * n if isinstance(x, int) else list(x)

    route = lens(route, [int(3 + v % 5) for v in u])
    path = lens(path, [int(v % 4) for v in u])
    if attr is None:
        attr = [[int(1 + v % 3) if (v + k) % 2 == 0 else None for v in u] for k in range(Kk)]
    attr = [lens(a, None) for a in attr]
    assert len(attr) == Kk
    if sql:
        query = lens(query, [int(5 + v % 9) if v % 3 else None for v in u])
    # the source arena is laid in another order than the block (query, the
    # attribute values from the last key, path, route) with a gap byte between
    # strings, so a copy that follows the source's layout shows
    chunks, pos = [], 1
    refs = {w: np.zeros((n, 2), np.uint32) for w in ("route", "path", "query")}
    b.attr_type = np.zeros(Kk * n, np.uint8)
    b.attr_val = np.zeros(Kk * n, np.uint64)
    flags = np.zeros(n, np.uint8)

    def put(uid, which, ln):
        nonlocal pos
        at = pos
        if ln:
            chunks.append((at, _text(uid, which, ln)))
            pos += ln + 1
        return at

    for i in range(n):
        uid = uid0 + i
        if sql and query[i] is not None:
            flags[i] |= native.DB_HAS_QUERY
            refs["query"][i] = (put(uid, 9, query[i]), query[i])
        if sql and opname and uid % 4 == 0:
            flags[i] |= native.DB_HAS_OPNAME
        for k in reversed(range(Kk)):
            ln = attr[k][i]
            if ln is None:   # not a string: the value travels as it stands
                b.attr_type[k * n + i] = (native.ATTR_ABSENT, native.ATTR_INT, native.ATTR_DOUBLE, native.ATTR_BOOL)[uid % 4]
                b.attr_val[k * n + i] = splitmix64(uid * 8 + k) if uid % 4 else 0
            else:
                b.attr_type[k * n + i] = native.ATTR_STR
                b.attr_val[k * n + i] = put(uid, 3 + k, ln) | (ln << 32)
        refs["path"][i] = (put(uid, 2, path[i]), path[i])
        refs["route"][i] = (put(uid, 1, route[i]), route[i])
    arena = np.full(pos + 48, 0xEE, np.uint8)   # (DeviceBatch reads up to 31 bytes past arena_bytes)
    for at, t in chunks:
        arena[at:at + len(t)] = t
    b.arena, b.arena_bytes = arena, pos
    b.route, b.path = refs["route"], refs["path"]
    if sql:
        b.db_flags, b.db_query = flags, refs["query"]
        b.res_sql_ok = ((ru >> 1) & 1).astype(np.uint8)
    for name in null:
        assert name in ALL_OPTIONAL + ("db_flags", "res_sql_ok"), name
        setattr(b, name, None)
    if Kk == 0:
        b.attr_type = b.attr_val = None
    return b


# ---------------------------------------------------------------------------
# the store's semantics, restated over columns

class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code, self.why = code, why


class Store:
    """What the store holds and hands out, as DESIGN.md §4.7 documents it."""

    def __init__(self, wait_ns, num_traces=1_000_000, workers=1, span_cap=None, arena_cap=None, sql=False):
        self.wait, self.W, self.sql = wait_ns, workers, sql
        self.wcap = num_traces // workers           # a worker's ring of ids (one worker: num_traces)
        self.span_cap = max(span_cap or 0, K.pool_floor)
        self.arena_cap = max(arena_cap or 0, K.arena_floor)
        self.numbered = [0] * workers               # traces each worker has numbered
        self.live = {}                              # id -> its newest trace
        self.traces = {}                            # creation number -> trace, until a release passes it
        self.pending = []                           # accepted adds no release has passed: (t, created, batch)
        self.next = 0
        self.scopes_seen = 0
        self.n_attrsets = 0
        self.last_now = None
        self.c = dict.fromkeys(("created", "released", "evicted", "released_spans", "added_spans"), 0)

    def _evicted(self, tr, numbered):
        # its worker's ring slot went to the trace numbered wcap after it
        return numbered[tr.w] > tr.q + self.wcap

    def add(self, b: Batch, now: int) -> int:
        """-> traces created.  Raises Refused; a refused add changes nothing."""
        if self.last_now is not None and now < self.last_now:
            raise Refused(native.OSE_EINVAL, "clock")
        if b.n == 0:
            return 0
        if sum(p.batch.n for p in self.pending) + b.n > self.span_cap:
            raise Refused(native.OSE_ERANGE, "spans")
        if sum(p.batch.S for p in self.pending) + b.S > self.span_cap:
            raise Refused(native.OSE_ERANGE, "scopes")
        nbytes = int(b.layout(self.sql).blen.sum())
        if sum(p.bytes for p in self.pending) + nbytes > self.arena_cap:
            raise Refused(native.OSE_ERANGE, "bytes")
        start = list(self.numbered)   # eviction as of the start of the add
        ep = SimpleNamespace(t=now, created=[], batch=b, bytes=nbytes, scope0=self.scopes_seen)
        joined = {}
        for i, key in enumerate(map(tuple, b.trace_id.tolist())):
            tr = joined.get(key)
            if tr is None:
                tr = self.live.get(key)
                if tr is not None and (tr.t + self.wait <= now or self._evicted(tr, start)):
                    tr = None   # past its deadline or evicted (a released one is past its deadline)
                if tr is None:
                    w = worker_of(key[0], key[1], self.W) if self.W > 1 else 0
                    tr = SimpleNamespace(seq=self.next, t=now, w=w, q=self.numbered[w], spans=[])
                    self.numbered[w] += 1
                    self.next += 1
                    self.live[key] = tr
                    self.traces[tr.seq] = tr
                    ep.created.append(tr.seq)
                joined[key] = tr
            tr.spans.append((ep, i))
        self.pending.append(ep)
        self.scopes_seen += b.S
        top = (max(b.attrset_map) if b.attrset_map is not None else b.A - 1) + 1 if b.A else 0
        self.n_attrsets = max(self.n_attrsets, top)
        self.c["created"] += len(ep.created)
        self.c["added_spans"] += b.n
        self.last_now = now
        return len(ep.created)

    def stats(self) -> dict:
        s = dict(self.c)
        s["waiting_traces"] = sum(1 for tr in self.traces.values() if not self._evicted(tr, self.numbered))
        s["held_spans"] = sum(p.batch.n for p in self.pending)
        s["held_bytes"] = sum(p.bytes for p in self.pending)
        return s

    def release(self, now: int) -> SimpleNamespace:
        """-> n_traces, dims and the released columns (names as GroupByTrace.download)"""
        if self.last_now is not None and now < self.last_now:
            raise Refused(native.OSE_EINVAL, "clock")
        self.last_now = now
        k = 0
        while k < len(self.pending) and self.pending[k].t + self.wait <= now:
            k += 1
        out = []
        for ep in self.pending[:k]:
            for seq in ep.created:   # creation order
                tr = self.traces.pop(seq)
                if self._evicted(tr, self.numbered):
                    self.c["evicted"] += 1   # dropped
                else:
                    out.append(tr)
        del self.pending[:k]
        self.c["released"] += len(out)
        r = self._columns(out)
        self.c["released_spans"] += r.n_spans
        return r

    def _columns(self, traces) -> SimpleNamespace:
        r = SimpleNamespace(n_traces=len(traces), n_spans=0, n_fragments=0, n_attrsets=0, arena_bytes=0, cols={},
                            trace_of_span=np.zeros(0, np.int64), head=np.zeros(0, bool))
        if not traces:
            return r
        eps, idx, tno = [], [], []
        for t, tr in enumerate(traces):
            for ep, i in tr.spans:   # arrival order
                eps.append(ep)
                idx.append(i)
                tno.append(t)
        m = len(idx)
        idx, tno = np.array(idx, np.int64), np.array(tno, np.int64)
        epochs = list({id(e): e for e in eps}.values())
        eno = {id(e): k for k, e in enumerate(epochs)}
        ep_of = np.array([eno[id(e)] for e in eps], np.int64)
        sel = [(e, np.nonzero(ep_of == k)[0]) for k, e in enumerate(epochs)]

        def gather(fn, dtype, shape=()):
            o = np.zeros((m,) + shape, dtype)
            for e, at in sel:
                o[at] = fn(e.batch, idx[at])
            return o

        def col(name, default, dtype):
            return gather(lambda b, i: getattr(b, name)[i] if getattr(b, name) is not None else default, dtype)

        origin = gather(lambda b, i: b.scope[i].astype(np.int64), np.int64) + np.array([e.scope0 for e in epochs])[ep_of]
        head = np.ones(m, bool)
        head[1:] = (tno[1:] != tno[:-1]) | (origin[1:] != origin[:-1])
        frag = np.cumsum(head) - 1
        F = int(frag[-1]) + 1
        blen = gather(lambda b, i: b.layout(self.sql).blen[i], np.int64)
        base = np.cumsum(blen) - blen
        c = r.cols
        c["trace_id"] = gather(lambda b, i: b.trace_id[i], np.uint64, (2,))
        c["start_ns"] = col("start_ns", 0, np.uint64)
        c["end_ns"] = col("end_ns", 0, np.uint64)
        c["status"] = col("status", 0, np.uint8)
        c["kind"] = col("kind", 0, np.uint8)
        c["resource"] = frag.astype(np.uint32)
        c["scope"] = frag.astype(np.uint32)
        c["url_flags"] = col("url_flags", 0, np.uint8)
        c["span_size"] = col("span_size", 0, np.uint32)
        c["name_len"] = col("name_len", 0, np.uint32)
        words = epochs[0].batch.words
        c["attr_match"] = np.concatenate([gather(
            lambda b, i, w=w: b.attr_match[w * b.n + i] if b.attr_match is not None else 0, np.uint64) for w in range(words)])

        def ref(off_name, len_name):
            o = np.zeros((m, 2), np.uint32)
            o[:, 0] = base + gather(lambda b, i: getattr(b.layout(self.sql), off_name)[i], np.int64)
            o[:, 1] = gather(lambda b, i: getattr(b.layout(self.sql), len_name)[i], np.int64)
            return o

        c["route"] = ref("route_off", "route_len")
        c["path"] = ref("path_off", "path_len")
        Kk = epochs[0].batch.K
        if Kk:
            types, vals = [], []
            for k in range(Kk):
                t = gather(lambda b, i, k=k: b.attr_type[k * b.n + i], np.uint8)
                v = gather(lambda b, i, k=k: b.attr_val[k * b.n + i], np.uint64)
                off = base + gather(lambda b, i, k=k: b.layout(self.sql).attr_off[k][i], np.int64)
                ln = gather(lambda b, i, k=k: b.layout(self.sql).attr_len[k][i], np.int64)
                s = t == native.ATTR_STR
                v[s] = off[s].astype(np.uint64) | (ln[s].astype(np.uint64) << np.uint64(32))
                types.append(t)
                vals.append(v)
            c["attr_type"], c["attr_val"] = np.concatenate(types), np.concatenate(vals)
        # a fragment: a run of one trace from one added scope, with that scope's
        # resource as it was added
        first = np.nonzero(head)[0]

        def fcol(fn, dtype):
            o = np.zeros(F, dtype)
            for f, j in enumerate(first):
                b = eps[j].batch
                s = int(b.scope[idx[j]])
                o[f] = fn(b, s, int(b.scope_resource[s]))
            return o

        c["res_svc"] = fcol(lambda b, s, x: b.res_svc[x], np.uint32)
        c["res_svc_str"] = fcol(lambda b, s, x: b.res_svc_str[x] if b.res_svc_str is not None else b.res_svc[x], np.uint32)
        c["res_url_ok"] = fcol(lambda b, s, x: b.res_url_ok[x] if b.res_url_ok is not None else 1, np.uint8)
        c["res_attrset"] = fcol(lambda b, s, x: b.attrset_map[b.res_attrset[x]] if b.attrset_map is not None
                                else b.res_attrset[x], np.uint32)
        c["res_size"] = fcol(lambda b, s, x: b.res_size[x] if b.res_size is not None else 0, np.uint32)
        c["scope_size"] = fcol(lambda b, s, x: b.scope_size[s] if b.scope_size is not None else 0, np.uint32)
        c["scope_resource"] = np.arange(F, dtype=np.uint32)
        if self.sql:
            c["db_flags"] = col("db_flags", 0, np.uint8)
            q = ref("q_off", "q_len")
            has = gather(lambda b, i: b.layout(True).has_q[i], bool)
            q[~has] = 0
            c["db_query"] = q
            c["res_sql_ok"] = fcol(lambda b, s, x: b.res_sql_ok[x] if b.res_sql_ok is not None else 1, np.uint8)
        with_bytes = np.nonzero(blen)[0]
        arena = b"".join(eps[j].batch.block(int(idx[j]), self.sql) for j in with_bytes)
        assert len(arena) == int(blen.sum())
        c["arena"] = np.frombuffer(arena, np.uint8)
        r.n_spans, r.n_fragments, r.n_attrsets, r.arena_bytes = m, F, self.n_attrsets, len(arena)
        r.trace_of_span, r.head = tno, head
        return r


# ---------------------------------------------------------------------------
# the host's bookkeeping, restated

class Census:
    """gbt_host.cpp's counters: ring positions, the id table's policy, the
    release's seq range.  Every call returns a record of the seams it met."""

    def __init__(self, wait_ns, num_traces=1_000_000, workers=1, span_cap=None, arena_cap=None):
        self.wait, self.num_traces, self.W = wait_ns, num_traces, workers
        self.pool_cap = max(span_cap or 0, K.pool_floor)
        self.arena_cap = max(arena_cap or 0, K.arena_floor)
        self.table_slots = self.epoch = self.slots_used = 0
        self.table_valid = False
        self.pool_begin = self.pool_end = self.scope_begin = self.scope_end = self.arena_begin = self.arena_end = 0
        self.next_seq = self.rel_end = 0
        self.epochs = []      # (t, seq1, pool1, scope1, arena1)
        self.n_attrsets = 0

    def state(self) -> tuple:
        return (self.table_slots, self.epoch, self.slots_used, self.pool_begin, self.pool_end, self.scope_begin,
                self.scope_end, self.arena_begin, self.arena_end, self.next_seq, self.rel_end, len(self.epochs),
                self.n_attrsets)

    def _evict_below(self):
        return self.next_seq - self.num_traces if self.W == 1 and self.next_seq > self.num_traces else 0

    def _live_lo(self):
        return max(self.rel_end, self._evict_below())

    def add(self, now, n, S, nbytes, created, top_set) -> SimpleNamespace:
        """created / top_set: what the semantics say the add numbers (the census
        restates counters, not lookups)"""
        r = SimpleNamespace(kind="add", n=n, refused=None, rebuild=False, grew=False, slots=self.table_slots,
                            pool_pos=self.pool_end, scope_pos=self.scope_end, arena_pos=self.arena_end,
                            pool_fill=self.pool_end - self.pool_begin + n, scope_fill=self.scope_end - self.scope_begin + S,
                            arena_fill=self.arena_end - self.arena_begin + nbytes, bytes=nbytes, claimed=None, live=None)
        if r.pool_fill > self.pool_cap or r.scope_fill > self.pool_cap:
            r.refused = "spans" if r.pool_fill > self.pool_cap else "scopes"
            return r
        b = self.rel_end
        for t, seq1, *_ in self.epochs:
            if t + self.wait > now:
                break
            b = max(b, seq1)
        live = self.next_seq - max(self._live_lo(), b)
        slots = K.table_floor
        while slots < K.table_factor * (live + n):
            slots <<= 1
        r.claimed = self.slots_used + n
        r.live = live
        r.rebuild = not self.table_valid or self.slots_used + n > self.table_slots // K.rebuild_div
        if slots > self.table_slots:
            self.table_slots, self.epoch, r.rebuild, r.grew = slots, 0, True, True
        if r.rebuild:
            self.epoch += 1
            self.slots_used = live
        self.table_valid = True
        r.slots = self.table_slots
        if r.arena_fill > self.arena_cap:
            self.slots_used += n   # the ids the lookups claimed stay as tombstones
            r.refused = "bytes"
            return r
        self.slots_used += created
        self.next_seq += created
        self.pool_end += n
        self.scope_end += S
        self.arena_end += nbytes
        self.n_attrsets = max(self.n_attrsets, top_set)
        self.epochs.append((now, self.next_seq, self.pool_end, self.scope_end, self.arena_end))
        return r

    def release(self, now) -> SimpleNamespace:
        k, b = 0, self.rel_end
        while k < len(self.epochs) and self.epochs[k][0] + self.wait <= now:
            b = max(b, self.epochs[k][1])
            k += 1
        lo = self._live_lo()
        rng = b - lo if b > lo else 0
        bits = 0
        while rng and bits < 32 and ((rng - 1) >> bits):
            bits += 1
        r = SimpleNamespace(kind="release", epochs=k, range=rng, bits=bits, passes=(bits + 7) // 8,
                            window=self.pool_end - self.pool_begin, pool_pos=self.pool_begin)
        self.rel_end = max(self.rel_end, b)
        if k:
            _, _, self.pool_begin, self.scope_begin, self.arena_begin = self.epochs[k - 1]
            del self.epochs[:k]
        return r


# ---------------------------------------------------------------------------
# layouts: a store's configuration and a list of steps

class Layout:
    """engine: "plain" (the suite's config: two attribute key columns), "k0"
    (none) or "sql" (the odigossqldboperationprocessor section)."""

    def __init__(self, name, wait="1s", wait_ns=SEC, num_traces=None, workers=1, span_cap=1024, arena_cap=1 << 16,
                 engine="plain"):
        self.name, self.engine = name, engine
        self.sql, self.K = engine == "sql", 0 if engine == "k0" else 2
        self.cfg = {"wait_duration": wait}
        if num_traces is not None:
            self.cfg["num_traces"] = num_traces
        if workers != 1:
            self.cfg["num_workers"] = workers
        self.wait_ns, self.num_traces, self.W = wait_ns, num_traces or 1_000_000, workers
        self.span_cap, self.arena_cap = span_cap, arena_cap
        self.steps = []
        self.uid = 0
        self.seams = []       # (text, predicate over the expected steps)
        self._expected = None

    def add(self, ids, now, **kw):
        b = lay(ids, uid0=self.uid, Kk=self.K, sql=self.sql, **kw)
        self.uid += max(b.n, b.S, b.R) + 1
        self.steps.append(("add", b, int(now)))
        return len(self.steps) - 1

    def release(self, now):
        self.steps.append(("release", None, int(now)))
        return len(self.steps) - 1

    def seam(self, text, pred):
        self.seams.append((text, pred))

    def expected(self) -> list:
        """Each step as the restatement and the census have it (computed once)."""
        if self._expected is not None:
            return self._expected
        st = Store(self.wait_ns, self.num_traces, self.W, self.span_cap, self.arena_cap, self.sql)
        cs = Census(self.wait_ns, self.num_traces, self.W, self.span_cap, self.arena_cap)
        out = []
        for kind, b, now in self.steps:
            e = SimpleNamespace(kind=kind, now=now, refused=None, created=0, released=None)
            if kind == "add":
                nbytes = int(b.layout(self.sql).blen.sum())
                try:
                    e.created = st.add(b, now)
                except Refused as x:
                    e.refused, e.why = x.code, x.why
                if e.refused is not None and e.why == "clock":
                    e.census = SimpleNamespace(kind="add", refused="clock")
                else:
                    e.census = cs.add(now, b.n, b.S, nbytes, e.created, st.n_attrsets)
                    assert e.census.refused == (e.why if e.refused is not None else None), (self.name, len(out))
            else:
                e.released = st.release(now)
                e.census = cs.release(now)
            e.stats, e.state = st.stats(), cs.state()
            # the two restatements agree where they overlap
            assert e.stats["held_spans"] == cs.pool_end - cs.pool_begin and e.stats["created"] == cs.next_seq
            assert e.stats["held_bytes"] == cs.arena_end - cs.arena_begin and cs.n_attrsets == st.n_attrsets
            out.append(e)
        self._expected = out
        return out


def grouped(sizes, first=0):
    """ids of consecutive traces, sizes[k] spans each: [t0, t0, t1, ...]"""
    return [tid(first + k) for k, c in enumerate(sizes) for _ in range(c)]


def _cycle(n, pattern):
    """trace sizes from `pattern`, cut to n spans in all"""
    sizes, k = [], 0
    while sum(sizes) < n:
        sizes.append(min(pattern[k % len(pattern)], n - sum(sizes)))
        k += 1
    return sizes


# ---- blocks ------------------------------------------------------------------

def blocks(engine="plain") -> list:
    T = K.kGbtThreads
    L = Layout("blocks-" + engine, engine=engine)
    now, first = 0, 0
    marks = {}
    for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024):
        # traces of three spans: 3 * 85 = 255, so trace 85 opens at output 255
        # and runs across the gather block's boundary (256 reads 255: same
        # trace, same scope: no head); n = 257: trace 85's last span comes
        # from another scope (a head at 256 by the scope alone)
        sizes = _cycle(n, [3])
        ids = grouped(sizes, first)
        scope = [0] * n
        kw = {}
        if n == 257:
            scope[256] = 1
        if n == 65:   # one trace interleaves two scopes: A, B, A -> three fragments
            scope[30], scope[31], scope[32] = 0, 1, 0   # trace 10's three spans
        if n == 1023:   # scope[i] not monotone, more scopes than resources
            scope = [(i * 7) % 5 for i in range(n)]
            kw = dict(n_scopes=5, n_resources=2, scope_resource=[1, 0, 1, 1, 0], attrset_map=[4, 2], n_attrsets=2)
        if n == 1024 and engine == "sql":
            kw = dict(null=("db_flags",))
        if n == 256 and engine == "sql":
            kw = dict(null=("res_sql_ok",))
        first += len(sizes)
        L.add(ids, now, scope=scope, **kw)
        marks[n] = L.release(now + SEC)
        now += 2 * SEC
    L.seam("n = 65 holds a trace laid A, B, A over two scopes: three fragments",
           lambda ex: ex[marks[65]].released.n_fragments == len(_cycle(65, [3])) + 2)
    L.seam("n = 257: outputs 255 and 256 are one trace and 256 is a fragment head (the scope changes)",
           lambda ex: (lambda r: r.trace_of_span[T - 1] == r.trace_of_span[T] and r.head[T])(ex[marks[257]].released))
    L.seam("n = 1024: outputs 255 and 256 are one trace and 256 is no head; 255 is one (the trace changes)",
           lambda ex: (lambda r: r.trace_of_span[T - 1] == r.trace_of_span[T] and not r.head[T] and r.head[T - 1])(
               ex[marks[1024]].released))
    L.seam("n = 1023: scope[i] is not monotone, so fragments are cut inside traces",
           lambda ex: ex[marks[1023]].released.n_fragments > ex[marks[1023]].released.n_traces)
    L.seam("every size is released whole", lambda ex: all(ex[s].released.n_spans == n for n, s in marks.items()))
    W = Layout("blocks-window-" + engine, engine=engine, span_cap=8192)
    two_tiles, two_sort = K.kScanTileItems + 1, K.kSortTile + 1
    W.add(grouped(_cycle(two_tiles, [2, 1, 4]), 5000), 0, scope=[i % 3 for i in range(two_tiles)])
    a = W.release(SEC)
    W.add(grouped(_cycle(two_sort, [5, 1, 2]), 9000), 2 * SEC, route=2, path=1)
    b = W.release(3 * SEC)
    W.seam("a release window of 1025 (two scan tiles) and one of 4097 (two sort tiles)",
           lambda ex: ex[a].census.window == two_tiles and ex[b].census.window == two_sort and
           ex[b].released.n_spans == two_sort and ex[b].census.passes == 2)
    return [L, W]


# ---- pool ring ---------------------------------------------------------------

def pool_ring(engine="plain") -> list:
    cap = K.pool_floor
    L = Layout("pool-ring-" + engine, engine=engine)
    h = SEC // 2

    def ids(first, n, back=()):
        # new traces of 1-3 spans; `back`: ids of the add before (their traces still wait)
        out = grouped(_cycle(n - len(back), [1, 3, 2]), first)
        for k, x in enumerate(back):
            out.insert((k * 5) % (len(out) + 1), x)
        return out

    a1 = ids(0, 400)
    L.add(a1, 0)
    L.add(ids(1000, 400, back=a1[:40]), h)
    L.release(2 * h)                                  # the first add leaves: pool_begin 400
    # 800 -> 1300 crosses the ring's end inside the batch; one trace lies on both sides of it
    cross = ids(2000, 498)
    straddler = tid(2999)
    cross.insert(cap - 800 - 1, straddler)            # ring position 1023
    cross.insert(cap - 800, straddler)                # ring position 0
    s_cross = L.add(cross, 2 * h + 1, null=("db_flags",) if engine == "sql" else ())
    L.release(3 * h)                                  # the second add leaves (pool_begin 800)
    r_cross = L.release(4 * h + 1)                    # the crossing add leaves: held 0
    s_end = L.add(ids(3000, 2 * cap - 1300), 5 * h)   # ends exactly on the ring's end
    s_full = L.add(ids(4000, cap - (2 * cap - 1300)), 5 * h + 1)   # fills the pool to exactly pool_cap: accepted
    s_over = L.add([tid(4999)], 5 * h + 2)            # one more span: OSE_ERANGE, nothing changes
    L.release(7 * h)                                  # s_end leaves
    s_next = L.add(ids(5000, 300, back=[tid(4000)]), 7 * h)   # the next add is right (and joins a waiting trace)
    L.release(8 * h)
    now = 9 * h + 2
    L.release(now)
    first = 6000
    while sum(s[1].n for s in L.steps if s[0] == "add") < 3 * cap + 600:   # past the third lap
        now += 1
        L.add(ids(first, 600, back=[tid(first - 1000)]), now, null=("res_sql_ok",) if engine == "sql" else ())
        first += 1000
        now += 2 * h
        L.release(now)
    L.seam("a batch crosses the pool ring's end inside itself",
           lambda ex: ex[s_cross].census.pool_pos % cap + ex[s_cross].census.n > cap and ex[s_cross].census.pool_pos % cap)
    L.seam("a trace has spans on both sides of the wrap",
           lambda ex: (lambda r: r.n_spans == 500 and r.cols["trace_id"].tolist().count(list(straddler)) == 2)(
               ex[r_cross].released))
    L.seam("a batch ends exactly on the ring's end", lambda ex: ex[s_end].state[4] % cap == 0 and ex[s_end].state[4])
    L.seam("a fill to exactly pool_cap is accepted, one more span is refused and changes nothing",
           lambda ex: ex[s_full].census.pool_fill == cap and ex[s_full].refused is None and
           ex[s_over].census.pool_fill == cap + 1 and ex[s_over].refused == native.OSE_ERANGE and
           ex[s_over].state == ex[s_full].state and ex[s_over].stats == ex[s_full].stats)
    L.seam("the add after the refusal joins a waiting trace", lambda ex: ex[s_next].created == len(set(ids(5000, 299))))
    L.seam("at least three laps of the ring", lambda ex: ex[-1].state[4] >= 3 * cap)
    return [L]


# ---- scope ring ----------------------------------------------------------------

def scope_ring() -> list:
    cap = K.pool_floor
    L = Layout("scope-ring")
    h = SEC // 2

    def scopes(n, S, lo):
        return [lo + (i * 13) % (S - lo) for i in range(n)]

    s_more = L.add(grouped([2] * 5, 0), 0, scope=scopes(10, 500, 0), n_scopes=500, n_resources=7)   # empty scopes
    L.add(grouped([1] * 20, 100), h, scope=scopes(20, 400, 0), n_scopes=400, n_resources=400)
    L.release(2 * h)                                    # scope_begin 500
    # scopes 900 -> 1200: the batch's scopes 124.. lie past the ring's end, and its spans use both sides
    sc = [100 + i for i in range(60)]
    s_wrap = L.add(grouped([3] * 20, 200), 2 * h + 1, scope=sc, n_scopes=300, n_resources=150)
    s_over = L.add(grouped([1] * 5, 300), 2 * h + 2, scope=scopes(5, 325, 0), n_scopes=325, n_resources=3)
    s_full = L.add(grouped([1] * 5, 300), 2 * h + 3, scope=scopes(5, 324, 0), n_scopes=324, n_resources=3)
    r1 = L.release(3 * h)
    r2 = L.release(5 * h)
    L.add(grouped([2] * 8, 400), 5 * h + 1, scope=scopes(16, 900, 800), n_scopes=900, n_resources=900)
    L.release(8 * h)
    L.seam("more scopes than spans", lambda ex: ex[s_more].state[6] == 500 and ex[s_more].state[4] == 10)
    L.seam("the scope ring wraps inside a batch, with spans on both sides",
           lambda ex: ex[s_wrap].census.scope_pos == 900 and (900 + min(sc)) < cap <= (900 + max(sc)))
    L.seam("OSE_ERANGE from the scopes alone, one scope past the ring",
           lambda ex: ex[s_over].refused == native.OSE_ERANGE and ex[s_over].why == "scopes" and
           ex[s_over].census.scope_fill == cap + 1 and ex[s_over].census.pool_fill < cap and
           ex[s_over].state == ex[s_wrap].state)
    L.seam("a fill to exactly scope_cap is accepted", lambda ex: ex[s_full].census.scope_fill == cap and ex[s_full].refused is None)
    L.seam("the releases hand out the wrapped scopes", lambda ex: ex[r1].released.n_spans == 20 and ex[r2].released.n_spans == 65)
    return [L]


# ---- arena ring ------------------------------------------------------------------

def arena_ring(engine="plain") -> list:
    """Each lap brings the ring position to a chosen distance before the ring's
    end with filler spans, then lays one span whose route, path, attribute
    value or query crosses the end, or whose block ends exactly on it."""
    cap = K.arena_floor
    L = Layout("arena-ring-" + engine, engine=engine)
    Kk, sql = L.K, L.sql
    kinds = ["route", "path"] + (["attr0", "attr1"] if Kk else []) + (["query"] if sql else []) + ["exact"]
    now, first, pos = 0, 0, 0
    marks = []

    def strings(n, route=0, path=0, a0=None, a1=None, q=None):
        kw = dict(route=[route] * n if isinstance(route, int) else route,
                  path=[path] * n if isinstance(path, int) else path)
        if Kk:
            kw["attr"] = [[a0] * n if not isinstance(a0, list) else a0, [a1] * n if not isinstance(a1, list) else a1]
        if sql:
            kw["query"] = [q] * n if not isinstance(q, list) else q
        return kw

    # zero-length strings of every kind, a few bytes: the ring position leaves 0
    s0 = L.add(grouped([1] * 8, first), now, **strings(8, [0, 9, 0, 9, 0, 9, 0, 9], [0, 0, 6, 6, 0, 0, 6, 6],
                                                       [0, None, 0, 5, 0, None, 0, 5], [None, 0, 4, 0, None, 0, 4, 0],
                                                       [0, None, 7, 0, 0, None, 7, 0]))
    pos += int(L.steps[-1][1].layout(sql).blen.sum())
    L.release(now + SEC)
    for lap, kind in enumerate(kinds):
        now += 2 * SEC
        first += 100
        # the crossing span: route 10, path 10, attr0 10, attr1 10, query 40; the
        # string named by `kind` starts 3 bytes before the ring's end
        order = ["route", "path"] + (["attr0", "attr1"] if Kk else []) + (["query"] if sql else [])
        before = 10 * order.index(kind) if kind != "exact" else sum(40 if o == "query" else 10 for o in order)
        lead = 3 if kind != "exact" else 0
        fill = cap - pos % cap - before - lead
        nf = 30
        per = [fill // nf + (1 if i < fill % nf else 0) for i in range(nf)]
        # the filler's bytes in one kind of string per lap, so every copy loop runs long once
        fk = order[lap % len(order)]
        z = [0] * nf
        kw = strings(nf + 2, (per if fk == "route" else z) + [10, 3], (per if fk == "path" else z) + [10, 0],
                     (per if fk == "attr0" else z) + [10, None], (per if fk == "attr1" else [None] * nf) + [10, 2],
                     (per if fk == "query" else [None] * nf) + [40, None])
        s = L.add(grouped([1] * (nf + 2), first), now, **kw)
        nbytes = int(L.steps[-1][1].layout(sql).blen.sum())
        marks.append((kind, s, pos, fill + before, nbytes))
        pos += nbytes
        L.release(now + SEC)
    for kind, s, p0, to_string, nbytes in marks:
        if kind == "exact":
            L.seam("a block ends exactly on the arena ring's end",
                   lambda ex, s=s, p0=p0, d=to_string: ex[s].census.arena_pos == p0 and (p0 + d) % cap == 0)
        else:
            L.seam(f"a {kind} value lies across the arena ring's end",
                   lambda ex, s=s, p0=p0, d=to_string, ln=40 if kind == "query" else 10:
                   ex[s].census.arena_pos == p0 and (p0 + d) % cap == cap - 3 and ln > 3 and ex[s].refused is None)
    # the remaining room: one byte more is refused, exactly the room is accepted from the same position
    now += 2 * SEC
    s_held = L.add(grouped([1] * 4, 5000), now, **strings(4, 25, 0, None, None, None))
    room = cap - 100
    big = [room // 16 + (1 if i < room % 16 else 0) for i in range(16)]
    over = list(big)
    over[5] += 1
    s_over = L.add(grouped([1] * 16, 5100), now + 1, **strings(16, 0, over, None, None, None))
    s_fit = L.add(grouped([1] * 16, 5100), now + 2, **strings(16, 0, big, None, None, None))
    L.release(now + 3 * SEC)
    # every optional column NULL in one step
    s_null = L.add(grouped([2] * 6, 5200), now + 4 * SEC,
                   null=ALL_OPTIONAL + (("db_flags", "res_sql_ok") if sql else ()), **strings(12, 0, 0, 0, None, None))
    r_null = L.release(now + 6 * SEC)
    L.seam("zero-length strings of every kind", lambda ex: ex[s0].refused is None and ex[s0].census.bytes > 0)
    L.seam("one byte more than the room is refused; exactly the room is accepted at the same ring position",
           lambda ex: ex[s_over].census.arena_fill == cap + 1 and ex[s_over].refused == native.OSE_ERANGE and
           ex[s_over].why == "bytes" and ex[s_over].state[3:] == ex[s_held].state[3:] and
           ex[s_over].stats == ex[s_held].stats and ex[s_fit].census.arena_fill == cap and ex[s_fit].refused is None and
           ex[s_fit].census.arena_pos == ex[s_over].census.arena_pos)
    L.seam("every optional column NULL in one step", lambda ex: ex[r_null].released.n_spans == 12)
    return [L]


# ---- id table ------------------------------------------------------------------

def id_table() -> list:
    F, X, D = K.table_floor, K.table_factor, K.rebuild_div
    G = Layout("id-table-growth", wait="100s", wait_ns=100 * SEC)
    q = F // X                                         # 256: 4 * 256 is not past 1024
    all_ids = [tid(k) for k in range(q + 1)]
    G.add(all_ids[:200], 0)
    s_at = G.add(all_ids[200:q], 1)                    # live + n = 256
    s_grow = G.add(all_ids[q:q + 1], 2)                # live + n = 257: 1024 -> 2048
    back = [all_ids[(k * 37) % (q + 1)] for k in range(100)]
    s_back = G.add(back, 3)                            # only spans of live ids, looked up in the re-inserted table
    r = G.release(200 * SEC)
    G.seam("live + n = 256 keeps the 1,024-slot floor", lambda ex: ex[s_at].census.live + ex[s_at].census.n == q and
           ex[s_at].state[0] == F and not ex[s_at].census.grew)
    G.seam("live + n = 257 grows the table to 2,048", lambda ex: ex[s_grow].census.live + 1 == q + 1 and
           ex[s_grow].census.grew and ex[s_grow].state[0] == 2 * F)
    G.seam("after the growth an add of live ids creates nothing", lambda ex: ex[s_back].created == 0 and
           not ex[s_back].census.rebuild and ex[r].released.n_traces == q + 1 and ex[r].released.n_spans == q + 101)

    R = Layout("id-table-rebuild")
    now = 0
    for k in range(4):                                 # four adds of 100 ids, each released: 400 slots claimed
        R.add([tid(1000 * k + j) for j in range(100)], now)
        now += SEC
        if k < 3:
            R.release(now)
    live = [tid(3000 + j) for j in range(100)]         # the fourth add's traces wait
    half = F // D
    t_at = R.add([live[j % 100] for j in range(half - 400)], now - 2)          # claimed + n = 512: no rebuild
    t_past = R.add([live[j] for j in range(100)] + [tid(9000 + j) for j in range(half - 400 + 1 - 100)], now - 1)
    t_r = R.release(now + 5 * SEC)
    R.seam("slots_used + n = slots / 2 does not rebuild", lambda ex: ex[t_at].census.claimed == half and
           not ex[t_at].census.rebuild and ex[t_at].state[1] == 1)
    R.seam("slots_used + n = slots / 2 + 1 is the first add after the first to rebuild (the epoch moves)",
           lambda ex: ex[t_past].census.claimed == half + 1 and ex[t_past].census.rebuild and ex[t_past].state[1] == 2 and
           ex[t_past].state[0] == F and [e.census.rebuild for e in ex if e.kind == "add"][1:-1] == [False] * 4)
    R.seam("the live ids are found again after the rebuild", lambda ex: ex[t_past].created == half - 400 + 1 - 100 and
           ex[t_r].released.n_traces == 100 + ex[t_past].created)

    Cn = Layout("id-table-chains")
    mask = F - 1
    g1 = ids_for_slot(500, mask, 60, seed=7)           # 40 + 20 later
    g2 = ids_for_slot(F - 4, mask, 18, seed=8)         # 12 + 6 later: the chain runs 1020..1023, 0, 1, ...
    first = [x for pair in zip(g1[:40], (g2[:12] * 4)[:40]) for x in pair]
    first = list(dict.fromkeys(first))
    s1 = Cn.add(first + first[::-1], 0)                # two spans per id
    r1 = Cn.release(SEC)                               # 52 tombstones
    again = g1[0:40:2] + g2[0:12:2]                    # half of them come back
    fresh = g1[40:] + g2[12:]
    mix = [x for k in range(26) for x in (again[k], fresh[k])]
    mix = mix + mix[::3]
    s2 = Cn.add(mix, SEC + 1)
    r2 = Cn.release(3 * SEC)
    Cn.seam("40 ids collide on slot 500 and 12 on the last four slots, so their chain wraps to slot 0",
            lambda ex: ex[s1].created == 52 and ex[s1].state[0] == F and F - 4 + 12 > F)
    Cn.seam("half of them come back through their tombstones, interleaved with new colliders, in one add of "
            "the same table epoch", lambda ex: ex[r1].released.n_traces == 52 and not ex[s2].census.rebuild and
            ex[s2].state[0] == F and ex[s2].created == 52 and
            [tuple(x) for x in ex[r2].released.cols["trace_id"][np.nonzero(np.diff(ex[r2].released.trace_of_span,
                                                                                  prepend=-1))[0]].tolist()] == mix[:52])
    return [G, R, Cn]


# ---- release sort ------------------------------------------------------------------

def sort_small() -> list:
    L = Layout("sort-small")
    now, marks = 0, []
    for k, rng in enumerate((1, 2, 256, 257)):
        sizes = [3 if j % 5 == 0 else 1 for j in range(rng)]
        ids = grouped(sizes, 1000 * k)
        ids = ids[::2] + ids[1::2]                     # a trace's spans apart; first appearance keeps the numbering
        L.add(ids, now)
        marks.append((rng, L.release(now + SEC)))
        now += 2 * SEC
    L.seam("releases of range 1, 2, 256, 257: 0, 1, 1, 2 sort passes",
           lambda ex: [(ex[s].census.range, ex[s].census.passes) for _, s in marks] == [(1, 0), (2, 1), (256, 1), (257, 2)])
    return [L]


def sort_large() -> list:
    L = Layout("sort-large", span_cap=1 << 17)
    marks = []
    now = 0
    for k, rng in enumerate((1 << 16, (1 << 16) + 1)):
        base = 100_000 * (k + 1)
        firsts = [tid(base + j) for j in range(rng)]
        # 256 traces of three spans whose creation numbers agree in the low
        # byte (7) and differ in the next: their second spans arrive in reverse
        # order and their third in order, far behind the first, so a pass that
        # is not stable, or one pass too few, reorders them
        three = [firsts[7 + 256 * m] for m in range(256)]
        ids = firsts + three[::-1] + three
        n = len(ids)
        L.add(ids, now, route=0, path=0, attr=[[None] * n, [None] * n], scope=[i % 2 for i in range(n)])
        marks.append((rng, L.release(now + SEC)))
        now += 2 * SEC
    L.seam("releases of range 65,536 (two passes) and 65,537 (three)",
           lambda ex: [(ex[s].census.range, ex[s].census.passes, ex[s].released.n_traces) for _, s in marks] ==
           [(1 << 16, 2, 1 << 16), ((1 << 16) + 1, 3, (1 << 16) + 1)])
    L.seam("the three-span traces come out whole, in arrival order",
           lambda ex: all(ex[s].released.n_spans == rng + 512 for rng, s in marks))
    return [L]


# ---- the ring of ids, one worker ---------------------------------------------------

def id_ring() -> list:
    N = 64
    L = Layout("id-ring", wait="100s", wait_ns=100 * SEC, num_traces=N, span_cap=2048)
    counts = (N, N + 1, 5 * N + 1, 5 * N + 1, 255)
    first, steps = 0, []
    for k, c in enumerate(counts):
        steps.append(L.add([tid(first + j) for j in range(c)], k))
        first += c
    survivors = [tid(first - N + j) for j in range(N)]
    s_back = L.add(survivors[::-1], 10)                # one span of each surviving id, nothing new
    r = L.release(500 * SEC)
    L.seam("adds that create num_traces, num_traces + 1 and 5 * num_traces + 1 traces (the last over several blocks)",
           lambda ex: [ex[s].created for s in steps[:3]] == [N, N + 1, 5 * N + 1] and 5 * N + 1 > K.kGbtThreads)
    L.seam("the add of the 64 surviving ids re-inserts the table from the ring of ids and creates nothing",
           lambda ex: ex[s_back].census.rebuild and not ex[s_back].census.grew and ex[s_back].census.live == N and
           ex[s_back].created == 0)
    L.seam("the release holds the 64 survivors, two spans each",
           lambda ex: ex[r].released.n_traces == N and ex[r].released.n_spans == 2 * N and
           ex[r].stats["evicted"] == sum(counts) - N and
           [tuple(x) for x in ex[r].released.cols["trace_id"][::2].tolist()] == survivors)
    return [L]


# ---- workers -----------------------------------------------------------------------

def workers() -> list:
    out = []
    cap = K.pool_floor
    A = Layout("workers-laps", workers=3, num_traces=12)
    now, first, prev = 0, 0, []
    while first < 2 * cap + 100:
        A.release(now)
        ids = [tid(first + j) for j in range(90)]
        batch = ids + prev[::9]                        # ten spans of the add before: waiting, or evicted since
        A.add(batch[::-1], now)
        prev, first = ids, first + 90
        now += 6 * SEC // 10
    A.release(now + 2 * SEC)
    A.seam("creation numbers pass pool_cap twice (tinfo and the ring of ids are indexed seq % pool_cap)",
           lambda ex: ex[-1].state[9] > 2 * cap and max(e.stats["held_spans"] for e in ex) <= cap)
    A.seam("traces are evicted per worker and the survivors released",
           lambda ex: ex[-1].stats["evicted"] > 0 and ex[-1].stats["released"] > 0 and ex[-1].stats["waiting_traces"] == 0)
    out.append(A)

    B = Layout("workers-wcap", workers=3, num_traces=12)
    mine, other = ids_for_worker(1, 3, 5), ids_for_worker(0, 3, 2)
    b1 = B.add(mine[:4] + other, 0)                    # worker 1 at exactly wcap = 4: nothing evicted
    b2 = B.add([mine[4]] + mine[:4], 1)                # wcap + 1: its first trace goes (its span here with it)
    b_r = B.release(3 * SEC)
    B.seam("a worker at exactly wcap traces evicts nothing; at wcap + 1 its oldest goes",
           lambda ex: ex[b1].stats["waiting_traces"] == 6 and ex[b2].stats["waiting_traces"] == 6 and ex[b2].created == 1 and
           ex[b_r].stats["evicted"] == 1 and ex[b_r].released.n_traces == 6 and ex[b_r].released.n_spans == 6 + 3)
    out.append(B)

    for W, nt, n1, n2 in ((256, 512, 600, 300), (257, 514, 600, 300), (1025, 2050, 1000, 20)):
        Lw = Layout(f"workers-{W}", workers=W, num_traces=nt)
        ids = [tid(50_000 + j) for j in range(n1)]
        s1 = Lw.add(ids, 0)
        Lw.release(SEC)
        more = [tid(60_000 + j) for j in range(n2)]
        s2 = Lw.add(more[:n2 // 2] + ids[:n2 // 4] + more[n2 // 2:], SEC + 1)
        Lw.release(3 * SEC)
        bits = (W - 1).bit_length()
        Lw.seam(f"{W} workers: the numbering sorts {bits}-bit keys ({(bits + 7) // 8} passes), "
                f"{(W + K.kScanTileItems - 1) // K.kScanTileItems} scan tile(s) over the workers; the second batch has "
                f"{'fewer' if n2 < W else 'more'} spans than workers",
                lambda ex, s1=s1, s2=s2, n1=n1: ex[s1].created == n1 and ex[s2].created > 0 and ex[-1].stats["evicted"] > 0)
        out.append(Lw)
    return out


# ---- clock -------------------------------------------------------------------------

def clock() -> list:
    a, b, c, d = (tid(k) for k in range(4))
    L = Layout("clock")
    L.add([a, b], 0)
    r_stay = L.release(SEC - 1)                        # one nanosecond early: stays
    s_new = L.add([a], SEC)                            # at exactly t + wait: the id starts a new trace
    r_go = L.release(SEC)                              # at exactly t + wait: leaves
    r_again = L.release(SEC)                           # the same now: empty
    h = SEC + SEC // 2
    same = [L.add([c], h), L.add([c, d], h), L.add([d, a], h)]   # three adds with one now (a's second trace waits)
    r_early = L.release(2 * SEC - 1)
    r_a = L.release(2 * SEC)
    L.release(h + SEC)
    t = 4 * SEC
    for k in range(4):                                 # four epochs a tenth of a second apart
        L.add([tid(10 + k), a], t + k * SEC // 10)
    r_part = L.release(t + SEC + SEC // 10)            # two of the four have waited
    s_back = L.add([b], t)                             # the clock goes backwards: OSE_EINVAL
    r_rest = L.release(t + 2 * SEC)
    L.seam("a release one nanosecond before t + wait keeps the trace, one at t + wait hands it out; repeated, it is empty",
           lambda ex: ex[r_stay].released.n_traces == 0 and ex[r_go].released.n_traces == 2 and
           ex[r_go].released.n_spans == 2 and ex[r_again].released.n_traces == 0)
    L.seam("an add at exactly t + wait starts a new trace for the id", lambda ex: ex[s_new].created == 1)
    L.seam("three adds with one now are three epochs; the later ones join the earlier one's traces",
           lambda ex: [ex[s].created for s in same] == [1, 1, 0] and ex[same[2]].state[11] == 4)
    L.seam("a's second trace leaves at its own deadline with the span added later",
           lambda ex: ex[r_early].released.n_traces == 0 and ex[r_a].released.n_traces == 1 and ex[r_a].released.n_spans == 2)
    L.seam("a partial expiry: two of four epochs", lambda ex: ex[r_part].census.epochs == 2 and
           ex[r_part].released.n_traces == 3 and ex[r_part].released.n_spans == 6 and ex[r_rest].released.n_traces == 2)
    L.seam("a clock that goes backwards is OSE_EINVAL and changes nothing",
           lambda ex: ex[s_back].refused == native.OSE_EINVAL and ex[s_back].state == ex[r_part].state)
    Z = Layout("clock-wait-0", wait="0", wait_ns=0)
    z1 = Z.add([a, b, a], 5)
    z2 = Z.add([a], 5)                                 # the first trace of `a` is at its deadline already
    rz = Z.release(5)
    Z.seam("wait_duration \"0\": every add starts new traces and the release at the same now hands them out",
           lambda ex: ex[z1].created == 2 and ex[z2].created == 1 and ex[rz].released.n_traces == 3 and
           ex[rz].stats["waiting_traces"] == 0)
    return [L, Z]


def all_layouts() -> list:
    """Every family; "sql" repeats blocks, the pool ring and the arena ring on
    an engine with the odigossqldboperationprocessor section."""
    global _ALL
    if _ALL is None:
        fam = {"blocks": blocks(), "pool_ring": pool_ring(), "scope_ring": scope_ring(),
               "arena_ring": arena_ring() + arena_ring("k0"), "id_table": id_table(), "sort": sort_small() + sort_large(),
               "id_ring": id_ring(), "workers": workers(), "clock": clock(),
               "sql": blocks("sql") + pool_ring("sql") + arena_ring("sql")}
        _ALL = fam
    return _ALL


_ALL = None
FAMILIES = ("blocks", "pool_ring", "scope_ring", "arena_ring", "id_table", "sort", "id_ring", "workers", "clock", "sql")
