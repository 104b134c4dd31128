"""Hand-laid OTLP messages for the GPU encoder (tests/test_encode_layouts.py).

A layout is a TracesData message written here byte by byte in pdata's
encoding (tags and varints from tests/otlp_gogo.py), the decisions the
stages would have left beside it (keep, url_out, templates, sql_op), and a
router.  Every span's span_id carries its global index and every
ResourceSpans' schema_url its resource index (r0262144), so a record at the
wrong offset or in the wrong output shows in the bytes.  Test
infrastructure only.

expected() is the restatement: for the small layouts test_otlp_sqlop._restate
(the processors' writes, the router's split and pdata's marshaler over the
OTLP/JSON tree of the message); for the large ones records concatenated in
numpy (a TracesData is the concatenation of `0A len record`), tied to the
restatement on their first and last three resources (sample()).

census() is the encoder's dispatch (encode_kernel.hip) as a pure function of
the layout and its decisions: which scan tile, thread slot and grid-stride
iteration a resource falls in, the 64-span chunks of a scope and the lanes
kept in each, the length varints before and after the decisions, and the
route table's probe walk of every lookup.  Each layout asserts through it
(test_layout_sits_on_its_seam) that it sits where its docstring says.

The constants are parsed from the sources at import (K); DESIGNED pins the
values the layouts were drawn for.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from odigos_amd import host, native
from tests import otlp_gogo as gg

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
WAVE = 64
M64 = (1 << 64) - 1
MODES = ("full", "keep", "identity")     # all decision bits; APPLY_KEEP alone; no decision bit


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    hip = (CSRC / "encode_kernel.hip").read_text()
    hpp = (CSRC / "kernels.hpp").read_text()
    hst = (CSRC / "otlp_host.cpp").read_text()
    dec = (CSRC / "otlp_kernel.hip").read_text()

    def one(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: definition not found"
        return m

    k = SimpleNamespace()
    k.kEncTiles = int(one(hpp, r"constexpr\s+uint32_t\s+kEncTiles\s*=\s*(\d+)\s*;", "kEncTiles").group(1))
    k.kEThreads = int(one(hip, r"constexpr\s+int\s+kEThreads\s*=\s*(\d+)\s*;", "kEThreads").group(1))
    k.OSE_ETHREADS = int(one(hip, r"#define\s+OSE_ETHREADS\s+(\d+)", "OSE_ETHREADS").group(1))
    k.span_cap = int(one(hip, r"grid_of\(a\.n_spans,\s*(\d+)\)", "the span grid's cap").group(1))
    k.write_cap = int(one(hip, r"grid_of\(a\.n_res\s*\*\s*kWave,\s*(\d+)\)", "the write grid's cap").group(1))
    m = one(hst, r"constexpr\s+size_t\s+kGpuScopeBytes\s*=\s*size_t\((\d+)\)\s*<<\s*(\d+)\s*;", "kGpuScopeBytes")
    k.kGpuScopeBytes = int(m.group(1)) << int(m.group(2))
    k.kSpanStageMax = int(one(dec, r"constexpr\s+uint64_t\s+kSpanStageMax\s*=\s*(\d+)\s*;", "kSpanStageMax").group(1))
    for name in ("kEncFbSpan", "kEncFbScope", "kEncFbRes", "kEncFbTmpl", "kEncFbRoute", "kEncFbWrite"):
        setattr(k, name, int(one(hpp, name + r"\s*=\s*(\d+)\s*,", name).group(1)))
    assert "constexpr uint32_t kPer = kEncTiles / kEThreads;" in hip and "constexpr int kERec = OSE_ETHREADS;" in hip
    assert "(uint64_t)cap * (kEThreads / kERec)" in hip, "grid_of changed"
    assert "2 * r.routes.size() + 2" in (CSRC / "otlp_encode.cpp").read_text(), "build_route_blob's slot count changed"
    return k


K = _parse_constants()
DESIGNED = dict(kEncTiles=1024, kEThreads=256, OSE_ETHREADS=64, span_cap=8192, write_cap=16384,
                kGpuScopeBytes=65536, kSpanStageMax=65536)
TILE = K.kEncTiles                                            # resources per scan tile
KPER = K.kEncTiles // K.kEThreads                             # resources one scan thread owns
TOP_EDGE = K.kEncTiles * K.kEThreads                          # resources one trip of enc_scan_top_kernel's loop covers
WRITE_WAVES = K.write_cap * K.kEThreads // K.OSE_ETHREADS * (K.OSE_ETHREADS // WAVE)   # the write grid's waves
SPAN_LANES = K.span_cap * (K.kEThreads // K.OSE_ETHREADS) * K.OSE_ETHREADS            # the span grid's lanes


# ---------------------------------------------------------------------------
# the message builder (pdata's encoding, from tests/otlp_gogo.py's primitives)

LEN, VAR = gg._len, gg._varint
TID = "0d160517" * 4
SET_ATTR, RENAME = gg.SET_ATTR, gg.RENAME


def sov(x: int) -> int:
    return len(VAR(int(x)))


def span_id(i: int) -> str:
    return "a5%014x" % i


def min_span(i: int) -> bytes:
    """32 bytes: the ids and the always-written parent id and Status."""
    return gg.span({"traceId": TID, "spanId": span_id(i)})


def http_span(i: int, attributes=None, name="GET", kind=2) -> bytes:
    at = {"http.request.method": "GET", "url.path": "/user/1234", "db.query.text": "select 1"}
    at.update(attributes or {})
    return gg.span(host.span(name=name, kind=kind, trace_id=TID, span_id=span_id(i), start=1739000000000000000,
                             end=1739000000000000009, attributes=at))


def fit(make, target: int, lo: int = 0) -> bytes:
    """make(k) for the k >= lo at which its length is target (make(k) grows by
    at least one byte with k; a length a varint step jumps over is not reached)."""
    k = lo + target - len(make(lo))
    while k >= lo:
        b = make(k)
        if len(b) == target:
            return b
        if len(b) < target:
            break
        k -= 1
    raise AssertionError("no filler reaches %d bytes" % target)


def pad_span(i: int, length: int) -> bytes:
    """A span of exactly `length` bytes (a pad attribute)."""
    return fit(lambda k: gg.span(host.span(name="f", kind=1, trace_id=TID, span_id=span_id(i), attributes={"pad": "p" * k})),
               length)


def res_hdr(attrs: dict, dropped: int = 0) -> bytes:
    """A Resource payload."""
    return gg._attrs(1, host.attrs(attrs)) + gg._uvar(2, dropped)


def hdr_of(length: int, field: int = 1) -> bytes:
    """A Resource (field 1: attributes) or InstrumentationScope (field 1: name)
    payload of exactly `length` bytes; 2 is the shortest non-empty one
    (dropped_attributes_count 1), so there is no payload of 1 byte."""
    if length == 0:
        return b""
    if length == 2:
        return gg._uvar(2 if field == 1 else 4, 1)
    if field == 1:
        return fit(lambda k: res_hdr({"pad": "h" * k}), length)
    return fit(lambda k: gg._str(1, "s" * k), length, lo=1)


class Scope:
    def __init__(self, spans=(), hdr: bytes | None = b"", schema: bytes = b""):
        self.spans, self.hdr, self.schema = list(spans), hdr, schema

    def body(self) -> bytes:
        return ((LEN(1, self.hdr) if self.hdr is not None else b"") + b"".join(LEN(2, s) for s in self.spans) +
                (LEN(3, self.schema) if self.schema else b""))


class Res:
    def __init__(self, hdr: bytes | None, scopes=(), schema: bytes = b""):
        self.hdr, self.scopes, self.schema = hdr, list(scopes), schema

    def body(self) -> bytes:
        return ((LEN(1, self.hdr) if self.hdr is not None else b"") + b"".join(LEN(2, s.body()) for s in self.scopes) +
                (LEN(3, self.schema) if self.schema else b""))


def schema_of(r: int) -> bytes:
    return b"r%07d" % r


class Dec:
    """The decisions, appended span by span in message order."""

    def __init__(self, first: int = 0):
        self.i = first
        self.keep, self.url_out, self.tmpls, self.sql_op = [], [], [], []

    def add(self, keep=1, u=0, t="", op=0) -> int:
        self.keep.append(int(keep))
        self.url_out.append(u)
        self.tmpls.append(t if u else "")
        self.sql_op.append(op)
        self.i += 1
        return self.i - 1

    def min(self, keep=1) -> bytes:
        return min_span(self.add(keep))

    def edited(self, keep=1, u=0, op=0, t="/user/{id}", **kw) -> bytes:
        return http_span(self.add(keep, u, t, op), **kw)


# ---------------------------------------------------------------------------
# routers.  The seven Resource messages of the scan layouts and the two
# routers they are laid against (three outputs: p0, p1, default).

def _src(ns, kind, name):
    return {"namespace": ns, "kind": kind, "name": name}


def _stream(name, sources, signals=("TRACES",)):
    return {"name": name, "sources": list(sources),
            "destinations": [{"destinationname": "d-" + name, "configuredsignals": list(signals)}]}


CFG_A = {"datastreams": [
    _stream("p0", [_src("prod", "Deployment", "w-one"), _src("prod", "deployment", "w-two"), _src("prod", "DaemonSet", "w-one")]),
    _stream("p1", [_src("prod", "Deployment", "w-two"), _src("prod", "Deployment", "w-ds")])]}
# the middle output receives nothing
CFG_B = {"datastreams": [
    _stream("p0", [_src("prod", "Deployment", "w-one"), _src("prod", "deployment", "w-two"), _src("prod", "Deployment", "w-ds")]),
    _stream("p1", [_src("prod", "Deployment", "nobody")])]}
VARIANTS = [
    ("one", res_hdr({"service.name": "a", "k8s.namespace.name": "prod", "k8s.deployment.name": "w-one"})),
    ("two", res_hdr({"service.name": "bb-two", "k8s.namespace.name": "prod", "k8s.deployment.name": "w-two"})),
    ("unmatched", res_hdr({"k8s.namespace.name": "prod", "k8s.deployment.name": "ghost", "service.name": "ccc"})),
    ("no_namespace", res_hdr({"k8s.deployment.name": "w-one"})),
    ("namespace_not_a_string", res_hdr({"k8s.namespace.name": 5, "k8s.deployment.name": "w-one", "service.name": "e" * 9})),
    ("daemonset_beside_deployment", res_hdr({"k8s.namespace.name": "prod", "k8s.daemonset.name": "w-one",
                                             "k8s.deployment.name": "w-ds"})),
    ("no_resource_field", None),
]
VARIANT_OUT = {"A": [[0], [0, 1], [2], [2], [2], [1], [2]], "B": [[0], [0], [2], [2], [2], [0], [2]]}

_routers: dict = {}


def router_of(cfg):
    """The product's Router for a config (built once)."""
    from odigos_amd.batch import Router
    key = host.dumps(cfg)
    if key not in _routers:
        _routers[key] = Router(cfg)
    return _routers[key]


def pipelines_of(cfg) -> list:
    """Router::pipelines restated: the TRACES streams' names, first appearance."""
    out = []
    for ds in cfg.get("datastreams") or []:
        if "TRACES" in gg.signals_for(ds) and ds.get("name", "") not in out:
            out.append(ds.get("name", ""))
    return out


# ---- the route table (build_route_blob / route_resource) ----

SLOT = np.dtype([("h", "<u8"), ("koff", "<u4"), ("klen", "<u4"), ("mask", "<u8")])
EMPTY = 0xFFFFFFFF


def fnv1a(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & M64
    return h


def table_bits(n_routes: int) -> int:
    bits = 1
    while (1 << bits) < 2 * n_routes + 2:
        bits += 1
    return bits


def restate_table(entries):
    """build_route_blob: entries [(key bytes, mask)] in insertion order -> (bits, slots, key bytes)."""
    bits = table_bits(len(entries))
    n = 1 << bits
    tab = np.zeros(n, dtype=SLOT)
    tab["klen"] = EMPTY
    keys = b""
    for key, mask in entries:
        h = fnv1a(key)
        s = h & (n - 1)
        while tab[s]["klen"] != EMPTY:
            s = (s + 1) & (n - 1)
        tab[s] = (h, len(keys), len(key), mask)
        keys += key
    return bits, tab, keys


def real_table(router):
    """(route_bits, slots, key bytes) of the product's Router::dev_blob."""
    L = native.lib()
    nb, bits, sb = C.c_uint64(), C.c_uint32(), C.c_uint64()
    native.check(L.osehost_router_table(router.h, None, 0, C.byref(nb), C.byref(bits), C.byref(sb)))
    buf = np.zeros(max(nb.value, 1), dtype=np.uint8)
    native.check(L.osehost_router_table(router.h, buf.ctypes.data, nb.value, None, None, None))
    tab = buf[:sb.value].view(SLOT).copy()
    return bits.value, tab, buf[sb.value:nb.value].tobytes()


def route_entries(cfg, order=None):
    """[(key bytes, pipelines mask)] of a config's TRACES routes; `order`: key
    bytes in the product's insertion order (Router::routes is an unordered
    map: its iteration order is read from the real table's key area)."""
    pipes = pipelines_of(cfg)
    m = gg.build_routing_map(cfg.get("datastreams") or [])
    ent = {}
    for key, idx in m.items():
        names = idx.get("TRACES") or []
        if names:
            ent[gg._b(key)] = sum(1 << pipes.index(p) for p in names)
    # build_router inserts the key of every source of a TRACES stream, listed or not
    keys = list(ent) if order is None else list(order)
    assert sorted(keys) == sorted(ent), (keys, list(ent))
    return [(k, ent[k]) for k in keys]


def table_of(cfg):
    """The restated table, inserted in the product's order."""
    bits, tab, keys = real_table(router_of(cfg))
    if bits == 0:      # no "datastreams" at all: no table is built, and the encoder does not look anything up
        return 0, tab, b""
    occ = np.nonzero(tab["klen"] != EMPTY)[0]
    occ = occ[np.argsort(tab["koff"][occ], kind="stable")]
    order = [keys[int(tab[s]["koff"]):int(tab[s]["koff"]) + int(tab[s]["klen"])] for s in occ]
    return restate_table(route_entries(cfg, order))


def routing_key(hdr: bytes | None, tree_attrs) -> bytes | None:
    """determineRoutingPipelines' key for a Resource (None: the default pipeline before any lookup)."""
    ns = gg._find(tree_attrs, "k8s.namespace.name")
    if hdr is None or ns is None:
        return None
    for key, kind in (("k8s.deployment.name", "deployment"), ("k8s.statefulset.name", "statefulset"),
                      ("k8s.daemonset.name", "daemonset")):
        v = gg._find(tree_attrs, key)
        if v is not None:
            name = gg._str_of(v["value"])
            return gg._b("%s/%s/%s" % (gg._str_of(ns["value"]), kind, name)) if name else None
    return None


def lookup(table, key: bytes) -> SimpleNamespace:
    """route_resource's probe loop."""
    bits, tab, keys = table
    mask = (1 << bits) - 1
    h = fnv1a(key)
    out = SimpleNamespace(home=h & mask, probes=0, wrapped=False, end="full", mask=0, same_len_miss=0)
    s = out.home
    while out.probes <= mask:
        out.probes += 1
        e = tab[s]
        if e["klen"] == EMPTY:
            out.end = "empty"
            return out
        if int(e["h"]) == h and int(e["klen"]) == len(key) and keys[int(e["koff"]):int(e["koff"]) + len(key)] == key:
            out.end, out.mask = "hit", int(e["mask"])
            return out
        out.same_len_miss += int(e["klen"]) == len(key)
        s = (s + 1) & mask
        out.wrapped |= s == 0
    return out


# ---------------------------------------------------------------------------
# small layouts

def _walk_lengths(msg: bytes):
    """[(resource body length, [scope body lengths])] of a TracesData."""
    out, p = [], 0

    def varint(p):
        v = s = 0
        while True:
            b = msg[p]
            p += 1
            v |= (b & 0x7F) << s
            s += 7
            if b < 0x80:
                return v, p

    while p < len(msg):
        assert msg[p] == 0x0A
        n, p = varint(p + 1)
        end, scopes = p + n, []
        while p < end:
            tag = msg[p]
            ln, p = varint(p + 1)
            if tag == 0x12:
                scopes.append(ln)
            p += ln
        assert p == end
        out.append((n, scopes))
    return out


class Layout:
    """A small layout: `res` [Res], the decisions `dec`, the router config `cfg`."""
    big = False

    def __init__(self, name, res, dec: Dec | None = None, cfg=CFG_A, marks=None):
        self.name, self.res, self.cfg, self.marks = name, list(res), cfg, dict(marks or {})
        self.R = len(self.res)
        self.S = sum(len(r.scopes) for r in self.res)
        self.n = sum(len(s.spans) for r in self.res for s in r.scopes)
        dec = dec or Dec()
        n = self.n
        assert len(dec.keep) in (0, n), (name, len(dec.keep), n)
        self.keep = np.array(dec.keep or [1] * n, dtype=np.uint8)
        self.url_out = np.array(dec.url_out or [0] * n, dtype=np.uint8)
        self.sql_op = np.array(dec.sql_op or [0] * n, dtype=np.uint8)
        self.tmpls = list(dec.tmpls or [""] * n)
        self.msg = b"".join(LEN(1, r.body()) for r in self.res)
        self._tree = None
        self._exp = {}

    # the decoder's columns
    def columns(self):
        scope_spans = np.array([len(s.spans) for r in self.res for s in r.scopes], dtype=np.int64)
        res_scopes = np.array([len(r.scopes) for r in self.res], dtype=np.int64)
        scope_resource = np.repeat(np.arange(self.R, dtype=np.uint32), res_scopes)
        scope = np.repeat(np.arange(self.S, dtype=np.uint32), scope_spans)
        return scope_resource[scope] if self.n else np.zeros(0, np.uint32), scope, scope_resource

    @property
    def tree(self):
        if self._tree is None:
            from tests.test_otlp import _pb_to_json
            self._tree = _pb_to_json(self.msg) if self.msg else {"resourceSpans": []}
            assert self._tree is not None, self.name
        return self._tree

    def decisions(self, mode="full") -> dict:
        """The keyword arguments of _restate / the CPU seam for a stage mask."""
        if mode == "identity":
            return {}
        if mode == "keep":
            return {"keep": self.keep.tolist()}
        return {"keep": self.keep.tolist(), "url_out": self.url_out.tolist(), "tmpls": self.tmpls,
                "sql_op": self.sql_op.tolist()}

    def expected(self, mode="full", routed=True):
        """[(pipeline, TracesData bytes, resources)] per output."""
        key = (mode, routed)
        if key not in self._exp:
            from tests.test_otlp_sqlop import _restate
            d = self.decisions(mode)
            if routed:
                self._exp[key] = _restate(self.tree, self.cfg.get("datastreams") or [], router_of(self.cfg).pipelines, **d)
            else:
                self._exp[key] = _restate(self.tree, **d)
        return self._exp[key]

    def sample(self):
        return None


def census(L, mode="full") -> SimpleNamespace:
    """The encoder's dispatch for a layout under a stage mask."""
    c = SimpleNamespace()
    R, S, n = L.R, L.S, L.n
    r = np.arange(R, dtype=np.int64)
    c.tiles = max(1, -(-R // TILE))
    c.tile, c.slot = r // TILE, r % KPER
    c.top_trips = -(-c.tiles // K.kEThreads)
    c.write_iter = r // WRITE_WAVES
    c.write_iters = -(-R // WRITE_WAVES)
    c.span_iters = -(-n // SPAN_LANES)
    c.n_out = len(pipelines_of(L.cfg)) + 1
    if L.big:
        return L.census_into(c, mode)
    keep = L.keep.astype(bool) if mode != "identity" else np.ones(n, dtype=bool)
    # scopes: chunks of 64 spans and the lanes kept in each; the removal rules
    c.chunks, c.scope_alive, c.res_alive, c.scope_before, c.res_before = [], [], [], [], []
    c.scope_state, c.res_state = [], []      # "empty" (no spans before the decisions), "emptied", "kept"
    i = 0
    for rs in L.res:
        had = any_alive = False
        for sc in rs.scopes:
            k = len(sc.spans)
            ks = keep[i:i + k]
            c.chunks.append([np.nonzero(ks[q:q + WAVE])[0].tolist() for q in range(0, k, WAVE)])
            alive = not k or bool(ks.any())
            c.scope_alive.append(alive)
            c.scope_state.append("empty" if not k else "kept" if alive else "emptied")
            c.scope_before.append(len(sc.body()))
            had |= k > 0
            any_alive |= alive
            i += k
        c.res_alive.append(not had or any_alive)
        c.res_state.append("spanless" if not had else "kept" if any_alive else "emptied")
        c.res_before.append(len(rs.body()))
    # the length varints after the decisions, read from the restatement's bytes
    after = _walk_lengths(L.expected(mode, routed=False)[0][1])
    assert len(after) == sum(c.res_alive), (L.name, len(after), sum(c.res_alive))
    c.res_after, c.scope_after = [None] * R, [None] * S
    it = iter(after)
    s = 0
    for q, rs in enumerate(L.res):
        lens = next(it) if c.res_alive[q] else None
        if lens is not None:
            c.res_after[q] = lens[0]
            live = [t for t in range(s, s + len(rs.scopes)) if c.scope_alive[t]]
            assert len(live) == len(lens[1]), (L.name, q)
            for t, v in zip(live, lens[1]):
                c.scope_after[t] = v
        s += len(rs.scopes)
    c.varints = lambda before, after: [(sov(b), sov(a) if a is not None else 0) for b, a in zip(before, after)]   # noqa: E731
    # routing
    c.table = table_of(L.cfg)
    c.lookups, c.out = [], []
    for rs, tr in zip(L.res, L.tree["resourceSpans"]):
        key = routing_key(rs.hdr, (tr.get("resource") or {}).get("attributes") or [])
        lk = lookup(c.table, key) if key is not None and c.table[0] else None
        c.lookups.append(lk)
        m = lk.mask if lk is not None else 0
        c.out.append([k for k in range(64) if (m >> k) & 1] or [c.n_out - 1])
    return c


# ---------------------------------------------------------------------------
# resources over the scans

def _scan_res(r: int):
    """Resource r of a scan layout: one of the seven Resource messages; spanless
    when r % 3 == 2, else one scope of one minimal span."""
    return r % 7, r % 3 != 2, r - r // 3          # variant, has a span, spans before it


def _scan_keep(i):
    """Period 5 (spans 2 and 4 of every five are dropped)."""
    return np.isin(np.asarray(i) % 5, (0, 1, 3))


def _scan_build(rs):
    res, dec = [], Dec()
    for r in rs:
        v, has, i = _scan_res(r)
        sc = []
        if has:
            dec.keep.append(int(_scan_keep(i)))
            sc = [Scope([min_span(i)])]
        res.append(Res(VARIANTS[v][1], sc, schema_of(r)))
    dec.url_out, dec.tmpls, dec.sql_op = [0] * len(dec.keep), [""] * len(dec.keep), [0] * len(dec.keep)
    return res, dec


def lay_scan(R: int, cfg=CFG_A):
    """R resources cycling the seven Resource messages (period 7, so the four
    records one scan thread owns differ in length), spanless or with one
    minimal span, keep of period 5, three outputs."""
    res, dec = _scan_build(range(R))
    return Layout(f"scan.{R}", res, dec, cfg)


def _be7(v):
    v = np.asarray(v, dtype=np.int64)
    return ((v[:, None] >> (8 * np.arange(6, -1, -1))) & 0xFF).astype(np.uint8)


def _digits7(v):
    v = np.asarray(v, dtype=np.int64)
    return (v[:, None] // 10 ** np.arange(6, -1, -1) % 10 + 48).astype(np.uint8)


class BigScan:
    """lay_scan at a size where nothing may loop in Python per resource: the
    records repeat with period 105 (7 Resource messages x spanless every
    third x keep of period 5 over the 70 spans of a block), so the message is
    a (R // 105, block bytes) array with the indices patched in by column, an
    output is a column mask of it, and the last R % 105 resources come from
    the small builder."""
    big = True
    P = 105

    def __init__(self, R: int, cfg=CFG_A):
        self.name, self.cfg, self.R, self.marks = f"scan.{R}", cfg, R, {}
        P = self.P
        self.nb = R // P
        res, _ = _scan_build(range(P))
        self.arr, _ = self._tiled(res)
        # what the encoder writes: an absent Resource field comes out as 0A 00
        self.out, self.width = self._tiled([Res(x.hdr or b"", x.scopes, x.schema) for x in res])
        self.tail = Layout(self.name + ".tail", *_scan_build(range(self.nb * P, R)), cfg) if R % P else None
        self.msg = self.arr.tobytes() + (self.tail.msg if self.tail else b"")
        rr = np.arange(R, dtype=np.int64)
        self.has = rr % 3 != 2
        self.S = self.n = int(self.has.sum())
        self.keep = _scan_keep(np.arange(self.n)).astype(np.uint8)

    def _tiled(self, res):
        """(nb, block bytes) of the block's records with each row's indices patched in; the records' widths."""
        recs = [LEN(1, x.body()) for x in res]
        width = np.array([len(x) for x in recs], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(width)])
        arr = np.tile(np.frombuffer(b"".join(recs), dtype=np.uint8), (self.nb, 1))
        blk = np.arange(self.nb, dtype=np.int64) * self.P
        for j in range(self.P):
            v, has, i = _scan_res(j)
            at = recs[j].rfind(schema_of(j))
            assert at > 0
            arr[:, start[j] + at + 1:start[j] + at + 8] = _digits7(blk + j)
            if has:
                at = recs[j].find(bytes.fromhex(span_id(i)))
                assert at > 0
                rr = blk + j
                arr[:, start[j] + at + 1:start[j] + at + 8] = _be7(rr - rr // 3)
        return arr, width

    def columns(self):
        scope_resource = np.nonzero(self.has)[0].astype(np.uint32)
        return scope_resource, np.arange(self.n, dtype=np.uint32), scope_resource

    def decisions(self, mode="full"):
        return {} if mode == "identity" else {"keep": self.keep}

    def _alive(self, mode):
        """Which of a block's 105 records stay."""
        j = np.arange(self.P)
        i = j - j // 3
        return (j % 3 == 2) | _scan_keep(i) | (mode == "identity")

    def expected(self, mode="full", routed=True):
        names = router_of(self.cfg).pipelines + ["default"] if routed else [""]
        outs = VARIANT_OUT["A" if self.cfg is CFG_A else "B"]
        alive = self._alive(mode)
        tail = self.tail.expected(mode, routed) if self.tail else None
        res = []
        for k, name in enumerate(names):
            take = np.array([alive[j] and (not routed or k in outs[j % 7]) for j in range(self.P)])
            cols = np.repeat(take, self.width)
            b = self.out[:, cols].tobytes()
            cnt = int(take.sum()) * self.nb
            if tail:
                assert tail[k][0] == name
                b, cnt = b + tail[k][1], cnt + tail[k][2]
            res.append((name, b, cnt))
        return res

    def sample(self):
        """(a small layout of the first and last three resources, their records' slices of the message)."""
        rs = [0, 1, 2, self.R - 3, self.R - 2, self.R - 1]
        first = Layout(self.name + ".first", *_scan_build(rs[:3]), self.cfg)
        last = Layout(self.name + ".last", *_scan_build(rs[3:]), self.cfg)
        # the last three's decisions are those of their own span indices
        return first, last

    def census_into(self, c, mode):
        rr = np.arange(self.R, dtype=np.int64)
        c.records = np.array([len(LEN(1, x.body())) for x in _scan_build(range(self.P))[0]])[rr % self.P]
        c.res_alive = (rr % 3 == 2) | _scan_keep(rr - rr // 3) | (mode == "identity")
        return c


def lay_scan_big(R, cfg=CFG_A):
    return BigScan(R, cfg)


# ---------------------------------------------------------------------------
# spans over the span grid

class BigSpans:
    """SPAN_LANES + 65 minimal spans (32 bytes, 34 framed): resources of 8
    scopes of 1024 spans (34 KiB a scope, under kGpuScopeBytes), routed to two
    pipelines, then one default-routed resource with the last 65 spans, which
    only the second grid-stride iteration of enc_span_body sees.  Keep has
    period 3; no edits.  The expected outputs are the message's own bytes
    with the dropped spans masked out and the length varints rewritten."""
    big = True
    KS, G = 1024, 8

    def __init__(self):
        self.name, self.cfg, self.marks = "span.grid", CFG_A, {}
        KS, G = self.KS, self.G
        self.n = n = SPAN_LANES + 65
        per = KS * G
        self.full = full = SPAN_LANES // per
        assert full * per == SPAN_LANES
        nf = full * per
        row = LEN(2, min_span(0))
        self.row_w = w = len(row)
        at = row.find(bytes.fromhex(span_id(0)))
        rows = np.tile(np.frombuffer(row, dtype=np.uint8), (nf, 1))
        rows[:, at + 1:at + 8] = _be7(np.arange(nf))
        self.keep = (np.arange(n) % 3 != 0).astype(np.uint8)
        hdr = VARIANTS[1][1]
        sc_body = 2 + KS * w
        sc_head = b"\x12" + VAR(sc_body) + LEN(1, b"")
        sc_w = len(sc_head) + KS * w
        body = len(LEN(1, hdr)) + G * sc_w + len(LEN(3, schema_of(0)))
        head = b"\x0A" + VAR(body) + LEN(1, hdr)
        W = len(head) + G * sc_w + 10
        arr = np.zeros((full, W), dtype=np.uint8)
        arr[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
        rows3 = rows.reshape(full, G, KS * w)
        for g in range(G):
            o = len(head) + g * sc_w
            arr[:, o:o + len(sc_head)] = np.frombuffer(sc_head, dtype=np.uint8)
            arr[:, o + len(sc_head):o + sc_w] = rows3[:, g]
        arr[:, W - 10:W - 8] = (0x1A, 8)
        arr[:, W - 8] = ord("r")
        arr[:, W - 7:] = _digits7(np.arange(full))
        self.arr, self.head, self.sc_head, self.sc_w, self.W = arr, head, sc_head, sc_w, W
        d = Dec(nf)
        d.keep = self.keep[nf:].tolist()
        spans = [min_span(nf + j) for j in range(65)]
        d.url_out, d.tmpls, d.sql_op = [0] * 65, [""] * 65, [0] * 65
        self.tail = Layout("span.grid.tail", [Res(VARIANTS[2][1], [Scope(spans)], schema_of(full))], d, CFG_A)
        self.msg = arr.tobytes() + self.tail.msg
        self.R, self.S = full + 1, full * G + 1
        self._kept = None

    def columns(self):
        scope = np.concatenate([np.repeat(np.arange(self.full * self.G, dtype=np.uint32), self.KS),
                                np.full(65, self.full * self.G, dtype=np.uint32)])
        scope_resource = np.concatenate([np.repeat(np.arange(self.full, dtype=np.uint32), self.G),
                                         np.array([self.full], dtype=np.uint32)])
        return scope_resource[scope], scope, scope_resource

    def decisions(self, mode="full"):
        return {} if mode == "identity" else {"keep": self.keep}

    @staticmethod
    def _put_varint(arr, mask, col, width, v):
        for b in range(width):
            part = v >> (7 * b)
            arr[:, col + b] = (part & 0x7F) | (((part >> 7) > 0).astype(np.int64) << 7)
            mask[:, col + b] = (part > 0) | (b == 0)

    def _kept_bytes(self):
        if self._kept is None:
            full, G, KS, w = self.full, self.G, self.KS, self.row_w
            arr = self.arr.copy()
            mask = np.ones(arr.shape, dtype=bool)
            kp = self.keep[:full * G * KS].astype(bool).reshape(full, G, KS)
            cnt = kp.sum(axis=2).astype(np.int64)
            assert cnt.min() > 0                      # no scope is emptied
            sb = 2 + cnt * w
            vw = len(self.sc_head) - 3                # the scope length's bytes in the message
            rb = np.full(full, len(LEN(1, VARIANTS[1][1])) + 10, dtype=np.int64)
            for g in range(G):
                o = len(self.head) + g * self.sc_w
                self._put_varint(arr, mask, o + 1, vw, sb[:, g])
                mask[:, o + len(self.sc_head):o + self.sc_w] = np.repeat(kp[:, g], w, axis=1)
                rb += 1 + np.array([sov(x) for x in sb[:, g]]) + sb[:, g]
            self._put_varint(arr, mask, 1, len(self.head) - 1 - len(LEN(1, VARIANTS[1][1])), rb)
            self._kept = arr[mask].tobytes()
        return self._kept

    def expected(self, mode="full", routed=True):
        body = self.arr.tobytes() if mode == "identity" else self._kept_bytes()
        tail = self.tail.expected(mode, routed)
        if not routed:
            return [("", body + tail[0][1], self.full + tail[0][2])]
        assert [t[0] for t in tail] == ["p0", "p1", "default"] and tail[0][2] == tail[1][2] == 0
        return [("p0", body, self.full), ("p1", body, self.full), tail[2]]

    def sample(self):
        """The first three resources and the last two full ones with the tail, as small layouts."""
        per = self.KS * self.G

        def part(r0, r1, with_tail):
            d = Dec(r0 * per)
            res = []
            for r in range(r0, r1):
                res.append(Res(VARIANTS[1][1], [Scope([d.min(self.keep[d.i]) for _ in range(self.KS)]) for _ in range(self.G)],
                               schema_of(r)))
            if with_tail:
                res.append(Res(VARIANTS[2][1], [Scope([d.min(self.keep[d.i]) for _ in range(65)])], schema_of(self.full)))
            return Layout(f"{self.name}.{r0}", res, d, CFG_A)
        return part(0, 3, False), part(self.full - 2, self.full, True)

    def census_into(self, c, mode):
        i = np.arange(self.n, dtype=np.int64)
        c.span_iter = i // SPAN_LANES
        c.scope_bytes = self.sc_w - 1 - sov(2 + self.KS * self.row_w)
        return c


# ---------------------------------------------------------------------------
# spans per scope (write_record's chunks)

CHUNK_SCOPES = [0, 1, 63, 64, 65, 127, 128, 129, 200]
CHUNK_MASKS = {
    "all": lambda j: True, "none": lambda j: False, "lane63": lambda j: j == 63, "chunk1_lane0": lambda j: j == 64,
    "alternate": lambda j: j % 2 == 0, "middle_chunk_dropped": lambda j: not 64 <= j < 128,
}
CHUNK_EDITS = {0: (SET_ATTR, 0), 63: (RENAME, 1), 64: (SET_ATTR | RENAME, 6)}    # lane 0, lane 63, lane 0 of chunk 1


def lay_chunks(mask: str):
    """One resource with scopes of 0, 1, 63, 64, 65, 127, 128, 129 and 200 spans
    under one keep mask over each scope's lanes; the spans on lane 0, lane 63
    and lane 0 of the second chunk are edited (url_out 1, 2, 3; sql_op)."""
    d = Dec()
    scopes = []
    for t, k in enumerate(CHUNK_SCOPES):
        spans = []
        for j in range(k):
            kp = CHUNK_MASKS[mask](j)
            if j in CHUNK_EDITS:
                u, op = CHUNK_EDITS[j]
                spans.append(d.edited(kp, u, op, kind=3 if t % 2 else 2))
            else:
                spans.append(d.min(kp))
        scopes.append(Scope(spans, gg._str(1, "lib%d" % t), b"s%d" % t if t % 2 else b""))
    return Layout(f"chunks.{mask}", [Res(VARIANTS[0][1], scopes, schema_of(0))], d)


# ---------------------------------------------------------------------------
# removal rules

def lay_removal():
    """Resources with no scopes first, in the middle and last; [emptied scope,
    originally empty scope] (PAIR: the empty one and the resource stay); an
    originally empty scope alone (ALONE: stays); a resource whose every span
    is dropped between two kept ones (BETWEEN: removed)."""
    d = Dec()
    res = [Res(VARIANTS[0][1], [], schema_of(0)),
           Res(VARIANTS[1][1], [Scope([d.min(0), d.min(0)], gg._str(1, "emptied")), Scope([], gg._str(1, "empty"))], schema_of(1)),
           Res(VARIANTS[0][1], [Scope([d.min(1)])], schema_of(2)),
           Res(VARIANTS[2][1], [], schema_of(3)),
           Res(VARIANTS[1][1], [Scope([], gg._str(1, "alone"))], schema_of(4)),
           Res(VARIANTS[5][1], [Scope([d.min(1), d.min(0)])], schema_of(5)),
           Res(VARIANTS[0][1], [Scope([d.min(0)]), Scope([d.min(0), d.min(0)])], schema_of(6)),
           Res(VARIANTS[1][1], [Scope([d.min(0), d.min(1)])], schema_of(7)),
           Res(None, [], schema_of(8))]
    return Layout("removal.mixed", res, d, marks={"PAIR": 1, "ALONE": 4, "BETWEEN": 6, "SPANLESS": [0, 3, 8]})


def lay_all_dropped():
    """Every span dropped: every output is empty."""
    d = Dec()
    res = [Res(VARIANTS[v][1], [Scope([d.min(0) for _ in range(1 + v)])], schema_of(v)) for v in range(5)]
    return Layout("removal.all_dropped", res, d)


def lay_empty_message():
    """R = 0."""
    return Layout("removal.empty_message", [], Dec())


# ---------------------------------------------------------------------------
# length varints

VARINT_EDGES = [127, 128, 16383, 16384]
SMALL_HDR = res_hdr({"a": "b"})


def lay_varint_bodies():
    """For N in 127, 128, 16383, 16384: a scope body of N bytes, a resource
    body of N bytes and a verbatim span of N bytes (its frame's varint), each
    in a resource of its own.  (A 2^28 body is out of reach at test size.)"""
    d = Dec()
    res, marks = [], {"scope": [], "res": [], "span": []}
    for N in VARINT_EDGES:
        i = d.add()
        res.append(Res(VARIANTS[0][1], [Scope([pad_span(i, N - 2 - 1 - sov(N - 4))])], schema_of(len(res))))
        marks["scope"].append(len(res) - 1)
        i = d.add()

        def make(k, i=i, r=len(res)):
            return Res(SMALL_HDR, [Scope([gg.span(host.span(name="f", kind=1, trace_id=TID, span_id=span_id(i),
                                                            attributes={"pad": "p" * k}))])], schema_of(r))
        k = next(k for k in range(max(0, N - 300), N) if len(make(k).body()) >= N)
        assert len(make(k).body()) == N, (N, len(make(k).body()))
        res.append(make(k))
        marks["res"].append(len(res) - 1)
        i = d.add()
        res.append(Res(VARIANTS[2][1], [Scope([pad_span(i, N)])], schema_of(len(res))))
        marks["span"].append(len(res) - 1)
    return Layout("varint.bodies", res, d, marks=marks)


def lay_varint_drop():
    """Scope and resource bodies of 128 and 16384 bytes that fall to the
    shorter varint once their second span (a minimal one) is dropped."""
    d = Dec()
    res, marks = [], {"scope": [], "res": []}
    for N in (128, 16384):
        i = d.add()
        first = pad_span(i, N - 2 - 34 - 1 - sov(N - 40))
        res.append(Res(VARIANTS[0][1], [Scope([first, d.min(0)])], schema_of(len(res))))
        marks["scope"].append(len(res) - 1)
        i, j = d.add(), d.add(0)

        def make(k, i=i, j=j, r=len(res)):
            return Res(SMALL_HDR, [Scope([gg.span(host.span(name="f", kind=1, trace_id=TID, span_id=span_id(i),
                                                            attributes={"pad": "p" * k})), min_span(j)])], schema_of(r))
        k = next(k for k in range(0, N) if len(make(k).body()) >= N)
        assert len(make(k).body()) == N, (N, len(make(k).body()))
        res.append(make(k))
        marks["res"].append(len(res) - 1)
    return Layout("varint.drop", res, d, marks=marks)


def lay_varint_res2m():
    """Resource bodies of 2097151 and 2097152 bytes (three and four length
    bytes), each 33 scopes of one padded span, every scope under kGpuScopeBytes."""
    d = Dec()
    res = []
    for N in (2097151, 2097152):
        ids = [d.add() for _ in range(33)]
        big = [Scope([pad_span(i, 63600)], gg._str(1, "l")) for i in ids[:32]]

        def make(k, big=big, i=ids[32], r=len(res)):
            return Res(VARIANTS[0][1], big + [Scope([gg.span(host.span(name="f", kind=1, trace_id=TID, span_id=span_id(i),
                                                                       attributes={"pad": "p" * k}))])], schema_of(r))
        k = N - len(make(0).body())
        while len(make(k).body()) > N:
            k -= 1
        assert len(make(k).body()) == N
        res.append(make(k))
    return Layout("varint.res2m", res, d)


# ---------------------------------------------------------------------------
# lane-strided copies

COPY_HDR = [0, 2, 63, 64, 65, 127, 128]      # (no Resource / InstrumentationScope payload is 1 byte long)
COPY_URL = [0, 1, 63, 64, 65, 127, 128]


def lay_copy_lengths():
    """Resource header, scope header, scope schema_url and resource schema_url
    of 0 / 1 (2 for the headers) / 63 / 64 / 65 / 127 / 128 bytes; then
    Resource and scope fields present with length 0 beside absent ones (both
    come out as 0A 00)."""
    d = Dec()
    res = []
    for q, (h, u) in enumerate(zip(COPY_HDR, COPY_URL)):
        u2 = COPY_URL[(q + 3) % len(COPY_URL)]
        url = (b"r%07d" % q + b"u" * 200)[:u]
        res.append(Res(hdr_of(h, 1), [Scope([d.min()], hdr_of(h, 2), b"x" * u2)], url))
    res += [Res(b"", [Scope([d.min()], b""), Scope([d.min()], None)], schema_of(7)),
            Res(None, [Scope([d.min()], None), Scope([d.min()], b"")], schema_of(8))]
    return Layout("copy.lengths", res, d, marks={"present_absent": [7, 8]})


# ---------------------------------------------------------------------------
# the two sources of the layout arrays

def lay_scope_64k():
    """A scope of exactly kGpuScopeBytes and one of kGpuScopeBytes + 1 among
    small ones: the second sends the decode's scope walk back to the host, so
    the encoder takes its layout arrays from the upload."""
    d = Dec()
    G = K.kGpuScopeBytes

    def scope_of(total):
        i = d.add()
        sp = pad_span(i, total - 2 - 1 - sov(total - 6))
        sc = Scope([sp])
        assert len(sc.body()) == total
        return sc
    res = [Res(VARIANTS[0][1], [Scope([d.min()]), scope_of(G), Scope([d.min(0), d.min()])], schema_of(0)),
           Res(VARIANTS[1][1], [Scope([d.min()]), scope_of(G + 1), Scope([d.min()])], schema_of(1)),
           Res(VARIANTS[2][1], [Scope([d.min(), d.min(0)])], schema_of(2))]
    return Layout("source.scope_64k", res, d)


def lay_scope_at_64k():
    """Every scope at or under kGpuScopeBytes (one exactly on it): the GPU walk keeps the layout arrays."""
    d = Dec()
    G = K.kGpuScopeBytes
    i = d.add()
    sc = Scope([pad_span(i, G - 2 - 1 - sov(G - 6))])
    assert len(sc.body()) == G
    res = [Res(VARIANTS[0][1], [Scope([d.min()]), sc, Scope([d.min(0), d.min()])], schema_of(0)),
           Res(VARIANTS[2][1], [Scope([d.min(), d.min(0)])], schema_of(1))]
    return Layout("source.scope_at_64k", res, d)


# ---------------------------------------------------------------------------
# routing

def _k8s(ns, name, kind="deployment", **more):
    at = {}
    if ns is not None:
        at["k8s.namespace.name"] = ns
    at["k8s.%s.name" % kind] = name
    at.update(more)
    return res_hdr(at)


def _routed(name, hdrs, cfg, marks=None):
    d = Dec()
    res = [Res(h, [Scope([d.min(), d.min(q % 2)])], schema_of(q)) for q, h in enumerate(hdrs)]
    return Layout(name, res, d, cfg, marks)


CFG_63 = {"datastreams": [_stream("p%02d" % k, [_src("prod", "Deployment", "w%02d" % k), _src("prod", "StatefulSet", "all")] +
                                  ([_src("prod", "DaemonSet", "both")] if k in (3, 40) else [])) for k in range(63)]}
CFG_64 = {"datastreams": CFG_63["datastreams"] + [_stream("p63", [_src("prod", "Deployment", "w63")])]}


def lay_63_pipelines():
    """63 pipelines: hits on pipelines 0, 31, 32 and 62, a default resource
    (bit 63), a source named by two data streams and one named by all 63."""
    hdrs = [_k8s("prod", "w00"), _k8s("prod", "w31"), _k8s("prod", "w32"), _k8s("prod", "w62"), _k8s("prod", "nobody"),
            _k8s("prod", "both", "daemonset"), _k8s("prod", "all", "statefulset")]
    return _routed("route.63_pipelines", hdrs, CFG_63)


def lay_64_pipelines():
    """64 pipelines: both encoders refuse the router."""
    return _routed("route.64_pipelines", [_k8s("prod", "w00"), _k8s("prod", "w63")], CFG_64)


def lay_no_source():
    """A router with a pipeline and no source (a table of two empty slots)."""
    return _routed("route.no_source", [_k8s("prod", "w-one"), None], {"datastreams": [_stream("p0", [])]})


def lay_no_pipeline():
    """Router({}): one output, default."""
    return _routed("route.no_pipeline", [_k8s("prod", "w-one"), None, VARIANTS[1][1]], {})


def lay_empty_list():
    """A router whose data stream list is empty: the two-slot table is built and read, one output."""
    return _routed("route.empty_list", [_k8s("prod", "w-one"), None, VARIANTS[1][1]], {"datastreams": []})


def lay_one_route():
    """One route: the 4-slot table."""
    return _routed("route.one", [_k8s("prod", "w-one"), _k8s("prod", "w-two"), _k8s("dev", "w-one")],
                   {"datastreams": [_stream("p0", [_src("prod", "Deployment", "w-one")])]})


def _find_chain_names():
    """Names w000, w001, ... (all of one length) whose keys prod/deployment/NAME
    fall, in the 16-slot table of five routes: four on one home slot X in
    2..11 (three routes and an absent key) and three on the last slot (two
    routes, the second wrapping to slot 0, and an absent key)."""
    slots = 1 << table_bits(5)
    by = {}
    for q in range(1000):
        name = "w%03d" % q
        by.setdefault(fnv1a(b"prod/deployment/" + name.encode()) & (slots - 1), []).append(name)
    x = next(s for s in range(2, slots - 4) if len(by.get(s, [])) >= 4)
    assert len(by.get(slots - 1, [])) >= 3
    return slots, x, by[x][:4], by[slots - 1][:3]


CHAIN_SLOTS, CHAIN_HOME, CHAIN_X, CHAIN_LAST = _find_chain_names()
CFG_CHAINS = {"datastreams": [_stream("p%d" % k, [_src("prod", "Deployment", nm)])
                              for k, nm in enumerate(CHAIN_X[:3] + CHAIN_LAST[:2])]}


def lay_chains():
    """A chain of three routes sharing a home slot, each looked up; a chain on
    the table's last slot that wraps to slot 0; absent keys (of an occupant's
    exact length) that walk each chain to the empty slot behind it."""
    names = CHAIN_X[:3] + CHAIN_LAST[:2] + [CHAIN_X[3], CHAIN_LAST[2]]
    return _routed("route.chains", [_k8s("prod", nm) for nm in names], CFG_CHAINS,
                   marks={"chain": [0, 1, 2], "wrap": [3, 4], "absent": 5, "absent_wrap": 6})


CFG_STRINGS = {"datastreams": [
    _stream("empty-ns", [_src("", "Deployment", "x")]),
    _stream("empty-name", [_src("prod", "Deployment", "")]),
    _stream("split", [_src("x/deployment/y", "Deployment", "z")])]}


def lay_strings():
    """Namespace "" against a source whose namespace is ""; a namespace that is
    not a string (Str() is ""); a workload name "" (default, though a source
    has that key); two splits of one key string, routed alike."""
    hdrs = [_k8s("", "x"), _k8s(5, "x"), _k8s("prod", ""), _k8s("x/deployment/y", "z"), _k8s("x", "y/deployment/z"),
            _k8s("prod", "x")]
    return _routed("route.strings", hdrs, CFG_STRINGS)


# ---------------------------------------------------------------------------

SCAN_SMALL = [1, 4, 5, TILE - 1, TILE, TILE + 1]
SCAN_BIG = [TOP_EDGE, TOP_EDGE + 1, WRITE_WAVES + 1]
SMALL = {
    **{f"scan.{R}": (lambda R=R: lay_scan(R, CFG_B if R == TILE + 1 else CFG_A)) for R in SCAN_SMALL},
    **{f"chunks.{m}": (lambda m=m: lay_chunks(m)) for m in CHUNK_MASKS},
    "removal.mixed": lay_removal, "removal.all_dropped": lay_all_dropped, "removal.empty_message": lay_empty_message,
    "varint.bodies": lay_varint_bodies, "varint.drop": lay_varint_drop, "varint.res2m": lay_varint_res2m,
    "copy.lengths": lay_copy_lengths, "source.scope_64k": lay_scope_64k, "source.scope_at_64k": lay_scope_at_64k,
    "route.63_pipelines": lay_63_pipelines, "route.no_source": lay_no_source, "route.no_pipeline": lay_no_pipeline,
    "route.empty_list": lay_empty_list,
    "route.one": lay_one_route, "route.chains": lay_chains, "route.strings": lay_strings,
}
LARGE = {**{f"scan.{R}": (lambda R=R: lay_scan_big(R)) for R in SCAN_BIG}, "span.grid": BigSpans}
REFUSED = {"route.64_pipelines": lay_64_pipelines}
_built: dict = {}


def layout(name):
    """The named layout, built once (nothing writes to it)."""
    if name not in _built:
        _built[name] = {**SMALL, **LARGE, **REFUSED}[name]()
    return _built[name]


def drop(name):
    """Forget a large layout (tens of megabytes)."""
    _built.pop(name, None)
