"""The OTLP encoder (encode_kernel.hip, encode_gpu in otlp_encode_host.cpp, and the
host encoder otlp_encode.cpp) on hand-laid messages at every scan, wave and
routing seam (tests/encode_layouts.py).

CPU: the constants the layouts were drawn for; each layout's census
assertion that it sits on its seam; expected() against the CPU seam
osehost_otlp_encode_sql with and without the router at 1 and 3 threads; the
numpy builder of the large layouts against the restatement on sampled
resources; the census of the route table against the product's table.
GPU: decode, check the decoder's counts and index columns, lay the decisions
into the outputs, ose_otlp_encode under three stage masks (all decisions,
keep alone, none) and, for the small layouts, four decoder options; the bytes
must equal expected() and come from the GPU encoder.
"""
import copy

import numpy as np
import pytest

from odigos_amd import native
from tests import encode_layouts as el
from tests import otlp_gogo as gg
from tests.encode_layouts import K, LEN, Dec, Layout, Res, Scope, census, layout

S = native
STAGES = {"full": S.STAGE_APPLY_KEEP | S.STAGE_TEMPLATE | S.STAGE_APPLY_SQLOP, "keep": S.STAGE_APPLY_KEEP, "identity": 0}
OPTIONS = [None, "otlp_host_resources", "otlp_host_scopes", "otlp_gpu_chain"]
ALL = sorted(el.SMALL) + sorted(el.LARGE)


def test_constants_as_designed():
    for name, v in el.DESIGNED.items():
        assert getattr(K, name) == v, f"{name} was retuned: redraw the layouts of tests/encode_layouts.py"
    assert (el.TILE, el.KPER, el.TOP_EDGE, el.WRITE_WAVES, el.SPAN_LANES) == (1024, 4, 262144, 65536, 2097152)
    assert (K.kEncFbSpan, K.kEncFbScope, K.kEncFbRes, K.kEncFbTmpl, K.kEncFbRoute, K.kEncFbWrite) == (1, 2, 4, 8, 16, 32)


# ---------------------------------------------------------------------------
# every layout sits on its seam

def _records(L):
    return [len(LEN(1, r.body())) for r in L.res]


def _scope_at(L, k):
    """(scope index, first span) of the first scope with k spans"""
    i = s = 0
    for r in L.res:
        for sc in r.scopes:
            if len(sc.spans) == k:
                return s, i
            i += len(sc.spans)
            s += 1
    raise AssertionError(k)


def _seam_scan(L, c):
    R = L.R
    assert c.n_out == 3 and c.tiles == -(-R // el.TILE)
    rec = np.array(_records(L)) if not L.big else c.records
    if R >= 4:   # the four resources of scan thread 0 differ in length
        assert len(set(rec[:4].tolist())) >= 3 and set(c.slot[:4].tolist()) == {0, 1, 2, 3}
    if R == 1:
        assert c.slot.tolist() == [0]
    if R == 5:
        assert c.slot[4] == 0 and R // el.KPER == 1          # a second thread's first slot
    if R in (el.TILE - 1, el.TILE):
        assert c.tiles == 1 and c.tile[-1] == 0 and (R - 1) // el.KPER == K.kEThreads - 1
    if R == el.TILE + 1:
        assert c.tiles == 2 and c.tile[-1] == 1 and c.tile[-2] == 0
        e = L.expected()
        assert e[1][2] == 0 and e[1][1] == b"" and e[0][2] and e[2][2]      # the middle output receives nothing
    assert c.top_trips == (2 if R > el.TOP_EDGE else 1)
    if R == el.TOP_EDGE:
        assert c.tiles == K.kEThreads
    if R == el.TOP_EDGE + 1:
        assert c.tiles == K.kEThreads + 1
    if R <= el.WRITE_WAVES:
        assert c.write_iters == 1
    if R == el.WRITE_WAVES + 1:
        assert c.write_iters == 2 and c.write_iter[-1] == 1 and c.write_iter[-2] == 0
    if R > el.TOP_EDGE:
        assert c.write_iters == 5 and c.write_iter[-1] == 4
    if R in (el.TILE + 1, el.TOP_EDGE + 1, el.WRITE_WAVES + 1):    # the resource past the edge has a record
        assert c.res_alive[R - 1] and (L.big or L.res[-1].scopes)
    if R >= 4:      # records removed among the ones that stay
        alive = np.asarray(c.res_alive)
        assert alive.any() and not alive.all()


def _seam_span_grid(L, c):
    assert L.n == el.SPAN_LANES + 65 and c.span_iters == 2 and L.n > K.kSpanStageMax
    assert (c.span_iter[:el.SPAN_LANES] == 0).all() and (c.span_iter[el.SPAN_LANES:] == 1).all()
    assert 0 < int(L.keep[el.SPAN_LANES:].sum()) < 65
    assert c.scope_bytes <= K.kGpuScopeBytes and 1000 < L.S < 5000
    assert 60e6 < len(L.msg) < 75e6


def _seam_chunks(L, c):
    mask = L.name.split(".")[1]
    assert [len(x) for x in c.chunks] == [0, 1, 1, 1, 2, 2, 2, 3, 4]
    by = {k: c.chunks[_scope_at(L, k)[0]] for k in el.CHUNK_SCOPES}
    full = list(range(64))
    if mask == "all":
        assert by[64] == [full] and by[65] == [full, [0]] and by[128] == [full, full] and by[129] == [full, full, [0]]
        assert by[63] == [full[:63]] and by[127] == [full, full[:63]] and by[200] == [full, full, full, full[:8]]
    if mask == "none":
        assert all(ch == [] for k in el.CHUNK_SCOPES for ch in by[k])
        assert c.scope_state == ["empty"] + ["emptied"] * 8 and c.res_alive == [True]
    if mask == "lane63":
        assert by[64] == [[63]] and by[65] == [[63], []] and by[200] == [[63], [], [], []] and by[63] == [[]]
    if mask == "chunk1_lane0":
        assert by[65] == [[], [0]] and by[129] == [[], [0], []] and by[64] == [[]]
    if mask == "alternate":
        assert by[129] == [full[::2], full[::2], [0]]
    if mask == "middle_chunk_dropped":
        assert by[200] == [full, [], full, full[:8]] and by[129] == [full, [], [0]] and by[128] == [full, []]
    # the edited spans: lane 0, lane 63, and lane 0 of the second chunk (the plan at a.edit + c + b with c > i0)
    for k in (65, 129, 200):
        s, i0 = _scope_at(L, k)
        assert L.url_out[i0] == 1 and L.url_out[i0 + 63] == 2 and L.url_out[i0 + 64] == 3
        assert L.sql_op[i0 + 63] == 1 and L.sql_op[i0 + 64] == 6
    if mask in ("all", "chunk1_lane0"):
        s, i0 = _scope_at(L, 129)
        assert L.keep[i0 + 64] and 0 in by[129][1]


def _seam_removal(L, c):
    if L.name == "removal.mixed":
        m = L.marks
        s0 = sum(len(r.scopes) for r in L.res[:m["PAIR"]])
        assert c.scope_state[s0:s0 + 2] == ["emptied", "empty"] and c.res_alive[m["PAIR"]]
        assert c.scope_alive[s0:s0 + 2] == [False, True]
        assert c.res_state[m["ALONE"]] == "spanless" and len(L.res[m["ALONE"]].scopes) == 1 and c.res_alive[m["ALONE"]]
        b = m["BETWEEN"]
        assert c.res_state[b - 1:b + 2] == ["kept", "emptied", "kept"] and not c.res_alive[b]
        assert m["SPANLESS"] == [0, 3, L.R - 1] and all(not L.res[q].scopes and c.res_alive[q] for q in m["SPANLESS"])
    elif L.name == "removal.all_dropped":
        assert c.res_state == ["emptied"] * L.R and all(e[1] == b"" and e[2] == 0 for e in L.expected())
        assert L.expected("identity")[0][2] > 0
    else:
        assert L.R == L.S == L.n == 0 and L.msg == b""


def _seam_varint(L, c):
    m = L.marks
    scope_of = lambda q: sum(len(r.scopes) for r in L.res[:q])   # noqa: E731
    if L.name == "varint.bodies":
        assert [c.scope_before[scope_of(q)] for q in m["scope"]] == el.VARINT_EDGES
        assert [c.res_before[q] for q in m["res"]] == el.VARINT_EDGES
        assert [len(L.res[q].scopes[0].spans[0]) for q in m["span"]] == el.VARINT_EDGES
        assert [el.sov(x) for x in el.VARINT_EDGES] == [1, 2, 2, 3]
    elif L.name == "varint.drop":
        sc = [scope_of(q) for q in m["scope"]]
        assert [c.scope_before[s] for s in sc] == [128, 16384] and [c.scope_after[s] for s in sc] == [94, 16350]
        assert [c.res_before[q] for q in m["res"]] == [128, 16384] and [c.res_after[q] for q in m["res"]] == [94, 16350]
        assert c.varints([128, 16384], [94, 16350]) == [(2, 1), (3, 2)]
    else:
        assert c.res_before == [2097151, 2097152] and c.varints(c.res_before, c.res_after) == [(3, 3), (4, 4)]
        assert [len(r.scopes) for r in L.res] == [33, 33] and max(c.scope_before) < K.kGpuScopeBytes


def _seam_copy(L, c):
    n = len(el.COPY_HDR)
    assert [len(r.hdr) for r in L.res[:n]] == el.COPY_HDR == [len(r.scopes[0].hdr) for r in L.res[:n]]
    assert [len(r.schema) for r in L.res[:n]] == el.COPY_URL
    assert sorted(len(r.scopes[0].schema) for r in L.res[:n]) == el.COPY_URL
    a, b = (L.res[q] for q in L.marks["present_absent"])
    assert (a.hdr, b.hdr) == (b"", None) and [s.hdr for s in a.scopes + b.scopes] == [b"", None, None, b""]
    # present with length 0 and absent are written alike
    t = L.expected("identity", routed=False)[0][1]
    assert t.count(b"\x0A\x00\x12") >= 2


def _seam_source(L, c):
    G = K.kGpuScopeBytes
    if L.name == "source.scope_64k":
        assert sorted(c.scope_before)[-2:] == [G, G + 1] and sorted(c.scope_before)[0] < 100
    else:
        assert max(c.scope_before) == G


def _seam_route(L, c):
    bits, tab, keys = c.table
    name = L.name.split(".", 1)[1]
    ends = [lk.end if lk is not None else None for lk in c.lookups]
    if name == "63_pipelines":
        assert c.n_out == 64 and c.out == [[0], [31], [32], [62], [63], [3, 40], list(range(63))]
    elif name == "no_source":
        assert c.n_out == 2 and bits == 1 and (tab["klen"] == el.EMPTY).all() and ends == ["empty", None] and c.out == [[1], [1]]
    elif name == "no_pipeline":
        assert c.n_out == 1 and bits == 0 and c.lookups == [None] * 3 and c.out == [[0]] * 3      # route_bits 0: no lookup
    elif name == "empty_list":
        assert c.n_out == 1 and bits == 1 and ends == ["empty", None, "empty"] and c.out == [[0]] * 3
    elif name == "one":
        assert bits == 2 and len(tab) == 4 and ends[0] == "hit" and ends[1:] == ["empty", "empty"] and c.out == [[0], [1], [1]]
    elif name == "chains":
        m = L.marks
        assert len(tab) == el.CHAIN_SLOTS == 16
        chain = [c.lookups[q] for q in m["chain"]]
        assert all(lk.home == el.CHAIN_HOME and lk.end == "hit" and not lk.wrapped for lk in chain)
        assert sorted(lk.probes for lk in chain) == [1, 2, 3]
        wrap = [c.lookups[q] for q in m["wrap"]]
        assert all(lk.home == 15 and lk.end == "hit" for lk in wrap) and sorted(lk.probes for lk in wrap) == [1, 2]
        assert sorted(lk.wrapped for lk in wrap) == [False, True]
        a, w = c.lookups[m["absent"]], c.lookups[m["absent_wrap"]]
        assert (a.home, a.probes, a.end, a.wrapped, a.same_len_miss) == (el.CHAIN_HOME, 4, "empty", False, 3)
        assert (w.home, w.probes, w.end, w.wrapped, w.same_len_miss) == (15, 3, "empty", True, 2)
        assert [o for o in c.out[:5]] == [[0], [1], [2], [3], [4]] and c.out[5:] == [[5], [5]]
    else:
        assert c.out == [[0], [0], [3], [2], [2], [3]] and c.lookups[2] is None
        assert b"/deployment/x" in keys and b"prod/deployment/" in keys and ends[5] == "empty"


SEAMS = {"scan": _seam_scan, "span": _seam_span_grid, "chunks": _seam_chunks, "removal": _seam_removal,
         "varint": _seam_varint, "copy": _seam_copy, "source": _seam_source, "route": _seam_route}


@pytest.mark.parametrize("name", ALL)
def test_layout_sits_on_its_seam(name):
    L = layout(name)
    SEAMS[name.split(".")[0]](L, census(L))
    rs, sc, sr = L.columns()
    assert (len(rs), len(sc), len(sr)) == (L.n, L.n, L.S)


def test_scan_variants_route_as_listed():
    """The outputs the large scan layouts assume for the seven Resource messages are the census's."""
    for cfg, key in ((el.CFG_A, "A"), (el.CFG_B, "B")):
        c = census(el.lay_scan(7, cfg))
        assert c.out == el.VARIANT_OUT[key]


# ---------------------------------------------------------------------------
# the route table

@pytest.mark.parametrize("cfg", ["CFG_A", "CFG_B", "CFG_63", "CFG_CHAINS", "CFG_STRINGS"])
def test_route_table_census_equals_the_real_table(cfg):
    cfg = getattr(el, cfg)
    bits, tab, keys = el.real_table(el.router_of(cfg))
    rbits, rtab, rkeys = el.table_of(cfg)
    assert (bits, keys[:len(rkeys)]) == (rbits, rkeys) and len(tab) == len(rtab)
    for f in ("h", "koff", "klen", "mask"):
        occ = rtab["klen"] != el.EMPTY
        np.testing.assert_array_equal(tab[f][occ | (f == "klen")], rtab[f][occ | (f == "klen")])
    assert el.pipelines_of(cfg) == el.router_of(cfg).pipelines
    # every key is found where the census says, with the product's pipelines
    for key, mask in el.route_entries(cfg):
        lk = el.lookup((rbits, rtab, rkeys), key)
        assert lk.end == "hit" and lk.mask == mask


def test_route_tables_without_routes():
    bits, tab, keys = el.real_table(el.router_of({"datastreams": [el._stream("p0", [])]}))
    assert bits == 1 and len(tab) == 2 and (tab["klen"] == el.EMPTY).all()
    bits, tab, keys = el.real_table(el.router_of({}))          # no "datastreams": no table, route_bits 0
    assert bits == 0 and len(tab) == 0
    bits, tab, keys = el.real_table(el.router_of(el.CFG_64))   # refused by the encoders: no table
    assert bits == 0 and len(tab) == 0


# ---------------------------------------------------------------------------
# the host encoder on the same seams

def _seam(L, mode, routed, threads):
    from tests.test_otlp_sqlop import _seam as seam
    d = L.decisions(mode)
    return seam(L.msg, d.get("keep"), d.get("url_out"), d.get("tmpls"), d.get("sql_op"),
                router=el.router_of(L.cfg) if routed else None, threads=threads)


@pytest.mark.parametrize("name", ALL)
def test_expected_equals_the_cpu_seam(name):
    L = layout(name)
    for routed in (True, False):
        want = L.expected("full", routed)
        for threads in (1, 3):
            got = _seam(L, "full", routed, threads)
            assert [(g[0], len(g[1]), g[2]) for g in got] == [(w[0], len(w[1]), w[2]) for w in want]
            assert got == want
    if not L.big:
        for mode in ("keep", "identity"):
            assert _seam(L, mode, True, 3) == L.expected(mode, True)
    else:
        assert _seam(L, "identity", True, 3) == L.expected("identity", True)
        el.drop(name)


@pytest.mark.parametrize("name", sorted(el.LARGE))
def test_numpy_builder_equals_the_restatement(name):
    L = layout(name)
    first, last = L.sample()
    assert L.msg.startswith(first.msg) and L.msg.endswith(last.msg)
    for mode in ("full", "identity"):      # (no edits in the large layouts: keep alone is the same call)
        for routed in (True, False):
            want = L.expected(mode, routed)
            for part, at in ((first, bytes.startswith), (last, bytes.endswith)):
                sub = part.expected(mode, routed)
                assert [w[0] for w in want] == [s[0] for s in sub]
                for w, s in zip(want, sub):
                    assert at(w[1], s[1]) and w[2] >= s[2]
    # the counts: every resource is in exactly the outputs its Resource message routes to
    ident = L.expected("identity", True)
    assert sum(e[2] for e in L.expected("identity", False)) == L.R <= sum(e[2] for e in ident)
    el.drop(name)


def test_scope_dropped_attributes_count_reaches_the_json_tree():
    """copy.lengths' two-byte InstrumentationScope is dropped_attributes_count
    alone; the host's OTLP/JSON writer left the field out, so the processors'
    JSON output lost it (the encoders copy it)."""
    from tests.test_otlp import _pb_to_json, _roundtrip
    L = layout("copy.lengths")
    assert L.res[1].scopes[0].hdr == b"\x20\x01"
    sc = L.tree["resourceSpans"][1]["scopeSpans"][0]["scope"]
    assert int(sc["droppedAttributesCount"]) == 1
    assert _roundtrip(L.tree) == L.tree and _pb_to_json(gg.marshal_traces(L.tree)) == L.tree


def test_64_pipelines_are_refused_by_the_host_encoder():
    L = layout("route.64_pipelines")
    assert len(el.router_of(L.cfg).pipelines) == 64
    with pytest.raises(native.OseError) as e:
        _seam(L, "full", True, 1)
    assert e.value.code == S.OSE_EINVAL and "63 pipelines" in str(e.value)
    assert _seam(L, "full", False, 1) == L.expected("full", False)


# ---------------------------------------------------------------------------
# GPU

def _engine():
    from tests.test_otlp_sqlop import _sql_engine
    return _sql_engine({})


def _lay_decisions(ob, L):
    """keep / url_out / sql_op / the templates of the layout into the batch's outputs"""
    import torch
    n = L.n
    dev = ob.o["keep"].device

    def put(name, a):
        a = np.array(a, copy=True).view(np.uint8).reshape(-1)
        if len(a):
            ob.o[name][:len(a)].copy_(torch.from_numpy(a).to(dev))
    put("keep", L.keep)
    for name in ("url_out", "sql_op"):
        ob.o[name][:n].zero_()
    used = 0
    if not L.big:
        put("url_out", L.url_out)
        put("sql_op", L.sql_op)
        refs = np.zeros((n, 2), dtype=np.uint32)
        arena = b""
        for i, t in enumerate(L.tmpls):
            refs[i] = (len(arena), len(t.encode()))
            arena += t.encode()
        put("tmpl", refs)
        put("tmpl_arena", np.frombuffer(arena, dtype=np.uint8))
        used = len(arena)
    else:
        ob.o["tmpl"][:8 * n].zero_()
    ob.o["used"][0] = used
    torch.cuda.synchronize()


def _decode(eng, L):
    from odigos_amd.batch import OtlpBatch
    ob = OtlpBatch(eng, L.msg, tmpl_cap=4096)
    assert (ob.cols.n_spans, ob.cols.n_scopes, ob.cols.n_resources) == (L.n, L.S, L.R), L.name
    got = ob.download()
    rs, sc, sr = L.columns()
    np.testing.assert_array_equal(got["resource"].view(np.uint32)[:L.n] if L.n else rs, rs)
    np.testing.assert_array_equal(got["scope"].view(np.uint32)[:L.n] if L.n else sc, sc)
    np.testing.assert_array_equal(got["scope_resource"].view(np.uint32)[:L.S] if L.S else sr, sr)
    _lay_decisions(ob, L)
    return ob


def _same(got, want, what):
    assert [(g[0], len(g[1]), g[2]) for g in got] == [(w[0], len(w[1]), w[2]) for w in want], what
    for g, w in zip(got, want):
        assert g[1] == w[1], (what, g[0])


def _encode_and_check(ob, L, modes=el.MODES, unrouted=False, what=""):
    router = el.router_of(L.cfg)
    for mode in modes:
        _same(ob.encode(STAGES[mode], S.GROUP_TRACE_ID, router), L.expected(mode, True), (L.name, mode, what))
        assert ob.encode_path == {"gpu": True, "fallback": 0}, (L.name, mode, what)
        if unrouted:
            _same(ob.encode(STAGES[mode]), L.expected(mode, False), (L.name, mode, what, "no router"))
            assert ob.encode_path == {"gpu": True, "fallback": 0}, (L.name, mode, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(el.SMALL))
def test_gpu_encode_small_layout(name):
    L = layout(name)
    eng = _engine()
    for opt in OPTIONS:
        if opt:
            eng.set_option(opt, 1)
        ob = _decode(eng, L)
        _encode_and_check(ob, L, unrouted=opt is None, what=opt)
        ob.close()
        if opt:
            eng.set_option(opt, 0)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(el.LARGE))
def test_gpu_encode_large_layout(name):
    L = layout(name)
    eng = _engine()
    ob = _decode(eng, L)
    _encode_and_check(ob, L)
    ob.close()
    eng.close()
    el.drop(name)


@pytest.mark.gpu
def test_gpu_encode_64_pipelines_goes_to_the_host():
    """otlp_encode.cpp refuses a router of more than 63 pipelines (OSE_EINVAL,
    "router: more than 63 pipelines"); the GPU encoder declines it unseen and
    the call gives the host encoder's error."""
    L = layout("route.64_pipelines")
    eng = _engine()
    ob = _decode(eng, L)
    ob.encode_path = {}
    with pytest.raises(native.OseError) as cpu:
        _seam(L, "full", True, 1)
    with pytest.raises(native.OseError) as gpu:
        ob.encode(STAGES["full"], S.GROUP_TRACE_ID, el.router_of(L.cfg))
    assert gpu.value.code == cpu.value.code == S.OSE_EINVAL and "63 pipelines" in str(gpu.value)
    assert not ob.encode_path.get("gpu")
    # the same batch without the router is the GPU encoder's
    _same(ob.encode(STAGES["full"]), L.expected("full", False), "no router")
    assert ob.encode_path == {"gpu": True, "fallback": 0}
    ob.close()
    eng.close()


def _fallback_layouts():
    """(layout, stage mode, the kEncFb* bit or 0)"""
    a = el.res_hdr({"k8s.namespace.name": "prod", "service.name": "m"})
    b = el.res_hdr({"k8s.deployment.name": "w-one"})
    out = []
    # a merged Resource: two field-1 messages (the host merges them, and routes the merged one)
    d = Dec()

    class Merged(Res):
        def body(self):
            return LEN(1, a) + Res.body(self)
    out.append((Layout("fallback.merged_resource", [Res(el.VARIANTS[0][1], [Scope([d.min()])], b"r0"),
                                                   Merged(b, [Scope([d.min(), d.min(0)])], b"r1")], d), "full", K.kEncFbRes))
    # a merged scope
    d = Dec()

    class MergedScope(Scope):
        def body(self):
            return LEN(1, gg._str(1, "lib")) + Scope.body(self)
    out.append((Layout("fallback.merged_scope", [Res(el.VARIANTS[1][1], [MergedScope([d.min(), d.min(0)], gg._str(2, "v1")),
                                                                         Scope([d.min()])], b"r0")], d), "full", K.kEncFbScope))
    # a routing KeyValue with its key field twice (the last one counts)
    d = Dec()
    kv = gg._str(1, "x") + gg.key_value({"key": "k8s.namespace.name", "value": {"stringValue": "prod"}})
    hdr = LEN(1, kv) + gg._attrs(1, [{"key": "k8s.deployment.name", "value": {"stringValue": "w-one"}}])
    out.append((Layout("fallback.key_twice", [Res(hdr, [Scope([d.min()])], b"r0"),
                                              Res(el.VARIANTS[1][1], [Scope([d.min(0), d.min()])], b"r1")], d), "full", K.kEncFbRoute))
    # a span in google.protobuf's encoding (no parent id, no Status) that keep drops: skipped before the canonical check
    d = Dec()
    short = lambda i: gg._id(1, el.TID) + gg._id(2, el.span_id(i))   # noqa: E731
    sp = [d.min(), short(d.add(0)), d.min()]
    out.append((Layout("fallback.dropped_noncanonical", [Res(el.VARIANTS[0][1], [Scope(sp)], b"r0")], d), "keep", 0))
    return out


def test_fallback_layouts_on_the_host_encoder():
    for L, mode, bit in _fallback_layouts():
        for routed in (True, False):
            assert _seam(L, mode, routed, 1) == L.expected(mode, routed), L.name
    L = _fallback_layouts()[0][0]
    assert L.expected()[0][2] == 2       # the merged Resource routes to p0 with the other one


@pytest.mark.gpu
def test_gpu_encode_fallbacks():
    eng = _engine()
    router = el.router_of(el.CFG_A)
    for L, mode, bit in _fallback_layouts():
        ob = _decode(eng, L)
        _same(ob.encode(STAGES[mode], S.GROUP_TRACE_ID, router), L.expected(mode, True), L.name)
        if bit:
            assert not ob.encode_path["gpu"] and ob.encode_path["fallback"] & bit, (L.name, ob.encode_path)
        else:
            assert ob.encode_path == {"gpu": True, "fallback": 0}, L.name
            # kept, the same span goes to the host
            ob.o["keep"][:L.n].fill_(1)
            kept = copy.copy(L)
            kept.keep, kept._exp = np.ones(L.n, dtype=np.uint8), {}
            _same(ob.encode(STAGES[mode], S.GROUP_TRACE_ID, router), kept.expected(mode, True), L.name + " kept")
            assert not ob.encode_path["gpu"] and ob.encode_path["fallback"] & K.kEncFbSpan
        ob.close()
    eng.close()


@pytest.mark.gpu
def test_gpu_encode_reuse():
    """One engine: the tile-edge layout, a three-resource one, the tile-edge
    one again with keep inverted (the workspace, the output buffer and the
    pooled batch and encoder state are reused, larger then smaller); then one
    batch under two routers."""
    eng = _engine()
    big = layout(f"scan.{el.TILE + 1}")
    ob = _decode(eng, big)
    _encode_and_check(ob, big, what="first")
    ob.close()
    small = layout("route.one")
    assert small.R == 3
    ob = _decode(eng, small)
    _encode_and_check(ob, small, what="small after large")
    ob.close()
    inv = copy.copy(big)
    inv.keep, inv._exp = (1 - big.keep).astype(np.uint8), {}
    ob = _decode(eng, inv)
    _encode_and_check(ob, inv, what="keep inverted")
    # a second ose_otlp_encode on the same batch with other decisions
    _lay_decisions(ob, big)
    _encode_and_check(ob, big, what="keep restored")
    ob.close()
    a, b = el.lay_scan(5, el.CFG_A), el.lay_scan(5, el.CFG_B)
    assert a.msg == b.msg and a.expected() != b.expected()
    ob = _decode(eng, a)
    for L in (a, b, a):
        _encode_and_check(ob, L, what="two routers")
    ob.close()
    eng.close()
