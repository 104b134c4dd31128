"""The OTLP decoder (otlp_kernel.hip, otlp_sqlop_kernel.hip, pb_device.hpp and
the walk in otlp_host.cpp) on hand-laid wire forms at every seam
(tests/decode_layouts.py).

CPU: the constants the layouts were drawn for; each layout's census assertion
that it sits on its seam; the reference tree (google.protobuf) against the host
unmarshaler otlp_pb.cpp on the same non-canonical bytes, which the host pass
depends on; the host structural walk against the reference's index columns;
the malformed variants rejected by the host unmarshaler.
GPU: every layout decoded on a fresh engine (cold), again on the same engine
(warm) and under its engine options; every column equal to the host
columniser's over the reference tree, db_flags / db_query / res_sql_ok
included; host_spans exactly the census's; ose_otlp_walk_info equal to the
census; for one layout per family SAMPLE|TEMPLATE|SIZE on the decoded columns
against the oracle chain; the malformed variants OSE_EINVAL, and a good message
decoded right after.  Every comparison is exact.
"""
import numpy as np
import pytest

from odigos_amd import host, native
from tests import decode_layouts as dl
from tests.decode_layouts import K, LAYOUTS, census
from tests.test_otlp import _arr, _compare, _pb_to_json, _roundtrip, _walk

ALL = list(LAYOUTS)
SEED = 0x0D16DEC0


def test_constants_as_designed():
    for name, v in dl.DESIGNED.items():
        assert getattr(K, name) == v, (f"{name} is {getattr(K, name)}, the layouts were drawn for {v}: redraw the "
                                       f"{dl.REDRAW[name]} layouts of tests/decode_layouts.py")
    assert set(dl.DESIGNED) == set(vars(K)) == set(dl.REDRAW)


def test_collision_suffixes_are_what_the_search_finds():
    # the literals collide under the restated FNV-1a (the search itself runs once, here, over a short span)
    slots = {dl.fnv1a(dl.collide_res(x)) & (K.kResSlots - 1) for x in dl.COLLIDE_SUFFIXES}
    assert len(slots) == 1 and len(set(dl.COLLIDE_SUFFIXES)) == 66
    found = dl.find_colliding_suffixes(n=1, span=1 << 17)
    assert len({dl.fnv1a(dl.collide_res(x)) & (K.kResSlots - 1) for x in found}) == 1


# ---------------------------------------------------------------------------
# every layout sits on its seam

def _labels(c):
    return {label: c.reasons[i] for i, (label, _) in enumerate(dl.WIRE)}


def _seam_wire(L, c):
    if L.name == "wire-top":
        assert c.n_res == 6 and c.host_spans == 0 and c.cold["res_keyed"] == 6
        assert sum(f != 1 for _, f, _ in c.structure.top) == 4 * 3 + 6 * 4
        return
    r = _labels(c)
    assert c.n_spans == len(dl.WIRE) <= 200
    want = {"kv-two-keys": ["merged_kv"], "kv-two-values": ["merged_kv"], "kv-two-values-second-empty": ["merged_kv"],
            "kv-two-keys-in-event": ["merged_kv"], "kv-two-values-in-link": ["merged_kv"], "kv-no-value": [],
            "kv-empty-value": [], "nested-values": ["nested"], "nested-in-event": ["nested"],
            "any-str-then-int-tier": [], "any-int-then-str-tier": [], "any-str-then-int-http.route": ["route"],
            "any-int-then-str-http.route": [], "any-str-then-int-db.query.text": ["query"],
            "any-int-then-str-db.query.text": [], "any-array-then-str": [], "bytes-tier": [], "bytes-http.route": ["route"],
            "bytes-db.query.text": ["query"], "bytes-url.path": ["path"], "dup-body-'{\"a\": 1}'": ["host_key"],
            "dup-http.route-7": ["route"], "dup-http.route-'/user/{id}'": [], "sql-no-value": ["query"],
            "sql-nonstring-42": ["query"], "sql-nonstring-{}": ["query"], "sql-lookalikes": [], "sql-in-event-only": [],
            "sql-lookalike-then-real": [], "scalars-twice": [], "reversed": []}
    for label, why in want.items():
        assert r[label] == why, (label, r[label])
    for w in (1, 2, 5, 10):
        for kind in ("tags", "lens", "values", "all"):
            assert r[f"{kind}-w{w}"] == []
    # a width-10 tag and length are in the bytes under test, and narrowed in the reference's
    i = [lab for lab, _ in dl.WIRE].index("all-w10")
    s, n = c.structure.spans[i]
    assert dl.V((9 << 3) | 2, 10) in L.pb[s:s + n] and dl.V((9 << 3) | 2, 10) not in L.ref_pb
    assert dl.V((9 << 3) | 2, 5) in L.ref_pb
    assert all(f"unknown-{lvl}-{f}" in r for lvl in ("span", "kv", "any", "status", "event", "link") for f in (17, 2047, 536870911))


def _seam_lengths(L, c):
    sp = L.tree_spans()
    sizes = [n for _, n in c.structure.spans]
    for k, n in enumerate(dl.LENGTHS):
        assert sizes[5 * k] == n
        assert len(host.find_attr(sp[5 * k + 1], "tier")["stringValue"]) == n
        assert len(sp[5 * k + 2]["name"]) == n and len(sp[5 * k + 3]["traceState"]) == n
        assert len(host.find_attr(sp[5 * k + 4], "url.path")["stringValue"]) == n
    assert c.host_spans == 0


def _seam_keys(L, c):
    n = int(L.name.split("-")[1])
    tab = dl.key_table(L.cfg)
    assert dl.skey(n).encode() in tab and dl.jkey(n).encode() in tab and len(dl.skey(n)) == n == len(dl.jkey(n))
    assert c.host == [False, True, False, False, False, False, False]
    assert c.reasons[1] == ["host_key"]
    sp = L.tree_spans()
    assert [kv["key"] for kv in sp[2]["attributes"][2:]] == [dl.skey(n)[:-1] + "y", dl.jkey(n)[:-1] + "y"]
    assert sp[3]["attributes"][2]["key"][:-1] == dl.skey(n) and sp[4]["attributes"][2]["key"] == dl.skey(n)[:-1]
    # the filter's bit: min(len, 63) on both sides, so 63, 64, 65 and 200 share a bit and the compare decides
    assert K.key_len_bits == 64 and {min(len(k), 63) for k in tab} >= {min(n, 63)}


def _seam_align(L, c):
    kind = L.name.rsplit("-", 1)[0]
    starts = {census(M).structure.spans[0][0] % 16 for M in LAYOUTS.values() if M.name.startswith(kind + "-")}
    assert starts == set(range(16)), (kind, starts)
    assert c.n_spans == 3 and c.host == [False, True, False] and c.reasons[1] == ["url_full"]
    if L.name == "align-top-0":   # over the 32 layouts a fixed64, a trace id, a tag and a length each cross a chunk edge
        crossed = set()
        for M in LAYOUTS.values():
            if M.family != "align":
                continue
            s, n = census(M).structure.spans[0]
            for f, wt, at, ps, pl in dl.fields(M.pb, s, s + n):
                if wt == 1 and ps // 16 != (ps + 7) // 16:
                    crossed.add("fixed64")
                if f == 1 and ps // 16 != (ps + 15) // 16:
                    crossed.add("id")
                if wt == 2 and ps % 16 == 0:
                    crossed.add("length|payload")   # the length varint ends a chunk
                if at % 16 == 15 and wt == 2:
                    crossed.add("tag|length")
        assert crossed == {"fixed64", "id", "length|payload", "tag|length"}, crossed


def _seam_end(L, c):
    s, n = c.structure.spans[-1]
    assert s + n == len(L.pb) and len(L.pb) % 16 == L.expect["len_mod"]
    path = host.find_attr(L.tree_spans()[-1], "url.path")["stringValue"].encode()
    assert L.pb.endswith(path) and c.host_spans == 0


def _seam_generic(L, c):
    e = L.expect
    checks = {
        "n_spans": lambda v: c.n_spans == v, "rounds": lambda v: len(c.rounds) == v,
        "chunks": lambda v: [r[0] for r in c.rounds] == v, "staged": lambda v: [r[1] for r in c.rounds] == v,
        "span_kernel": lambda v: c.span_kernel == v, "host_all": lambda v: c.host_spans == c.n_spans > 64,
        "host_none": lambda v: c.host_spans == 0 and c.n_spans > 64, "regrown": lambda v: c.regrown is v,
        "max_len": lambda v: len(L.pb) < v, "key_lds": lambda v: c.key_lds is v, "n_keys": lambda v: c.n_keys == v,
        "key_bytes": lambda v: c.key_bytes == v, "n_res": lambda v: c.n_res == v,
        "cold_misses": lambda v: c.cold["res_misses"] == v == c.cold["res_keyed"] and c.warm["res_misses"] == 0,
        "unkeyed": lambda v: c.res_kind.count("unkeyed") == v == c.warm["res_misses"],
        "never": lambda v: len(c.res_never) == v, "warm_misses": lambda v: c.warm["res_misses"] == v == c.warm["res_keyed"],
        "scope_bytes": lambda v: c.structure.scopes[1][1] == v,
        "host_sized": lambda v: [q for q, k in enumerate(c.scope_kind) if k == "host_sized"] == v == list(range(c.host_scopes)),
        "empty_scope": lambda v: c.structure.span_scope.count(v) == 0 and v - 1 in c.structure.span_scope and v + 1 in c.structure.span_scope,
        "n_scopes": lambda v: c.n_scopes == v,
    }
    for key, v in e.items():
        assert checks[key](v), (L.name, key, v)
    assert c.regrown is not None, "the census cannot tell whether the arena is regrown: tighten appended_bounds"


def _seam_waves(L, c):
    _seam_generic(L, c)
    if L.name == "spans-65":
        assert c.n_spans % 64 == 1          # a last round with one live lane
    if L.big:
        want = [i for i in dl.BIG_SPECIAL if i < c.n_spans]
        assert [i for i, h in enumerate(c.host) if h] == want and all(c.reasons[i] == ["route"] for i in want)
        assert c.n_spans - K.kSpanStageMax == (0 if c.span_kernel == 1 else 1)
        assert len(L.pb) < 3 << 20
    elif L.name.startswith("spans-"):
        assert c.host_spans == len([i for i in range(c.n_spans) if i % 7 == 3])
    if L.name == "big-span":
        assert max(n for _, n in c.structure.spans) > K.kSpanStage and c.n_spans == 65


def _seam_keytab(L, c):
    _seam_generic(L, c)
    carried = {kv["key"].encode() for sp in L.tree_spans() for kv in sp["attributes"]}
    tab = dl.key_table(L.cfg)
    assert tab[-1] == c.key_last == b"zz-last" and tab[-1] in carried and tab[0] in carried
    assert dl.plan_keys(L.cfg)[0] == "zz-last"       # column 0: decoded on the GPU from the table's end
    assert c.host == [False, False, False] + [len(dl.plan_keys(L.cfg)) > K.kOtlpMaxAttrKeys] * 2 + [False, False]
    assert (c.n_keys <= K.kKeyLds and c.key_bytes <= K.kKeyBytesLds) is c.key_lds


def _seam_resources(L, c):
    _seam_generic(L, c)
    n = c.n_res
    if L.name in ("res-64", "res-65"):
        assert -(-n // K.kOThreads) == (1 if n == 64 else 2)
    if L.name in ("res-256", "res-257"):
        assert c.sync_whole is (n == 257) and len(c.res_table) == n
    if L.name == "res-collide":
        slots = sorted(c.res_table)
        assert len(slots) == K.res_probes and slots == list(range(slots[0], slots[0] + K.res_probes))
        assert c.res_never == [dl.collide_res(x) for x in dl.COLLIDE_SUFFIXES[64:]]
    if L.name == "res-fields":
        st = c.structure
        assert [len(f) for f in st.res_fields] == [0, 1, 2, 1, 1, 1, 1, 1, 1] and st.schema_len == [0, 0, 0, 0, 0, 1, 128, 0, 0]
        assert st.scope_res.count(3) == 2 and st.scope_res.count(4) == 1      # field 1000 alone: taken; beside field 2: ignored
        # the absent and the empty Resource, the repeated one and the one under two schema_urls share entries
        assert len(c.res_table) == 5
    h = census(L, ("otlp_host_resources",))
    assert h.cold == h.warm == dict(res_misses=0, res_keyed=0)


def _seam_scopes(L, c):
    _seam_generic(L, c)
    h = census(L, ("otlp_host_resources",))
    if "scope_bytes" in L.expect:
        assert h.scopes_on_host_walk == [False, L.expect["scope_bytes"] > K.kGpuScopeBytes, False]
    if L.name.startswith("scopes-"):
        assert -(-c.n_scopes // K.kOThreads) == (1 if c.n_scopes == 64 else 2)
    assert census(L, ("otlp_host_scopes",)).host_scopes == 0


def _seam_chain(L, c):
    ch = census(L, ("otlp_gpu_chain",)).chain
    e = L.expect
    assert ch.n_seg == e["n_seg"] and ch.linked is e["linked"]
    for t, pos in e.get("enters", {}).items():
        assert ch.enters[t] == pos
    for t, k in e.get("listed_before", {}).items():
        if e["linked"]:
            assert ch.listed_before[t] == k
        else:   # the true entry is the (k+1)-th field start of the segment's walk: past the list
            assert ch.listed[t].index(ch.enters[t]) == k >= K.kChainList
    assert ch.covered == e.get("covered", [])
    if L.name == "chain-edges":
        st = c.structure
        assert st.records[0][1] + st.records[0][2] == K.kChainSeg == st.records[1][0]
        assert sum(f != 1 for _, f, _ in st.top) == 8
    if L.name == "chain-fake":
        assert ch.start[1] == K.kChainSeg and ch.bad[1] and len(ch.listed[1]) == 4


SEAMS = dict(wire=_seam_wire, lengths=_seam_lengths, keys=_seam_keys, align=_seam_align, end=_seam_end, waves=_seam_waves,
             hostpass=_seam_generic, keytab=_seam_keytab, resources=_seam_resources, scopes=_seam_scopes, chain=_seam_chain)


@pytest.mark.parametrize("name", ALL)
def test_layout_sits_on_its_seam(name):
    L = LAYOUTS[name]
    assert L.doc.strip() and L.family in SEAMS
    SEAMS[L.family](L, census(L))


def test_families_are_complete():
    assert {L.family for L in LAYOUTS.values()} == set(SEAMS)
    assert {n.split("-", 1)[1] for n in ALL if n.startswith("keys-")} == {str(n) for n in dl.KEY_LENGTHS}


# ---------------------------------------------------------------------------
# CPU: the reference against the host unmarshaler and the host walk

_REF: dict = {}


def _ref(name):
    """(processor, host batch, (db_flags, queries, res_sql_ok)) of a layout's reference tree, computed once"""
    if name not in _REF:
        from tests.test_sqlop import _flags_of
        L = LAYOUTS[name]
        proc = host.Processor("pipeline", L.cfg)
        hb = proc.columnarize(L.tree)
        sql = _flags_of(host.Processor(dl.SQL_SECTION, L.cfg[dl.SQL_SECTION]), L.tree)
        _REF[name] = (proc, hb, sql)
    return _REF[name]


@pytest.mark.parametrize("name", ALL)
def test_reference_equals_host_unmarshaler(name):
    L = LAYOUTS[name]
    assert _pb_to_json(L.pb) == _roundtrip(L.tree)
    if L.ref_pb != L.pb:
        assert _pb_to_json(L.ref_pb) == _pb_to_json(L.pb)


@pytest.mark.parametrize("name", ALL)
def test_host_walk_equals_reference(name):
    L = LAYOUTS[name]
    w = _walk(L.cfg_no_sql(), L.pb)
    c = _ref(name)[1].cols
    n, R, S = c.n_spans, c.n_resources, c.n_scopes
    st = census(L).structure
    assert w["span_ref"] == [s | (ln << 32) for s, ln in st.spans]
    assert (len(w["res_svc"]), len(w["scope_size"])) == (R, S) == (len(st.records), len(st.scopes))
    for key, col, cnt in (("span_res", "resource", n), ("span_scope", "scope", n), ("res_svc", "res_svc", R),
                          ("res_svc_str", "res_svc_str", R), ("res_attrset", "res_attrset", R), ("res_size", "res_size", R),
                          ("scope_size", "scope_size", S), ("scope_res", "scope_resource", S)):
        np.testing.assert_array_equal(np.array(w[key], dtype=np.uint32), _arr(getattr(c, col), cnt, np.uint32), err_msg=key)
    assert w["n_sets"] == c.n_attrsets


@pytest.mark.parametrize("name", list(dl.MALFORMED))
def test_malformed_rejected_by_host(name):
    assert _pb_to_json(dl.MALFORMED[name]) is None


# ---------------------------------------------------------------------------
# GPU

def _engine(L, options=()):
    from odigos_amd.batch import Engine
    eng = Engine(L.cfg)
    eng.set_option("otlp_sqlop", 1)
    for o in options:
        eng.set_option(o, 1)
    return eng


def _check(L, name, ob, c, warm):
    from tests.test_otlp_sqlop import _db_columns
    _, hb, (want_flags, want_queries, want_ok) = _ref(name)
    got = ob.download()
    _compare(ob.cols, hb.cols, got)
    flags, queries, ok = _db_columns(ob.cols, got)
    np.testing.assert_array_equal(flags, want_flags)
    assert queries == want_queries
    np.testing.assert_array_equal(ok, want_ok)
    assert ob.host_spans == c.host_spans, "more: a silent fallback; fewer: a span the GPU should not have finished"
    want = c.walk_info(warm)
    info = dict(ob.walk_info)
    if warm:   # the engine's pooled arena may have grown already
        assert info.pop("arena_regrown") <= want.pop("arena_regrown")
    assert info == want


def _modes():
    return [(n, o) for n in ALL for o in (None,) + LAYOUTS[n].options]


@pytest.mark.gpu
@pytest.mark.parametrize("name,option", _modes())
def test_gpu_decode_equals_reference(name, option):
    from odigos_amd.batch import OtlpBatch
    L = LAYOUTS[name]
    options = (option,) if option else ()
    c = census(L, options)
    eng = _engine(L, options)
    for warm in (False, True):   # a cold engine, then the same engine with its resource table filled
        ob = OtlpBatch(eng, L.pb)
        _check(L, name, ob, c, warm)
        ob.close()


@pytest.mark.gpu
def test_gpu_truncated_chain_is_rejected():
    # the chain layouts with their last 1000 bytes removed: the link cannot reach the end, the host walk reports it
    from odigos_amd.batch import OtlpBatch
    for name in ("chain-edges", "chain-list-15"):
        L = LAYOUTS[name]
        eng = _engine(L, ("otlp_gpu_chain",))
        with pytest.raises(native.OseError) as ei:
            OtlpBatch(eng, L.pb[:-1000])
        assert ei.value.code == native.OSE_EINVAL
        ob = OtlpBatch(eng, L.pb)
        _check(L, name, ob, census(L, ("otlp_gpu_chain",)), False)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(dl.FAMILY_STAGE_LAYOUT))
def test_gpu_stages_on_decoded_columns(family):
    """SAMPLE|TEMPLATE|SIZE on the decoded columns equals the oracle chain on
    the reference's batch: the columns are consumable, not just equal."""
    import torch
    from odigos_amd.batch import Engine, HostOutputs, OtlpBatch
    from tests.oracle_lib import SamplingOracle, UrlOracle, size_process
    name = dl.FAMILY_STAGE_LAYOUT[family]
    L = LAYOUTS[name]
    cfg = L.cfg_no_sql()
    hb = host.Processor("pipeline", cfg).columnarize(L.tree)
    ob = OtlpBatch(Engine(cfg), L.pb)
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    ob.eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=SEED)
    torch.cuda.synchronize()
    cols = hb.cols
    ho = HostOutputs(cols)
    assert SamplingOracle(cfg["odigossampling"]).process(cols, ho.outs, native.GROUP_TRACE_ID, SEED, 4) == 0
    assert UrlOracle(cfg["odigosurltemplate"]).process(cols, ho.outs, 4) == 0
    assert size_process(cols, ho.outs, st, native.GROUP_TRACE_ID, ho.outs, 1, 1.0, 0.0, 4) == 0
    n, A = cols.n_spans, cols.n_attrsets
    np.testing.assert_array_equal(ob.out_numpy("keep", n=n), ho.view("keep", np.uint8)[:n])
    np.testing.assert_array_equal(ob.out_numpy("url_out", n=n), ho.view("url_out", np.uint8)[:n])
    used = ob.used()
    assert used == int(ho.used[0])
    np.testing.assert_array_equal(ob.out_numpy("tmpl_arena", n=used), ho.bufs["tmpl_arena"][:used])
    np.testing.assert_array_equal(ob.out_numpy("attrset_bytes", np.int64, n=A), ho.view("attrset_bytes", np.int64)[:A])
    assert int(ob.out_numpy("accepted_spans", np.int64, n=1)[0]) == int(ho.view("accepted_spans", np.int64)[0])


@pytest.mark.gpu
def test_gpu_malformed_is_einval_and_the_engine_goes_on():
    from odigos_amd.batch import OtlpBatch
    L = LAYOUTS["spans-65"]
    c = census(L)
    for options in ((), ("otlp_gpu_chain",), ("otlp_host_resources",), ("otlp_host_scopes",)):
        eng = _engine(L, options)
        accepted = []
        for name, bad in dl.MALFORMED.items():
            try:
                OtlpBatch(eng, bad)
                accepted.append(name)
            except native.OseError as e:
                assert e.code == native.OSE_EINVAL, (name, options)
        assert not accepted, (options, accepted)
        ob = OtlpBatch(eng, L.pb)
        _compare(ob.cols, _ref("spans-65")[1].cols, ob.download())
        assert ob.host_spans == c.host_spans


@pytest.mark.gpu
def test_gpu_walk_info_of_a_released_batch_is_enotsup():
    import ctypes as C
    from odigos_amd.batch import Engine, GroupByTrace, OtlpBatch
    L = LAYOUTS["spans-65"]
    eng = Engine(L.cfg_no_sql())
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, 1 << 16)
    ob = OtlpBatch(eng, L.pb)
    g.add_otlp(ob, now_ns=0)
    rb, _ = g.release_otlp(now_ns=10 ** 12)
    out = (C.c_uint32 * 8)()
    assert native.lib().ose_otlp_walk_info(rb.h, out) == native.OSE_ENOTSUP
    assert native.lib().ose_otlp_walk_info(ob.h, out) == 0 and out[6] == 1
