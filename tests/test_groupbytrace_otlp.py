"""groupbytrace on the OTLP path: ose_gbt_add_otlp / ose_gbt_release_otlp
(gbt_host.cpp, gbt_kernel.hip, the released batch in otlp_host.cpp, its
encode in otlp_encode_host.cpp).

decode -> add_otlp -> release_otlp -> stages -> encode, no pdata in between:
an OTLP-fed store keeps every span's message and every added scope's header
block, and a release is a batch ose_otlp_encode writes out.

The expected side is restated independently of the engine:
tests/gbt_ref.py says which traces leave at which release, their pieces and
order; tests/gbt_otlp_ref.py turns a release into the TracesData sent
downstream and lays out what the store keeps of a hand-laid batch;
tests/otlp_gogo.py gives the processors' writes, the connector and pdata's
marshaler; the oracles give the decisions and counters.

A Span message of 1 byte does not exist on the wire (a field is at least a tag
and a value byte), so the hand-laid lengths start at 0 (an empty message) and
2; pdata's own encoding starts at 8 (the three ids and the Status are always
framed) and cannot be 9.
"""
import ctypes as C
import random
import re
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import host, native
from tests import gbt_otlp_ref as gr
from tests import otlp_gogo as gg
from tests.gbt_ref import GroupByTraceRef
from tests.test_groupbytrace import _Shim, _compare_release, _expected_columns, _set_of
from tests.test_otlp import CFG, CFG_JSON_RULE, SEED, _http_traces, _pb_to_json, _roundtrip, to_pb
from tests.test_router_encode import _expected, _routable

S = 1_000_000_000
ROOT = Path(__file__).resolve().parent.parent
MIN_RING = 1 << 16   # the store's smallest arena ring

STREAMS2 = [
    {"name": "ds-a", "sources": [{"namespace": "prod", "kind": "Deployment", "name": "api"},
                                 {"namespace": "default", "kind": "StatefulSet", "name": "db"}],
     "destinations": [{"destinationname": "d0", "configuredsignals": ["TRACES"]}]},
    {"name": "ds-b", "sources": [{"namespace": "prod", "kind": "Deployment", "name": "web"},
                                 {"namespace": "prod", "kind": "Deployment", "name": "api"},
                                 {"namespace": "dev", "kind": "DaemonSet", "name": "agent"}],
     "destinations": [{"destinationname": "d1", "configuredsignals": ["TRACES", "LOGS"]}]},
]


# ---- CPU -------------------------------------------------------------------------

def test_header_declares_the_two_calls():
    text = (ROOT / "include" / "odigos_amd.h").read_text()
    flat = re.sub(r"\s+", " ", text)
    assert ("int ose_gbt_add_otlp(ose_gbt* g, const ose_otlp_batch* b, const uint32_t* attrset_map, int64_t now_ns, "
            "void* hip_stream);") in flat
    assert ("int ose_gbt_release_otlp(ose_gbt* g, int64_t now_ns, void* hip_stream, const ose_otlp_batch** out, "
            "uint32_t* n_traces);") in flat
    assert re.search(r"#define OSE_ABI_VERSION 5\b", text)
    # appended: after every declaration the header had
    assert flat.index("int ose_gbt_add_otlp(") > flat.index("int ose_device_info(")


def test_abi_structs_unchanged_and_calls_bound():
    assert (C.sizeof(native.Columns), C.sizeof(native.Outputs)) == (264, 128)
    L = native.lib()
    assert L.ose_gbt_add_otlp.restype is C.c_int and L.ose_gbt_release_otlp.restype is C.c_int
    assert len(L.ose_gbt_add_otlp.argtypes) == 5 and len(L.ose_gbt_release_otlp.argtypes) == 5


def test_release_restated_as_traces_data():
    """Each piece is a ResourceSpans with the piece's Resource, one ScopeSpans
    and its spans in arrival order; over a run with evictions the released and
    the evicted spans are exactly the input multiset."""
    rng = random.Random(0x0717)
    td = _roundtrip(_routable(_http_traces(rng, 60), rng))
    rss = td["resourceSpans"]
    ref = GroupByTraceRef(30 * S, num_traces=16)
    key = lambda sp: gg.span(sp)
    out, gone, now = [], [], 0
    for k in range(0, len(rss), 9):
        now += 4 * S
        before = dict(ref.inst)
        part = {"resourceSpans": rss[k:k + 9]}
        ref.consume(part, now)
        gone += [sp for i, t in before.items() if i not in ref.inst for p in t["pieces"] for sp in gr.spans_of(
            {"resourceSpans": [p]})]
        rel = ref.release(now)
        rtd = gr.release_traces_data(rel)
        assert len(rtd["resourceSpans"]) == sum(len(tr) for tr in rel)
        for rs in rtd["resourceSpans"]:
            assert len(rs["scopeSpans"]) == 1 and rs["scopeSpans"][0]["spans"]
            assert len({sp.get("traceId", "") for sp in rs["scopeSpans"][0]["spans"]}) == 1
        assert _pb_to_json(gg.marshal_traces(rtd)) == _roundtrip(rtd)   # it marshals as pdata would
        out += gr.spans_of(rtd)
    out += gr.spans_of(gr.release_traces_data(ref.release(now + 31 * S)))
    assert ref.evicted > 0 and not ref.inst
    assert sorted(map(key, out + gone)) == sorted(map(key, gr.spans_of(td)))
    # a piece keeps its Resource, scope and schema URLs: one source scope, one trace
    one = {"resourceSpans": [{"resource": {"attributes": host.attrs({"service.name": "x"})}, "schemaUrl": "r",
                              "scopeSpans": [{"scope": {"name": "lib"}, "schemaUrl": "s",
                                              "spans": [host.span(name="a", trace_id="%032x" % 5),
                                                        host.span(name="b", trace_id="%032x" % 6),
                                                        host.span(name="c", trace_id="%032x" % 5)]}]}]}
    ref = GroupByTraceRef(S)
    ref.consume(one, 0)
    rtd = gr.release_traces_data(ref.release(S))
    assert [[sp["name"] for sp in rs["scopeSpans"][0]["spans"]] for rs in rtd["resourceSpans"]] == [["a", "c"], ["b"]]
    assert all(rs["schemaUrl"] == "r" and rs["scopeSpans"][0]["schemaUrl"] == "s" and
               rs["scopeSpans"][0]["scope"] == {"name": "lib"} for rs in rtd["resourceSpans"])


# The hand-laid batches of the seam test.  RES / SCOPE: the header fields.
RES = gg._len(1, gg._attrs(1, host.attrs({"service.name": "svc-a", "k8s.pod.name": "pod-1"})))
SCOPE = gg._len(1, gg._str(1, "lib") + gg._str(2, "1.0"))


def _pdata_lengths(lens, tid=""):
    return [gg.span(sp) for sp in (gr.span_of_len(n, tid) for n in lens) if sp is not None]


def _seam_batches():
    """[(name, message bytes, arena ring bytes)]"""
    out = []
    # every pdata length 8..600 in five adds of one trace each (the empty id's), so
    # consecutive messages meet every source and destination alignment mod 16
    lens = list(range(8, 601))
    for k in range(5):
        out.append(("lengths-%d" % k, gr.raw_batch(RES, SCOPE, _pdata_lengths(lens[k::5]), gg._str(3, "u")), MIN_RING))
    # ... and an add whose header block lies across the ring's end (the adds above end at 180598 = 2 * 65536 + 49526)
    out.append(("header-across-end", gr.raw_batch(RES, SCOPE, _pdata_lengths([600] * 26 + [380])), MIN_RING))
    # messages below pdata's smallest: 0 and 2..7 bytes (a name of 0..5 bytes), and no header at all
    tiny = [b""] + [gg._tag(5, 2) + gg._varint(k) + b"x" * k for k in range(6)]
    out.append(("tiny-no-header", gr.raw_batch(b"", b"", tiny * 3), MIN_RING))
    # a lone message at lane 0 of its wave (the 65th span) and at lane 63 (63 empty ones before it)
    out.append(("lone-lane-0", gr.raw_batch(RES, SCOPE, _pdata_lengths([40] * 64 + [77])), MIN_RING))
    out.append(("lone-lane-63", gr.raw_batch(RES, SCOPE, [b""] * 63 + _pdata_lengths([77])), MIN_RING))
    # the last Span message ends on the decoded message's last byte
    out.append(("ends-on-last-byte", gr.raw_batch(RES, SCOPE, _pdata_lengths([33, 250])), MIN_RING))
    # one 64 KiB span (a ring that holds it)
    out.append(("64KiB", gr.raw_batch(RES, SCOPE, _pdata_lengths([1 << 16])), 1 << 18))
    return out


def test_seam_batches_census():
    """The hand-laid batches, pinned byte for byte: what the store keeps of
    each, where it lies in a ring of the smallest size, and that the seams the
    GPU test is about are in them."""
    batches = _seam_batches()
    c = gr.RingCensus(MIN_RING)
    took = {}
    for name, pb, ring in batches:
        if ring == MIN_RING:
            took[name] = c.add(pb)
    hdr = len(RES) + len(SCOPE)   # (the lengths-* batches have a 3-byte schema_url after their spans as well)
    assert (len(RES), len(SCOPE)) == (52, 12)
    assert took == {"lengths-0": 36124, "lengths-1": 36234, "lengths-2": 36362, "lengths-3": 35880, "lengths-4": 35998,
                    "header-across-end": 15980 + hdr, "tiny-no-header": 81, "lone-lane-0": 64 * 40 + 77 + hdr,
                    "lone-lane-63": 77 + hdr, "ends-on-last-byte": 33 + 250 + hdr}
    assert c.end == sum(took.values()) > 2 * MIN_RING
    # every source and every destination alignment mod 16
    pairs = {(off % 16, pos % 16) for pos, off, ln in c.msgs if ln}
    assert {p[0] for p in pairs} == set(range(16)) and {p[1] for p in pairs} == set(range(16))
    # a message and a header block across the ring's end; a header block of length 0
    assert c.straddles(c.msgs) and c.straddles(c.hdrs)
    assert (0 in [ln for _, ln in c.hdrs]) and 0 in [ln for _, _, ln in c.msgs]
    name, pb, _ = batches[-2]
    off, ln = gr.pieces_of(pb)[0][2][-1]
    assert name == "ends-on-last-byte" and off + ln == len(pb)
    name, pb, _ = batches[-1]
    assert gr.pieces_of(pb)[0][2] == [(len(pb) - (1 << 16), 1 << 16)]


# ---- GPU -------------------------------------------------------------------------

class _OtlpShim(_Shim):
    """decode, intern the attribute sets, ose_gbt_add_otlp"""

    def add_pb(self, pb, now):
        from odigos_amd.batch import OtlpBatch
        ob = OtlpBatch(self.eng, pb)
        ids = []
        for k in range(ob.cols.n_attrsets):
            key = tuple(sorted(ob.attrset(k).items()))
            if key not in self.sets:
                self.sets[key] = len(self.names)
                self.names.append(key)
            ids.append(self.sets[key])
        try:
            self.g.add_otlp(ob, now, ids)
        finally:
            ob.close()


def _trees(rng, n_traces, odd=0.05):
    """Trees whose traces straddle resources: several scopes per resource,
    empty scopes, spanless resources, scope and resource schema URLs."""
    return _roundtrip(_routable(_http_traces(rng, n_traces, odd=odd), rng))


def _marshal(td, encoding, bare_resource=False):
    if encoding == "google":
        return to_pb(td)
    out = b""
    for rs in td["resourceSpans"]:
        body = gg.resource_spans(rs)
        if bare_resource and body.startswith(b"\x0a\x00"):
            body = body[2:]   # a ResourceSpans without a Resource message (pdata writes "0A 00" for it)
        out += gg._len(1, body)
    return out


def _three_adds(td, rng):
    rss = list(td["resourceSpans"])
    rss.append({"resource": {}, "scopeSpans": [{"scope": {}, "spans": [host.span(name="bare", trace_id="%032x" % 77)]}]})
    a, b = sorted((rng.randrange(len(rss) + 1), rng.randrange(len(rss) + 1)))
    return [_roundtrip({"resourceSpans": part}) for part in (rss[:a], rss[a:b], rss[b:])]


def _check_columns(shim, rb, want):
    td_w, _, hb = _expected_columns(want)
    got = rb.download()
    g_sets, h_sets = _compare_release(got, rb.cols, hb, shim.names)
    assert [shim.names[x] for x in g_sets] == [_set_of(rs) for rs in td_w["resourceSpans"]]
    return hb, g_sets, h_sets


def _round_trip(eng, n_traces, encoding="pdata", seed=0, store_cfg=None, ring=1 << 22, ref_kw=None):
    """Three adds, a release after each and four more: encode(stages=0) equals
    the restated release byte for byte, the released columns equal the host
    columniser's on the restated traces."""
    rng = random.Random(0x6B70 + 131 * n_traces + seed)
    shim = _OtlpShim(eng, dict({"wait_duration": "30s"}, **(store_cfg or {})), arena_capacity=ring)
    ref = GroupByTraceRef(30 * S, **(ref_kw or {}))
    parts = _three_adds(_trees(rng, n_traces), rng)
    now, released, spans = 0, 0, 0
    for step, part in enumerate(parts + [None] * 4):
        now += rng.choice([3, 7, 11, 20]) * S
        if part is not None:
            shim.add_pb(_marshal(part, encoding, bare_resource=True), now)
            ref.consume(part, now)
        rb, ntr = shim.g.release_otlp(now)
        want = ref.release(now)
        assert ntr == len(want), step
        if not want:
            assert rb.cols.n_spans == 0
            continue
        released += len(want)
        rtd = gr.release_traces_data(want)
        spans += len(gr.spans_of(rtd))
        assert rb.encode(0) == [("", gg.marshal_traces(rtd), len(rtd["resourceSpans"]))], step
        assert rb.encode_path["gpu"] is (encoding == "pdata")
        _check_columns(shim, rb, want)
    st = shim.g.stats()
    assert released == st["released"] > 0 and st["released_spans"] == spans
    assert st["waiting_traces"] == 0 and st["held_spans"] == 0 and st["held_bytes"] == 0
    return shim, st


@pytest.mark.gpu
@pytest.mark.parametrize("n_traces", [1, 65, 700])
def test_gpu_round_trip_no_stages(n_traces):
    from odigos_amd.batch import Engine
    _, st = _round_trip(Engine(CFG), n_traces)
    assert st["evicted"] == 0


def _stage_outputs(rb):
    n = rb.cols.n_spans
    url_out = rb.out_numpy("url_out", n=n)
    refs = rb.out_numpy("tmpl", np.uint32, n=2 * n).reshape(-1, 2)
    arena = rb.out_numpy("tmpl_arena", n=rb.used()).tobytes()
    tmpls = [arena[o:o + ln].decode("utf-8", "surrogateescape") if u else "" for (o, ln), u in zip(refs, url_out)]
    return list(rb.out_numpy("keep", n=n)), list(url_out), tmpls


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["pdata", "google"])
def test_gpu_stages_on_a_release(encoding):
    """SAMPLE | TEMPLATE | SIZE on each release and a two-pipeline router:
    the outputs equal the restatement applied with the GPU's decisions, the
    decisions and counters equal the oracles'; pdata's encoding is written by
    the GPU encoder with no fallback, google.protobuf's by the host encoder
    (the released buffer comes down, layout_to_host fills the layout), also
    under the engine option encode_host."""
    import torch
    from odigos_amd.batch import Engine, HostOutputs, Router
    from tests.oracle_lib import SamplingOracle, UrlOracle, size_process
    rng = random.Random(0x57A6)
    eng = Engine(CFG)
    router = Router({"datastreams": STREAMS2})
    assert len(router.pipelines) == 2
    shim = _OtlpShim(eng, {"wait_duration": "30s"})
    ref = GroupByTraceRef(30 * S)
    parts = _three_adds(_trees(rng, 150, odd=0.0), rng)
    stages = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    now, seen = 0, 0
    for part in parts + [None] * 3:
        now += 12 * S
        if part is not None:
            shim.add_pb(_marshal(part, encoding), now)
            ref.consume(part, now)
        rb, ntr = shim.g.release_otlp(now)
        want = ref.release(now)
        assert ntr == len(want)
        if not want:
            continue
        seen += ntr
        hb, g_sets, h_sets = _check_columns(shim, rb, want)
        eng.process_device(rb, stages, native.GROUP_TRACE_ID, seed=SEED)
        torch.cuda.synchronize()
        cols = hb.cols
        ho = HostOutputs(cols)
        assert SamplingOracle(CFG["odigossampling"]).process(cols, ho.outs, native.GROUP_TRACE_ID, SEED, 4) == 0
        assert UrlOracle(CFG["odigosurltemplate"]).process(cols, ho.outs, 4) == 0
        assert size_process(cols, ho.outs, stages, native.GROUP_TRACE_ID, ho.outs, 1, 1.0, 0.0, 4) == 0
        n = cols.n_spans
        keep, url_out, tmpls = _stage_outputs(rb)
        np.testing.assert_array_equal(keep, ho.view("keep", np.uint8)[:n])
        np.testing.assert_array_equal(url_out, ho.view("url_out", np.uint8)[:n])
        assert int(rb.out_numpy("accepted_spans", np.int64, n=1)[0]) == int(ho.view("accepted_spans", np.int64)[0])
        # the store's attribute set ids are the shim's: counters compared set by set
        gb = rb.out_numpy("attrset_bytes", np.int64, n=rb.cols.n_attrsets)
        hbytes = ho.view("attrset_bytes", np.int64)
        assert {int(g): int(gb[g]) for g in g_sets} == {int(g): int(hbytes[h]) for g, h in zip(g_sets, h_sets)}
        rtd = gr.release_traces_data(want)
        for r in (router, None):
            exp = _expected(rtd, STREAMS2 if r else None, router.pipelines if r else None, keep=keep, url_out=url_out,
                            tmpls=tmpls)
            assert rb.encode(stages, native.GROUP_TRACE_ID, r) == exp
            if encoding == "pdata":
                assert rb.encode_path == {"gpu": True, "fallback": 0}
            else:
                assert rb.encode_path["gpu"] is False and rb.encode_path["fallback"] != 0
            eng.set_option("encode_host", 1)
            try:
                assert rb.encode(stages, native.GROUP_TRACE_ID, r) == exp
                assert rb.encode_path["gpu"] is False
            finally:
                eng.set_option("encode_host", 0)
        # OSE_GROUP_BATCH's all-or-nothing is the host encoder's: the third trigger of the host leg
        eng.process_device(rb, stages, native.GROUP_BATCH, seed=SEED)
        torch.cuda.synchronize()
        _, url_out, tmpls = _stage_outputs(rb)
        tk = int(rb.out_numpy("trace_keep", n=1)[0])
        assert rb.encode(stages, native.GROUP_BATCH, router) == _expected(rtd, STREAMS2, router.pipelines, url_out=url_out,
                                                                          tmpls=tmpls, drop_all=not tk)
        assert rb.encode_path["gpu"] is False
    assert seen == shim.g.stats()["released"] > 100


@pytest.mark.gpu
def test_gpu_stages_with_sqlop_on_a_release():
    """An engine with the odigossqldboperationprocessor section and otlp_sqlop
    on: the store carries db_flags / db_query / res_sql_ok from the decoder,
    SAMPLE | TEMPLATE | SQLOP | SIZE runs on the release, sql_op equals the
    restatement of processor.go and the GPU encoder writes the attribute and
    the longer name with no fallback."""
    import torch
    import tests.test_groupbytrace as tg
    from odigos_amd.batch import Router
    from tests import test_otlp_sqlop as ts
    rng = random.Random(0x5A1)
    eng = ts._sql_engine({})
    router = Router({"datastreams": STREAMS2})
    shim = _OtlpShim(eng, {"wait_duration": "30s"})
    ref = GroupByTraceRef(30 * S)
    td = ts._canonical_tree(rng, 120)
    rss = td["resourceSpans"]
    parts = [_roundtrip({"resourceSpans": rss[k::3]}) for k in range(3)]
    now, ops = 0, set()
    old, tg.CFG = tg.CFG, ts._full_cfg({})   # the columniser of the comparison runs the engine's config
    try:
        for part in parts + [None] * 3:
            now += 12 * S
            if part is not None:
                shim.add_pb(gg.marshal_traces(part), now)
                ref.consume(part, now)
            rb, ntr = shim.g.release_otlp(now)
            want = ref.release(now)
            assert ntr == len(want)
            if not want:
                continue
            assert rb.cols.db_flags and rb.cols.db_query and rb.cols.res_sql_ok
            _check_columns(shim, rb, want)
            eng.process_device(rb, ts.ST_SQL, native.GROUP_TRACE_ID, seed=SEED)
            torch.cuda.synchronize()
            assert int(rb.out_numpy("device_status", np.uint32)[0]) == 0
            rtd = gr.release_traces_data(want)
            dec = ts._gpu_decisions(rb)
            np.testing.assert_array_equal(dec["sql_op"], ts._expected_sql_op({}, rtd))
            ops |= set(dec["sql_op"])
            for r in (router, None):
                exp = ts._restate(rtd, STREAMS2 if r else None, router.pipelines if r else None, **dec)
                assert rb.encode(ts.ST_SQL, native.GROUP_TRACE_ID, r) == exp
                assert rb.encode_path == {"gpu": True, "fallback": 0}
                eng.set_option("encode_host", 1)
                try:
                    assert rb.encode(ts.ST_SQL, native.GROUP_TRACE_ID, r) == exp
                finally:
                    eng.set_option("encode_host", 0)
    finally:
        tg.CFG = old
    assert len(ops) >= 4


@pytest.mark.gpu
def test_gpu_merged_header_fields_go_through_the_host_encoder():
    """A resource whose Resource and scope arrive in two fields each and whose
    schema URLs are written twice (kMulti): the header block keeps every field
    as it stands, the release's scope header is kMulti again, and the host
    encoder merges them as pdata does."""
    from odigos_amd.batch import Engine
    eng = Engine(CFG)
    sp = gg.span(host.span(name="GET", kind=2, trace_id="%032x" % 9, attributes={"url.path": "/a/1"}))
    res = gg._len(1, gg.key_value({"key": "k8s.namespace.name", "value": {"stringValue": "prod"}}))
    res2 = gg._len(1, gg.key_value({"key": "k8s.deployment.name", "value": {"stringValue": "api"}}))
    ss = gg._len(1, gg._str(1, "lib")) + gg._len(2, sp) + gg._len(1, gg._str(2, "v2")) + gg._str(3, "u1") + \
        gg._str(3, "u2") + b"\x20\x07"
    msg = b"\x10\x01" + gg._len(1, gg._len(1, res) + gg._len(2, ss) + gg._len(1, res2) + gg._str(3, "x") + gg._str(3, "y"))
    td = _pb_to_json(msg)
    shim = _OtlpShim(eng, {"wait_duration": "1s"}, arena_capacity=MIN_RING)
    ref = GroupByTraceRef(S)
    shim.add_pb(msg, 0)
    ref.consume(td, 0)
    rb, ntr = shim.g.release_otlp(S)
    rtd = gr.release_traces_data(ref.release(S))
    assert ntr == 1
    assert rb.encode(0) == [("", gg.marshal_traces(rtd), 1)]
    assert rb.encode_path["gpu"] is False and rb.encode_path["fallback"] != 0


@pytest.mark.gpu
def test_gpu_seams_of_the_copies():
    """The hand-laid batches of test_seam_batches_census through a ring of the
    smallest size, one add and one release each: held_bytes is the census's
    figure after every add, and every release marshals to the restatement."""
    from odigos_amd.batch import Engine, GroupByTrace, OtlpBatch
    eng = Engine(CFG)
    stores = {}
    census = gr.RingCensus(MIN_RING)
    now = 0
    for name, pb, ring in _seam_batches():
        if ring not in stores:
            stores[ring] = (GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, ring), GroupByTraceRef(S))
        g, ref = stores[ring]
        td = _pb_to_json(pb)
        now += 2 * S
        ob = OtlpBatch(eng, pb)
        g.add_otlp(ob, now)
        ob.close()
        ref.consume(td, now)
        took = census.add(pb) if ring == MIN_RING else gr.RingCensus(ring).add(pb)
        assert g.stats()["held_bytes"] == took, name
        now += 2 * S
        rb, ntr = g.release_otlp(now)
        rtd = gr.release_traces_data(ref.release(now))
        assert ntr == 1 and rb.cols.n_spans == len(gr.spans_of(rtd)), name
        assert rb.cols.arena_bytes == took, name   # one fragment: its header once, then every block
        assert rb.encode(0) == [("", gg.marshal_traces(rtd), 1)], name
        assert g.stats()["held_bytes"] == 0, name


@pytest.mark.gpu
def test_gpu_refusals_and_modes():
    from odigos_amd.batch import Engine, GroupByTrace, OtlpBatch
    L = native.lib()
    eng, eng2 = Engine(CFG), Engine(CFG)
    rng = random.Random(0x0EF5)

    def code(fn, *a):
        with pytest.raises(native.OseError) as ei:
            fn(*a)
        return ei.value.code

    small = _marshal(_trees(rng, 8), "pdata")
    # an add refused by its message bytes alone: ~100 KiB of messages, no strings to speak of
    big = gr.raw_batch(RES, SCOPE, _pdata_lengths([600] * 170, "%032x" % 3))
    runs = []
    for refuse in (False, True):
        g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, MIN_RING)
        ob = OtlpBatch(eng, small)
        g.add_otlp(ob, 0)
        before = g.stats()
        if refuse:
            ob_big = OtlpBatch(eng, big)
            assert code(g.add_otlp, ob_big, 1) == native.OSE_ERANGE
            assert g.stats() == before   # nothing stored
            ob_big.close()
        g.add_otlp(ob, 2)
        out = []
        for now in (S, S + 2, 3 * S):
            rb, ntr = g.release_otlp(now)
            out.append((ntr, rb.encode(0) if rb.cols.n_spans else None))
        runs.append(out)
        # mixed modes, the wrong calls for the mode
        assert code(g.add, ob.cols, 4 * S) == native.OSE_EINVAL
        assert code(g.release, 4 * S) == native.OSE_EINVAL
        assert code(g.download, ob.cols) == native.OSE_EINVAL
        # another engine's batch; a released batch added again
        ob2 = OtlpBatch(eng2, small)
        assert code(g.add_otlp, ob2, 4 * S) == native.OSE_EINVAL
        assert code(g.add_otlp, rb, 4 * S) == native.OSE_EINVAL
        ob2.close()
        # what a released batch does not answer
        assert code(rb.attrset, 0) == native.OSE_ENOTSUP
        t = (C.c_double * 5)()
        assert L.ose_otlp_timings(rb.h, t) == native.OSE_ENOTSUP
        assert L.ose_otlp_host_spans(rb.h) == native.OSE_ENOTSUP & 0xFFFFFFFF
        ob.close()
    assert runs[0] == runs[1] and runs[0][0][0] > 0
    # a columns-fed store
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, MIN_RING)
    ob = OtlpBatch(eng, small)
    g.add(ob.cols, 0)
    assert code(g.add_otlp, ob, 1) == native.OSE_EINVAL
    assert code(g.release_otlp, 1) == native.OSE_EINVAL
    ob.close()
    # 2^32 bytes of ring or more: refused at the first OTLP add; the columns add still works
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, 1 << 32)
    ob = OtlpBatch(eng, small)
    assert code(g.add_otlp, ob, 0) == native.OSE_ERANGE
    g.add(ob.cols, 0)
    g.close()
    ob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_cfg,ref_kw", [({"num_traces": 4}, {"num_traces": 4}),
                                              ({"num_traces": 13, "num_workers": 3}, {"num_traces": 13, "num_workers": 3})])
def test_gpu_eviction_and_workers(store_cfg, ref_kw):
    """A 4-trace ring, and num_workers 3: the evicted traces' bytes appear in
    no output (every release equals the restatement, which drops them)."""
    from odigos_amd.batch import Engine
    rng = random.Random(0xE71C + len(store_cfg))
    eng = Engine(CFG)
    shim = _OtlpShim(eng, dict({"wait_duration": "30s"}, **store_cfg))
    ref = GroupByTraceRef(30 * S, **ref_kw)
    rss = _trees(rng, 40)["resourceSpans"]
    now, outs = 0, b""
    for k in range(0, len(rss) + 40, 10):
        now += 9 * S
        part = _roundtrip({"resourceSpans": rss[k:k + 10]})
        if part["resourceSpans"]:
            shim.add_pb(_marshal(part, "pdata"), now)
            ref.consume(part, now)
        rb, ntr = shim.g.release_otlp(now)
        want = ref.release(now)
        assert ntr == len(want)
        if want:
            rtd = gr.release_traces_data(want)
            got = rb.encode(0)
            assert got == [("", gg.marshal_traces(rtd), len(rtd["resourceSpans"]))]
            outs += got[0][1]
            _check_columns(shim, rb, want)
    st = shim.g.stats()
    # (the two evicted counts differ where an add creates more traces than a ring holds: the store applies
    # eviction per add, DESIGN.md §4.7, and numbers fewer instances of an id that returns within the add; what
    # leaves is the same, checked above)
    assert st["evicted"] > 0 and ref.evicted > 0 and st["created"] == st["released"] + st["evicted"]
    assert st["waiting_traces"] == 0 and st["held_bytes"] == 0 and st["held_spans"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["otlp_gpu_chain", "otlp_host_resources", "otlp_host_scopes", "host_pass"])
def test_gpu_every_decode_layout_placement(placement):
    """The round trip at one size with the layout left where each decode
    variant leaves it: the TracesData chain walked on the GPU, the
    ResourceSpans on the host, the scopes on the host too, and a batch with
    host-pass spans (non-string http.route values, a json rule's key)."""
    from odigos_amd.batch import Engine
    cfg = CFG_JSON_RULE if placement == "host_pass" else CFG
    eng = Engine(cfg)
    if placement != "host_pass":
        eng.set_option(placement, 1)
    _round_trip_cfg(eng, cfg, 65, seed=3)


def _round_trip_cfg(eng, cfg, n_traces, seed):
    # the host columniser of the comparison runs the engine's own config
    import tests.test_groupbytrace as tg
    old = tg.CFG
    tg.CFG = cfg
    try:
        _round_trip(eng, n_traces, seed=seed)
    finally:
        tg.CFG = old


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["store_first", "engine_first"])
def test_gpu_lifetime(order):
    """The store destroyed while a released batch's outputs are still held;
    the engine destroyed before the store: no error recorded either way (the
    conftest's ose_dropped_errors check)."""
    import torch
    from odigos_amd.batch import Engine, GroupByTrace, OtlpBatch, take_otlp_out
    L = native.lib()
    eng = Engine(CFG)
    td = _trees(random.Random(0x11FE), 20)
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, 1 << 20)
    ob = OtlpBatch(eng, _marshal(td, "pdata"))
    g.add_otlp(ob, 0)
    ob.close()
    ref = GroupByTraceRef(S)
    ref.consume(td, 0)
    rb, ntr = g.release_otlp(S)
    h = C.c_void_p()
    native.check(L.ose_otlp_encode(eng.h, rb.h, C.byref(rb.outs), 0, native.GROUP_TRACE_ID, None, None, C.byref(h)))
    rtd = gr.release_traces_data(ref.release(S))
    if order == "store_first":
        g.close()
        assert take_otlp_out(L, h) == [("", gg.marshal_traces(rtd), len(rtd["resourceSpans"]))]
    else:
        eh = eng.h
        eng.h = None   # bypass Engine.close (which releases the children first)
        L.ose_engine_destroy(eh)
        assert take_otlp_out(L, h) == [("", gg.marshal_traces(rtd), len(rtd["resourceSpans"]))]
        g.close()
    torch.cuda.synchronize()
