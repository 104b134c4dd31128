"""odigossqldboperationprocessor through the OTLP path (engine option
otlp_sqlop): ose_otlp_decode fills db_flags / db_query / res_sql_ok from the
message (otlp_sqlop_kernel.hip, the host pass for the values that need
AsString), the stages run on the decoded columns, ose_otlp_encode writes the
attribute and the longer name (encode_kernel.hip, otlp_encode.cpp), and
ose_otlp_pipeline runs the stage.

Expected columns come from the host columniser over the OTLP/JSON form of
the same traces (host.Processor(SECTION, cfg).columnarize), expected
decisions from the restatement of processor.go (tests/sqlop_ref.py), expected
sizes and output bytes from marshalling the tree with the decisions applied
(_restate below, on tests/otlp_gogo.py).  The messages are written by
tests/otlp_gogo.py (pdata's encoding) and by google.protobuf
(tests/test_otlp.py to_pb).
"""
import base64
import copy
import ctypes as C
import random

import numpy as np
import pytest

from odigos_amd import host, native
from tests import otlp_gogo as gg
from tests import sqlop_ref as ref
from tests.test_otlp import CFG as OTLP_CFG
from tests.test_otlp import _compare, to_pb
from tests.test_sqlop import SECTION, _flags_of, _size_expectation, _size_tree

Q, O = ref.QUERY_KEY, ref.OPNAME_KEY
SQL_CFGS = {
    "no_list": {},
    "list_matches": {"exclude": {"language": ["python", "5"]}},
    # nothing listed matches, so only the resources without telemetry.sdk.language are excluded
    "missing_language": {"exclude": {"language": ["rust"]}},
}
MARSHAL = {"pdata": gg.marshal_traces, "protobuf": to_pb}
LONG_QUERY = "select " + "x" * (4096 - 7)


def _kv(key, value):
    """value: a Python scalar, or an AnyValue dict ({} = no value set)"""
    if isinstance(value, dict):
        return {"key": key, "value": value}
    return {"key": key, "value": host.attr_value(value)}


def _cases():
    """Attribute lists (in wire order) of the spans: every query case of the decoder."""
    text = "insert into t values (1, 2, 3)"
    out = [
        [],
        [_kv(Q, "SELECT * FROM users WHERE id = ?")],
        [_kv("http.request.method", "GET"), _kv("url.path", "/user/1234"), _kv(Q, "insert into t values (1)")],
    ]
    out += [[_kv(Q, text[:k])] for k in (0, 1, 15, 16, 17)]
    # values that need AsString: every AnyValue kind but string_value
    out += [[_kv(Q, v)] for v in (
        {"intValue": "42"}, {"doubleValue": 2.5}, {"boolValue": True},
        {"bytesValue": base64.b64encode(b"select 1").decode()},
        {"arrayValue": {"values": [{"stringValue": "select 1"}, {"intValue": "2"}]}},
        {"kvlistValue": {"values": [{"key": "a", "value": {"stringValue": "select"}}]}},
        {},
    )]
    out += [
        [_kv(Q, "select 1"), _kv(O, 7)],                    # a non-string db.operation.name
        [_kv(O, {}), _kv("x", 1), _kv(Q, "drop table t")],  # ... with no value at all, before the query
        [_kv(O, "SELECT")],
        [_kv(Q, "delete from t"), _kv(Q, "select 1")],      # the key twice: the first wins
        [_kv(Q, {"intValue": "5"}), _kv(Q, "select 1")],    # ... and a first that needs AsString
        [_kv(Q, "update t set a = 1"), _kv(Q, {"intValue": "5"})],
        # look-alike keys: shorter, longer, same length with another last / first byte
        [_kv("db.query.tex", "select 1"), _kv("db.query.text2", "select 1"), _kv("db.operation.nam", "x")],
        [_kv("db.query.texu", "select 1"), _kv("dc.query.text", "select 1"), _kv("db.operation.namf", "x"),
         _kv("db.operatiom.name", "x")],
        [_kv("db.query.texu", "select 1"), _kv(Q, "alter table t add c int"), _kv("db.operation.namf", "x")],
        # spans the span kernel already hands to the host pass (url.Parse; AsString of a route)
        [_kv("http.request.method", "GET"), _kv("url.full", "https://example.com/api/v1/users/7?x=1"),
         _kv(Q, "create table t")],
        [_kv("http.route", 7), _kv(Q, {"doubleValue": 1.5}), _kv(O, "X")],
        [_kv("http.method", "POST"), _kv("url.full", "https://example.com/a"), _kv("tier", "gold")],
    ]
    return out


RESOURCES = [
    {"service.name": "svc-a", "k8s.pod.name": "pod-0", "telemetry.sdk.language": "go"},
    {"service.name": "svc-b", "k8s.pod.name": "pod-1", "telemetry.sdk.language": "python"},
    {"service.name": "svc-c", "k8s.pod.name": "pod-2"},
    {"service.name": "svc-d", "k8s.pod.name": "pod-3", "telemetry.sdk.language": 5},
    {"service.name": "svc-a", "k8s.pod.name": "pod-1", "telemetry.sdk.language": "java"},
]


def _db_tree(n, seed=1, long_at=None):
    """n spans cycling through _cases() (a 4 KiB query at span long_at) in
    resources with and without telemetry.sdk.language, two scopes in some."""
    rng = random.Random(seed)
    cases = _cases()
    spans = []
    for k in range(n):
        at = copy.deepcopy(cases[k % len(cases)])
        if k == long_at:
            at = [_kv("a", 1), _kv(Q, LONG_QUERY)]
        sp = host.span(name=rng.choice(["GET", "op", "", "query"]), kind=rng.choice([1, 2, 3]),
                       trace_id="%032x" % (1 + k % 7), span_id="%016x" % (k + 1), start=1739000000000000000 + k,
                       end=1739000000000000000 + k + rng.randrange(10 ** 9), status=k % 3)
        sp["attributes"] = at
        if k % 11 == 0:
            sp["events"] = [{"timeUnixNano": "5", "name": "ev", "attributes": [_kv(Q, "select 1")]}]   # not the span's
        spans.append(sp)
    rss = []
    per = max(1, (n + len(RESOURCES) - 1) // len(RESOURCES))
    for r, res in enumerate(RESOURCES):
        part = spans[r * per:(r + 1) * per]
        if not part:
            continue
        if len(part) > 3:
            rss.append(host.resource_spans(res, scopes=[{"scope": {"name": "l0"}, "spans": part[:2]},
                                                        {"scope": {"name": "l1"}, "spans": part[2:]}]))
        else:
            rss.append(host.resource_spans(res, part))
    return host.traces(*rss)


def _full_cfg(sql):
    c = copy.deepcopy(OTLP_CFG)
    c[SECTION] = sql
    return c


def _db_columns(cols, got):
    """(db_flags, query bytes or None, res_sql_ok) of a downloaded OtlpBatch"""
    n, R = cols.n_spans, cols.n_resources
    assert cols.db_flags and cols.db_query and cols.res_sql_ok
    flags = got["db_flags"][:n]
    refs = got["db_query"].view(np.uint32).reshape(-1, 2)[:n]
    arena = got["arena"]
    assert all(int(o) + int(l) <= cols.arena_bytes for o, l in refs)
    queries = [bytes(arena[o:o + l]) if f & native.DB_HAS_QUERY else None for f, (o, l) in zip(flags, refs)]
    return flags, queries, got["res_sql_ok"][:R]


def _needs_as_string(td):
    """spans whose first db.query.text is not a string_value"""
    k = 0
    for rs in td["resourceSpans"]:
        for ss in rs["scopeSpans"]:
            for sp in ss["spans"]:
                v = ref._get(sp.get("attributes"), Q)
                k += v is not None and "stringValue" not in v
    return k


def _check_decode(eng, msg, td, sql, others=True):
    from odigos_amd.batch import OtlpBatch
    ob = OtlpBatch(eng, msg) if isinstance(msg, bytes) else OtlpBatch(eng, msg.p, length=msg.n)
    got = ob.download()
    p = host.Processor(SECTION, sql)
    want_flags, want_queries, want_ok = _flags_of(p, td)
    flags, queries, ok = _db_columns(ob.cols, got)
    np.testing.assert_array_equal(flags, want_flags)
    assert queries == want_queries
    np.testing.assert_array_equal(ok, want_ok)
    assert ob.host_spans >= _needs_as_string(td)
    if others:   # every other column as without the option
        pp = host.Processor("pipeline", _full_cfg(sql))
        hb = pp.columnarize(td)
        _compare(ob.cols, hb.cols, got)
        pp.close()
    p.close()
    return ob


def _sql_engine(sql):
    from odigos_amd.batch import Engine
    eng = Engine(_full_cfg(sql))
    eng.set_option("otlp_sqlop", 1)
    return eng


def test_cases_cover_the_ground():
    td = _db_tree(300, long_at=150)
    p = host.Processor(SECTION, SQL_CFGS["list_matches"])
    flags, queries, ok = _flags_of(p, td)
    lens = {len(q) for q in queries if q is not None}
    assert {0, 1, 15, 16, 17, 4096} <= lens
    assert {0, 1, 2, 3} == set(int(f) for f in flags)
    assert b"42" in queries and b"2.5" in queries and b"true" in queries and b"" in queries
    assert any(q.startswith(b"[") for q in queries if q) and any(q.startswith(b"{") for q in queries if q)
    assert base64.b64encode(b"select 1") in queries          # AsString of bytes
    assert b"delete from t" in queries and b"5" in queries   # the first of two wins
    assert list(ok) == [1, 0, 0, 0, 1]
    assert list(_flags_of(host.Processor(SECTION, SQL_CFGS["missing_language"]), td)[2]) == [1, 1, 0, 1, 1]
    assert _needs_as_string(td) >= 8 * (300 // len(_cases()))


# ---------------------------------------------------------------------------
# GPU: decode

@pytest.mark.gpu
@pytest.mark.parametrize("enc", ["pdata", "protobuf"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_gpu_decode_db_columns(n, enc):
    td = _db_tree(n, seed=n, long_at=n // 2 if n >= 63 else None)
    msg = MARSHAL[enc](td)
    for name, sql in SQL_CFGS.items():
        eng = _sql_engine(sql)
        for _ in range(2):   # cold (resources resolved on the host), then from the device table
            _check_decode(eng, msg, td, sql).close()
        eng.set_option("otlp_host_resources", 1)
        _check_decode(eng, msg, td, sql, others=False).close()
        eng.set_option("otlp_host_resources", 0)
        eng.set_option("otlp_host_scopes", 1)
        _check_decode(eng, msg, td, sql, others=False).close()
        eng.close()


@pytest.mark.gpu
def test_gpu_decode_db_columns_70000_spans():
    # above the LDS-staged span kernel's bound (65536 spans): the HBM-read span
    # kernel runs first.  The message is 100 copies of a 700-span one; so are
    # the expected columns.
    from odigos_amd.batch import OtlpBatch
    td = _db_tree(700, seed=7)
    sql = SQL_CFGS["list_matches"]
    p = host.Processor(SECTION, sql)
    f1, q1, ok1 = _flags_of(p, td)
    eng = _sql_engine(sql)
    ob = OtlpBatch(eng, gg.marshal_traces(td) * 100)
    assert ob.cols.n_spans == 70000
    flags, queries, ok = _db_columns(ob.cols, ob.download())
    np.testing.assert_array_equal(flags, np.tile(f1, 100))
    assert queries == q1 * 100
    np.testing.assert_array_equal(ok, np.tile(ok1, 100))
    assert ob.host_spans >= 100 * _needs_as_string(td)


def _message_ending_in_query(td, query):
    """td's bytes with one more resource whose only span carries `query` as
    its last attribute, the last field of the span: the string ends on the
    message's final byte.  Returns (bytes, the tree they encode)."""
    kvd = _kv(Q, query)
    sp = host.span(name="last", kind=1, trace_id="%032x" % 9, span_id="%016x" % 9, start=5, end=6)
    res = {"service.name": "svc-a", "telemetry.sdk.language": "go"}
    span_b = gg.span(sp) + gg._len(9, gg.key_value(kvd))
    rs_b = gg._len(1, gg._attrs(1, host.attrs(res))) + gg._len(2, gg._len(1, b"") + gg._len(2, span_b))
    msg = gg.marshal_traces(td) + gg._len(1, rs_b)
    assert msg.endswith(query.encode())
    sp["attributes"] = [kvd]
    full = host.traces(*(copy.deepcopy(td["resourceSpans"]) + [host.resource_spans(res, [sp])]))
    return msg, full


@pytest.mark.gpu
@pytest.mark.parametrize("query", ["select 1", "  DROP TABLE t", "x" * 33 + " select"])
def test_gpu_decode_query_at_message_end(query):
    import torch
    from odigos_amd.batch import PinnedBuffer
    msg, td = _message_ending_in_query(_db_tree(20, seed=3), query)
    sql = SQL_CFGS["no_list"]
    eng = _sql_engine(sql)
    pin = PinnedBuffer(msg)
    for m in (msg, pin):
        ob = _check_decode(eng, m, td, sql)
        # the SQLOP stage reads the query's first 16 bytes as a window: the arena's slack holds
        eng.process_device(ob, native.STAGE_SQLOP)
        torch.cuda.synchronize()
        assert int(ob.out_numpy("sql_op", n=ob.cols.n_spans)[-1]) == ref.code(query.encode())
        ob.close()
    pin.close()


@pytest.mark.gpu
def test_gpu_option_toggle():
    from odigos_amd.batch import Engine, OtlpBatch
    td = _db_tree(40, seed=4)
    msg = gg.marshal_traces(td)
    sql = SQL_CFGS["list_matches"]
    eng = Engine(_full_cfg(sql))
    ob = OtlpBatch(eng, msg)   # the default: off
    plain_host_spans = ob.host_spans
    assert not ob.cols.db_flags and not ob.cols.db_query and not ob.cols.res_sql_ok
    ob.close()
    eng.set_option("otlp_sqlop", 1)
    ob = _check_decode(eng, msg, td, sql)
    assert ob.host_spans > plain_host_spans   # the spans whose query needs AsString joined the host pass
    ob.close()
    eng.set_option("otlp_sqlop", 0)
    ob = OtlpBatch(eng, msg)
    assert not ob.cols.db_flags and not ob.cols.db_query and not ob.cols.res_sql_ok
    assert ob.host_spans == plain_host_spans
    for bit in (native.STAGE_SQLOP, native.STAGE_APPLY_SQLOP):
        with pytest.raises(native.OseError) as e:
            ob.encode(native.STAGE_TEMPLATE | bit)
        assert e.value.code == native.OSE_ENOTSUP
    ob.close()


@pytest.mark.gpu
def test_gpu_option_needs_the_section():
    from odigos_amd.batch import Engine
    eng = Engine({"odigosurltemplate": {}, "odigostrafficmetrics": {}})
    for v in (1, 0):
        with pytest.raises(native.OseError) as e:
            eng.set_option("otlp_sqlop", v)
        assert e.value.code == native.OSE_EINVAL and SECTION in str(e.value)


# ---------------------------------------------------------------------------
# GPU: the stages on decoded columns

def _expected_sql_op(sql, td):
    out = []
    for rs in td["resourceSpans"]:
        skip = ref.should_exclude_language(sql, rs["resource"].get("attributes"))
        for ss in rs["scopeSpans"]:
            for sp in ss["spans"]:
                q = ref._get(sp.get("attributes"), Q)
                if skip or q is None or ref._get(sp.get("attributes"), O) is not None:
                    out.append(0)
                else:
                    out.append(ref.code(ref.as_string_simple(q)))
    return np.array(out, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("enc", ["pdata", "protobuf"])
def test_gpu_stages_on_decoded_columns(enc):
    import torch
    from odigos_amd.batch import Engine, OtlpBatch
    S = native
    td = _size_tree(random.Random(5))
    proc, hb, cfg, tree, want_res, want_sets, accepted = _size_expectation(td, 1, with_sampling=False)
    eng = Engine(cfg)
    eng.set_option("otlp_sqlop", 1)
    ob = OtlpBatch(eng, MARSHAL[enc](td))
    n, R, A = ob.cols.n_spans, ob.cols.n_resources, ob.cols.n_attrsets
    assert (n, R, A) == (hb.cols.n_spans, hb.cols.n_resources, hb.cols.n_attrsets)
    ob.o["sql_op"].fill_(0xEE)
    eng.process_device(ob, S.STAGE_TEMPLATE | S.STAGE_SQLOP | S.STAGE_SIZE)
    torch.cuda.synchronize()
    assert int(ob.out_numpy("device_status", np.uint32)[0]) == 0
    want_op = _expected_sql_op(cfg[SECTION], td)
    assert want_op.any() and not want_op.all()
    np.testing.assert_array_equal(ob.out_numpy("sql_op", n=n), want_op)
    np.testing.assert_array_equal(ob.out_numpy("res_bytes", np.uint64, n=R), want_res)
    np.testing.assert_array_equal(ob.out_numpy("attrset_bytes", np.int64, n=A), want_sets)
    assert int(ob.out_numpy("accepted_spans", np.int64)[0]) == accepted
    proc.close()


# ---------------------------------------------------------------------------
# The encoder: the restatement, and the CPU seam against it

OPS = ["", "SELECT", "INSERT", "UPDATE", "DELETE", "CREATE", "DROP", "ALTER"]


def _spans(td):
    return [sp for rs in td["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]


def _applied(td, keep=None, url_out=None, tmpls=None, sql_op=None, drop_all=False):
    """The tree the exporters see: the template decisions (tests/otlp_gogo.apply),
    then processor.go:68-72 per span with sql_op (PutStr replaces the first
    db.operation.name or appends; SetName), then keep."""
    t = gg.apply(td, url_out=url_out, tmpls=tmpls)
    if sql_op is not None:
        for sp, k in zip(_spans(t), sql_op):
            k = int(k)
            if not k:
                continue
            attrs = sp.setdefault("attributes", [])
            kv = gg._find(attrs, O)
            if kv is None:
                attrs.append({"key": O, "value": {"stringValue": OPS[k]}})
            else:
                kv["value"] = {"stringValue": OPS[k]}
            sp["name"] = (sp.get("name") or "") + " " + OPS[k]
    return gg.apply(t, keep=keep, drop_all=drop_all)


def _restate(td, streams=None, pipelines=None, **dec):
    """[(pipeline, TracesData bytes, n_resources)]: _applied, the router's split, pdata's marshaler"""
    t = _applied(td, **dec)
    if streams is None:
        return [("", gg.marshal_traces(t), len(t["resourceSpans"]))]
    return [(p, gg.marshal_traces(x), len(x["resourceSpans"])) for p, x in gg.split_by_pipeline(t, streams, pipelines)]


def _seam(pb, keep=None, url_out=None, tmpls=None, sql_op=None, drop_all=False, router=None, threads=1, old=False):
    from odigos_amd.batch import take_otlp_out
    L = native.lib()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)   # noqa: E731
    keep_a, url_a, sql_a = arr(keep), arr(url_out), arr(sql_op)
    refs = arena = None
    if tmpls is not None:
        bs = [t.encode("utf-8", "surrogateescape") for t in tmpls]
        arena = np.frombuffer(b"".join(bs) + b"\0" * 16, dtype=np.uint8).copy()
        refs = np.zeros((len(bs) + 1, 2), dtype=np.uint32)
        off = 0
        for i, b in enumerate(bs):
            refs[i] = (off, len(b))
            off += len(b)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    h = C.c_void_p()
    args = [pb, len(pb), ptr(keep_a), int(drop_all), ptr(url_a), ptr(refs), ptr(arena),
            0 if arena is None else len(arena) - 16, router.h if router is not None else None, threads, C.byref(h)]
    if old:
        assert sql_op is None
        native.check(L.osehost_otlp_encode(*args))
    else:
        native.check(L.osehost_otlp_encode_sql(*args, ptr(sql_a)))
    return take_otlp_out(L, h)


def _roundtrip(td):
    return host.loads(native.take_bytes(native.lib().osehost_roundtrip(host.dumps(td).encode())).decode("ascii"))


def _mixed_tree(rng, n_traces=40):
    """HTTP traces (tests/test_otlp.py) with DB attributes on some spans: a
    query, a query beside an existing db.operation.name (before or after
    it), a non-string query; routable resources."""
    from tests.test_otlp import _http_traces
    from tests.test_router_encode import _routable
    td = _http_traces(rng, n_traces, odd=0.05)
    for sp in _spans(td):
        r = rng.random()
        q = _kv(Q, rng.choice(["select 1", "DROP TABLE t", "  update t set a=1", "explain x", "", {"intValue": "7"}]))
        if r < 0.35:
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), q)
        elif r < 0.5:
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), q)
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), _kv(O, rng.choice(["OLD", 5, ""])))
        elif r < 0.55:
            sp["attributes"] += [_kv(O, "A"), _kv(O, "B")]   # the key twice: the first is replaced
    return _roundtrip(_routable(td, rng))


def _all_decisions(n, rng):
    """keep x url_out x sql_op: every combination, in random order over the spans"""
    combos = [(k, u, s) for k in (0, 1) for u in (0, 1, 2, 3) for s in range(8)]
    assert n >= len(combos)
    dec = [combos[i % len(combos)] for i in range(n)]
    rng.shuffle(dec)
    keep = [d[0] for d in dec]
    url_out = [d[1] for d in dec]
    sql_op = [d[2] for d in dec]
    tmpls = [rng.choice(["/api/v1/users/{id}", "", "/items/{id}/x"]) if u else "" for u in url_out]
    return keep, url_out, tmpls, sql_op


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("encoding", ["pdata", "protobuf"])
def test_encode_sql_matches_restatement(seed, encoding):
    from tests.test_router_encode import Router, _streams
    rng = random.Random(0x5A1 + seed * 2 + (encoding == "protobuf"))
    td = _mixed_tree(rng)
    pb = MARSHAL[encoding](td)
    n = len(_spans(td))
    keep, url_out, tmpls, sql_op = _all_decisions(n, rng)
    streams = _streams(rng)
    router = Router({"datastreams": streams})
    want = _restate(td, streams, router.pipelines, keep=keep, url_out=url_out, tmpls=tmpls, sql_op=sql_op)
    for threads in (1, 3):
        assert _seam(pb, keep, url_out, tmpls, sql_op, router=router, threads=threads) == want
    # no router: one output
    assert _seam(pb, keep, url_out, tmpls, sql_op) == _restate(td, keep=keep, url_out=url_out, tmpls=tmpls, sql_op=sql_op)
    # sql_op alone (no template stage, nothing dropped)
    assert _seam(pb, sql_op=sql_op, threads=3) == _restate(td, sql_op=sql_op)
    # OSE_GROUP_BATCH, the trace kept and dropped
    assert _seam(pb, None, url_out, tmpls, sql_op, router=router) == \
        _restate(td, streams, router.pipelines, url_out=url_out, tmpls=tmpls, sql_op=sql_op)
    got = _seam(pb, None, url_out, tmpls, sql_op, drop_all=True, router=router)
    assert all(g[1] == b"" and g[2] == 0 for g in got)


def test_encode_sql_null_equals_old_seam():
    from tests.test_router_encode import Router, _decisions, _streams
    rng = random.Random(77)
    td = _mixed_tree(rng, 25)
    router = Router({"datastreams": _streams(rng)})
    keep, url_out, tmpls = _decisions(td, rng)
    for pb in (gg.marshal_traces(td), to_pb(td)):
        for kw in ({}, {"keep": keep}, {"keep": keep, "url_out": url_out, "tmpls": tmpls, "router": router, "threads": 2}):
            assert _seam(pb, **kw) == _seam(pb, old=True, **kw)
    n = len(_spans(td))
    pb = gg.marshal_traces(td)
    assert _seam(pb, keep, url_out, tmpls, [0] * n) == _seam(pb, keep, url_out, tmpls, old=True)


def _padded_span(target_len, **kw):
    """a span whose pdata encoding is exactly target_len bytes (a pad attribute)"""
    pad = max(0, target_len - 100)
    for _ in range(8):
        at = dict(kw.get("attributes") or {})
        at["pad"] = "p" * pad
        sp = host.span(**{**kw, "attributes": at})
        d = target_len - len(gg.span(sp))
        if d == 0:
            return sp
        pad += d
    raise AssertionError("no pad reaches %d" % target_len)


def _edge_cases():
    """(name, tree, decisions)"""
    ids = dict(trace_id="%032x" % 1, span_id="%016x" % 2, start=1739000000000000000, end=1739000000000000005)
    res = {"service.name": "a", "k8s.namespace.name": "prod", "k8s.deployment.name": "api"}
    one = lambda sp, **dec: (host.traces(host.resource_spans(res, sp if isinstance(sp, list) else [sp])), dec)   # noqa: E731
    http = {"http.request.method": "GET", "url.path": "/user/1234"}
    ev = [{"timeUnixNano": "7", "name": "ev", "attributes": host.attrs({"e": 1})}]
    out = {}
    # no name field: " SELECT" at field 5's place (before kind / the times / the attributes)
    out["no_name"] = one([host.span(name="", kind=2, attributes={Q: "select 1"}, **ids),
                          host.span(name="", attributes={Q: "select 1"}), host.span(name="")], sql_op=[1, 6, 7])
    sp = host.span(name="n", status=2, **ids)
    sp["events"] = ev
    sp["droppedEventsCount"] = 2
    out["no_attributes_events_status"] = one(sp, sql_op=[4])
    out["replace_in_place"] = one([host.span(name="x", attributes={"a": 1, O: "OLD", Q: "select 1", "z": "y"}, **ids),
                                   host.span(name="y", attributes={O: 5}), host.span(name="z", attributes={Q: "q", O: ""})],
                                  sql_op=[3, 6, 7])
    # rename + set-attr + sql: http.route appended / replaced; db.operation.name appended / replaced on either side
    spans, n = [], 0
    for route in (None, "/old"):
        for opname in (None, "first", "last"):
            at = {}
            if opname == "first":
                at[O] = "OLD"
            at.update(http)
            if route is not None:
                at["http.route"] = route
            at[Q] = "select 1"
            if opname == "last":
                at[O] = "OLD"
            for kind in (2, 3):   # SERVER: http.route; CLIENT: url.template (appended here)
                s = host.span(name="GET", kind=kind, attributes=at, status=1, **ids)
                s["events"] = ev
                spans.append(s)
                n += 1
    out["rename_set_attr_sql"] = one(spans, url_out=[3] * n, tmpls=["/user/{id}"] * n, sql_op=[1 + k % 7 for k in range(n)])
    out["set_attr_sql"] = one(copy.deepcopy(spans), url_out=[1] * n, tmpls=["/user/{id}"] * n, sql_op=[2] * n)
    out["rename_sql"] = one(copy.deepcopy(spans), url_out=[2] * n, tmpls=[""] * n, sql_op=[6] * n)
    out["dropped_with_sql_op"] = one([host.span(name="a", attributes={Q: "select 1"}, **ids),
                                      host.span(name="b", attributes={Q: "select 1"}, **ids)], keep=[0, 1], sql_op=[1, 1])
    out["name_127_128"] = one([host.span(name="n" * 120, attributes={Q: "s"}, **ids),
                               host.span(name="n" * 121, attributes={Q: "s"}, **ids),
                               host.span(name="n" * 122, attributes={Q: "s"}, **ids),
                               host.span(name="n" * 16377, attributes={Q: "s"}, **ids)], sql_op=[1, 1, 6, 1])
    frames = [_padded_span(L, name="f", kind=1, **ids) for L in (96, 97, 127, 128, 16352, 16353, 16383, 16384)]
    out["framed_length"] = one(frames, sql_op=[1, 1, 6, 6, 1, 1, 6, 6])
    td = host.traces(host.resource_spans(res, [host.span(name="a", attributes={Q: "select 1"}, **ids)]),
                     host.resource_spans({"service.name": "b"}, scopes=[
                         {"scope": {"name": "l"}, "spans": [host.span(name="b", attributes={Q: "drop t"}, **ids)]},
                         {"scope": {}, "spans": [host.span(name="c", **ids)]}]),
                     host.resource_spans({"service.name": "idle"}, scopes=[]))
    out["resource_all_dropped"] = (td, {"keep": [1, 0, 0], "sql_op": [1, 6, 0]})
    return out


def test_edge_frames_cross_the_varint_bounds():
    td, dec = _edge_cases()["framed_length"]
    before = [len(gg.span(s)) for s in _spans(td)]
    assert before == [96, 97, 127, 128, 16352, 16353, 16383, 16384]
    # the KeyValue and " NAME" add 38 bytes (SELECT) or 34 (DROP): the span's own length varint grows
    t = gg.apply(td)
    for sp, k in zip(_spans(t), dec["sql_op"]):
        sp["attributes"].append({"key": O, "value": {"stringValue": OPS[k]}})
        sp["name"] += " " + OPS[k]
    grown = [len(gg.span(s)) for s in _spans(t)]
    assert [b - a for a, b in zip(before, grown)] == [38, 38, 34, 34] * 2
    assert sum(a <= 127 < b for a, b in zip(before, grown)) == 3
    assert sum(a <= 16383 < b for a, b in zip(before, grown)) == 3


@pytest.mark.parametrize("case", sorted(_edge_cases()))
@pytest.mark.parametrize("encoding", ["pdata", "protobuf"])
def test_encode_sql_edge_trees(case, encoding):
    from tests.test_router_encode import Router
    td, dec = _edge_cases()[case]
    td = _roundtrip(td)
    pb = MARSHAL[encoding](td)
    streams = [{"name": "p", "sources": [{"namespace": "prod", "kind": "Deployment", "name": "api"}],
                "destinations": [{"destinationname": "d", "configuredsignals": ["TRACES"]}]}]
    router = Router({"datastreams": streams})
    want = _restate(td, **dec)
    assert want[0][1] != gg.marshal_traces(td)   # the decisions change the bytes
    for threads in (1, 3):
        assert _seam(pb, threads=threads, **dec) == want
    assert _seam(pb, router=router, **dec) == _restate(td, streams, router.pipelines, **dec)


def test_encode_sql_rejects_unknown_code():
    td = _roundtrip(host.traces(host.resource_spans({}, [host.span(name="a")])))
    L = native.lib()
    bad = np.array([8], dtype=np.uint8)
    h = C.c_void_p()
    pb = gg.marshal_traces(td)
    rc = L.osehost_otlp_encode_sql(pb, len(pb), None, 0, None, None, None, 0, None, 1, C.byref(h), bad.ctypes.data)
    assert rc == native.OSE_EINVAL


# ---------------------------------------------------------------------------
# GPU: encode, pipeline, refusals

ST_SQL = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SQLOP | native.STAGE_SIZE


def _gpu_decisions(ob):
    """keep / url_out / templates / sql_op the stages left in the batch's outputs"""
    n = ob.cols.n_spans
    url_out = ob.out_numpy("url_out", n=n)
    refs = ob.out_numpy("tmpl", np.uint32, n=2 * n).reshape(-1, 2)
    arena = ob.out_numpy("tmpl_arena", n=ob.used()).tobytes()
    tmpls = [arena[o:o + ln].decode("utf-8", "surrogateescape") if u else "" for (o, ln), u in zip(refs, url_out)]
    return {"keep": ob.out_numpy("keep", n=n).tolist(), "url_out": url_out.tolist(), "tmpls": tmpls,
            "sql_op": ob.out_numpy("sql_op", n=n).tolist()}


def _canonical_tree(rng, n_traces):
    """_mixed_tree without the values the GPU encoder leaves to the host (AsString methods)"""
    from tests.test_otlp import _http_traces
    from tests.test_router_encode import _routable
    td = _http_traces(rng, n_traces)
    for sp in _spans(td):
        r = rng.random()
        q = _kv(Q, rng.choice(["select 1", "DROP TABLE t", "  update t set a=1", "explain x", "", {"intValue": "7"},
                               "insert into t values (1)", "Alter table t", "delete from t where a = 1"]))
        if r < 0.4:
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), q)
        elif r < 0.5:
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), q)
            sp["attributes"].insert(rng.randrange(len(sp["attributes"]) + 1), _kv(O, rng.choice(["OLD", 5, ""])))
    return _roundtrip(_routable(td, rng))


@pytest.mark.gpu
@pytest.mark.parametrize("group_mode", [native.GROUP_TRACE_ID, native.GROUP_BATCH])
def test_gpu_encode_after_stages(group_mode):
    import torch
    from odigos_amd.batch import OtlpBatch
    from tests.test_router_encode import Router, _streams
    S = native
    rng = random.Random(0x5E7C + group_mode)
    td = _canonical_tree(rng, 250 if group_mode == S.GROUP_TRACE_ID else 12)
    streams = _streams(rng)
    router = Router({"datastreams": streams})
    eng = _sql_engine({})
    apply_bits = S.STAGE_SAMPLE | S.STAGE_TEMPLATE | S.STAGE_APPLY_SQLOP | S.STAGE_SIZE
    ops_seen = set()
    for encoding in ("pdata", "protobuf"):
        ob = OtlpBatch(eng, MARSHAL[encoding](td))
        for seed in (0x0D16F00D, 0x0D16F00E):
            eng.process_device(ob, ST_SQL, group_mode, seed=seed)
            torch.cuda.synchronize()
            assert int(ob.out_numpy("device_status", np.uint32)[0]) == 0
            dec = _gpu_decisions(ob)
            ops_seen |= set(int(x) for x in dec["sql_op"])
            if group_mode == S.GROUP_BATCH:
                del dec["keep"]
                dec["drop_all"] = not int(ob.out_numpy("trace_keep", n=1)[0])
            else:
                assert 0 < sum(dec["keep"]) < len(dec["keep"])
            want = _restate(td, streams, router.pipelines, **dec)
            got = ob.encode(ST_SQL, group_mode, router)
            assert got == want
            if group_mode == S.GROUP_TRACE_ID:   # (OSE_GROUP_BATCH's all-or-nothing is the host encoder's)
                if encoding == "pdata":
                    assert ob.encode_path == {"gpu": True, "fallback": 0}
                else:
                    assert not ob.encode_path["gpu"]
            # sql_op applied as an earlier call's result
            assert ob.encode(apply_bits, group_mode, router) == want
            # without a router, and the host encoder on the same decisions
            assert ob.encode(ST_SQL, group_mode) == _restate(td, **dec)
            eng.set_option("encode_host", 1)
            assert ob.encode(ST_SQL, group_mode, router) == want
            assert not ob.encode_path["gpu"]
            eng.set_option("encode_host", 0)
        ob.close()
    assert ops_seen >= ({0, 1, 2, 3, 4, 6, 7} if group_mode == S.GROUP_TRACE_ID else {0, 1})


@pytest.mark.gpu
def test_gpu_encode_edge_trees():
    """The CPU seam's edge trees through ose_otlp_encode with forced decisions: the GPU encoder writes them."""
    import torch
    from odigos_amd.batch import OtlpBatch
    eng = _sql_engine({})
    st = native.STAGE_APPLY_KEEP | native.STAGE_TEMPLATE | native.STAGE_APPLY_SQLOP
    for case, (td, dec) in sorted(_edge_cases().items()):
        td = _roundtrip(td)
        ob = OtlpBatch(eng, gg.marshal_traces(td), tmpl_cap=4096)
        n = ob.cols.n_spans
        keep = dec.get("keep") or [1] * n
        url_out = dec.get("url_out") or [0] * n
        tmpls = dec.get("tmpls") or [""] * n
        arena = "".join(tmpls).encode()
        refs = np.zeros((n, 2), dtype=np.uint32)
        off = 0
        for i, t in enumerate(tmpls):
            refs[i] = (off, len(t.encode()))
            off += len(t.encode())
        put = lambda name, a: ob.o[name][:len(a)].copy_(torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()))   # noqa: E731
        put("keep", bytes(keep))
        put("url_out", bytes(url_out))
        put("sql_op", bytes(dec["sql_op"]))
        put("tmpl", refs.tobytes())
        if arena:
            put("tmpl_arena", arena)
        ob.o["used"][0] = len(arena)
        torch.cuda.synchronize()
        got = ob.encode(st)
        assert got == _restate(td, keep=keep, url_out=url_out, tmpls=tmpls, sql_op=dec["sql_op"]), case
        assert ob.encode_path == {"gpu": True, "fallback": 0}, case
        ob.close()


def _keep_all_cfg():
    return {"odigossampling": {"global_rules": [{"name": "errors", "type": "error",
                                                 "rule_details": {"fallback_sampling_ratio": 100}}]},
            "odigosurltemplate": {}, SECTION: {},
            "odigostrafficmetrics": {"res_attributes_keys": ["service.name", "k8s.pod.name"]}}


@pytest.mark.gpu
def test_gpu_pipeline_with_sqlop():
    import threading

    import torch
    from odigos_amd.batch import Engine, OtlpBatch, OtlpPipeline
    from tests.test_router_encode import Router, _streams
    rng = random.Random(0x919E)
    streams = _streams(rng)
    router = Router({"datastreams": streams})
    eng = Engine(_keep_all_cfg())
    eng.set_option("otlp_sqlop", 1)
    n_req = 8
    trees = [_canonical_tree(rng, 35) for _ in range(n_req)]
    reqs = [gg.marshal_traces(t) for t in trees]
    assert all(150 <= len(_spans(t)) <= 300 for t in trees)
    want, size = [], 0
    for td, pb in zip(trees, reqs):   # the GPU's own decisions for each request, from the ordinary calls
        ob = OtlpBatch(eng, pb)
        eng.process_device(ob, ST_SQL, native.GROUP_TRACE_ID, seed=0x5EED)
        torch.cuda.synchronize()
        dec = _gpu_decisions(ob)
        assert all(dec["keep"]) and any(dec["sql_op"]) and any(dec["url_out"])
        want.append(_restate(td, streams, router.pipelines, **dec))
        size += sum(len(gg.resource_spans(rs)) for rs in _applied(td, **dec)["resourceSpans"])
        ob.close()
    pipe = OtlpPipeline(eng, router, stages=ST_SQL)
    pipe.hold(n_req)
    got, errs = [None] * n_req, [None] * n_req

    def run(k):
        try:
            got[k] = pipe.consume(reqs[k], seed=0x5EED)
        except Exception as ex:   # noqa: BLE001
            errs[k] = ex

    th = [threading.Thread(target=run, args=(k,)) for k in range(n_req)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert errs == [None] * n_req
    c = pipe.counters()
    assert c["batches"] == 1 and c["batched_requests"] == n_req and c["alone"] == 0, c
    for g, w in zip(got, want):
        assert g == w
    assert sum(v for _, v in c["data_size"]) == size
    assert c["accepted_spans"] == sum(len(_spans(t)) for t in trees)
    # a request alone takes the fallback path: the same bytes
    alone = OtlpPipeline(eng, router, stages=ST_SQL)
    assert alone.consume(reqs[0], seed=0x5EED) == want[0]
    assert alone.counters()["alone"] == 1
    pipe.close()
    alone.close()


@pytest.mark.gpu
def test_gpu_otlp_sqlop_refusals():
    import torch
    from odigos_amd.batch import Engine, OtlpBatch
    S = native
    td = _roundtrip(host.traces(host.resource_spans({"service.name": "a"}, [
        host.span(name="s", trace_id="%032x" % 1, span_id="%016x" % 1, attributes={Q: "select 1"})])))
    eng = _sql_engine({})
    ob = OtlpBatch(eng, gg.marshal_traces(td))
    eng.process_device(ob, S.STAGE_TEMPLATE | S.STAGE_SQLOP)
    torch.cuda.synchronize()
    with pytest.raises(native.OseError) as e:   # both bits
        ob.encode(S.STAGE_TEMPLATE | S.STAGE_SQLOP | S.STAGE_APPLY_SQLOP)
    assert e.value.code == S.OSE_EINVAL
    saved = ob.outs.sql_op
    ob.outs.sql_op = None
    for bit in (S.STAGE_SQLOP, S.STAGE_APPLY_SQLOP):
        with pytest.raises(native.OseError) as e:
            ob.encode(S.STAGE_TEMPLATE | bit)
        assert e.value.code == S.OSE_EINVAL and "sql_op" in str(e.value)
    ob.outs.sql_op = saved
    assert ob.encode(S.STAGE_TEMPLATE | S.STAGE_SQLOP) == _restate(td, sql_op=[1])
    h = C.c_void_p()
    L = native.lib()
    assert L.ose_otlp_pipeline_create(eng.h, None, S.STAGE_TEMPLATE | S.STAGE_APPLY_SQLOP, 0, C.byref(h)) == S.OSE_EINVAL
    assert L.ose_otlp_pipeline_create(eng.h, None, S.STAGE_TEMPLATE | S.STAGE_SQLOP | S.STAGE_APPLY_TEMPLATE, 0,
                                      C.byref(h)) == S.OSE_EINVAL
    # the option is read when the pipeline is created
    eng.set_option("otlp_sqlop", 0)
    assert L.ose_otlp_pipeline_create(eng.h, None, S.STAGE_TEMPLATE | S.STAGE_SQLOP, 0, C.byref(h)) == S.OSE_ENOTSUP
    ob.close()
    # an engine without the section cannot turn the option on
    plain = Engine({"odigosurltemplate": {}})
    with pytest.raises(native.OseError) as e:
        plain.set_option("otlp_sqlop", 1)
    assert e.value.code == S.OSE_EINVAL
