"""odigossqldboperationprocessor as the SQLOP stage.

CPU: the Python restatement (tests/sqlop_ref.py) against the golden cases
(tests/golden/sqldbop_kats.json: the reference's processor_test.go cases and
a hand-derived table of edge cases), the host-compiled classifier
(osehost_sqlop_detect, the source the kernel's general path compiles) against
the restatement, config decoding, and the columns the host walk fills.

GPU: sql_op against the restatement through ose_process and
ose_process_device, an adversarial batch across the 16-byte window of the
kernel's fast path, the size stage after SQLOP against the marshalled size of
the restatement-mutated tree, the drop-in processors, the refusals and a
hipGraph capture.
"""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import host, native
from tests import otlp_gogo as gg
from tests import sqlop_ref as ref
from tests.oracle_lib import SamplingOracle, UrlOracle
from tests.workloads import c3_sampling_config

GOLDEN = json.loads((Path(__file__).parent / "golden" / "sqldbop_kats.json").read_text())
SECTION = "odigossqldboperationprocessor"


def golden_queries():
    """[(query bytes, expected name)] of every golden case with a query."""
    out = [(c["query"].encode(), c["expected"]) for c in GOLDEN["set_db_operation_name"]]
    assert GOLDEN["derived_cases"]["derived"] is True
    out += [(bytes.fromhex(c["query_hex"]), c["expected"]) for c in GOLDEN["derived_cases"]["cases"]]
    return out


# ---------------------------------------------------------------------------
# the fragment alphabet of the random strings

def _enc(r: int) -> bytes:
    return chr(r).encode("utf-8")


SPACE_RUNES = [_enc(r) for r in [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B),
                                 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]]
ASCII_BLANKS = [b" ", b"\t", b"\n", b"\r", b"\v", b"\f"]
NEAR_SPACE = [_enc(0x200B), _enc(0xFEFF), b"\x1c", b"\x1f"]
INVALID = [b"\xff", b"\xa0", b"\x85", b"\xe2", b"\xc2", b"\xe2\x80", b"\xe3\x80", b"\xc0\xa0", b"\x80", b"\xe1\x9a"]
DELIMS = [b" ", b"\t", b"\n"]
NON_DELIMS = [b"\r", b"\v", b"\f", b";", b"(", b"\x00", b"x", b"*"]
NEAR_WORDS = [b"SELEC", b"SELECTX", b"selects", b"DROPS", b"DRO", b"ALTE", b"ALTERS", b"INSERTED", b"UPDAT", b"DELETED",
              b"CREAT", b"SEL\xc3\x89CT", b"\xe2\x84\xaaELECT", b"S\xc4\xb0NSERT", b"1SELECT", b"_DROP", b"EXEC", b"WITH"]
TAILS = [b"* FROM users WHERE id = ?", b"INTO t VALUES (1)", b"t SET a = 1", b"TABLE t", b"1", b""]


def space_run(rng, max_bytes, runes=SPACE_RUNES):
    n = rng.randrange(0, max_bytes + 1)
    out = b""
    while True:
        r = rng.choice(runes)
        if len(out) + len(r) > n:
            return out
        out += r


def keyword(rng) -> bytes:
    out = b""
    for ch in rng.choice(ref.KEYWORDS):
        x = rng.random()
        if ch == "S" and x < 0.12:
            out += b"\xc5\xbf"      # U+017F
        elif ch == "I" and x < 0.12:
            out += b"\xc4\xb1"      # U+0131
        else:
            out += (ch.lower() if x < 0.56 else ch).encode()
    return out


def rand_query(rng) -> bytes:
    x = rng.random()
    lead = b"" if x < 0.35 else space_run(rng, 40, ASCII_BLANKS if x < 0.7 else SPACE_RUNES)
    if rng.random() < 0.06:
        lead += rng.choice(NEAR_SPACE + INVALID)
    word = keyword(rng) if rng.random() < 0.8 else rng.choice(NEAR_WORDS)
    x = rng.random()
    if x < 0.15:
        rest = b""
    elif x < 0.50:
        rest = rng.choice(DELIMS) + space_run(rng, 6) + rng.choice(TAILS)
    elif x < 0.75:
        rest = space_run(rng, 40, ASCII_BLANKS if rng.random() < 0.5 else SPACE_RUNES)
    elif x < 0.85:
        rest = rng.choice(NON_DELIMS) + rng.choice(TAILS)
    elif x < 0.93:
        rest = space_run(rng, 20) + rng.choice(NEAR_SPACE + INVALID + [b"x"]) + space_run(rng, 4)
    else:
        rest = rng.choice(INVALID + NEAR_SPACE)
    return lead + word + rest


# ---------------------------------------------------------------------------
# CPU

def test_restatement_matches_golden():
    for q, want in golden_queries():
        assert ref.detect(q) == want, q
    # the two whole-processor cases of processor_test.go
    ex = GOLDEN["existing_db_operation_name"]
    td = host.traces(host.resource_spans({}, [host.span(name="s", attributes={ref.QUERY_KEY: ex["query"],
                                                                           ref.OPNAME_KEY: ex["existing"]})]))
    assert ref.process_traces({}, td) == td
    td = host.traces(host.resource_spans({}, [host.span(name="s")]))
    assert ref.process_traces({}, td) == td
    td = host.traces(host.resource_spans({}, [host.span(name="s", attributes={ref.QUERY_KEY: "SELECT * FROM users"})]))
    sp = ref.process_traces({}, td)["resourceSpans"][0]["scopeSpans"][0]["spans"][0]
    assert sp["name"] == "s SELECT" and sp["attributes"][-1] == {"key": ref.OPNAME_KEY, "value": {"stringValue": "SELECT"}}


def test_restatement_differs_from_python_strip():
    # the runes where Go's unicode.IsSpace and Python's strip() part ways
    assert ref.detect(b"\x1cSELECT 1") == "UNKNOWN" and "\x1cSELECT 1".strip().startswith("SELECT")
    assert ref.detect("\u0085SELECT 1".encode()) == "SELECT"
    assert ref.detect((chr(0x200B) + "SELECT 1").encode()) == "UNKNOWN"
    assert ref.detect((chr(0xFEFF) + "SELECT 1").encode()) == "UNKNOWN"
    assert ref.to_upper(chr(0xFB05).encode()) == chr(0xFB05).encode()   # no full case mapping (str.upper: "ST")


def host_detect(q: bytes) -> int:
    return native.lib().osehost_sqlop_detect(q, len(q))


def test_host_classifier_matches_golden():
    for q, want in golden_queries():
        assert native.SQLOP_NAMES[host_detect(q)] == want, q


def test_host_classifier_matches_restatement_random():
    rng = random.Random(0x5A10)
    seen = [0] * 8
    for _ in range(50_000):
        q = rand_query(rng)
        want = ref.code(q)
        assert host_detect(q) == want, q
        seen[want] += 1
    assert all(s >= 1000 for s in seen), seen   # every keyword and UNKNOWN well covered


def _create(cfg) -> int:
    h = C.c_void_p()
    return native.lib().ose_engine_create(host.dumps(cfg).encode(), C.byref(h))


def test_config_decoding():
    # accepted forms: Validate never fails (config.go:20-23)
    for cfg in ({}, None, {"exclude": None}, {"exclude": {}}, {"exclude": {"language": None}}, {"exclude": {"language": []}},
                {"exclude": {"language": ["python", "java"]}}):
        host.Processor(SECTION, cfg).close()
        host.Processor("pipeline", {SECTION: cfg, "odigosurltemplate": {}}).close()
    # type errors
    for cfg, msg in (([], "expected a map"), ("x", "expected a map"), ({"exclude": []}, "expected a map"),
                     ({"exclude": {"language": "python"}}, "must be an array or slice"),
                     ({"exclude": {"language": [1]}}, "expected type 'string'")):
        with pytest.raises(ValueError, match=msg):
            host.Processor("pipeline", {SECTION: cfg})
        # ose_engine_create refuses them before touching a device
        assert _create({SECTION: cfg}) == native.OSE_EINVAL
        assert msg in native.last_error()


def _flags_of(proc, td):
    hb = proc.columnarize(td)
    c = hb.cols
    n, R = c.n_spans, c.n_resources
    flags = np.ctypeslib.as_array((C.c_uint8 * n).from_address(c.db_flags)).copy()
    refs = np.ctypeslib.as_array((C.c_uint32 * (2 * n)).from_address(c.db_query)).reshape(n, 2).copy()
    arena = bytes((C.c_uint8 * c.arena_bytes).from_address(c.arena)) if c.arena_bytes else b""
    ok = np.ctypeslib.as_array((C.c_uint8 * R).from_address(c.res_sql_ok)).copy()
    queries = [arena[o:o + l] if f & native.DB_HAS_QUERY else None for f, (o, l) in zip(flags, refs)]
    return flags, queries, ok


def test_columnarize_flags():
    Q, O = native.DB_HAS_QUERY, native.DB_HAS_OPNAME
    m = {"kvlistValue": {"values": [{"key": "a", "value": {"stringValue": "select"}}]}}
    spans = [
        host.span(name="a", attributes={ref.QUERY_KEY: "SELECT 1"}),
        host.span(name="b", attributes={ref.QUERY_KEY: 42}),
        host.span(name="c", attributes={ref.QUERY_KEY: m}),
        host.span(name="d", attributes={ref.QUERY_KEY: "select 1", ref.OPNAME_KEY: 7}),
        host.span(name="e", attributes={ref.OPNAME_KEY: "SELECT"}),
        host.span(name="f"),
        host.span(name="g", attributes={ref.QUERY_KEY: ""}),
    ]
    td = host.traces(host.resource_spans({"telemetry.sdk.language": "go"}, spans),
                     host.resource_spans({"service.name": "x"}, [host.span(name="h", attributes={ref.QUERY_KEY: "drop t"})]),
                     host.resource_spans({"telemetry.sdk.language": "python"}, []),
                     host.resource_spans({"telemetry.sdk.language": 5}, []))
    p = host.Processor(SECTION, {"exclude": {"language": ["python", "5"]}})
    flags, queries, ok = _flags_of(p, td)
    assert list(flags) == [Q, Q, Q, Q | O, O, 0, Q, Q]
    assert queries[0] == b"SELECT 1" and queries[1] == b"42" and queries[6] == b"" and queries[7] == b"drop t"
    assert queries[2] == host.as_string(m).encode() and queries[2].startswith(b"{")
    # go passes; no telemetry.sdk.language under a non-empty list: excluded;
    # python listed; the Int 5 excluded through AsString
    assert list(ok) == [1, 0, 0, 0]
    # without a list nothing is excluded
    for cfg in ({}, {"exclude": {}}, {"exclude": {"language": []}}):
        assert list(_flags_of(host.Processor(SECTION, cfg), td)[2]) == [1, 1, 1, 1]
    # a processor without the section leaves the columns NULL
    hb = host.Processor("odigosurltemplate", {}).columnarize(td)
    assert not hb.cols.db_flags and not hb.cols.db_query and not hb.cols.res_sql_ok and not hb.outs.sql_op


def test_engine_info_and_abi_version():
    hdr = (Path(__file__).parent.parent / "include" / "odigos_amd.h").read_text()
    assert "#define OSE_ABI_VERSION 5" in hdr
    for name, val in (("OSE_STAGE_SQLOP", native.STAGE_SQLOP), ("OSE_STAGE_APPLY_SQLOP", native.STAGE_APPLY_SQLOP)):
        assert f"#define {name}" in hdr and hex(val) in hdr.lower()
    # appended at the end: every earlier field keeps its offset
    assert native.Columns.attr_val.offset + 8 == native.Columns.db_flags.offset == C.sizeof(native.Columns) - 24
    assert native.Outputs.device_status.offset + 8 == native.Outputs.sql_op.offset
    assert native.Outputs.sql_op.offset == C.sizeof(native.Outputs) - 8


# ---------------------------------------------------------------------------
# GPU

class SqlBatch:
    """Host columns for the SQLOP stage built in numpy: query k at arena
    alignment k % 16; the arena ends with the last query's last byte."""

    def __init__(self, queries, flags, resource, res_ok):
        n = len(queries)
        self.n = n
        refs = np.zeros((max(n, 1), 2), dtype=np.uint32)
        buf = bytearray()
        for k, q in enumerate(queries):
            buf += bytes((k % 16 - len(buf) % 16) % 16)
            refs[k] = (len(buf), len(q))
            buf += q
        self.arena_bytes = len(buf)
        self.arena = np.zeros((len(buf) + 15) // 16 * 16 + 16, dtype=np.uint8)
        self.arena[:len(buf)] = np.frombuffer(bytes(buf), dtype=np.uint8)
        self.refs = refs
        self.flags = np.ascontiguousarray(np.resize(np.asarray(flags, dtype=np.uint8), max(n, 1)))
        self.resource = np.ascontiguousarray(np.resize(np.asarray(resource, dtype=np.uint32), max(n, 1)))
        self.res_ok = None if res_ok is None else np.ascontiguousarray(np.asarray(res_ok, dtype=np.uint8))
        self.R = int(max(resource) + 1) if n else 1
        c = native.Columns()
        c.n_spans, c.n_resources, c.arena_bytes = n, self.R, self.arena_bytes
        c.arena = self.arena.ctypes.data
        c.db_flags, c.db_query, c.resource = self.flags.ctypes.data, self.refs.ctypes.data, self.resource.ctypes.data
        if self.res_ok is not None:
            c.res_sql_ok = self.res_ok.ctypes.data
        self.cols = c
        self.queries = queries

    def want(self):
        out = np.zeros(self.n, dtype=np.uint8)
        for k, q in enumerate(self.queries):
            ok = 1 if self.res_ok is None else self.res_ok[self.resource[k]]
            if ok and (self.flags[k] & 3) == native.DB_HAS_QUERY:
                out[k] = ref.code(q)
        return out


def run_device(eng, sb):
    import torch
    from odigos_amd.batch import DeviceBatch
    db = DeviceBatch(sb.cols)
    db.o["sql_op"].fill_(0xEE)
    eng.process_device(db, native.STAGE_SQLOP)
    torch.cuda.synchronize()
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    return db.out_numpy("sql_op", n=sb.n)


def run_pinned(eng, sb):
    from odigos_amd.batch import PinnedBatch
    pb = PinnedBatch(eng, sb.cols)
    pb.fill(sb.cols)
    pb.process(native.STAGE_SQLOP)
    got = np.ctypeslib.as_array((C.c_uint8 * max(sb.n, 1)).from_address(pb.outs.sql_op))[:sb.n].copy()
    pb.close()
    return got


@pytest.mark.gpu
def test_gpu_golden_cases():
    from odigos_amd.batch import Engine
    eng = Engine({SECTION: {}})
    assert eng.info().stages == native.STAGE_SQLOP
    qs = golden_queries()
    sb = SqlBatch([q for q, _ in qs], [native.DB_HAS_QUERY] * len(qs), [0] * len(qs), None)
    want = np.array([ref.CODES[w] for _, w in qs], dtype=np.uint8)
    np.testing.assert_array_equal(sb.want(), want)
    np.testing.assert_array_equal(run_device(eng, sb), want)
    np.testing.assert_array_equal(run_pinned(eng, sb), want)


def adversarial_batch(with_res: bool):
    rng = random.Random(0xADBA7C4)
    n, R = 4099, 37
    queries = [rand_query(rng) for _ in range(n)]
    queries[7] = b""
    queries[1000] = b" " * 70_000 + b"update x"
    queries[2000] = b"\t" * 16 + b"drop t"          # the blanks fill the window exactly
    queries[2001] = b" " * 10 + b"SELECT"            # the keyword ends with the window
    queries[2002] = b" " * 10 + b"SELECT\r"
    queries[2003] = b" " * 11 + b"SELECT 1"          # the keyword crosses the window's end
    queries[n - 1] = b"  alter table t"              # its last byte is the arena's last byte
    flags = [rng.choice([1, 1, 1, 1, 1, 1, 1, 1, 0, 2, 3, 3]) for _ in range(n)]
    for k in (7, 1000, 2000, 2001, 2002, 2003, n - 1):
        flags[k] = native.DB_HAS_QUERY
    resource = sorted(rng.randrange(R) for _ in range(n))
    resource[-1] = R - 1
    res_ok = [0 if rng.random() < 0.12 else 1 for _ in range(R)] if with_res else None
    if res_ok:
        for k in (7, 1000, 2000, 2001, 2002, 2003, n - 1):
            res_ok[resource[k]] = 1
    return SqlBatch(queries, flags, resource, res_ok)


def test_adversarial_batch_covers_the_ground():
    # checkable without a device: on the restatement's output alone
    sb = adversarial_batch(True)
    want = sb.want()
    assert sb.arena_bytes == int(sb.refs[-1][0]) + int(sb.refs[-1][1])
    assert sorted(set(int(o) % 16 for o, _ in sb.refs)) == list(range(16))
    for op in range(1, 8):
        assert int((want == op).sum()) >= 100, (op, int((want == op).sum()))
    active = np.array([(sb.flags[k] & 3) == 1 and sb.res_ok[sb.resource[k]] for k in range(sb.n)])
    has_q = (sb.flags[:sb.n] & 1) == 1
    unknown = sum(1 for k in range(sb.n) if has_q[k] and ref.code(sb.queries[k]) == 0)
    assert unknown >= 500, unknown
    assert int((~active).sum()) >= 200
    assert want[1000] == native.SQLOP_UPDATE and want[7] == 0 and want[sb.n - 1] == native.SQLOP_ALTER
    assert list(want[2000:2004]) == [native.SQLOP_DROP, native.SQLOP_SELECT, native.SQLOP_SELECT, native.SQLOP_SELECT]


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False])
def test_gpu_adversarial_batch(with_res):
    from odigos_amd.batch import Engine
    eng = Engine({SECTION: {"exclude": {"language": ["x"]}}})
    sb = adversarial_batch(with_res)
    want = sb.want()
    got = run_device(eng, sb)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(k), sb.queries[k][:60], int(got[k]), int(want[k])) for k in bad[:5]]
    np.testing.assert_array_equal(run_pinned(eng, sb), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_gpu_sizes(n):
    from odigos_amd.batch import Engine
    eng = Engine({SECTION: {}})
    rng = random.Random(n)
    qs = [rand_query(rng) for _ in range(n)]
    sb = SqlBatch(qs, [native.DB_HAS_QUERY] * n, [0] * n, None)
    np.testing.assert_array_equal(run_device(eng, sb), sb.want())
    np.testing.assert_array_equal(run_pinned(eng, sb), sb.want())


# ---- SIZE after SQLOP ------------------------------------------------------

TRAFFIC = {"res_attributes_keys": ["service.name", "k8s.namespace.name"]}
SQL_CFG = {"exclude": {"language": ["python"]}}


def _size_tree(rng, matching=True):
    """About 40 spans in 3 resources: names of length 0, 120-127 and
    16376-16383 (the name varint crosses 1 -> 2 and 2 -> 3 bytes when " OP" is
    appended), spans whose sizes straddle 127 / 128, spans the URL stage also
    renames and templates, several trace ids, one excluded resource."""
    name_lens = [0, 1, 5, 17, 30, 44, 58] + list(range(120, 128)) + list(range(16376, 16384))
    qs = ["select 1", "DROP TABLE t", "alter table t add c int", "INSERT INTO t VALUES (1)", " \t update t set a=1",
          "delete from t", "create table t", "explain select 1", "SELECT;"]
    if not matching:
        qs = ["explain select 1", "SELECT;", "(select 1)", ""]
    spans = []
    for k, nl in enumerate(name_lens):
        spans.append(host.span(name="n" * nl, kind=1, trace_id="%032x" % (1 + k % 5), span_id="%016x" % (k + 1),
                               start=1739000000000000000 + k, end=1739000002000000000, status=[0, 0, 2][k % 3],
                               attributes={ref.QUERY_KEY: qs[k % len(qs)]}))
    for k in range(8):   # the URL stage renames these (name == method) and sets http.route
        at = {"http.request.method": "GET", "url.path": "/user/%d" % (1000 + k)}
        if k != 3:
            at[ref.QUERY_KEY] = qs[k % len(qs)]
        if k == 5:
            at[ref.OPNAME_KEY] = "EXISTING"
        spans.append(host.span(name="GET", kind=[2, 3][k % 2], trace_id="%032x" % (1 + k % 5), span_id="%016x" % (100 + k),
                               start=1739000000000000000, end=1739000000000000000 + rng.randrange(10**9, 3 * 10**9),
                               status=[0, 2][k % 2], attributes=at))
    for k in range(9):   # no query at all
        spans.append(host.span(name="plain", kind=1, trace_id="%032x" % (1 + k % 5), span_id="%016x" % (200 + k)))
    rng.shuffle(spans)
    a, b = len(spans) // 3, 2 * len(spans) // 3
    # traces stay inside one resource (one service), so the service rules drop some and keep others
    for j, sp_ in enumerate(spans):
        sp_["traceId"] = "%032x" % ((1 + j % 2) if j < a else (3 + j % 2) if j < b else (5 + j % 5))
    return host.traces(
        host.resource_spans({"service.name": "svc-00", "k8s.namespace.name": "ns0", "telemetry.sdk.language": "go"},
                            scopes=[{"scope": {"name": "l0"}, "spans": spans[:a // 2]}, {"scope": {}, "spans": []},
                                    {"scope": {"name": "l1"}, "spans": spans[a // 2:a]}]),
        host.resource_spans({"service.name": "svc-02", "k8s.namespace.name": "ns1", "telemetry.sdk.language": "python"},
                            spans[a:b]),
        host.resource_spans({"service.name": "svc-01", "k8s.namespace.name": "ns0", "telemetry.sdk.language": "java"},
                            spans[b:]))


def _size_expectation(td, seed, with_sampling=True):
    """(host batch, expected res_bytes per original resource, expected
    attrset sums, expected accepted spans): sampling and templating by the
    CPU oracle, odigossqldboperationprocessor by the restatement, sizes by
    marshalling the resulting tree (tests/otlp_gogo.py)."""
    cfg = {"odigosurltemplate": {}, SECTION: SQL_CFG, "odigostrafficmetrics": TRAFFIC}
    if with_sampling:
        cfg["odigossampling"] = c3_sampling_config()
    proc = host.Processor("pipeline", cfg)
    proc.configure(seed, native.GROUP_TRACE_ID)
    hb = proc.columnarize(td)
    c, o = hb.cols, hb.outs
    n, R = c.n_spans, c.n_resources
    if with_sampling:
        assert SamplingOracle(cfg["odigossampling"]).process(c, o, native.GROUP_TRACE_ID, seed) == 0
    assert UrlOracle({}).process(c, o) == 0
    tree = ref.process_traces(SQL_CFG, hb.apply())   # sql_op is all zero here: apply does sampling + templating only
    sizes = [len(gg.resource_spans(rs)) for rs in tree["resourceSpans"]]
    sets = np.ctypeslib.as_array((C.c_uint32 * R).from_address(c.res_attrset))
    # the surviving resources, by their (unique) service.name
    svc = lambda rs: host.find_attr(rs["resource"], "service.name")["stringValue"]
    by_svc = {svc(rs): sz for rs, sz in zip(tree["resourceSpans"], sizes)}
    assert len(by_svc) == len(sizes)
    want_res = np.array([by_svc.get(svc(rs), 0) for rs in td["resourceSpans"]], dtype=np.uint64)
    want_sets = np.zeros(c.n_attrsets, dtype=np.int64)
    for r in range(R):
        want_sets[sets[r]] += int(want_res[r])
    accepted = sum(len(ss["spans"]) for rs in tree["resourceSpans"] for ss in rs["scopeSpans"])
    return proc, hb, cfg, tree, want_res, want_sets, accepted


def _counters(db, hb):
    R, A = hb.cols.n_resources, hb.cols.n_attrsets
    return (db.out_numpy("res_bytes", np.uint64, n=R), db.out_numpy("attrset_bytes", np.int64, n=A),
            int(db.out_numpy("accepted_spans", np.int64)[0]))


def test_size_tree_covers_the_edges():
    td = _size_tree(random.Random(5))
    before = [sp for rs in td["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]
    after_t = ref.process_traces({}, td)
    after = [sp for rs in after_t["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]
    grown = [(len(gg.span(a)), len(gg.span(b))) for a, b in zip(before, after) if a != b]
    assert len(before) in range(36, 48) and len(grown) >= 15
    assert any(x <= 127 < y for x, y in grown)                       # a span's own length varint grows
    names = {len(a["name"]): len(b["name"]) for a, b in zip(before, after) if a != b}
    assert any(x <= 127 < y for x, y in names.items()) and any(x <= 16383 < y for x, y in names.items())
    assert 0 in names and names[0] in (5, 6, 7)                      # "" -> " DROP" ...


@pytest.mark.gpu
def test_gpu_size_after_sqlop():
    import torch
    from odigos_amd.batch import DeviceBatch, Engine
    td = _size_tree(random.Random(5))
    S = native
    dropped_some = False
    for seed in (0x0D21, 0x0D22, 0x0D23):
        proc, hb, cfg, tree, want_res, want_sets, accepted = _size_expectation(td, seed)
        n_in = hb.cols.n_spans
        dropped_some |= 0 < accepted < n_in
        eng = Engine(cfg)
        db = DeviceBatch(hb.cols)
        eng.process_device(db, S.STAGE_SAMPLE | S.STAGE_TEMPLATE | S.STAGE_SQLOP | S.STAGE_SIZE, S.GROUP_TRACE_ID, seed=seed)
        torch.cuda.synchronize()
        assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
        rb, ab, acc = _counters(db, hb)
        print("seed", hex(seed), "res_bytes", rb.tolist(), "want", want_res.tolist(), "accepted", acc, accepted)
        np.testing.assert_array_equal(rb, want_res)
        np.testing.assert_array_equal(ab, want_sets)
        assert acc == accepted
        # the same through the APPLY bits, on the outputs the first call left
        for name in ("attrset_bytes", "accepted_spans", "res_bytes"):
            db.o[name].zero_()
        eng.process_device(db, S.STAGE_APPLY_KEEP | S.STAGE_APPLY_TEMPLATE | S.STAGE_APPLY_SQLOP | S.STAGE_SIZE,
                           S.GROUP_TRACE_ID, seed=seed)
        torch.cuda.synchronize()
        rb2, ab2, acc2 = _counters(db, hb)
        np.testing.assert_array_equal(rb2, want_res)
        np.testing.assert_array_equal(ab2, want_sets)
        assert acc2 == accepted
        proc.close()
        eng.close()
    assert dropped_some   # some seed dropped traces and kept others


@pytest.mark.gpu
def test_gpu_size_sqlop_without_matches_equals_plain_mask():
    import torch
    from odigos_amd.batch import DeviceBatch, Engine
    td = _size_tree(random.Random(6), matching=False)
    proc, hb, cfg, tree, want_res, want_sets, accepted = _size_expectation(td, 1, with_sampling=False)
    eng = Engine(cfg)
    S = native
    got = []
    for mask in (S.STAGE_TEMPLATE | S.STAGE_SQLOP | S.STAGE_SIZE, S.STAGE_TEMPLATE | S.STAGE_SIZE,
                 S.STAGE_TEMPLATE | S.STAGE_TEMPLATE_REFS | S.STAGE_SQLOP | S.STAGE_SIZE):
        db = DeviceBatch(hb.cols)
        eng.process_device(db, mask)
        torch.cuda.synchronize()
        got.append(_counters(db, hb))
        if mask & S.STAGE_SQLOP:
            assert not db.out_numpy("sql_op", n=hb.cols.n_spans).any()
    for rb, ab, acc in got:
        np.testing.assert_array_equal(rb, want_res)
        np.testing.assert_array_equal(ab, want_sets)
        assert acc == accepted


@pytest.mark.gpu
def test_gpu_size_sqlop_beside_forked_url_stage():
    # From 1M spans on, SAMPLE | TEMPLATE by trace id plans the URLs on a second
    # stream, and the refs form joins it early when the spans pass is fused into
    # url_copy_kernel.  With a SQL bit the spans pass is a kernel of its own that
    # reads the refs after the full join: on a batch where no query matches (the
    # URL paths stand in as queries) the counters must equal the fused path's.
    import torch
    from odigos_amd.batch import DeviceBatch, Engine, Generator
    S = native
    g = Generator("fused", seed=0x0D160951, n_spans=(1 << 20) + 4099)
    n, R, A = g.cols.n_spans, g.cols.n_resources, g.cols.n_attrsets
    cfg = {"odigossampling": c3_sampling_config(), "odigosurltemplate": {}, SECTION: {},
           "odigostrafficmetrics": {"res_attributes_keys": ["service.name", "k8s.namespace.name"]}}
    eng = Engine(cfg)
    eng.reserve(n, g.cols.arena_bytes)
    base = S.STAGE_SAMPLE | S.STAGE_TEMPLATE | S.STAGE_TEMPLATE_REFS | S.STAGE_SIZE
    got = []
    for mask in (base, base | S.STAGE_SQLOP):
        db = DeviceBatch(g.cols)
        flags = torch.full((n + 16,), S.DB_HAS_QUERY, dtype=torch.uint8, device="cuda")
        db.cols.db_flags, db.cols.db_query = flags.data_ptr(), db.t["path"].data_ptr()
        db.o["sql_op"].fill_(0xEE)
        eng.process_device(db, mask, S.GROUP_TRACE_ID, seed=0x5EED)
        torch.cuda.synchronize()
        assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
        if mask & S.STAGE_SQLOP:
            assert not db.out_numpy("sql_op", n=n).any()
        got.append((db.out_numpy("res_bytes", np.uint64, n=R), db.out_numpy("attrset_bytes", np.int64, n=A),
                    int(db.out_numpy("accepted_spans", np.int64)[0]), db.out_numpy("keep", n=n)))
    assert 0 < got[0][2] < n
    for x, y in zip(got[0], got[1]):
        np.testing.assert_array_equal(x, y)


# ---- drop-in processors ----------------------------------------------------

def _dropin_tree():
    sp = host.span
    return host.traces(
        host.resource_spans({"service.name": "a", "telemetry.sdk.language": "go"}, [
            sp(name="q1", attributes={"x": 1, ref.QUERY_KEY: "  select * from t"}),
            sp(name="", attributes={ref.QUERY_KEY: "DROP\ttable t"}),
            sp(name="q3", attributes={ref.QUERY_KEY: "select\r\n1"}),
            sp(name="q4", attributes={ref.QUERY_KEY: "update t", ref.OPNAME_KEY: False}),
            sp(name="q5", attributes={ref.QUERY_KEY: chr(0x3000) + chr(0x85) + "delete from t ", "y": "z"}),
            sp(name="q6", attributes={ref.QUERY_KEY: chr(0x17F) + "elect 1"}),
            sp(name="q7"),
            sp(name="GET", kind=2, attributes={"http.request.method": "GET", "url.path": "/user/1234",
                                               ref.QUERY_KEY: "insert into t values (1)"}),
        ]),
        host.resource_spans({"service.name": "b"}, [sp(name="nolang", attributes={ref.QUERY_KEY: "select 1"})]),
        host.resource_spans({"service.name": "c", "telemetry.sdk.language": "python"},
                            [sp(name="py", attributes={ref.QUERY_KEY: "select 1"})]),
    )


def _roundtrip(td):
    """The tree as the host layer writes an unchanged one."""
    L = native.lib()
    return host.loads(native.take_bytes(L.osehost_roundtrip(host.dumps(td).encode())).decode("ascii"))


@pytest.mark.gpu
def test_gpu_dropin_processor():
    td = _dropin_tree()
    for cfg in ({}, {"exclude": {"language": ["python"]}}, {"exclude": {"language": []}}):
        got = host.Processor(SECTION, cfg).consume(td)
        want = ref.process_traces(cfg, _roundtrip(td))
        assert got == want, cfg
    # the exclude-language quirk: a resource without telemetry.sdk.language is skipped too
    got = host.Processor(SECTION, {"exclude": {"language": ["python"]}}).consume(td)
    names = [[s["name"] for s in rs["scopeSpans"][0]["spans"]] for rs in got["resourceSpans"]]
    assert names[1] == ["nolang"] and names[2] == ["py"] and names[0][0] == "q1 SELECT" and names[0][1] == " DROP"
    sp0 = got["resourceSpans"][0]["scopeSpans"][0]["spans"][0]
    assert sp0["attributes"][-1] == {"key": ref.OPNAME_KEY, "value": {"stringValue": "SELECT"}}   # appended last


@pytest.mark.gpu
def test_gpu_dropin_pipeline_four_sections():
    td = _size_tree(random.Random(9))
    seed = 0x0D31
    proc, hb, cfg, tree, want_res, want_sets, accepted = _size_expectation(td, seed)
    p = host.Processor("pipeline", cfg)
    p.configure(seed, native.GROUP_TRACE_ID)
    got = p.consume(td)
    assert got == tree
    m = p.metrics()
    assert int(m["otelcol_odigos_accepted_spans"]) == accepted
    assert sum(int(x["value"]) for x in m["otelcol_odigos_trace_data_size"]) == int(want_sets.sum())
    # the URL stage's attribute comes before this stage's; the name carries both
    for rs in got["resourceSpans"]:
        for ss in rs["scopeSpans"]:
            for sp in ss["spans"]:
                if sp["name"].startswith("GET /user/{id} "):
                    assert sp["attributes"][-1]["key"] == ref.OPNAME_KEY
                    return
    pytest.fail("no span was both templated and given an operation name")


# ---- refusals, hipGraph ----------------------------------------------------

@pytest.mark.gpu
def test_gpu_refusals():
    import torch
    from odigos_amd.batch import DeviceBatch, Engine, OtlpBatch
    sb = SqlBatch([b"select 1", b"x"], [1, 1], [0, 0], None)
    plain = Engine({"odigosurltemplate": {}})
    db = DeviceBatch(sb.cols)
    with pytest.raises(native.OseError) as e:
        plain.process_device(db, native.STAGE_SQLOP)
    assert e.value.code == native.OSE_EINVAL and "not configured" in str(e.value)
    assert not plain.info().stages & native.STAGE_SQLOP
    eng = Engine({SECTION: {}, "odigostrafficmetrics": {}, "odigosurltemplate": {}})
    assert eng.info().stages & native.STAGE_SQLOP
    db.cols.db_flags = None
    with pytest.raises(native.OseError) as e:
        eng.process_device(db, native.STAGE_SQLOP)
    assert e.value.code == native.OSE_EINVAL and "db_flags" in str(e.value)
    db = DeviceBatch(sb.cols)
    with pytest.raises(native.OseError) as e:
        eng.process_device(db, native.STAGE_SQLOP | native.STAGE_APPLY_SQLOP)
    assert e.value.code == native.OSE_EINVAL
    # the OTLP path does not carry the stage
    td = host.traces(host.resource_spans({"service.name": "a"}, [host.span(name="s", trace_id="%032x" % 1, span_id="%016x" % 1)]))
    ob = OtlpBatch(eng, gg.marshal_traces(td))
    assert not ob.cols.db_flags and not ob.cols.db_query and not ob.cols.res_sql_ok
    for bit in (native.STAGE_SQLOP, native.STAGE_APPLY_SQLOP):
        with pytest.raises(native.OseError) as e:
            ob.encode(native.STAGE_TEMPLATE | bit)
        assert e.value.code == native.OSE_ENOTSUP
        h = C.c_void_p()
        assert native.lib().ose_otlp_pipeline_create(eng.h, None, native.STAGE_TEMPLATE | bit, 0, C.byref(h)) == native.OSE_ENOTSUP
    ob.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_graph_capture_template_sqlop_size():
    import torch
    from odigos_amd.batch import DeviceBatch, Engine
    td = _size_tree(random.Random(11))
    proc, hb, cfg, tree, want_res, want_sets, accepted = _size_expectation(td, 1, with_sampling=False)
    eng = Engine(cfg)
    st = native.STAGE_TEMPLATE | native.STAGE_SQLOP | native.STAGE_SIZE
    eager, cap = DeviceBatch(hb.cols), DeviceBatch(hb.cols)
    eng.reserve(hb.cols.n_spans, hb.cols.arena_bytes)
    eng.process_device(eager, st, native.GROUP_BATCH, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            eng.process_device(cap, st, native.GROUP_BATCH, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for name in ("attrset_bytes", "accepted_spans", "res_bytes", "sql_op"):
        cap.o[name].zero_()
    graph.replay()
    torch.cuda.synchronize()
    n, A, R = hb.cols.n_spans, hb.cols.n_attrsets, hb.cols.n_resources
    assert eager.out_numpy("sql_op", n=n).any()
    for name, dt, k in (("sql_op", np.uint8, n), ("url_out", np.uint8, n), ("tmpl", np.uint64, n),
                        ("attrset_bytes", np.int64, A), ("res_bytes", np.uint64, R), ("accepted_spans", np.int64, 1)):
        np.testing.assert_array_equal(cap.out_numpy(name, dt, n=k), eager.out_numpy(name, dt, n=k))
    np.testing.assert_array_equal(eager.out_numpy("res_bytes", np.uint64, n=R), want_res)
