"""odigosconditionalattributes on the OTLP path (engine option otlp_condattr).

CPU: the host encoder applying the stage's puts (osehost_otlp_encode_condattr)
byte for byte against the restatement (tests/condattr_ref.py) marshalled as
pdata does (tests/otlp_gogo.py) — the golden cases, the shipped profile,
seeded adversarial trees in both encodings, hand-laid edge spans, the router —
the restatement's put order against Go's contract, the refusals of the seam and
the ctypes mirrors against the header.

GPU: the decoded columns (ose_otlp_condattr_columns) against the columniser's
at 0 to 70,000 spans in both encodings under every decode mode, over a case
list of every AnyValue kind, repeated, look-alike and zero-length keys, event
and link attributes, the span kernel's own host-pass spans and a value that
ends the message; a redone decode and a regrown arena; the node collector's
pipeline (decode, ose_condattr_process_device, SIZE, ose_otlp_encode_condattr)
on an engine with the condattr and traffic-metrics sections only, byte for
byte, with the data_size counters, through the GPU and the host encoder, with
and without a router; the option and the refusals.

The expected bytes: the puts of condattr_ref.process_traces applied to the
input tree in target order (the first KeyValue with the key replaced where it
stands, its value becoming a string; else a new KeyValue after the span's last
attribute), then otlp_gogo.marshal_traces.
"""
import copy
import ctypes as C
import random
import re
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import host, native
from tests import condattr_ref as ref
from tests import otlp_gogo as gg
from tests.test_condattr import KATS, adv_config, adv_tree, kat_cases, kat_tree, profile_config
from tests.test_otlp import to_pb

CSRC = Path(__file__).parent.parent / "odigos_amd" / "csrc"
STREAMS = [{"name": "p0", "sources": [{"namespace": "ns0", "kind": "Deployment", "name": "d0"}],
            "destinations": [{"destinationname": "x", "configuredsignals": ["TRACES"]}]},
           {"name": "p1", "sources": [{"namespace": "ns1", "kind": "Deployment", "name": "d1"},
                                      {"namespace": "ns0", "kind": "Deployment", "name": "d0"}],
            "destinations": [{"destinationname": "y", "configuredsignals": ["TRACES", "LOGS"]}]}]


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


def spans_of(td):
    return [sp for rs in td["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]


def restated_puts(cfg, td):
    """(target names, per span {target: value}) of the restatement."""
    detail = []
    ref.process_traces(cfg, td, detail)
    return ref.targets(cfg), [p for p, _ in detail]


def apply_puts(td, targets, puts):
    """The tree after every span's puts, in target order."""
    out = copy.deepcopy(td)
    for sp, p in zip(spans_of(out), puts):
        attrs = sp.setdefault("attributes", [])
        for t in targets:
            if t in p:
                ref.put_str(attrs, t, p[t])
    return out


def expected(td, targets, puts, streams=None, pipelines=None):
    t = apply_puts(td, targets, puts)
    if streams is None:
        return [("", gg.marshal_traces(t), len(t["resourceSpans"]))]
    return [(p, gg.marshal_traces(x), len(x["resourceSpans"])) for p, x in gg.split_by_pipeline(t, streams, pipelines)]


def put_columns(targets, puts, mix=True):
    """src [T*n], val [T*n, 2], arena, strings: the values of even (target +
    span) live in the arena, the others in the string table (mix), both behind
    a few bytes that belong to no value."""
    n, T = len(puts), len(targets)
    src = np.zeros(max(1, T * n), dtype=np.uint8)
    val = np.zeros((max(1, T * n), 2), dtype=np.uint32)
    bufs = {native.CA_ARENA: bytearray(b"\xa5" * 3), native.CA_CONFIG: bytearray(b"\x5a" * 5)}
    for u, t in enumerate(targets):
        for i, p in enumerate(puts):
            if t not in p:
                continue
            s = native.CA_CONFIG if mix and (u + i) % 2 else native.CA_ARENA
            b = _b(p[t])
            src[u * n + i] = s
            val[u * n + i] = (len(bufs[s]), len(b))
            bufs[s] += b
    return src, val, bytes(bufs[native.CA_ARENA]), bytes(bufs[native.CA_CONFIG])


def seam_rc(pb, n, src, val, targets, arena, strings, router=None, threads=1, arena_bytes=None, string_bytes=None):
    L = native.lib()
    names = b"".join(_b(t) for t in targets)
    lens = np.array([len(_b(t)) for t in targets] + [0], dtype=np.uint32)
    a = np.frombuffer(arena + bytes(16), dtype=np.uint8).copy()
    s = np.frombuffer(strings + bytes(16), dtype=np.uint8).copy()
    nm = np.frombuffer(names + bytes(16), dtype=np.uint8).copy()
    h = C.c_void_p()
    rc = L.osehost_otlp_encode_condattr(pb, len(pb), n, None if src is None else src.ctypes.data,
                                        None if val is None else val.ctypes.data, len(targets), a.ctypes.data,
                                        len(arena) if arena_bytes is None else arena_bytes, s.ctypes.data,
                                        len(strings) if string_bytes is None else string_bytes, nm.ctypes.data,
                                        lens.ctypes.data, router.h if router is not None else None, threads, C.byref(h))
    return rc, h


def seam(pb, targets, puts, router=None, threads=1, mix=True):
    from odigos_amd.batch import take_otlp_out
    src, val, arena, strings = put_columns(targets, puts, mix)
    rc, h = seam_rc(pb, len(puts), src, val, targets, arena, strings, router, threads)
    native.check(rc)
    return take_otlp_out(native.lib(), h)


def check_tree(cfg, td, encodings=(gg.marshal_traces, to_pb), threads=(1,)):
    targets, puts = restated_puts(cfg, td)
    want = expected(td, targets, puts)
    for enc in encodings:
        pb = enc(td)
        for t in threads:
            got = seam(pb, targets, puts, threads=t)
            assert got == want, (enc.__name__, t)
    return want


# ---------------------------------------------------------------------------
# CPU: the host encoder against the restatement

def test_seam_golden_cases():
    for cfg, c in kat_cases():
        check_tree(cfg, kat_tree(c))
    # the README's cases as one message of several resources
    cfg = KATS["readme_examples"]["config"]
    td = {"resourceSpans": [kat_tree(c)["resourceSpans"][0] for c in KATS["readme_examples"]["cases"]]}
    check_tree(cfg, td)


def profile_tree(rng, n_spans=600, n_scopes=40):
    cfg = profile_config()
    names = list(cfg["rules"][0]["new_attribute_value_configurations"])
    scopes = []
    for s in range(n_scopes):
        nm = rng.choice(names) if s % 4 else rng.choice(["", "unknown.library", names[s % len(names)] + "x", names[3][:-1]])
        scopes.append({"scope": {"name": nm}, "spans": []})
    for i in range(n_spans):
        at = {}
        if rng.random() < 0.5:
            at[rng.choice(["http.request.method", "http.method"])] = rng.choice(["GET", "POST", 7])
        if rng.random() < 0.1:
            at["odigos.category"] = rng.choice(["mine", 3])
        rng.choice(scopes)["spans"].append(host.span(name="s%d" % i, kind=1 + i % 5, attributes=at, trace_id="%032x" % (i + 1),
                                                     span_id="%016x" % (i + 1)))
    h = n_scopes // 2
    return cfg, host.traces(host.resource_spans({"service.name": "a", "k8s.namespace.name": "ns0", "k8s.deployment.name": "d0"},
                                                scopes=scopes[:h]),
                            host.resource_spans({"service.name": "b"}, scopes=scopes[h:]))


def test_seam_shipped_profile():
    cfg, td = profile_tree(random.Random(0xCA7E))
    want = check_tree(cfg, td, threads=(1, 3))
    assert want[0][1].count(b"odigos.category") >= 600


def test_seam_adversarial_trees_both_encodings():
    cfg = adv_config()
    td = adv_tree(0x07C4, 2000, 9, 40)
    targets, puts = restated_puts(cfg, td)
    assert len(targets) == 17 and "" in targets
    # the ground: in-place replacements of non-string values, appends, spans without a put
    replaced = sum(1 for sp, p in zip(spans_of(td), puts) for t in p
                   if (kv := ref._get(sp["attributes"], t)) is not None and "stringValue" not in kv["value"])
    assert replaced >= 50 and sum(1 for p in puts if len(p) >= 4) >= 50
    check_tree(cfg, td, threads=(1, 4))


def test_seam_routes_like_the_plain_encoder():
    from odigos_amd.batch import Router
    from tests.test_otlp_sqlop import _seam as plain_seam
    cfg = adv_config()
    td = adv_tree(0x20D7, 300, 6, 14)
    for r, rs in enumerate(td["resourceSpans"]):
        if r % 3 != 2:
            rs["resource"]["attributes"] += host.attrs({"k8s.deployment.name": "d%d" % (r % 3)})
    targets, puts = restated_puts(cfg, td)
    router = Router({"datastreams": STREAMS})
    assert router.pipelines == ["p0", "p1"]
    for enc in (gg.marshal_traces, to_pb):
        pb = enc(td)
        got = seam(pb, targets, puts, router=router, threads=2)
        assert got == expected(td, targets, puts, STREAMS, router.pipelines)
        # resource for resource the routing of the plain encoder
        plain = plain_seam(pb, router=router)
        assert [(p, n) for p, _, n in got] == [(p, n) for p, _, n in plain]
        assert [n for _, _, n in got].count(0) < 3
    router.close()


def one_span(sp_bytes: bytes) -> bytes:
    """A TracesData of one resource, one scope and the given Span bytes."""
    return gg._len(1, gg._len(1, b"") + gg._len(2, gg._len(1, b"") + gg._len(2, sp_bytes)))


def tree_of(*spans):
    return host.traces(host.resource_spans({}, list(spans)))


def check_puts(td, targets, puts, pbs=None):
    want = expected(td, targets, puts)
    for pb in (pbs if pbs is not None else (gg.marshal_traces(td), to_pb(td))):
        for mix in (False, True):
            assert seam(pb, targets, puts, mix=mix) == want
    return want[0][1]


def test_edge_replaced_in_place_and_typed():
    m = {"kvlistValue": {"values": [{"key": "a", "value": {"stringValue": "b"}}]}}
    sp = host.span(name="s", attributes={"a": "x", "t": 7, "b": "y", "u": m, "c": 2.5})
    sp["attributes"].insert(2, {"key": "e", "value": {}})   # an empty AnyValue
    td = tree_of(sp)
    out = check_puts(td, ["t", "u", "e", "new"], [{"t": "T", "u": "U", "e": "E", "new": "N"}])
    after = spans_of(apply_puts(td, ["t", "u", "e", "new"], [{"t": "T", "u": "U", "e": "E", "new": "N"}]))[0]["attributes"]
    assert [kv["key"] for kv in after] == ["a", "t", "e", "b", "u", "c", "new"]
    assert all(after[k]["value"] == {"stringValue": v} for k, v in ((1, "T"), (2, "E"), (4, "U"), (6, "N")))
    assert gg._len(9, gg.key_value({"key": "t", "value": {"stringValue": "T"}})) in out


def test_edge_repeated_key_only_the_first():
    sp = host.span(name="s", attributes={"a": 1})
    sp["attributes"] += [{"key": "t", "value": {"intValue": "1"}}, {"key": "b", "value": {"stringValue": ""}},
                         {"key": "t", "value": {"stringValue": "second"}}]
    out = check_puts(tree_of(sp), ["t"], [{"t": "first"}])
    assert out.count(b"second") == 1 and out.index(b"first") < out.index(b"second")


def test_edge_no_attributes_later_fields():
    ev = [{"timeUnixNano": "5", "name": "ev", "attributes": host.attrs({"t": "in-event"})}]
    lk = [{"traceId": "0" * 31 + "1", "spanId": "0" * 15 + "2", "attributes": host.attrs({"t": "in-link"})}]
    sp = host.span(name="s", kind=2, status=2, events=ev, links=lk)
    sp["status"]["message"] = "boom"
    td = tree_of(sp, host.span(name="dropped", droppedAttributesCount=3))
    out = check_puts(td, ["t", "u"], [{"t": "T", "u": ""}, {"u": "U"}])
    # the appended KeyValues stand before field 10 and above; the event's and the link's "t" are not the span's
    new_t = gg._len(9, gg.key_value({"key": "t", "value": {"stringValue": "T"}}))
    assert out.index(new_t) < out.index(b"in-event") < out.index(b"in-link") < out.index(b"boom")
    new_u = gg._len(9, gg.key_value({"key": "u", "value": {"stringValue": "U"}}))
    assert out[out.index(new_u) + len(new_u):][:2] == gg._uvar(10, 3)


def test_edge_no_field_after_the_attributes():
    # hand-laid: a Span of attributes alone (no status, no ids), and an empty Span
    at = host.attrs({"a": "x", "t": 1})
    td = tree_of({"attributes": at}, {})
    pb = one_span(gg._attrs(9, at))
    pb2 =gg._len(1, gg._len(1, b"") + gg._len(2, gg._len(1, b"") + gg._len(2, gg._attrs(9, at)) + gg._len(2, b"")))
    check_puts(td, ["t", "n"], [{"t": "T", "n": "N"}, {"n": "only"}], pbs=(pb2,))
    check_puts(tree_of({"attributes": at}), ["t", "n"], [{"t": "T", "n": "N"}], pbs=(pb,))


def test_edge_empty_value_and_zero_length_key():
    sp = host.span(name="s", attributes={"a": "x"})
    sp["attributes"].append({"key": "", "value": {"intValue": "9"}})
    td = tree_of(sp, host.span(name="t"))
    out = check_puts(td, ["e", ""], [{"e": "", "": "nameless"}, {"": ""}])
    # pdata omits an empty key and writes the empty string oneof
    assert gg._len(9, gg._len(2, gg._len(1, b"nameless"))) in out
    assert gg._len(9, gg._len(2, gg._len(1, b""))) in out
    assert gg._len(9, gg._len(1, b"e") + gg._len(2, gg._len(1, b""))) in out


def test_edge_varint_growth():
    spans, puts = [], []
    for ln in (126, 127, 128, 129):   # the value's own length
        spans.append(host.span(name="v%d" % ln, attributes={"t": "old"}))
        puts.append({"t": "V" * ln})
    kv = lambda n: len(gg._len(9, gg.key_value({"key": "t", "value": {"stringValue": "V" * n}})))   # noqa: E731
    for edge in (127, 16383):   # the KeyValue's framed length: ..., edge, edge + 1, ...
        n0 = next(n for n in range(1, 20000) if len(gg.key_value({"key": "t", "value": {"stringValue": "V" * n}})) == edge)
        for n in (n0 - 1, n0, n0 + 1, n0 + 2):
            spans.append(host.span(name="k", attributes={"a": 1}))
            puts.append({"t": "V" * n})
        assert kv(n0 + 1) - kv(n0) == 2
    for edge in (127, 16383):   # the span's length
        base = len(gg.span(host.span(name="", attributes={"t": 5})))
        for ln in range(edge - base - 12, edge - base + 3):
            spans.append(host.span(name="n" * ln, attributes={"t": 5}))
            puts.append({"t": "grown-by-some"})
    td = tree_of(*spans)
    grown = [(len(gg.span(a)), len(gg.span(b))) for a, b in zip(spans, spans_of(apply_puts(td, ["t"], puts)))]
    assert any(x <= 127 < y for x, y in grown) and any(x <= 16383 < y for x, y in grown)
    check_puts(td, ["t"], puts)


def test_restatement_order_against_go():
    """Where Go fixes the order: the attribute map equals condattr_ref's, and a
    replaced attribute keeps its index; appended ones are in target order."""
    for cfg, td in ((adv_config(), adv_tree(0x60, 500, 4, 12)), profile_tree(random.Random(5), 200, 12)):
        targets, puts = restated_puts(cfg, td)
        mine, go = apply_puts(td, targets, puts), ref.process_traces(cfg, td)
        assert ref.canon(mine, td) == ref.canon(go, td)
        for a, b, c in zip(spans_of(td), spans_of(mine), spans_of(go)):
            n0 = len(a["attributes"])
            assert [kv["key"] for kv in b["attributes"][:n0]] == [kv["key"] for kv in a["attributes"]]
            assert b["attributes"][:n0] == c["attributes"][:n0]
            added = [kv["key"] for kv in b["attributes"][n0:]]
            assert added == [t for t in targets if t in added] and len(set(added)) == len(added)


def test_seam_refusals():
    from odigos_amd.batch import take_otlp_out
    L = native.lib()
    td = tree_of(host.span(name="a", attributes={"t": 1}), host.span(name="b"))
    pb = gg.marshal_traces(td)
    targets, puts = ["t"], [{"t": "abc"}, {"t": "defg"}]
    src, val, arena, strings = put_columns(targets, puts, mix=False)
    ok = expected(td, targets, puts)

    def run(**kw):
        a = dict(pb=pb, n=2, src=src, val=val, targets=targets, arena=arena, strings=strings)
        a.update(kw)
        rc, h = seam_rc(**a)
        return rc, (take_otlp_out(L, h) if rc == 0 else native.last_error())
    assert run() == (0, ok)
    assert run(src=None)[0] == native.OSE_EINVAL and run(val=None)[0] == native.OSE_EINVAL
    assert run(n=3)[0] == native.OSE_EINVAL
    bad = src.copy()
    bad[1] = 3
    rc, msg = run(src=bad)
    assert rc == native.OSE_EINVAL and "OSE_CA_CONFIG" in msg
    # a ref that ends on the arena's last byte is fine, one byte further is not
    assert int(val[1][0] + val[1][1]) == len(arena)
    rc, msg = run(arena_bytes=len(arena) - 1)
    assert rc == native.OSE_ERANGE and "arena_bytes" in msg
    cfgsrc = src.copy()
    cfgsrc[:] = native.CA_CONFIG
    assert run(src=cfgsrc, strings=arena) == (0, ok)
    rc, msg = run(src=cfgsrc, strings=arena, string_bytes=len(arena) - 1)
    assert rc == native.OSE_ERANGE and "string table" in msg
    far = val.copy()
    far[0] = (0xFFFFFFFF, 2)   # off + len wraps 32 bits
    assert run(val=far)[0] == native.OSE_ERANGE
    # a KEEP entry's val is not read
    keep = src.copy()
    keep[0] = native.CA_KEEP
    assert run(src=keep, val=far) == (0, expected(td, targets, [{}, puts[1]]))
    assert L.osehost_otlp_encode_condattr(b"\x0a\x05", 2, 0, None, None, 0, None, 0, None, 0, None, None, None, 1,
                                          C.byref(C.c_void_p())) == native.OSE_EINVAL


def enc_ca_targets() -> int:
    """kEncCaTargets, the GPU encoder's bound on the targets, from the source."""
    m = re.search(r"constexpr\s+uint32_t\s+kEncCaTargets\s*=\s*(\d+)\s*;", (CSRC / "kernels.hpp").read_text())
    assert m, "kEncCaTargets is not where it was"
    return int(m.group(1))


def many_targets(T):
    """T targets t00.., and spans that replace, append and keep across all of them."""
    targets = ["t%02d" % k for k in range(T)]
    spans = [host.span(name="all"), host.span(name="some", attributes={targets[-1]: 1, "x": "y", targets[0]: True}),
             host.span(name="none", attributes={targets[T // 2]: "kept"})]
    puts = [{t: "v-" + t for t in targets}, {t: "w" * (k % 5) for k, t in enumerate(targets) if k % 3 != 1}, {}]
    return tree_of(*spans), targets, puts


def test_edge_target_counts_at_the_gpu_bound():
    T = enc_ca_targets()
    assert 8 <= T < 32
    for t in (T, T + 1):
        td, targets, puts = many_targets(t)
        check_puts(td, targets, puts)


def test_struct_mirrors_and_symbols():
    from tests.test_condattr import _header_struct
    hdr = (Path(__file__).parent.parent / "include" / "odigos_amd.h").read_text()
    assert "#define OSE_ABI_VERSION 5" in hdr
    for cname, mirror in (("ose_condattr_columns", native.CondAttrColumns), ("ose_condattr_outputs", native.CondAttrOutputs)):
        fields = _header_struct(cname)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_]
        off = 0
        for (ctype, f), (_, py) in zip(fields, mirror._fields_):
            size = 8 if "*" in ctype or "uint64_t" in ctype else 4
            off = (off + size - 1) // size * size
            assert getattr(mirror, f).offset == off and C.sizeof(py) == size, (cname, f)
            off += size
    # no existing struct changed size
    assert (C.sizeof(native.Columns), C.sizeof(native.Outputs), C.sizeof(native.CondAttrColumns),
            C.sizeof(native.CondAttrOutputs)) == (264, 128, 120, 40)
    L = native.lib()
    for sym in ("ose_otlp_condattr_columns", "ose_otlp_condattr_download", "ose_otlp_encode_condattr"):
        assert sym in native.exported_symbols() and hasattr(L, sym)
    assert hasattr(L, "osehost_otlp_encode_condattr")
    assert L.ose_otlp_condattr_columns.restype == C.POINTER(native.CondAttrColumns)
    assert re.search(r'"otlp_condattr"', hdr)


# ---------------------------------------------------------------------------
# GPU

SECTION, SCOPE = ref.SECTION, ref.OTTL_SCOPE_NAME_KEY
TRAFFIC = {"res_attributes_keys": ["service.name", "k8s.namespace.name"]}
MODES = (None, "otlp_host_scopes", "otlp_host_resources", "otlp_gpu_chain")


def node_engine(cfg, option=True):
    """The node collector's engine: odigosconditionalattributes and odigostrafficmetrics only."""
    from odigos_amd.batch import Engine
    eng = Engine({SECTION: cfg, "odigostrafficmetrics": TRAFFIC})
    if option:
        eng.set_option("otlp_condattr", 1)
    return eng


# keys rk, ff, tg, "", tg2 (targets tg, "", tg2)
DEC_CFG = {"global_default": "dflt", "rules": [
    {"field_to_check": "rk", "new_attribute_value_configurations": {
        "v": [{"new_attribute": "tg", "from_field": "ff"}, {"new_attribute": "", "value": "nameless"}]}},
    {"field_to_check": SCOPE, "new_attribute_value_configurations": {"lib": [{"new_attribute": "tg2", "value": "x"}]}}]}
_KV = lambda k, v: {"key": k, "value": host.attr_value(v)}   # noqa: E731
_NESTED = {"kvlistValue": {"values": [{"key": "a", "value": {"stringValue": "b"}}]}}
_ARRAY = {"arrayValue": {"values": [{"stringValue": "a"}, {"intValue": "2"}]}}
_BYTES = {"bytesValue": "AAEC"}
# (attributes, other span fields, a value of one of the keys needs AsString)
CASES = [
    ([_KV("rk", "v"), _KV("ff", "from")], {}, False),
    ([_KV("rk", 7)], {}, True), ([_KV("rk", 2.5)], {}, True), ([_KV("rk", True)], {}, True),
    ([_KV("rk", _BYTES)], {}, True), ([_KV("rk", _ARRAY)], {}, True), ([_KV("rk", _NESTED)], {}, True),
    ([{"key": "rk", "value": {}}], {}, True),
    ([_KV("ff", ""), _KV("tg", "")], {}, False),                                  # string values of length 0
    ([_KV("rk", "first"), _KV("rk", 5)], {}, False), ([_KV("rk", 5), _KV("rk", "second")], {}, True),
    ([_KV("r", "n"), _KV("rkx", "n"), _KV("xk", "n"), _KV("rx", "n"), _KV("tg3", "n"), _KV("t", "n")], {}, False),   # look-alikes
    ([_KV("other", 1)], {"events": [{"timeUnixNano": "1", "name": "e", "attributes": [_KV("rk", 9), _KV("tg", "ev")]}],
                         "links": [{"traceId": "0" * 31 + "1", "spanId": "0" * 15 + "1", "attributes": [_KV("ff", 3)]}]}, False),
    ([_KV("", "empty-key")], {}, False), ([_KV("", 4)], {}, True), ([_KV("a", "b"), {"key": "", "value": {"stringValue": ""}}], {}, False),
    ([_KV("url.full", "https://h/a/b?q=1"), _KV("tg", "t")], {}, False),           # the span kernel's own host pass
    ([_KV("http.route", 5), _KV("rk", "v")], {}, False), ([_KV("http.route", 5), _KV("ff", 6)], {}, True),
    ([], {}, False),
    ([_KV("tg", "x" * 127), _KV("tg2", "y" * 128), _KV("ff", "z" * 300)], {}, False),
    ([_KV("x%d" % k, "pad") for k in range(12)] + [_KV("tg2", 1.5)], {}, True),
]
TAIL_ATTRS = [_KV("a", "b"), _KV("ff", "ends-the-message")]


def _case_span(c, i):
    at, extra, _ = CASES[c]
    sp = host.span(name="s%d" % (i % 10), kind=1 + i % 5, trace_id="%032x" % (i + 1), span_id="%016x" % (i + 1),
                   start=1739000000000000000 + i, end=1739000001000000000)
    sp["attributes"] = copy.deepcopy(at)
    sp.update(copy.deepcopy(extra))
    return sp


_TREES = {}


def dec_tree(n):
    """(tree, the case of every span in tree order): n case spans over 3 resources and 7
    scopes (one empty, one unnamed, one with typed attributes), then the
    hand-laid tail: a resource whose ScopeSpans has no scope field and whose
    one span ends the message with a value of a key."""
    if n in _TREES:
        return _TREES[n]
    scopes = [{"scope": {"name": "lib", "attributes": [_KV("rk", True), _KV("ff", 2.5), _KV("", "e"), _KV("tg", _NESTED)]}, "spans": []},
              {"scope": {"name": "", "attributes": []}, "spans": []},
              {"scope": {"name": "lib", "version": "1.2"}, "spans": []},
              {"scope": {"name": "other", "attributes": [_KV("tg2", "s")]}, "spans": []},
              {"scope": {"name": "empty-scope-spans"}, "spans": []},
              {"scope": {"name": "lib", "attributes": [_KV("rk", True), _KV("ff", 2.5), _KV("", "e"), _KV("tg", _NESTED)]}, "spans": []},
              {"scope": {"name": "x" * 200, "attributes": [_KV("rk", "v")]}, "spans": []}]
    fill = [0, 1, 2, 3, 5, 6]
    case_ids = []
    per = [[] for _ in scopes]
    for i in range(n):
        per[fill[(i // 5) % len(fill)]].append(i)
    for s, idx in enumerate(per):
        for i in idx:
            scopes[s]["spans"].append(_case_span(i % len(CASES), i))
            case_ids.append(i % len(CASES))
    td = host.traces(
        {"resource": {"attributes": [_KV("service.name", "a"), _KV("rk", 5), _KV("tg", "res"), _KV("rk", "second")]},
         "scopeSpans": scopes[:3]},
        {"resource": {"attributes": []}, "scopeSpans": scopes[3:5]},
        {"resource": {"attributes": [_KV("service.name", "a"), _KV("", _ARRAY)]}, "scopeSpans": scopes[5:]})
    _TREES[n] = (td, case_ids)
    return _TREES[n]


def tail_tree_and_bytes():
    sp = {"traceId": "ab" * 16, "spanId": "cd" * 8, "attributes": TAIL_ATTRS}
    rs = {"resource": {"attributes": [_KV("tg2", "tail-res")]}, "scopeSpans": [{"spans": [sp]}]}
    raw = gg._len(1, bytes.fromhex("ab" * 16)) + gg._len(2, bytes.fromhex("cd" * 8)) + gg._attrs(9, TAIL_ATTRS)
    b = gg._len(1, gg._len(1, gg._attrs(1, rs["resource"]["attributes"])) + gg._len(2, gg._len(2, raw)))
    assert b.endswith(b"ends-the-message")
    return rs, b


_MSGS = {}


def dec_message(n, enc):
    """(tree, message bytes, the case spans' cases) of n spans in all, built once
    per size and encoding: n - 1 case spans and the tail's one; n == 0: the
    resources and scopes without any span, and no tail."""
    key = (n, enc.__name__)
    if key not in _MSGS:
        td, case_ids = dec_tree(max(n - 1, 0))
        if n == 0:
            _MSGS[key] = (td, enc(td), case_ids)
        else:
            rs, tail = tail_tree_and_bytes()
            _MSGS[key] = ({"resourceSpans": td["resourceSpans"] + [rs]}, enc(td) + tail, case_ids)
        assert len(spans_of(_MSGS[key][0])) == n
    return _MSGS[key]


_WANT = {}


def want_columns(cfg, n, td):
    """The columniser's condattr columns as {name: list}, strings as bytes."""
    key = (id(cfg), n)
    if key in _WANT:
        return _WANT[key]
    p = host.Processor(SECTION, cfg)
    hb = p.columnarize(td)
    c = hb.condattr_cols
    K = len(ref.keys(cfg))
    arr = lambda ptr, dt, cnt: np.ctypeslib.as_array((dt * max(1, cnt)).from_address(ptr))[:cnt].copy()   # noqa: E731
    arena = bytes((C.c_uint8 * c.arena_bytes).from_address(c.arena)) if c.arena_bytes else b""
    out = {"dims": (c.n_spans, c.n_scopes, c.n_resources)}
    for name, rows in (("span", c.n_spans), ("scope", c.n_scopes), ("res", c.n_resources)):
        has = arr(getattr(c, name + "_has"), C.c_uint8, K * rows)
        val = arr(getattr(c, name + "_val"), C.c_uint32, 2 * K * rows).reshape(-1, 2)
        out[name] = (has, {int(x): arena[val[x][0]:val[x][0] + val[x][1]] for x in np.nonzero(has)[0]})
    out["kv"] = arr(c.span_kv_size, C.c_uint32, K * c.n_spans)
    names = arr(c.scope_name, C.c_uint32, 2 * c.n_scopes).reshape(-1, 2)
    out["scope_name"] = [arena[o:o + ln] for o, ln in names]
    out["span_scope"] = arr(c.scope, C.c_uint32, c.n_spans)
    out["scope_resource"] = arr(c.scope_resource, C.c_uint32, c.n_scopes)
    p.close()
    _WANT[key] = out
    return out


def compare_columns(cfg, ob, want):
    c = ob.condattr_cols
    assert c is not None
    got = ob.condattr_download()
    keys = ref.keys(cfg)
    K = len(keys)
    n, S, R = want["dims"]
    assert (c.n_spans, c.n_scopes, c.n_resources) == (n, S, R)
    assert (c.arena, c.arena_bytes, c.scope, c.scope_resource, c.span_size) == \
        (ob.cols.arena, ob.cols.arena_bytes, ob.cols.scope, ob.cols.scope_resource, ob.cols.span_size)
    arena = got["arena"][:c.arena_bytes].tobytes()
    for name, rows in (("span", n), ("scope", S), ("res", R)):
        has = got[name + "_has"][:K * rows]
        val = got[name + "_val"][:8 * K * rows].view(np.uint32).reshape(-1, 2)
        whas, wstr = want[name]
        np.testing.assert_array_equal(has, whas, err_msg=name + "_has")
        for x, w in wstr.items():
            o, ln = int(val[x][0]), int(val[x][1])
            assert o + ln <= c.arena_bytes and arena[o:o + ln] == w, (name, keys[x // rows], x % rows, arena[o:o + ln][:40], w[:40])
    tk = [k for k, key in enumerate(keys) if key in ref.targets(cfg)]
    kv = got["span_kv_size"][:4 * K * n].view(np.uint32)
    whas = want["span"][0]
    for k in tk:
        m = whas[k * n:(k + 1) * n] != 0
        np.testing.assert_array_equal(kv[k * n:(k + 1) * n][m], want["kv"][k * n:(k + 1) * n][m], err_msg="span_kv_size " + keys[k])
    names = got["scope_name"][:8 * S].view(np.uint32).reshape(-1, 2)
    assert [arena[o:o + ln] for o, ln in names] == want["scope_name"]
    np.testing.assert_array_equal(got["scope"][:4 * n].view(np.uint32), want["span_scope"])
    np.testing.assert_array_equal(got["scope_resource"][:4 * S].view(np.uint32), want["scope_resource"])
    return got


_LISTED = {}


def kernel_listed(enc):
    """Per case: the span kernel alone (option off) sends the span to the host pass."""
    from odigos_amd.batch import OtlpBatch
    if enc.__name__ not in _LISTED:
        eng = node_engine(DEC_CFG, option=False)
        out = []
        for c in range(len(CASES)):
            ob = OtlpBatch(eng, enc(tree_of(_case_span(c, c))))
            assert ob.condattr_cols is None and ob.host_spans in (0, 1)
            out.append(ob.host_spans == 1)
            ob.close()
        _, tail = tail_tree_and_bytes()
        ob = OtlpBatch(eng, tail)
        assert ob.host_spans == 0   # the tail span is the condattr kernel's to read, up to the message's last byte
        ob.close()
        eng.close()
        _LISTED[enc.__name__] = out
    return _LISTED[enc.__name__]


@pytest.mark.gpu
def test_gpu_case_list_covers_the_ground():
    for enc in (gg.marshal_traces, to_pb):
        listed = kernel_listed(enc)
        needs = [c[2] for c in CASES]
        # spans only this stage sends to the host pass, spans only the span kernel sends, and both
        assert any(a and not b for a, b in zip(needs, listed)) and any(b and not a for a, b in zip(needs, listed))
        assert any(a and b for a, b in zip(needs, listed)) and any(not a and not b for a, b in zip(needs, listed))
    # span_kv_size against the marshalled KeyValue, for the target keys of the case list
    td, _, _ = dec_message(66, gg.marshal_traces)
    want = want_columns(DEC_CFG, 66, td)
    keys = ref.keys(DEC_CFG)
    seen = 0
    for i, sp in enumerate(spans_of(td)):
        for k, key in enumerate(keys):
            kv = ref._get(sp.get("attributes"), key)
            assert bool(want["span"][0][k * 66 + i]) == (kv is not None)
            if kv is not None and key in ref.targets(DEC_CFG):
                assert want["kv"][k * 66 + i] == len(gg._len(9, gg.key_value(kv)))
                seen += 1
    assert seen >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("enc", [gg.marshal_traces, to_pb], ids=["pdata", "protobuf"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 70_000])
def test_gpu_decode_columns(n, enc, mode):
    from odigos_amd.batch import OtlpBatch
    td, pb, case_ids = dec_message(n, enc)
    assert len(case_ids) == max(n - 1, 0)
    want = want_columns(DEC_CFG, n, td)
    assert want["dims"][0] == n
    listed = kernel_listed(enc)
    eng = node_engine(DEC_CFG)
    if mode:
        eng.set_option(mode, 1)
    ob = OtlpBatch(eng, pb)
    assert ob.cols.n_spans == n
    compare_columns(DEC_CFG, ob, want)
    # the spans that need AsString for one of the keys, together with those the span kernel lists (the tail: neither)
    expect_host = sum(1 for c in case_ids if CASES[c][2] or listed[c])
    print("n", n, "host_spans", ob.host_spans, "want", expect_host, "walk", ob.walk_info)
    assert ob.host_spans == expect_host
    if mode == "otlp_gpu_chain":
        assert ob.walk_info["gpu_chain"] == 1
    # a second decode on the warm engine (resources found in the device table, the batch object reused)
    ob.close()
    ob = OtlpBatch(eng, pb)
    compare_columns(DEC_CFG, ob, want)
    assert ob.host_spans == expect_host
    ob.close()
    eng.close()


@pytest.mark.gpu
def test_gpu_decode_redone_and_regrown():
    from odigos_amd.batch import OtlpBatch
    # a ScopeSpans with an unknown group field: the GPU scope walk hands the decode to the host walk (the redo)
    td, _ = dec_tree(65)
    grp = bytes([0xA3, 0x01, 0x08, 0x01, 0xA4, 0x01])   # field 20: start group, field 1 varint, end group
    extra_scope = {"scope": {"name": "lib", "attributes": [_KV("tg", 9)]}, "spans": [_case_span(0, 900), _case_span(1, 901)]}
    body = gg._len(1, gg._str(1, "lib") + gg._attrs(3, extra_scope["scope"]["attributes"])) + grp + \
        b"".join(gg._len(2, gg.span(sp)) for sp in extra_scope["spans"])
    rs = {"resource": {"attributes": [_KV("rk", "v")]}, "scopeSpans": [extra_scope]}
    pb = gg.marshal_traces(td) + gg._len(1, gg._len(1, gg._attrs(1, rs["resource"]["attributes"])) + gg._len(2, body))
    full = {"resourceSpans": td["resourceSpans"] + [rs]}
    want = want_columns(DEC_CFG, -65, full)
    eng = node_engine(DEC_CFG)
    ob = OtlpBatch(eng, pb)
    print("walk", ob.walk_info)
    assert ob.walk_info["scope_redo"] == 1
    compare_columns(DEC_CFG, ob, want)
    ob.close()
    # host-made strings past the arena's reserve: the arena is regrown and keeps what it held
    big = "B" * 400_000
    scopes = [{"scope": {"name": "n%d-" % s + big, "attributes": [_KV("rk", 1000 + s)]},
               "spans": [_case_span(1, s), _case_span(0, 100 + s)]} for s in range(4)]
    td2 = host.traces({"resource": {"attributes": [_KV("ff", 5)]}, "scopeSpans": scopes})
    want2 = want_columns(DEC_CFG, -2, td2)
    ob = OtlpBatch(eng, gg.marshal_traces(td2))
    print("walk", ob.walk_info)
    assert ob.walk_info["arena_regrown"] == 1
    compare_columns(DEC_CFG, ob, want2)
    ob.close()
    eng.close()


def _zero_outs(eng, n):
    import torch
    T = eng.condattr_info().n_targets
    t = {"src": torch.zeros(max(16, T * n), dtype=torch.uint8, device="cuda"),
         "val": torch.zeros(max(16, 8 * T * n), dtype=torch.uint8, device="cuda")}
    o = native.CondAttrOutputs()
    o.src, o.val = t["src"].data_ptr(), t["val"].data_ptr()
    return o, t


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [gg.marshal_traces, to_pb], ids=["pdata", "protobuf"])
def test_gpu_zero_spans(enc):
    """No span at all: an empty TracesData, and resources and scopes without
    spans — decoded, downloaded, run through the stage and encoded with the option on."""
    import torch
    from odigos_amd.batch import OtlpBatch
    eng = node_engine(DEC_CFG)
    td, pb, _ = dec_message(0, enc)
    for tree, msg, key in (({"resourceSpans": []}, b"", -1000), (td, pb, 0)):
        want = want_columns(DEC_CFG, key, tree)
        assert want["dims"][0] == 0
        ob = OtlpBatch(eng, msg)
        c = ob.condattr_cols
        assert c is not None and (c.n_spans, c.n_scopes, c.n_resources) == want["dims"] and ob.host_spans == 0
        compare_columns(DEC_CFG, ob, want)
        o, keep = _zero_outs(eng, 0)
        native.check(eng.L.ose_condattr_process_device(eng.h, C.byref(c), C.byref(o),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        path = {}
        got = eng.otlp_encode_condattr(ob, o, path=path)
        assert got == [("", gg.marshal_traces(tree), len(tree["resourceSpans"]))]
        assert got == ob.encode(0)
        # src / val may be NULL when there is nothing to index
        assert eng.otlp_encode_condattr(ob, native.CondAttrOutputs()) == got
        ob.close()
    eng.close()


@pytest.mark.gpu
def test_gpu_repeated_value_field_is_the_host_pass():
    """A KeyValue whose value field comes twice (protobuf merges them: the later
    string wins) and one whose key comes twice: otlp_condattr_kernel reads the
    last of each and relies on the span kernel sending such spans to the host
    pass, which this pins."""
    from odigos_amd.batch import OtlpBatch
    ids = gg._len(1, bytes.fromhex("11" * 16)) + gg._len(2, bytes.fromhex("22" * 8))
    two_values = gg._len(9, gg._len(1, b"rk") + gg._len(2, gg._len(1, b"first")) + gg._len(2, gg._len(1, b"v")))
    two_keys = gg._len(9, gg._len(1, b"zz") + gg._len(1, b"tg") + gg._len(2, gg._len(1, b"mine")))
    int_then_str = gg._len(9, gg._len(1, b"ff") + gg._len(2, gg._tag(3, 0) + gg._varint(7)) + gg._len(2, gg._len(1, b"s")))
    pb = gg._len(1, gg._len(1, b"") + gg._len(2, gg._len(1, b"") + gg._len(2, ids + two_values) + gg._len(2, ids + two_keys) +
                                              gg._len(2, ids + int_then_str) + gg._len(2, ids + gg._attrs(9, [_KV("rk", "v")]))))
    tid, sid = "11" * 16, "22" * 8
    td = tree_of({"traceId": tid, "spanId": sid, "attributes": [_KV("rk", "v")]},
                 {"traceId": tid, "spanId": sid, "attributes": [_KV("tg", "mine")]},
                 {"traceId": tid, "spanId": sid, "attributes": [_KV("ff", "s")]},
                 {"traceId": tid, "spanId": sid, "attributes": [_KV("rk", "v")]})
    from tests.test_otlp import _pb_to_json
    assert [sp["attributes"] for sp in spans_of(_pb_to_json(pb))] == [sp["attributes"] for sp in spans_of(td)]
    want = want_columns(DEC_CFG, -3000, td)
    for option in (False, True):
        eng = node_engine(DEC_CFG, option=option)
        ob = OtlpBatch(eng, pb)
        print("option", option, "host_spans", ob.host_spans)
        assert ob.host_spans == 3   # the span kernel's, with the option off too
        if option:
            compare_columns(DEC_CFG, ob, want)
        ob.close()
        eng.close()


@pytest.mark.gpu
def test_gpu_store_batch_is_refused():
    """A batch a groupbytrace store released has no columns of the stage, and
    the new download and encode refuse it."""
    from odigos_amd.batch import GroupByTrace, OtlpBatch
    L = native.lib()
    cfg, td = profile_tree(random.Random(4), 50, 6)
    eng = node_engine(cfg)
    ob = OtlpBatch(eng, gg.marshal_traces(td))
    assert ob.condattr_cols is not None
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, 1 << 20)
    g.add_otlp(ob, 0)
    rb, ntr = g.release_otlp(5_000_000_000)
    assert ntr > 0 and rb.cols.n_spans == 50 and rb.condattr_cols is None
    assert not L.ose_otlp_condattr_columns(rb.h)
    dst = native.CondAttrColumns()
    assert L.ose_otlp_condattr_download(rb.h, C.byref(dst)) == native.OSE_EINVAL
    o, keep = _zero_outs(eng, 50)
    out = C.c_void_p()
    assert L.ose_otlp_encode_condattr(eng.h, rb.h, C.byref(o), None, None, C.byref(out)) == native.OSE_EINVAL
    assert "groupbytrace" in native.last_error()
    assert len(rb.encode(0)[0][1]) > 0   # the plain encode still takes it
    # the decoded batch itself is still served
    assert eng.otlp_encode_condattr(ob, o) == ob.encode(0)
    g.close()
    ob.close()
    eng.close()


@pytest.mark.gpu
def test_gpu_decode_many_scopes_and_resources():
    """3,000 resources of 4 scopes each: the per-scope and per-resource columns
    are made by several threads, each with its own strings."""
    from odigos_amd.batch import OtlpBatch
    vals = ["v", 5, True, "", _NESTED, 2.5, "w" * 40]
    res = []
    for r in range(3000):
        ra = [_KV("service.name", "s%d" % (r % 7))] + ([_KV("rk", vals[r % 7]), _KV("tg2", "res-%d" % r)] if r % 3 else [])
        scopes = []
        for s in range(4):
            q = 4 * r + s
            sa = [_KV("ff", vals[q % 7])] + ([_KV("", "e%d" % (q % 11))] if q % 5 == 0 else [])
            scopes.append({"scope": {"name": "lib" if q % 2 else "name-%d" % (q % 97), "attributes": sa if q % 4 else []},
                           "spans": [_case_span(q % 4, q)] if q % 6 else []})
        res.append({"resource": {"attributes": ra}, "scopeSpans": scopes})
    td = {"resourceSpans": res}
    want = want_columns(DEC_CFG, -4000, td)
    assert want["dims"][1:] == (12000, 3000)
    eng = node_engine(DEC_CFG)
    for mode in (None, "otlp_host_scopes"):
        if mode:
            eng.set_option(mode, 1)
        ob = OtlpBatch(eng, gg.marshal_traces(td))
        compare_columns(DEC_CFG, ob, want)
        ob.close()
    eng.close()


class NodeRun:
    """decode -> ose_condattr_process_device on the decoded columns -> SIZE
    with span_size_out -> ose_otlp_encode_condattr, all on one stream."""

    def __init__(self, eng, pb, router=None, src_patch=None, val_patch=None, arena_bytes=None):
        import torch
        from odigos_amd.batch import OtlpBatch
        self.eng = eng
        ob = self.ob = OtlpBatch(eng, pb)
        c = ob.condattr_cols
        info = eng.condattr_info()
        n, T = c.n_spans, info.n_targets
        self.n, self.T = n, T
        words = int(eng.L.ose_condattr_scratch_words(eng.h, c.n_scopes))
        z = lambda nbytes: torch.zeros(max(16, nbytes), dtype=torch.uint8, device="cuda")   # noqa: E731
        self.t = {"src": torch.full((max(16, T * n),), 0xEE, dtype=torch.uint8, device="cuda"), "val": z(8 * T * n),
                  "span_size_out": z(4 * n), "scratch": z(4 * words), "device_status": z(16)}
        o = native.CondAttrOutputs()
        for k, v in self.t.items():
            setattr(o, k, v.data_ptr())
        self.outs = o
        st = torch.cuda.current_stream().cuda_stream
        native.check(eng.L.ose_condattr_process_device(eng.h, C.byref(c), C.byref(o), C.c_void_p(st)))
        ob.cols.span_size = self.t["span_size_out"].data_ptr()
        eng.process_device(ob, native.STAGE_SIZE, native.GROUP_TRACE_ID, stream=st)
        torch.cuda.synchronize()
        self.src = self.t["src"].cpu().numpy()[:T * n].copy()
        self.val = self.t["val"].cpu().numpy()[:8 * T * n].view(np.uint32).reshape(-1, 2).copy()
        self.res_bytes = ob.out_numpy("res_bytes", np.uint64, n=c.n_resources).copy()
        self.path = {}
        self.out = eng.otlp_encode_condattr(ob, o, router, stream=st, path=self.path)

    def values(self):
        """Per target and span: None (KEEP) or the put's bytes."""
        arena = self.ob.condattr_download()["arena"].tobytes()
        strings = self.eng.condattr_strings()
        out = []
        for x in range(self.T * self.n):
            s = int(self.src[x])
            assert s in (native.CA_KEEP, native.CA_ARENA, native.CA_CONFIG)
            o, ln = int(self.val[x][0]), int(self.val[x][1])
            out.append(None if s == native.CA_KEEP else (strings if s == native.CA_CONFIG else arena)[o:o + ln])
        return out


def check_node(cfg, td, enc, eng, gpu):
    from tests.test_condattr import Batch
    targets, puts = restated_puts(cfg, td)
    run = NodeRun(eng, enc(td))
    n = run.n
    print("path", run.path, "host_spans", run.ob.host_spans)
    assert run.path["gpu"] == gpu, run.path
    assert run.out == expected(td, targets, puts)
    applied = apply_puts(td, targets, puts)
    np.testing.assert_array_equal(run.res_bytes, np.array([len(gg.resource_spans(rs)) for rs in applied["resourceSpans"]],
                                                          dtype=np.uint64))
    # src / val: the restatement's puts, and ose_condattr_process on the columniser's batch
    vals = run.values()
    assert vals == [None if t not in puts[i] else _b(puts[i][t]) for t in targets for i in range(n)]
    b = Batch(cfg, td)
    eng.condattr_process(b.hb)
    np.testing.assert_array_equal(run.src, b.hb.src[:len(run.src)])
    strings = eng.condattr_strings()
    for x in np.nonzero(run.src)[0]:
        o, ln = (int(v) for v in b.hb.val[x])
        assert (strings if b.hb.src[x] == native.CA_CONFIG else b.arena)[o:o + ln] == vals[x]
    run.ob.close()
    return run


@pytest.mark.gpu
def test_gpu_node_pipeline_golden_cases():
    by_cfg = {}
    for cfg, c in kat_cases():
        by_cfg.setdefault(host.dumps(cfg), (cfg, []))[1].append(c)
    assert len(by_cfg) >= 2
    for cfg, cases in by_cfg.values():
        eng = node_engine(cfg)
        td = {"resourceSpans": [kat_tree(c)["resourceSpans"][0] for c in cases]}
        check_node(cfg, td, gg.marshal_traces, eng, gpu=True)
        check_node(cfg, td, to_pb, eng, gpu=False)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("enc,gpu", [(gg.marshal_traces, True), (to_pb, False)], ids=["pdata", "protobuf"])
def test_gpu_node_pipeline_profile_and_adversarial(enc, gpu):
    from tests.test_condattr import adversarial
    cfg, td = profile_tree(random.Random(0xCA7E), 2000, 80)
    eng = node_engine(cfg)
    run = check_node(cfg, td, enc, eng, gpu)
    if not gpu:
        assert run.path["fallback"] & 1   # kEncFbSpan: spans that are not in pdata's encoding
    eng.close()
    b, _ = adversarial()
    assert b.n == 4099 and len(b.targets) <= enc_ca_targets()
    eng = node_engine(b.cfg)
    check_node(b.cfg, b.td, enc, eng, gpu)
    eng.close()


@pytest.mark.gpu
def test_gpu_encoder_bound_and_host_path():
    T = enc_ca_targets()
    for t, gpu in ((T, True), (T + 1, False)):
        targets = ["t%02d" % k for k in range(t)]
        cfg = {"global_default": "d", "rules": [{"field_to_check": "k", "new_attribute_value_configurations": {
            "v": [{"new_attribute": x, "value": "val-" + x} for x in targets[::2]] +
                 [{"new_attribute": x, "from_field": "f"} for x in targets[1::2]]}}]}
        assert ref.targets(cfg) == sorted(targets, key=lambda x: (targets.index(x) % 2, x))
        spans = [host.span(name="a", attributes={"k": "v", "f": "copied", targets[3]: 1, targets[-1]: "z"}),
                 host.span(name="b", attributes={"k": "v"}), host.span(name="c", attributes={targets[0]: "mine"}),
                 host.span(name="d")]
        td = host.traces(host.resource_spans({"service.name": "s"}, [copy.deepcopy(sp) for sp in spans * 40]))
        eng = node_engine(cfg)
        run = check_node(cfg, td, gg.marshal_traces, eng, gpu)
        if not gpu:
            assert run.path["fallback"] == 64   # kEncFbCa
        eng.set_option("encode_host", 1)
        check_node(cfg, td, gg.marshal_traces, eng, False)
        eng.close()


@pytest.mark.gpu
def test_gpu_node_pipeline_routes_like_the_plain_encoder():
    from odigos_amd.batch import OtlpBatch, Router
    cfg = adv_config()
    td = adv_tree(0x20D7, 600, 9, 30)
    for r, rs in enumerate(td["resourceSpans"]):
        if r % 3 != 2:
            rs["resource"]["attributes"] += host.attrs({"k8s.deployment.name": "d%d" % (r % 3)})
    targets, puts = restated_puts(cfg, td)
    router = Router({"datastreams": STREAMS})
    eng = node_engine(cfg)
    for enc, gpu in ((gg.marshal_traces, True), (to_pb, False)):
        pb = enc(td)
        run = NodeRun(eng, pb, router=router)
        assert run.path["gpu"] == gpu
        assert run.out == expected(td, targets, puts, STREAMS, router.pipelines)
        plain = OtlpBatch(eng, pb)
        routed = plain.encode(0, router=router)
        assert [(p, k) for p, _, k in run.out] == [(p, k) for p, _, k in routed]
        assert routed == [(p, gg.marshal_traces(x), len(x["resourceSpans"]))
                          for p, x in gg.split_by_pipeline(td, STREAMS, router.pipelines)]
        assert sum(1 for _, _, k in routed if k) == 3
        plain.close()
        run.ob.close()
    eng.close()
    router.close()


@pytest.mark.gpu
def test_gpu_option_and_refusals():
    import torch
    from odigos_amd.batch import Engine, OtlpBatch
    L = native.lib()
    cfg, td = profile_tree(random.Random(3), 200, 12)
    pb = gg.marshal_traces(td)
    eng = node_engine(cfg, option=False)
    # option off: no columns, the new encode refused, and everything as with the option on
    off = OtlpBatch(eng, pb)
    assert off.condattr_cols is None and not L.ose_otlp_condattr_columns(off.h)
    out = C.c_void_p()
    ca = native.CondAttrOutputs()
    assert L.ose_otlp_encode_condattr(eng.h, off.h, C.byref(ca), None, None, C.byref(out)) == native.OSE_ENOTSUP
    assert "otlp_condattr" in native.last_error()
    cols_off, bytes_off = off.download(), off.encode(0)
    eng.set_option("otlp_condattr", 1)
    on = OtlpBatch(eng, pb)
    assert on.condattr_cols is not None
    cols_on = on.download()
    assert set(cols_on) == set(cols_off)
    for name in cols_off:   # (the arena: the same bytes, then the strings of the stage's per-scope and per-resource columns)
        k = off.cols.arena_bytes if name == "arena" else len(cols_off[name])
        np.testing.assert_array_equal(cols_on[name][:k], cols_off[name][:k], err_msg=name)
    for f, _ in native.Columns._fields_:
        if f.startswith("n_") or f in ("attr_match_words", "match_planes"):
            assert getattr(on.cols, f) == getattr(off.cols, f), f
    assert on.encode(0) == bytes_off == [("", pb, len(td["resourceSpans"]))]
    # the host pass: the span kernel's own spans (an int method) and those whose odigos.category needs AsString
    ints = lambda key: {i for i, sp in enumerate(spans_of(td))   # noqa: E731
                        if (kv := ref._get(sp["attributes"], key)) is not None and "stringValue" not in kv["value"]}
    mine, theirs = ints("odigos.category"), ints("http.request.method") | ints("http.method")
    assert mine - theirs and off.host_spans == len(theirs) and on.host_spans == len(mine | theirs)
    assert on.cols.arena_bytes >= off.cols.arena_bytes
    # a batch decoded with the option off
    n, T = on.cols.n_spans, eng.condattr_info().n_targets
    src = torch.zeros(T * n + 16, dtype=torch.uint8, device="cuda")
    val = torch.zeros(8 * T * n + 16, dtype=torch.uint8, device="cuda")
    ca.src, ca.val = src.data_ptr(), val.data_ptr()
    assert L.ose_otlp_encode_condattr(eng.h, off.h, C.byref(ca), None, None, C.byref(out)) == native.OSE_EINVAL
    assert "option" in native.last_error()
    # all KEEP: the message as it is; NULL src / val
    assert eng.otlp_encode_condattr(on, ca) == [("", pb, len(td["resourceSpans"]))]
    for hole in ("src", "val"):
        bad = native.CondAttrOutputs()
        bad.src, bad.val = ca.src, ca.val
        setattr(bad, hole, None)
        assert L.ose_otlp_encode_condattr(eng.h, on.h, C.byref(bad), None, None, C.byref(out)) == native.OSE_EINVAL
    assert L.ose_otlp_encode_condattr(eng.h, on.h, None, None, None, C.byref(out)) == native.OSE_EINVAL
    # a src of 3; refs one byte past the arena and the string table (device and host memory)
    strings = eng.condattr_strings()
    for host_mem in (False, True):
        for s, ref_, code in ((3, (0, 0), native.OSE_EINVAL),
                              (native.CA_ARENA, (on.cols.arena_bytes - 3, 4), native.OSE_ERANGE),
                              (native.CA_ARENA, (on.cols.arena_bytes + 1, 0), native.OSE_ERANGE),
                              (native.CA_CONFIG, (len(strings) - 1, 2), native.OSE_ERANGE),
                              (native.CA_CONFIG, (0xFFFFFFFF, 2), native.OSE_ERANGE)):
            hs = np.zeros(T * n + 16, dtype=np.uint8)
            hv = np.zeros((T * n + 2, 2), dtype=np.uint32)
            hs[n + 5] = s
            hv[n + 5] = ref_
            if host_mem:
                keep = (hs, hv)
                ca.src, ca.val = hs.ctypes.data, hv.ctypes.data
            else:
                keep = (torch.from_numpy(hs).cuda(), torch.from_numpy(hv.view(np.uint8).reshape(-1)).cuda())
                ca.src, ca.val = keep[0].data_ptr(), keep[1].data_ptr()
            assert L.ose_otlp_encode_condattr(eng.h, on.h, C.byref(ca), None, None, C.byref(out)) == code, (s, ref_, host_mem)
        # the last bytes of both buffers are fine
        hs[n + 5] = native.CA_ARENA
        hv[n + 5] = (on.cols.arena_bytes - 4, 4)
        hs[n + 6] = native.CA_CONFIG
        hv[n + 6] = (len(strings) - 2, 2)
        if host_mem:
            ca.src, ca.val = hs.ctypes.data, hv.ctypes.data
        else:
            keep = (torch.from_numpy(hs).cuda(), torch.from_numpy(hv.view(np.uint8).reshape(-1)).cuda())
            ca.src, ca.val = keep[0].data_ptr(), keep[1].data_ptr()
        got = eng.otlp_encode_condattr(on, ca)
        assert got[0][1].count(strings[-2:]) >= 1 and len(got[0][1]) > len(pb)
    # the option needs the section; another engine's batch is refused (a store's batch: test_gpu_store_batch_is_refused)
    plain = Engine({"odigostrafficmetrics": TRAFFIC})
    with pytest.raises(native.OseError, match="not configured") as ei:
        plain.set_option("otlp_condattr", 1)
    assert ei.value.code == native.OSE_EINVAL
    other = node_engine(cfg)
    ca.src, ca.val = src.data_ptr(), val.data_ptr()
    assert L.ose_otlp_encode_condattr(other.h, on.h, C.byref(ca), None, None, C.byref(out)) == native.OSE_EINVAL
    # OSE_STAGE_CONDATTR stays refused by the entry points with a stage mask
    assert L.ose_otlp_encode(eng.h, on.h, None, native.STAGE_CONDATTR, 0, None, None, C.byref(out)) == native.OSE_ENOTSUP
    eng.set_option("otlp_condattr", 0)
    assert OtlpBatch(eng, pb).condattr_cols is None
    for e in (other, plain, eng):
        e.close()
