"""Hand-laid OTLP wire forms for the GPU decoder (tests/test_decode_layouts.py):
otlp_kernel.hip, otlp_sqlop_kernel.hip, pb_device.hpp and the walk in
otlp_host.cpp (decode, res_walk_gpu, scope_walk_gpu, DevResTable).

A layout is a TracesData message written here byte by byte, with the wire
form under control: varints padded with continuation bytes (V(x, width)),
fields in any order, raw unknown fields of every wire type, repeated scalars,
merged sub-messages.  Every span's span_id carries its global index, so a span
decoded into the wrong row shows in the columns.  Test infrastructure only.

The reference is independent of the engine's parser: from_pb() parses the
message with google.protobuf (the descriptor of tests/test_size.py) into the
OTLP/JSON tree, the inverse of tests/test_otlp.to_pb; the host columniser over
that tree (host.Processor.columnarize, the path every other test pins to the C
oracle) gives the expected columns.

census() restates the decoder's dispatch (not its parsing) as a pure function
of the layout and its config: which spans take the host pass and why, the
chunks of every 64-span round and whether it is staged, which span kernel
runs, where the key table sits, what the resource table does with every
resource on a cold and on a warm engine (the probe walk under the restated
FNV-1a), how every scope is sized, and, for the chain layouts, where the true
chain enters every 64 KiB segment and whether the link holds.  Each layout
asserts through it that it sits where its docstring says.

The constants are parsed from the sources at import (K); DESIGNED pins the
values the layouts were drawn for, REDRAW says which families a change moves.

Forms left out, and why
-----------------------
* Field numbers of 2^29 and above: not a protobuf field number; gogo's
  generated code takes the tag as a uint64 and skips it, upb rejects it.
* Strings that are not valid UTF-8: proto3 `string` fields; google.protobuf
  refuses to parse them, gogo does not check.
* Groups (wire types 3 and 4): upb and gogo both skip unknown groups, but the
  device decoder hands every group to the host pass or the host walk by design;
  the host unmarshaler's group skipping is tested in test_otlp.py.
* The same message-typed oneof member twice in one AnyValue (two array_value
  fields): google.protobuf merges them, gogo replaces the first by the second.
* Tags and length varints wider than 5 bytes: gogo reads both as 64-bit
  varints, upb refuses a tag or a length of more than 5 bytes.  These widths
  ARE decoded and compared (the width-10 layouts); their reference is parsed
  from the same layout built with those two kinds of varint narrowed to 5 bytes
  (Layout.ref_pb).  Padding a varint with zero continuation groups changes
  no field's value, so both builds carry the same tree.  Value varints are
  padded to 10 bytes in both builds.

Restated from the raw bytes in from_pb (the descriptor of test_size.py cannot
say them): the TracesData level itself (a chain of field 1 records, everything
else skipped) and ResourceSpans field 1000, the retired
instrumentation_library_spans, which takes the place of an absent field 2 as
pdata's migration does.  Enum values outside the named ones need no
restatement: the descriptor types kind and the status code as int32.

Malformed messages (MALFORMED) have no reference columns, only OSE_EINVAL.
"""
from __future__ import annotations

import base64
import copy
import re
import struct
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from odigos_amd import host
from tests import encode_layouts as el
from tests import otlp_gogo as gg
from tests.encode_layouts import TID, Res, Scope, fit, pad_span, span_id

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
M64 = (1 << 64) - 1
WAVE = 64
SQL_SECTION = "odigossqldboperationprocessor"


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    dec = (CSRC / "otlp_kernel.hip").read_text()
    hpp = (CSRC / "kernels.hpp").read_text()
    hst = (CSRC / "otlp_host.cpp").read_text()

    def one(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: definition not found"
        return m

    def num(text, name, ctype=r"uint\d+_t"):
        return int(one(text, r"constexpr\s+" + ctype + r"\s+" + name + r"\s*=\s*(\d+)\s*;", name).group(1))

    k = SimpleNamespace()
    k.kSpanStage = num(dec, "kSpanStage")
    k.kSpanStageMax = num(dec, "kSpanStageMax")
    m = one(dec, r"constexpr\s+uint32_t\s+kKeyLds\s*=\s*(\d+)\s*,\s*kKeyBytesLds\s*=\s*(\d+)\s*;", "kKeyLds")
    k.kKeyLds, k.kKeyBytesLds = int(m.group(1)), int(m.group(2))
    k.kOtlpMaxAttrKeys = num(hpp, "kOtlpMaxAttrKeys")
    k.kOThreads = int(one(dec, r"#define\s+OSE_OTHREADS\s+(\d+)", "OSE_OTHREADS").group(1))
    assert "constexpr int kOThreads = OSE_OTHREADS;" in dec
    m = one(hpp, r"constexpr\s+uint32_t\s+kChainSeg\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", "kChainSeg")
    k.kChainSeg = int(m.group(1)) << int(m.group(2))
    k.kChainList = num(hpp, "kChainList")
    m = one(hpp, r"constexpr\s+uint32_t\s+kResSlots\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", "kResSlots")
    k.kResSlots = int(m.group(1)) << int(m.group(2))
    probes = set(re.findall(r"probe\s*<\s*(\d+)\s*;", dec) + re.findall(r"probe\s*<\s*(\d+)\s*;", hst))
    assert len(probes) == 1, f"the resource table's probe limit differs between lookup and insert: {probes}"
    k.res_probes = int(probes.pop())
    k.sync_whole = int(one(hst, r"changed\.size\(\)\s*>\s*(\d+)", "DevResTable::sync's whole-table threshold").group(1))
    m = one(hst, r"constexpr\s+size_t\s+kGpuScopeBytes\s*=\s*size_t\((\d+)\)\s*<<\s*(\d+)\s*;", "kGpuScopeBytes")
    k.kGpuScopeBytes = int(m.group(1)) << int(m.group(2))
    m = one(hst, r"fix_reserve\s*=\s*std::max<size_t>\(1\s*<<\s*(\d+),\s*len\s*/\s*(\d+)\)", "fix_reserve")
    k.fix_reserve_min, k.fix_reserve_div = 1 << int(m.group(1)), int(m.group(2))
    m = one(hst, r"want\s*=\s*up\(std::max<size_t>\(bytes \+ bytes / (\d+), 1 << (\d+)\), 1 << (\d+)\)", "DevBuf::need")
    k.buf_slack_div, k.buf_min, k.buf_round = int(m.group(1)), 1 << int(m.group(2)), 1 << int(m.group(3))
    k.fnv_seed = int(one(hpp, r"kResHashSeed\s*=\s*0x([0-9A-Fa-f]+)ull", "kResHashSeed").group(1), 16)
    k.fnv_prime = int(one(hpp, r"res_key_hash_step[^}]*\(h \^ b\) \* 0x([0-9A-Fa-f]+)ull", "res_key_hash_step").group(1), 16)
    # the key-length filter: bit min(len, 63) on both sides
    k.key_len_bits = 64 if ("std::min<size_t>(kv.first.size(), 63)" in hst and "(l < 63 ? l : 63)" in dec) else 0
    return k


K = _parse_constants()
DESIGNED = dict(kSpanStage=24576, kSpanStageMax=65536, kKeyLds=128, kKeyBytesLds=4096, kOtlpMaxAttrKeys=56,
                kOThreads=64, kChainSeg=65536, kChainList=16, kResSlots=1 << 17, res_probes=64, sync_whole=256,
                kGpuScopeBytes=65536, fix_reserve_min=65536, fix_reserve_div=8, buf_slack_div=4, buf_min=1 << 20,
                buf_round=1 << 16, fnv_seed=0xCBF29CE484222325, fnv_prime=0x100000001B3, key_len_bits=64)
# the layout families a constant's change moves
REDRAW = dict(kSpanStage="waves (stage-*, big-span)", kSpanStageMax="waves (spans-65536, spans-65537)",
              kKeyLds="keytab (keys-128, keys-129)", kKeyBytesLds="keytab (bytes-4096, bytes-4097)",
              kOtlpMaxAttrKeys="keytab (the keys past the role word)", kOThreads="resources (res-64, res-65), scopes (scopes-64, scopes-65)",
              kChainSeg="chain (every layout)", kChainList="chain (list-15, list-16, list-17)",
              kResSlots="resources (res-collide: the literal suffixes)", res_probes="resources (res-collide)",
              sync_whole="resources (res-256, res-257)", kGpuScopeBytes="scopes (scope-64k, scope-64k+1)",
              fix_reserve_min="hostpass (regrow)", fix_reserve_div="hostpass (regrow)", buf_slack_div="hostpass (regrow)",
              buf_min="hostpass (regrow)", buf_round="hostpass (regrow)", fnv_seed="resources (res-collide: the literal suffixes)",
              fnv_prime="resources (res-collide: the literal suffixes)", key_len_bits="keys (every layout), keytab (bytes-*)")


# ---------------------------------------------------------------------------
# the raw builder

_CAP = [10]   # the widest tag / length varint of the build in progress (Layout.ref_pb: 5)


def V(x: int, width: int = 0) -> bytes:
    """varint of x, padded with continuation bytes to `width` bytes (at most 10)"""
    b = bytearray(gg._varint(x))
    assert width <= 10
    while len(b) < width:
        b[-1] |= 0x80
        b.append(0)
    return bytes(b)


def tagv(f: int, wt: int, w: int = 0) -> bytes:
    return V((f << 3) | wt, min(w, _CAP[0]))


def lenv(n: int, w: int = 0) -> bytes:
    return V(n, min(w, _CAP[0]))


def lenf(f: int, payload, tw: int = 0, lw: int = 0) -> bytes:
    payload = gg._b(payload)
    return tagv(f, 2, tw) + lenv(len(payload), lw) + payload


def varf(f: int, v: int, tw: int = 0, vw: int = 0) -> bytes:
    return tagv(f, 0, tw) + V(v & M64, vw)


def f64(f: int, v: int, tw: int = 0) -> bytes:
    return tagv(f, 1, tw) + struct.pack("<Q", v)


def f32(f: int, v: int, tw: int = 0) -> bytes:
    return tagv(f, 5, tw) + struct.pack("<I", v)


def unknown(f: int, wt: int) -> bytes:
    """an unknown field of number f and wire type wt"""
    return {0: lambda: varf(f, 300), 1: lambda: f64(f, 0x1122334455667788), 2: lambda: lenf(f, b"\x0a\x03unk"),
            5: lambda: f32(f, 0xA1B2C3D4)}[wt]()


def unknowns(f: int) -> bytes:
    return b"".join(unknown(f, wt) for wt in (0, 1, 2, 5))


UNKNOWN_FIELDS = (17, 2047, (1 << 29) - 1)


def anyb(v, tw=0, lw=0, vw=0) -> bytes:
    """AnyValue payload of a Python scalar / AnyValue dict"""
    v = host.attr_value(v) if not (isinstance(v, dict) and not v) else {}
    if not v:
        return b""
    k, x = next(iter(v.items()))
    if k == "stringValue":
        return lenf(1, x, tw, lw)
    if k == "boolValue":
        return varf(2, 1 if x else 0, tw, vw)
    if k == "intValue":
        return varf(3, int(x), tw, vw)
    if k == "bytesValue":
        return lenf(7, base64.b64decode(x), tw, lw)
    return gg.any_value(v)


def kvb(key, value, tw=0, lw=0, vw=0) -> bytes:
    """KeyValue payload (pdata's form: key, then the value always framed)"""
    return lenf(1, key, tw, lw) + lenf(2, anyb(value, tw, lw, vw), tw, lw)


def attr(key, value, f=9, tw=0, lw=0, vw=0) -> bytes:
    return lenf(f, kvb(key, value, tw, lw, vw), tw, lw)


def ids(i: int, tw=0, lw=0) -> list:
    return [lenf(1, bytes.fromhex(TID), tw, lw), lenf(2, bytes.fromhex(span_id(i)), tw, lw)]


def S(i: int, *fields) -> bytes:
    """a Span payload: the ids, then the fields as given"""
    return b"".join(ids(i) + list(fields))


HTTP = ("http.request.method", "GET"), ("url.path", "/user/1234")
T0 = 1739000000000000000


def http(i: int, *more, kind=2, name="GET") -> bytes:
    return S(i, lenf(5, name), varf(6, kind), f64(7, T0 + i), f64(8, T0 + i + 9), *[attr(k, v) for k, v in HTTP], *more)


def full_fields(i: int, tw=0, lw=0, vw=0) -> list:
    """every field of a Span, every nested message non-empty"""
    a = dict(tw=tw, lw=lw, vw=vw)
    ev = f64(1, T0 + 5, tw) + lenf(2, "ev", tw, lw) + attr("e", 1, 3, **a) + attr("f", "x", 3, **a) + varf(4, 2, tw, vw)
    lk = (lenf(1, bytes.fromhex("ab" * 16), tw, lw) + lenf(2, bytes.fromhex("cd" * 8), tw, lw) + lenf(3, "ls=1", tw, lw) +
          attr("l", True, 4, **a) + varf(5, 3, tw, vw) + f32(6, 1, tw))
    return ids(i, tw, lw) + [
        lenf(3, "k=v", tw, lw), lenf(4, bytes.fromhex("ee" * 8), tw, lw), lenf(5, "GET", tw, lw), varf(6, 2, tw, vw),
        f64(7, T0 + i, tw), f64(8, T0 + i + 77, tw),
        attr("http.request.method", "GET", **a), attr("url.path", "/user/1234", **a), attr("http.route", "/user/{id}", **a),
        attr("tier", "gold", **a), attr("code", 503, **a), attr("flag", True, **a), attr("db.query.text", "select 1", **a),
        attr("db.operation.name", "SELECT", **a),
        varf(10, 4, tw, vw), lenf(11, ev, tw, lw), varf(12, 5, tw, vw), lenf(13, lk, tw, lw), varf(14, 6, tw, vw),
        lenf(15, lenf(2, "boom", tw, lw) + varf(3, 2, tw, vw), tw, lw), f32(16, 257, tw)]


def message(*res, prefix=b"", between=b"") -> bytes:
    """TracesData: `0A len record` per resource (Res, or raw record bytes)"""
    recs = [lenf(1, r.body() if isinstance(r, Res) else r) for r in res]
    return prefix + between.join(recs)


def res_hdr(attrs: dict, dropped: int = 0) -> bytes:
    return el.res_hdr(attrs, dropped)


SVC_A = res_hdr({"service.name": "svc-a", "k8s.pod.name": "pod-0", "telemetry.sdk.language": "go"})


def one_res(spans, hdr=SVC_A, scope_hdr=b"") -> bytes:
    return message(Res(hdr, [Scope(spans, scope_hdr)]))


# ---------------------------------------------------------------------------
# configs

def _rule(name, key, ctype="string", svc="svc-a", **kw):
    d = {"service_name": svc, "attribute_key": key, "condition_type": ctype, "sampling_ratio": 50}
    if ctype == "string":
        d.update(operation="equals", expected_value="gold")
    elif ctype == "number":
        d.update(operation="greater_than", expected_value="499")
    elif ctype == "json":
        d.update(operation="contains_key", json_path="$.a")
    d.update(kw)
    return {"name": name, "type": "span_attribute", "rule_details": d}


def make_cfg(rules, sql=True) -> dict:
    c = {"odigossampling": {
             "global_rules": [{"name": "errors", "type": "error", "rule_details": {"fallback_sampling_ratio": 40}}],
             "endpoint_rules": [{"name": "lat", "type": "http_latency",
                                 "rule_details": {"http_route": "/user", "service_name": "svc-a", "threshold": 20,
                                                  "fallback_sampling_ratio": 10}}] + list(rules)},
         "odigosurltemplate": {},
         "odigostrafficmetrics": {"res_attributes_keys": ["service.name", "k8s.pod.name"]}}
    if sql:
        c[SQL_SECTION] = {"exclude": {"language": ["python"]}}
    return c


BASE = make_cfg([_rule("tier", "tier"), _rule("num", "code", "number"), _rule("js", "body", "json")])
BUILTIN_KEYS = ("http.request.method", "http.method", "http.route", "url.template", "url.path", "http.target", "url.full",
                "http.url")


def _span_rules(cfg):
    s = cfg.get("odigossampling") or {}
    return [r["rule_details"] for lvl in ("global_rules", "service_rules", "endpoint_rules") for r in s.get(lvl) or []
            if r["type"] == "span_attribute"]


def plan_keys(cfg) -> list:
    """AttrPlan::keys: the distinct keys of the GPU-evaluated rules, level order"""
    out = []
    for d in _span_rules(cfg):
        if d["condition_type"] != "json" and d["attribute_key"] not in out:
            out.append(d["attribute_key"])
    return out


def json_keys(cfg) -> set:
    return {d["attribute_key"] for d in _span_rules(cfg) if d["condition_type"] == "json"}


def key_table(cfg) -> list:
    """the decoder's key table (otlp_engine: a std::map, so in byte order)"""
    return sorted({gg._b(k) for k in list(BUILTIN_KEYS) + plan_keys(cfg) + list(json_keys(cfg))})


def host_keys(cfg) -> set:
    """keys whose first occurrence sends the span to the host pass (kRoleHost)"""
    return set(json_keys(cfg)) | set(plan_keys(cfg)[K.kOtlpMaxAttrKeys:])


# ---------------------------------------------------------------------------
# the reference: google.protobuf -> OTLP/JSON

def _rd_varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v & M64, i


def fields(b, s=0, e=None):
    """(field, wire type, field start, payload start | varint value, payload length) of a well-formed message [s, e)"""
    e = len(b) if e is None else e
    i = s
    while i < e:
        at = i
        t, i = _rd_varint(b, i)
        f, wt = t >> 3, t & 7
        if wt == 0:
            v, i = _rd_varint(b, i)
            yield f, wt, at, v, 0
        elif wt == 2:
            n, i = _rd_varint(b, i)
            yield f, wt, at, i, n
            i += n
        else:
            n = {1: 8, 5: 4}[wt]
            yield f, wt, at, i, n
            i += n
    assert i == e, "a field runs past its message"


def _classes():
    from tests.test_size import _otlp_classes
    if not hasattr(_classes, "c"):
        _classes.c = _otlp_classes()
    return _classes.c


def _av(m) -> dict:
    w = m.WhichOneof("value")
    if w is None:
        return {}
    if w == "string_value":
        return {"stringValue": m.string_value}
    if w == "bool_value":
        return {"boolValue": bool(m.bool_value)}
    if w == "int_value":
        return {"intValue": str(m.int_value)}
    if w == "double_value":
        return host.attr_value(float(m.double_value))
    if w == "bytes_value":
        return {"bytesValue": base64.b64encode(m.bytes_value).decode()}
    if w == "array_value":
        return {"arrayValue": {"values": [_av(e) for e in m.array_value.values]}}
    return {"kvlistValue": {"values": [_kv(e) for e in m.kvlist_value.values]}}


def _kv(m) -> dict:
    return {"key": m.key, "value": _av(m.value)}


def _kvs(ms) -> list:
    return [_kv(m) for m in ms]


def _span(m) -> dict:
    st = {}
    if m.status.message:
        st["message"] = m.status.message
    if m.status.code:
        st["code"] = m.status.code
    return {"traceId": m.trace_id.hex(), "spanId": m.span_id.hex(), "parentSpanId": m.parent_span_id.hex(),
            "traceState": m.trace_state, "name": m.name, "kind": m.kind,
            "startTimeUnixNano": str(m.start_time_unix_nano), "endTimeUnixNano": str(m.end_time_unix_nano),
            "attributes": _kvs(m.attributes), "droppedAttributesCount": m.dropped_attributes_count,
            "events": [{"timeUnixNano": str(e.time_unix_nano), "name": e.name, "attributes": _kvs(e.attributes),
                        "droppedAttributesCount": e.dropped_attributes_count} for e in m.events],
            "droppedEventsCount": m.dropped_events_count,
            "links": [{"traceId": l.trace_id.hex(), "spanId": l.span_id.hex(), "traceState": l.trace_state,
                       "attributes": _kvs(l.attributes), "droppedAttributesCount": l.dropped_attributes_count,
                       "flags": l.flags} for l in m.links],
            "droppedLinksCount": m.dropped_links_count, "status": st, "flags": m.flags}


def _scope_spans(m) -> dict:
    return {"scope": {"name": m.scope.name, "version": m.scope.version, "attributes": _kvs(m.scope.attributes),
                      "droppedAttributesCount": m.scope.dropped_attributes_count},
            "spans": [_span(s) for s in m.spans], "schemaUrl": m.schema_url}


def from_pb(pb: bytes) -> dict:
    """The OTLP/JSON tree of a TracesData message (google.protobuf's parse)."""
    cls = _classes()
    rss = []
    for f, wt, _, ps, pl in fields(pb):
        if f != 1 or wt != 2:
            continue   # TracesData has one field
        rec = bytes(pb[ps:ps + pl])
        m = cls["ResourceSpans"]()
        m.ParseFromString(rec)
        scopes = list(m.scope_spans)
        if not scopes:   # field 1000 in the place of an absent field 2
            for f2, w2, _, qs, ql in fields(rec):
                if f2 == 1000 and w2 == 2:
                    s = cls["ScopeSpans"]()
                    s.ParseFromString(rec[qs:qs + ql])
                    scopes.append(s)
        rss.append({"resource": {"attributes": _kvs(m.resource.attributes),
                                 "droppedAttributesCount": m.resource.dropped_attributes_count},
                    "scopeSpans": [_scope_spans(s) for s in scopes], "schemaUrl": m.schema_url})
    return {"resourceSpans": rss}


# ---------------------------------------------------------------------------
# layouts

class Layout:
    """name, family, the message builder, the config; options: the engine
    options the layout is decoded under besides none; expect: what the
    layout's docstring claims, asserted through census()."""

    def __init__(self, name, family, make, doc, cfg=None, options=(), expect=None, big=False):
        self.name, self.family, self.make, self.doc = name, family, make, doc
        self.cfg = BASE if cfg is None else cfg
        self.options, self.expect, self.big = tuple(options), dict(expect or {}), big
        self._c = {}

    def _build(self, cap):
        if cap not in self._c:
            _CAP[0] = cap
            try:
                self._c[cap] = bytes(self.make())
            finally:
                _CAP[0] = 10
        return self._c[cap]

    @property
    def pb(self) -> bytes:
        return self._build(10)

    @property
    def ref_pb(self) -> bytes:
        """the same layout with tags and lengths no wider than 5 bytes (the module docstring)"""
        return self._build(5)

    @property
    def tree(self) -> dict:
        if "tree" not in self._c:
            self._c["tree"] = from_pb(self.ref_pb)
        return self._c["tree"]

    def tree_spans(self) -> list:
        return [sp for rs in self.tree["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]

    def cfg_no_sql(self) -> dict:
        c = copy.deepcopy(self.cfg)
        c.pop(SQL_SECTION, None)
        return c


LAYOUTS: dict = {}
# one layout per family for the SAMPLE|TEMPLATE|SIZE run (a family not named here: its first layout)
FAMILY_STAGE_LAYOUT = dict(keys="keys-64", waves="spans-129", scopes="scope-forms", resources="res-fields",
                           keytab="keytab-keys-129", hostpass="regrow")


def layout(name, family, doc, **kw):
    def deco(make):
        assert name not in LAYOUTS
        LAYOUTS[name] = Layout(name, family, make, doc, **kw)
        FAMILY_STAGE_LAYOUT.setdefault(family, name)
        return make
    return deco


# ---- wire forms ------------------------------------------------------------------

def _wire_spans():
    """[(label, builder(i))]: one span per lane"""
    out = []
    for w in (1, 2, 5, 10):
        out.append((f"tags-w{w}", lambda i, w=w: b"".join(full_fields(i, tw=w))))
        out.append((f"lens-w{w}", lambda i, w=w: b"".join(full_fields(i, lw=w))))
        out.append((f"values-w{w}", lambda i, w=w: b"".join(full_fields(i, vw=w))))
        out.append((f"all-w{w}", lambda i, w=w: b"".join(full_fields(i, tw=w, lw=w, vw=w))))
    out.append(("reversed", lambda i: b"".join(reversed(full_fields(i)))))
    # value before key; code before message; the Event and the Link backwards
    out.append(("reversed-inside", lambda i: S(
        i, lenf(9, lenf(2, anyb("gold")) + lenf(1, "tier")), lenf(15, varf(3, 2) + lenf(2, "boom")),
        lenf(11, varf(4, 2) + attr("e", 1, 3) + lenf(2, "ev") + f64(1, T0)),
        lenf(13, f32(6, 1) + varf(5, 3) + attr("l", 2.5, 4) + lenf(3, "s") + lenf(2, bytes.fromhex("cd" * 8)) +
             lenf(1, bytes.fromhex("ab" * 16))))))
    for f in UNKNOWN_FIELDS:
        u = unknowns(f)
        out.append((f"unknown-span-{f}", lambda i, u=u: S(i, u, lenf(5, "GET"), u, attr("tier", "gold"), u)))
        out.append((f"unknown-kv-{f}", lambda i, u=u: S(i, lenf(9, u + lenf(1, "tier") + u + lenf(2, anyb("gold")) + u))))
        out.append((f"unknown-any-{f}", lambda i, u=u: S(i, lenf(9, lenf(1, "tier") + lenf(2, u + anyb("gold") + u)),
                                                         lenf(9, lenf(1, "http.route") + lenf(2, anyb("/user") + u)))))
        out.append((f"unknown-status-{f}", lambda i, u=u: S(i, lenf(15, u + lenf(2, "boom") + u + varf(3, 2) + u))))
        out.append((f"unknown-event-{f}", lambda i, u=u: S(i, lenf(11, u + f64(1, T0) + u + lenf(2, "ev") + attr("e", 1, 3) + u))))
        out.append((f"unknown-link-{f}", lambda i, u=u: S(i, lenf(13, u + lenf(1, bytes.fromhex("ab" * 16)) + u +
                                                                  lenf(3, "s") + attr("l", 1, 4) + f32(6, 1) + u))))
    # each scalar twice: the last wins (the first span_id is another span's)
    out.append(("scalars-twice", lambda i: b"".join([
        lenf(1, bytes.fromhex("11" * 16)), lenf(2, bytes.fromhex(span_id(i + 1))), lenf(3, "first=1"),
        lenf(4, bytes.fromhex("22" * 8)), lenf(5, "first"), varf(6, 1), f64(7, 5), f64(8, 6), varf(10, 9), varf(12, 9),
        varf(14, 9), f32(16, 9)] + ids(i) + [lenf(3, "k=v"), lenf(4, b""), lenf(5, "GET"), varf(6, 3), f64(7, T0), f64(8, T0 + 1),
        varf(10, 1), varf(12, 0), varf(14, 300), f32(16, 0), attr("http.request.method", "GET"), attr("url.path", "/a/1")])))
    out.append(("trace-id-then-empty", lambda i: S(i, lenf(1, b""), lenf(4, bytes.fromhex("22" * 8)), lenf(4, b""))))
    # two Status messages merge
    out.append(("status-msg-then-code", lambda i: S(i, lenf(15, lenf(2, "boom")), lenf(15, varf(3, 2)))))
    out.append(("status-code-then-msg", lambda i: S(i, lenf(15, varf(3, 1)), lenf(5, "x"), lenf(15, lenf(2, "late")))))
    out.append(("status-code-overridden", lambda i: S(i, lenf(15, varf(3, 2) + lenf(2, "a")), lenf(15, varf(3, 0) + lenf(2, "")))))
    out.append(("status-empty-after", lambda i: S(i, lenf(15, varf(3, 2) + lenf(2, "kept")), lenf(15, b""))))
    # KeyValue forms
    out.append(("kv-two-keys", lambda i: S(i, lenf(9, lenf(1, "other") + lenf(1, "tier") + lenf(2, anyb("gold"))))))
    out.append(("kv-two-values", lambda i: S(i, lenf(9, lenf(1, "tier") + lenf(2, anyb("silver")) + lenf(2, anyb("gold"))))))
    out.append(("kv-two-values-second-empty", lambda i: S(i, lenf(9, lenf(1, "tier") + lenf(2, anyb("gold")) + lenf(2, b"")))))
    out.append(("kv-no-value", lambda i: S(i, lenf(9, lenf(1, "tier")), lenf(9, lenf(1, "code")))))
    out.append(("kv-empty-value", lambda i: S(i, lenf(9, lenf(1, "tier") + lenf(2, b"")))))
    out.append(("kv-no-key", lambda i: S(i, lenf(9, lenf(2, anyb("gold"))), lenf(9, b""))))
    out.append(("kv-two-keys-in-event", lambda i: S(i, lenf(11, lenf(3, lenf(1, "a") + lenf(1, "b") + lenf(2, anyb(1)))))))
    out.append(("kv-two-values-in-link", lambda i: S(i, lenf(13, lenf(4, lenf(1, "a") + lenf(2, anyb(1)) + lenf(2, anyb(2)))))))
    # AnyValue with two oneof members: the last wins
    for key in ("tier", "http.route", "db.query.text"):
        out.append((f"any-str-then-int-{key}", lambda i, key=key: S(i, lenf(9, lenf(1, key) + lenf(2, anyb("gold") + anyb(7))))))
        out.append((f"any-int-then-str-{key}", lambda i, key=key: S(i, lenf(9, lenf(1, key) + lenf(2, anyb(7) + anyb("gold"))))))
    out.append(("any-str-then-bytes", lambda i: S(i, lenf(9, lenf(1, "tier") + lenf(2, anyb("gold") + lenf(7, b"raw"))))))
    out.append(("any-array-then-str", lambda i: S(i, lenf(9, lenf(1, "tier") + lenf(2, lenf(5, lenf(1, anyb(1))) + anyb("gold"))))))
    out.append(("any-double-bool", lambda i: S(i, attr("code", 503.5), attr("tier", True), attr("flag", False))))
    # the same key twice: the first wins
    for key, a, b in (("tier", "gold", "silver"), ("tier", "silver", "gold"), ("http.route", "/user/{id}", "/other"),
                      ("db.query.text", "select 1", "select 2"), ("code", 500, 200), ("tier", 5, "gold"),
                      ("body", '{"a": 1}', "{"), ("http.route", 7, "/user")):
        out.append((f"dup-{key}-{a!r}", lambda i, key=key, a=a, b=b: http(i, attr(key, a), attr("x", 1), attr(key, b))))
    # bytes values
    raw = {"bytesValue": base64.b64encode(b"select 1").decode()}
    for key in ("tier", "http.route", "db.query.text", "url.path", "other"):
        out.append((f"bytes-{key}", lambda i, key=key: S(i, varf(6, 2), attr("http.method", "GET"), attr(key, raw))))
    # enums and counts at their edges
    for kind in (-1, 5, 255, 256, (1 << 32) + 3, 3):
        out.append((f"kind-{kind}", lambda i, kind=kind: S(i, varf(6, kind), attr("http.request.method", "GET"),
                                                            attr("url.template", "/t/{id}"), attr("http.route", "/r"))))
    for code in (-1, 3, 0, 2, (1 << 32) + 2):
        out.append((f"code-{code}", lambda i, code=code: S(i, lenf(15, varf(3, code)))))
    for d in (0, 1, (1 << 32) + 1, (1 << 32), (1 << 32) - 1):
        out.append((f"dropped-{d}", lambda i, d=d: S(i, varf(10, d), lenf(11, lenf(2, "ev") + varf(4, d)), varf(12, d),
                                                      lenf(13, varf(5, d)), varf(14, d))))
    out.append(("zero-times", lambda i: S(i, f64(7, 0), f64(8, 0), lenf(11, f64(1, 0)), lenf(13, f32(6, 0)), f32(16, 0))))
    out.append(("start-only", lambda i: S(i, f64(7, T0))))
    out.append(("end-only", lambda i: S(i, f64(8, T0))))
    out.append(("zero-ids", lambda i: b"".join([lenf(1, bytes(16)), lenf(2, bytes(8)), lenf(4, bytes(8)),
                                                lenf(13, lenf(1, bytes(16)) + lenf(2, bytes(8)))])))
    out.append(("nested-values", lambda i: S(i, attr("n", {"arrayValue": {"values": [{"intValue": "1"}]}}))))
    out.append(("nested-in-event", lambda i: S(i, lenf(11, attr("n", {"kvlistValue": {"values": []}}, 3)))))
    # db.query.text / db.operation.name in each form
    Q, O = "db.query.text", "db.operation.name"
    out.append(("sql-plain", lambda i: S(i, attr(Q, "select * from t"), attr(O, "SELECT"))))
    out.append(("sql-wide", lambda i: S(i, attr(Q, "select * from t", tw=5, lw=5), attr(O, 7, tw=2, lw=2, vw=10))))
    out.append(("sql-value-first", lambda i: S(i, lenf(9, lenf(2, anyb("select 1")) + lenf(1, Q)))))
    out.append(("sql-unknowns", lambda i: S(i, lenf(9, unknowns(17) + lenf(1, Q) + lenf(2, unknowns(2047) + anyb("select 1"))))))
    for v in (42, 2.5, True, {}, {"arrayValue": {"values": [{"stringValue": "select 1"}]}}):
        out.append((f"sql-nonstring-{v!r}"[:40], lambda i, v=v: S(i, attr(Q, v))))
    out.append(("sql-no-value", lambda i: S(i, lenf(9, lenf(1, Q)))))
    out.append(("sql-lookalikes", lambda i: S(i, attr("db.operation.namf", "x"), attr("db.query.texu", "select 1"),
                                              attr("db.query.tex", "s"), attr("db.operation.name2", "x"))))
    out.append(("sql-lookalike-then-real", lambda i: S(i, attr("db.operation.namf", "x"), attr(O, {}), attr("db.query.texu", 1),
                                                       attr(Q, "drop table t"))))
    out.append(("sql-in-event-only", lambda i: S(i, lenf(11, attr(Q, "select 1", 3)))))
    return out


WIRE = _wire_spans()
assert len(WIRE) <= 200 and len({w[0] for w in WIRE}) == len(WIRE)


@layout("wire", "wire", """Every wire form of the module docstring, one span per lane in one scope:
every varint-carrying field at widths 1, 2, 5 and 10; reversed order; unknown
varint / fixed64 / LEN / fixed32 fields 17, 2047 and 2^29-1 in Span,
KeyValue, AnyValue, Status, Event and Link; each scalar twice; merged Status;
KeyValues with two keys / two values (host pass) / none; two oneof members;
duplicate keys; bytes values; kind and status code outside their enums; dropped
counts past 2^32; explicit zeros; db.query.text and db.operation.name in each
form.""")
def _wire():
    return one_res([mk(i) for i, (_, mk) in enumerate(WIRE)])


@layout("wire-top", "wire", """Unknown fields of every wire type at the TracesData, ResourceSpans, ScopeSpans,
Resource and InstrumentationScope levels (fields 17, 2047, 2^29-1), level
fields out of order (spans before the scope, schema_url first), two schema_urls
(the last wins) and padded tags and lengths at every level.""")
def _wire_top():
    recs, i = [], 0
    for f in UNKNOWN_FIELDS:
        u = unknowns(f)
        scope = u + lenf(2, http(i)) + u + lenf(1, u + lenf(1, "lib") + u) + lenf(3, "first") + lenf(2, http(i + 1)) + lenf(3, "s-url") + u
        recs.append(u + lenf(3, "r-first") + lenf(2, scope) + u + lenf(1, u + SVC_A + u) + lenf(3, "r-url") + u)
        i += 2
    for w in (2, 5, 10):
        scope = lenf(1, lenf(1, "lib", w, w) + varf(4, 3, w, w), w, w) + lenf(2, http(i), w, w) + lenf(3, "s", w, w)
        recs.append(lenf(1, SVC_A, w, w) + lenf(2, scope, w, w) + lenf(3, "r", w, w))
        i += 1
    return b"".join(unknowns(f) for f in UNKNOWN_FIELDS) + b"".join(lenf(1, r, w, w) + unknowns(17)
                                                                    for r, w in zip(recs, (0, 2, 5, 0, 10, 1)))


# ---- lengths ----------------------------------------------------------------------

LENGTHS = (0, 127, 128, 16383, 16384)


@layout("lengths", "lengths", """Span, attribute value (tier, url.path), name and trace_state at 0, 127, 128,
16383 and 16384 bytes: every 1 -> 2 -> 3 byte step of a length varint, and the
empty Span message (`12 00`).""")
def _lengths():
    spans, i = [], 0
    for n in LENGTHS:
        spans.append(b"" if n == 0 else pad_span(i, n))
        spans.append(http(i + 1, attr("tier", "g" * n), attr("http.route", "/" * n)))
        spans.append(S(i + 2, lenf(5, "n" * n), attr("http.request.method", "n" * n)))
        spans.append(S(i + 3, lenf(3, "t" * n)))
        spans.append(S(i + 4, attr("http.method", "GET"), attr("url.path", "/" + "p" * (n - 1) if n else "")))
        i += 5
    return one_res(spans)


# ---- keys -------------------------------------------------------------------------

KEY_LENGTHS = (62, 63, 64, 65, 200)


def skey(n):   # the string rule's key of n bytes
    return "s" * (n - 1) + "x"


def jkey(n):   # the json rule's
    return "j" * (n - 1) + "x"


KEYS_CFG = make_cfg([_rule("tier", "tier")] + [_rule(f"s{n}", skey(n)) for n in KEY_LENGTHS] +
                    [_rule(f"j{n}", jkey(n), "json") for n in KEY_LENGTHS])


def _keys_layout(n):
    def make():
        body = '{"a": 1}'
        return one_res([
            http(0, attr(skey(n), "gold")),                       # the string rule's key: a STR column entry
            http(1, attr(jkey(n), body)),                         # the json rule's key: the host pass
            http(2, attr(skey(n)[:-1] + "y", "gold"), attr(jkey(n)[:-1] + "y", body)),   # lookalikes: the last byte differs
            http(3, attr(skey(n) + "z", "gold"), attr(jkey(n) + "z", body)),             # the key of interest is a proper prefix
            http(4, attr(skey(n)[:-1], "gold"), attr(jkey(n)[:-1], body)),               # ... and the carried key is
            http(5, attr(skey(n)[:-1] + "y", "silver"), attr(skey(n), 5), attr(skey(n), "gold")),   # first occurrence: an int
            http(6, attr("tier", "gold")),
        ])
    return make


for _n in KEY_LENGTHS:
    layout(f"keys-{_n}", "keys", f"""A string span_attribute rule and a json rule on keys of {_n} bytes (the key
filter's bit min(len, 63)): spans carrying the key, a lookalike of the same
length, and keys the rule's key is a prefix of / that are a prefix of it.""", cfg=KEYS_CFG,
           expect=dict(host_spans=[1]))(_keys_layout(_n))


# ---- alignment and message end ------------------------------------------------------

def _align_spans(i0=0):
    return [b"".join(full_fields(i0)), S(i0 + 1, attr("http.method", "GET"), attr("url.full", "https://example.com/a/1?x=1")),
            http(i0 + 2, attr("tier", "gold"), attr("db.query.text", "select 1"))]


for _k in range(16):
    layout(f"align-top-{_k}", "align", f"""The 3-span message behind a top-level unknown LEN field of {_k} payload bytes:
with align-top-0..15 the first span starts at every offset of a 16-byte chunk.""")(
        lambda k=_k: lenf(7, b"\x00" * k) + one_res(_align_spans()))
    layout(f"align-schema-{_k + 1}", "align", f"""The 3-span message with a ResourceSpans schema_url of {_k + 1} bytes written
before its scope_spans: the spans shift by one byte per layout.""")(
        lambda k=_k: message(lenf(1, SVC_A) + lenf(3, "u" * (k + 1)) + lenf(2, Scope(_align_spans()).body())))


def _end_layout(mod):
    def make():
        def build(k):
            last = S(1, attr("http.request.method", "GET"), attr("url.path", "/user/" + "7" * k))
            return one_res([http(0), last])
        return next(b for b in (build(k) for k in range(1, 40)) if len(b) % 16 == mod)
    return make


for _m in (0, 1, 15):
    layout(f"end-{_m}", "end", f"""The last span ends at the message's last byte, len % 16 == {_m}; its last
field is the url.path string, whose last word ByteReader::word reads past.""",
           expect=dict(len_mod=_m))(_end_layout(_m))


# ---- waves and staging ---------------------------------------------------------------

def host_span(i):
    return http(i, attr("http.route", 7))   # AsString of an int route: the host pass


def _mixed(i):
    if i % 7 == 3:
        return host_span(i)
    if i % 5 == 1:
        return el.min_span(i)
    return http(i, attr("tier", "gold" if i % 2 else "silver"))


for _n in (1, 63, 64, 65, 129):
    layout(f"spans-{_n}", "waves", f"""{_n} spans (every 7th takes the host pass): {-(-_n // 64)} round(s), the last
with {(_n - 1) % 64 + 1} live lane(s).""", expect=dict(n_spans=_n, rounds=-(-_n // 64)))(
        lambda n=_n: one_res([_mixed(i) for i in range(n)]))


def _np_min_spans(i0, n) -> np.ndarray:
    """n framed minimal spans (`12 20` + 32 bytes) with span ids i0.."""
    one = np.frombuffer(lenf(2, el.min_span(0)), dtype=np.uint8)
    a = np.tile(one, (n, 1))
    at = bytes(one).index(bytes.fromhex(span_id(0)))
    idx = np.arange(i0, i0 + n, dtype=np.uint64)
    for b in range(7):
        a[:, at + 1 + b] = ((idx >> np.uint64(8 * (6 - b))) & np.uint64(0xFF)).astype(np.uint8)
    return a.reshape(-1)


BIG_SPECIAL = (0, 63, 64, 4095, 4096, 40000, 65535)   # the host-pass spans among the minimal ones
BIG_SCOPE = 4096


def _big_layout(n):
    def make():
        scopes = []
        for s0 in range(0, n, BIG_SCOPE):
            s1 = min(n, s0 + BIG_SCOPE)
            parts, at = [lenf(1, b"")], s0
            for sp in [x for x in BIG_SPECIAL if s0 <= x < s1] + [s1]:
                if sp > at:
                    parts.append(_np_min_spans(at, sp - at).tobytes())
                if sp < s1:
                    parts.append(lenf(2, host_span(sp)))
                at = sp + 1
            scopes.append(lenf(2, b"".join(parts)))
        return lenf(1, lenf(1, SVC_A) + b"".join(scopes))
    return make


for _n, _kern in ((65536, 1), (65537, 2)):
    layout(f"spans-{_n}", "waves", f"""{_n} minimal 32-byte spans in scopes of {BIG_SCOPE} (built in numpy), a
scattering of them host-pass: {'the last batch of' if _kern == 1 else 'the first past'} kSpanStageMax, so the
{'LDS-staged' if _kern == 1 else 'HBM'} span kernel runs.""", expect=dict(n_spans=_n, span_kernel=_kern), big=True)(_big_layout(_n))


def _stage_layout(target):
    def make():
        def build(k):
            return one_res([el.min_span(i) for i in range(63)] + [S(63, attr("pad", "p" * k))])
        lo = 16 * (target - 145)
        for k in range(lo, lo + 400):
            b = build(k)
            if _rounds(spans_of(b))[0][0] == target:
                return b
        raise AssertionError("no pad reaches %d chunks" % target)
    return make


layout("stage-max", "waves", """A round of exactly kSpanStage/16 chunks: the largest that is staged in LDS.""",
       expect=dict(chunks=[K.kSpanStage // 16], staged=[True]))(_stage_layout(K.kSpanStage // 16))
layout("stage-over", "waves", """A round of kSpanStage/16 + 1 chunks: read from HBM by the LDS kernel.""",
       expect=dict(chunks=[K.kSpanStage // 16 + 1], staged=[False]))(_stage_layout(K.kSpanStage // 16 + 1))
layout("big-span", "waves", """One span above 24 KiB among 63 minimal ones (unstaged), then a staged round of
one live lane.""", expect=dict(staged=[False, True], rounds=2))(
    lambda: one_res([el.min_span(i) for i in range(31)] + [http(31, attr("tier", "g" * 25000))] +
                    [el.min_span(i) for i in range(32, 65)]))


# ---- host pass ---------------------------------------------------------------------

layout("host-all", "hostpass", """Every span takes the host pass (host_count == n): url.full, an int route, a
nested value, a json rule's key, a merged KeyValue in turn.""", expect=dict(host_all=True))(
    lambda: one_res([[S(i, attr("http.method", "PUT"), attr("http.url", "https://example.com/a/1")), http(i, attr("http.route", 7)),
                      http(i, attr("n", {"arrayValue": {"values": []}})), http(i, attr("body", '{"a": 1}')),
                      S(i, lenf(9, lenf(1, "a") + lenf(1, "tier") + lenf(2, anyb("gold"))))][i % 5] for i in range(70)]))
layout("host-none", "hostpass", """No span takes the host pass.""", expect=dict(host_none=True))(
    lambda: one_res([http(i, attr("tier", "gold")) if i % 2 else el.min_span(i) for i in range(70)]))

REGROW_CFG = make_cfg([_rule("tier", "tier"), _rule("route", "http.route"), _rule("path", "url.path"),
                       _rule("q", "db.query.text")])


def _regrow():
    spans = []
    for i in range(96):
        if i % 3 == 2:   # decoded on the GPU: its refs point into the message bytes, which move
            spans.append(http(i, attr("tier", "gold"), attr("http.route", "/user/{id}"), attr("db.query.text", "select %d" % i)))
        else:            # host pass (an int method): a 2 KiB path, route and query, each appended twice
            spans.append(S(i, varf(6, 2), attr("http.request.method", 7), attr("url.path", "/p%04d/" % i + "a" * 2300),
                           attr("http.route", "/r%04d/" % i + "b" * 2300), attr("db.query.text", "select %04d " % i + "c" * 2300)))
    return one_res(spans)


layout("regrow", "hostpass", """A message under 512 KiB whose host-pass spans carry long paths, routes and
queries that are also span_attribute keys, so the strings the host pass appends
exceed what the first arena holds past the message: the arena is regrown and
the message bytes move with it; the GPU-decoded spans' refs must still resolve.""", cfg=REGROW_CFG,
       expect=dict(regrown=True, max_len=512 << 10))(_regrow)


# ---- key table ---------------------------------------------------------------------

def _keytab_cfg(n_keys=None, n_bytes=None):
    """a config whose key table has n_keys keys, or n_bytes key bytes (the 8 built-in keys count)"""
    base = [_rule("last", "zz-last")]   # column 0, and the table's last key in byte order
    have = len(BUILTIN_KEYS) + 1
    if n_keys is not None:
        return make_cfg(base + [_rule(f"k{j}", "k%03d" % j) for j in range(n_keys - have)])
    used = sum(len(k) for k in BUILTIN_KEYS) + len("zz-last")
    rules, j = [], 0
    while n_bytes - used > 0:
        n = min(200, n_bytes - used)
        if 0 < n_bytes - used - n < 8:
            n -= 8
        rules.append(_rule(f"b{j}", ("b%03d-" % j).ljust(n, "k")))
        used += n
        j += 1
    return make_cfg(base + rules)


def _keytab_layout(cfg):
    def make():
        pk = plan_keys(cfg)
        tab = key_table(cfg)
        carried = [tab[-1].decode(), tab[0].decode(), pk[1], pk[-1], pk[min(len(pk) - 1, K.kOtlpMaxAttrKeys)],
                   pk[min(len(pk), K.kOtlpMaxAttrKeys) - 1]]
        return one_res([http(i, attr(k, "gold")) for i, k in enumerate(carried)] + [http(len(carried), attr("zz-lasu", "gold"))])
    return make


for _name, _kw, _lds in (("keys-128", dict(n_keys=128), True), ("keys-129", dict(n_keys=129), False),
                         ("bytes-4096", dict(n_bytes=4096), True), ("bytes-4097", dict(n_bytes=4097), False)):
    _cfg = _keytab_cfg(**_kw)
    layout("keytab-" + _name, "keytab", f"""A key table of {_name.replace('-', ' ')}: the workgroup's LDS copy is
{'still' if _lds else 'no longer'} taken; spans carry the table's last and first key.""", cfg=_cfg,
           expect=dict(key_lds=_lds, **{("n_keys" if "n_keys" in _kw else "key_bytes"): list(_kw.values())[0]}))(_keytab_layout(_cfg))


# ---- resources -----------------------------------------------------------------------

def _res_attrs(k, extra=None):
    d = {"service.name": "svc-" + "abcd"[k % 4], "k8s.pod.name": "pod-%d" % k}
    d.update(extra or {})
    return res_hdr(d)


def _scope1(i, n=1):
    return Scope([_mixed(i + j) for j in range(n)])


RES2 = gg._attrs(1, host.attrs({"k8s.namespace.name": "prod"}))

layout("res-fields", "resources", """No Resource field, one, and two (merged on the host, never keyed); field 1000
alone (taken for the scopes) and beside field 2 (ignored); schema_url of 0, 1
and 128 bytes; an empty Resource; the same Resource in two records.""",
       options=("otlp_host_resources",), expect=dict(unkeyed=1, n_res=9))(
    lambda: message(
        Res(None, [_scope1(0)]),
        Res(_res_attrs(1), [_scope1(1, 2)]),
        lenf(1, _res_attrs(2)) + lenf(2, _scope1(3).body()) + lenf(1, RES2),                      # two Resource fields
        lenf(1, _res_attrs(3)) + lenf(1000, _scope1(4).body()) + lenf(1000, _scope1(5).body()),     # field 1000 alone
        lenf(1, _res_attrs(4)) + lenf(1000, _scope1(6).body()) + lenf(2, _scope1(7).body()),        # ... beside field 2
        Res(_res_attrs(5), [_scope1(8)], schema=b"u"),
        Res(_res_attrs(5), [_scope1(9)], schema=b"u" * 128),
        Res(b"", [_scope1(10)]),
        Res(_res_attrs(1), [_scope1(11)])))

for _n in (64, 65, 256, 257):
    layout(f"res-{_n}", "resources", f"""{_n} distinct new resources in one call: {'one workgroup / two' if _n < 100 else "DevResTable::sync's per-slot copies / its whole-table copy"}
({'at' if _n in (64, 256) else 'past'} the edge).""", options=("otlp_host_resources",), expect=dict(n_res=_n, cold_misses=_n))(
        lambda n=_n: message(*[Res(_res_attrs(k), [_scope1(k)]) for k in range(n)]))

# 66 eight-byte suffixes of the attribute value "collide-" whose Resource bytes' FNV-1a
# values share their low 17 bits (found once by find_colliding_suffixes; fixed here)
COLLIDE_SUFFIXES = (
    47974, 70647, 137118, 148135, 307810, 1005888, 1190729, 1491359, 1513692, 1670167, 1685791, 1703599, 1751008,
    1754863, 1777091, 1805586, 1834706, 1927651, 2024134, 2078162, 2184560, 2224881, 2239579, 2243678, 2280163, 2366613,
    2408770, 2450030, 2465849, 2524237, 2910203, 2959946, 3003341, 3010681, 3128646, 3170333, 3321141, 3464402, 3470832,
    3510110, 3543416, 3645679, 3698684, 3762622, 3807524, 3849043, 3932923, 4541136, 4817690, 4979690, 5130284, 5187089,
    5197417, 5264782, 5364018, 5364958, 5418219, 5521488, 5659539, 5956932, 6052349, 6095565, 6119801, 6195230, 6247246,
    6250711)


def collide_res(suffix: int) -> bytes:
    return res_hdr({"service.name": "svc-a", "k8s.pod.name": "collide-%08x" % suffix})


def fnv1a(b: bytes) -> int:
    h = K.fnv_seed
    for c in b:
        h = ((h ^ c) * K.fnv_prime) & M64
    return h


def find_colliding_suffixes(n=66, span=1 << 24):
    """vectorised search: hash the fixed prefix once, then the 8 hex bytes of every suffix in numpy"""
    probe = collide_res(0)
    at = probe.index(b"00000000")
    assert probe[at + 8:] == b"", "the suffix is the Resource's last 8 bytes"
    h0 = fnv1a(probe[:at])
    idx = np.arange(span, dtype=np.uint64)
    h = np.full(span, h0, dtype=np.uint64)
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    with np.errstate(over="ignore"):
        for d in range(8):
            c = hexd[((idx >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)].astype(np.uint64)
            h = (h ^ c) * np.uint64(K.fnv_prime)
    low = (h & np.uint64(K.kResSlots - 1)).astype(np.int64)
    counts = np.bincount(low, minlength=K.kResSlots)
    slot = int(np.argmax(counts))
    assert counts[slot] >= n, "widen the search"
    return tuple(int(x) for x in np.nonzero(low == slot)[0][:n])


layout("res-collide", "resources", """66 resources whose FNV-1a values share their low 17 bits: the first 64 fill
the probe window, the 65th and 66th never enter the table and are resolved on
the host on every call.""", options=("otlp_host_resources",), expect=dict(n_res=66, never=2, warm_misses=2))(
    lambda: message(*[Res(collide_res(x), [_scope1(k)]) for k, x in enumerate(COLLIDE_SUFFIXES)]))


# ---- scopes --------------------------------------------------------------------------

def _scope_of_bytes(i, n):
    """ScopeSpans payload of exactly n bytes: an empty scope header, one padded span"""
    return fit(lambda k: Scope([S(i, attr("pad", "p" * k))]).body(), n, lo=1)


SCOPE_MODES = ("otlp_host_resources", "otlp_host_scopes")
layout("scope-64k", "scopes", """A ScopeSpans payload of exactly kGpuScopeBytes (walked on the GPU also under
otlp_host_resources) between two small ones.""", options=SCOPE_MODES, expect=dict(scope_bytes=K.kGpuScopeBytes))(
    lambda: message(Res(SVC_A, [_scope1(0)]).body() + lenf(2, _scope_of_bytes(1, K.kGpuScopeBytes)) + lenf(2, _scope1(2).body())))
layout("scope-64k+1", "scopes", """A ScopeSpans payload of kGpuScopeBytes + 1: walked on the host under
otlp_host_resources.""", options=SCOPE_MODES, expect=dict(scope_bytes=K.kGpuScopeBytes + 1))(
    lambda: message(Res(SVC_A, [_scope1(0)]).body() + lenf(2, _scope_of_bytes(1, K.kGpuScopeBytes + 1)) + lenf(2, _scope1(2).body())))
layout("scope-forms", "scopes", """Two InstrumentationScope fields (kOtlpScopeMulti: the host sizes the merge); a
scope attribute with an array value and one with a merged KeyValue (flags = 1:
host-sized); a scope with no spans between two that have spans; no
InstrumentationScope field; name, version, attributes and dropped count set;
two schema_urls.""", options=SCOPE_MODES, expect=dict(host_sized=[0, 1, 2], empty_scope=4))(
    lambda: message(Res(SVC_A, []).body() +
                    lenf(2, lenf(1, lenf(1, "lib")) + lenf(2, _mixed(0)) + lenf(1, lenf(2, "v2"))) +
                    lenf(2, lenf(1, lenf(1, "lib") + attr("a", {"arrayValue": {"values": [{"intValue": "1"}]}}, 3)) + lenf(2, _mixed(1))) +
                    lenf(2, lenf(1, lenf(3, lenf(1, "k") + lenf(2, anyb(1)) + lenf(2, anyb("s")))) + lenf(2, _mixed(2))) +
                    lenf(2, lenf(2, _mixed(3)) + lenf(2, _mixed(4))) +
                    lenf(2, lenf(1, lenf(1, "empty"))) +
                    lenf(2, lenf(1, lenf(1, "lib") + lenf(2, "1.0") + attr("a", "b", 3) + attr("c", 2, 3) + varf(4, 3)) +
                         lenf(3, "first") + lenf(2, _mixed(5)) + lenf(3, "schema"))))
for _n in (64, 65):
    layout(f"scopes-{_n}", "scopes", f"""{_n} scopes of one or two spans in 3 resources: {'one workgroup' if _n == 64 else 'two workgroups'} of the scope passes.""",
           options=SCOPE_MODES, expect=dict(n_scopes=_n))(
        lambda n=_n: message(*[Res(_res_attrs(r), [Scope([_mixed(2 * q), _mixed(2 * q + 1)][:1 + q % 2], gg._str(1, "lib%d" % (q % 3)))
                                                    for q in range(n) if q % 3 == r]) for r in range(3)]))


# ---- the TracesData chain (engine option otlp_gpu_chain) --------------------------------

def _rec_of(i, n, hdr=SVC_A):
    """a ResourceSpans record (tag and length included) of exactly n bytes with one span"""
    return fit(lambda k: lenf(1, Res(hdr, [Scope([S(i, attr("pad", "p" * k))])]).body()), n, lo=1)


def _small_rec(i):
    return lenf(1, Res(SVC_A, [_scope1(i)]).body())


CHAIN = ("otlp_gpu_chain",)
SEG = K.kChainSeg


def _chain_edges():
    a = _rec_of(0, SEG)                      # ends exactly at kChainSeg: the next starts exactly there
    b = _small_rec(1) + _small_rec(2)
    c = _rec_of(3, 2 * SEG + 1000)           # covers all of segment 2
    return a + b + c + b"".join(_small_rec(4 + j) for j in range(4)) + unknowns(17) + _small_rec(8) + unknowns(2047)


layout("chain-edges", "chain", """A record ending exactly at kChainSeg and the next starting exactly there; a
record that covers a whole segment; top-level unknown fields between records.""", options=CHAIN,
       expect=dict(n_seg=4, linked=True, enters={1: SEG}, covered=[2]))(_chain_edges)


def _chain_list(n_before):
    def make():
        # segment 1: the speculated start is inside segment 0's last record's long string, which
        # holds n_before small plausible records and then runs into the true chain
        inner = b"".join(_small_rec(100 + j) for j in range(n_before))
        head = _small_rec(0)
        def build(k):
            raw = {"bytesValue": base64.b64encode(b"p" * k + inner).decode()}   # (span ids are not UTF-8: a bytes value)
            last = lenf(1, Res(SVC_A, [Scope([S(1, attr("pad", raw))])]).body())
            return head + last
        # the inner records start right at the segment edge
        for k in range(SEG - 400, SEG):
            b = build(k)
            if b.index(inner) == SEG:
                return b + b"".join(_small_rec(2 + j) for j in range(4))
        raise AssertionError("the inner records do not reach the segment edge")
    return make


for _n, _ok in ((K.kChainList - 1, True), (K.kChainList, False), (K.kChainList + 1, False)):
    layout(f"chain-list-{_n}", "chain", f"""Segment 1's speculated start lies inside a long string of segment 0's last
record (a bytes value) that holds {_n} small records: the walk lists {_n} field starts before
the true entry, {'within' if _ok else 'past'} kChainList, so the link {'holds' if _ok else 'fails and the host walk decides'}.""",
           options=CHAIN, expect=dict(n_seg=2, linked=_ok, listed_before={1: _n}))(_chain_list(_n))


def _chain_fake():
    fake = b"".join(b"\x0a\x03\x0a\x01x" for _ in range(4)) + b"\x07\x07\x07"   # four plausible records, then field number 0
    def build(k):
        return _small_rec(0) + lenf(1, Res(SVC_A, [Scope([S(1, attr("pad", "p" * k + fake.decode() + "p" * 600))])]).body())
    for k in range(SEG - 400, SEG):
        b = build(k)
        if b.index(fake) == SEG:
            return b + _small_rec(2)
    raise AssertionError


layout("chain-fake", "chain", """A string attribute whose bytes at segment 1's start form four plausible
`0A len 0A ...` records and then break off: the segment's walk goes bad, the link
fails, the host walk decides.""", options=CHAIN, expect=dict(n_seg=2, linked=False))(_chain_fake)


# ---------------------------------------------------------------------------
# malformed messages: OSE_EINVAL, no reference

def _wrap(span: bytes) -> bytes:
    return one_res([http(0), span, http(2)])


MALFORMED = {
    "trace-id-3-bytes": _wrap(lenf(1, b"abc")),
    "span-id-7-bytes": _wrap(lenf(2, b"1234567")),
    "parent-id-16-bytes": _wrap(S(1, lenf(4, b"p" * 16))),
    "link-trace-id-8-bytes": _wrap(S(1, lenf(13, lenf(1, b"l" * 8)))),
    "truncated-kind-varint": _wrap(S(1) + b"\x30\x80"),
    "varint-of-11-bytes": _wrap(S(1) + b"\x30" + b"\x80" * 10 + b"\x01"),
    "length-past-the-span": _wrap(S(1) + b"\x2a\x7fab"),
    "attr-length-past-the-end": _wrap(S(1, b"\x4a\x05\x0a\x10ab")),
    "kind-as-fixed32": _wrap(S(1, f32(6, 2))),
    "start-as-varint": _wrap(S(1, varf(7, 5))),
    "field-0": _wrap(S(1) + b"\x00\x00"),
    "wire-type-6": _wrap(S(1) + b"\x8e\x01\x00"),
    "string-value-as-varint": _wrap(S(1, lenf(9, lenf(1, "k") + lenf(2, varf(1, 5))))),
    "message-cut-in-a-span": one_res([http(0), http(1)])[:-5],
    "record-length-past-the-end": b"\x0a\x7f" + lenf(1, SVC_A),
    "scope-spans-as-varint": lenf(1, lenf(1, SVC_A) + varf(2, 1)),
    "resource-spans-as-fixed64": f64(1, 7),
}


# ---------------------------------------------------------------------------
# census: the decoder's dispatch

def structure(pb: bytes) -> SimpleNamespace:
    """Where the parts of a well-formed message lie: records, Resource fields,
    scopes and spans as (payload start, payload length)."""
    s = SimpleNamespace(top=[], records=[], res_fields=[], schema_len=[], scopes=[], scope_res=[], scope_hdrs=[], spans=[],
                        span_scope=[])
    for f, wt, at, ps, pl in fields(pb):
        s.top.append((at, f, wt))
        if f != 1 or wt != 2:
            continue
        r = len(s.records)
        s.records.append((at, ps, pl))
        resf, sc2, sc1000, schema = [], [], [], 0
        for f2, w2, _, qs, ql in fields(pb, ps, ps + pl):
            if w2 != 2:
                continue
            if f2 == 1:
                resf.append((qs, ql))
            elif f2 == 2:
                sc2.append((qs, ql))
            elif f2 == 1000:
                sc1000.append((qs, ql))
            elif f2 == 3:
                schema = ql
        s.res_fields.append(resf)
        s.schema_len.append(schema)
        for qs, ql in (sc2 or sc1000):
            q = len(s.scopes)
            s.scopes.append((qs, ql))
            s.scope_res.append(r)
            hdrs = []
            for f3, w3, _, us, ul in fields(pb, qs, qs + ql):
                if f3 == 1 and w3 == 2:
                    hdrs.append((us, ul))
                elif f3 == 2 and w3 == 2:
                    s.spans.append((us, ul))
                    s.span_scope.append(q)
            s.scope_hdrs.append(hdrs)
    return s


def spans_of(pb: bytes) -> list:
    return structure(pb).spans


def _rounds(spans) -> list:
    """[(chunks, staged)] of otlp_span_lds_kernel's 64-span rounds"""
    out = []
    for r0 in range(0, len(spans), WAVE):
        part = spans[r0:r0 + WAVE]
        lo = min(s for s, _ in part) & ~15
        hi = max(s + n for s, n in part)
        nchunk = ((hi + 15) >> 4) - (lo >> 4) + 1
        out.append((nchunk, nchunk <= K.kSpanStage // 16))
    return out


def _kv_repeats(pb, s, n, attr_field) -> bool:
    """a KeyValue of message [s, s + n) with its key or its value field repeated"""
    for f, wt, _, ps, pl in fields(pb, s, s + n):
        if f == attr_field and wt == 2:
            cnt = {1: 0, 2: 0}
            for f2, w2, _, _, _ in fields(pb, ps, ps + pl):
                if f2 in cnt and w2 == 2:
                    cnt[f2] += 1
            if max(cnt.values()) > 1:
                return True
    return False


def _is_nested(v) -> bool:
    return "arrayValue" in v or "kvlistValue" in v


def span_reasons(sp: dict, pb: bytes, ref, hostk: set, sql: bool) -> list:
    """why the span decoder hands span `sp` (message bytes `ref`) to the host pass"""
    s, n = ref
    why = []
    merged = _kv_repeats(pb, s, n, 9)
    for f, wt, _, ps, pl in fields(pb, s, s + n):
        if wt == 2 and f in (11, 13):
            merged |= _kv_repeats(pb, ps, pl, 3 if f == 11 else 4)
    if merged:
        why.append("merged_kv")
    if any(_is_nested(kv["value"]) for kv in sp["attributes"]) or \
            any(_is_nested(kv["value"]) for x in sp["events"] + sp["links"] for kv in x["attributes"]):
        why.append("nested")
    first = {}
    for kv in sp["attributes"]:
        first.setdefault(kv["key"], kv["value"])
    is_str = lambda v: "stringValue" in v   # noqa: E731
    if set(first) & hostk:
        why.append("host_key")
    if "http.route" in first and not is_str(first["http.route"]):
        why.append("route")
    m = first.get("http.request.method", first.get("http.method"))
    if m is not None:
        if not is_str(m):
            why.append("method")
        if "url.path" in first:
            if not is_str(first["url.path"]):
                why.append("path")
        elif "http.target" in first:
            if not is_str(first["http.target"]):
                why.append("target")
        elif "url.full" in first or "http.url" in first:
            why.append("url_full")
    if sql and "db.query.text" in first and not is_str(first["db.query.text"]):
        why.append("query")
    return why


def restate_res_table(keys, table=None):
    """DevResTable::insert over `keys` (Resource bytes, row order) into `table`
    ({slot: key}); returns the table and, per key, whether a lookup finds it"""
    table = {} if table is None else table
    mask = K.kResSlots - 1

    def walk(key, insert):
        slot = fnv1a(key) & mask
        for _ in range(K.res_probes):
            if slot not in table:
                if insert:
                    table[slot] = key
                return insert
            if table[slot] == key:
                return True
            slot = (slot + 1) & mask
        return False
    for k in keys:
        walk(k, True)
    return table, [walk(k, False) for k in keys]


def buf_cap(nbytes: int) -> int:
    """DevBuf::need's capacity for a first request of nbytes"""
    want = max(nbytes + nbytes // K.buf_slack_div, K.buf_min)
    return -(-want // K.buf_round) * K.buf_round


def census(L: Layout, options=()) -> SimpleNamespace:
    """The decoder's dispatch for layout L on a fresh engine with `options` set."""
    pb, cfg = L.pb, L.cfg
    st = structure(pb)
    c = SimpleNamespace(structure=st, n_spans=len(st.spans), n_res=len(st.records), n_scopes=len(st.scopes))
    sql = SQL_SECTION in cfg
    tree_spans = L.tree_spans()
    assert len(tree_spans) == c.n_spans
    hk = host_keys(cfg)
    if L.big:   # the minimal spans carry nothing: only the special ones are looked at
        c.reasons = [[] for _ in range(c.n_spans)]
        for i in BIG_SPECIAL:
            if i < c.n_spans:
                c.reasons[i] = span_reasons(tree_spans[i], pb, st.spans[i], hk, sql)
    else:
        c.reasons = [span_reasons(sp, pb, ref, hk, sql) for sp, ref in zip(tree_spans, st.spans)]
    c.host = [bool(r) for r in c.reasons]
    c.host_spans = sum(c.host)
    # the span kernel and its rounds
    c.span_kernel = 0 if not c.n_spans else (1 if c.n_spans <= K.kSpanStageMax else 2)
    c.rounds = _rounds(st.spans) if c.span_kernel == 1 else []
    # the key table
    tab = key_table(cfg)
    c.n_keys, c.key_bytes = len(tab), sum(len(k) for k in tab)
    c.key_lds = c.n_keys <= K.kKeyLds and c.key_bytes <= K.kKeyBytesLds
    c.key_last = tab[-1]
    # resources: cold, then warm, on one engine
    gpu_res = "otlp_host_resources" not in options and "otlp_host_scopes" not in options
    rkeys, c.res_kind = [], []
    for resf in st.res_fields:
        keyed = len(resf) <= 1
        c.res_kind.append("keyed" if keyed else "unkeyed")
        if keyed:
            rkeys.append(bytes(pb[resf[0][0]:resf[0][0] + resf[0][1]]) if resf else b"")
    table, found = restate_res_table(rkeys)
    c.res_table = table
    c.cold = dict(res_misses=c.n_res, res_keyed=len(rkeys)) if gpu_res else dict(res_misses=0, res_keyed=0)
    warm_miss = (c.n_res - len(rkeys)) + found.count(False)
    c.warm = dict(res_misses=warm_miss, res_keyed=found.count(False)) if gpu_res else dict(res_misses=0, res_keyed=0)
    c.res_never = [k for k, f in zip(rkeys, found) if not f]
    c.sync_whole = len(table) > K.sync_whole
    # scopes
    c.scope_kind = []
    tree_scopes = [ss for rs in L.tree["resourceSpans"] for ss in rs["scopeSpans"]]
    assert len(tree_scopes) == c.n_scopes
    for q, (ps, pl) in enumerate(st.scopes):
        kind = "gpu"
        if len(st.scope_hdrs[q]) > 1:
            kind = "host_sized"
        elif st.scope_hdrs[q]:
            hs, hl = st.scope_hdrs[q][0]
            if _kv_repeats(pb, hs, hl, 3) or any(_is_nested(kv["value"]) for kv in tree_scopes[q]["scope"]["attributes"]):
                kind = "host_sized"
        c.scope_kind.append(kind)
    gpu_scopes = "otlp_host_scopes" not in options
    if not gpu_scopes:
        c.host_scopes = 0
    elif gpu_res:
        c.host_scopes = sum(k == "host_sized" for k in c.scope_kind)
    else:   # the host walked the scopes above kGpuScopeBytes; the GPU flags the others
        c.host_scopes = sum(k == "host_sized" and pl <= K.kGpuScopeBytes for k, (_, pl) in zip(c.scope_kind, st.scopes))
    c.scopes_on_host_walk = [pl > K.kGpuScopeBytes for _, pl in st.scopes] if (gpu_scopes and not gpu_res) else []
    # the chain
    c.chain = chain_census(pb, st) if "otlp_gpu_chain" in options and gpu_res else None
    # the arena: lower and upper bounds of what the host pass appends
    lo = hi = 0
    pk = plan_keys(cfg)
    for sp, h in zip(tree_spans, c.host) if not L.big else ():
        if not h:
            continue
        first = {}
        for kv in sp["attributes"]:
            first.setdefault(kv["key"], kv["value"])
        lo += sum(len(gg._b(first[k]["stringValue"])) for k in pk if k in first and "stringValue" in first[k])
        for k in ["http.route"] + (["db.query.text"] if sql else []):   # the route and the query are appended too
            if "stringValue" in first.get(k, {}):
                lo += len(gg._b(first[k]["stringValue"]))
        hi += 3 * sum(len(host.dumps(v)) + 64 for v in first.values())
    pb_cap = -(-(len(pb) + 16) // 16) * 16
    cap = buf_cap(pb_cap + max(K.fix_reserve_min, len(pb) // K.fix_reserve_div) + 16)
    c.arena_cap, c.appended_bounds = cap, (lo, hi)
    c.regrown = True if pb_cap + lo + 16 > cap else (False if pb_cap + hi + 16 <= cap else None)
    c.walk_info = lambda warm=False: dict(   # noqa: E731
        gpu_chain=int(bool(c.chain and c.chain.linked)), scope_redo=0, res_redo=0, span_kernel=c.span_kernel,
        host_scopes=c.host_scopes, arena_regrown=int(bool(c.regrown)), **(c.warm if warm else c.cold))
    return c


def _plausible(pb, q) -> bool:
    """chain_plausible: four `0A len {0A|12}...` records in a row from q (or the message end)"""
    n, pos = len(pb), q
    for _ in range(4):
        if pos >= n:
            break
        try:
            t, i = _rd_varint(pb, pos)
            if t != 0x0A:
                return False
            ln, i = _rd_varint(pb, i)
        except IndexError:
            return False
        if ln == 0 or ln > n - i or pb[i] not in (0x0A, 0x12):
            return False
        pos = i + ln
    return True


def chain_census(pb: bytes, st) -> SimpleNamespace:
    """otlp_chain_seg_kernel and res_walk_gpu's link, restated: per segment the
    speculated start, the field starts listed from it, where the true chain
    enters and how many starts are listed before that; whether every link holds."""
    n = len(pb)
    T = -(-n // K.kChainSeg)
    true_starts = [at for at, _, _ in st.top]
    true_end = {}
    for k, (at, f, wt) in enumerate(st.top):
        true_end[at] = st.top[k + 1][0] if k + 1 < len(st.top) else n
    ch = SimpleNamespace(n_seg=T, start=[], listed=[], bad=[], end=[], enters={}, listed_before={}, covered=[], linked=True)
    for t in range(T):
        s0, s1 = t * K.kChainSeg, min(n, (t + 1) * K.kChainSeg)
        c0 = 0 if t == 0 else next((q for q in range(s0, s1) if pb[q] == 0x0A and _plausible(pb, q)), None)
        ch.start.append(c0)
        lst, bad, i = [], False, c0
        while c0 is not None and i < s1 and i < n:
            at = i
            try:
                tg, i = _rd_varint(pb, i)
                f, wt = tg >> 3, tg & 7
                if f == 0 or f > 0x1FFFFFFF or wt in (3, 4, 6, 7) or (f == 1 and wt != 2):
                    bad = True
                    break
                lst.append(at)
                if wt == 0:
                    _, i = _rd_varint(pb, i)
                elif wt == 2:
                    ln, i = _rd_varint(pb, i)
                    if ln > n - i:
                        bad = True
                        break
                    i += ln
                else:
                    i += 8 if wt == 1 else 4
                    if i > n:
                        bad = True
                        break
            except IndexError:
                bad = True
                break
        ch.listed.append(lst)
        ch.bad.append(bad)
        ch.end.append(i)
    pos = 0
    for t in range(T):
        s1 = min(n, (t + 1) * K.kChainSeg)
        if pos >= s1:
            ch.covered.append(t)
            continue
        ch.enters[t] = pos
        lst = ch.listed[t][:K.kChainList]
        if ch.start[t] is None or pos not in lst or ch.bad[t]:
            ch.linked = False
            break
        ch.listed_before[t] = lst.index(pos)
        # from the entry on the segment's walk is the true chain
        while pos < s1:
            pos = true_end[pos]
    if ch.linked and pos != n:
        ch.linked = False
    assert all(p in true_starts for p in ch.enters.values())
    return ch
