"""odigosconditionalattributes as the CONDATTR stage.

CPU: the Python restatement (tests/condattr_ref.py) against the golden cases
(tests/golden/condattr_kats.json: the README's three trace examples and a
hand-derived table), the shipped category-attributes profile
(tests/golden/category_attributes_profile.json), the host seam
(osehost_condattr_span, the source the kernels compile) against the
restatement on seeded batches, config type errors, the columns the host walk
fills, the ctypes mirrors against the header, and what the adversarial batch
covers.

GPU: src / val / span_size_out against the restatement through
ose_condattr_process and ose_condattr_process_device, the sizes, the
adversarial batch, the profile, the size stage after CONDATTR against the
marshalled size of the restatement-mutated tree, the drop-in processor and
pipeline, the refusals and a hipGraph capture.

ose_engine_create needs a device, so the CPU tests compile configs through
osehost_condattr_compile (the function ose_engine_create calls) and the
engine's own answers are checked in the GPU tests.
"""
import ctypes as C
import functools
import json
import random
import re
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import host, native
from odigos_amd.batch import CondAttrHostBatch
from tests import condattr_ref as ref
from tests import otlp_gogo as gg

GOLD = Path(__file__).parent / "golden"
KATS = json.loads((GOLD / "condattr_kats.json").read_text())
SECTION = ref.SECTION
SCOPE = ref.OTTL_SCOPE_NAME_KEY
TRAFFIC = {"res_attributes_keys": ["service.name", "k8s.namespace.name"]}


def profile_config() -> dict:
    p = json.loads((GOLD / "category_attributes_profile.json").read_text())
    rules = [{"field_to_check": r["field_to_check"],
              "new_attribute_value_configurations": {v: r["action_lists"][k] for v, k in r["values"].items()}}
             for r in p["rules"]]
    return {"global_default": p["global_default"], "rules": rules}


def _attrs(pairs) -> list:
    return [{"key": k, "value": host.attr_value(v)} for k, v in pairs]


def kat_tree(case) -> dict:
    sp = host.span(name="s")
    sp["attributes"] = _attrs(case["span"])
    return {"resourceSpans": [{"resource": {"attributes": _attrs(case.get("resource", []))},
                               "scopeSpans": [{"scope": {"name": case.get("scope_name", ""),
                                                         "attributes": _attrs(case.get("scope", []))}, "spans": [sp]}]}]}


def kat_cases():
    r = KATS["readme_examples"]
    assert "README.md" in r["source"]
    out = [(r["config"], c) for c in r["cases"]]
    assert KATS["derived_cases"]["derived"] is True
    out += [(c["config"], c) for c in KATS["derived_cases"]["cases"]]
    return out


def kat_expected(case, td):
    n0 = len(case["span"])
    e = _attrs(case["expected"])
    return [(e[:n0], sorted(e[n0:], key=lambda kv: kv["key"].encode()))]


# ---------------------------------------------------------------------------
# the compiled config (no device) and the columns, built independently in numpy

def compile_info(cfg):
    """(rc, CondAttrInfo, [(key bytes, target or None)], string table) of osehost_condattr_compile."""
    L = native.lib()
    info, p = native.CondAttrInfo(), C.c_void_p()
    rc = L.osehost_condattr_compile(host.dumps({SECTION: cfg}).encode(), C.byref(info), C.byref(p))
    if rc:
        return rc, None, None, None
    j = json.loads(native.take_bytes(p.value).decode())
    keys = [(bytes.fromhex(k), None if t == native.OSE_NONE else t) for k, t in zip(j["keys"], j["key_target"])]
    return 0, info, keys, bytes.fromhex(j["strings"])


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


class Batch:
    """ose_condattr_columns of a tree, for the keys of ref.keys(cfg).  align:
    string k starts at arena offset = k mod 16; the arena ends with the last
    string's last byte."""

    def __init__(self, cfg, td, align=False, sized=True):
        self.cfg, self.td = cfg, td
        keys, self.targets = ref.keys(cfg), ref.targets(cfg)
        K = len(keys)
        res = td["resourceSpans"]
        scopes = [(ri, ss) for ri, rs in enumerate(res) for ss in rs["scopeSpans"]]
        spans = [(si, sp) for si, (_, ss) in enumerate(scopes) for sp in ss["spans"]]
        n, S, R = len(spans), len(scopes), len(res)
        buf, cnt = bytearray(), [0]

        def add(b: bytes):
            if align:
                buf.extend(bytes((cnt[0] % 16 - len(buf) % 16) % 16))
                cnt[0] += 1
            off = len(buf)
            buf.extend(b)
            return off, len(b)
        z = lambda rows, m, dt: np.zeros(max(1, rows * m) if dt != "ref" else (max(1, rows * m), 2),
                                         dtype=np.uint32 if dt == "ref" else dt)
        a = {"scope": z(1, n, np.uint32), "scope_resource": z(1, S, np.uint32), "scope_name": z(1, S, "ref"),
             "span_has": z(K, n, np.uint8), "span_val": z(K, n, "ref"), "span_kv_size": z(K, n, np.uint32),
             "scope_has": z(K, S, np.uint8), "scope_val": z(K, S, "ref"), "res_has": z(K, R, np.uint8),
             "res_val": z(K, R, "ref"), "span_size": z(1, n, np.uint32)}

        def fill(attrs, has, val, row, m, kv_size=None):
            for k, key in enumerate(keys):
                kv = ref._get(attrs, key)
                if kv is not None:
                    has[k * m + row] = 1
                    val[k * m + row] = add(_b(ref.as_string(kv["value"])))
                    if kv_size is not None:
                        kv_size[k * m + row] = len(gg._len(9, gg.key_value(kv)))
        for ri, rs in enumerate(res):
            fill((rs.get("resource") or {}).get("attributes") or [], a["res_has"], a["res_val"], ri, R)
        for si, (ri, ss) in enumerate(scopes):
            sc = ss.get("scope") or {}
            a["scope_resource"][si] = ri
            a["scope_name"][si] = add(_b(sc.get("name", "") or ""))
            fill(sc.get("attributes") or [], a["scope_has"], a["scope_val"], si, S)
        for i, (si, sp) in enumerate(spans):
            a["scope"][i] = si
            a["span_size"][i] = len(gg.span(sp))
            fill(sp.get("attributes") or [], a["span_has"], a["span_val"], i, n, a["span_kv_size"])
        self.arena_bytes = len(buf)
        arena = np.zeros((len(buf) + 15) // 16 * 16 + 16, dtype=np.uint8)
        arena[:len(buf)] = np.frombuffer(bytes(buf), dtype=np.uint8)
        a["arena"] = arena
        self.n, self.S, self.R, self.K, self.keys = n, S, R, K, keys
        self.arena = bytes(buf)
        self.hb = CondAttrHostBatch(n, R, S, len(buf), a, len(self.targets), sized)
        self.spans = [sp for _, sp in spans]

    def want(self):
        """Per span (puts, events, mutated span) of the restatement."""
        detail = []
        tree = ref.process_traces(self.cfg, self.td, detail)
        after = [sp for rs in tree["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]
        return [(p, e, sp) for (p, e), sp in zip(detail, after)]

    def check(self, src, val, size_out, strings, want=None):
        want = want if want is not None else self.want()
        n = self.n
        for u, name in enumerate(self.targets):
            for i in range(n):
                s = int(src[u * n + i])
                off, ln = (int(x) for x in val[u * n + i])
                got = None if s == native.CA_KEEP else (strings if s == native.CA_CONFIG else self.arena)[off:off + ln]
                assert s in (native.CA_KEEP, native.CA_ARENA, native.CA_CONFIG), (u, i, s)
                w = want[i][0].get(name)
                assert got == (None if w is None else _b(w)), (name, i, got, w, want[i][1])
        if size_out is not None:
            np.testing.assert_array_equal(size_out[:n], np.array([len(gg.span(w[2])) for w in want], dtype=np.uint32))


def run_seam(b: Batch):
    L = native.lib()
    rc = L.osehost_condattr_span(host.dumps({SECTION: b.cfg}).encode(), C.byref(b.hb.cols), C.byref(b.hb.outs))
    assert rc == 0, native.last_error()
    return b.hb.src, b.hb.val, b.hb.span_size_out


def strings_of(cfg) -> bytes:
    rc, _, _, strings = compile_info(cfg)
    assert rc == 0, native.last_error()
    return strings


# ---------------------------------------------------------------------------
# the adversarial config and trees (seeded)

EDGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33]
LONG = "Z" * 69_999 + "!"
TARGETS = ["t%d" % k for k in range(16)] + [""]
FROMS = ["f%d" % k for k in range(20)]


@functools.lru_cache(maxsize=None)
def adv_config() -> dict:
    rng = random.Random(0xCA77)
    t, f = TARGETS, FROMS
    nf = [0]

    def rand_list(lo):
        out = []
        for _ in range(rng.randrange(1, 4)):
            name = rng.choice(t[lo:])
            if rng.random() < 0.5:
                out.append({"new_attribute": name, "value": "val-%d" % rng.randrange(40)})
            else:
                out.append({"new_attribute": name, "from_field": f[nf[0] % len(f)]})
                nf[0] += 1
        return out
    pool = [rand_list(3) for _ in range(40)]
    big = {"v%04d" % k: pool[k % len(pool)] for k in range(5000)}
    for ln in EDGE_LENS:
        big["L" * ln] = [{"new_attribute": "t3", "value": "len-%d" % ln}]
    big[LONG] = [{"new_attribute": "t3", "value": "long"}]
    big.update({"ab": [{"new_attribute": "t4", "value": "ab"}], "abc": [{"new_attribute": "t4", "value": "abc"}],
                "abcd": [{"new_attribute": "t4", "from_field": "f0"}],
                "same-prefix-x": [{"new_attribute": "t5", "value": "x"}], "same-prefix-y": [{"new_attribute": "t5", "value": "y"}],
                "0123456789abcdef-A": [{"new_attribute": "t5", "value": "A"}],
                "0123456789abcdef-B": [{"new_attribute": "t5", "value": "B"}],
                "42": [{"new_attribute": "t6", "value": "int"}, {"new_attribute": "", "value": "nameless"}],
                "true": [{"new_attribute": "t6", "from_field": "k1"}]})
    rules = [
        {"field_to_check": SCOPE, "new_attribute_value_configurations": {
            **{"lib.%d" % k: [{"new_attribute": "t0", "value": "cat-%d" % (k % 5)}, {"new_attribute": "t1", "from_field": "f0"},
                              {"new_attribute": "t1", "from_field": "f1"}, {"new_attribute": "t2", "value": "web"}]
               for k in range(30)},
            "lib": [{"new_attribute": "t0", "value": "prefix"}], "": [{"new_attribute": "t2", "value": "unnamed"}]}},
        {"field_to_check": "k1", "field_to_check_metrics": "ignored", "new_attribute_value_configurations": big},
        {"field_to_check": "k2", "new_attribute_value_configurations": {
            "s1": [{"new_attribute": "t7", "value": "scope-1"}], "r1": [{"new_attribute": "t7", "value": "res-1"}],
            "": [{"new_attribute": "t8", "value": "no-k2"}], "p1": [{"new_attribute": "t7", "from_field": "f2"}]}},
        {"field_to_check": "t3", "new_attribute_value_configurations": {
            "long": [{"new_attribute": "t9", "value": "chained-long"}], "len-16": [{"new_attribute": "t9", "from_field": "t3"}]}},
        {"field_to_check": "k4", "new_attribute_value_configurations": {
            "on": [{"new_attribute": "t10", "value": "over"}, {"new_attribute": "t11", "from_field": "f3"},
                   {"new_attribute": "t12", "value": "V", "from_field": "f4"}, {"new_attribute": "t13"}]}},
        {"field_to_check": SCOPE, "new_attribute_value_configurations": {
            "lib.1": [{"new_attribute": "t10", "value": "scope-rule"}, {"new_attribute": "t14", "from_field": "t0"},
                      {"new_attribute": "t15", "value": "fifteen"}]}},
    ]
    return {"global_default": "Unknown", "rules": rules}


def adv_tree(seed: int, n_spans: int, R: int, S: int) -> dict:
    rng = random.Random(seed)
    cfg = adv_config()
    big = list(cfg["rules"][1]["new_attribute_value_configurations"])
    special = [v for v in big if not v.startswith("v0") and not v.startswith("v1") and not v.startswith("v2")
               and not v.startswith("v3") and not v.startswith("v4") and v != LONG]
    typed = lambda: rng.choice(["s", 7, True, 2.5, "", "x" * rng.choice([1, 120, 127, 128])])
    res = []
    for r in range(R):
        at = {}
        if r != 1:   # resource 1 is empty
            at["service.name"] = "svc-%02d" % r
            at["k8s.namespace.name"] = "ns%d" % (r % 3)
            if rng.random() < 0.4:
                at["k2"] = rng.choice(["r1", "zz", 5])
            if rng.random() < 0.3:
                at["k1"] = rng.choice(["v0007", "ab", "nope"])
            for name in ("t10", "t11", "t4", "t0"):
                if rng.random() < 0.5:
                    at[name] = typed()
        res.append({"resource": {"attributes": host.attrs(at)}, "scopeSpans": []})
    for s in range(S):
        x = rng.random()
        name = ("lib.%d" % rng.randrange(34)) if x < 0.6 else rng.choice(["", "lib", "lib.", "other", "lib.1x"])
        at = {}
        if s % 7 != 3:   # some scopes are empty
            if rng.random() < 0.4:
                at["k2"] = rng.choice(["s1", "p1", "zz", ""])
            for tn in ("t10", "t11", "t4", "t0"):
                if rng.random() < 0.5:
                    at[tn] = typed()
        else:
            name = ""
        res[s % R if s < R else rng.randrange(R)]["scopeSpans"].append({"scope": {"name": name, "attributes": host.attrs(at)},
                                                                        "spans": []})
    scopes = [ss for rs in res for ss in rs["scopeSpans"]]
    for i in range(n_spans):
        at = {}
        x = rng.random()
        if x < 0.35:
            at["k1"] = rng.choice(special)
        elif x < 0.55:
            at["k1"] = "v%04d" % rng.randrange(5000)
        elif x < 0.70:
            v = rng.choice(special + ["v0001"])
            at["k1"] = rng.choice([v + "x", v[:-1], "V" + v[1:], 42, True, 43])
        if rng.random() < 0.08:
            at["k2"] = rng.choice(["s1", "p1", "", "q"])
        if rng.random() < 0.5:
            at["k4"] = rng.choice(["on", "on", "off"])
        for fn in rng.sample(FROMS, rng.randrange(0, 6)):
            at[fn] = typed()
        for tn in ("t10", "t11", "t4", "t0", "t3", "t13"):
            if rng.random() < 0.25:
                at[tn] = typed()
        sp = host.span(name="n" * rng.choice([0, 3, 40]), kind=1 + i % 5, trace_id="%032x" % (1 + i), span_id="%016x" % (1 + i),
                       start=1739000000000000000 + i, end=1739000001000000000, attributes=at)
        scopes[rng.randrange(len(scopes))]["spans"].append(sp)
    return {"resourceSpans": res}


@functools.lru_cache(maxsize=None)
def adversarial():
    """(Batch, want) of the GPU batch: 4,099 spans, 37 resources, 150 scopes;
    one span carries the 70,000-byte value, one a near miss of it, and the
    last span's k1 value ends on the arena's last byte."""
    td = adv_tree(0xADE5, 4097, 37, 150)
    last = td["resourceSpans"][-1]["scopeSpans"][-1]["spans"]
    last.append(host.span(name="long", attributes={"k1": LONG}))
    last.append(host.span(name="miss", attributes={"k1": LONG[:-1] + "?"}))
    last.append(host.span(name="end", attributes={"f0": "m", "k1": "abcd"}))
    td["resourceSpans"][0]["scopeSpans"][0]["spans"] = td["resourceSpans"][0]["scopeSpans"][0]["spans"][1:]
    b = Batch(adv_config(), td, align=True)
    return b, b.want()


OUTCOMES = ("KEEP", "static", "copied", "default", "overwrite")


def outcome_table(b: Batch, want):
    per_target = {t: {} for t in b.targets}
    events = {}
    for (puts, ev, _), sp in zip(want, b.spans):
        last = {}
        for e in ev:
            if isinstance(e, tuple):
                events[e[0]] = events.get(e[0], 0) + 1
                if e[0] in OUTCOMES:
                    last[e[1]] = e[0]
            else:
                events[e] = events.get(e, 0) + 1
        for t in b.targets:
            o = last.get(t, "KEEP")
            per_target[t][o] = per_target[t].get(o, 0) + 1
            events["KEEP"] = events.get("KEEP", 0) + (o == "KEEP")
    return per_target, events


# ---------------------------------------------------------------------------
# CPU

def test_restatement_matches_golden():
    cases = kat_cases()
    assert len(cases) >= 40
    for cfg, c in cases:
        td = kat_tree(c)
        assert ref.canon(ref.process_traces(cfg, td), td) == kat_expected(c, td), c["name"]


def test_host_seam_matches_golden():
    for cfg, c in kat_cases():
        b = Batch(cfg, kat_tree(c))
        b.check(*run_seam(b), strings_of(cfg))


def test_key_and_target_numbering():
    for cfg in (adv_config(), profile_config(), KATS["readme_examples"]["config"]):
        rc, info, keys, _ = compile_info(cfg)
        assert rc == 0
        assert [k for k, _ in keys] == [_b(k) for k in ref.keys(cfg)]
        tg = ref.targets(cfg)
        assert [t for _, t in keys] == [tg.index(k) if k in tg else None for k in ref.keys(cfg)]
        assert (info.n_rules, info.n_keys, info.n_targets) == (len(cfg["rules"]), len(keys), len(tg))
    rc, info, keys, _ = compile_info(adv_config())
    assert (info.n_keys, info.n_targets) == (40, 17)


def test_shipped_profile():
    p = json.loads((GOLD / "category_attributes_profile.json").read_text())
    assert p["type"] == SECTION and p["signals"] == ["TRACES"] and p["collectorRoles"] == ["NODE_COLLECTOR"]
    cfg = profile_config()
    assert len(cfg["rules"]) == 1 and cfg["rules"][0]["field_to_check"] == SCOPE and cfg["global_default"] == "Unknown"
    assert len(cfg["rules"][0]["new_attribute_value_configurations"]) == 269
    rc, info, keys, _ = compile_info(cfg)
    assert rc == 0 and info.n_targets == 3 and info.n_rules == 1
    assert ref.targets(cfg) == ["odigos.category", "odigos.sub_category", "odigos.transaction.type"]
    host.Processor(SECTION, cfg).close()
    host.Processor("pipeline", {SECTION: cfg, "odigostrafficmetrics": TRAFFIC}).close()


def test_host_seam_matches_restatement_random():
    td = adv_tree(0x5EA7, 20_000, 61, 400)
    b = Batch(adv_config(), td, align=True)
    assert b.n == 20_000
    b.check(*run_seam(b), strings_of(adv_config()))


def test_adversarial_batch_covers_the_ground():
    b, want = adversarial()
    assert (b.n, b.R, b.S) == (4099, 37, 150) and b.K == 40 and len(b.targets) == 17
    per_target, ev = outcome_table(b, want)
    for name in ("KEEP", "static", "copied", "default", "overwrite", "suppressed", "hit_scope_name", "hit_span", "hit_scope",
                 "hit_resource", "empty_match"):
        assert ev.get(name, 0) >= 50, (name, ev)
    for t, outs in per_target.items():
        assert len(outs) >= 2, (t, outs)
    # the layout: all 16 alignments, the lengths, the arena's last byte, empties
    val, has = b.hb.arrays["span_val"], b.hb.arrays["span_has"]
    k1 = b.keys.index("k1")
    refs = [tuple(int(x) for x in val[k1 * b.n + i]) for i in range(b.n) if has[k1 * b.n + i]]
    assert {o % 16 for o, _ in refs} == set(range(16))
    assert set(EDGE_LENS + [70_000]) <= {ln for _, ln in refs}
    assert any(o + ln == b.arena_bytes for o, ln in refs)
    res = b.td["resourceSpans"]
    assert any(not rs["resource"]["attributes"] for rs in res)
    assert sum(1 for rs in res for ss in rs["scopeSpans"] if not ss["scope"]["name"] and not ss["scope"]["attributes"]) >= 5


def test_config_type_errors():
    ok = ({}, None, {"rules": None}, {"rules": []}, {"global_default": "x", "rules": [{}]},
          {"rules": [{"field_to_check": "a", "field_to_check_metrics": "m", "new_attribute_value_configurations": None}]},
          {"rules": [{"new_attribute_value_configurations": {"v": None, "w": [], "x": [{}], "y": [{"new_attribute": "t"}]}}]})
    for cfg in ok:
        host.Processor(SECTION, cfg).close()
        assert compile_info(cfg)[0] == 0
    bad = (([], "expected a map"), ("x", "expected a map"), ({"global_default": 1}, "expected type 'string'"),
           ({"rules": {}}, "must be an array or slice"), ({"rules": [1]}, "expected a map"),
           ({"rules": [{"field_to_check": 1}]}, "expected type 'string'"),
           ({"rules": [{"field_to_check_metrics": []}]}, "expected type 'string'"),
           ({"rules": [{"new_attribute_value_configurations": []}]}, "expected a map"),
           ({"rules": [{"new_attribute_value_configurations": {"v": {}}}]}, "must be an array or slice"),
           ({"rules": [{"new_attribute_value_configurations": {"v": ["a"]}}]}, "expected a map"),
           ({"rules": [{"new_attribute_value_configurations": {"v": [{"value": 1}]}}]}, "expected type 'string'"),
           ({"rules": [{"new_attribute_value_configurations": {"v": [{"from_field": True}]}}]}, "expected type 'string'"),
           ({"rules": [{"new_attribute_value_configurations": {"v": [{"new_attribute": 2.5}]}}]}, "expected type 'string'"))
    for cfg, msg in bad:
        if cfg:   # (Processor reads a falsy config as {})
            with pytest.raises(ValueError, match=msg):
                host.Processor(SECTION, cfg)
        with pytest.raises(ValueError, match=msg):
            host.Processor("pipeline", {SECTION: cfg, "odigostrafficmetrics": {}})
        # ose_engine_create refuses them before touching a device
        h = C.c_void_p()
        assert native.lib().ose_engine_create(host.dumps({SECTION: cfg}).encode(), C.byref(h)) == native.OSE_EINVAL
        assert re.search(msg, native.last_error())


def test_pipeline_takes_traffic_metrics_only():
    cfg = KATS["readme_examples"]["config"]
    for other in ("odigossampling", "odigosurltemplate", "odigossqldboperationprocessor"):
        with pytest.raises(ValueError, match="OSE_ENOTSUP"):
            host.Processor("pipeline", {SECTION: cfg, other: {}, "odigostrafficmetrics": {}})


def test_columnarize_columns():
    cfg = {"global_default": "d", "rules": [{"field_to_check": "k", "new_attribute_value_configurations": {
        "v": [{"new_attribute": "t", "from_field": "f"}]}}]}
    m = {"kvlistValue": {"values": [{"key": "a", "value": {"stringValue": "b"}}]}}
    td = host.traces(
        host.resource_spans({"k": 5, "t": "r"}, scopes=[
            {"scope": {"name": "lib", "attributes": host.attrs({"f": True})},
             "spans": [host.span(name="a", attributes={"k": "v", "f": m, "x": 1}), host.span(name="b", attributes={"t": 7})]},
            {"scope": {}, "spans": []}]),
        host.resource_spans({}, [host.span(name="c", attributes={"k": ""})]))
    p = host.Processor(SECTION, cfg)
    hb = p.columnarize(td)
    c = hb.condattr_cols
    assert (c.n_spans, c.n_scopes, c.n_resources) == (3, 3, 2)
    arena = bytes((C.c_uint8 * c.arena_bytes).from_address(c.arena))
    arr = lambda ptr, dt, cnt: np.ctypeslib.as_array((dt * cnt).from_address(ptr)).copy()
    keys = ref.keys(cfg)
    assert keys == ["k", "f", "t"]

    def col(has_p, val_p, m_):
        has = arr(has_p, C.c_uint8, 3 * m_)
        val = arr(val_p, C.c_uint32, 6 * m_).reshape(-1, 2)
        return [[arena[val[k * m_ + j][0]:val[k * m_ + j][0] + val[k * m_ + j][1]] if has[k * m_ + j] else None
                 for j in range(m_)] for k in range(3)]
    assert col(c.span_has, c.span_val, 3) == [[b"v", None, b""], [host.as_string(m).encode(), None, None], [None, b"7", None]]
    assert col(c.scope_has, c.scope_val, 3) == [[None] * 3, [b"true", None, None], [None] * 3]
    assert col(c.res_has, c.res_val, 2) == [[b"5", None], [None, None], [b"r", None]]
    assert list(arr(c.scope, C.c_uint32, 3)) == [0, 0, 2] and list(arr(c.scope_resource, C.c_uint32, 3)) == [0, 0, 1]
    names = arr(c.scope_name, C.c_uint32, 6).reshape(3, 2)
    assert [arena[o:o + ln] for o, ln in names] == [b"lib", b"", b""]
    kv = arr(c.span_kv_size, C.c_uint32, 9)
    sp_b = td["resourceSpans"][0]["scopeSpans"][0]["spans"][1]
    assert kv[2 * 3 + 1] == len(gg._len(9, gg.key_value(sp_b["attributes"][0])))
    assert list(arr(c.span_size, C.c_uint32, 3)) == [len(gg.span(sp)) for rs in td["resourceSpans"] for ss in rs["scopeSpans"]
                                                     for sp in ss["spans"]]
    # a processor without the section has no such columns
    assert host.Processor("odigostrafficmetrics", {}).columnarize(td).condattr_cols is None


def _header_struct(name):
    hdr = (Path(__file__).parent.parent / "include" / "odigos_amd.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t.strip(), f) for t, f in re.findall(r"([\w\s\*]+?)\b(\w+);", body)]


def test_struct_mirrors_match_the_header():
    hdr = (Path(__file__).parent.parent / "include" / "odigos_amd.h").read_text()
    assert "#define OSE_ABI_VERSION 5" in hdr and "#define OSE_STAGE_CONDATTR     0x100u" in hdr
    assert native.STAGE_CONDATTR == 0x100
    for k, name in enumerate(("OSE_CA_KEEP", "OSE_CA_ARENA", "OSE_CA_CONFIG")):
        assert re.search(r"#define %s\s+%d\b" % (name, k), hdr)
    for cname, mirror in (("ose_condattr_columns", native.CondAttrColumns), ("ose_condattr_outputs", native.CondAttrOutputs),
                          ("ose_condattr_info", native.CondAttrInfo)):
        fields = _header_struct(cname)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_]
        off = 0
        for (ctype, f), (_, py) in zip(fields, mirror._fields_):
            size = 8 if "*" in ctype or "uint64_t" in ctype else 4
            off = (off + size - 1) // size * size
            assert getattr(mirror, f).offset == off and C.sizeof(py) == size, (cname, f)
            off += size
        assert C.sizeof(mirror) == (off + 7) // 8 * 8 or C.sizeof(mirror) == off
    # the existing structs keep their sizes
    assert C.sizeof(native.Columns) == 264 and C.sizeof(native.Outputs) == 128
    for sym in ("ose_engine_condattr_info", "ose_engine_condattr_key", "ose_engine_condattr_string", "ose_condattr_scratch_words",
                "ose_condattr_process", "ose_condattr_process_device"):
        assert sym in native.exported_symbols() and hasattr(native.lib(), sym)


def _size_tree():
    """Spans whose message crosses 127/128 and 16383/16384 bytes through the
    additions, a value whose length crosses 127/128, an "" key, a replaced int."""
    cfg = {"global_default": "Unknown", "rules": [
        {"field_to_check": SCOPE, "new_attribute_value_configurations": {
            "lib": [{"new_attribute": "cat", "value": "HTTP"}, {"new_attribute": "sub", "from_field": "m"}]}},
        {"field_to_check": "k", "new_attribute_value_configurations": {
            "e": [{"new_attribute": "", "value": "nameless"}], "r": [{"new_attribute": "n", "value": "was-int"}]}}]}
    spans = []
    for k, ln in enumerate(list(range(60, 128, 3)) + list(range(16290, 16384, 4))):
        spans.append(host.span(name="n" * ln, kind=2, trace_id="%032x" % (k + 1), span_id="%016x" % (k + 1),
                               start=1739000000000000000, end=1739000001000000000))
    for ln in (120, 126, 127, 128, 129):
        spans.append(host.span(name="v", attributes={"m": "M" * ln}))
    spans.append(host.span(name="e", attributes={"k": "e"}))
    spans.append(host.span(name="r", attributes={"k": "r", "n": 123456789}))
    spans.append(host.span(name="keep", attributes={"cat": 1, "sub": 2}))
    a = len(spans) // 2
    td = host.traces(
        host.resource_spans({"service.name": "svc-a", "k8s.namespace.name": "ns0"},
                            scopes=[{"scope": {"name": "lib"}, "spans": spans[:a]}, {"scope": {"name": "zzz"}, "spans": []}]),
        host.resource_spans({"service.name": "svc-b", "k8s.namespace.name": "ns1", "n": "res"},
                            scopes=[{"scope": {"name": "other"}, "spans": spans[a::2]}, {"scope": {"name": "lib"}, "spans": spans[a + 1::2]}]))
    return cfg, td


def test_size_tree_covers_the_edges():
    cfg, td = _size_tree()
    b = Batch(cfg, td)
    want = b.want()
    grown = [(len(gg.span(sp)), len(gg.span(w[2]))) for sp, w in zip(b.spans, want)]
    assert any(x <= 127 < y for x, y in grown) and any(x <= 16383 < y for x, y in grown)
    subs = [len(w[0]["sub"]) for w in want if "sub" in w[0]]
    assert any(x <= 127 for x in subs) and any(x >= 128 for x in subs)
    assert any("" in w[0] for w in want)
    assert any(w[0].get("n") == "was-int" and ref._get(sp["attributes"], "n")["value"] == {"intValue": "123456789"}
               for sp, w in zip(b.spans, want))
    b.check(*run_seam(b), strings_of(cfg), want)


# ---------------------------------------------------------------------------
# GPU

def run_pinned(eng, b: Batch):
    b.hb.src.fill(0xEE)
    eng.condattr_process(b.hb)
    return b.hb.src.copy(), b.hb.val.copy(), b.hb.span_size_out.copy()


def run_device(eng, b: Batch):
    import torch
    from odigos_amd.batch import CondAttrDeviceBatch
    db = CondAttrDeviceBatch(eng, b.hb)
    eng.condattr_process_device(db, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not db.o["device_status"].any()
    return db.results()


def _engine(cfg, **more):
    from odigos_amd.batch import Engine
    return Engine({SECTION: cfg, **more})


@pytest.mark.gpu
def test_gpu_golden_cases():
    for cfg, c in kat_cases():
        eng = _engine(cfg)
        assert eng.info().stages == native.STAGE_CONDATTR
        b = Batch(cfg, kat_tree(c))
        strings = eng.condattr_strings()
        assert strings == strings_of(cfg)
        want = b.want()
        b.check(*run_pinned(eng, b), strings, want)
        b.check(*run_device(eng, b), strings, want)
        eng.close()


@pytest.mark.gpu
def test_gpu_engine_queries():
    cfg = profile_config()
    eng = _engine(cfg)
    info = eng.condattr_info()
    assert (info.n_rules, info.n_targets) == (1, 3)
    assert eng.condattr_keys() == compile_info(cfg)[2]
    assert [k for k, t in eng.condattr_keys() if t is not None] == [b"odigos.category", b"odigos.sub_category",
                                                                    b"odigos.transaction.type"]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_gpu_sizes(n):
    cfg = adv_config()
    eng = _engine(cfg)
    b = Batch(cfg, adv_tree(0x51 + n, n, 3, 5), align=True)
    assert b.n == n
    want = b.want()
    strings = eng.condattr_strings()
    b.check(*run_pinned(eng, b), strings, want)
    b.check(*run_device(eng, b), strings, want)
    eng.close()


@pytest.mark.gpu
def test_gpu_adversarial_batch():
    b, want = adversarial()
    eng = _engine(b.cfg)
    strings = eng.condattr_strings()
    b.check(*run_device(eng, b), strings, want)
    b.check(*run_pinned(eng, b), strings, want)
    eng.close()


@pytest.mark.gpu
def test_gpu_shipped_profile():
    cfg = profile_config()
    names = list(cfg["rules"][0]["new_attribute_value_configurations"])
    rng = random.Random(0xCA7E)
    scopes = []
    for s in range(80):
        nm = rng.choice(names) if s % 4 else rng.choice(["", "unknown.library", names[s % len(names)] + "x", names[3][:-1]])
        scopes.append({"scope": {"name": nm}, "spans": []})
    for i in range(2000):
        at = {}
        if rng.random() < 0.5:
            at[rng.choice(["http.request.method", "http.method"])] = rng.choice(["GET", "POST", 7])
        if rng.random() < 0.1:
            at["odigos.category"] = "mine"
        rng.choice(scopes)["spans"].append(host.span(name="s%d" % i, attributes=at))
    td = host.traces(host.resource_spans({"service.name": "a"}, scopes=scopes[:50]),
                     host.resource_spans({"service.name": "b"}, scopes=scopes[50:]))
    b = Batch(cfg, td)
    want = b.want()
    hits = sum(1 for w in want if "hit_scope_name" in w[1])
    assert 1000 < hits < 2000
    eng = _engine(cfg)
    b.check(*run_device(eng, b), eng.condattr_strings(), want)
    b.check(*run_pinned(eng, b), eng.condattr_strings(), want)
    eng.close()


def _counters(db, hb):
    R, A = hb.cols.n_resources, hb.cols.n_attrsets
    return (db.out_numpy("res_bytes", np.uint64, n=R), db.out_numpy("attrset_bytes", np.int64, n=A),
            int(db.out_numpy("accepted_spans", np.int64)[0]))


@pytest.mark.gpu
def test_gpu_size_after_condattr():
    import torch
    from odigos_amd.batch import CondAttrDeviceBatch, DeviceBatch
    cfg, td = _size_tree()
    tree = ref.process_traces(cfg, td)
    want_res = np.array([len(gg.resource_spans(rs)) for rs in tree["resourceSpans"]], dtype=np.uint64)
    eng = _engine(cfg, odigostrafficmetrics=TRAFFIC)
    assert eng.info().stages == native.STAGE_CONDATTR | native.STAGE_SIZE
    proc = host.Processor("odigostrafficmetrics", TRAFFIC)
    hb = proc.columnarize(td)
    b = Batch(cfg, td)
    cdb = CondAttrDeviceBatch(eng, b.hb)
    db = DeviceBatch(hb.cols)
    st = torch.cuda.current_stream().cuda_stream
    eng.condattr_process_device(cdb, stream=st)
    # span_size_out is the SIZE call's span_size column
    db.cols.span_size = cdb.o["span_size_out"].data_ptr()
    eng.process_device(db, native.STAGE_SIZE, native.GROUP_TRACE_ID, stream=st)
    torch.cuda.synchronize()
    rb, ab, acc = _counters(db, hb)
    print("res_bytes", rb.tolist(), "want", want_res.tolist())
    np.testing.assert_array_equal(rb, want_res)
    sets = np.ctypeslib.as_array((C.c_uint32 * hb.cols.n_resources).from_address(hb.cols.res_attrset))
    want_sets = np.zeros(hb.cols.n_attrsets, dtype=np.int64)
    for r in range(hb.cols.n_resources):
        want_sets[sets[r]] += int(want_res[r])
    np.testing.assert_array_equal(ab, want_sets)
    assert acc == b.n
    eng.close()


@pytest.mark.gpu
def test_gpu_dropin_processor_and_pipeline():
    for cfg, td in ((KATS["readme_examples"]["config"], None), _size_tree(), (adv_config(), adv_tree(0xD0, 300, 4, 9))):
        if td is None:
            td = {"resourceSpans": [kat_tree(c)["resourceSpans"][0] for c in KATS["readme_examples"]["cases"]]}
        want = ref.process_traces(cfg, td)
        p = host.Processor(SECTION, cfg)
        out = p.consume(td)
        assert ref.canon(out, td) == ref.canon(want, td)
        # everything but the span attributes is untouched
        strip = lambda t: [[{k: v for k, v in sp.items() if k != "attributes"} for ss in rs["scopeSpans"] for sp in ss["spans"]]
                           for rs in t["resourceSpans"]]
        assert strip(out) == strip(host.loads(host.dumps(td)))
        p.close()
        pipe = host.Processor("pipeline", {SECTION: cfg, "odigostrafficmetrics": TRAFFIC})
        out = pipe.consume(td)
        assert ref.canon(out, td) == ref.canon(want, td)
        m = pipe.metrics()
        total = sum(int(pt["value"]) for pt in m["otelcol_odigos_trace_data_size"])
        assert total == sum(len(gg.resource_spans(rs)) for rs in want["resourceSpans"])
        assert int(m["otelcol_odigos_accepted_spans"]) == sum(len(ss["spans"]) for rs in td["resourceSpans"] for ss in rs["scopeSpans"])
        pipe.close()


@pytest.mark.gpu
def test_gpu_refusals():
    from odigos_amd.batch import DeviceBatch, Engine, Generator, PinnedBatch
    L = native.lib()
    cfg = KATS["readme_examples"]["config"]
    eng = _engine(cfg, odigostrafficmetrics=TRAFFIC)
    g = Generator("url", seed=3, n_spans=64)
    db = DeviceBatch(g.cols)
    for mask in (native.STAGE_CONDATTR, native.STAGE_CONDATTR | native.STAGE_SIZE):
        with pytest.raises(native.OseError, match="ose_condattr_process") as ei:
            eng.process_device(db, mask)
        assert ei.value.code == native.OSE_ENOTSUP
        pb = PinnedBatch(eng, g.cols)
        with pytest.raises(native.OseError, match="ose_condattr_process") as ei:
            pb.process(mask)
        assert ei.value.code == native.OSE_ENOTSUP
        pb.close()
        h = C.c_void_p()
        assert L.ose_otlp_pipeline_create(eng.h, None, mask, 1 << 20, C.byref(h)) == native.OSE_ENOTSUP
        assert "ose_condattr_process" in native.last_error()
        out = C.c_void_p()
        fake = C.c_void_p(1)   # refused before the batch is looked at
        assert L.ose_otlp_encode(eng.h, fake, None, mask, native.GROUP_TRACE_ID, None, None, C.byref(out)) == native.OSE_ENOTSUP
        assert "ose_condattr_process" in native.last_error()
    # an engine without the section has no such stage
    plain = Engine({"odigostrafficmetrics": TRAFFIC})
    b = Batch(cfg, kat_tree(KATS["readme_examples"]["cases"][0]))
    with pytest.raises(native.OseError, match="not configured") as ei:
        plain.condattr_process(b.hb)
    assert ei.value.code == native.OSE_EINVAL
    info = native.CondAttrInfo()
    assert L.ose_engine_condattr_info(plain.h, C.byref(info)) == native.OSE_EINVAL
    # host columns that would lead a kernel out of bounds are refused
    b.hb.arrays["scope"][0] = 7
    with pytest.raises(native.OseError, match="out of range"):
        eng.condattr_process(b.hb)
    plain.close()
    eng.close()


@pytest.mark.gpu
def test_gpu_graph_capture():
    import torch
    from odigos_amd.batch import CondAttrDeviceBatch
    cfg = adv_config()
    b = Batch(cfg, adv_tree(0x6A, 700, 5, 20), align=True)
    want = b.want()
    eng = _engine(cfg)
    eager, cap = CondAttrDeviceBatch(eng, b.hb), CondAttrDeviceBatch(eng, b.hb)
    eng.condattr_process_device(eager, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            eng.condattr_process_device(cap, stream=s.cuda_stream)
    torch.cuda.synchronize()
    results = []
    for _ in range(2):
        for name in ("src", "val", "span_size_out", "scratch"):
            cap.o[name].fill_(0xEE)
        graph.replay()
        torch.cuda.synchronize()
        results.append(cap.results())
    for r in results:
        b.check(*r, eng.condattr_strings(), want)
    e = eager.results()
    np.testing.assert_array_equal(results[0][0], e[0])
    np.testing.assert_array_equal(results[0][0], results[1][0])
    np.testing.assert_array_equal(results[0][2], results[1][2])
    keep = results[0][0] != native.CA_KEEP
    np.testing.assert_array_equal(results[0][1][keep], results[1][1][keep])
    eng.close()
