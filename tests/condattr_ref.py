"""Literal Python restatement of the traces half of
collector/processors/odigosconditionalattributes (processor.go:26-137,
factory.go:64-76, config.go), on OTLP/JSON trees.  Test infrastructure,
written from the Go text line by line; the line numbers are processor.go's
unless a file is named.

Go ranges over uniqueNewAttributes, a map, so the defaults are appended in
random order (:132): the order of appended attributes is no contract.  This
restatement appends them in target order (targets()), the order the engine's
Apply uses; compare trees with canon().
"""
from __future__ import annotations

import copy

from tests import otlp_gogo as gg

SECTION = "odigosconditionalattributes"
OTTL_SCOPE_NAME_KEY = "instrumentation_scope.name"   # :13


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


def _get(attrs, key):
    """pcommon.Map.Get: the first entry with the key."""
    for kv in attrs or []:
        if kv["key"] == key:
            return kv
    return None


def as_string(v: dict) -> str:
    """pcommon.Value.AsString"""
    return gg._as_string(v) if v else ""


def put_str(attrs: list, key: str, val: str):
    """pcommon.Map.PutStr: in place (the type becomes Str) or appended."""
    kv = _get(attrs, key)
    if kv is None:
        attrs.append({"key": key, "value": {"stringValue": val}})
    else:
        kv["value"] = {"stringValue": val}


def rules_of(cfg: dict) -> list:
    return [r or {} for r in (cfg or {}).get("rules") or []]


def values_of(rule: dict) -> list:
    """[(value, actions)] in byte order (the order the ABI numbers keys in)."""
    m = rule.get("new_attribute_value_configurations") or {}
    return sorted(((k, [a or {} for a in (v or [])]) for k, v in m.items()), key=lambda kv: _b(kv[0]))


def unique_new_attributes(cfg: dict) -> list:
    """calculateUniqueNewAttributes (factory.go:64-76), in target order."""
    return [t for t in targets(cfg) if t != ""]   # factory.go:69


def keys(cfg: dict) -> list:
    """The ABI's key numbering (include/odigos_amd.h): first appearance,
    rules in order; field_to_check, then per value in byte order per action
    from_field (when it is what the action uses) and new_attribute."""
    out = []

    def add(k):
        if k not in out:
            out.append(k)
    for r in rules_of(cfg):
        if r.get("field_to_check", "") != OTTL_SCOPE_NAME_KEY:
            add(r.get("field_to_check", ""))
        for _, acts in values_of(r):
            for a in acts:
                if not a.get("value") and a.get("from_field"):
                    add(a["from_field"])
                add(a.get("new_attribute", "") or "")
    return out


def targets(cfg: dict) -> list:
    out = []
    for r in rules_of(cfg):
        for _, acts in values_of(r):
            for a in acts:
                n = a.get("new_attribute", "") or ""
                if n not in out:
                    out.append(n)
    return out


def add_attributes(span_attrs: list, rule: dict, scope_name: str, scope_attrs: list, res_attrs: list, puts: dict, ev: list):
    """addAttributes (:55-102) and handleScopeNameConditionalAttribute (:104-126).
    puts[name] = the value of the last PutStr; ev collects what happened."""
    field = rule.get("field_to_check", "") or ""
    vmap = rule.get("new_attribute_value_configurations") or {}
    if field == OTTL_SCOPE_NAME_KEY:                                     # :59
        if scope_name in vmap:                                            # :109
            ev.append("hit_scope_name")
            for a in vmap[scope_name] or []:
                a = a or {}
                name = a.get("new_attribute", "") or ""
                if a.get("value"):                                        # :111
                    if _get(span_attrs, name) is None:                    # :113
                        put_str(span_attrs, name, a["value"])
                        puts[name] = a["value"]
                        ev.append(("static", name))
                    else:
                        ev.append(("present", name))
                elif a.get("from_field"):                                 # :116
                    f = _get(span_attrs, a["from_field"])                 # :118
                    if f is not None:
                        if _get(span_attrs, name) is None:                # :119
                            v = as_string(f["value"])
                            put_str(span_attrs, name, v)
                            puts[name] = v
                            ev.append(("copied", name))
                        else:
                            ev.append(("present", name))
        return                                                            # :61
    attr_str = ""                                                         # :64
    via = "absent"
    for which, attrs in (("span", span_attrs), ("scope", scope_attrs), ("resource", res_attrs)):   # :66-67
        kv = _get(attrs, field)
        if kv is not None:                                                # :68
            attr_str = as_string(kv["value"])                             # :69
            via = which
            break                                                         # :70
    if attr_str in vmap:                                                  # :75 (no early return for "")
        ev.append("hit_" + via)
        if attr_str == "" and via == "absent":
            ev.append("empty_match")
        for a in vmap[attr_str] or []:                                    # :76
            a = a or {}
            name = a.get("new_attribute", "") or ""

            def put(v, kind):
                had = _get(span_attrs, name) is not None
                if not had:                                               # :80 / :89
                    pass
                elif _get(scope_attrs, name) is None:                     # :82 / :91
                    pass
                elif _get(res_attrs, name) is None:                       # :84 / :93
                    pass
                else:
                    ev.append(("suppressed", name))
                    return
                put_str(span_attrs, name, v)
                puts[name] = v
                ev.append(("overwrite" if had else kind, name))
            if a.get("value"):                                            # :79
                put(a["value"], "static")
            elif a.get("from_field"):                                     # :87
                f = _get(span_attrs, a["from_field"])                     # :88
                if f is not None:
                    put(as_string(f["value"]), "copied")


def process_span(cfg: dict, span: dict, scope_name: str, scope_attrs: list, res_attrs: list, unique=None):
    """processSpan (:43-53) in place; returns (puts, events).  unique: the
    processor's uniqueNewAttributes, computed once per processor (factory.go:32)."""
    attrs = span.setdefault("attributes", [])
    puts, ev = {}, []
    for rule in rules_of(cfg):                                            # :48
        add_attributes(attrs, rule, scope_name, scope_attrs, res_attrs, puts, ev)
    gd = (cfg or {}).get("global_default", "") or ""
    for name in (unique if unique is not None else unique_new_attributes(cfg)):   # :132
        if _get(attrs, name) is None:                                     # :133
            put_str(attrs, name, gd)                                      # :134
            puts[name] = gd
            ev.append(("default", name))
    return puts, ev


def process_traces(cfg: dict, td: dict, detail: list | None = None) -> dict:
    """processTraces (:26-41) on a copy; detail receives (puts, events) per span."""
    td = copy.deepcopy(td)
    unique = unique_new_attributes(cfg)                                   # factory.go:32
    for rs in td.get("resourceSpans") or []:
        ra = (rs.get("resource") or {}).get("attributes") or []
        for ss in rs.get("scopeSpans") or []:
            sc = ss.get("scope") or {}
            for sp in ss.get("spans") or []:
                d = process_span(cfg, sp, sc.get("name", "") or "", sc.get("attributes") or [], ra, unique)
                if detail is not None:
                    detail.append(d)
    return td


def canon(td: dict, orig: dict) -> list:
    """Per span: the attributes the input had, in place, then the appended
    ones sorted by key (their order is no contract)."""
    out = []
    for rs, ro in zip(td["resourceSpans"], orig["resourceSpans"]):
        for ss, so in zip(rs["scopeSpans"], ro["scopeSpans"]):
            for sp, spo in zip(ss["spans"], so["spans"]):
                n0 = len(spo.get("attributes") or [])
                a = sp.get("attributes") or []
                out.append((a[:n0], sorted(a[n0:], key=lambda kv: _b(kv["key"]))))
    return out
