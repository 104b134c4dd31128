"""Test infrastructure: odigossqldboperationprocessor restated over bytes and
OTLP/JSON dicts, independently of the engine.

The source is `collector/processors/odigossqldboperationprocessor/
processor.go:30-143` of the reference.  Go is not available to the tests, so
the Go standard library functions the processor calls are restated here
literally from their published source, not in the forward form the kernel
uses:

* `strings.TrimSpace`: the ASCII loops from both ends, handing over to
  `TrimFunc` / `TrimRightFunc` with `unicode.IsSpace` at the first byte
  >= 0x80; `TrimRightFunc` walks back with `utf8.DecodeLastRune` and
  re-decodes the last kept rune forwards for its width.
* `utf8.DecodeRune` / `utf8.DecodeLastRune`: the accept-range tables; an
  invalid or short sequence is (RuneError, 1).
* `strings.ToUpper`: rune by rune; an invalid byte becomes U+FFFD.  Only the
  comparison with seven ASCII keywords matters, and U+0131 and U+017F are the
  only non-ASCII runes unicode.ToUpper maps to an ASCII letter, so every other
  non-ASCII rune is kept as it is (Python's str.upper() is NOT used: it
  applies full case mappings, e.g. U+FB05 -> "ST").

Python's bytes.strip() / str.strip() are not used either: they treat
0x1C-0x1F as space and know nothing of U+0085.
"""
from __future__ import annotations

import copy

RUNE_ERROR = 0xFFFD
UTF_MAX = 4
KEYWORDS = ("SELECT", "INSERT", "UPDATE", "DELETE", "CREATE", "DROP", "ALTER")   # processor.go:20-26
UNKNOWN = "UNKNOWN"
CODES = {UNKNOWN: 0, "SELECT": 1, "INSERT": 2, "UPDATE": 3, "DELETE": 4, "CREATE": 5, "DROP": 6, "ALTER": 7}

QUERY_KEY = "db.query.text"          # semconv.DBQueryTextKey
OPNAME_KEY = "db.operation.name"     # semconv.DBOperationNameKey
LANG_KEY = "telemetry.sdk.language"  # semconv.TelemetrySDKLanguageKey

_ASCII_SPACE = b"\t\n\v\f\r "


def is_space(r: int) -> bool:
    """unicode.IsSpace"""
    if r <= 0xFF:
        return r in (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0)
    return (r == 0x1680 or 0x2000 <= r <= 0x200A or r in (0x2028, 0x2029, 0x202F, 0x205F, 0x3000))


def _first(p0: int):
    """utf8.first[p0] as (size, lo, hi) of the second byte; size 0: invalid"""
    if 0xC2 <= p0 <= 0xDF:
        return 2, 0x80, 0xBF
    if p0 == 0xE0:
        return 3, 0xA0, 0xBF
    if 0xE1 <= p0 <= 0xEC or 0xEE <= p0 <= 0xEF:
        return 3, 0x80, 0xBF
    if p0 == 0xED:
        return 3, 0x80, 0x9F
    if p0 == 0xF0:
        return 4, 0x90, 0xBF
    if 0xF1 <= p0 <= 0xF3:
        return 4, 0x80, 0xBF
    if p0 == 0xF4:
        return 4, 0x80, 0x8F
    return 0, 0, 0


def decode_rune(p: bytes):
    """utf8.DecodeRune"""
    n = len(p)
    if n < 1:
        return RUNE_ERROR, 0
    p0 = p[0]
    if p0 < 0x80:
        return p0, 1
    sz, lo, hi = _first(p0)
    if sz == 0 or n < sz:
        return RUNE_ERROR, 1
    b1 = p[1]
    if b1 < lo or hi < b1:
        return RUNE_ERROR, 1
    if sz <= 2:
        return (p0 & 0x1F) << 6 | (b1 & 0x3F), 2
    b2 = p[2]
    if b2 < 0x80 or 0xBF < b2:
        return RUNE_ERROR, 1
    if sz <= 3:
        return (p0 & 0x0F) << 12 | (b1 & 0x3F) << 6 | (b2 & 0x3F), 3
    b3 = p[3]
    if b3 < 0x80 or 0xBF < b3:
        return RUNE_ERROR, 1
    return (p0 & 0x07) << 18 | (b1 & 0x3F) << 12 | (b2 & 0x3F) << 6 | (b3 & 0x3F), 4


def _rune_start(b: int) -> bool:
    return b & 0xC0 != 0x80


def decode_last_rune(p: bytes):
    """utf8.DecodeLastRune"""
    end = len(p)
    if end == 0:
        return RUNE_ERROR, 0
    start = end - 1
    r = p[start]
    if r < 0x80:
        return r, 1
    lim = max(end - UTF_MAX, 0)
    start -= 1
    while start >= lim:
        if _rune_start(p[start]):
            break
        start -= 1
    if start < 0:
        start = 0
    r, size = decode_rune(p[start:end])
    if start + size != end:
        return RUNE_ERROR, 1
    return r, size


def _trim_left_func(s: bytes) -> bytes:
    i = 0
    while i < len(s):
        r, w = decode_rune(s[i:])
        if not is_space(r):
            return s[i:]
        i += w
    return b""


def _trim_right_func(s: bytes) -> bytes:
    i = len(s)
    found = -1
    while i > 0:
        r, size = decode_last_rune(s[:i])
        i -= size
        if not is_space(r):
            found = i
            break
    i = found
    if i >= 0 and s[i] >= 0x80:
        _, wid = decode_rune(s[i:])
        i += wid
    else:
        i += 1
    return s[:i]


def trim_space(s: bytes) -> bytes:
    """strings.TrimSpace"""
    start = 0
    while start < len(s):
        c = s[start]
        if c >= 0x80:
            return _trim_right_func(_trim_left_func(s[start:]))
        if c not in _ASCII_SPACE:
            break
        start += 1
    stop = len(s)
    while stop > start:
        c = s[stop - 1]
        if c >= 0x80:
            return _trim_right_func(s[start:stop])
        if c not in _ASCII_SPACE:
            break
        stop -= 1
    return s[start:stop]


def extract_first_word(q: bytes) -> bytes:
    """extractFirstWord (processor.go:106-115)"""
    for i, c in enumerate(q):
        if c in b" \t\n":
            return q[:i]
    return q


def to_upper(s: bytes) -> bytes:
    """strings.ToUpper, exact wherever the result is compared with ASCII."""
    out = bytearray()
    i = 0
    while i < len(s):
        r, w = decode_rune(s[i:])
        if r == RUNE_ERROR and w == 1:
            out += b"\xef\xbf\xbd"
        elif 0x61 <= r <= 0x7A:
            out.append(r - 0x20)
        elif r == 0x0131:
            out += b"I"
        elif r == 0x017F:
            out += b"S"
        else:
            out += s[i:i + w]
        i += w
    return bytes(out)


def detect(query: bytes) -> str:
    """DetectSQLOperationName (processor.go:84-101)"""
    q = trim_space(bytes(query))
    if len(q) == 0:
        return UNKNOWN
    word = to_upper(extract_first_word(q))
    for k in KEYWORDS:
        if word == k.encode():
            return k
    return UNKNOWN


def code(query: bytes) -> int:
    return CODES[detect(query)]


# ---------------------------------------------------------------------------
# processTraces over an OTLP/JSON tree (odigos_amd.host.traces)

def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


def as_string_simple(v: dict) -> bytes:
    """pcommon.Value.AsString for the scalar types; other types need the
    caller's as_string."""
    if not v:
        return b""
    k, x = next(iter(v.items()))
    if k == "stringValue":
        return _b(x)
    if k == "intValue":
        return str(int(x)).encode()
    if k == "boolValue":
        return b"true" if x else b"false"
    raise ValueError(f"as_string_simple: {k}")


def _get(attrs, key):
    for kv in attrs or []:
        if kv["key"] == key:
            return kv.get("value") or {}
    return None


def should_exclude_language(cfg: dict, resource_attrs, as_string=as_string_simple) -> bool:
    """shouldExcludeLanguage (processor.go:119-143)"""
    ex = (cfg or {}).get("exclude")
    if ex is None:
        return False
    langs = ex.get("language") or []
    if len(langs) == 0:
        return False
    v = _get(resource_attrs, LANG_KEY)
    if v is None:
        return True
    return as_string(v) in [_b(x) for x in langs]


def process_traces(cfg: dict, td: dict, as_string=as_string_simple) -> dict:
    """processTraces (processor.go:30-78) on a copy of td."""
    td = copy.deepcopy(td)
    for rs in td.get("resourceSpans") or []:
        if should_exclude_language(cfg, (rs.get("resource") or {}).get("attributes"), as_string):
            continue
        for ss in rs.get("scopeSpans") or []:
            for sp in ss.get("spans") or []:
                q = _get(sp.get("attributes"), QUERY_KEY)
                if q is None:
                    continue
                if _get(sp.get("attributes"), OPNAME_KEY) is not None:
                    continue
                op = detect(as_string(q))
                if op != UNKNOWN:
                    sp.setdefault("attributes", []).append({"key": OPNAME_KEY, "value": {"stringValue": op}})
                    name = sp.get("name") or ""
                    sp["name"] = (name + b" " + op.encode()) if isinstance(name, bytes) else name + " " + op
    return td
