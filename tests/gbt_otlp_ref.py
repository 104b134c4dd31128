"""Test infrastructure for groupbytrace on the OTLP path
(tests/test_groupbytrace_otlp.py), written independently of the engine.

* release_traces_data: a release of tests/gbt_ref.py as the TracesData the
  collector sends downstream: every piece of every released trace, in order,
  as one ResourceSpans with the piece's Resource, one ScopeSpans and the
  piece's spans in arrival order;
* hand-laid batches (raw protobuf bytes with Span messages of chosen
  lengths) and their census: what an OTLP-fed store keeps of an added batch,
  byte for byte (per span its message followed by its strings, per added
  scope a header block: the ResourceSpans payload without scope_spans, then
  the ScopeSpans payload without spans), and where each lies in the arena ring.
"""
from __future__ import annotations

from tests import otlp_gogo as gg


def release_traces_data(traces: list) -> dict:
    return {"resourceSpans": [p for tr in traces for p in tr]}


def spans_of(td: dict) -> list:
    return [sp for rs in td.get("resourceSpans") or [] for ss in rs.get("scopeSpans") or []
            for sp in ss.get("spans") or []]


# ---- hand-laid batches ---------------------------------------------------------

def span_of_len(n: int, tid: str = "") -> dict | None:
    """A span whose pdata encoding is exactly n bytes (None: no such span).
    pdata frames the three ids and the Status even when empty (8 bytes); the
    name and the trace state pad the rest."""
    base = {"traceId": tid, "spanId": "", "parentSpanId": "", "name": "", "kind": 0, "status": {}}
    have = len(gg.span(base))
    if n < have:
        return None
    if n == have:
        return base
    for kind in (0, 1):
        for ts in (0, 1, 2, 3):
            rest = n - have - (2 if kind else 0) - ((2 + ts) if ts else 0)
            # name of k bytes: 0 (absent), else tag + varint(k) + k
            for k in (rest, rest - 2, rest - 3, rest - 4):
                if k < 0:
                    continue
                sp = dict(base, name="n" * k, kind=kind)
                if ts:
                    sp["traceState"] = "t" * ts
                if len(gg.span(sp)) == n:
                    return sp
    return None


def raw_batch(resource: bytes, scope_fields: bytes, span_msgs: list, tail: bytes = b"") -> bytes:
    """TracesData with one ResourceSpans: `resource` (its fields other than
    scope_spans, written first), one ScopeSpans of `scope_fields` (its fields
    other than spans, written first) and the Span messages; `tail` follows
    the spans inside the ScopeSpans (a schema_url after them, say)."""
    ss = scope_fields + b"".join(gg._len(2, m) for m in span_msgs) + tail
    return gg._len(1, resource + gg._len(2, ss))


def _fields(b: bytes, lo: int, hi: int) -> list:
    """[(field, wire type, start, end, payload start or None)] of b[lo:hi]"""
    i, out = lo, []
    while i < hi:
        s = i
        t, i = _rv(b, i)
        wt, pay = t & 7, None
        if wt == 0:
            _, i = _rv(b, i)
        elif wt == 1:
            i += 8
        elif wt == 5:
            i += 4
        else:
            ln, i = _rv(b, i)
            pay = i
            i += ln
        out.append((t >> 3, wt, s, i, pay))
    return out


def pieces_of(pb: bytes) -> list:
    """The batch's layout, read with a plain protobuf walk:
    [(res_header, scope_header, [(offset, length) of each Span message])] per
    scope in order."""
    out = []
    for f, wt, s, e, pay in _fields(pb, 0, len(pb)):
        if f != 1 or wt != 2:
            continue
        rf = _fields(pb, pay, e)
        rh = b"".join(pb[a:z] for ff, w, a, z, _ in rf if not (ff == 2 and w == 2))
        for ff, w, a, z, sp in rf:
            if ff == 2 and w == 2:
                sf = _fields(pb, sp, z)
                sh = b"".join(pb[a2:z2] for f2, w2, a2, z2, _ in sf if not (f2 == 2 and w2 == 2))
                out.append((rh, sh, [(p2, z2 - p2) for f2, w2, _, z2, p2 in sf if f2 == 2 and w2 == 2]))
    return out


def _rv(b, i):
    v = s = 0
    while True:
        x = b[i]
        i += 1
        v |= (x & 0x7F) << s
        s += 7
        if x < 0x80:
            return v, i


class RingCensus:
    """Where an OTLP-fed store puts what it keeps: the spans' blocks of an add
    in span order, then the header blocks of its scopes in scope order, from
    the ring position the last add ended at.  `strings` gives the bytes that
    follow a span's message in its block (route, path, string attribute
    values, query: none for the hand-laid spans, which carry no attributes)."""

    def __init__(self, cap: int):
        self.cap = cap
        self.end = 0          # bytes ever added
        self.begin = 0        # bytes reclaimed
        self.marks = []       # (end after the add)
        self.msgs = []        # (position, source offset in the message, length)
        self.hdrs = []        # (position, length)

    def add(self, pb: bytes, strings=lambda m: 0) -> int:
        """-> bytes the add takes"""
        pos = self.end
        scopes = pieces_of(pb)
        for rh, sh, msgs in scopes:
            for off, ln in msgs:
                self.msgs.append((pos, off, ln))
                pos += ln + strings(pb[off:off + ln])
        for rh, sh, _ in scopes:
            self.hdrs.append((pos, len(rh) + len(sh)))
            pos += len(rh) + len(sh)
        took = pos - self.end
        self.end = pos
        self.marks.append(pos)
        return took

    def reclaim_all(self):
        self.begin = self.end

    @property
    def held(self) -> int:
        return self.end - self.begin

    def straddles(self, items) -> list:
        """the items lying across the ring's end"""
        return [it for it in items if it[-1] and it[0] % self.cap + it[-1] > self.cap]
