"""Hand-laid batches for the size stage (tests/test_size_layouts.py).

A layout is a list of resources, each a list of scopes, each scope a span
count (spans with default columns) or a list of spans (span_size, keep,
url_out, tmpl_len, kind, name_len); the large layouts give the same three
levels as numpy arrays.  Everything the size stage reads is built here in
numpy, the way SqlBatch (tests/test_sqlop.py) and tests/trace_layouts.py
build theirs, including the columns earlier stages would have written (keep,
url_out, tmpl[i].len): OSE_STAGE_APPLY_KEEP / OSE_STAGE_APPLY_TEMPLATE read
them as laid.  Test infrastructure only.

restate() is the stage written again from processor.go:71-84 and the pdata
sizer's framing in exact integers; census() is the stage's dispatch (which
window finishes, cuts or fixes which run, which lane sees which gap, which
grid-stride iterations run), a pure function of the scope and span indices.

The constants a layout is laid against are parsed from size_kernel.hip and
size_device.hpp at import (K); DESIGNED pins the values the layouts were
drawn for, and test_constants_as_designed fails when one is retuned.
"""
from __future__ import annotations

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from odigos_amd import native

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
WAVE = 64
SET_ATTR, RENAME = native.OUT_SET_ATTR, native.OUT_RENAME
SERVER, CLIENT, INTERNAL = native.KIND_SERVER, native.KIND_CLIENT, native.KIND_INTERNAL
TAIL_LANES = [0, 1, 15, 16, 31, 32, 47, 48, 62, 63]      # the DPP row / bank edges of wave_seg_sum
LANE_RUNS = [1, 1, 14, 1, 15, 1, 15, 1, 14, 1]          # run lengths whose tails are TAIL_LANES


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    hip = (CSRC / "size_kernel.hip").read_text()
    dev = (CSRC / "size_device.hpp").read_text()

    def one(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: definition not found"
        return int(m.group(1))

    k = SimpleNamespace()
    k.kSThreads = one(hip, r"constexpr\s+int\s+kSThreads\s*=\s*(\d+)\s*;", "kSThreads")
    k.kLdsAttrsets = one(hip, r"constexpr\s+uint32_t\s+kLdsAttrsets\s*=\s*(\d+)\s*;", "kLdsAttrsets")
    k.tail_tiles = one(hip, r"#define\s+OSE_SIZE_TAIL_TILES\s+(\d+)", "OSE_SIZE_TAIL_TILES")
    k.tail_cap = one(hip, r"#define\s+OSE_SIZE_TAIL_CAP\s+(\d+)", "OSE_SIZE_TAIL_CAP")
    k.span_cap = one(hip, r"void launch_size_spans[^}]*?constexpr\s+uint64_t\s+cap\s*=\s*(\d+)\s*;", "launch_size_spans cap")
    k.s0_cap = one(hip, r"if\s*\(!blocks\s*&&\s*a\.n_resources\)[^;]*kSThreads,\s*(\d+)\)\s*;", "the S == 0 grid's cap")
    k.kSumBits = one(dev, r"constexpr\s+uint32_t\s+kSumBits\s*=\s*(\d+)\s*;", "kSumBits")
    assert "constexpr int kTailTiles = OSE_SIZE_TAIL_TILES;" in hip
    # two tiles per iteration of size_span_kernel
    assert "base += 2 * stride" in hip and "base + stride + threadIdx.x" in hip, "size_span_kernel's tiling changed"
    assert "t0 += kTailTiles * gstride" in hip, "size_tail_kernel's tiling changed"
    return k


K = _parse_constants()
DESIGNED = dict(kSThreads=256, tail_tiles=4, tail_cap=4096, kLdsAttrsets=2048, span_cap=1024, s0_cap=1024, kSumBits=40)
TILE = K.kSThreads
TAIL_STRIDE = K.tail_cap * K.tail_tiles * TILE      # scopes one size_tail_kernel iteration covers at the capped grid
SPAN_STRIDE = K.span_cap * TILE                     # spans one tile slot of size_span_kernel covers at the capped grid


# ---------------------------------------------------------------------------
# the pdata framing, in exact integers

def sov(x):
    """Bytes of the varint of x (proto.SizeVarint): 7 payload bits per byte."""
    x = np.asarray(x, dtype=np.int64)
    n = np.ones(x.shape, dtype=np.int64)
    for k in range(1, 10):
        n += x >= (1 << (7 * k))
    return n


def field_len(x):
    """A length-delimited field below number 16: tag, length, payload."""
    x = np.asarray(x, dtype=np.int64)
    return 1 + sov(x) + x


def sov_int(x: int) -> int:
    return max(1, -(-int(x).bit_length() // 7))


def _seg_sum(key, val, n):
    """Sum of val per key (0..n-1) for non-decreasing keys, in int64."""
    key = np.asarray(key, dtype=np.int64)
    assert key.size == 0 or (np.diff(key) >= 0).all(), "keys must be non-decreasing"
    c = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(val, dtype=np.int64))])
    ids = np.arange(n, dtype=np.int64)
    return c[np.searchsorted(key, ids, "right")] - c[np.searchsorted(key, ids, "left")]


def _pad(a, extra=16):
    """a with zeroed slack behind it (a zero-length column still has an address)."""
    a = np.ascontiguousarray(a)
    out = np.zeros((a.shape[0] + extra,) + a.shape[1:], dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


# ---------------------------------------------------------------------------
# the builder

def default_spans(k, salt=0):
    """k spans with varied sizes, all kept, untemplated."""
    return [(60 + (salt * 7 + j * 11) % 90, 1, 0, 0, SERVER, 3) for j in range(k)]


class Layout:
    """Host columns of a laid-out batch (numpy) and their ose_columns view.

    res_scopes: scopes per resource (0: a scopeless resource); scope_spans:
    spans per scope; span: dict of per-span arrays (span_size, keep, url_out,
    tmpl_len, kind, name_len), missing ones take a default pattern."""

    def __init__(self, name, res_scopes, scope_spans, span=None, n_attrsets=8, res_attrset=None, scope_size=None,
                 res_size=None, marks=None):
        self.name = name
        self.marks = dict(marks or {})          # seam name -> resource / scope / span index
        res_scopes = np.asarray(res_scopes, dtype=np.int64)
        scope_spans = np.asarray(scope_spans, dtype=np.int64)
        R, S, n = len(res_scopes), int(res_scopes.sum()), int(scope_spans.sum())
        assert len(scope_spans) == S, (name, len(scope_spans), S)
        self.R, self.S, self.n, self.A = R, S, n, int(n_attrsets)
        self.res_scopes, self.scope_spans = res_scopes, scope_spans
        self.scope_resource = np.repeat(np.arange(R, dtype=np.uint32), res_scopes)
        self.scope = np.repeat(np.arange(S, dtype=np.uint32), scope_spans)
        sidx, ridx, i = np.arange(S, dtype=np.int64), np.arange(R, dtype=np.int64), np.arange(n, dtype=np.int64)
        self.scope_size = (np.asarray(scope_size) if scope_size is not None else 5 + sidx * 7 % 23).astype(np.uint32)
        self.res_size = (np.asarray(res_size) if res_size is not None else 40 + ridx * 13 % 50).astype(np.uint32)
        self.res_attrset = (np.asarray(res_attrset) if res_attrset is not None else ridx % self.A).astype(np.uint32)
        assert self.res_attrset.size == 0 or int(self.res_attrset.max()) < self.A
        span = dict(span or {})
        self.span_size = np.asarray(span.get("span_size", 60 + i * 11 % 90)).astype(np.uint32)
        self.keep = np.asarray(span.get("keep", np.ones(n))).astype(np.uint8)
        self.url_out = np.asarray(span.get("url_out", np.zeros(n))).astype(np.uint8)
        self.tmpl_len = np.asarray(span.get("tmpl_len", np.zeros(n))).astype(np.uint32)
        self.kind = np.asarray(span.get("kind", np.full(n, SERVER))).astype(np.uint8)
        self.name_len = np.asarray(span.get("name_len", np.full(n, 3))).astype(np.uint32)
        for a, m in ((self.scope_size, S), (self.res_size, R), (self.res_attrset, R), (self.span_size, n), (self.keep, n),
                     (self.url_out, n), (self.tmpl_len, n), (self.kind, n), (self.name_len, n)):
            assert a.shape == (m,), (name, a.shape, m)
        self.tmpl = np.stack([np.zeros(n, dtype=np.uint32), self.tmpl_len], axis=1)     # ose_strref {off, len}
        self.url = None                          # the real-path columns of a fused form (with_paths)
        self._bind()

    @classmethod
    def from_tree(cls, name, resources, **kw):
        """resources: [[scope, ...], ...]; a scope is a span count or a list of
        (span_size, keep, url_out, tmpl_len, kind, name_len)."""
        res_scopes, scope_spans, rows = [], [], []
        for res in resources:
            res_scopes.append(len(res))
            for sc in res:
                spans = default_spans(sc, len(scope_spans)) if isinstance(sc, int) else list(sc)
                scope_spans.append(len(spans))
                rows += spans
        cols = np.array(rows, dtype=np.int64).reshape(-1, 6)
        span = dict(zip(("span_size", "keep", "url_out", "tmpl_len", "kind", "name_len"), cols.T))
        return cls(name, res_scopes, scope_spans, span, **kw)

    def _bind(self):
        c = native.Columns()
        c.n_spans, c.n_scopes, c.n_resources, c.n_attrsets = self.n, self.S, self.R, self.A
        self._held = {}
        for f in ("scope", "span_size", "name_len", "kind", "scope_size", "scope_resource", "res_size", "res_attrset"):
            a = _pad(getattr(self, f))
            self._held[f] = a
            setattr(c, f, a.ctypes.data)
        if self.url is not None:
            c.arena_bytes = self.url.arena_bytes
            for f, a in (("arena", self.url.arena), ("path", self.url.path), ("url_flags", self.url.flags)):
                self._held[f] = a
                setattr(c, f, a.ctypes.data)
        self.cols = c

    # ---- the fused form: real paths, url_out / tmpl from the URL oracle ----
    PATHS = [b"/user/1234", b"/a/b", b"/", b"/items/123e4567-e89b-12d3-a456-426614174000", b"/health",
             b"/orders/2024-01-02/items/12345678/" + b"detail/" * 19 + b"x", b"/v1/" + b"segment-name/" * 12 + b"99999999"]

    def with_paths(self):
        """The same tree with a path, method flags and a kind per span from a
        short list (templates of different lengths, some above 127 bytes);
        url_out / tmpl are then what the URL oracle gives (url_oracle)."""
        import copy
        b = copy.copy(self)
        b.name = self.name + ".paths"
        n = self.n
        i = np.arange(n, dtype=np.int64)
        has = native.URL_HAS_METHOD | native.URL_PATH_RAW
        eq = native.URL_NAME_EQ_METHOD
        flag_tab = np.array([has, has | eq, has, 0, has | eq, has | native.URL_TGT_STR_EMPTY | eq, has], dtype=np.uint8)
        kind_tab = np.array([SERVER, CLIENT, SERVER, SERVER, INTERNAL, CLIENT], dtype=np.uint8)
        pick = (i * 5 + i // 64) % len(self.PATHS)
        blob, offs = bytearray(b"\0" * 64), []
        for p in self.PATHS:
            offs.append(len(blob))
            blob += p + b"?" * 3
        u = SimpleNamespace()
        u.arena_bytes = len(blob) + 16
        u.arena = np.zeros((u.arena_bytes + 15) // 16 * 16 + 32, dtype=np.uint8)
        u.arena[:len(blob)] = np.frombuffer(bytes(blob), dtype=np.uint8)
        u.path = _pad(np.stack([np.array(offs, dtype=np.uint32)[pick],
                                np.array([len(p) for p in self.PATHS], dtype=np.uint32)[pick]], axis=1)).reshape(-1)
        u.flags = _pad(flag_tab[(i * 3 + i // 7) % len(flag_tab)])
        b.kind = kind_tab[(i + i // 5) % len(kind_tab)]
        b.name_len = np.where(u.flags[:n] & eq, 3, (i % 3) * 4).astype(np.uint32)
        b.url = u
        b._url_oracle = None
        b._bind()
        return b

    def url_oracle(self):
        """(url_out, tmpl lengths) of oracle/url.c under the default config; the
        layout's url_out / tmpl columns are set to them."""
        if self._url_oracle is None:
            from odigos_amd.batch import HostOutputs
            from tests.oracle_lib import UrlOracle
            # (the spans share a few paths: the output is far larger than the input arena)
            ho = HostOutputs(self.cols, tmpl_cap=int(4 * self.url.path[1::2].astype(np.int64).sum() + 16 * self.n + 4096))
            assert UrlOracle({}).process(self.cols, ho.outs, 4) == 0
            self.url_out = ho.view("url_out", np.uint8)[:self.n].copy()
            self.tmpl = ho.view("tmpl", np.uint32)[:2 * self.n].reshape(-1, 2).copy()
            self.tmpl_len = self.tmpl[:, 1].copy()
            self._url_oracle = (self.url_out, self.tmpl_len)
        return self._url_oracle

    # ---- sampling columns for SAMPLE | SIZE in OSE_GROUP_BATCH ----
    def with_sampling(self):
        """The same batch with trace_id / status / resource / res_svc(_str):
        every resource is the service with id 0 of a one-rule config
        (batch_config)."""
        import copy
        b = copy.copy(self)
        b._bind()
        b._add_sampling()
        return b

    def _add_sampling(self):
        span_res = self.scope_resource[self.scope].astype(np.uint32) if self.n else np.zeros(0, dtype=np.uint32)
        add = {"trace_id": _pad(np.tile(np.array([[7, 9]], dtype=np.uint64), (self.n, 1))).reshape(-1),
               "status": _pad(np.zeros(self.n, dtype=np.uint8)), "resource": _pad(span_res),
               "start_ns": _pad(np.full(self.n, 1_700_000_000_000_000_000, dtype=np.uint64)),
               "end_ns": _pad(np.full(self.n, 1_700_000_000_000_001_000, dtype=np.uint64)),
               "res_svc": _pad(np.zeros(self.R, dtype=np.uint32)), "res_svc_str": _pad(np.zeros(self.R, dtype=np.uint32))}
        for f, a in add.items():
            self._held[f] = a
            setattr(self.cols, f, a.ctypes.data)


def batch_config(ratio: float) -> dict:
    """odigossampling whose decision does not depend on the uniform: every
    resource is svc-00, kept with ratio 100 (u * 100 < 100) or dropped with 0."""
    return {"service_rules": [{"name": "all", "type": "service_name",
                               "rule_details": {"service_name": "svc-00", "sampling_ratio": ratio,
                                                "fallback_sampling_ratio": ratio}}]}


# ---------------------------------------------------------------------------
# the restatement (processor.go:71-84 over ptrace's ResourceSpansSize)

def span_sizes_after(L, templated: bool):
    """Each span's size after odigosurltemplate's writes."""
    sz = L.span_size.astype(np.int64)
    if not templated:
        return sz
    tl = L.tmpl_len.astype(np.int64)
    u = L.url_out
    # attr.PutStr(http.route | url.template, tmpl): KeyValue{key, AnyValue{string_value}} appended to attributes
    key = np.where(L.kind == CLIENT, len("url.template"), len("http.route"))
    kv = field_len(key) + field_len(field_len(tl))
    sz = sz + np.where(u & SET_ATTR, field_len(kv), 0)
    # span.SetName(method + " " + tmpl); an empty name is not on the wire
    old = L.name_len.astype(np.int64)
    sz = sz + np.where(u & RENAME, field_len(old + 1 + tl) - np.where(old > 0, field_len(old), 0), 0)
    return sz


def restate(L, sampled: bool, templated: bool, remove_empty: bool, inverse: int = 1):
    """(res_bytes[R], attrset_bytes[A], accepted_spans) the stage adds for one call."""
    kept = L.keep.astype(np.int64) != 0 if sampled else np.ones(L.n, dtype=bool)
    framed = np.where(kept, field_len(span_sizes_after(L, templated)), 0)        # ScopeSpans.spans
    body = _seg_sum(L.scope, framed, L.S)
    n_kept = _seg_sum(L.scope, kept, L.S)
    spanless = L.scope_spans == 0
    alive = spanless | (n_kept > 0)                                             # an emptied ScopeSpans is removed
    scope_framed = np.where(alive, field_len(L.scope_size.astype(np.int64) + body), 0)   # ResourceSpans.scope_spans
    res_body = _seg_sum(L.scope_resource, scope_framed, L.R)
    res_alive = _seg_sum(L.scope_resource, alive, L.R)
    res_had = _seg_sum(L.scope_resource, ~spanless, L.R) > 0
    removed = res_had & (res_alive == 0) if remove_empty else np.zeros(L.R, dtype=bool)
    size = np.where(removed, 0, L.res_size.astype(np.int64) + res_body)
    attr = np.zeros(L.A, dtype=np.int64)
    np.add.at(attr, L.res_attrset.astype(np.int64), size * int(inverse))
    return size.astype(np.uint64), attr, int(kept.sum())


# ---------------------------------------------------------------------------
# the census: the dispatch of size_span_kernel, size_tail_kernel and
# size_fix_kernel from the scope and span indices alone

def census(L) -> SimpleNamespace:
    c = SimpleNamespace()
    S, R, n = L.S, L.R, L.n
    sr = L.scope_resource.astype(np.int64)
    # ---- size_tail_kernel's grid ----
    tiles = -(-S // TILE)
    blocks = min(-(-tiles // K.tail_tiles), K.tail_cap)
    if not blocks and R:
        blocks = min(-(-R // TILE), K.s0_cap)
    gstride = blocks * TILE
    c.tail_blocks = blocks
    c.tail_second_iter = S > K.tail_tiles * gstride
    c.gap_s0 = R if S == 0 else 0
    c.s0_second_iter = S == 0 and R > gstride
    c.fix = c.in_window = c.cut_head = c.cut_tail = c.cut_both = c.empty_windows = 0
    c.gap_first = c.gap_inner = c.gap_lane0 = c.gap_after = 0
    c.walks, c.fix_windows, c.gap_sizes = [], [], []
    if S:
        W = -(-S // WAVE)
        s0 = np.arange(W, dtype=np.int64) * WAVE
        last = np.minimum(s0 + WAVE - 1, S - 1)
        r0, rl = sr[s0], sr[last]
        before = np.where(s0 > 0, sr[np.maximum(s0 - 1, 0)], -1)
        after = np.where(last + 1 < S, sr[np.minimum(last + 1, S - 1)], -1)
        whole_head = (s0 == 0) | (before != r0)
        whole_tail = (last + 1 >= S) | (after != rl)
        single = r0 == rl                       # non-decreasing keys: one run iff the ends agree
        fix = ~whole_head & (~single | whole_tail)
        c.fix = int(fix.sum())
        c.fix_windows = np.nonzero(fix)[0].tolist()
        for w in c.fix_windows:                 # size_fix_kernel's walk over the part slots
            visits, k = 0, w - 1
            while k >= 0:
                visits += 1
                if r0[k] != r0[w] or whole_head[k]:
                    break
                k -= 1
            c.walks.append(visits)
        s = np.arange(S, dtype=np.int64)
        nxt = np.append(sr[1:], -1)
        prv = np.append(-1, sr[:-1])
        tail = (s == S - 1) | (s % WAVE == WAVE - 1) | (nxt != sr)
        head = (s % WAVE == 0) | (prv != sr)
        c.cut_head, c.cut_tail = int((~whole_head).sum()), int((~whole_tail).sum())
        c.cut_both = int((single & ~whole_head & ~whole_tail).sum())
        c.in_window = int(tail.sum()) - (c.cut_head + c.cut_tail - c.cut_both)
        c.tails = tail
        gap = np.where(head, np.maximum(sr - prv - 1, 0), 0)
        c.gap_first = int(gap[0])
        lane0 = s % WAVE == 0
        c.gap_lane0 = int(gap[lane0][1:].sum())
        c.gap_inner = int(gap[~lane0].sum())
        c.gap_after = R - 1 - int(sr[-1])
        c.gap_sizes = sorted(set(gap[gap > 0].tolist()) | ({c.gap_after} if c.gap_after else set()))
        # every resource is finished exactly once
        assert c.gap_first + c.gap_lane0 + c.gap_inner + c.gap_after == R - len(np.unique(sr))
        # windows past the last scope inside launched tiles
        b = np.arange(blocks, dtype=np.int64) * TILE
        it = 0
        while True:
            t0 = b + it * K.tail_tiles * gstride
            live = t0 < S
            if not live.any():
                break
            for j in range(K.tail_tiles):
                for wv in range(TILE // WAVE):
                    c.empty_windows += int((t0[live] + j * gstride + wv * WAVE >= S).sum())
            it += 1
        c.tail_iters = it
    # ---- the spans pass ----
    sblocks = min(-(-n // TILE), K.span_cap)
    c.span_blocks = sblocks
    c.span_x1 = n > sblocks * TILE
    c.span_second_iter = n > 2 * sblocks * TILE
    c.partial_wave = n % WAVE
    if n:
        sc = L.scope.astype(np.int64)
        i = np.arange(n, dtype=np.int64)
        stail = (i == n - 1) | (i % WAVE == WAVE - 1) | (np.append(sc[1:], -1) != sc)
        c.span_tails = stail
        per_scope = np.bincount(sc[stail], minlength=L.S)
        c.max_scope_atomics = int(per_scope.max())
        full = n // WAVE * WAVE
        c.dropped_waves = int((L.keep[:full].reshape(-1, WAVE).sum(axis=1) == 0).sum())
    else:
        c.max_scope_atomics = c.dropped_waves = 0
    return c


def tail_lanes(tails, w):
    """The lanes of window / wave w that end a run."""
    return np.nonzero(tails[w * WAVE:(w + 1) * WAVE])[0].tolist()


# ---------------------------------------------------------------------------
# the layouts.  Tail-pass layouts give scopes per resource; their spans come
# from a fixed pattern (spanless scopes, kept and dropped spans mixed).

def _spans_pattern(S):
    return np.arange(S, dtype=np.int64) * 5 % 4          # 0, 1, 2, 3 spans per scope


def _tail_layout(name, res_scopes, marks=None, n_attrsets=8, res_attrset=None, drop_every=5):
    S = int(np.sum(res_scopes))
    sp = _spans_pattern(S)
    n = int(sp.sum())
    i = np.arange(n, dtype=np.int64)
    span = {"keep": (i % drop_every != 1) if drop_every else np.ones(n),
            "url_out": i % 4, "tmpl_len": 3 + i * 7 % 40, "kind": np.where(i % 3 == 0, CLIENT, SERVER),
            "name_len": np.where(i % 5 == 0, 0, 3)}
    return Layout(name, res_scopes, sp, span, n_attrsets=n_attrsets, res_attrset=res_attrset, marks=marks)


def lay_run_ends():
    """Runs wholly inside their windows: 64 runs of one scope; keys changing at
    every 16-lane row edge; tails on TAIL_LANES, the last on lane 63 with the
    next resource starting on lane 0; a partial last window."""
    return _tail_layout("run.ends", [1] * 64 + [16] * 4 + LANE_RUNS + [3, 61] + [4, 6])


def lay_run_cross():
    """A: lane 63 of window 0 to lane 0 of window 1; B: lane 1 of window 1 to
    lane 62 of window 2; C: the last run of window 2 (lane 63) and the first
    of window 3, both windows holding other runs."""
    rs = [20, 20, 23, 2, 126, 11, 30, 24, 5]
    return _tail_layout("run.cross", rs, marks={"A": 3, "B": 4, "C": 5})


def lay_run_long():
    """Runs over 2, 3 and 5 whole windows with partial ends (L2, L3, L5); H0
    starts on lane 0 and crosses; E63 began earlier and ends on lane 63; ONE
    is exactly one window; TWO exactly two."""
    rs = [13, 27, 173, 19, 237, 19, 365, 20, 23, 74, 20, 98, 64, 128, 7]
    return _tail_layout("run.long", rs, marks={"L2": 2, "L3": 4, "L5": 6, "H0": 9, "E63": 11, "ONE": 12, "TWO": 13})


def lay_run_tiles():
    """2600 scopes: 11 tiles over 3 blocks.  X crosses scope 255/256 (another
    block's tile follows); BIG covers more than 1024 scopes, among them whole
    tiles of every block and the edges between one block's in-flight tiles."""
    rs = [100, 150, 12, 438, 1200, 3, 61, 300, 336]
    return _tail_layout("run.tiles", rs, marks={"X": 2, "BIG": 4})


def lay_gaps(g):
    """Scopeless resources, g at a time: before the first scope, between runs
    inside a window, between a run ending on lane 63 and the next window's
    lane 0, and after the last scope."""
    rs = [0] * g + [10] + [0] * g + [20, 34] + [0] * g + [15, 70, 9] + [0] * g
    return _tail_layout(f"gaps.{g}", rs)


def lay_s0(R):
    """No scopes at all: every resource keeps its fixed size (the S == 0 loop)."""
    return Layout(f"gaps.S0.{R}", [0] * R, [], n_attrsets=8)


ENDS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def lay_ends(S):
    """S scopes in short runs, the last run ending at S - 1."""
    rs, tot, k = [], 0, 0
    while tot < S:
        r = min([3, 1, 5, 2, 9][k % 5], S - tot)
        rs.append(r)
        tot += r
        k += 1
    return _tail_layout(f"ends.{S}", rs)


def lay_removed():
    """Emptied scopes beside spanless ones; EMPTY: a resource whose scopes are
    all emptied and straddle a window edge (removed); STAYS: the same with one
    spanless scope; CARRY: the only scope with spans (emptied) lies three
    windows before the resource's end."""
    kept, dropped = (80, 1, 0, 0, SERVER, 3), (70, 0, 0, 0, SERVER, 3)
    emptied = [dropped, dropped]
    mixed = [dropped, kept, dropped]
    res = [[emptied, [], [kept], emptied, []],                       # 5 scopes: two emptied, two spanless
           [[kept]] * 20, [mixed] * 35,                              # -> lane 60
           [emptied] * 8,                                            # EMPTY: lanes 60..67
           [[kept]] * 52,                                            # -> lane 56 of window 1
           [emptied] * 8 + [[]] + [emptied] * 3,                     # STAYS: lanes 56..67 (window 1 -> 2)
           [[kept]] * 46,                                            # -> lane 50 of window 2
           [emptied] + [[]] * (13 + 64 * 3 + 20),                    # CARRY: lane 50 of window 2 into window 6
           [emptied], [[]], [mixed, emptied]]
    return Layout.from_tree("removed", res, marks={"EMPTY": 3, "STAYS": 5, "CARRY": 7, "LAST_EMPTY": 8})


def lay_attrsets(A):
    """A attribute sets, sets 0, A - 1 and kLdsAttrsets - 1 in use, most
    resources in set 7 over three blocks; a scopeless resource and a resource
    finished by size_fix_kernel in each of the marked sets."""
    rs = ([2, 3, 1] * 10 + [0] + [62, 4]) * 30      # each 127-scope block ends with a run that crosses a window edge
    R = len(rs)
    sets = np.full(R, 7, dtype=np.int64)
    marked = [0, K.kLdsAttrsets - 1, A - 1]
    for k, a in enumerate(marked):
        blk = 33 * (3 + 9 * k)
        sets[blk + 30] = a          # the scopeless resource
        sets[blk + 31] = a          # the 62-scope run
        sets[blk + 32] = a
        sets[blk + 1] = a
    return _tail_layout(f"attrsets.{A}", rs, n_attrsets=A, res_attrset=sets, marks={"sets": marked})


def lay_tail_stride():
    """cap * tiles * 256 + 257 scopes, nearly all spanless, in resources of 2
    to 4 scopes; one run crosses the first iteration's last scope; a few
    thousand spans over the first and the last tile."""
    S = TAIL_STRIDE + TILE + 1
    edge = TAIL_STRIDE                    # X covers edge - 2 .. edge + 1
    head = np.tile([2, 3, 4], (edge - 2) // 9 + 1)
    cs = np.cumsum(head)
    k = int(np.searchsorted(cs, edge - 2, "right"))
    head = head[:k].tolist()
    rest = edge - 2 - int(np.sum(head))
    if rest:
        head.append(rest)
    x = len(head)
    tail = [3, 2] * ((S - edge - 2) // 5 + 1)
    rs = np.array(head + [4] + tail, dtype=np.int64)
    cs = np.cumsum(rs)
    k = int(np.searchsorted(cs, S, "left"))
    rs = rs[:k + 1]
    rs[-1] -= int(rs.sum()) - S
    assert rs.min() > 0
    sp = np.zeros(S, dtype=np.int64)
    sp[:TILE] = np.arange(TILE) % 9
    sp[S - TILE:] = np.arange(TILE) % 11
    sp[edge - 2:edge + 2] = [2, 0, 1, 3]
    n = int(sp.sum())
    i = np.arange(n, dtype=np.int64)
    span = {"keep": i % 3 != 0, "url_out": i % 4, "tmpl_len": i % 200, "kind": np.where(i % 2 == 0, CLIENT, SERVER)}
    return Layout("tail.stride", rs, sp, span, n_attrsets=16, marks={"X": x, "edge": edge})


# ---- the spans pass ----

def lay_scope_runs():
    """Waves (64 spans) of the spans pass: 64 scopes of one span; scopes of 16;
    scope runs ending on TAIL_LANES; LONG: 700 spans from lane 10 over several
    waves and three 256-span blocks; DROPPED: a whole wave of dropped spans;
    HT: dropped spans at the head and the tail of a run; a partial last wave."""
    kept = lambda k, salt=0: default_spans(k, salt)
    drop = lambda k: [(75, 0, 0, 0, SERVER, 3)] * k
    scopes = [kept(1, j) for j in range(64)]                         # wave 0
    scopes += [kept(16, j) for j in range(4)]                        # wave 1
    scopes += [kept(k, j) for j, k in enumerate(LANE_RUNS)]          # wave 2
    scopes += [kept(10)]                                             # wave 3, lanes 0..9
    long_at = len(scopes)
    scopes += [kept(700)]                                            # lane 10 of wave 3 .. lane 5 of wave 14
    scopes += [kept(58)]                                             # -> wave 15
    dropped_at = len(scopes)
    scopes += [drop(64)]                                             # wave 15
    ht_at = len(scopes)
    scopes += [drop(2) + kept(6) + drop(2), drop(3) + kept(1), kept(1) + drop(3), [], kept(9)]
    # resources: runs of scopes, one per 7 scopes
    res, k = [], 0
    while k < len(scopes):
        res.append(scopes[k:k + 7])
        k += 7
    return Layout.from_tree("scope.runs", res, marks={"LONG": long_at, "DROPPED": dropped_at, "HT": ht_at})


SPAN_STRIDE_NS = [SPAN_STRIDE, SPAN_STRIDE + 1, 2 * SPAN_STRIDE, 2 * SPAN_STRIDE + 1 + 37]


def lay_span_stride(n):
    """n spans in scopes of 1 to 13 spans; one scope straddles span
    cap * 256 - 1 / cap * 256 (the x0 / x1 tile edge) when the batch reaches it."""
    edge = SPAN_STRIDE
    sizes = np.tile(np.array([1, 5, 13, 2, 8, 3, 64, 7], dtype=np.int64), n // 103 + 2)
    cs = np.cumsum(sizes)
    k = int(np.searchsorted(cs, n, "left"))
    sp = sizes[:k + 1].copy()
    sp[-1] -= int(sp.sum()) - n
    if n > edge:                               # make the scope holding span edge - 1 also hold span edge
        cs = np.cumsum(sp)
        j = int(np.searchsorted(cs, edge, "left"))       # scope j ends at cs[j] >= edge
        if cs[j] == edge:                      # it ends exactly at the edge: move one span over from the next scope
            sp[j] += 1
            sp[j + 1] -= 1
    S = len(sp)
    rs = np.full(-(-S // 5), 5, dtype=np.int64)
    rs[-1] -= int(rs.sum()) - S
    i = np.arange(n, dtype=np.int64)
    span = {"keep": (i * 7 % 11 != 0), "url_out": i % 4, "tmpl_len": i % 300, "kind": np.where(i % 2 == 0, CLIENT, SERVER),
            "name_len": np.where(i % 7 == 0, 0, 4)}
    return Layout(f"span.stride.{n}", rs, sp, span, n_attrsets=8, marks={"edge": edge})


def _both_sides(k):
    return [(1 << k) - 1, 1 << k]


VARINT_SPAN = [v for k in (7, 14, 21, 28) for v in _both_sides(k)] + [(1 << 32) - 1]
VARINT_SCOPE = [7, 14, 21, 28, 32, 35]


def _tmpl_lens():
    """tmpl_len 0 and the lengths at which the added KeyValue's payload, the
    AnyValue, the string and the renamed name cross 2^7 and 2^14."""
    fl = lambda x: 1 + sov_int(x) + x
    out = {0, 1}
    for lim in (1 << 7, 1 << 14):
        for key in (10, 12):
            for old in (0, 3):
                for f in (lambda t: fl(key) + fl(fl(t)),      # KeyValue payload
                          lambda t: fl(t),                    # AnyValue payload
                          lambda t: t,                        # the string
                          lambda t: old + 1 + t):             # the new name
                    t = next(t for t in range(lim - 64, lim + 1) if f(t) >= lim)
                    out |= {t - 1, t}
    return sorted(x for x in out if x >= 0)


def lay_varints():
    """Every level's length varint on both sides of its byte boundaries; all
    sums stay below 2^kSumBits.  span_size is a 32-bit column: 2^32 - 1 is its
    largest value, and scope bodies reach 2^32 and 2^35 as sums of such spans."""
    sp = lambda size: (size, 1, 0, 0, SERVER, 3)
    M = (1 << 32) - 1
    scopes = [[sp(v)] for v in VARINT_SPAN]
    # scope_size + body on both sides of 2^k: spanless, and with spans
    sizes = [5] * len(scopes)
    for k in (7, 14, 21, 28):
        for v in _both_sides(k):
            scopes.append([])
            sizes.append(v)
            scopes.append([sp(10)])                                  # framed 12
            sizes.append(v - 12)
    for v in _both_sides(32):                                        # 2^31 + 6 and 2^31 - 14 framed: 2^32 - 8
        scopes.append([sp(1 << 31), sp((1 << 31) - 20)])
        sizes.append(v - ((1 << 32) - 8))
    for v in _both_sides(35):                                        # 7 x (2^32 + 5) and one of 2^32 - 48 + 6
        scopes.append([sp(M)] * 7 + [sp(M - 47)])
        sizes.append(v - (7 * ((1 << 32) + 5) + M - 47 + 6))
    assert min(sizes) >= 0
    first_tmpl = len(scopes)
    for tl in _tmpl_lens():
        sc = []
        for kind in (CLIENT, SERVER, INTERNAL):
            for old in (0, 3):
                for u in (SET_ATTR, RENAME, SET_ATTR | RENAME):
                    sc.append((100, 1, u, tl, kind, old))
        sc.append((100, 0, SET_ATTR | RENAME, tl, CLIENT, 3))        # dropped: adds nothing
        scopes.append(sc)
        sizes.append(9)
    res, k = [], 0
    while k < len(scopes):
        res.append(scopes[k:k + 3])
        k += 3
    return Layout.from_tree("varints", res, scope_size=sizes, marks={"first_tmpl": first_tmpl})


SMALL = {
    "run.ends": lay_run_ends, "run.cross": lay_run_cross, "run.long": lay_run_long, "run.tiles": lay_run_tiles,
    "gaps.1": lambda: lay_gaps(1), "gaps.2": lambda: lay_gaps(2), "gaps.300": lambda: lay_gaps(300),
    "gaps.S0.1": lambda: lay_s0(1), "gaps.S0.255": lambda: lay_s0(255), "gaps.S0.257": lambda: lay_s0(257),
    f"gaps.S0.{K.s0_cap * TILE + 1}": lambda: lay_s0(K.s0_cap * TILE + 1),
    **{f"ends.{S}": (lambda S=S: lay_ends(S)) for S in ENDS},
    "removed": lay_removed,
    f"attrsets.{K.kLdsAttrsets}": lambda: lay_attrsets(K.kLdsAttrsets),
    f"attrsets.{K.kLdsAttrsets + 1}": lambda: lay_attrsets(K.kLdsAttrsets + 1),
    "scope.runs": lay_scope_runs, "varints": lay_varints,
}
LARGE = {"tail.stride": lay_tail_stride, **{f"span.stride.{n}": (lambda n=n: lay_span_stride(n)) for n in SPAN_STRIDE_NS}}
FUSED = ["scope.runs", "removed", "run.cross"]
_built = {}


def layout(name) -> Layout:
    """The named layout, built once (nothing writes to its columns)."""
    if name not in _built:
        if name.endswith(".paths"):
            b = layout(name[:-len(".paths")]).with_paths()
            b.url_oracle()
            _built[name] = b
        else:
            _built[name] = {**SMALL, **LARGE}[name]()
    return _built[name]


def drop(name):
    """Forget a large layout (its columns are tens of megabytes)."""
    _built.pop(name, None)
