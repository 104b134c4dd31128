"""Hand-laid batches for the URL stage (tests/test_url_layouts.py).

A layout is a list of 64-lane groups; each lane gives a path (bytes), where it
lies in the arena ((align, rem): the next offset with off % align == rem;
an int: that offset; ("at", tag): the offset of the tagged lane, ("rel", d): d
bytes from the group's start, so paths may share bytes), its url_flags and its
kind.  Everything the URL stage reads is
built here in numpy (arena, path, kind, url_flags, arena_bytes), the way
tests/test_unicode_regex.py::_cols_from_paths does.  The bytes between paths
are a seeded filler of '/', '?', '@', digits and 0xFF, so a mask that leaks a
neighbour's byte changes the result.  Test infrastructure only.

The constants a layout is laid against are parsed from url_kernel.hip and
kernels.hpp at import (K); DESIGNED pins the values the layouts were drawn
for, and test_constants_as_designed fails when one is retuned, so a layout
cannot slide off its seam unnoticed.

dispatch() restates which kernel takes a group (url_plan_kernel's staging and
list limits, url_plan_slow_kernel's subsets, the LDS image limit) from the
columns alone; it does not restate templating.  py_process() restates the
default-config templating (processor.go:150-190, templatize.go:242-269) with
Python `re`, independently of oracle/url.c.
"""
from __future__ import annotations

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from odigos_amd import native

CSRC = Path(__file__).resolve().parent.parent / "odigos_amd" / "csrc"
WAVE = 64


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    hip = (CSRC / "url_kernel.hip").read_text()
    hpp = (CSRC / "kernels.hpp").read_text()
    known = {}

    def const(text, name):
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, f"{name}: definition not found"
        expr = re.sub(r"(\d)u\b", r"\1", m.group(1)).replace("/", "//")
        assert re.fullmatch(r"[\w\s*+/()-]+", expr), (name, expr)
        known[name] = int(eval(expr, {"__builtins__": {}}, dict(known)))   # (sums and products of earlier constants)
        return known[name]

    k = SimpleNamespace()
    for name in ("kStage", "kNameTab", "kRowVec", "kWaveOut", "kBNames", "kSegCap", "kPlanStage", "kPlanBmRows", "kImgCap"):
        setattr(k, name, const(hip, name))
    for name in ("kUrlMaxWaves", "kUrlWaveSlack"):
        setattr(k, name, const(hpp, name))

    def literal(pattern, what):
        m = re.search(pattern, hip)
        assert m, f"url_kernel.hip: {what} changed; tests/url_layouts.py must follow it"
        return [int(x) for x in m.groups()]

    # the longest segment classified from a 64-bit window (plan_group_list)
    k.win_seg, = literal(r"if \(L <= (\d+)\)\s*\n\s*id = classify_spec\(", "the windowed segment limit")
    # the 6-row window of a path
    k.win_bits, = literal(r"const bool win = needs_path && b0 \+ plen <= (\d+);", "the path window")
    # the branch-free fold
    k.fold, = literal(r"if \(nseg <= (\d+)\) \{\s*// one read of the", "the fold's entry count")
    # the plan code's nibbles: 16 segments, ids below 15
    k.code_nibbles, k.code_ids = literal(r"if \(k < (\d+) && id < (\d+)\) p\.code \|=", "the plan code's nibbles")
    # the dispatch rules restated by dispatch()
    for line, what in (("if (bytes <= kPlanStage) {", "the contiguous staging rule"),
                       ("if (total * 16 > kPlanStage) {", "the gathered staging rule"),
                       ("if (total > kSegCap) return false;", "the segment list limit"),
                       ("bool take = todo && cs + nc <= kPlanStage / 16;", "the slow planner's subsets"),
                       ("__ballot(p.mode == M_RULE || big) == 0 && sum <= kImgCap;", "the fast assembly rule"),
                       ("const bool direct = img_bytes > kWaveOut || lo16 == ~0u;", "the slow writer's image rule"),
                       ("if (bytes > kStage) return ~0u;", "the slow writer's stage rule"),
                       ("if (o + l + 1 > kBNames || l > 255) { ok = false; break; }", "the braced-name table rule"),
                       ("return std::min<uint64_t>(256 << 10, cap / 8 / std::max<uint32_t>(1, waves)) & ~15ull;",
                        "url_refs_chunk"),
                       ("return std::min<uint32_t>(cap, (a.n_groups + kWaves - 1) / kWaves);", "the plan grid's size"),
                       ("const uint64_t csz = max(a.refs_chunk, need);", "the refs form's chunk size")):
        assert line in hip, f"url_kernel.hip: {what} changed; tests/url_layouts.py must follow it"
    return k


K = _parse_constants()
DESIGNED = dict(kPlanStage=3072, kSegCap=192, kImgCap=4752, kStage=4096, kWaveOut=4096, kNameTab=64, kBNames=1024,
                kUrlMaxWaves=4096, kUrlWaveSlack=8192, kRowVec=3, kPlanBmRows=99, win_seg=64, win_bits=192, fold=8,
                code_nibbles=16, code_ids=15)

HAS = native.URL_HAS_METHOD
RAW = HAS | native.URL_PATH_RAW
TARGET = HAS | native.URL_PATH_TARGET
EQ = native.URL_NAME_EQ_METHOD
SERVER, CLIENT, INTERNAL = 2, 3, 1
GATE1 = HAS | native.URL_TGT_STR_EMPTY | EQ | native.URL_PATH_RAW     # a lone "/" and RENAME


# ---------------------------------------------------------------------------
# the default-config templating in Python (nothing here calls the oracle)

NO_LETTERS = re.compile(rb"^[\d_\-!@#$%^&*()=+{}\[\]:;\"'<>,.?/\\|`~]+\Z")
UUID = re.compile(rb"(^[0-9a-fA-F]{8}-[0-9a-fA-F]{4}-[0-9a-fA-F]{4}-[0-9a-fA-F]{4}-[0-9a-fA-F]{12})|"
                  rb"([0-9a-fA-F]{8}-[0-9a-fA-F]{4}-[0-9a-fA-F]{4}-[0-9a-fA-F]{4}-[0-9a-fA-F]{12}\Z)")
HEX = re.compile(rb"^(?:[0-9a-fA-F]{2}){8,}\Z")
LONGNUM = re.compile(rb"[0-9]{7,}")
DATE = re.compile(rb"^[0-9]{4}-[0-9]{2}-[0-9]{2}(?:T[0-9]{2}:[0-9]{2}(?::[0-9]{2})?)?(?:Z|[+-][0-9]{4})?\Z")
EMAIL = re.compile(rb"^[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}\Z")


def reference_name(seg: bytes):
    """getSegmentTemplatizationString (templatize.go:242-269) with Python re
    (the patterns of tests/test_url_random.py) and the U+FFFD rule: Go decodes
    a byte that is no valid UTF-8 as U+FFFD, which the id pattern holds."""
    if DATE.search(seg):
        return "date"
    if EMAIL.search(seg):
        return "email"
    if NO_LETTERS.search(seg) or LONGNUM.search(seg) or UUID.search(seg) or HEX.search(seg):
        return "id"
    if "\ufffd" in seg.decode("utf-8", "replace"):
        return "id"
    return None


_tmpl_memo = {}


def py_template(path: bytes, target: bool) -> bytes:
    """applyTemplatizationOnPath without rules or custom ids."""
    key = (path, target)
    if key in _tmpl_memo:
        return _tmpl_memo[key]
    p = path.split(b"?", 1)[0] if target else path        # strings.SplitN(target, "?", 2)[0]
    lead = p[:1] == b"/"
    body = p[1:] if lead else p
    if body == b"":
        out = b"/"                                          # "" and "/" (processor.go:156-160)
    else:
        segs = body.split(b"/")
        names = [reference_name(s) for s in segs]
        if not any(names):
            out = b"/" + body                               # the slash-prefixed original (:182-185)
        else:
            out = (b"/" if lead else b"") + b"/".join(b"{" + n.encode() + b"}" if n else s for s, n in zip(segs, names))
    _tmpl_memo[key] = out
    return out


def gate_of(flags: int, kind: int) -> int:
    """enhanceSpan's gate (processor.go:235-259): 0 skip, 1 rename to "/", 2 template the path."""
    if not flags & HAS or kind not in (SERVER, CLIENT):
        return 0
    tgt = flags & native.URL_TGT_MASK
    if tgt != native.URL_TGT_ABSENT:
        return 1 if tgt == native.URL_TGT_STR_EMPTY and flags & EQ else 0
    return 2 if flags & native.URL_PATH_MASK else 0


# ---------------------------------------------------------------------------
# the builder

class Lane:
    """One span.  path None: no path ref ({0, 0}).  before / after: bytes laid
    directly around the path in place of the filler.  seam: the name the
    census finds the lane by."""

    def __init__(self, path=b"", at=(16, 0), flags=RAW, kind=SERVER, tag=None, before=b"", after=b"", seam=None):
        self.path, self.at, self.flags, self.kind = path, at, flags, kind
        self.tag, self.before, self.after, self.seam = tag, before, after, seam


FILL = np.frombuffer(b"/?@0123456789\xff\xff//??@@", dtype=np.uint8)


class Layout:
    """Host columns of a laid-out batch (numpy) and their ose_columns view.
    cfg: the odigosurltemplate config it runs under (None: any config whose
    rules and custom ids match nothing); fused: the braced-name table loads
    under cfg; big: template names outside the braced table under cfg.
    prefix: (arena bytes, path refs, flags, kinds) of spans laid before the
    groups (whole groups)."""

    def __init__(self, name, groups, seed, cfg=None, fused=True, big=(), prefix=None):
        self.name, self.seed, self.cfg, self.fused, self.big = name, seed, cfg, fused, tuple(big)
        lanes = []
        for k, g in enumerate(groups):
            assert len(g) == WAVE or (k == len(groups) - 1 and 0 < len(g) <= WAVE), (name, k, len(g))
            lanes += g
        n0 = 0 if prefix is None else len(prefix[2])
        assert n0 % WAVE == 0
        n = n0 + len(lanes)
        path = np.zeros((n, 2), dtype=np.uint32)
        flags = np.zeros(n, dtype=np.uint8)
        kind = np.zeros(n, dtype=np.uint8)
        cursor = 64
        if prefix is not None:
            path[:n0], flags[:n0], kind[:n0] = prefix[1], prefix[2], prefix[3]
            cursor = len(prefix[0])
        writes, tags = [], {}
        for i, ln in enumerate(lanes):
            if i % WAVE == 0:
                cursor = -(-cursor // 64) * 64
                tags, gstart = {}, cursor
            flags[n0 + i], kind[n0 + i] = ln.flags, ln.kind
            if ln.path is None:
                continue
            at = ln.at
            if isinstance(at, int):
                off = at
                assert off - len(ln.before) >= cursor, (name, i, off, cursor)
            elif at[0] == "at":
                off = tags[at[1]]
            elif at[0] == "rel":
                off = gstart + at[1]
            else:
                off = cursor + (at[1] - cursor) % at[0]
                while off - cursor < len(ln.before):
                    off += at[0]
            writes.append((off - len(ln.before), ln.before + ln.path + ln.after))
            cursor = max(cursor, off + len(ln.path) + len(ln.after))
            if ln.tag is not None:
                tags[ln.tag] = off
            path[n0 + i] = (off, len(ln.path))
        self.arena_bytes = cursor + 16
        size = (self.arena_bytes + 15) // 16 * 16 + 32
        rng = np.random.default_rng(seed)
        arena = FILL[rng.integers(0, len(FILL), size=size)]
        if prefix is not None:
            arena[:len(prefix[0])] = prefix[0]
        for off, b in writes:
            arena[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
        for i, ln in enumerate(lanes):       # paths that share bytes agree on them
            if ln.path is not None:
                o = int(path[n0 + i, 0])
                assert arena[o:o + len(ln.path)].tobytes() == ln.path, (name, i)
        self.n, self.n0, self.lanes = n, n0, lanes
        self.arena, self.path, self.flags, self.kind = arena, path, flags, kind
        self.n_groups = (n + WAVE - 1) // WAVE
        self._dispatch = self._oracle = None
        self._bind()

    def _bind(self):
        c = native.Columns()
        c.n_spans, c.arena_bytes = self.n, self.arena_bytes
        self._path_flat = np.ascontiguousarray(self.path.reshape(-1))
        for f, a in (("arena", self.arena), ("path", self._path_flat), ("kind", self.kind), ("url_flags", self.flags)):
            assert a.flags["C_CONTIGUOUS"]
            setattr(c, f, a.ctypes.data)
        self.cols = c

    def find(self, seam):
        """[(group, lane)] of the lanes carrying a seam label, in batch order."""
        return [divmod(self.n0 + i, WAVE) for i, ln in enumerate(self.lanes) if ln.seam == seam]

    def seams(self):
        return sorted({ln.seam for ln in self.lanes if ln.seam is not None})

    def path_bytes(self, i) -> bytes:
        o, l = int(self.path[i, 0]), int(self.path[i, 1])
        return self.arena[o:o + l].tobytes()

    # ---- the default-config templating, in Python ----
    def py_process(self):
        """(url_out, [template bytes]) of every span under the default config."""
        out = np.zeros(self.n, dtype=np.uint8)
        tm = [b""] * self.n
        for i in range(self.n):
            f = int(self.flags[i])
            g = gate_of(f, int(self.kind[i]))
            if g == 1:
                out[i], tm[i] = native.OUT_RENAME, b"/"
            elif g == 2:
                tm[i] = py_template(self.path_bytes(i), (f & native.URL_PATH_MASK) == native.URL_PATH_TARGET)
                out[i] = native.OUT_SET_ATTR | (native.OUT_RENAME if f & EQ else 0)
        return out, tm

    # ---- the census: which kernel takes a group, from the columns alone ----
    def dispatch(self):
        if self._dispatch is None:
            memo = {}
            self._dispatch = [self._dispatch_group(g, memo) for g in range(self.n_groups)]
        return self._dispatch

    def _dispatch_group(self, g, memo):
        a, e = g * WAVE, min(self.n, (g + 1) * WAVE)
        off = self.path[a:e, 0].astype(np.int64)
        ln = self.path[a:e, 1].astype(np.int64)
        gate = np.array([gate_of(int(f), int(k)) for f, k in zip(self.flags[a:e], self.kind[a:e])])
        g2 = gate == 2
        lo = int(off[g2].min()) if g2.any() else 0
        hi = int((off + ln)[g2].max()) if g2.any() else 0
        key = None
        if g2.any() and hi - lo <= 2 * K.kStage:
            key = ((off - lo)[g2].tobytes(), ln.tobytes(), self.flags[a:e].tobytes(), self.kind[a:e].tobytes(), lo & 31,
                   self.arena[lo:hi].tobytes())
            if key in memo:
                return memo[key]
        d = SimpleNamespace(gate=gate, lo=lo, hi=hi, needs=int(g2.sum()))
        lo16 = lo & ~15
        d.range_bytes = (hi - lo16 + 15) & ~15 if lo < hi else 0
        nc = np.where(g2 & (ln > 0), ((off + ln + 15) >> 4) - (off >> 4), 0)
        d.nc, d.chunks = nc, int(nc.sum())
        cs = np.cumsum(nc) - nc
        if lo >= hi:
            d.staging = "empty"
            base = np.zeros(e - a, dtype=np.int64)
        elif d.range_bytes <= K.kPlanStage:
            d.staging = "contiguous"
            base = np.full(e - a, lo16, dtype=np.int64)
        elif 16 * d.chunks <= K.kPlanStage:
            d.staging = "gathered"
            base = np.where(g2 & (ln > 0), off - (16 * cs + (off & 15)), 0)
        else:
            d.staging = "unplanned"
            base = np.full(e - a, lo16, dtype=np.int64)
        d.p0 = off - base                       # stage offset of each path
        d.n = np.zeros(e - a, dtype=np.int64)   # the path's bytes after the '?' cut
        d.lead = np.zeros(e - a, dtype=np.int64)
        d.nseg = np.zeros(e - a, dtype=np.int64)
        d.longest = np.zeros(e - a, dtype=np.int64)
        d.win = np.zeros(e - a, dtype=bool)
        d.segs = [None] * (e - a)
        for j in np.nonzero(g2)[0]:
            p = self.path_bytes(a + j)
            if (int(self.flags[a + j]) & native.URL_PATH_MASK) == native.URL_PATH_TARGET:
                p = p.split(b"?", 1)[0]
            d.n[j] = len(p)
            d.lead[j] = int(p[:1] == b"/")
            d.win[j] = (int(d.p0[j]) & 31) + int(ln[j]) <= K.win_bits
            if len(p) != d.lead[j]:
                sl = [len(s) for s in p[d.lead[j]:].split(b"/")]
                d.segs[j] = sl
                d.nseg[j], d.longest[j] = len(sl), max(sl)
        d.total = int(d.nseg.sum())
        d.listed = d.staging != "unplanned" and d.total <= K.kSegCap and int(d.longest.max(initial=0)) <= K.win_seg
        d.unplanned = bool(g2.any()) and not d.listed
        d.subsets = self._subsets(nc, g2) if d.unplanned else []
        if key is not None:
            memo[key] = d
        return d

    @staticmethod
    def _subsets(nc, todo):
        """url_plan_slow_kernel's rounds: [("subset", lanes, chunks) | ("alone", lane, chunks)]."""
        todo = todo.copy()
        out = []
        while todo.any():
            c = np.where(todo, nc, 0)
            cs = np.cumsum(c) - c
            take = todo & (cs + nc <= K.kPlanStage // 16)
            if not take.any():
                first = int(np.nonzero(todo)[0][0])
                out.append(("alone", first, int(nc[first])))
                todo[first] = False
                continue
            out.append(("subset", int(take.sum()), int(nc[take].sum())))
            todo &= ~take
        return out

    # ---- the oracle's result (built once; nothing writes to it) ----
    def oracle(self, cfg=None):
        """(url_out, refs (n, 2), output arena, used) of oracle/url.c under cfg (default: self.cfg or {})."""
        from odigos_amd.batch import HostOutputs
        from tests.oracle_lib import UrlOracle
        cfg = cfg if cfg is not None else (self.cfg or {})
        key = repr(cfg)
        if self._oracle is None:
            self._oracle = {}
        if key not in self._oracle:
            ho = HostOutputs(self.cols, tmpl_cap=tmpl_cap(self))
            assert UrlOracle(cfg).process(self.cols, ho.outs, nthreads=8) == 0
            used = int(ho.used[0])
            self._oracle[key] = (ho.view("url_out", np.uint8)[:self.n].copy(),
                                 ho.view("tmpl", np.uint32)[:2 * self.n].reshape(-1, 2).copy(),
                                 ho.bufs["tmpl_arena"][:used].copy(), used)
        return self._oracle[key]

    def group_sums(self, cfg=None):
        """Output bytes per group (the oracle's template lengths)."""
        url_out, refs, _, _ = self.oracle(cfg)
        lens = np.where(url_out != 0, refs[:, 1], 0).astype(np.int64)
        pad = np.zeros(self.n_groups * WAVE, dtype=np.int64)
        pad[:self.n] = lens
        return pad.reshape(-1, WAVE).sum(axis=1)

    def lane_out_offsets(self, cfg=None):
        """Each span's offset in its group's image and its template length."""
        url_out, refs, _, _ = self.oracle(cfg)
        pad = np.zeros(self.n_groups * WAVE, dtype=np.int64)
        pad[:self.n] = np.where(url_out != 0, refs[:, 1], 0)
        lens = pad.reshape(-1, WAVE)
        return (np.cumsum(lens, axis=1) - lens).reshape(-1)[:self.n], pad[:self.n]

    def expect(self, cfg=None):
        """{"url_unplanned", "url_slow"}: the groups url_plan_slow_kernel plans
        and url_emit_slow_kernel emits.  url_slow holds for batches of at most
        kUrlMaxWaves groups (every wave then has one group and a region of at
        least kUrlWaveSlack > kImgCap bytes, so no region refuses an image)."""
        d = self.dispatch()
        sums = self.group_sums(cfg)
        big = np.zeros(self.n_groups, dtype=bool)
        if self.big:
            url_out, refs, arena, _ = self.oracle(cfg)
            for i in np.nonzero(url_out)[0]:
                t = arena[int(refs[i, 0]):int(refs[i, 0]) + int(refs[i, 1])].tobytes()
                if any(b"{" + nm + b"}" in t for nm in self.big):
                    big[i // WAVE] = True
        slow = 0
        for g in range(self.n_groups):
            fast = self.fused and d[g].listed and not big[g] and sums[g] <= K.kImgCap
            slow += int(sums[g] > 0 and (d[g].unplanned or not fast))
        return dict(url_unplanned=sum(int(x.unplanned) for x in d), url_slow=slow)


def tmpl_cap(L) -> int:
    """An output arena every template of the layout fits ({email} for "a@b.cc/": at most 4 bytes out per byte in)."""
    return int(4 * L.path[:, 1].astype(np.int64).sum() + 16 * L.n + 4096)


# ---------------------------------------------------------------------------
# paths

def letters(n, salt=0) -> bytes:
    """n lower-case letters, never all hex digits from two letters up."""
    return bytes(ord("a") + (salt + 7 * (i + 1)) % 26 for i in range(n))


def path_of(*segs, lead=True) -> bytes:
    return (b"/" if lead else b"") + b"/".join(segs)


def path_len(n, salt=0, seg=20, last=None) -> bytes:
    """A path of exactly n bytes of letter segments (at most `seg` bytes each) that
    stays as it is; last: its last segment."""
    out = b""
    tail = b"" if last is None else b"/" + last
    k = 0
    while len(out) + len(tail) < n:
        room = n - len(out) - len(tail) - 1
        out += b"/" + letters(min(seg, room), salt + k)
        k += 1
    out += tail
    assert len(out) == n, (n, len(out))
    return out


ORD = [(b"/api/v1/users/12345678", RAW), (b"/health", RAW), (b"/a/b/c", RAW), (b"/orders/2024-01-02/items", RAW),
       (b"static/app.css", RAW), (b"/u/jo@ex.io/p", RAW), (b"/", RAW), (b"/x/550e8400-e29b-41d4-a716-446655440000", RAW),
       (b"/img/abc.png", TARGET), (b"/v2/deadbeefdeadbeef/z", RAW), (b"/k/_-_/q", RAW), (b"/t?x=1/2", TARGET)]


def ordinary(k, salt=0):
    """k ordinary lanes (short generator-like paths, packed or 16-aligned)."""
    out = []
    for i in range(k):
        p, f = ORD[(i + salt) % len(ORD)]
        out.append(Lane(p, at=(16, 0) if (i + salt) % 3 == 0 else (1, 0), flags=f | (EQ if (i + salt) % 5 == 0 else 0),
                        kind=CLIENT if (i + salt) % 4 == 1 else SERVER))
    return out


def gate0(k, salt=0):
    """k lanes the gate skips: no method, an internal span, a target that is present and not empty."""
    kinds = [dict(flags=native.URL_PATH_RAW), dict(kind=INTERNAL), dict(flags=RAW | native.URL_TGT_STR)]
    return [Lane(None, **kinds[(i + salt) % 3]) for i in range(k)]


def grp(seam, before=3, fill="ordinary", salt=0):
    """A 64-lane group: `before` ordinary lanes, the seam lanes, then ordinary
    (or gate-0) lanes up to 64."""
    assert before + len(seam) <= WAVE, len(seam)
    rest = WAVE - before - len(seam)
    return ordinary(before, salt) + list(seam) + (ordinary(rest, salt + before) if fill == "ordinary" else gate0(rest, salt))


def wrap(groups, salt=0):
    """Ordinary groups around the seam groups; the last one is ragged."""
    return [ordinary(WAVE, salt)] + list(groups) + [ordinary(37, salt + 5)]


def sum_group(S, seam=None, first=()):
    """A group whose untouched paths put out exactly S bytes from few arena
    bytes: after the lanes of `first`, every lane is a prefix of one 100-byte
    path (the lanes share its bytes), so the output is free of the stage's size."""
    base = path_len(100, salt=3, seg=60)
    lanes = list(first)
    k = WAVE - len(lanes)
    assert k > 0 and 2 * k <= S <= 100 * k, S
    q, r = divmod(S, k)
    for j in range(k):
        ln = q + (1 if j < r else 0)
        lanes.append(Lane(base[:ln], at=(16, 0) if j == 0 else ("at", "base"), tag="base" if j == 0 else None,
                          seam=seam if j == 0 else None))
    return lanes


# ---------------------------------------------------------------------------
# staging (stage_dma, url_plan_slow_kernel, url_emit_slow_kernel)

def mixed_path(n, salt=0) -> bytes:
    """A path of exactly n bytes: letter segments with ids and dates among them."""
    cyc = [letters(30, salt), b"12345678", letters(17, salt + 1), b"2024-01-02", letters(41, salt + 2), b"a@b.cc"]
    out, k = b"", 0
    while len(out) + len(cyc[k % len(cyc)]) + 1 <= n - 45:
        out += b"/" + cyc[k % len(cyc)]
        k += 1
    return out + path_len(n - len(out), salt + 9)


def _g_stage(shift):
    def groups():
        lanes = []
        for j in range(WAVE):
            last = b"7" if j == WAVE - 1 else letters(3, j)
            p = b"/1234567" + path_len(40, j, seg=35, last=last) if j % 4 == 1 else path_len(48, j, seg=22 if j == WAVE - 1 else 21, last=last)
            lanes.append(Lane(p, at=(16, shift) if j == 0 else (1, 0), seam=f"p{j}" if j in (0, WAVE - 1) else None))
        return [lanes]
    return groups


def _g_gather(long_lane=None):
    def groups():
        a = [Lane(path_len(49 if j == long_lane else 40, j, last=b"7654321" if j % 7 == 0 else None), at=(64, 0),
                  seam="a0" if j == 0 else None) for j in range(WAVE)]
        b = [Lane(path_len(33, j, last=b"2024-01-02" if j % 5 == 0 else None), at=(64, 15), seam="b0" if j == 0 else None)
             for j in range(WAVE)]
        return [a, b]
    return groups


def _g_gather_sparse():
    MB = 1 << 20
    where = {0: MB + 3, 31: 2 * MB + 15, 32: 3 * MB, 63: 3 * MB + 4096 + 9}
    lanes = []
    for j in range(WAVE):
        if j in where:
            lanes.append(Lane(ORD[j % 4][0] + b"/" + letters(5, j) + b"/87654321", at=where[j], seam=f"s{j}"))
        elif j % 3 == 0:
            lanes.append(Lane(b"", at=(1, 0), flags=RAW | (EQ if j % 2 else 0)))     # gate 2, len == 0
        elif j % 3 == 1:
            lanes.append(Lane(None, flags=GATE1))
        else:
            lanes += gate0(1, j)
    return [lanes]


def _g_gather_rounds():
    out = []
    for total in (64, 65, 128, 129):
        per = 16 if total < 100 else 32
        lanes, k = [], 0
        for j in range(WAVE):
            if j % (WAVE // per) == 0:
                ln = 65 if (k == per // 2 and total % 2) else 64
                lanes.append(Lane(path_len(ln, j, last=b"1234567" if k % 3 == 0 else None), at=(4096 // per, 0),
                                  seam=f"r{total}" if k == 0 else None))
                k += 1
            elif j % 5 == 1:
                lanes.append(Lane(None, flags=GATE1))
            else:
                lanes += gate0(1, j)
        out.append(lanes)
    return out


def _g_slow_subsets():
    return [[Lane(path_len(96, j, last=b"1234567" if j % 3 == 0 else None), seam="two" if j == 0 else None) for j in range(WAVE)],
            [Lane(path_len(128, j, last=b"a@b.cc" if j % 3 == 0 else None), seam="three" if j == 0 else None)
             for j in range(WAVE)]]


def _g_slow_alone(n):
    def groups():
        return [[Lane(mixed_path(n, 1), seam="first")] + ordinary(WAVE - 1, 1),
                ordinary(WAVE - 1, 2) + [Lane(mixed_path(n + 7, 2), at=(1, 0), seam="last")]]
    return groups


def _g_slow_img():
    long = Lane(b"/" + letters(K.win_seg + 1), seam="long")
    return [sum_group(K.kWaveOut - 66, first=[long]), sum_group(K.kWaveOut + 1 - 66, first=[long]),
            sum_group(K.kWaveOut - 1 - 66, first=[long])]


# ---------------------------------------------------------------------------
# enumeration (plan_group_list)

def _g_win():
    return [grp([Lane(path_len(192, 1, seg=50, last=b"12345678"), at=(32, 0), seam="w192.0"),
                 Lane(path_len(193, 2, seg=50, last=b"12345678"), at=(32, 0), seam="w193.0"),
                 Lane(path_len(161, 3, seg=50, last=b"2024-01-02"), at=(32, 31), seam="w192.31"),
                 Lane(path_len(162, 4, seg=50, last=b"2024-01-02"), at=(32, 31), seam="w193.31")])]


def _g_slash():
    a, b = letters(62, 1), letters(63, 2)
    return [grp([Lane(b"/" + a + b"/x", at=(32, 0), seam="s63"), Lane(b"/" + b + b"/x", at=(32, 0), seam="s64"),
                 Lane(b"/" + a + b"/" + b + b"/1234567", at=(32, 0), seam="s127"),
                 Lane(b"/" + b + b"/" + b + b"/x", at=(32, 0), seam="s128"),
                 Lane(b"/" + a + b"/" + b + b"/" + b + b"/", at=(32, 0), seam="s191"),
                 Lane(b"////", seam="only"), Lane(b"/a/b/", seam="trail"), Lane(b"a/123456789", seam="nolead.t"),
                 Lane(b"a/b", seam="nolead.u")])]


def _g_qm():
    a, b = letters(62, 3), letters(63, 4)
    one = [(b"?x=1/2", "n0"), (b"/?x=1", "n1"), (b"/" + a + b"?/9999999", "q63"), (b"/" + b + b"?/9999999", "q64")]
    two = [(b"/" + a + b"/" + b + b"?/a/1234567", "q127"), (b"/" + b + b"/" + b + b"?/a/1234567", "q128"),
           (path_len(250, 5, seg=60) + b"?" + b"/1234567" * 3, "far"), (b"/a/b?c?d/1234567", "two"), (b"/a/1234567", "none"),
           (b"/a?/1234567/x", "slash")]
    out = []
    for cases in (one, two):
        lanes = []
        for p, name in cases:
            lanes.append(Lane(p, at=(32, 0), flags=TARGET, seam=name))
            lanes.append(Lane(p, at=(32, 0), flags=RAW, seam=name + ".raw"))
        if cases is two:
            # a non-window path without a '?' whose last segment stays; digits that would make it an id and a
            # '?' are laid right after it, for 200 and 225 inside the last 32-byte window first_of reads
            # (`& low_mask(e - a)`), for 223 and 224 in the window after it
            for ln in (200, 223, 224, 225):
                lanes.append(Lane(path_len(ln, ln, seg=60), at=(32, 0), flags=TARGET, after=b"1234567?",
                                  seam=f"far.none{ln}"))
        out.append(grp(lanes, fill="gate0" if cases is two else "ordinary"))
    return out


def _g_segcap():
    out = []
    for total in (64, 65, 128, 129, 192, 193):
        per, extra = divmod(total, WAVE)
        lanes = []
        for j in range(WAVE):
            k = per + (1 if j == 10 and extra else 0)
            segs = [b"12" if (j + s) % 3 == 0 else letters(1 + (j + s) % 3, j + s) for s in range(k)]
            lanes.append(Lane(path_of(*segs), at=(1, 0) if j % 2 else (16, 0), seam=f"t{total}" if j == 0 else None))
        out.append(lanes)
    return out


def _g_seg6465():
    stay, over = [], []
    for a in (0, 1, 31):
        at = (32, (a - 1) % 32)
        stay.append(Lane(b"/" + letters(K.win_seg, a), at=at, after=b"a", seam=f"stay@{a}"))
        stay.append(Lane(b"/" + (b"a1b2c3d4e5f6a7b8" * 4)[:K.win_seg], at=at, after=b"f", seam=f"hex@{a}"))
        over.append(Lane(b"/" + letters(K.win_seg + 1, a), at=at, after=b"a", seam=f"long@{a}"))
        # 64 bytes without a letter, then one: the 65th byte decides (it stays)
        over.append(Lane(b"/" + b"-_" * (K.win_seg // 2) + b"a", at=at, after=b"-", seam=f"longnl@{a}"))
    return [grp(stay), grp(over)]


FOLD = [(n, t) for n in (1, 7, 8, 9, 16, 17) for t in sorted({0, n - 1, 7, 8, 15, 16}) if t < n]


def _fold_lanes(ns):
    lanes = []
    for n, t in FOLD:
        if n not in ns:
            continue
        segs = [b"1234567" if s == t else letters(2 + s % 2, s + n) for s in range(n)]
        lanes.append(Lane(path_of(*segs), at=(1, 0) if (n + t) % 2 else (16, 0), seam=f"f{n}.{t}"))
    if 17 in ns:
        segs = [b"2024-01-02" if s >= 15 else letters(2, s) for s in range(17)]
        lanes.append(Lane(path_of(*segs), seam="f17.15+16"))
    return lanes


def _g_fold():
    """nseg up to 9 among ordinary lanes; 16 and 17 assembled fast, and again in
    groups whose image is over kImgCap (45 lanes sharing one 110-byte path),
    where p.code, p.slow and emit_path's re-classification decide the bytes."""
    base = path_len(110, salt=3, seg=60)

    def over(ns):
        lanes = _fold_lanes(ns)
        lanes += [Lane(base, tag="base", seam="over")] + [Lane(base, at=("at", "base")) for _ in range(44)]
        return lanes + gate0(WAVE - len(lanes))
    return [grp(_fold_lanes((1, 7, 8, 9))), grp(_fold_lanes((16,)), fill="gate0"), grp(_fold_lanes((17,)), fill="gate0"),
            over((16,)), over((17,))]


def _g_gates():
    mix = [Lane(b"/secret/12345678", flags=native.URL_PATH_RAW, seam="nomethod"),
           Lane(b"/secret/12345678", kind=INTERNAL, seam="internal"),
           Lane(b"/secret/12345678", flags=RAW | native.URL_TGT_STR, seam="tgt.str"),
           Lane(b"/secret/12345678", flags=RAW | native.URL_TGT_NONSTR | EQ, seam="tgt.nonstr"),
           Lane(b"/secret/12345678", flags=GATE1, seam="gate1"), Lane(None, flags=GATE1, kind=CLIENT, seam="gate1.nopath"),
           Lane(b"", flags=RAW, seam="len0"), Lane(b"", flags=RAW | EQ, seam="len0.eq"),
           Lane(b"/a/1234567", flags=RAW | EQ, seam="eq"), Lane(None, flags=HAS, seam="path.none")]
    return [grp(mix * 3), ordinary(WAVE, 3), gate0(WAVE), ordinary(WAVE, 4)]


# ---------------------------------------------------------------------------
# classification (classify_spec, classify_win): (label, segment, the bytes that
# would flip the verdict if the segment's mask leaked them)

DATES = [b"2024-01-02", b"2024-01-02Z", b"2024-01-02+0530", b"2024-01-02T10:20", b"2024-01-02T10:20Z", b"2024-01-02T10:20:30",
         b"2024-01-02T10:20:30Z", b"2024-01-02T10:20+0530", b"2024-01-02T10:20:30-0530"]
WRONG = {ord("-"): b"_", ord("T"): b"t", ord(":"): b";", ord("+"): b"*", ord("Z"): b"z"}
UUID_S = b"a50e84f0-e29b-41d4-a716-4466b544c0d0"
HEX_S = b"a1b2c3d4e5f6a7b8" * 4


def _date_cases():
    out = []
    for v in DATES:
        L = len(v)
        out.append((f"date.{L}", v, b"T10:20"))
        for q, c in enumerate(v):
            if c in WRONG:
                out.append((f"date.{L}.p{q}", v[:q] + WRONG[c] + v[q + 1:], b"0"))
        for m in re.finditer(rb"[0-9]+", v):
            q = (m.start() + m.end()) // 2
            out.append((f"date.{L}.d{q}", v[:q] + b"a" + v[q + 1:], b"0"))
        out.append((f"date.{L}-1", v[:-1], v[-1:]))
        out.append((f"date.{L}+1", v + b"0", b"0"))
    out.append(("date.zone3", b"2024-01-02+053", b"0"))
    out.append(("date.zone5", b"2024-01-02+05300", b"0"))
    return out


def _cases():
    c = {}
    c["date"] = _date_cases()
    c["hex"] = [(f"hex.{n}", HEX_S[:n], b"a") for n in (14, 15, 16, 17, 18, 64)] + \
               [("hex.16g", HEX_S[:5] + b"g" + HEX_S[6:16], b"a"), ("hex.mixed", b"A1b2C3d4E5f6A7b8", b"a")]
    c["digits"] = [("digits.6", b"ab123456cd", b"7"), ("digits.7", b"ab1234567cd", b"7"),
                   ("digits.7end64", letters(57, 2) + b"1234567", b"8"), ("digits.6end64", letters(58, 2) + b"123456", b"7"),
                   ("digits.split", b"ab1234/567cd", b"7")]
    c["uuid"] = [("uuid.36", UUID_S, b"-"), ("uuid.37pre", b"x" + UUID_S, b"a"), ("uuid.37suf", UUID_S + b"x", b"a"),
                 ("uuid.64end", letters(28, 5) + UUID_S, b"a"), ("uuid.64start", UUID_S + letters(28, 5), b"a"),
                 ("uuid.mid", b"x" + UUID_S + b"y", b"a"), ("uuid.dash", UUID_S[:8] + b"e-" + UUID_S[10:], b"a"),
                 ("uuid.35", UUID_S[:-1], UUID_S[-1:])]
    c["email"] = [("email.at0", b"@b.cc", b"c"), ("email.two", b"a@b@c.dd", b"d"), ("email.dot0", b"a@.cc", b"c"),
                  ("email.dot1", b"a@b.cc", b"1"), ("email.tld1", b"a@b.c", b"c"), ("email.tld.digit", b"a@b.c1", b"c"),
                  ("email.pct", b"a@b%.cc", b"c"), ("email.64", letters(59, 6) + b"@b.cc", b"1"),
                  ("email.local", b"a.b_c%d+e-f@g-h.i.jk", b"1")]
    c["noletters"] = [("noletters.dash", b"-", b"a"), ("noletters.under", b"_", b"a"), ("noletters.pct", b"%20", b"a"),
                      ("noletters.one", b"1", b"a"), ("noletters.empty", b"", b"a")]
    c["fffd"] = [("fffd.v2", b"ab\xc3\xa9", b"\x80"), ("fffd.v3", b"ab\xe2\x82\xac", b"\x80"),
                 ("fffd.v4", b"ab\xf0\x9f\x98\x80", b"\x80"), ("fffd.t2", b"ab\xc3", b"\xa9"), ("fffd.t3", b"ab\xe2\x82", b"\xac"),
                 ("fffd.t4", b"ab\xf0\x9f\x98", b"\x80"), ("fffd.e080", b"a\xe0\x80\x80b", b"a"),
                 ("fffd.eda0", b"a\xed\xa0\x80b", b"a"), ("fffd.f08f", b"a\xf0\x8f\x80\x80b", b"a"),
                 ("fffd.f490", b"a\xf4\x90\x80\x80b", b"a"), ("fffd.c0", b"a\xc0\x80b", b"a"), ("fffd.c1", b"a\xc1\x80b", b"a"),
                 ("fffd.f5", b"a\xf5\x80\x80\x80b", b"a"), ("fffd.ff", b"a\xffb", b"a"), ("fffd.cont", b"a\x80b", b"a"),
                 ("fffd.literal", b"a\xef\xbf\xbdb", b"a"), ("fffd.e9", b"caf\xc3\xa9s", b"a")]
    return c


CASES = _cases()
ALIGN = (0, 1, 31)


def _g_classify(family):
    def groups():
        lanes = []
        for label, seg, after in CASES[family]:
            for a in ALIGN:
                k = (a - 2) % 32 or 32
                p = b"/" + letters(k, a) + b"/" + seg      # from a 32-aligned offset the segment starts at row bit a
                lanes.append(Lane(p, at=(32, 0), after=after, seam=f"{label}@{a}"))
                lanes.append(Lane(p + b"/" + after + b"q", at=(32, 0), seam=f"{label}@{a}m"))
        out, cur, size = [], [], 0
        for ln in lanes:
            need = -(-(len(ln.path) + len(ln.after)) // 32) * 32
            if len(cur) == 44 or size + need > 2400:
                out.append(grp(cur, fill="gate0", salt=len(out)))
                cur, size = [], 0
            cur.append(ln)
            size += need
        out.append(grp(cur, fill="gate0", salt=len(out)))
        return out
    return groups


# ---------------------------------------------------------------------------
# assembly and copy

def _g_asm_tails():
    targets = [(b"/" + letters(L, L), L + 1, f"u{L}") for L in range(1, 18)] + \
              [(b"/1", 5, "id"), (b"/2024-01-02", 7, "date"), (b"/a@b.cc", 8, "email")]
    lanes = []
    for p, out, name in targets:
        s = (1 - out) % 8 or 8
        for _ in range(8):       # eight times, each a byte further on (mod 8) in the group's image
            lanes.append(Lane(p, at=(1, 0), seam=name))
            lanes.append(Lane(b"/" + letters(s - 1, out), at=(1, 0)))
    return [lanes[k:k + WAVE] for k in range(0, len(lanes), WAVE)]


def _g_img():
    return [sum_group(K.kImgCap - 1, "cap-1"), sum_group(K.kImgCap, "cap"), sum_group(K.kImgCap + 1, "cap+1")]


def _tiny(out, where=5):
    lanes = gate0(WAVE)
    seam = {1: [Lane(None, flags=GATE1)], 2: [Lane(None, flags=GATE1), Lane(None, flags=GATE1)], 3: [Lane(b"/ab")], 0: [],
            5: [Lane(b"/1")], 7: [Lane(b"/abcdef")], 6: [Lane(b"/abcde")]}[out]
    for k, ln in enumerate(seam):
        lanes[(where + 31 * k) % WAVE] = ln
    return lanes


TINY = (1, 1, 1, 1, 2, 3, 0, 5)


def _g_copy_tiny():
    return [_tiny(o, where=(0, 63, 5, 32)[k % 4]) for k, o in enumerate(TINY)] + [_tiny(7), _tiny(6), _tiny(5)] + \
           [sum_group(s) for s in (129, 129, 129, 131)]


REFS_CHUNK = 1024             # the chunk the refs.chunk layout is laid for
REFS_CHUNK_CAP = REFS_CHUNK * 8 * 8


def refs_chunk(cap, n_groups):
    """url_refs_chunk for a batch small enough that the plan grid is one wave
    per group, rounded up to whole workgroups of four waves."""
    waves = 4 * -(-n_groups // 4)
    return min(256 << 10, cap // 8 // waves) & ~15


def _g_refs_chunk():
    """Refs form, tmpl_cap = REFS_CHUNK_CAP, 8 plan waves: a wave's chunk is
    1024 bytes.  Images of 1024 (the chunk ends exactly at the image), 1023 and
    1009 (need 1024 as well), 1008 (16 bytes short of the chunk's end) and 1025
    bytes (need 1040: the wave takes exactly its size instead)."""
    return [sum_group(s, seam=f"c{s}") for s in (REFS_CHUNK, REFS_CHUNK - 1, REFS_CHUNK - 15, REFS_CHUNK - 16, REFS_CHUNK + 1)]


def _g_copy_rounds():
    """copy_round's carry: n16 == 64 with nchunk == 65 needs shift + sum > 1024
    with sum <= 1024 and shift <= 3, so of the sums 1009..1024 only 1022, 1023
    and 1024 can reach it (and 2046..2048 the second carry); the lower sums
    copy in 64 chunks whatever the shift and are not laid.  1022 at shift 1 is
    the (64, 64) case next to the seam."""
    return [_tiny(1), sum_group(1024), sum_group(1022), sum_group(1023), sum_group(2048), sum_group(2047)]


# ---------------------------------------------------------------------------
# names (the general instance with real custom ids)

def names_cfg(n, long_name=False):
    ids = [{"regexp": "^cid%03d$" % k, "template_name": "n%03d" % k} for k in range(n)]
    if long_name:
        ids[0]["template_name"] = "n" * 254      # "{name}" of 256 bytes: load_braced_names gives up (l > 255)
    return {"custom_ids": ids}


def _names(n, picks, long_name=False):
    """Custom id k has name id 3 + k (after id, date and email); the braced
    table holds name ids 0..14."""
    def build(name):
        groups = [grp([Lane(b"/x/cid%03d/y" % k, seam=f"id{3 + k}"), Lane(b"/cid%03d" % k, at=(1, 0), seam=f"id{3 + k}.only"),
                       Lane(b"/x/cid%03dz/y" % k, seam=f"id{3 + k}.near")], salt=k) for k in picks]
        return Layout(name, wrap(groups), seed=0x0D17 + n, cfg=names_cfg(n, long_name), fused=not long_name,
                      big=[b"n%03d" % k for k in picks if 3 + k >= K.code_ids])
    return build


# ---------------------------------------------------------------------------
# the registry

STAGING = {"stage.3072": _g_stage(0), "stage.3073": _g_stage(1), "gather.fit": _g_gather(), "gather.over1": _g_gather(20),
           "gather.sparse": _g_gather_sparse, "gather.rounds": _g_gather_rounds, "slow.subsets": _g_slow_subsets,
           "slow.alone": _g_slow_alone(K.kPlanStage + 28), "slow.alone4k": _g_slow_alone(K.kStage + 104),
           "slow.img4096": _g_slow_img}
ENUM = {"win.192/193": _g_win, "slash.halves": _g_slash, "qm": _g_qm, "segcap.192/193": _g_segcap, "seg.64/65": _g_seg6465,
        "fold.8/9": _g_fold, "gates": _g_gates}
CLASSIFY = {f"{f}": _g_classify(f) for f in CASES}
ASM = {"asm.tails": _g_asm_tails, "img.cap/over": _g_img, "copy.tiny": _g_copy_tiny, "copy.rounds": _g_copy_rounds,
       "refs.chunk": _g_refs_chunk}
GROUPS = {**STAGING, **ENUM, **CLASSIFY, **ASM}
NO_LEAD = {"slow.img4096", "copy.tiny", "copy.rounds"}       # laid from output offset 0
NAMES = {"names.15/16": _names(20, (10, 11, 12)), "names.64/65": _names(70, (60, 61)),
         "names.254/255": _names(260, (250, 251, 252)), "names.braced": _names(5, (0, 1), long_name=True)}
DIRTY = "dirty.then.seam"
DEFAULT_NAMES = list(GROUPS) + [DIRTY]

# a config that selects url_plan_kernel<1> and matches nothing
NEVER_CFG = {"custom_ids": [{"regexp": "^\x01never\x01$"}],
             "templatization_rules": ["/" + "/".join("lit%d" % k for k in range(40))]}


DIRTY_FF = (5, 40)        # the blocks whose second segment is a run of 0xFF


def dirty_lanes(variant):
    """A full kPlanStage stage of '/', '?', '@', digits, 0xFF and a few
    letters, 192 segments, and an image within 16 bytes of kImgCap (the image
    overlays the class bitmaps: it must cover all of their rows).  The stage is
    64 blocks of 48 bytes with slashes at +0 and +27; path j runs from block j
    74 or 75 bytes on, into block j + 1's first segment, so the paths share
    bytes and put out more than the stage holds; the last path runs from block
    62's second slash to the stage's end.  Every segment stays as it is but
    the two runs of 0xFF ({id}); the number of 75-byte paths is tuned to the
    image size with the Python restatement."""
    rng = np.random.default_rng(0x0D17D0 + variant)
    alpha = np.frombuffer(b"?@0123456789aZ-:.%+T_g??@@", dtype=np.uint8)

    def stays(n, also_short=False):
        while True:
            s = alpha[rng.integers(0, len(alpha), size=n)].tobytes()
            if reference_name(s) is None and not (also_short and reference_name(s[:-1]) is not None):
                return s
    block = bytearray()
    for j in range(WAVE):
        second = b"\xff" * 20 if j in DIRTY_FF else stays(20)
        block += b"/" + stays(26, also_short=True) + b"/" + second
    block = bytes(block)
    assert len(block) == K.kPlanStage

    def lanes(k75):
        out = [Lane(block[48 * j:48 * j + (75 if j < k75 else 74)], at=("rel", 48 * j)) for j in range(WAVE - 1)]
        return out + [Lane(block[48 * 62 + 27:], at=("rel", 48 * 62 + 27))]
    base = sum(len(py_template(ln.path, False)) for ln in lanes(0))
    k75 = K.kImgCap - 5 - base
    assert 0 <= k75 <= WAVE - 1, (base, k75)
    return lanes(k75)


def seam_kinds():
    """The enumeration, classification and assembly seam groups, one after another."""
    out = []
    for name in list(ENUM) + list(CLASSIFY) + list(ASM):
        out += [(f"{name}#{k}", g) for k, g in enumerate(GROUPS[name]())]
    return out


def _dirty():
    W = K.kUrlMaxWaves
    units = [Layout("dirty.unit", [dirty_lanes(v)], seed=1) for v in (0, 1)]
    blocks, paths = [], []
    for k in range(W):
        u = units[k % 2]
        blocks.append(u.arena[64:64 + K.kPlanStage])
        p = u.path.copy()
        p[:, 0] += K.kPlanStage * k
        paths.append(p)
    arena = np.concatenate([units[0].arena[:64]] + blocks)
    prefix = (arena, np.concatenate(paths), np.tile(units[0].flags, W), np.tile(units[0].kind, W))
    kinds = seam_kinds()
    groups = [kinds[k % len(kinds)][1] for k in range(W)]
    L = Layout(DIRTY, groups, seed=0x0D17DD, prefix=prefix)
    L.kinds = [k for k, _ in kinds]
    return L


_built = {}


def layout(name) -> Layout:
    """The named batch (built once; nothing writes to it)."""
    if name not in _built:
        if name == DIRTY:
            _built[name] = _dirty()
        elif name in NAMES:
            _built[name] = NAMES[name](name)
        else:
            g = GROUPS[name]()
            g = g + [ordinary(37, 5)] if name in NO_LEAD else wrap(g)
            _built[name] = Layout(name, g, seed=0x0D1700 + sum(map(ord, name)))
    return _built[name]
