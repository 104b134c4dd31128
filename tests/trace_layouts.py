"""Hand-laid batches for the trace stage (tests/test_sampling_layouts.py).

A batch is a list of segments (a trace label, a position, a length and
per-span choices: the resource's service, zero starts, ERROR statuses, routes
with or without a rule's prefix, early / late start times) over a filler of
short random traces from a seeded numpy generator.  Everything the trace
stage reads is built here in numpy, the way SqlBatch (tests/test_sqlop.py)
builds the SQLOP columns.  Test infrastructure only.

The constants a layout is laid against are parsed from kernels.hpp,
trace_kernel.hip and sampling_host.cpp at import (K); DESIGNED pins the
values the layouts were drawn for, and test_constants_as_designed fails when
one is retuned, so a layout cannot slide off its seam unnoticed.
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
    hpp = (CSRC / "kernels.hpp").read_text()
    hip = (CSRC / "trace_kernel.hip").read_text()
    host = (CSRC / "sampling_host.cpp").read_text()

    def const(text, name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\w+)\s*;" % name, text)
        assert m, f"{name}: definition not found"
        v = m.group(1)
        if not v.isdigit():   # a macro with a default (#define OSE_LONG_PIECE 2048)
            d = re.search(r"#define\s+%s\s+(\d+)" % v, text)
            assert d, f"{name} = {v}: no #define default found"
            v = d.group(1)
        return int(v)

    k = SimpleNamespace()
    for name in ("kMaxRuns", "kMaxFoldSpans", "kMaxFoldSlots", "kWinPerWave", "kWinPerWaveBeside", "kLongPiece",
                 "kLongSteps", "kDupBucketCap"):
        setattr(k, name, const(hpp, name))
    for name in ("kQ", "kHeadQ", "kPlanWaves"):
        setattr(k, name, const(hip, name))
    # a.win_per_wave = min(cap, max(1, n_windows / D))
    m = re.search(r"a\.win_per_wave\s*=\s*\(uint32_t\)std::min<uint64_t>\(wpw_cap,\s*std::max<uint64_t>\(1,\s*"
                  r"a\.n_windows\s*/\s*(\d+)\)\);", host)
    assert m, "sampling_host.cpp: the win_per_wave formula changed; trace_layouts.win_per_wave must follow it"
    k.wpw_div = int(m.group(1))
    assert re.search(r"wpw_cap\s*=\s*ws->beside_url\s*\?\s*kWinPerWaveBeside\s*:\s*kWinPerWave;", host), \
        "sampling_host.cpp: the win_per_wave cap changed"
    # the fingerprint buckets' sizing (Workspace::reserve_table)
    assert re.search(r"while\s*\(\(uint64_t\(kDupBucketCap\)\s*/\s*2\s*<<\s*dup_bkt_bits\)\s*<\s*n_spans\s*/\s*4\)\s*"
                     r"dup_bkt_bits\+\+;", host), "sampling_host.cpp: the bucket sizing rule changed"
    # the hand-off test of trace_eval_kernel
    assert "base >= range_end + (uint64_t)a.long_steps * kWave" in hip, "trace_kernel.hip: the hand-off test changed"
    return k


K = _parse_constants()
DESIGNED = dict(kQ=64, kHeadQ=128, kLongSteps=4, kLongPiece=2048, kPlanWaves=16, kMaxRuns=8, kMaxFoldSpans=4096,
                kMaxFoldSlots=8, kDupBucketCap=1024, kWinPerWave=16, wpw_div=4096)


def win_per_wave(n: int) -> int:
    """Windows one wave owns in a SAMPLE-only call of n spans (sampling_host.cpp)."""
    n_windows = max(1, (n + 63) // 64)
    return min(K.kWinPerWave, max(1, n_windows // K.wpw_div))


def n_for(W: int) -> int:
    """The smallest batch that runs W windows per wave."""
    return (W * K.wpw_div - 1) * WAVE + 1 if W > 1 else 1


def dup_bucket_slots(n: int) -> int:
    """Fingerprints the buckets of a fresh engine hold for an n-span batch."""
    bits = 1
    while (K.kDupBucketCap // 2 << bits) < n // 4:
        bits += 1
    return K.kDupBucketCap << bits


# ---------------------------------------------------------------------------
# services and routes (C3 numbering: svc-NN <-> NN, tests/workloads.py)

A, B, N = 4, 5, 20        # two latency services of the C3 config and one with no rule
LAT8 = [4, 5, 6, 7, 8, 9, 10, 11]    # kMaxFoldSlots latency services of C3 (none with a service_name rule)
ROUTES = ["/api/v1/users/{id}", "/api/v2/orders", "/api/items", "/health/live", "/a", "/x/y", "zzz/none", ""]
NO_PREFIX = 6             # carries no rule's prefix in any config of the suite
T0 = 1_700_000_000_000_000_000
LATE = 1_000_000_000      # a late span starts a second after an early one
DUR = 40_000_000          # and lasts 40 ms: below every C3 threshold


def lat_services(cfg) -> dict:
    """{raw service number: [http_route prefixes]} of a config's latency rules."""
    out = {}
    for lvl in ("global_rules", "service_rules", "endpoint_rules"):
        for r in cfg.get(lvl) or []:
            if r["type"] == "http_latency":
                d = r["rule_details"]
                out.setdefault(int(d["service_name"][4:]), []).append(d["http_route"])
    return out


def _prefix_route(svc: int) -> int:
    """A route of ROUTES that carries the prefix of one of the C3 rules of svc."""
    from tests.workloads import c3_sampling_config
    pre = lat_services(c3_sampling_config()).get(svc)
    if not pre:
        return 0
    for k, r in enumerate(ROUTES):
        if any(r.startswith(p) for p in pre):
            return k
    raise AssertionError(f"no route for svc {svc}")


class Seg:
    """One run of a trace: `length` spans of trace `label` from position `at`.
    svc: a service number or [(service, spans), ...]; zero / error: span
    indices within the run with a zero start / an ERROR status (every other
    span has neither); route: True = every span carries a prefix of its
    service's rules, False = none does, None = the filler's draw; early: the
    first `early` spans start at T0 and the rest LATE after it, every span
    ending within DUR of the late start (None: the filler's draw)."""

    def __init__(self, label, at, length, svc=A, zero=(), error=(), route=True, early=None):
        self.label, self.at, self.length = label, int(at), int(length)
        self.svc = [(svc, self.length)] if isinstance(svc, int) else list(svc)
        assert sum(c for _, c in self.svc) == self.length, (label, self.svc, length)
        self.zero, self.error, self.route, self.early = tuple(zero), tuple(error), route, early
        assert all(0 <= z < self.length for z in self.zero + self.error)

    def shifted(self, by, suffix=""):
        return Seg(f"{self.label}{suffix}", self.at + by, self.length, self.svc, self.zero, self.error, self.route,
                   self.early)


def _mix(x):
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


FILL_BLOCK = 1 << 18


class Batch:
    """Host columns of a laid-out batch (numpy) and their ose_columns view."""

    def __init__(self, segs, n, seed, singles=False):
        """singles: the filler is single-span traces (distinct ids)."""
        segs = sorted(segs, key=lambda s: s.at)
        for s, t in zip(segs, segs[1:]):
            assert s.at + s.length <= t.at, f"segments {s.label} and {t.label} overlap"
        assert not segs or (segs[0].at >= 0 and segs[-1].at + segs[-1].length <= n), "segment outside the batch"
        self.n, self.seed, self.segs = int(n), seed, segs
        rng = np.random.default_rng(seed)
        Bn = min(n, FILL_BLOCK)
        # ---- the filler: a block of short traces, tiled ----
        lens = np.ones(Bn, dtype=np.int64) if singles else rng.integers(1, 9, size=Bn)
        ends = np.cumsum(lens)
        k = int(np.searchsorted(ends, Bn))
        lens = lens[:k + 1].copy()
        lens[-1] -= ends[k] - Bn
        starts = np.cumsum(lens) - lens
        nruns = len(lens)
        run_of = np.repeat(np.arange(nruns), lens)
        pos_in = np.arange(Bn) - starts[run_of]
        sa, sb, cut = rng.integers(0, 24, nruns), rng.integers(0, 24, nruns), rng.integers(1, 9, nruns)
        svc_b = np.where(pos_in < cut[run_of], sa[run_of], sb[run_of]).astype(np.uint32)
        status_b = rng.choice(np.array([0, 1, 2], dtype=np.uint8), p=[0.5, 0.47, 0.03], size=Bn)
        start_b = (T0 + rng.integers(0, 2_500_000_000, Bn)).astype(np.uint64)
        end_b = start_b + rng.integers(0, 200_000_000, Bn).astype(np.uint64)
        start_b[rng.random(Bn) < 0.01] = 0
        route_b = rng.integers(0, len(ROUTES), Bn)
        none_b = rng.random(Bn) < 0.02       # (per resource, read at its first span) service.name not a Str
        reps = -(-n // Bn)

        def tile(a):
            return np.tile(a, reps)[:n].copy()

        svc, status, start, end = tile(svc_b), tile(status_b), tile(start_b), tile(end_b)
        route_i, none = tile(route_b), tile(none_b)
        label = tile(run_of).astype(np.uint64) + np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(nruns), Bn)[:n]
        seg_before = np.zeros(n, dtype=np.uint64)
        boundary = np.zeros(n + 1, dtype=bool)
        in_seg = np.zeros(n, dtype=bool)
        # ---- the segments ----
        names = {}
        for s in segs:
            a, b = s.at, s.at + s.length
            seg_before[b:] += np.uint64(1)
            boundary[a] = boundary[b] = True
            in_seg[a:b] = True
            names.setdefault(s.label, len(names))
            label[a:b] = np.uint64((1 << 62) + names[s.label])
            sv = np.concatenate([np.full(c, v, dtype=np.uint32) for v, c in s.svc])
            svc[a:b] = sv
            status[a:b] = np.arange(a, b) % 2          # UNSET / OK
            for e in s.error:
                status[a + e] = native.STATUS_ERROR
            if s.early is not None:
                q = np.arange(s.length)
                start[a:b] = np.where(q < s.early, T0 + q, T0 + LATE + q).astype(np.uint64)
                end[a:b] = np.where(q < s.early, T0 + q + 1000, T0 + LATE + DUR - 1000 + q).astype(np.uint64)
            else:
                z = start[a:b] == 0
                start[a:b][z] = end[a:b][z]
            for zz in s.zero:
                start[a + zz] = 0
            if s.route is True:
                route_i[a:b] = np.array([_prefix_route(int(v)) for v, _ in s.svc]).repeat([c for _, c in s.svc])
            elif s.route is False:
                route_i[a:b] = NO_PREFIX
        # a filler run cut in two by a segment is two traces
        label = np.where(in_seg, label, (label << np.uint64(20)) + seg_before)
        self.n_labels = len(np.unique(label)) if n <= (1 << 20) else None     # (census: distinct labels, distinct ids)
        lo = _mix(label ^ np.uint64(seed & 0xFFFFFFFF))
        hi = _mix(lo ^ np.uint64(0xA5A5A5A55A5A5A5A))
        self.tid = np.ascontiguousarray(np.stack([hi, lo], axis=1))
        self.ids = {name: (int(_mix(np.array([(1 << 62) + k], dtype=np.uint64) ^ np.uint64(seed & 0xFFFFFFFF))[0]))
                    for name, k in names.items()}      # label -> the id's low word
        # ---- resources: a new one wherever the service changes (and at segment edges) ----
        change = np.ones(n, dtype=bool)
        change[1:] = (svc[1:] != svc[:-1]) | boundary[1:n]
        self.resource = (np.cumsum(change) - 1).astype(np.uint32)
        self.res_svc = np.ascontiguousarray(svc[change])
        self.res_svc_str = self.res_svc.copy()
        self.res_svc_str[none[change] & ~in_seg[change]] = native.OSE_NONE
        self.svc = svc
        self.status, self.start, self.end = status, start, end
        # ---- routes ----
        blob, offs = bytearray(), []
        for r in ROUTES:
            offs.append(len(blob))
            blob += r.encode()
            blob += b"\0" * ((-len(blob)) % 16 + 3)     # (odd alignments)
        self.arena_bytes = len(blob)
        self.arena = np.zeros((len(blob) + 15) // 16 * 16 + 32, dtype=np.uint8)
        self.arena[:len(blob)] = np.frombuffer(bytes(blob), dtype=np.uint8)
        self.route = np.ascontiguousarray(np.stack([np.array(offs, dtype=np.uint32)[route_i],
                                                    np.array([len(r) for r in ROUTES], dtype=np.uint32)[route_i]], axis=1))
        self.route_i = route_i
        self._bind()

    def _bind(self):
        c = native.Columns()
        c.n_spans, c.n_resources, c.arena_bytes = self.n, len(self.res_svc), self.arena_bytes
        for f, a in (("arena", self.arena), ("trace_id", self.tid), ("start_ns", self.start), ("end_ns", self.end),
                     ("status", self.status), ("resource", self.resource), ("route", self.route),
                     ("res_svc", self.res_svc), ("res_svc_str", self.res_svc_str)):
            assert a.flags["C_CONTIGUOUS"]
            setattr(c, f, a.ctypes.data)
        self.cols = c

    def cut(self, n):
        """The first n spans of this batch as a batch of its own."""
        import copy
        b = copy.copy(self)
        b.n = n
        b.segs = [s for s in self.segs if s.at + s.length <= n]
        for f in ("tid", "resource", "status", "start", "end", "route", "svc", "route_i"):
            setattr(b, f, np.ascontiguousarray(getattr(self, f)[:n]).copy())
        R = int(b.resource[-1]) + 1
        b.res_svc, b.res_svc_str = self.res_svc[:R].copy(), self.res_svc_str[:R].copy()
        b._bind()
        return b

    # ---- census: everything below reads the built columns alone ----
    def heads(self):
        h = np.ones(self.n, dtype=bool)
        h[1:] = (self.tid[1:] != self.tid[:-1]).any(axis=1)
        return h

    def runs(self):
        """(start positions, exclusive ends, trace index per run)"""
        hp, ends = self.run_bounds()
        _, tr = np.unique(self.tid[hp], axis=0, return_inverse=True)
        return hp, ends, tr.reshape(-1)

    def run_bounds(self):
        if getattr(self, "_rb", None) is None or self._rb[2] != self.n:
            hp = np.nonzero(self.heads())[0]
            self._rb = (hp, np.append(hp[1:], self.n), self.n)
        return self._rb[:2]

    def runs_of(self, label):
        """[(start, exclusive end)] of the runs of a segment label, in batch order."""
        hp, ends = self.run_bounds()
        m = self.tid[hp, 1] == np.uint64(self.ids[label])
        return list(zip(hp[m].tolist(), ends[m].tolist()))

    def repeated(self, lat=()):
        """[(runs, spans, latency services)] of every trace in more than one run."""
        hp, ends, tr = self.runs()
        nr = np.bincount(tr)
        out = []
        for t in np.nonzero(nr > 1)[0]:
            m = tr == t
            sv = np.concatenate([self.svc[a:b] for a, b in zip(hp[m], ends[m])])
            out.append((int(nr[t]), int((ends[m] - hp[m]).sum()), len(set(sv.tolist()) & set(lat))))
        return out

    def walk(self, W, w_lo=0, w_hi=None):
        """The fast pass's bookkeeping for the waves owning windows [w_lo, w_hi)
        at W windows per wave, restated from the columns: how the decide queue
        (kQ) and the head queue (kHeadQ) fill and flush, and which runs are
        handed to the long-run kernels.  Returns (events, handed, headless):
        events = {("q_exact",), ("q_over", by, carried_close), ("h_exact",),
        ("h_over", by, carried_close)}, handed = start positions, headless =
        ranges (first window) in which no trace starts."""
        hp, ends = self.run_bounds()
        n = self.n
        n_win = (n + 63) // 64
        w_hi = n_win if w_hi is None else min(w_hi, n_win)
        events, handed, headless = set(), [], []
        for w0 in range(w_lo // W * W, w_hi, W):
            a, b = w0 * WAVE, min((w0 + W) * WAVE, n)
            i0 = int(np.searchsorted(hp, a))
            if i0 == len(hp) or hp[i0] >= b:
                headless.append(w0)
                continue
            base = int(hp[i0]) // WAVE * WAVE
            qn = hn = 0
            open_run = None
            while True:
                in_range = base < b
                step_end = min(base + WAVE, n)
                j0, j1 = int(np.searchsorted(hp, base)), int(np.searchsorted(hp, step_end))
                carried = open_run is not None and ends[open_run] <= step_end
                nh = j1 - j0
                if in_range and nh:
                    if hn + nh > K.kHeadQ:
                        events.add(("h_over", hn + nh - K.kHeadQ, carried))
                        hn = 0
                    hn += nh
                    if hn == K.kHeadQ:
                        events.add(("h_exact",))
                if carried:
                    if qn == K.kQ:
                        events.add(("q_over", 1, True))
                        qn = 0
                    qn += 1
                    open_run = None
                nq = 0
                if in_range:
                    nq = int((ends[j0:j1] <= step_end).sum())
                    if j1 > j0 and ends[j1 - 1] > step_end:
                        open_run = j1 - 1
                if nq:
                    if qn + nq > K.kQ:
                        events.add(("q_over", qn + nq - K.kQ, carried))
                        qn = 0
                    qn += nq
                if qn == K.kQ:
                    events.add(("q_exact",))
                base += WAVE
                if open_run is None and base >= b:
                    break
                if open_run is not None and base >= b + K.kLongSteps * WAVE:
                    handed.append(int(hp[open_run]))
                    break
        return events, handed, headless

    def closes_per_step(self, w_lo, w_hi):
        _, ends = self.run_bounds()
        return np.bincount((ends - 1) // WAVE, minlength=w_hi)[w_lo:w_hi]

    def heads_per_step(self, w_lo, w_hi):
        hp, _ = self.run_bounds()
        return np.bincount(hp // WAVE, minlength=w_hi)[w_lo:w_hi]


# ---------------------------------------------------------------------------
# blocks: segments relative to the start of a wave's range (a multiple of
# 64 * W spans); a block's length is a multiple of the range too

def _round(x, R):
    return -(-x // R) * R


def step_block(W):
    """Step seams.  T1/T2/T5 fill exactly one, two and five steps (each ends
    at lane 63 with the next trace starting at lane 0; T1 opens at lane 0 of
    the range's first window); T63 opens at lane 63; TL opens at lane 0 of a
    range's last window and runs through the first W - 1 windows of the next
    range (W = 1: T5 covers whole ranges), which therefore hold no head."""
    R = WAVE * W
    segs = [Seg("T1", 0, 64, early=1), Seg("T2", 64, 128, [(A, 64), (B, 64)], early=65),
            Seg("T5", 192, 320, [(N, 100), (A, 220)], early=101, zero=(99,)),
            Seg("T63", 512 + 63, 10, [(A, 1), (B, 9)], early=2)]
    p = _round(512 + 64 + 10, R)
    segs.append(Seg("TL", p + R - 64, 64 + 64 * (W - 1) + 10, [(B, 64), (A, 64 * (W - 1) + 10)], early=65))
    return segs, _round(p + R + 64 * W + 10, R)


QUEUE_STEPS = [64, 1, 63, 2, 31, 33, 32, 32]


def queue_block(W):
    """Decide queue.  Steps in which 64, 1, 63, 2, 31, 33, 32 and 32 traces
    close (c - 1 single spans and one trace over the step's other lanes; the
    last step's 32 singles are followed by a trace QC that closes in the next
    step).  Waves of two windows take them in pairs: 64 + 1 (fills kQ
    exactly, overflows by one, nothing carried), 63 + 2, 31 + 33 (fills
    exactly, no flush), 32 + 32 then QC closing as the carried trace with the
    queue full."""
    segs, at = [], 0
    for k, c in enumerate(QUEUE_STEPS):
        last = k == len(QUEUE_STEPS) - 1
        for j in range(c - 1 if not last else c):
            segs.append(Seg(f"Q{k}.{j}", at + j, 1, svc=[A, B, N][j % 3], early=None))
        if last:
            segs.append(Seg("QC", at + c, 64 - c + 10, [(A, 20), (B, 64 - c - 10)], early=21))
        else:
            segs.append(Seg(f"Q{k}.t", at + c - 1, 64 - (c - 1), svc=[(A, 64 - (c - 1))], early=1 if c < 64 else None))
        at += 64
    return segs, _round(at + 64, WAVE * W)


def head_block(W):
    """Head queue.  64 + 64 heads fill kHeadQ exactly, then a step with one
    head (a 64-span trace) overflows it by one with nothing carried; again
    with the 128th head's trace HC closing as the carried trace in the
    overflowing step, whose only head is H2 (W >= 3: a wave of two windows
    counts at most 128 heads)."""
    segs = []
    for j in range(128):
        segs.append(Seg(f"Ha.{j}", j, 1, svc=[A, B, N][j % 3], early=None))
    segs.append(Seg("H1", 128, 64, early=1))
    at = _round(192, WAVE * W)
    for j in range(127):
        segs.append(Seg(f"Hb.{j}", at + j, 1, svc=[B, N, A][j % 3], early=None))
    segs.append(Seg("HC", at + 127, 11, [(A, 3), (B, 8)], early=3, zero=(2,)))
    segs.append(Seg("H2", at + 138, 54, early=1))
    return segs, _round(at + 192, WAVE * W)


ABA = [(A, 3), (B, 2), (A, 3)]
ABAB = [(A, 2), (B, 2), (A, 2), (B, 2)]
ANA = [(A, 3), (N, 2), (A, 3)]


def stretch_block(W):
    """Latency stretches.  Traces of 8 spans inside one step with services
    A B A, A B A B and A N A (N has no latency rule); the same as the part of
    a carried trace (opened at lane 50 of the step before) and of a trace left
    open (from lane 40, closing in the next step); zero starts in the first
    stretch, in the second A stretch, and in the first span of a carried
    trace's part of a step (and in its very first span).  Early spans make the
    decision depend on where minStart is reset (latency.go:69-73)."""
    segs, at = [], 0
    # step 0: closed inside the step
    segs += [Seg("S.aba", at + 4, 8, ABA, early=3), Seg("S.abab", at + 14, 8, ABAB, early=2),
             Seg("S.ana", at + 24, 8, ANA, early=3),
             Seg("S.aba.z1", at + 34, 8, ABA, early=2, zero=(1,)),       # zero in the first stretch: both early spans gone
             Seg("S.aba.z1k", at + 44, 8, ABA, early=3, zero=(1,)),      # ... an early span survives it
             Seg("S.aba.z2", at + 54, 8, ABA, early=3, zero=(5,))]       # zero opening the second A stretch
    # steps 1-2, 3-4, 5-6: carried traces whose part of the next step is the pattern
    for k, (name, pat) in enumerate((("aba", ABA), ("abab", ABAB), ("ana", ANA))):
        at = 64 + 128 * k
        segs.append(Seg(f"C.{name}", at + 50, 14 + 8, [(N, 14)] + pat, early=14 + pat[0][1]))
    # steps 7-8: the A stretch itself crosses the step
    segs.append(Seg("C.a|ba", 64 * 7 + 50, 14 + 5, [(A, 14), (B, 2), (A, 3)], early=14))
    # steps 9-10: zero start in the first span of the carried part / of the trace
    segs.append(Seg("C.z.part", 64 * 9 + 60, 4 + 6, early=4, zero=(4,)))
    segs.append(Seg("C.z.first", 64 * 10 + 60, 4 + 6, early=3, zero=(0,)))
    # steps 12-13, 14-15, 16-17: left open with the pattern in the opening step
    for k, (name, pat) in enumerate((("aba", ABA), ("abab", ABAB), ("ana", ANA))):
        at = 64 * 12 + 128 * k
        segs.append(Seg(f"O.{name}", at + 40, 24 + 10, [(v, 3 * c) for v, c in pat] + [(B, 10)], early=3 * pat[0][1]))
    segs.append(Seg("O.aba.z", 64 * 18 + 40, 24 + 10, [(A, 8), (N, 8), (A, 8), (B, 10)], early=16, zero=(16,)))
    return segs, _round(64 * 20, WAVE * W)


HANDOFF_ENDS = (K.kLongSteps * WAVE - 1, K.kLongSteps * WAVE, K.kLongSteps * WAVE + 1, (K.kLongSteps + 1) * WAVE)


def handoff_segs(W, lane_first, end_off, label="HO"):
    """Two runs, each from the first (or last) lane of a range of its own to
    range_end + end_off (exclusive): handed to the long-run kernels iff
    end_off > kLongSteps * 64.  The decision of `label` hangs on its last span
    (a zero start there satisfies the latency rule), that of `label'` on its
    first (the only early one).  Returns (segments, spans used)."""
    R = WAVE * W
    at = 0 if lane_first else R - 1
    ln = R + end_off - at
    step = _round(R + end_off + 1, R) + R
    return [Seg(label, at, ln, early=0, zero=(ln - 1,)), Seg(label + "'", step + at, ln, early=1)], 2 * step


def handoff_block(W):
    """Every hand-off run in turn, each in a range of its own."""
    segs, at = [], 0
    for lane_first in (True, False):
        for e in HANDOFF_ENDS:
            hs, ln = handoff_segs(W, lane_first, e, f"HO.{int(lane_first)}.{e}")
            segs += [s.shifted(at) for s in hs]
            at += ln
    return segs, at


BLOCKS = {"step": step_block, "queue": queue_block, "head": head_block, "stretch": stretch_block,
          "handoff": handoff_block}


def place(blocks, W, n, seed, where, extra=()):
    """One batch of n spans with the blocks laid one after another from each
    position of `where` (multiples of the range); returns (batch, {(block,
    position): (first window, last window)})."""
    segs, spans = [], {}
    for pk, p0 in enumerate(where):
        at = p0
        assert at % (WAVE * W) == 0
        for name in blocks:
            bs, ln = BLOCKS[name](W)
            segs += [s.shifted(at, f"@{pk}") for s in bs]
            spans[(name, pk)] = (at // WAVE, (at + ln) // WAVE)
            at += ln
    return Batch(segs + list(extra), n, seed), spans


# ---------------------------------------------------------------------------
# the W = 1 layouts: small batches, each named for the seam it holds

LEAD = 192          # filler before a block


def _rle(a):
    a = np.asarray(a)
    cut = np.nonzero(a[1:] != a[:-1])[0] + 1
    return [int(a[k]) for k in np.concatenate([[0], cut])]


def _of_block(name, ragged=0):
    def build():
        segs, ln = BLOCKS[name](1)
        n = LEAD + ln + 128 + ragged
        b = Batch([s.shifted(LEAD) for s in segs], n, seed=0x1A70 + sum(map(ord, name)) + ragged)
        b.block = (LEAD // WAVE, (LEAD + ln) // WAVE)
        b.expect = dict(run_list=0, sort=0, long_runs=int(name == "handoff"))
        return b
    return build


def _handoff(lane_first, end_off):
    def build():
        hs, ln = handoff_segs(1, lane_first, end_off)
        b = Batch([s.shifted(LEAD) for s in hs], LEAD + ln + 100, seed=0x1A80 + end_off + int(lane_first))
        b.expect = dict(run_list=0, sort=0, long_runs=int(end_off > K.kLongSteps * WAVE))
        return b
    return build


def _long(length, last=False):
    def build():
        n = LEAD + length if last else LEAD + length + 150
        assert not last or n % WAVE not in (0, 63)
        # L's decision hangs on its last span (a zero start there), M's on its first (the only early one)
        segs = [Seg("L", LEAD, length, [(A, length - 7), (B, 7)], early=0, zero=(length - 1,))]
        if not last:
            at = _round(LEAD + length + 20, WAVE)
            segs.append(Seg("M", at, length, [(A, length - 7), (B, 7)], early=1))
            n = at + length + 150
        b = Batch(segs, n, seed=0x1A90 + length)
        b.expect = dict(run_list=0, sort=0, long_runs=1)
        return b
    return build


LONG_RUN = (K.kLongSteps + 1) * WAVE + 10     # from lane 0 of a window: handed off at W = 1


def _long_many(count):
    def build():
        segs = [Seg(f"L{k}", LEAD + k * 448, LONG_RUN + 3 * k, [(A, LONG_RUN - 20), (B, 20 + 3 * k)],
                    early=LONG_RUN - 20 - k, zero=(LONG_RUN - 21 - 2 * k,)) for k in range(count)]
        b = Batch(segs, LEAD + count * 448 + 100, seed=0x1AA0 + count)
        b.expect = dict(run_list=0, sort=0, long_runs=1)
        return b
    return build


PIECES3 = 2 * K.kLongPiece + 1      # three pieces: [0, P), [P, 2P), [2P, 2P + 1)


def _long_marks():
    """Runs of three pieces with a zero start / an ERROR status in the first
    span of a piece, the last span of a piece, the middle piece only; Zc has
    no zero (satisfied), Zo an early span after the zero (satisfied)."""
    P = K.kLongPiece
    specs = [("Zc", dict(early=P)), ("Zf", dict(early=P, zero=(P,))), ("Zl", dict(early=P, zero=(P - 1,))),
             ("Zo", dict(early=P + 1, zero=(P - 1,))), ("Zm", dict(early=P + 400, zero=(P + 900,))),
             ("Ef", dict(early=0, error=(P,))), ("El", dict(early=0, error=(P - 1,))), ("Em", dict(early=0, error=(P + 900,)))]
    segs = [Seg(name, LEAD + k * (PIECES3 + 63), PIECES3, **kw) for k, (name, kw) in enumerate(specs)]
    b = Batch(segs, LEAD + len(specs) * (PIECES3 + 63) + 40, seed=0x1AB0)
    b.expect = dict(run_list=0, sort=0, long_runs=1)
    return b


def _repeat(name, runs, n=6000, sort=0, long_runs=0, singles=False):
    """runs: [(position, length, svc)] of one trace X."""
    def build():
        segs = [Seg("X", at, ln, svc, early=(1 if k == 0 else 0)) for k, (at, ln, svc) in enumerate(runs)]
        b = Batch(segs, n, seed=0x1AC0 + sum(map(ord, name)), singles=singles)
        b.expect = dict(run_list=1, sort=sort, long_runs=long_runs)
        return b
    return build


def _slots(k):
    # two runs that touch k latency services of C3 between them
    sv = (LAT8 + [12])[:k]
    return [(LEAD + 5, 2 * 5, [(v, 2) for v in sv[:5]]), (LEAD + 700, 2 * (k - 5), [(v, 2) for v in sv[5:]])]


def _dup_overflow():
    b = Batch([], 5000, seed=0x1AD0, singles=True)
    b.expect = dict(run_list=1, sort=0, long_runs=0)
    return b


HALF = K.kMaxFoldSpans // 2
LAYOUTS = {
    "step": _of_block("step"), "step.ragged1": _of_block("step", 1), "step.ragged63": _of_block("step", 63),
    "queue": _of_block("queue"), "head": _of_block("head"), "stretch": _of_block("stretch"),
    **{f"handoff.{'first' if f else 'last'}.{e}": _handoff(f, e) for f in (True, False) for e in HANDOFF_ENDS},
    **{f"long.{L}": _long(L) for L in (K.kLongPiece, K.kLongPiece + 1, 2 * K.kLongPiece, 2 * K.kLongPiece + 1,
                                      3 * K.kLongPiece + 1)},
    "long.last": _long(K.kLongPiece + 1, last=True),
    "long.17": _long_many(K.kPlanWaves + 1), "long.33": _long_many(2 * K.kPlanWaves + 1),
    "long.marks": _long_marks,
    "repeat.runs8": _repeat("runs8", [(LEAD + 300 * k + 7 * k, 3, A) for k in range(K.kMaxRuns)]),
    "repeat.runs9": _repeat("runs9", [(LEAD + 300 * k + 7 * k, 3, A) for k in range(K.kMaxRuns + 1)], sort=1),
    "repeat.spans4096": _repeat("spans4096", [(LEAD, HALF, A), (LEAD + HALF + 300, HALF, B)], n=5000, long_runs=1),
    "repeat.spans4097": _repeat("spans4097", [(LEAD, HALF, A), (LEAD + HALF + 300, HALF + 1, B)], n=5000, sort=1,
                                long_runs=1),
    "repeat.slots8": _repeat("slots8", _slots(K.kMaxFoldSlots)),
    "repeat.slots9": _repeat("slots9", _slots(K.kMaxFoldSlots + 1), sort=1),
    # (the order in which trace_runs_kernel lists a trace's runs is decided by
    # its atomics, not by the data: the runs are spread over windows that
    # different workgroups take, the last one in the batch's last windows, so
    # that trace_fold_kernel's sort of the list has something to do)
    "repeat.spread": _repeat("spread", [(64 * w + 61, 5, [(A, 2), (B, 3)]) for w in (3, 150, 301, 452, 603)]
                             + [(64 * 620 + 1, 3, A)], n=64 * 620 + 9),
    "repeat.first_long": _repeat("first_long", [(LEAD, LONG_RUN, A), (LEAD + 1000, 3, B)], long_runs=1),
    "dup.overflow": _dup_overflow,
}

_built = {}


def layout(name) -> Batch:
    """The named W = 1 batch (built once; nothing writes to it)."""
    if name not in _built:
        b = LAYOUTS[name]()
        assert win_per_wave(b.n) == 1, name
        _built[name] = b
    return _built[name]
