"""Hand-laid inputs for the trace-id exchange (tests/test_exchange_layouts.py).

Source side: span batches (tests/trace_layouts.py Seg / Batch, plus exact
start / end / status marks, span_attribute bits and route_match planes) laid
on the seams of shard_hist_kernel, shard_counts_kernel and
shard_scatter_kernel.  Owner side: raw record arrays for ose_shard_decide,
whose trace ids are searched (seeded) for a wanted bucket of
owner_bucket_kernel and slot of owner_fold_kernel's LDS table.  Test
infrastructure only.

The constants a layout is laid against are parsed from kernels.hpp,
trace_device.hpp, shard_kernel.hip and shard_host.cpp at import (K); DESIGNED
pins the values the layouts were drawn for, and test_constants_as_designed
fails when one is retuned.
"""
from __future__ import annotations

import re
from types import SimpleNamespace

import numpy as np

from odigos_amd import native
from tests import trace_layouts as tl
from tests.exchange_emul import INF, NONE24, XERR, XLAT, XRESET, RuleLayout, _splitmix, pack, xdt
from tests.trace_layouts import A, B, DUR, LATE, N, ROUTES, T0, WAVE, Batch, Seg

SEED = 0x5EED          # DeviceExchange.seed: the seed of every owner decision here


# ---------------------------------------------------------------------------
# constants, read from the sources

def _parse_constants() -> SimpleNamespace:
    hpp = (tl.CSRC / "kernels.hpp").read_text()
    dev = (tl.CSRC / "trace_device.hpp").read_text()
    hip = (tl.CSRC / "shard_kernel.hip").read_text()
    host = (tl.CSRC / "shard_host.cpp").read_text()
    k = SimpleNamespace()

    def const(text, name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, f"{name}: definition not found"
        v = 1
        for f in m.group(1).split("*"):      # a product of literals and constants parsed before
            f = f.strip().rstrip("u")
            v *= int(f) if f.isdigit() else getattr(k, f)
        setattr(k, name, v)

    for name in ("kXSteps", "kXChunk", "kXFixedWords", "kScanTileItems", "kOwnerCap", "kOwnerAvg", "kOwnerSlotWords"):
        const(hpp, name)
    const(dev, "kSortThreads")
    const(hip, "kOwnerTable")
    assert re.search(r"const uint64_t B = std::max<uint64_t>\(1, \(n_recv \+ kOwnerAvg - 1\) / kOwnerAvg\);", host), \
        "shard_host.cpp: owner_decide's bucket count changed; exchange_layouts.n_buckets must follow it"
    assert re.search(r"const uint32_t T = \(uint32_t\)\(\(n \+ kXChunk - 1\) / kXChunk\);", host), \
        "shard_host.cpp: ose_shard_pack's chunk count changed"
    assert "* 0x9E3779B1u) >> 23" in hip and "(h & 0xFFFFFFFFull) * n_buckets) >> 32" in hip, \
        "shard_kernel.hip: the owner's bucket / table hashes changed"
    return k


K = _parse_constants()
DESIGNED = dict(kXSteps=16, kXChunk=1024, kXFixedWords=5, kScanTileItems=1024, kSortThreads=256, kOwnerCap=256,
                kOwnerAvg=80, kOwnerSlotWords=8, kOwnerTable=512)
WAVES_PER_WG = K.kSortThreads // WAVE


def n_buckets(n_recv: int) -> int:
    """B of owner_decide (shard_host.cpp)."""
    return max(1, (n_recv + K.kOwnerAvg - 1) // K.kOwnerAvg)


def n_tiles(n: int) -> int:
    """Packing waves of ose_shard_pack."""
    return (n + K.kXChunk - 1) // K.kXChunk


# ---------------------------------------------------------------------------
# hashes (trace_device.hpp tid_hash; shard_kernel.hip owner_bucket_of and the fold's table slot)

def tid_hash(hi, lo):
    return _splitmix(np.asarray(hi, np.uint64) ^ _splitmix(np.asarray(lo, np.uint64)))


def owner_bucket_of(h, n_bkt: int):
    return (((np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)) * np.uint64(n_bkt)) >> np.uint64(32)).astype(np.int64)


def table_slot(h):
    x = ((np.asarray(h, np.uint64) >> np.uint64(32)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(23)).astype(np.int64)


def find_ids(seed: int, count: int, n_bkt: int = 1, bucket=None, not_bucket=None, slot=None, world: int = 1,
             owner=None, draws: int = 1 << 18) -> np.ndarray:
    """`count` trace ids [count, 2] (hi, lo) whose owner of `world`, bucket of
    `n_bkt` and table slot are the wanted ones; deterministic by seed."""
    rng = np.random.default_rng(seed)
    tid = rng.integers(1, 2**63, size=(draws, 2), dtype=np.int64).astype(np.uint64)
    h = tid_hash(tid[:, 0], tid[:, 1])
    ok = np.ones(draws, dtype=bool)
    if bucket is not None:
        ok &= owner_bucket_of(h, n_bkt) == bucket
    if not_bucket is not None:
        ok &= owner_bucket_of(h, n_bkt) != not_bucket
    if slot is not None:
        ok &= table_slot(h) == slot
    if owner is not None:
        ok &= ((h >> np.uint64(32)) % np.uint64(world)).astype(np.int64) == owner
    got = tid[ok][:count]
    assert len(got) == count, f"find_ids: {len(got)} of {count} ids in {draws} draws"
    return got


# ---------------------------------------------------------------------------
# configs

def c3():
    from tests.workloads import c3_sampling_config
    return c3_sampling_config()


def fractional():
    from tests.test_exchange import _fractional
    return _fractional(c3())


def c3_attr():
    """C3 and one span_attribute rule: its bit rides after the service rules'
    bits (last in the list, so that svc-NN keeps the id NN)."""
    cfg = c3()
    cfg["endpoint_rules"] = cfg["endpoint_rules"] + [
        {"name": "attr", "type": "span_attribute",
         "rule_details": {"service_name": "svc-attr", "attribute_key": "env", "condition_type": "string",
                          "operation": "equals", "expected_value": "prod", "sampling_ratio": 50.0}}]
    return cfg


def c3_lat0():
    """C3 and an http_latency rule on svc-00: a latency service with id 0."""
    cfg = c3()
    cfg["endpoint_rules"] = cfg["endpoint_rules"] + [
        {"name": "lat-svc0", "type": "http_latency",
         "rule_details": {"http_route": "/a", "service_name": "svc-00", "threshold": 60, "fallback_sampling_ratio": 0}}]
    return cfg


def latency3():
    from tests.workloads import wide_latency_config
    return wide_latency_config()


def chunk_configs(cname):
    """The rule chunks of a config as configs of their own (None: one chunk).
    latency3: the engine cuts the level-ordered list after 64 http_latency
    rules (test_chunk_counts: 64 + 64 + 22), so chunk 0 holds the error rule,
    the service rules and rules 0..63, chunks 1 and 2 latency rules only."""
    if cname != "latency3":
        return None
    cfg = config(cname)
    ep = cfg["endpoint_rules"]
    return [dict(cfg, endpoint_rules=ep[:64]), {"endpoint_rules": ep[64:128]}, {"endpoint_rules": ep[128:]}]


CONFIGS = {"c3": c3, "fractional": fractional, "c3_attr": c3_attr, "c3_lat0": c3_lat0, "latency3": latency3}
ONE_CHUNK = ("c3", "fractional", "c3_attr", "c3_lat0")
_cfgs = {}


def config(name):
    if name not in _cfgs:
        _cfgs[name] = CONFIGS[name]()
    return _cfgs[name]


# ---------------------------------------------------------------------------
# source side

LEAD = 128             # filler before a layout's first segment (two whole steps)
SENTINEL = 0xA5


class Src:
    """A source batch laid on a seam: the Batch, the world it is packed for,
    optional span_attribute bits, and whether the pack gets route_match
    instead of route + arena."""

    def __init__(self, b: Batch, world: int = 3, attr=None, planes: bool = False, **meta):
        self.b, self.world, self.attr, self.planes, self.meta = b, world, attr, planes, meta
        self.n = b.n
        self._pack = {}

    def svc_str(self):
        return self.b.res_svc_str[self.b.resource]

    def endpoint_bits(self, cfg, lay=None):
        """bit r = HasPrefix(route, prefix of latency rule r) && the rule's
        service is the span's (memoised per (service, route))."""
        lay = lay or RuleLayout(cfg)
        memo, out = {}, np.zeros(self.n, dtype=np.uint64)
        for i, (s, ri) in enumerate(zip(self.b.svc.tolist(), self.b.route_i.tolist())):
            if (s, ri) not in memo:
                rb, v = ROUTES[ri].encode(), 0
                for k, (ls, pre) in enumerate(lay.lat):
                    if ls == s and rb.startswith(pre):
                        v |= 1 << k
                memo[(s, ri)] = v
            out[i] = memo[(s, ri)]
        return out

    def route_match(self, cfg, lay=None):
        """What a caller would hand in as route_match: the endpoint bits, and on
        every third span the bits of the other services' rules as well (the
        pack keeps the span's own service's)."""
        lay = lay or RuleLayout(cfg)
        own = np.array([lay.slot_rules.get(k, 0) for k in range(len(lay.slot))] + [0], dtype=np.uint64)
        noise = np.uint64((1 << len(lay.lat)) - 1) & ~own[lay.slot_of(self.b.svc)]
        return self.endpoint_bits(cfg, lay) | np.where(np.arange(self.n) % 3 == 0, noise, np.uint64(0))

    def match_planes(self, cname):
        """[K, n]: plane k = the endpoint bits (planes: the route_match column)
        under rule chunk k's bit layout."""
        cfg = config(cname)
        ids = RuleLayout(cfg).ids
        lays = [RuleLayout(c, ids) for c in chunk_configs(cname) or [cfg]]
        return np.ascontiguousarray(np.stack([(self.route_match if self.planes else self.endpoint_bits)(cfg, lay)
                                              for lay in lays]))

    def pack(self, cname):
        """The numpy pack: (records in bucket order, counts, pack_pos)."""
        if cname not in self._pack:
            cfg, b = config(cname), self.b
            self._pack[cname] = pack(b.tid, b.start, b.end, b.status, b.svc, self.svc_str(), self.match_planes(cname),
                                     self.world, self.attr, cfg=cfg, chunk_cfgs=chunk_configs(cname))
        return self._pack[cname]

    def rec_of(self, cname, span):
        rec, _, pos = self.pack(cname)
        return rec[pos[span]]

    def columns(self, cname):
        """ose_columns of this source for a config, what must stay alive, and
        (planes) the [K, n] route_match planes to hand in instead of route + arena."""
        c = native.Columns.from_buffer_copy(self.b.cols)
        keep, planes = [], None
        if self.attr is not None:
            keep.append(np.ascontiguousarray(self.attr, np.uint64))
            c.attr_match, c.attr_match_words = keep[-1].ctypes.data, 1
        if self.planes:
            planes = self.match_planes(cname)
            c.route, c.arena, c.arena_bytes = None, None, 0
        return c, keep, planes


def span_heads(b: Batch, lat: set):
    """Record heads restated from the columns alone: a new trace id, a new
    latency service (services without a latency rule count as one), lane 0."""
    sv = np.where(np.isin(b.svc, sorted(lat)), b.svc.astype(np.int64), -1)
    h = np.ones(b.n, dtype=bool)
    h[1:] = (b.tid[1:] != b.tid[:-1]).any(axis=1) | (sv[1:] != sv[:-1])
    h |= np.arange(b.n) % WAVE == 0
    return h


def _times(b: Batch, a: int, e: int):
    """Plain times over [a, e): late starts, short durations, nothing zero."""
    q = np.arange(e - a, dtype=np.uint64)
    b.start[a:e] = np.uint64(T0 + LATE) + q
    b.end[a:e] = np.uint64(T0 + LATE + DUR // 2) + q


def _n(n):
    def build():
        segs = [Seg("E", n - 3, 3, [(A, 2), (B, 1)], early=1)] if n >= 3 else []
        return Src(Batch(segs, n, seed=0x2B00 + n), n=n)
    return build


def _step(kind):
    def build():
        if kind == "cross":
            segs = [Seg("X", LEAD + 60, 8, early=2)]
        elif kind == "full":
            segs = [Seg("F", LEAD, 64, early=1, zero=(5,), error=(40,))]
        else:
            segs = [Seg(f"S{j}", LEAD + j, 1, svc=[A, B, N][j % 3], early=None) for j in range(64)]
        return Src(Batch(segs, LEAD + 64 + 70, seed=0x2B10 + len(kind)))
    return build


ROW_MARKS = ("zero", "err", "min", "max")


def _row(s):
    """Seam between lanes s and s + 1 of a DPP row step.  R.end's tail is lane
    s and R.start's head lane s + 1; the four straddlers cover lanes s - 3 ..
    s + 4 (tail s + 4) with their one mark at or below lane s."""
    def build():
        segs = [Seg("R.end", LEAD + s - 5, 6, A, early=2), Seg("R.start", LEAD + s + 1, 6, B, early=2)]
        for k, m in enumerate(ROW_MARKS):
            segs.append(Seg(f"R.{m}", LEAD + 64 * (k + 1) + s - 3, 8, A, early=None))
        b = Batch(segs, LEAD + 64 * 5 + 40, seed=0x2B20 + s)
        at = {}
        for k, m in enumerate(ROW_MARKS):
            a = LEAD + 64 * (k + 1) + s - 3
            _times(b, a, a + 8)
            b.status[a:a + 8] = native.STATUS_OK
            at[m] = a
        b.start[at["zero"] + 1] = T0                      # an early start (lane s - 2) ...
        b.start[at["zero"] + 2] = 0                       # ... wiped by the zero start at lane s - 1
        b.status[at["err"] + 3] = native.STATUS_ERROR     # lane s
        b.start[at["min"]] = T0                           # lane s - 3
        b.end[at["max"] + 3] = T0 + 10 * LATE             # lane s
        return Src(b, seam=s, at=at)
    return build


def _head_svc():
    none = native.OSE_NONE
    segs = [Seg("AB", LEAD + 2, 4, [(A, 2), (B, 2)], early=1),
            Seg("AN", LEAD + 10, 4, [(A, 2), (N, 2)], early=1),
            Seg("NN", LEAD + 20, 8, [(0, 2), (1, 2), (N, 2), (none, 2)], early=1, error=(7,))]
    return Src(Batch(segs, LEAD + 100, seed=0x2B30))


def _aba():
    return Src(Batch([Seg("ABA", LEAD + 5, 8, tl.ABA, early=3)], LEAD + 100, seed=0x2B31), world=2)


def _zero(kind):
    z = {"first": (0,), "last": (5,), "mid": (2,), "all": tuple(range(6))}[kind]

    def build():
        return Src(Batch([Seg("Z", LEAD + 9, 6, A, zero=z, early=2)], LEAD + 100, seed=0x2B40 + len(kind)), zero=z)
    return build


def _chunk(n):
    def build():
        segs = [Seg("C", K.kXChunk - 4, min(n, K.kXChunk + 1) - (K.kXChunk - 4), [(A, 2), (B, n - K.kXChunk + 2)],
                    early=1)] if n > K.kXChunk else [Seg("C", n - 4, 4, [(A, 2), (B, 2)], early=1)]
        return Src(Batch(segs, n, seed=0x2B50 + n), n=n)
    return build


def _wg(n):
    def build():
        at = K.kXChunk * WAVES_PER_WG - 3
        segs = [Seg("W", at, min(6, n - at), early=2)]
        return Src(Batch(segs, n, seed=0x2B60 + n), n=n)
    return build


def _ranks(world):
    def build():
        return Src(Batch([Seg("X", LEAD + 60, 8, early=2)], 2100, seed=0x2B70 + world, singles=True), world=world)
    return build


def _hole(kind):
    def build():
        if kind == "one":     # one trace is the whole batch: one owner gets every record
            segs = [Seg("ONE", 0, 300, [(A, 100), (B, 100), (N, 50), (A, 50)], early=120, zero=(130,), error=(7,))]
            return Src(Batch(segs, 300, seed=0x2B80), world=64)
        # a dozen traces for 64 owners: interior owners with nothing
        segs = [Seg(f"H{j}", 20 * j, 20, [(A, 7), (B, 13)], early=3) for j in range(12)]
        return Src(Batch(segs, 240, seed=0x2B81), world=64)
    return build


def _scan(n):
    def build():
        segs = [Seg("X", n - 70, 70, [(A, 30), (B, 40)], early=31)]
        return Src(Batch(segs, n, seed=0x2B90 + n), world=64, n=n)
    return build


def _planes():
    segs, _ = tl.stretch_block(1)
    return Src(Batch([s.shifted(LEAD) for s in segs], LEAD + 64 * 20 + 30, seed=0x2BA0), planes=True)


def _attr():
    segs = [Seg("AT.first", LEAD + 3, 5, A, early=1), Seg("AT.last", LEAD + 20, 5, B, early=1),
            Seg("AT.none", LEAD + 30, 5, A, early=1)]
    b = Batch(segs, LEAD + 100, seed=0x2BB0)
    attr = np.zeros(b.n, dtype=np.uint64)
    attr[LEAD + 3] = 1
    attr[LEAD + 24] = 1
    return Src(b, attr=attr)


SOURCE = {
    **{f"n.{n}": _n(n) for n in (1, 63, 64, 65)},
    "step.cross": _step("cross"), "step.full": _step("full"), "step.singles": _step("singles"),
    **{f"row.{s}": _row(s) for s in (15, 31, 47)},
    "head.svc": _head_svc, "aba": _aba,
    **{f"zero.{k}": _zero(k) for k in ("first", "last", "mid", "all")},
    **{f"chunk.{n}": _chunk(n) for n in (K.kXChunk - 1, K.kXChunk, K.kXChunk + 1)},
    **{f"wg.{n}": _wg(n) for n in (K.kXChunk * WAVES_PER_WG, K.kXChunk * WAVES_PER_WG + 1)},
    **{f"ranks.{w}": _ranks(w) for w in (1, 2, 63, 64)},
    "ranks.hole.one": _hole("one"), "ranks.hole.interior": _hole("interior"),
    "scan.1024": _scan(K.kScanTileItems // 64 * K.kXChunk), "scan.1025": _scan(K.kScanTileItems // 64 * K.kXChunk + 1),
    "planes": _planes, "attr": _attr,
}
# the configs a layout is packed under.  latency3 (three rule chunks; every
# service 0..63 a latency service) leaves out head.svc, whose meaning is C3's
# service numbering, and attr (the chunked pack is restated without
# span_attribute bits)
SOURCE_CONFIGS = {name: (("c3_attr",) if name == "attr" else ("c3", "fractional") if name == "head.svc" else
                         ("c3", "fractional", "latency3")) for name in SOURCE}
_src = {}


def source(name) -> Src:
    if name not in _src:
        _src[name] = SOURCE[name]()
    return _src[name]


# ---- end to end: one laid batch cut into W rank batches -------------------

class RankSlice:
    """Spans [lo, hi) of a Batch as a source of its own (resources renumbered;
    the arena shared), with the Generator surface oracle_lib's concatenation
    reads (cols, array)."""

    def __init__(self, b: Batch, lo: int, hi: int):
        self.n = hi - lo
        c = native.Columns()
        self.a = {}
        if self.n:
            r0, r1 = int(b.resource[lo]), int(b.resource[hi - 1]) + 1
            self.a = dict(trace_id=b.tid[lo:hi].copy(), start_ns=b.start[lo:hi].copy(), end_ns=b.end[lo:hi].copy(),
                          status=b.status[lo:hi].copy(), resource=(b.resource[lo:hi] - np.uint32(r0)).copy(),
                          route=b.route[lo:hi].copy(), res_svc=b.res_svc[r0:r1].copy(),
                          res_svc_str=b.res_svc_str[r0:r1].copy(), arena=b.arena)
            c.n_spans, c.n_resources, c.arena_bytes = self.n, r1 - r0, b.arena_bytes
            for f, v in self.a.items():
                assert v.flags["C_CONTIGUOUS"]
                setattr(c, f, v.ctypes.data)
        self.cols = c

    def array(self, field):
        return self.a[field].view(np.uint8).reshape(-1) if field in self.a else np.zeros(0, np.uint8)


def e2e_batch(W: int):
    """(batch, cut positions): the stretch and step blocks, the zero-start and
    service-change segments and, across every cut between two ranks, a trace
    A A | A B B whose latency stretch the cut divides.  W = 64: 300 spans a rank."""
    per = 300 if W == 64 else 1500
    n = W * per - (7 if W != 64 else 0)
    cuts = [k * per for k in range(1, W)]
    segs = [s.shifted(LEAD) for s in tl.stretch_block(1)[0]] if W != 64 else \
        [Seg("S.aba", LEAD + 4, 8, tl.ABA, early=3), Seg("S.z", LEAD + 20, 6, A, zero=(2,), early=2)]
    for k, c in enumerate(cuts):
        segs.append(Seg(f"CUT{k}", c - 2, 5, [(A, 3), (B, 2)], early=(2 if k % 2 else 0), zero=((3,) if k % 3 == 0 else ())))
    # one trace with a piece on the first and on the last rank: the owner folds across sources
    segs.append(Seg("FAR", per - 40, 4, A, early=0))
    segs.append(Seg("FAR", n - 30, 4, A, early=4))
    return Batch(segs, n, seed=0x2BC0 + W), cuts


def rank_slices(b: Batch, cuts):
    edges = [0] + list(cuts) + [b.n]
    return [RankSlice(b, lo, hi) for lo, hi in zip(edges, edges[1:])]


# ---------------------------------------------------------------------------
# owner side: raw records

C3_LAT = sorted(tl.lat_services(c3()))


class Recs:
    """Records under construction (one-chunk fields; chunk k >= 1 words by name)."""

    def __init__(self, chunks=1):
        self.chunks, self.rows = chunks, []

    def add(self, tid, sv=None, m=None, e=0, err=False, reset=False, ep=0, svcb=0, lat=None, **more):
        lat = (sv is not None) if lat is None else lat
        flags = (XERR if err else 0) | (XLAT if lat else 0) | (XRESET if reset else 0)
        row = dict(hi=int(tid[0]), lo=int(tid[1]), m=int(INF) if m is None else int(m), e=int(e),
                   w4=(NONE24 if sv is None else int(sv)) | (flags << 24), ep=int(ep), svcb=int(svcb))
        row.update(more)
        self.rows.append(row)
        return len(self.rows) - 1

    def array(self, order=None):
        r = np.zeros(len(self.rows), dtype=xdt(self.chunks))
        for k, row in enumerate(self.rows):
            for f, v in row.items():
                r[k][f] = v
        return r if order is None else r[np.asarray(order)]


def _rand_rec(rng, lay: RuleLayout, out: Recs, tid):
    """A well-formed record of a C3-numbered config: endpoint bits only of its
    own service's rules, times set only on a latency record."""
    svcb = int(rng.integers(0, 16)) if rng.random() < 0.1 else 0
    err = rng.random() < 0.03
    if rng.random() < 0.25:
        return out.add(tid, None, None, 0, err=err, svcb=svcb)
    sv = int(rng.choice(C3_LAT))
    reset = rng.random() < 0.15
    m = None if reset and rng.random() < 0.4 else T0 + int(rng.integers(0, 2 * LATE))
    e = (T0 if m is None else m) + int(rng.integers(0, 2 * LATE))
    ep = int(rng.integers(0, 1 << 20)) & lay.slot_rules[lay.slot[sv]]
    return out.add(tid, sv, m, e, err=err, reset=reset, ep=ep, svcb=svcb)


def _filler(rng, lay, out: Recs, ids, count):
    """`count` records over the traces `ids`, each record's trace drawn at
    random: traces in several pieces, their services in any order."""
    return [_rand_rec(rng, lay, out, ids[int(rng.integers(0, len(ids)))]) for _ in range(count)]


def _merge(rng, first, second):
    """An order of first + second that keeps each list's own order and
    interleaves the two at random."""
    take = np.zeros(len(first) + len(second), dtype=bool)
    take[rng.choice(len(take), size=len(first), replace=False)] = True
    a, b = iter(first), iter(second)
    return [next(a) if t else next(b) for t in take]


class Owner:
    """Records for ose_shard_decide: recv (structured), the config, what the
    layout is about (target: indices of its records in recv) and whether the
    fold must fall back (general)."""

    def __init__(self, recv, cname="c3", general=False, chunks=1, **meta):
        self.recv, self.cname, self.general, self.chunks, self.meta = recv, cname, general, chunks, meta
        self.n = len(recv)
        self.B = n_buckets(self.n)
        h = tid_hash(recv["hi"], recv["lo"])
        self.bucket = owner_bucket_of(h, self.B)
        self.slot = table_slot(h)
        self.counts = np.bincount(self.bucket, minlength=self.B)
        self._oracle = None

    def bytes(self):
        return np.ascontiguousarray(self.recv).view(np.uint8).reshape(-1)

    def oracle(self):
        """keep per record: the oracle on the expanded records (one-chunk configs)."""
        if self._oracle is None:
            self._oracle = oracle_keep(self.recv, config(self.cname))
        return self._oracle


def oracle_keep(recv, cfg):
    from odigos_amd.batch import HostOutputs
    from tests.exchange_emul import expand_for_oracle
    from tests.oracle_lib import SamplingOracle
    hc, main = expand_for_oracle(np.ascontiguousarray(recv).view(np.uint8).reshape(-1), cfg)
    ho = HostOutputs(hc.cols)
    assert SamplingOracle(cfg).process(hc.cols, ho.outs, native.GROUP_TRACE_ID, SEED, 1) == 0
    return ho.view("keep", np.uint8)[main].copy()


def _lay(cname="c3"):
    return RuleLayout(config(cname))


def _b(n):
    def build():
        rng = np.random.default_rng(0x3C00 + n)
        out = Recs()
        _filler(rng, _lay(), out, find_ids(0x3C00 + n, 30), n)
        return Owner(out.array())
    return build


def _in_bucket(seed, n, target_count, bucket, make_target, cname="c3", extra=0):
    """n records for B = n_buckets(n + extra) buckets: `target_count` records
    made by make_target(rng, out, ids_of(count)) in `bucket`, the rest filler
    in the other buckets, interleaved."""
    Bn = n_buckets(n + extra)
    rng = np.random.default_rng(seed)
    out = Recs()
    tgt = make_target(rng, out, lambda c, **kw: find_ids(seed + 1, c, Bn, bucket=bucket, **kw))
    assert len(tgt) == target_count
    fill = _filler(rng, _lay(cname), out, find_ids(seed + 2, 90, Bn, not_bucket=bucket), n - target_count)
    order = _merge(rng, tgt, fill)
    return out, order, tgt


def _cnt(cnt):
    def build():
        def target(rng, out, ids):
            return _filler(rng, _lay(), out, ids(max(1, cnt // 3)), cnt)
        out, order, tgt = _in_bucket(0x3C10 + cnt, 400, cnt, 2, target)
        return Owner(out.array(order), bucket_of_interest=2, count=cnt)
    return build


CAP_N = 10 * K.kOwnerAvg - 1       # 799 records: ten buckets, and still ten with one record more


def _cap(cnt, one_trace):
    def build():
        base = min(cnt, K.kOwnerCap)

        def target(rng, out, ids):
            return _filler(rng, _lay(), out, ids(1 if one_trace else base), base) if one_trace else \
                [_rand_rec(rng, _lay(), out, t) for t in ids(base)]
        out, order, tgt = _in_bucket(0x3C20 + base + int(one_trace), CAP_N, base, 3, target)
        if cnt > K.kOwnerCap:       # cap.256 and one record more in the same bucket
            tid = (out.rows[tgt[0]]["hi"], out.rows[tgt[0]]["lo"])
            extra = _rand_rec(np.random.default_rng(0x3C2F), _lay(), out, tid)
            order = order[:CAP_N // 2] + [extra] + order[CAP_N // 2:]
        return Owner(out.array(order), general=cnt > K.kOwnerCap, bucket_of_interest=3, count=cnt)
    return build


def _flip_trace(out: Recs, tid, sv=A, rule_bit=None):
    """Three records of one trace whose decision hangs on their order: an
    early start, a reset with no start after it (m == kInf), a late start
    with a short duration.  In this order the latency rule is not satisfied
    (min start after the reset = the late one); with the first and last
    swapped the early start survives and the duration passes every threshold."""
    lay = _lay()
    ep = lay.slot_rules[lay.slot[sv]] if rule_bit is None else rule_bit
    return [out.add(tid, sv, T0, T0 + 1000, ep=ep),
            out.add(tid, sv, None, T0 + LATE // 2, reset=True),
            out.add(tid, sv, T0 + LATE, T0 + LATE + DUR // 2)]


def flip_ids(seed, count, n_bkt, bucket):
    """Ids (in `bucket`) for which _flip_trace decides 0 in order and 1 with the
    first and last record swapped, by the oracle on the expanded records."""
    got = []
    for tid in find_ids(seed, 40, n_bkt, bucket=bucket):
        out = Recs()
        k = _flip_trace(out, tid)
        if oracle_keep(out.array(k), c3())[0] == 0 and oracle_keep(out.array(k[::-1]), c3())[0] == 1:
            got.append(tid)
            if len(got) == count:
                return np.array(got)
    raise AssertionError("flip_ids: no trace id decides 0 / 1 by order")


def _probe(kind):
    def build():
        n, bkt = 160, 1
        Bn = n_buckets(n)
        slots = {"pair": [300, 300], "chain": [77] * 5, "wrap": [510, 511, 511, 511, 0]}[kind]
        K_T = K.kOwnerTable
        assert K_T == 512
        rng = np.random.default_rng(0x3C30 + len(kind))
        out = Recs()
        ids = [find_ids(0x3C31 + s + 7 * j, 1, Bn, bucket=bkt, slot=s)[0] for j, s in enumerate(slots)]
        assert len({(int(t[0]), int(t[1])) for t in ids}) == len(ids)
        per = [[_rand_rec(rng, _lay(), out, t) for _ in range(4)] for t in ids]
        tgt = [p[j] for j in range(4) for p in per]          # a b c a b c ...: the colliding traces interleaved
        others = find_ids(0x3C3F, 60, Bn)
        others = others[~np.isin(table_slot(tid_hash(others[:, 0], others[:, 1])),
                                 [(s + d) % K_T for s in set(slots) for d in range(8)])]
        fill = _filler(rng, _lay(), out, others, n - len(tgt))
        order = _merge(rng, tgt, fill)
        return Owner(out.array(order), slots=slots, ids=np.array(ids), bucket_of_interest=bkt)
    return build


def _order_reset():
    n, bkt = 160, 0
    Bn = n_buckets(n)
    rng = np.random.default_rng(0x3C40)
    out = Recs()
    tid = flip_ids(0x3C41, 1, Bn, bkt)[0]
    x = _flip_trace(out, tid)
    fill = _filler(rng, _lay(), out, find_ids(0x3C42, 40, Bn), n - 3)
    order = fill[:20] + [x[0]] + fill[20:70] + [x[1]] + fill[70:120] + [x[2]] + fill[120:]
    return Owner(out.array(order), x=[20, 71, 122], tid=tid)


def _order_split():
    n, bkt, foreign = 480, 1, 200
    Bn = n_buckets(n)
    rng = np.random.default_rng(0x3C50)
    out = Recs()
    tid = flip_ids(0x3C51, 1, Bn, bkt)[0]
    k = _flip_trace(out, tid)
    early = [k[0], out.add(tid, B, T0 + 5, T0 + 900), out.add(tid, None, None, 0, svcb=0)]
    late = [k[1], k[2], out.add(tid, B, T0 + LATE, T0 + LATE + 100)]
    same = _filler(rng, _lay(), out, find_ids(0x3C52, 50, Bn, bucket=bkt), foreign)
    other = _filler(rng, _lay(), out, find_ids(0x3C53, 60, Bn, not_bucket=bkt), n - foreign - 6)
    mid = _merge(rng, same, other[30:-30])
    order = other[:30] + early + mid + late + other[-30:]
    return Owner(out.array(order), early=list(range(30, 33)), late=list(range(n - 33, n - 30)), tid=tid,
                 bucket_of_interest=bkt, foreign=foreign)


def _simple(seed, make, cname="c3", n=160, **meta):
    """Marked traces (made by make(out, ids) -> {name: [record indices]})
    interleaved with filler."""
    def build():
        rng = np.random.default_rng(seed)
        out = Recs()
        marks = make(out, find_ids(seed + 1, 16, n_buckets(n)))
        tgt = [i for v in marks.values() for i in v]
        fill = _filler(rng, _lay(cname), out, find_ids(seed + 2, 40, n_buckets(n)), n - len(tgt))
        order = _merge(rng, tgt, fill)
        where = {name: [order.index(i) for i in v] for name, v in marks.items()}
        return Owner(out.array(order), cname=cname, marks=where, **meta)
    return build


def _late_short(out, tid, sv, ep, **kw):      # not satisfied: 20 ms
    return out.add(tid, sv, T0 + LATE, T0 + LATE + DUR // 2, ep=ep, **kw)


def _long_dur(out, tid, sv, ep, **kw):        # satisfied whatever the threshold: 3 s
    return out.add(tid, sv, T0, T0 + 3 * LATE, ep=ep, **kw)


def _make_svc0(out, ids):
    lay = _lay("c3_lat0")
    ep0, epA = lay.slot_rules[lay.slot[0]], lay.slot_rules[lay.slot[A]]
    return {"sat0": [_late_short(out, ids[0], A, epA), _long_dur(out, ids[0], 0, ep0)],     # only service 0 satisfies
            "unsat0": [_late_short(out, ids[1], 0, ep0), _late_short(out, ids[1], A, epA)],
            "only0": [_long_dur(out, ids[2], 0, ep0)]}


def _make_multi(out, ids):
    lay = _lay()
    ep = lambda s: lay.slot_rules[lay.slot[s]]
    # ids out of order in recv; the satisfied service (13: its second rule is the
    # config's last, so no later unsatisfied rule replaces the level's ratio) is
    # neither first nor last there, and the last the fold visits
    nine = [12, 4, 11, 5, 13, 6, 10, 7, 9]
    two = [9, 4]
    return {"one": [_long_dur(out, ids[0], 7, ep(7))],
            "two": [_late_short(out, ids[1], two[0], ep(two[0])), _long_dur(out, ids[1], two[1], ep(two[1]))],
            "nine": [(_long_dur if s == 13 else _late_short)(out, ids[2], s, ep(s)) for s in nine],
            "nine.unsat": [_late_short(out, ids[3], s, ep(s)) for s in nine],
            # one service in two records around another's: its element is combined in recv order
            "nine.split": [out.add(ids[4], 13, T0, T0 + 10, ep=ep(13)), _late_short(out, ids[4], 5, ep(5)),
                           out.add(ids[4], 13, T0 + 20, T0 + 3 * LATE, ep=0)]}


def _make_none(out, ids):
    lay = _lay()
    return {"none": [out.add(ids[0], None), out.add(ids[0], None, svcb=1)],
            "none.err": [out.add(ids[1], None), out.add(ids[1], None, err=True)],
            "lat": [_long_dur(out, ids[2], A, lay.slot_rules[lay.slot[A]])]}


def _make_unknown(out, ids):
    lay = _lay()
    return {"unknown": [out.add(ids[0], 500, T0, T0 + 3 * LATE, ep=0)],
            "unknown+A": [out.add(ids[1], 0xFFFFFE, T0, T0 + 3 * LATE, ep=0),
                          _late_short(out, ids[1], A, lay.slot_rules[lay.slot[A]])],
            "14": [out.add(ids[2], 14, T0, T0 + 3 * LATE, ep=0)]}        # the first id past C3's services


def _make_err(out, ids):
    lay = _lay()
    epA = lay.slot_rules[lay.slot[A]]
    recs = [_late_short(out, ids[0], A, epA, err=(j == 11)) for j in range(17)]
    return {"err": recs, "noerr": [_late_short(out, ids[1], A, epA) for _ in range(17)]}


def _ratio():
    n = 400
    rng = np.random.default_rng(0x3C90)
    out = Recs()
    lay = _lay("fractional")
    ids = find_ids(0x3C91, 260, n_buckets(n))
    order = []
    for j, t in enumerate(ids):         # matched, never satisfied: the fractional fallback ratios decide
        sv = C3_LAT[j % len(C3_LAT)]
        order.append(_late_short(out, t, sv, lay.slot_rules[lay.slot[sv]]))
    for j, t in enumerate(ids[:n - 260]):   # the first 140 traces get a second record far from the first
        order.append(out.add(t, None, svcb=0))
    return Owner(out.array(order), cname="fractional", singles=260)


def chunk_bit(rule: int):
    """(chunk, bit) of latency3's endpoint rule `rule`: 64 latency rules a chunk."""
    return rule // 64, rule % 64


def _chunks():
    """latency3 (3 chunks, rule j on service j % 64): per trace one record of
    service s whose only endpoint bit is rule 64 + s's (chunk 1) or rule
    128 + s's (chunk 2), over a long duration: the rule is satisfied through
    a word the fold re-reads from recv; `bare` is the same with no bit."""
    n = 240
    rng = np.random.default_rng(0x3CA0)
    ids = find_ids(0x3CA1, n // 2, n_buckets(n))
    out, bare = Recs(3), Recs(3)
    order = []
    for j, t in enumerate(ids):
        s = j % 22                       # services with a rule in all three chunks
        ck = 1 + j % 2
        order.append(out.add(t, s, T0, T0 + 3 * LATE, **{f"ep{ck}": 1 << s}))
        bare.add(t, s, T0, T0 + 3 * LATE)
        order.append(out.add(t, None))   # and a second record without latency
        bare.add(t, None)
    perm = list(rng.permutation(len(order)))
    return Owner(out.array(perm), cname="latency3", chunks=3, bare=bare.array(perm))


OWNER = {
    "b.80": _b(K.kOwnerAvg), "b.81": _b(K.kOwnerAvg + 1),
    **{f"cnt.{c}": _cnt(c) for c in (1, 2, 3, 128, 129)},
    **{f"cap.{c}.{'one' if o else 'many'}": _cap(c, o) for c in (255, 256, 257) for o in (True, False)},
    "probe.pair": _probe("pair"), "probe.chain": _probe("chain"), "probe.wrap": _probe("wrap"),
    "order.reset": _order_reset, "order.split": _order_split,
    "lat.svc0": _simple(0x3C60, _make_svc0, "c3_lat0"), "lat.multi": _simple(0x3C68, _make_multi),
    "lat.none": _simple(0x3C70, _make_none), "lat.unknown": _simple(0x3C78, _make_unknown),
    "err.one": _simple(0x3C80, _make_err),
    "ratio": _ratio, "chunks": _chunks,
}
_own = {}


def owner(name) -> Owner:
    if name not in _own:
        _own[name] = OWNER[name]()
    return _own[name]
