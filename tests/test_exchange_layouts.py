"""The trace-id exchange on hand-laid spans and records: one named layout per
seam of the pack kernels (shard_hist_kernel, shard_counts_kernel,
shard_scatter_kernel), of shard_unpack_kernel and of the owner's bucketed
fold (owner_bucket_kernel, owner_fold_kernel), each compared byte for byte
(tests/exchange_layouts.py builds them).

The generated workloads of tests/test_exchange.py reach these seams by
chance, if at all.  Here every layout's census (from the built columns or
records and the numpy restatement alone) first proves that the input holds its
seam; on the CPU the numpy pack's records fold to the oracle's decisions on
the spans, and the owner layouts are decided by the oracle on the expanded
records; on the GPU the kernels must give the numpy pack's bytes, the numpy
unpack's columns, and the oracle's and the general path's decisions.

Source layout                  guards (constant / code line)
-----------------------------  ------------------------------------------------
n.1, n.63, n.64, n.65          `valid` / `vm` of x_bounds and bit 63 of `nxt`:
                               the batch ends at lane 0, 62, 63 and at lane 0
                               of a second step
step.cross                     a trace run across a 64-span step: two records
                               with one id, the second's `head` at lane 0
step.full, step.singles        one record of 64 lanes; 64 records in a step
row.15, row.31, row.47         the DPP row steps of seg_or_scan / seg_lat_scan:
                               a record ending on lane s, one starting on s + 1,
                               four over lanes s - 3 .. s + 4 with a zero start,
                               the only ERROR, the min start and the max end at
                               or below lane s (the tail is lane s + 4)
head.svc                       the `ps != x.sv` head: A->B (two records), A->N
                               (latency, then none), 0->1->20->OSE_NONE (services
                               without a latency rule and ids past the interned
                               services: one record)
aba                            A B A inside a step: three records, in source
                               order in their owner's bucket (`off`, `mine`)
zero.first/last/mid/all        LAT_OF_SPAN, kXReset, the `m == kInf` record and
                               shard_unpack_kernel's kStatusReset rule
chunk.1023/1024/1025           kXChunk (1024): n_tiles 1 -> 2, a trace run
                               across the wave's chunk end
wg.4096, wg.4097               kSortThreads / 64 waves a workgroup: the second
                               workgroup, three of whose waves have `ch >= n_tiles`
ranks.1/2/63/64                `lane < n_ranks`, the `for o < n_ranks` ballot loop
ranks.hole.one / .interior     every record to one owner; interior owners with
                               none (shard_counts_kernel's `hi - lo == 0`)
scan.1024, scan.1025           kScanTileItems (1024): n_ranks * n_tiles = 1024
                               and 1088 (world 64 at 16 and 17 chunks): one and
                               two tiles of launch_scan_u32
planes                         route_match instead of route + arena (`& slot_rules`:
                               the column also carries other services' bits);
                               under latency3 one plane per rule chunk (rm_stride)
attr                           span_attribute bits on the first / the last span
                               of a record only (c3_attr; its bit after the
                               service rules')

Configs: C3 and its fractional form for every layout but attr (C3 + a
span_attribute rule), and latency3 (wide_latency_config: three rule chunks,
88-byte records whose chunk k words follow chunk k's own bit layout,
tests/exchange_emul.py pack(chunk_cfgs=...)) for every layout but head.svc
(its meaning is C3's service numbering: under latency3 every service 0..63 has
a latency rule) and attr (the chunked pack is restated without span_attribute
bits).  The census and the CPU comparison with the oracle on the spans run
under the one-chunk configs; latency3's decisions are checked end to end.

Owner layout                   guards
-----------------------------  ------------------------------------------------
b.80, b.81                     B = ceil(n / kOwnerAvg): 1 -> 2 buckets
cnt.1/2/3/128/129              `P` and the bitonic sort's padding keys (P = 1,
                               2, 4, 128, 256)
cap.255/256 .one / .many       kOwnerCap (256): a bucket filled to the brim by
                               one trace in pieces / by distinct traces; stays
                               on the fold (osehost_owner_last_general == 0)
cap.257 .one / .many           cap.256 and one record more in that bucket: the
                               designed fallback (witness 1), same decisions
probe.pair / .chain / .wrap    kOwnerTable (512): 2 and 5 traces on one slot,
                               a chain from 510 / 511 that wraps to 0, the
                               colliding traces' records interleaved
order.reset                    the record index in the sort key: early start /
                               reset with m == kInf / late start decide 0 in
                               order and 1 with first and last swapped
order.split                    the same, as a block early and a block late in
                               recv with 200 foreign records of the bucket between
lat.svc0                       `first || sv > last`: latency service id 0 (c3_lat0)
lat.multi                      1, 2 and 9 latency services, ids out of order;
                               one service in two records around another's
lat.none                       `any_lat` false beside traces with latency
lat.unknown                    a latency service id >= n_global_svc
err.one                        the ERROR bit on one record of 17
ratio                          trace_uniform(s_hi[g], s_lo[g], seed) under
                               fractional ratios, 140 traces in two records
chunks                         latency3: the deciding endpoint bit only in chunk
                               1 or 2 (the `R + ri * words + kXFixedWords + 2 *
                               ck` re-read).  Reference: the general path only
                               (the oracle's expansion restates one chunk)

End to end: a laid batch cut into W = 2, 3 and 64 rank batches (every cut
inside a trace's latency stretch) through pack, the per-owner concatenation,
ose_shard_decide and ose_shard_scatter_keep on one engine, and at W = 2, 3
through osehost_exchange_sample_local beside a one-span rank and an empty one,
against the oracle on the concatenated batch.
"""
import ctypes as C

import numpy as np
import pytest

from odigos_amd import native
from tests import exchange_layouts as xl
from tests.exchange_emul import INF, NONE24, REC_BYTES, XERR, XLAT, XRESET, chunk_words, owners, unpack, xdt
from tests.exchange_layouts import A, B, C3_LAT, K, LATE, N, T0, WAVE

SOURCES = list(xl.SOURCE)
OWNERS = list(xl.OWNER)
SRC_CASES = [(n, c) for n in SOURCES for c in xl.SOURCE_CONFIGS[n]]


# ---------------------------------------------------------------------------
# constants and hashes

def test_constants_as_designed():
    got = {k: getattr(K, k) for k in xl.DESIGNED}
    assert got == xl.DESIGNED, "an exchange constant changed: re-lay tests/exchange_layouts.py against it"
    assert K.kXChunk == K.kXSteps * WAVE and K.kOwnerTable == 2 * K.kOwnerCap
    assert xl.n_buckets(1) == 1 and xl.n_buckets(80) == 1 and xl.n_buckets(81) == 2
    assert xl.n_buckets(xl.CAP_N) == xl.n_buckets(xl.CAP_N + 1) == 10
    assert xdt(1).itemsize == REC_BYTES == 8 * (K.kXFixedWords + 2) and xdt(3).itemsize == 8 * (K.kXFixedWords + 6)
    assert len(C3_LAT) == 11 and A in C3_LAT and B in C3_LAT and N not in C3_LAT and 0 not in C3_LAT


def test_layout_configs():
    from tests.test_sampling_chunks import _chunks
    from tests.workloads import check_interning
    for cname in xl.CONFIGS:
        check_interning({k: [r for r in v if r["name"] != "attr"] for k, v in xl.config(cname).items()})
        parts = xl.chunk_configs(cname)
        assert _chunks(xl.config(cname)) == len(parts or [0]) == (3 if cname == "latency3" else 1)
    parts = xl.chunk_configs("latency3")
    assert [len(p["endpoint_rules"]) for p in parts] == [64, 64, 22]
    assert sum((p.get("endpoint_rules") for p in parts), []) == xl.config("latency3")["endpoint_rules"]
    assert [bool(p.get("service_rules")) for p in parts] == [True, False, False]


def test_owner_hash_matches_abi():
    L = native.lib()
    tid = xl.find_ids(3, 400)
    for world in (1, 2, 63, 64):
        got = owners(tid[:, 0], tid[:, 1], world)
        assert list(got) == [L.ose_shard_owner(int(h), int(l), world) for h, l in tid]
        h = xl.tid_hash(tid[:, 0], tid[:, 1])
        np.testing.assert_array_equal(got, ((h >> np.uint64(32)) % np.uint64(world)).astype(np.int64))


def test_hash_restatements():
    # python integers against the numpy forms, and the ranges
    tid = xl.find_ids(4, 300)
    h = xl.tid_hash(tid[:, 0], tid[:, 1])
    for Bn in (1, 2, 10):
        assert xl.owner_bucket_of(h, Bn).tolist() == [((int(x) & 0xFFFFFFFF) * Bn) >> 32 for x in h]
    assert xl.table_slot(h).tolist() == [(((int(x) >> 32) * 0x9E3779B1) & 0xFFFFFFFF) >> 23 for x in h]
    assert xl.table_slot(h).max() < K.kOwnerTable


def test_find_ids_finds_what_it_is_asked_for():
    got = xl.find_ids(5, 5, 7, bucket=3, slot=511, world=64, owner=63, draws=1 << 21)
    h = xl.tid_hash(got[:, 0], got[:, 1])
    assert (xl.owner_bucket_of(h, 7) == 3).all() and (xl.table_slot(h) == 511).all()
    assert (owners(got[:, 0], got[:, 1], 64) == 63).all()
    np.testing.assert_array_equal(got, xl.find_ids(5, 5, 7, bucket=3, slot=511, world=64, owner=63, draws=1 << 21))
    assert (xl.owner_bucket_of(xl.tid_hash(*xl.find_ids(6, 50, 7, not_bucket=3).T), 7) != 3).all()


# ---------------------------------------------------------------------------
# source side: census

def _run(b, label, k=0):
    return b.runs_of(label)[k]


def _flags(r):
    return int(r["w4"]) >> 24


def _sv(r):
    return int(r["w4"]) & NONE24


def census_source(name, s):
    b, cname = s.b, xl.SOURCE_CONFIGS[name][0]
    rec, counts, pos = s.pack(cname)
    R = len(rec)
    heads = xl.span_heads(b, set(C3_LAT))
    assert R == int(heads.sum()) == int(counts.sum()) and len(counts) == s.world
    if b.n > 1:   # a span starts a record exactly where its slot differs from its neighbour's
        np.testing.assert_array_equal(pos[1:] != pos[:-1], heads[1:])
    own = owners(rec["hi"], rec["lo"], s.world)
    assert (np.diff(own) >= 0).all()
    fam = name.split(".")[0]
    if fam == "n":
        n = int(name[2:])
        assert b.n == n and xl.n_tiles(n) == 1 and (n - 1) % WAVE == {1: 0, 63: 62, 64: 63, 65: 0}[n]
        if n == 65:
            assert heads[64] and (b.tid[63] == b.tid[64]).all()       # the last span: a record of its own at lane 0
    elif name == "step.cross":
        a, e = _run(b, "X")
        cut = a // WAVE * WAVE + WAVE
        assert a < cut < e and pos[cut - 1] != pos[cut] and len(set(pos[a:e])) == 2
        assert s.rec_of(cname, a)["lo"] == s.rec_of(cname, cut)["lo"] and _sv(s.rec_of(cname, cut)) == A
    elif name == "step.full":
        a, e = _run(b, "F")
        assert a % WAVE == 0 and e - a == WAVE and len(set(pos[a:e])) == 1
        r = s.rec_of(cname, a)
        assert _flags(r) == XERR | XLAT | XRESET and r["m"] == b.start[a + 6:e].min()
    elif name == "step.singles":
        assert heads[xl.LEAD:xl.LEAD + WAVE].all() and len(set(pos[xl.LEAD:xl.LEAD + WAVE])) == WAVE
    elif fam == "row":
        sm = s.meta["seam"]
        assert sm in (15, 31, 47) and sm == int(name[4:])
        a, e = _run(b, "R.end")
        assert (e - 1) % WAVE == sm and len(set(pos[a:e])) == 1           # the tail is lane s
        a2, e2 = _run(b, "R.start")
        assert a2 == e and a2 % WAVE == sm + 1 and len(set(pos[a2:e2])) == 1   # the next head is lane s + 1
        for m in xl.ROW_MARKS:
            a = s.meta["at"][m]
            assert a % WAVE == sm - 3 and len(set(pos[a:a + 8])) == 1 and heads[a] and heads[a + 8]
            assert (a + 7) % WAVE == sm + 4                                # the tail, past the seam
        r = {m: s.rec_of(cname, s.meta["at"][m]) for m in xl.ROW_MARKS}
        a = s.meta["at"]["zero"]
        assert np.nonzero(b.start[a:a + 8] == 0)[0].tolist() == [2] and (a + 2) % WAVE == sm - 1
        assert _flags(r["zero"]) == XLAT | XRESET and r["zero"]["m"] == b.start[a + 3:a + 8].min() > b.start[a + 1] == T0
        a = s.meta["at"]["err"]
        assert np.nonzero(b.status[a:a + 8] == native.STATUS_ERROR)[0].tolist() == [3] and (a + 3) % WAVE == sm
        assert _flags(r["err"]) == XLAT | XERR
        a = s.meta["at"]["min"]
        assert r["min"]["m"] == T0 == b.start[a] and a % WAVE <= sm and (b.start[a + 1:a + 8] > T0).all()
        a = s.meta["at"]["max"]
        assert r["max"]["e"] == T0 + 10 * LATE == b.end[a + 3] and (a + 3) % WAVE == sm
        assert (np.delete(b.end[a:a + 8], 3) < T0 + 10 * LATE).all()
        for m in ("err", "min", "max"):
            assert _flags(r[m]) & XRESET == 0
    elif name == "head.svc":
        a, e = _run(b, "AB")
        assert [_sv(s.rec_of(cname, i)) for i in range(a, e)] == [A, A, B, B] and len(set(pos[a:e])) == 2
        a, e = _run(b, "AN")
        assert [_sv(s.rec_of(cname, i)) for i in range(a, e)] == [A, A, NONE24, NONE24] and len(set(pos[a:e])) == 2
        assert _flags(s.rec_of(cname, e - 1)) == 0 and s.rec_of(cname, e - 1)["e"] == 0
        a, e = _run(b, "NN")
        assert tl_rle(b.svc[a:e]) == [0, 1, N, native.OSE_NONE] and len(set(pos[a:e])) == 1
        r = s.rec_of(cname, a)
        assert _sv(r) == NONE24 and _flags(r) == XERR and r["svcb"] == 3 and r["m"] == INF     # svc-00's and svc-01's rules
        assert N >= xl.RuleLayout(xl.config(cname)).nsvc
    elif name == "aba":
        a, e = _run(b, "ABA")
        assert a // WAVE == (e - 1) // WAVE
        p = [int(pos[a]), int(pos[a + 3]), int(pos[a + 5])]
        assert [_sv(rec[k]) for k in p] == [A, B, A] and p == [p[0], p[0] + 1, p[0] + 2]    # source order at the owner
    elif fam == "zero":
        a, e = _run(b, "Z")
        z = list(s.meta["zero"])
        assert np.nonzero(b.start[a:e] == 0)[0].tolist() == z and len(set(pos[a:e])) == 1
        r = s.rec_of(cname, a)
        assert _flags(r) == XLAT | XRESET
        after = b.start[a + z[-1] + 1:e]
        assert r["m"] == (after.min() if len(after) else INF)
        st = unpack(rec.view(np.uint8)).a["status"][pos[a]]
        assert bool(st & 0x80) == (len(after) > 0) == (name in ("zero.first", "zero.mid"))
    elif fam == "chunk":
        n = int(name[6:])
        assert b.n == n and xl.n_tiles(n) == (2 if n > K.kXChunk else 1)
        if n > K.kXChunk:
            a, e = _run(b, "C")
            assert a < K.kXChunk < e and pos[K.kXChunk - 1] != pos[K.kXChunk]
    elif fam == "wg":
        n = int(name[3:])
        tiles = xl.n_tiles(n)
        wgs = -(-tiles // xl.WAVES_PER_WG)
        assert b.n == n and (tiles, wgs) == ((4, 1) if n == 4096 else (5, 2))
        a, e = _run(b, "W")
        assert e == b.n and a < 4096 and (n == 4096 or pos[4095] != pos[4096])
    elif name.startswith("ranks.hole"):
        assert s.world == 64
        if name.endswith("one"):
            assert (counts > 0).sum() == 1 and counts.max() == R > 1
        else:
            nz = np.nonzero(counts)[0]
            hole = [d for d in range(nz[0] + 1, nz[-1]) if counts[d] == 0]
            assert hole and 0 < hole[0] < 63 and len(nz) >= 3
    elif fam == "ranks":
        w = int(name[6:])
        assert s.world == w and counts.min() >= 1 and xl.n_tiles(b.n) == 3        # every lane d < n_ranks has records
    elif fam == "scan":
        H = s.world * xl.n_tiles(b.n)
        want = {"scan.1024": (16384, 1024, 1), "scan.1025": (16385, 1088, 2)}[name]
        assert (b.n, H, -(-H // K.kScanTileItems)) == want and s.world == 64
    elif name == "planes":
        cfg = xl.config(cname)
        rm, ep = s.route_match(cfg), s.endpoint_bits(cfg)
        assert s.planes and (rm & ~ep).any() and ((rm & ep) == ep).all() and ep.any()
        lay = xl.RuleLayout(cfg)
        assert all(int(r["ep"]) & ~lay.slot_rules[lay.slot[_sv(r)]] == 0 for r in rec if _sv(r) != NONE24)
        assert any(int(r["ep"]) for r in rec)
    elif name == "attr":
        shift = xl.RuleLayout(xl.config(cname)).attr_shift
        assert shift == 4
        a, e = _run(b, "AT.first")
        assert s.attr[a] == 1 and not s.attr[a + 1:e].any() and s.rec_of(cname, a)["svcb"] >> np.uint64(shift) == 1
        a, e = _run(b, "AT.last")
        assert s.attr[e - 1] == 1 and not s.attr[a:e - 1].any() and s.rec_of(cname, a)["svcb"] >> np.uint64(shift) == 1
        a, e = _run(b, "AT.none")
        assert s.rec_of(cname, a)["svcb"] >> np.uint64(shift) == 0 and int(s.attr.sum()) == 2
    else:
        raise AssertionError(f"layout {name} has no census")


def tl_rle(a):
    from tests.trace_layouts import _rle
    return _rle(a)


@pytest.mark.parametrize("name", SOURCES)
def test_census_source(name):
    census_source(name, xl.source(name))


def _oracle_spans(b, cfg):
    from odigos_amd.batch import HostOutputs
    from tests.oracle_lib import SamplingOracle
    ho = HostOutputs(b.cols)
    assert SamplingOracle(cfg).process(b.cols, ho.outs, native.GROUP_TRACE_ID, xl.SEED, 2) == 0
    return ho.view("keep", np.uint8)[: b.n].copy()


@pytest.mark.parametrize("cname", ["c3", "fractional"])
@pytest.mark.parametrize("name", SOURCES)
def test_records_fold_like_spans(name, cname):
    # numpy pack -> expansion -> oracle decides every span as the oracle on the spans does
    s = xl.source(name)
    rec, _, pos = s.pack(cname)
    keep_rec = xl.oracle_keep(rec, xl.config(cname))
    np.testing.assert_array_equal(keep_rec[pos], _oracle_spans(s.b, xl.config(cname)))


def test_marked_spans_decide_as_laid():
    # the marks of the row layouts reach the decision: a record's zero start
    # (far side of the seam) turns its trace from satisfied to not
    s = xl.source("row.31")
    keep = _oracle_spans(s.b, xl.c3())
    a = s.meta["at"]
    assert keep[a["min"]] == 1 and keep[a["max"]] == 1 and keep[a["err"]] == 1      # 1 s and 9 s; the error rule


# ---------------------------------------------------------------------------
# owner side: census

def _probe_places(slots):
    """Where linear probing puts traces with these home slots, inserted in any order."""
    used = set()
    for s in slots:
        while s in used:
            s = (s + 1) % K.kOwnerTable
        used.add(s)
    return used


def _swapped(recv, i, j):
    r = recv.copy()
    r[[i, j]] = r[[j, i]]
    return r


def census_owner(name, o):
    r = o.recv
    assert o.B == xl.n_buckets(o.n) and o.counts.sum() == o.n
    assert o.general == bool((o.counts > K.kOwnerCap).any())
    # restated bucket and table slot of every record
    h = [xl.tid_hash(int(a), int(b)) for a, b in zip(r["hi"][:8], r["lo"][:8])]
    assert [int(xl.owner_bucket_of(x, o.B)) for x in h] == o.bucket[:8].tolist()
    flags = (r["w4"] >> np.uint64(24)).astype(np.int64)
    sv = (r["w4"] & np.uint64(NONE24)).astype(np.int64)
    lat = (flags & XLAT) != 0
    assert ((sv != NONE24) == lat).all() and (r["e"][~lat] == 0).all() and (r["m"][~lat] == INF).all()
    tid = [(int(a), int(b)) for a, b in zip(r["hi"], r["lo"])]
    fam = name.split(".")[0]
    if fam == "b":
        assert (o.n, o.B) == ((80, 1) if name == "b.80" else (81, 2)) and (o.counts > 0).all()
    elif fam == "cnt":
        c = int(name[4:])
        P = 1
        while P < c:
            P <<= 1
        assert o.counts[2] == c and P == {1: 1, 2: 2, 3: 4, 128: 128, 129: 256}[c] and o.B == 5
    elif fam == "cap":
        c = int(name.split(".")[1])
        assert o.counts[3] == c and o.B == 10 and (np.delete(o.counts, 3) < K.kOwnerCap).all()
        traces = {t for t, bk in zip(tid, o.bucket) if bk == 3}
        assert len(traces) == (1 if name.endswith("one") else min(c, K.kOwnerCap))
        if c == 257:     # cap.256 and one record more
            base = xl.owner(name.replace("257", "256")).recv
            at = xl.CAP_N // 2
            np.testing.assert_array_equal(np.delete(r, at), base)
            assert o.bucket[at] == 3
    elif fam == "probe":
        slots, ids = o.meta["slots"], o.meta["ids"]
        hh = xl.tid_hash(ids[:, 0], ids[:, 1])
        assert xl.table_slot(hh).tolist() == slots and (xl.owner_bucket_of(hh, o.B) == o.meta["bucket_of_interest"]).all()
        places = _probe_places(slots)
        assert places == {"pair": {300, 301}, "chain": {77, 78, 79, 80, 81}, "wrap": {510, 511, 0, 1, 2}}[name[6:]]
        # no other trace of the bucket sits in the chain's way, and the colliding traces alternate in recv
        mine = {(int(a), int(b)) for a, b in ids}
        bk = o.meta["bucket_of_interest"]
        assert not any(int(s) in places for t, s, k in zip(tid, o.slot, o.bucket) if k == bk and t not in mine)
        seq = [t for t in tid if t in mine]
        assert len(seq) == 4 * len(ids) and all(x != y for x, y in zip(seq, seq[1:]))
    elif name == "order.reset":
        x = o.meta["x"]
        assert [tid[i] for i in x] == [tid[x[0]]] * 3 and min(np.diff(x)) > 40 and tid.count(tid[x[0]]) == 3
        assert r["m"][x[1]] == INF and flags[x[1]] == XLAT | XRESET and r["m"][x[0]] < r["m"][x[2]]
        keep = o.oracle()
        other = xl.oracle_keep(_swapped(r, x[0], x[2]), xl.config(o.cname))
        assert keep[x].tolist() == [0, 0, 0] and other[x].tolist() == [1, 1, 1]
        assert np.array_equal(np.delete(keep, x), np.delete(other, x))
    elif name == "order.split":
        e, l = o.meta["early"], o.meta["late"]
        bk = o.meta["bucket_of_interest"]
        assert {tid[i] for i in e + l} == {tid[e[0]]} and tid.count(tid[e[0]]) == 6
        between = [i for i in range(e[-1] + 1, l[0]) if o.bucket[i] == bk]
        assert len(between) == o.meta["foreign"] == 200 and o.counts[bk] == 206 <= K.kOwnerCap
        keep = o.oracle()
        sw = r.copy()
        sw[e], sw[l] = r[l], r[e]
        other = xl.oracle_keep(sw, xl.config(o.cname))
        assert keep[e + l].tolist() == [0] * 6 and other[e + l].tolist() == [1] * 6
    elif name == "lat.svc0":
        mk = o.meta["marks"]
        keep = o.oracle()
        assert sorted(sv[mk["sat0"]].tolist()) == [0, A] and lat[mk["sat0"]].all() and sv[mk["only0"]].tolist() == [0]
        assert keep[mk["sat0"]].tolist() == [1, 1] and keep[mk["only0"]].tolist() == [1]
        bare = r.copy()            # without service 0's endpoint bits nothing is satisfied
        bare["ep"][mk["sat0"] + mk["only0"]] &= np.uint64(0xFFFF)
        kb = xl.oracle_keep(bare, xl.config(o.cname))
        assert kb[mk["sat0"]].tolist() == [0, 0] or kb[mk["only0"]].tolist() == [0]
    elif name == "lat.multi":
        mk = o.meta["marks"]
        keep = o.oracle()
        for nm, k in (("one", 1), ("two", 2), ("nine", 9), ("nine.unsat", 9), ("nine.split", 2)):
            assert len(set(sv[mk[nm]].tolist())) == k and lat[mk[nm]].all()
        in_recv = sv[sorted(mk["nine"])].tolist()
        assert in_recv != sorted(in_recv) and in_recv != sorted(in_recv, reverse=True)
        for nm in ("one", "two", "nine", "nine.split"):
            assert keep[mk[nm]].all(), nm
    elif name == "lat.none":
        mk = o.meta["marks"]
        assert not lat[mk["none"]].any() and not lat[mk["none.err"]].any() and lat[mk["lat"]].all()
        assert flags[mk["none.err"]].max() == XERR and o.oracle()[mk["lat"]].all() and o.oracle()[mk["none.err"]].all()
    elif name == "lat.unknown":
        mk = o.meta["marks"]
        nsvc = xl.RuleLayout(xl.config(o.cname)).nsvc
        assert nsvc == 14 and sv[mk["unknown"]].tolist() == [500] and sv[mk["14"]].tolist() == [14]
        assert sorted(sv[mk["unknown+A"]].tolist()) == [A, 0xFFFFFE] and lat[mk["unknown"] + mk["14"]].all()
    elif name == "err.one":
        mk = o.meta["marks"]
        assert (flags[mk["err"]] & XERR).sum() == 1 and len(mk["err"]) == 17 and not (flags[mk["noerr"]] & XERR).any()
        assert o.oracle()[mk["err"]].all()
    elif name == "ratio":
        keep = o.oracle()
        n1 = o.meta["singles"]
        assert len(set(tid)) == n1 == 260 and o.n == 400 and 0 < keep[:n1].sum() < n1
        assert tid[:140] == tid[260:] and np.array_equal(keep[:140], keep[260:])
    elif name == "chunks":
        assert o.chunks == 3 and not r["ep"].any() and (r["ep1"] != 0).sum() == (r["ep2"] != 0).sum() == 60
        bare = o.meta["bare"]
        assert not bare["ep1"].any() and not bare["ep2"].any()
        for f in ("hi", "lo", "m", "e", "w4", "ep", "svcb"):
            np.testing.assert_array_equal(r[f], bare[f])
    else:
        raise AssertionError(f"layout {name} has no census")


@pytest.mark.parametrize("name", OWNERS)
def test_census_owner(name):
    census_owner(name, xl.owner(name))


def test_unpack_chunked_restatement():
    # the K-chunk record: chunk k's words land in plane k
    o = xl.owner("chunks")
    hc = unpack(o.bytes(), 3)
    ep, sb = chunk_words(o.recv, 3)
    n = o.n
    np.testing.assert_array_equal(hc.a["route_match"][n:2 * n], o.recv["ep1"])
    np.testing.assert_array_equal(hc.a["route_match"][2 * n:3 * n], o.recv["ep2"])
    assert ep.shape == sb.shape == (3, n) and not hc.a["svc_match"].any()


def _e2e(W):
    if W not in _e2e_cache:
        b, cuts = xl.e2e_batch(W)
        _e2e_cache[W] = (b, cuts, xl.rank_slices(b, cuts))
    return _e2e_cache[W]


_e2e_cache = {}


@pytest.mark.parametrize("W", [2, 3, 64])
def test_census_e2e(W):
    b, cuts, slices = _e2e(W)
    assert len(slices) == W and sum(s.n for s in slices) == b.n and len(cuts) == W - 1
    if W == 64:
        assert all(s.n == 300 for s in slices)
    for c in cuts:      # every cut divides a trace's latency stretch
        assert (b.tid[c - 1] == b.tid[c]).all() and b.svc[c - 1] == b.svc[c] == A
    far = b.runs_of("FAR")
    edges = [0] + cuts + [b.n]
    assert len(far) == 2 and far[0][1] <= edges[1] and far[1][0] >= edges[-2]
    # a slice's columns are the batch's
    for s, lo in zip(slices, edges):
        np.testing.assert_array_equal(s.a["res_svc"][s.a["resource"]], b.svc[lo:lo + s.n])
    from tests.oracle_lib import concat_keep_oracle
    want = np.concatenate(concat_keep_oracle(slices, xl.c3(), xl.SEED, 2))
    np.testing.assert_array_equal(want, _oracle_spans(b, xl.c3()))      # the concatenation is the batch


# ---------------------------------------------------------------------------
# GPU

_engines = {}


def engine(cname):
    from odigos_amd.batch import Engine
    if cname not in _engines:
        _engines[cname] = Engine({"odigossampling": xl.config(cname)})
    return _engines[cname]


def _sentinel(nbytes):
    import torch
    return torch.full((nbytes,), xl.SENTINEL, dtype=torch.uint8, device="cuda")


PAD = 8       # records / spans of sentinel past every output


def _gpu_pack(eng, cols, world, rb, planes=None):
    """ose_shard_pack into sentinel-filled buffers: (send bytes, counts, pos
    bytes, the device batch).  planes: [K, n] route_match planes to hand in."""
    import torch
    from odigos_amd.batch import DeviceBatch
    db = DeviceBatch(cols)
    n = cols.n_spans
    if planes is not None:
        db.t["route_match_planes"] = torch.from_numpy(planes.view(np.uint8).reshape(-1).copy()).cuda()
        db.cols.route_match = db.t["route_match_planes"].data_ptr()
        db.cols.match_planes = len(planes) if len(planes) > 1 else 0
    send, pos = _sentinel((n + PAD) * rb), _sentinel((n + PAD) * 4)
    counts = torch.full((world,), -1, dtype=torch.int64, device="cuda")
    native.check(native.lib().ose_shard_pack(eng.h, C.byref(db.cols), world, send.data_ptr(), counts.data_ptr(),
                                             pos.data_ptr(), None))
    torch.cuda.synchronize()
    return send, counts.cpu().numpy(), pos, db


def _gpu_unpack(recv_t, R, rb, chunks):
    """ose_shard_unpack into sentinel-filled columns: {column: bytes}"""
    import torch
    from odigos_amd.exchange import OWNER_COLS
    planes = {"route_match": chunks, "svc_match": chunks}
    cols = {k: _sentinel((R * planes.get(k, 1) + PAD) * w) for k, w in OWNER_COLS}
    native.check(native.lib().ose_shard_unpack(recv_t.data_ptr(), R, rb, *[cols[k].data_ptr() for k, _ in OWNER_COLS], None))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in cols.items()}


def _check_unpack(got, recv_bytes, R, chunks):
    from odigos_amd.exchange import OWNER_COLS
    hc = unpack(recv_bytes, chunks)
    for k, w in OWNER_COLS:
        m = R * w * (chunks if k in ("route_match", "svc_match") else 1)
        np.testing.assert_array_equal(got[k][:m], hc.a[k].view(np.uint8)[:m], err_msg=k)
        assert (got[k][m:] == xl.SENTINEL).all(), f"{k}: written past {R} records"


@pytest.mark.gpu
@pytest.mark.parametrize("name,cname", SRC_CASES)
def test_gpu_pack_unpack(name, cname):
    s = xl.source(name)
    eng = engine(cname)
    rb = int(native.lib().ose_shard_record_bytes(eng.h))
    chunks = len(xl.chunk_configs(cname) or [0])
    assert rb == xdt(chunks).itemsize
    cols, alive, planes = s.columns(cname)
    assert (planes is not None) == (name == "planes")
    send, counts, pos, _ = _gpu_pack(eng, cols, s.world, rb, planes)
    rec, cnt, p = s.pack(cname)
    R, n = len(rec), s.n
    np.testing.assert_array_equal(counts, cnt)
    pos = pos.cpu().numpy()
    np.testing.assert_array_equal(pos[: 4 * n].view(np.int32), p)
    assert (pos[4 * n:] == xl.SENTINEL).all(), "pack_pos written past n"
    sb = send.cpu().numpy()
    np.testing.assert_array_equal(sb[: R * rb], rec.view(np.uint8))
    assert (sb[R * rb:] == xl.SENTINEL).all(), "send written past the records"
    _check_unpack(_gpu_unpack(send, R, rb, chunks), rec.view(np.uint8), R, chunks)
    del alive


@pytest.mark.gpu
def test_gpu_pack_refuses_ranks_out_of_range():
    # the host's check, before any launch
    import torch
    from odigos_amd.batch import DeviceBatch
    s = xl.source("n.65")
    eng = engine("c3")
    db = DeviceBatch(s.b.cols)
    send, pos = _sentinel(80 * REC_BYTES), _sentinel(80 * 4)
    counts = torch.zeros(80, dtype=torch.int64, device="cuda")
    for w in (0, 65):
        rc = native.lib().ose_shard_pack(eng.h, C.byref(db.cols), w, send.data_ptr(), counts.data_ptr(), pos.data_ptr(), None)
        assert rc == native.OSE_EINVAL
    torch.cuda.synchronize()
    assert (send.cpu().numpy() == xl.SENTINEL).all()


def _decide(eng, recv_t, n, rb):
    """(ose_shard_decide's keep, the general path's keep, the fallback witness)"""
    import torch
    from odigos_amd.exchange import DeviceExchange
    keep = _sentinel(n + 64)
    status = torch.zeros(16, dtype=torch.uint8, device="cuda")
    L = native.lib()
    native.check(L.ose_shard_decide(eng.h, recv_t.data_ptr(), n, rb, keep.data_ptr(), status.data_ptr(),
                                    C.byref(native.Rand(xl.SEED, 0.0)), None))
    torch.cuda.synchronize()
    general = int(L.osehost_owner_last_general(eng.h))
    k = keep.cpu().numpy()
    assert (k[n:] == xl.SENTINEL).all(), "keep written past the records"
    assert DeviceExchange.seed == xl.SEED
    ref = DeviceExchange.receiver(eng, rb).unpack_sample(recv_t, n)[:n].cpu().numpy().copy()
    return k[:n].copy(), ref, general


@pytest.mark.gpu
@pytest.mark.parametrize("name", OWNERS)
def test_gpu_owner_decide(name):
    import torch
    o = xl.owner(name)
    eng = engine(o.cname)
    rb = int(native.lib().ose_shard_record_bytes(eng.h))
    assert rb == xdt(o.chunks).itemsize
    want = o.oracle() if o.cname in xl.ONE_CHUNK else None      # (the CPU side first)
    recv = torch.from_numpy(o.bytes().copy()).cuda()
    fold, ref, general = _decide(eng, recv, o.n, rb)
    assert general == int(o.general)
    assert set(np.unique(fold).tolist()) <= {0, 1}
    np.testing.assert_array_equal(fold, ref)
    if want is not None:
        np.testing.assert_array_equal(fold, want)
    _check_unpack(_gpu_unpack(recv, o.n, rb, o.chunks), o.bytes(), o.n, o.chunks)
    if name == "chunks":
        bare = torch.from_numpy(np.ascontiguousarray(o.meta["bare"]).view(np.uint8).reshape(-1).copy()).cuda()
        fold0, ref0, general0 = _decide(eng, bare, o.n, rb)
        np.testing.assert_array_equal(fold0, ref0)
        assert general0 == 0 and fold.all() and not fold0.all()     # the bit of chunk 1 / 2 is what keeps the trace


def _owner_path(slices, cname):
    """The exchange on one engine, sequentially: pack every rank's batch for
    W owners, hand each owner its buckets in rank order, decide, send the keep
    bytes back, scatter.  Returns (keep per rank, records, fallbacks)."""
    import torch
    W = len(slices)
    eng = engine(cname)
    L = native.lib()
    rb = int(L.ose_shard_record_bytes(eng.h))
    packs = []
    for s in slices:
        send, counts, pos, db = _gpu_pack(eng, s.cols, W, rb)
        packs.append((send, np.concatenate([[0], np.cumsum(counts)]), pos, db))
    backs = [_sentinel(max(int(p[1][-1]), 1)) for p in packs]
    records = fallbacks = 0
    for o in range(W):
        recv = torch.cat([p[0][p[1][o] * rb: p[1][o + 1] * rb] for p in packs])
        k = recv.numel() // rb
        if not k:
            continue
        records += k
        keep = _sentinel(k + 64)
        status = torch.zeros(16, dtype=torch.uint8, device="cuda")
        native.check(L.ose_shard_decide(eng.h, recv.data_ptr(), k, rb, keep.data_ptr(), status.data_ptr(),
                                        C.byref(native.Rand(xl.SEED, 0.0)), None))
        torch.cuda.synchronize()
        fallbacks += int(L.osehost_owner_last_general(eng.h))
        off = 0
        for s, p in enumerate(packs):
            m = int(p[1][o + 1] - p[1][o])
            backs[s][p[1][o]: p[1][o + 1]] = keep[off: off + m]
            off += m
    out = []
    for s, p in zip(slices, packs):
        db = p[3]
        native.check(L.ose_shard_scatter_keep(backs[len(out)].data_ptr(), p[2].data_ptr(), s.n, db.outs.keep, None))
        torch.cuda.synchronize()
        out.append(db.out_numpy("keep", n=s.n).copy())
    return out, records, fallbacks


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["c3", "fractional", "latency3"])
@pytest.mark.parametrize("W", [2, 3, 64])
def test_gpu_end_to_end(W, cname):
    from tests.oracle_lib import concat_keep_oracle
    from tests.test_sampling_chunks import _chunks
    assert _chunks(xl.config(cname)) == (3 if cname == "latency3" else 1)
    b, cuts, slices = _e2e(W)
    got, records, fallbacks = _owner_path(slices, cname)
    want = concat_keep_oracle(slices, xl.config(cname), xl.SEED, 4)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert 0 < records < b.n and fallbacks == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["c3", "latency3"])
@pytest.mark.parametrize("W", [2, 3])
def test_gpu_round_local(W, cname):
    # the product round on the same rank batches, beside a one-span rank and an empty one
    from tests.oracle_lib import concat_keep_oracle
    from tests.test_exchange import _local_round
    _, _, slices = _e2e(W)
    one = xl.source("n.1").b
    sources = list(slices) + [xl.RankSlice(one, 0, 1), xl.RankSlice(one, 0, 0)]
    got, stats = _local_round(sources, xl.config(cname))
    want = concat_keep_oracle(sources, xl.config(cname), xl.SEED, 4)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert [s[2] for s in stats] == [s.n for s in sources] and stats[-1][0] == 0 and stats[-2][0] == 1
    assert sum(s[0] for s in stats) == sum(s[1] for s in stats)
