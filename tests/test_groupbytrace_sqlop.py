"""odigossqldboperationprocessor through the groupbytrace store: a store on an
engine with the section carries db_flags, db_query (the query bytes join the
span's string block in the arena ring) and res_sql_ok from ose_gbt_add to
ose_gbt_release (odigos_amd/csrc/gbt_{host.cpp,kernel.hip}).

Expected releases come from tests/gbt_ref.py (which traces leave, in which
order) and the host columniser over those traces (what their columns hold);
expected sql_op from the restatement of processor.go (tests/sqlop_ref.py via
tests/test_otlp_sqlop.py).

CPU: a census of the hand-laid batches of the seam test, computed from the
trees and their messages alone with the documented block layout (a batch's
blocks are laid in span order from the ring position where the previous
accepted batch ended; a block is route, path, string attribute values,
query).  GPU: releases against the columniser, the stages on a release, the
copy's seams on a ring of the minimum size, refusal, NULL columns, three
workers.
"""
import ctypes as C
import random

import numpy as np
import pytest

from odigos_amd import host, native
from tests.gbt_ref import GroupByTraceRef
from tests.test_groupbytrace import S, _compare_release, _set_of, _Shim
from tests.test_otlp import SEED, to_pb
from tests.test_sqlop import _size_tree
from tests.test_otlp_sqlop import (LONG_QUERY, RESOURCES, SQL_CFGS, _db_columns, _db_tree, _expected_sql_op,
                                   _full_cfg)

Q = "db.query.text"
RING = 1 << 16   # the smallest arena ring the store accepts
HAS_QUERY = native.DB_HAS_QUERY


def _tid(k):
    return "%032x" % (k + 1)


# ---------------------------------------------------------------------------
# the hand-laid batches of the seam test

SEAM_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096]


def _text(uid, n):
    """n printable bytes that differ from span to span and from byte to byte"""
    return "".join(chr(33 + (uid * 7 + i * 13 + i // 90) % 90) for i in range(n))


def _laid_batches():
    """[[("q", text) | ("p", path)]]: one entry per span, each span its own
    trace.  A "q" span carries only a query (its block is the query), a "p"
    span only an 8-byte url.path (its block is the path)."""
    uid = [0]

    def q(n):
        uid[0] += 1
        return ("q", _text(uid[0], n))

    def p():
        uid[0] += 1
        return ("p", "/p/%05d" % uid[0])

    out = []
    out.append([q(4096)])                                                     # 1 span
    b = []
    for k, n in enumerate(SEAM_LENGTHS):                                      # 63 spans: every listed length
        b += [q(n)] + [p() for _ in range(5 if k < 3 else 4)]
    out.append(b)
    out.append([q(33)] + [p() for _ in range(63)])                            # 64 spans: the query at lane 0
    out.append([p() for _ in range(63)] + [q(47), p()])                       # 65 spans: the query at lane 63
    out.append([q(17 + k % 5) for k in range(48)])                            # every alignment, both sides
    out.append([q(4096) for _ in range(13)])                                  # towards the ring's end
    out.append([p() for _ in range(10)] + [q(1000)] + [p() for _ in range(9)])    # a query across the end
    out.append([q(4096) for _ in range(15)] + [q(3574)])                      # ... and round again
    out.append([p() for _ in range(6)] + [q(300)])                            # a path across the end
    return out


def _laid_tree(batch, first_uid):
    spans = []
    for k, (kind, text) in enumerate(batch):
        if kind == "q":
            spans.append(host.span("q%d" % k, kind=3, trace_id=_tid(first_uid + k), attributes={Q: text}))
        else:
            spans.append(host.span("p%d" % k, kind=2, trace_id=_tid(first_uid + k),
                                   attributes={"http.request.method": "GET", "url.path": text}))
    return host.traces(host.resource_spans(RESOURCES[0], spans))


def _laid_trees():
    out, uid = [], 1000
    for b in _laid_batches():
        out.append(_laid_tree(b, uid))
        uid += len(b)
    return out


def _varint(b, i):
    v = s = 0
    while True:
        v |= (b[i] & 0x7F) << s
        s += 7
        i += 1
        if not b[i - 1] & 0x80:
            return v, i


def _query_offsets(msg):
    """[(offset, length)] of every db.query.text string value in the message,
    in wire order: KeyValue{key = 1, value = 2: AnyValue{string_value = 1}}"""
    key = b"\x0a\x0d" + Q.encode() + b"\x12"
    out, pos = [], 0
    while True:
        k = msg.find(key, pos)
        if k < 0:
            return out
        alen, i = _varint(msg, k + len(key))
        if alen == 0:
            out.append((i, 0))
        else:
            assert msg[i] == 0x0A
            n, i = _varint(msg, i + 1)
            out.append((i, n))
            i += n
        pos = i


def _census():
    """Per batch: ring position where it starts, its bytes, and per span
    (kind, ring position of the block, length, offset of the query in the
    message or None)."""
    pos, out = 0, []
    for batch, td in zip(_laid_batches(), _laid_trees()):
        src = _query_offsets(to_pb(td))
        assert len(src) == sum(kind == "q" for kind, _ in batch)
        spans, at, qi = [], pos, 0
        for kind, text in batch:
            n = len(text.encode())
            off = None
            if kind == "q":
                off, ln = src[qi]
                assert ln == n
                qi += 1
            spans.append((kind, at % RING, n, off))
            at += n
        out.append({"start": pos % RING, "bytes": at - pos, "spans": spans})
        pos = at
    return out


def _straddles(start, n):
    return n > 0 and start + n > RING


def test_census_of_the_laid_batches():
    cen = _census()
    # the layout itself: a block that moves by a byte changes these
    assert [(b["start"], b["bytes"], len(b["spans"])) for b in cen] == [
        (0, 4096, 1), (4096, 5513, 63), (9609, 537, 64), (10146, 559, 65), (10705, 909, 48), (11614, 53248, 13),
        (64862, 1152, 20), (478, 65014, 16), (65492, 348, 7)]
    assert all(b["bytes"] < RING for b in cen)
    assert [len(b["spans"]) for b in cen][:4] == [1, 63, 64, 65]
    qs = [s for b in cen for s in b["spans"] if s[0] == "q"]
    assert set(SEAM_LENGTHS) <= {n for _, _, n, _ in qs}
    assert {at % 16 for _, at, n, _ in qs if n} == set(range(16))          # where the add writes
    assert {off % 16 for _, _, n, off in qs if n} == set(range(16))        # where it reads
    # a release hands the batch out alone, its blocks packed from 0: where the release writes
    rel = set()
    for b in cen:
        for _, at, n, _ in b["spans"]:
            if n:
                rel.add((at - b["start"]) % RING % 16)
    assert rel == set(range(16))
    lanes = lambda b: [k for k, s in enumerate(b["spans"][:64]) if s[0] == "q"]   # noqa: E731
    assert lanes(cen[2]) == [0] and lanes(cen[3]) == [63]
    across = [(k, j, s[0]) for k, b in enumerate(cen) for j, s in enumerate(b["spans"]) if _straddles(s[1], s[2])]
    assert across == [(6, 10, "q"), (8, 5, "p")]
    assert cen[6]["spans"][10][1:3] == (64942, 1000) and cen[8]["spans"][5][1:3] == (RING - 4, 8)


# ---------------------------------------------------------------------------
# GPU

def _sql_shim(sql, gcfg, **caps):
    from odigos_amd.batch import Engine
    eng = Engine(_full_cfg(sql))
    eng.set_option("otlp_sqlop", 1)
    return _Shim(eng, gcfg, **caps)


def _add(shim, td, now, edit=None):
    """_Shim.add with a hook that edits the decoded columns before the add"""
    from odigos_amd.batch import OtlpBatch
    ob = OtlpBatch(shim.eng, to_pb(td))
    try:
        ids = []
        for k in range(ob.cols.n_attrsets):
            key = tuple(sorted(ob.attrset(k).items()))
            if key not in shim.sets:
                shim.sets[key] = len(shim.names)
                shim.names.append(key)
            ids.append(shim.sets[key])
        cols = native.Columns.from_buffer_copy(ob.cols)
        got = edit(cols, ob) if edit else None
        shim.g.add(cols, now, ids)
        return got
    finally:
        ob.close()


def _host_db(c):
    """(db_flags, query bytes or None, res_sql_ok) of a host batch"""
    n, R = c.n_spans, c.n_resources
    flags = np.ctypeslib.as_array((C.c_uint8 * n).from_address(c.db_flags)).copy()
    refs = np.ctypeslib.as_array((C.c_uint32 * (2 * n)).from_address(c.db_query)).reshape(n, 2).copy()
    arena = bytes((C.c_uint8 * c.arena_bytes).from_address(c.arena)) if c.arena_bytes else b""
    ok = np.ctypeslib.as_array((C.c_uint8 * R).from_address(c.res_sql_ok)).copy()
    return flags, [arena[o:o + ln] if f & HAS_QUERY else None for f, (o, ln) in zip(flags, refs)], ok


def _check_release(shim, ref, now, sql):
    """One release against the restatement and the columniser.  Returns
    (cols, downloaded columns, the released tree, its host batch, processor,
    store attribute set ids, host ids, traces released) or None when nothing
    leaves."""
    cols, ntr = shim.g.release(now)
    want = ref.release(now)
    assert ntr == len(want)
    if not want:
        assert cols.n_spans == 0
        return None
    td_w = host.traces(*[p for tr in want for p in tr])
    proc = host.Processor("pipeline", _full_cfg(sql))
    hb = proc.columnarize(td_w)
    got = shim.g.download(cols)
    g_sets, h_sets = _compare_release(got, cols, hb, shim.names)
    assert [shim.names[x] for x in g_sets] == [_set_of(rs) for rs in td_w["resourceSpans"]]
    flags, queries, ok = _db_columns(cols, got)
    h_flags, h_queries, h_ok = _host_db(hb.cols)
    np.testing.assert_array_equal(flags, h_flags)
    assert queries == h_queries
    np.testing.assert_array_equal(ok, h_ok)
    return cols, got, td_w, hb, proc, g_sets, h_sets, ntr


@pytest.mark.gpu
@pytest.mark.parametrize("sql_name", ["no_list", "list_matches"])
@pytest.mark.parametrize("n", [1, 65, 700])
def test_gpu_releases_equal_columniser(n, sql_name):
    sql = SQL_CFGS[sql_name]
    shim = _sql_shim(sql, {"wait_duration": "10s"})
    ref = GroupByTraceRef(10 * S)
    td = _db_tree(n, seed=n, long_at=n // 2 if n >= 65 else None)
    rss = td["resourceSpans"]
    # the tree over several adds 7 s apart, a release after each: the traces of
    # the first add leave between the second and the third, whose spans of
    # the same ids start new traces
    parts = [rss[k:k + 2] for k in range(0, len(rss), 2)]
    now, released, long_seen, any_ok = 0, 0, False, set()
    for part in parts + [[], [], []]:
        now += 7 * S
        if part:
            t = host.traces(*part)
            _add(shim, t, now)
            ref.consume(t, now)
        r = _check_release(shim, ref, now, sql)
        if r:
            cols, got = r[0], r[1]
            released += cols.n_spans
            _, queries, ok = _db_columns(cols, got)
            long_seen |= LONG_QUERY.encode() in queries
            any_ok |= set(int(x) for x in ok)
            r[4].close()
    assert released == n and long_seen == (n >= 65)
    if n == 700:
        assert any_ok == ({1} if sql_name == "no_list" else {0, 1})
    st = shim.g.stats()
    assert st["waiting_traces"] == st["held_spans"] == st["held_bytes"] == 0


@pytest.mark.gpu
def test_gpu_stages_on_a_release():
    import torch
    from odigos_amd.batch import DeviceView, HostOutputs, PinnedBatch
    from tests.oracle_lib import SamplingOracle, UrlOracle
    sql = SQL_CFGS["list_matches"]
    cfg = _full_cfg(sql)
    shim = _sql_shim(sql, {"wait_duration": "10s"})
    ref = GroupByTraceRef(10 * S)
    # (queries that are strings: the values _expected_sql_op restates; python's resource is excluded)
    td = _size_tree(random.Random(5))
    _add(shim, td, 0)
    ref.consume(td, 0)
    cols, got, td_w, hb, proc, g_sets, h_sets, _ = _check_release(shim, ref, 10 * S, sql)
    n = hb.cols.n_spans
    assert n == sum(len(ss["spans"]) for rs in td["resourceSpans"] for ss in rs["scopeSpans"]) == 40
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SQLOP | native.STAGE_SIZE
    dv = DeviceView(cols)
    dv.o["sql_op"].fill_(0xEE)
    shim.eng.process_device(dv, st, native.GROUP_TRACE_ID, seed=SEED)
    torch.cuda.synchronize()
    assert int(dv.out_numpy("device_status", np.uint32)[0]) == 0
    want_op = _expected_sql_op(sql, td_w)
    assert want_op.any() and not want_op.all()
    np.testing.assert_array_equal(dv.out_numpy("sql_op", n=n), want_op)
    ho = HostOutputs(hb.cols)
    assert SamplingOracle(cfg["odigossampling"]).process(hb.cols, ho.outs, native.GROUP_TRACE_ID, SEED, 4) == 0
    assert UrlOracle(cfg["odigosurltemplate"]).process(hb.cols, ho.outs, 4) == 0
    np.testing.assert_array_equal(dv.out_numpy("keep", n=n), ho.view("keep", np.uint8)[:n])
    np.testing.assert_array_equal(dv.out_numpy("url_out", n=n), ho.view("url_out", np.uint8)[:n])
    # sizes: the same stage mask through ose_process (a path this store is not
    # part of) on the columniser's batch of the same traces; attribute sets by content
    pb = PinnedBatch(shim.eng, hb.cols)
    pb.fill(hb.cols)
    pb.process(st, native.GROUP_TRACE_ID, seed=SEED)
    A = hb.cols.n_attrsets
    h_bytes = np.ctypeslib.as_array((C.c_int64 * max(A, 1)).from_address(pb.outs.attrset_bytes))[:A].copy()
    h_acc = int(np.ctypeslib.as_array((C.c_int64 * 1).from_address(pb.outs.accepted_spans))[0])
    h_op = np.ctypeslib.as_array((C.c_uint8 * n).from_address(pb.outs.sql_op)).copy()
    np.testing.assert_array_equal(h_op, want_op)
    g_bytes = dv.out_numpy("attrset_bytes", np.int64, n=cols.n_attrsets)
    assert h_bytes.any()
    by_g, by_h = {}, {}
    for gs, hs in zip(g_sets, h_sets):
        by_g[shim.names[gs]] = int(g_bytes[gs])
        by_h[shim.names[gs]] = int(h_bytes[hs])
    assert by_g == by_h and sum(by_g.values()) == int(h_bytes.sum()) == int(g_bytes.sum())
    assert int(dv.out_numpy("accepted_spans", np.int64)[0]) == h_acc > 0
    pb.close()
    proc.close()


@pytest.mark.gpu
def test_gpu_seams_of_the_copy():
    sql = SQL_CFGS["no_list"]
    shim = _sql_shim(sql, {"wait_duration": "1s"}, span_capacity=4096, arena_capacity=RING)
    ref = GroupByTraceRef(1 * S)
    cen, batches, trees = _census(), _laid_batches(), _laid_trees()

    def decoded_refs(cols, ob):
        return ob.download()["db_query"].view(np.uint32).reshape(-1, 2)[:cols.n_spans].copy()

    now, prev = 0, None
    for k in range(len(trees) + 1):
        now += 2 * S
        # release before add: the ring frees, the next batch runs on from where the last one ended
        r = _check_release(shim, ref, now, sql)
        if prev is None:
            assert r is None
        else:
            cols, got = r[0], r[1]
            _, queries, _ = _db_columns(cols, got)
            assert queries == [text.encode() if kind == "q" else None for kind, text in batches[prev]]
            assert cols.arena_bytes == cen[prev]["bytes"]
            r[4].close()
        assert shim.g.stats()["held_bytes"] == 0
        if k == len(trees):
            break
        refs = _add(shim, trees[k], now, decoded_refs)
        ref.consume(trees[k], now)
        # the decoder hands the store the message offsets the census assumes
        for (kind, _, ln, off), (o, l) in zip(cen[k]["spans"], refs):
            if kind == "q" and ln:
                assert (int(o), int(l)) == (off, ln)
        st = shim.g.stats()
        assert st["held_bytes"] == cen[k]["bytes"] and st["held_spans"] == len(batches[k])
        prev = k
    st = shim.g.stats()
    assert st["held_spans"] == st["held_bytes"] == st["waiting_traces"] == 0
    assert st["released_spans"] == st["added_spans"] == sum(len(b) for b in batches)


def _mk(ks, tag, svc="svc-a", qlen=None):
    return host.traces(host.resource_spans(
        {"service.name": svc, "telemetry.sdk.language": "go"},
        [host.span(f"{tag}{k}", kind=2, trace_id=_tid(k),
                   attributes={"http.request.method": "GET", "url.path": f"/u/{k}",
                               Q: _text(k, qlen) if qlen is not None else f"select {k} from {tag}"}) for k in ks]))


@pytest.mark.gpu
def test_gpu_refused_add_counts_the_queries():
    sql = SQL_CFGS["no_list"]
    shim = _sql_shim(sql, {"wait_duration": "10s", "num_traces": 8}, span_capacity=4096, arena_capacity=RING)
    ref = GroupByTraceRef(10 * S, num_traces=8)
    for now, ks in ((0, [1, 2, 3]), (1 * S, [4, 5, 6, 7])):
        td = _mk(ks, "p%d-" % now)
        _add(shim, td, now)
        ref.consume(td, now)
    before = shim.g.stats()
    # 80 spans: paths of 6 bytes fit the ring many times over, 80 queries of 999 bytes do not
    big = _mk(range(200, 280), "x", qlen=999)
    assert 80 * 6 < RING - before["held_bytes"] < 80 * 999
    with pytest.raises(native.OseError) as ei:
        _add(shim, big, 2 * S)
    assert ei.value.code == native.OSE_ERANGE
    assert shim.g.stats() == before
    for now, ks in ((3 * S, [1, 8, 200]), (4 * S, [9, 10, 12])):
        td = _mk(ks, "q%d-" % now)
        _add(shim, td, now)
        ref.consume(td, now)
    r = _check_release(shim, ref, 30 * S, sql)
    assert r is not None and r[0].n_spans > 0
    assert shim.g.stats()["evicted"] == ref.evicted > 0


@pytest.mark.gpu
def test_gpu_null_columns():
    from odigos_amd.batch import Engine
    sql = SQL_CFGS["list_matches"]
    td = _db_tree(65, seed=5)
    hb = host.Processor("pipeline", _full_cfg(sql)).columnarize(td)
    h_flags, h_queries, h_ok = _host_db(hb.cols)
    assert h_flags.any() and set(int(x) for x in h_ok) == {0, 1}
    ids = lambda c: np.array([int(x) for x in c])   # noqa: E731

    def released(shim, now):
        cols, ntr = shim.g.release(now)
        assert ntr == 7 and cols.n_spans == 65   # _db_tree's seven traces
        return cols, shim.g.download(cols)

    def frag_ok(got, cols):
        # a fragment's resource: that of its first span in the added tree (start_ns = base + span index)
        first = {}
        for j, f in enumerate(got["resource"].view(np.uint32)[:cols.n_spans]):
            first.setdefault(int(f), j)
        k = [int(got["start_ns"].view(np.uint64)[first[f]]) - 1739000000000000000 for f in range(cols.n_resources)]
        res_of_span = np.ctypeslib.as_array((C.c_uint32 * 65).from_address(hb.cols.resource))
        return ids(h_ok[res_of_span[k]])

    def no_flags(cols, ob):
        cols.db_flags = None

    def no_query(cols, ob):
        cols.db_query = None

    def no_ok(cols, ob):
        cols.res_sql_ok = None

    shim = _sql_shim(sql, {"wait_duration": "1s"})
    # db_flags NULL: flags 0, no query bytes held, res_sql_ok as given
    plain = _Shim(Engine(_full_cfg(sql)), {"wait_duration": "1s"})   # the option off: the columns NULL from the decoder
    plain.add(td, 0)
    _add(shim, td, 0, no_flags)
    assert shim.g.stats()["held_bytes"] == plain.g.stats()["held_bytes"]
    cols, got = released(shim, 2 * S)
    flags, queries, ok = _db_columns(cols, got)
    assert not flags.any() and queries == [None] * 65
    np.testing.assert_array_equal(ok, frag_ok(got, cols))
    # the decoder's NULL res_sql_ok on a section engine: all ones
    cols_p, got_p = released(plain, 2 * S)
    flags, queries, ok = _db_columns(cols_p, got_p)
    assert not flags.any() and ok.all() and len(ok) == cols_p.n_resources
    # db_flags without db_query: refused before anything is stored
    before = shim.g.stats()
    with pytest.raises(native.OseError) as ei:
        _add(shim, td, 3 * S, no_query)
    assert ei.value.code == native.OSE_EINVAL and shim.g.stats() == before
    # res_sql_ok NULL: every resource passes; the flags and queries are carried
    _add(shim, td, 4 * S, no_ok)
    cols, got = released(shim, 6 * S)
    flags, queries, ok = _db_columns(cols, got)
    assert ok.all() and len(ok) == cols.n_resources and flags.any()
    assert sorted(q for q in queries if q is not None) == sorted(q for q in h_queries if q is not None)
    # a store on an engine without the section ignores the three pointers and releases them NULL
    bare = Engine({k: v for k, v in _full_cfg(sql).items() if k != "odigossqldboperationprocessor"})
    store = _Shim(bare, {"wait_duration": "1s"})

    def has_all(cols, ob):
        assert cols.db_flags and cols.db_query and cols.res_sql_ok

    store.eng = shim.eng   # (the batch is decoded by the engine with the section, so it has the columns)
    _add(store, td, 0, has_all)
    cols_b, ntr = store.g.release(2 * S)
    assert ntr == 7 and cols_b.n_spans == 65
    assert not cols_b.db_flags and not cols_b.db_query and not cols_b.res_sql_ok
    got_b = store.g.download(cols_b)
    assert "db_flags" not in got_b and "db_query" not in got_b and "res_sql_ok" not in got_b
    assert cols_b.arena_bytes == cols_p.arena_bytes   # no query bytes in its blocks


@pytest.mark.gpu
def test_gpu_three_workers_with_queries():
    # the small case of test_gpu_num_workers_rings, every span with a query:
    # per-worker eviction plus the new columns.  Rings of 4 ids and about 2 new
    # traces per worker and second: with a wait of 1 s and a release every
    # 2 s, the traces of the even steps leave in time and some of the odd
    # steps' are evicted first.
    workers, num_traces, per_batch = 3, 13, 6
    sql = SQL_CFGS["no_list"]
    rng = random.Random(0x3C0 + workers)
    shim = _sql_shim(sql, {"wait_duration": "1s", "num_traces": num_traces, "num_workers": workers},
                     span_capacity=1 << 15, arena_capacity=1 << 21)
    ref = GroupByTraceRef(1 * S, num_traces=num_traces, num_workers=workers)
    seen, nxt, now, total = [], 1, 0, 0

    def check(now):
        r = _check_release(shim, ref, now, sql)
        if r is None:
            return 0
        flags = _db_columns(r[0], r[1])[0]
        assert (flags & HAS_QUERY).all()
        r[4].close()
        return r[7]

    for step in range(30):
        now += S
        back = rng.sample(seen, min(len(seen), per_batch // 3))
        ref._expire(now)
        waiting = lambda k: ref.live.get(_tid(k)) in ref.inst  # noqa: E731
        back = [k for k in back if waiting(k)] + [k for k in back if not waiting(k)]
        fresh = list(range(nxt, nxt + per_batch))
        nxt += per_batch
        seen += fresh
        td = _mk(back + fresh, "w%d-" % step, svc=rng.choice(["svc-a", "svc-b"]), qlen=20 + step * 9)
        _add(shim, td, now)
        ref.consume(td, now)
        if step % 2 == 1:
            total += check(now)
    assert ref.evicted > 0 and total > 0
    total += check(now + 10 * S)
    st = shim.g.stats()
    assert st["evicted"] == ref.evicted and st["waiting_traces"] == 0 and st["released"] == total
