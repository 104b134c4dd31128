"""The groupbytrace store (gbt_kernel.hip, gbt_host.cpp) on hand-laid column
batches at every seam of its state machine (tests/gbt_layouts.py): the pool,
scope and arena rings' ends and refusals, the id table's floor, growth,
rebuild, wrapped and tombstoned probe chains, the release sort's pass counts,
the ring of ids with more creations than slots in one add, the per-worker
rings, the clock's edges, and the same seams on a store that carries the
odigossqldboperationprocessor columns.

CPU: the column-level restatement against tests/gbt_ref.py (the Go-level
one) and against cases worked by hand; a census that shows every layout on
the seam it was laid for; the constants the layouts are laid against.
GPU: every step of every layout — each released column, the arena bytes,
n_traces, stats() and the host's bookkeeping (osehost_gbt_state) — equals the
restatement and the census exactly.  Everything is integers and bytes: there
are no tolerances.
"""
import ctypes as C
import random

import numpy as np
import pytest

from odigos_amd import host, native
from tests import gbt_layouts as gl
from tests.gbt_layouts import SEC, Batch, Store, lay, tid
from tests.gbt_ref import GroupByTraceRef
from tests.test_otlp import CFG

CFG_K0 = {"odigossampling": {"global_rules": [{"name": "errors", "type": "error",
                                               "rule_details": {"fallback_sampling_ratio": 40}}]}}
CFG_SQL = dict(CFG, odigossqldboperationprocessor={})


# ---- CPU ----------------------------------------------------------------------------

def test_constants_as_designed():
    assert {k: getattr(gl.K, k) for k in gl.DESIGNED} == gl.DESIGNED


def test_hashes():
    # splitmix64's published first output for state 0, and the slot search
    assert gl.splitmix64(0) == 0xE220A8397B1DCDAF
    ids = gl.ids_for_slot(1020, 1023, 5, seed=3)
    assert len(set(ids)) == 5 and all(gl.tid_hash(h, l) & 1023 == 1020 for h, l in ids)
    # FNV-1 as tests/gbt_ref.py has it (pinned there by Go's hash/fnv vectors)
    from tests.gbt_ref import worker_index
    for k in range(50):
        h, l = tid(k)
        assert gl.worker_of(h, l, 7) == worker_index("%016x%016x" % (h, l), 7)


def _starts(r):
    """[(trace id, [start_ns, ...]), ...] of a restated release"""
    out = []
    for j in range(r.n_spans):
        if j == 0 or r.trace_of_span[j] != r.trace_of_span[j - 1]:
            out.append((tuple(int(x) for x in r.cols["trace_id"][j]), []))
        out[-1][1].append(int(r.cols["start_ns"][j]))
    return out


def _ref_starts(traces):
    out = []
    for pieces in traces:
        spans = [sp for p in pieces for sp in p["scopeSpans"][0]["spans"]]
        t = spans[0]["traceId"]
        out.append(((int(t[:16], 16), int(t[16:], 16)), [int(sp["startTimeUnixNano"]) for sp in spans]))
    return out


@pytest.mark.parametrize("workers,num_traces", [(1, 1_000_000), (1, 40), (3, 60)])
def test_restatement_agrees_with_gbt_ref(workers, num_traces):
    # the same small trees to both: the host columniser's columns to the
    # column-level restatement, the dicts to the Go-level one.  Ids come back
    # only in later adds and no add creates more than a ring holds, so no id
    # is evicted by a creation of its own add (the documented divergence)
    rng = random.Random(0x6B7 + workers)
    proc = host.Processor("pipeline", CFG)
    st = Store(3 * SEC, num_traces, workers)
    ref = GroupByTraceRef(3 * SEC, num_traces=num_traces, num_workers=workers)
    now, nxt, seen, uid, total = 0, 0, [], 0, 0
    for step in range(24):
        now += rng.choice([SEC // 2, SEC, 2 * SEC])
        ref._expire(now)
        back = [k for k in rng.sample(seen, min(len(seen), 4))]
        waiting = lambda k: ref.live.get("%032x" % (k + 1)) in ref.inst   # noqa: E731
        back = [k for k in back if waiting(k)] + [k for k in back if not waiting(k)]
        fresh = list(range(nxt, nxt + 6))
        nxt += 6
        seen += fresh
        rss = []
        for r in range(2):
            scopes = []
            for s in range(2):
                ks = [k for k in back + fresh if (k + r + s) % 2 == 0] * (1 + s)
                spans = []
                for k in ks:
                    uid += 1
                    spans.append(host.span(f"s{uid}", kind=2, trace_id="%032x" % (k + 1), start=uid, end=uid + 3,
                                           attributes={"http.request.method": "GET", "url.path": f"/u/{k}"}))
                scopes.append({"scope": {"name": f"lib{s}"}, "spans": spans})
            rss.append(host.resource_spans({"service.name": ["svc-a", "svc-b"][r]}, scopes=scopes))
        td = host.traces(*rss)
        hb = proc.columnarize(td)
        st.add(Batch.from_columns(hb.cols), now)
        ref.consume(td, now)
        if step % 3 == 2:
            r, want = st.release(now), ref.release(now)
            assert _starts(r) == _ref_starts(want), step
            assert r.n_fragments == sum(len(p) for p in want) and r.n_traces == len(want)
            total += len(want)
    r, want = st.release(now + 10 * SEC), ref.release(now + 10 * SEC)
    assert _starts(r) == _ref_starts(want)
    s = st.stats()
    assert s["released"] == total + len(want) > 0 and s["evicted"] == ref.evicted and s["waiting_traces"] == 0
    assert (ref.evicted > 0) == (num_traces < 1000)


def _plain(ids, starts):
    b = lay(ids)
    b.start_ns = np.asarray(starts, np.uint64)
    return b


def test_hand_worked_expired_id():
    # test_gpu_expired_id_hand_worked's case (worked from contrib's timer
    # semantics): trace 1 is past its 10 s wait at 11 s, so its spans in the 11 s
    # batch start a new trace; new traces are numbered by first appearance (2,
    # 1, 3) and leave in that order, each trace's spans in arrival order
    st = Store(10 * SEC)
    st.add(_plain([tid(1)], [1]), 0)
    st.add(_plain([tid(k) for k in (2, 1, 1, 2, 3, 1)], [100, 101, 102, 103, 104, 105]), 11 * SEC)
    r = st.release(12 * SEC)
    assert (r.n_traces, r.cols["start_ns"].tolist()) == (1, [1])
    r = st.release(25 * SEC)
    assert (r.n_traces, r.cols["start_ns"].tolist()) == (3, [100, 103, 101, 102, 105, 104])


def test_documented_divergence_same_add_eviction():
    # num_traces 2.  add 1: ids A, B -> traces 0, 1.  add 2: C, A, D.  As of the
    # start of add 2 trace 0 (A) waits, so A's span (start 21) joins it; C and D
    # become traces 2 and 3, and a ring of 2 then holds only those: traces 0 and
    # 1 are evicted, and A's span of add 2 is lost with trace 0.  (contrib
    # handles the pieces one by one: C evicts A's trace, so A's piece starts a
    # new one, which D evicts... the store applies eviction per add, DESIGN.md
    # §4.7.)  The release holds C then D; two traces were dropped.
    A, B_, Cc, D = (tid(k) for k in range(4))
    st = Store(10 * SEC, num_traces=2)
    assert st.add(_plain([A, B_], [10, 11]), 0) == 2
    assert st.add(_plain([Cc, A, D], [20, 21, 22]), SEC) == 2
    assert st.stats()["waiting_traces"] == 2
    r = st.release(20 * SEC)
    assert (r.n_traces, r.cols["start_ns"].tolist()) == (2, [20, 22])
    assert [tuple(x) for x in r.cols["trace_id"].tolist()] == [Cc, D]
    s = st.stats()
    assert (s["evicted"], s["released"], s["released_spans"], s["added_spans"], s["held_spans"]) == (2, 2, 2, 5, 0)


def test_restated_columns_hand_worked():
    # two spans of one trace from two scopes: refs and arena bytes by hand.
    # span 0: route "ab" (2), path NULL, attr0 STR 3 bytes, attr1 INT; span 1:
    # route 0 bytes, attr0 not a string, attr1 STR 1 byte.  Blocks: 5 bytes,
    # then 1 byte.
    b = lay([tid(1), tid(1)], scope=[1, 0], n_resources=2, scope_resource=[1, 0], route=[2, 0],
            attr=[[3, None], [None, 1]], null=("path", "res_url_ok", "res_svc_str"), attrset_map=[5, 3], n_attrsets=2)
    st = Store(SEC)
    st.add(b, 0)
    r = st.release(SEC)
    c = r.cols
    assert (r.n_spans, r.n_fragments, r.n_attrsets, r.arena_bytes) == (2, 2, 6, 6)
    assert c["route"].tolist() == [[0, 2], [5, 0]] and c["path"].tolist() == [[0, 0], [5, 0]]
    assert c["attr_type"].tolist()[0] == native.ATTR_STR and int(c["attr_val"][0]) == 2 | (3 << 32)
    assert c["attr_type"].tolist()[3] == native.ATTR_STR and int(c["attr_val"][3]) == 5 | (1 << 32)
    assert int(c["attr_val"][1]) == int(b.attr_val[1]) and int(c["attr_val"][2]) == int(b.attr_val[2])
    want = np.concatenate([gl._text(0, 1, 2), gl._text(0, 3, 3), gl._text(1, 4, 1)])
    np.testing.assert_array_equal(c["arena"], want)
    # fragment 0 is span 0's scope 1 -> resource 0; fragment 1 is scope 0 -> resource 1
    assert c["res_svc"].tolist() == [int(b.res_svc[0]), int(b.res_svc[1])]
    assert c["res_svc_str"].tolist() == c["res_svc"].tolist() and c["res_url_ok"].tolist() == [1, 1]
    assert c["res_attrset"].tolist() == [5, 3] and c["scope_size"].tolist() == [int(b.scope_size[1]), int(b.scope_size[0])]
    assert c["resource"].tolist() == c["scope"].tolist() == c["scope_resource"].tolist() == [0, 1]


LAYOUTS = [(fam, k) for fam in gl.FAMILIES for k in range(len(gl.all_layouts()[fam]))]
IDS = [gl.all_layouts()[fam][k].name for fam, k in LAYOUTS]


@pytest.mark.parametrize("fam,k", LAYOUTS, ids=IDS)
def test_census(fam, k):
    L = gl.all_layouts()[fam][k]
    ex = L.expected()
    assert L.seams
    for text, pred in L.seams:
        assert pred(ex), f"{L.name}: off its seam: {text}"


# ---- GPU ----------------------------------------------------------------------------

_ENGINES = {}


def _engine(kind):
    from odigos_amd.batch import Engine
    if kind not in _ENGINES:
        _ENGINES[kind] = Engine({"plain": CFG, "k0": CFG_K0, "sql": CFG_SQL}[kind])
    return _ENGINES[kind]


def _state(g):
    v = (C.c_uint64 * len(gl.STATE))()
    assert native.lib().osehost_gbt_state(g.h, v, len(gl.STATE)) == len(gl.STATE)
    return tuple(v)


def _compare(L, step, cols, got, want):
    where = f"{L.name} step {step}"
    assert (cols.n_spans, cols.n_resources, cols.n_scopes, cols.n_attrsets, cols.arena_bytes) == \
        (want.n_spans, want.n_fragments, want.n_fragments, want.n_attrsets, want.arena_bytes), where
    assert sorted(got) == sorted(want.cols), where
    for name, w in want.cols.items():
        w = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        np.testing.assert_array_equal(got[name][:len(w)], w, err_msg=f"{where}: {name}")


def _play(L):
    from odigos_amd.batch import DeviceBatch, GroupByTrace
    eng = _engine(L.engine)
    assert eng.info().n_attr_keys == L.K
    g = GroupByTrace(eng, L.cfg, L.span_cap, L.arena_cap)
    try:
        for step, ((kind, b, now), e) in enumerate(zip(L.steps, L.expected())):
            where = f"{L.name} step {step}"
            if kind == "add":
                db = DeviceBatch(b.columns())
                if e.refused is None:
                    g.add(db.cols, now, b.attrset_map)
                else:
                    with pytest.raises(native.OseError) as ei:
                        g.add(db.cols, now, b.attrset_map)
                    assert ei.value.code == e.refused, where
            else:
                cols, ntr = g.release(now)
                assert ntr == e.released.n_traces, where
                _compare(L, step, cols, g.download(cols), e.released)
            assert g.stats() == e.stats, where
            assert dict(zip(gl.STATE, _state(g))) == dict(zip(gl.STATE, e.state)), where
    finally:
        g.close()


def _family(fam):
    for L in gl.all_layouts()[fam]:
        _play(L)


@pytest.mark.gpu
def test_gpu_blocks():
    _family("blocks")


@pytest.mark.gpu
def test_gpu_pool_ring():
    _family("pool_ring")


@pytest.mark.gpu
def test_gpu_scope_ring():
    _family("scope_ring")


@pytest.mark.gpu
def test_gpu_arena_ring():
    _family("arena_ring")


@pytest.mark.gpu
def test_gpu_id_table():
    _family("id_table")


@pytest.mark.gpu
def test_gpu_sort():
    _family("sort")


@pytest.mark.gpu
def test_gpu_id_ring():
    _family("id_ring")


@pytest.mark.gpu
def test_gpu_workers():
    _family("workers")


@pytest.mark.gpu
def test_gpu_clock():
    _family("clock")


@pytest.mark.gpu
def test_gpu_sql_pass():
    _family("sql")
