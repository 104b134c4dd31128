"""SAMPLE | TEMPLATE | TEMPLATE_REFS | SIZE by trace id with the plan and the
spans pass cut into K slices (engine.cpp run_stages, kernels.hpp UrlSlices;
the engine option "url_tail_slices" forces K and the fork at any span
count), against the oracle chain as tests/test_tail_order.py builds it and
against the same engine at K = 1, both exact.

What a slice can get wrong, and the batch that shows it:
* its group range: span counts around one group, around K groups (fewer
  groups than slices, a slice of exactly one group, a last slice holding
  one partial group) and many groups per slice;
* the per-scope sums two slices add into: a scope run and a trace across
  every slice boundary, and one scope per span on both sides of each;
* the order plan -> slow plan -> spans pass within a slice: unplanned
  groups (tests/url_layouts.py's builders) as the first and the last group
  of a slice, in every slice and with one slice holding none, the engine's
  path counts equal to the layout's census;
* the lists shared by all slices: groups that go to url_emit_slow_kernel
  in the first and in the last slice, the refs bump when the arena is too
  small, the repeated-id path of the trace stage (the final keep bytes).
"""
import ctypes as C

import numpy as np
import pytest

from odigos_amd import native
from odigos_amd.batch import DeviceBatch, Engine, Generator
from tests import url_layouts as ul
from tests.oracle_lib import span_template_bytes
from tests.test_tail_order import FUSED, RULES, _cfg, _check, _oracle

SEED = 0x5EED
KS = (2, 3, 4, 8)
FORMS = {"in_order": 1, "staggered": 2}   # the option "url_tail_form"'s values
MAX_SLICES = 8
WAVE = 64


def slice_bounds(n_groups, k, form):
    out = (C.c_uint32 * 20)()
    native.lib().osehost_url_slices(n_groups, k, FORMS[form] - 1, out)
    return [int(out[2 + j]) for j in range(k + 1)]


class _Batch:
    """A generated batch with some columns replaced (numpy arrays kept here),
    its oracle result and its result at K = 1 per engine, each built once."""

    def __init__(self, g, dims=None, **columns):
        self.g = g
        self.cols = native.Columns.from_buffer_copy(g.cols)
        self.keep = {k: np.ascontiguousarray(v) for k, v in columns.items()}
        for name, a in self.keep.items():
            setattr(self.cols, name, a.ctypes.data)
        for name, v in (dims or {}).items():
            setattr(self.cols, name, v)
        self._oracle = {}
        self._one = {}

    def oracle(self, cfg):
        key = repr(cfg)
        if key not in self._oracle:
            self._oracle[key] = _oracle(self.cols, FUSED, cfg, SEED)
        return self._oracle[key]


_ENGINES = {}


def engine(cfg):
    key = repr(cfg)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(cfg)
        _ENGINES[key].set_option("url_path_counts", 1)
    return _ENGINES[key]


def run(eng, b, k, form="in_order", calls=1, tmpl_cap=None):
    import torch
    eng.set_option("url_tail_slices", k)
    eng.set_option("url_tail_form", FORMS[form])
    try:
        db = DeviceBatch(b.cols, tmpl_cap=tmpl_cap)
        for name in ("keep", "url_out", "tmpl", "res_bytes", "tmpl_arena"):
            db.o[name].fill_(0xEE)
        for _ in range(calls):
            eng.process_device(db, FUSED, native.GROUP_TRACE_ID, seed=SEED)
        torch.cuda.synchronize()
    finally:
        eng.set_option("url_tail_slices", 0)
        eng.set_option("url_tail_form", 0)
    return db


def fields(db, cols):
    ns, A, R = cols.n_spans, cols.n_attrsets, cols.n_resources
    url_out = db.out_numpy("url_out")[:ns].copy()
    tb = span_template_bytes(db.out_numpy("tmpl", np.uint32)[: 2 * ns], db.out_numpy("tmpl_arena")[: db.used()], url_out != 0)
    return {"keep": db.out_numpy("keep")[:ns].copy(), "url_out": url_out, "tmpl_len": tb[1], "tmpl_bytes": tb[0],
            "res_bytes": db.out_numpy("res_bytes", np.uint64)[:R].copy(),
            "attrset_bytes": db.out_numpy("attrset_bytes", np.int64)[:A].copy(),
            "accepted_spans": db.out_numpy("accepted_spans", np.int64)[:1].copy(),
            "device_status": db.out_numpy("device_status", np.uint32)[:1].copy()}


def check(b, cfg, k, form):
    """K slices against the oracle chain and against the same engine at K = 1."""
    eng = engine(cfg)
    db = run(eng, b, k, form)
    counts = eng.path_counts()
    _check(db, b.oracle(cfg), b.cols, FUSED)
    key = repr(cfg)
    if key not in b._one:
        one = run(eng, b, 1)
        b._one[key] = (fields(one, b.cols), eng.path_counts())
    want, want_counts = b._one[key]
    got = fields(db, b.cols)
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert (counts["url_unplanned"], counts["url_slow"]) == (want_counts["url_unplanned"], want_counts["url_slow"])
    return counts


_GEN = {}


def generated(n):
    if n not in _GEN:
        _GEN[n] = _Batch(Generator("fused", seed=0x0D160100 + n, n_spans=n))
        assert _GEN[n].cols.n_spans == n
    return _GEN[n]


# ---------------------------------------------------------------------------
# span counts

def _span_counts(k):
    return (1, 63, 64, 65, 130, 64 * k, 64 * k + 1, 8192)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", KS)
def test_gpu_slices_span_counts(k, form):
    for n in _span_counts(k):
        check(generated(n), _cfg(), k, form)


# ---------------------------------------------------------------------------
# scopes and a trace across the slice boundaries

N_B = 8192


def _boundary_batch(k, form, scopes):
    src = generated(N_B)
    n = N_B
    bounds = [WAVE * g for g in slice_bounds(n // WAVE, k, form)[1:-1]]
    assert bounds and all(0 < b < n for b in bounds)
    if scopes == "run":       # one scope run across every boundary
        scope = np.zeros(n, dtype=np.uint32)
        scope[bounds[0] - 100:] = 1
        scope[bounds[-1] + 100:] = 2
    else:                     # one scope per span on both sides of each boundary
        inc = np.zeros(n, dtype=np.int64)
        for b in bounds:
            inc[b - 2:b + 3] = 1
        scope = np.cumsum(inc).astype(np.uint32)
    n_scopes = int(scope[-1]) + 1
    tid = src.g.array("trace_id").view(np.uint64).reshape(-1, 2)[:n].copy()
    tid[bounds[0] - 3:bounds[-1] + 3] = tid[bounds[0] - 3]     # one trace across every boundary
    rng = np.random.default_rng(k)
    return _Batch(src.g, dims={"n_scopes": n_scopes, "n_resources": 1}, scope=scope, trace_id=tid.reshape(-1),
                  resource=np.zeros(n, dtype=np.uint32), scope_resource=np.zeros(n_scopes, dtype=np.uint32),
                  scope_size=rng.integers(20, 60, n_scopes, dtype=np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("scopes", ["run", "per_span"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", KS)
def test_gpu_slices_scopes_across_boundaries(k, form, scopes):
    check(_boundary_batch(k, form, scopes), _cfg(), k, form)


# ---------------------------------------------------------------------------
# unplanned groups at the slices' edges

N_G = 32   # groups of the laid batches: at least four per slice


def _unplanned_group(kind, salt):
    if kind == 0:     # a byte range past the 3 KB stage, and more chunks than the gather takes
        return ul._g_slow_subsets()[0]
    if kind == 1:     # 193 segments
        return ul._g_segcap()[5]
    return ul._g_seg6465()[1]   # 65-byte segments


def _laid_batch(name, seam_groups, extra=None):
    """N_G groups: ordinary ones, seam_groups {group: lanes} in their places.
    The generated batch's arena (its route strings) stays in front of the
    laid paths."""
    src = generated(N_G * WAVE)
    groups = [seam_groups.get(g) or ul.ordinary(WAVE, g) for g in range(N_G)]
    garena = np.zeros((src.cols.arena_bytes + 63) // 64 * 64, dtype=np.uint8)
    garena[: src.cols.arena_bytes] = src.g.array("arena")[: src.cols.arena_bytes]
    empty = (garena, np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
    L = ul.Layout(name, groups, seed=len(name), prefix=empty)
    assert L.n == N_G * WAVE
    # (no res_url_ok column: every resource passes, as the layout's census assumes)
    b = _Batch(src.g, dims={"arena_bytes": L.arena_bytes, "res_url_ok": None}, arena=L.arena, path=L._path_flat,
               url_flags=L.flags, kind=L.kind)
    b.layout = L
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["every_slice", "one_slice_none"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", KS)
def test_gpu_slices_unplanned_at_edges(k, form, where):
    g = slice_bounds(N_G, k, form)
    seams, j = {}, 0
    for s in range(k):
        if where == "one_slice_none" and s == 1:
            continue
        for at in sorted({g[s], g[s + 1] - 1}):     # the slice's first and last group
            seams[at] = _unplanned_group(j % 3, j)
            j += 1
    b = _laid_batch(f"slices.{k}.{form}.{where}", seams)
    census = b.layout.expect()
    assert census["url_unplanned"] == len(seams)
    counts = check(b, _cfg(), k, form)
    assert counts["url_unplanned"] == census["url_unplanned"]
    assert counts["url_slow"] == census["url_slow"]


# ---------------------------------------------------------------------------
# groups for url_emit_slow_kernel (a user rule matches) in the first and the last slice

@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", KS)
def test_gpu_slices_rule_groups_first_and_last(k, form):
    rule = [ul.Lane(b"/users/bob/orders/123"), ul.Lane(b"/users/al/orders/7", at=(1, 0), flags=ul.RAW | ul.EQ),
            ul.Lane(b"/api/v1/things")]
    b = _laid_batch(f"slices.rules.{k}", {0: ul.grp(rule), N_G - 1: ul.grp(rule, before=40, salt=3)})
    counts = check(b, _cfg(RULES), k, form)
    assert counts["url_slow"] >= 2


# ---------------------------------------------------------------------------
# the trace stage's repeated-id path: the spans pass must see the final keep

@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("k", (2, 8))
def test_gpu_slices_repeated_trace_ids(k, form):
    src = generated(N_B)
    tid = src.g.array("trace_id").view(np.uint64).reshape(-1, 2)[:N_B].copy()
    tid[5000:5200] = tid[100:300]      # the ids of one part of the batch again in another
    tid[8000:8100] = tid[100:200]
    b = _Batch(src.g, trace_id=tid.reshape(-1))
    eng = engine(_cfg())
    before = eng.path_counts()
    check(b, _cfg(), k, form)
    after = eng.path_counts()
    assert after["run_list"] + after["sort"] > before["run_list"] + before["sort"]


# ---------------------------------------------------------------------------
# the template arena: too small, and what the slices leave unused

def _plan_waves(n_groups, k, form):
    g = slice_bounds(n_groups, k, form)
    return sum(4 * ((g[s + 1] - g[s] + 3) // 4) for s in range(k))   # four waves per workgroup


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_slices_arena_too_small(form):
    b = generated(N_B)
    eng = engine(_cfg())
    small = 4096
    db = run(eng, b, 4, form, tmpl_cap=small)
    assert int(db.out_numpy("device_status", np.uint32)[0]) & 2
    need = db.used()
    assert need > small
    db2 = run(eng, b, 4, form, tmpl_cap=need)          # what the shim retries with
    assert int(db2.out_numpy("device_status", np.uint32)[0]) == 0
    _check(db2, b.oracle(_cfg()), b.cols, FUSED)
    # a fitting arena: the slices' waves leave no more unused than one chunk each
    cap = db2.outs.tmpl_arena_cap
    one = run(eng, b, 1, tmpl_cap=cap)
    assert int(one.out_numpy("device_status", np.uint32)[0]) == 0
    waves = _plan_waves(N_B // WAVE, 4, form)
    chunk = min(256 << 10, cap // 8 // waves) & ~15
    assert db2.used() <= one.used() + chunk * waves


# ---------------------------------------------------------------------------
# the counters are added to: a second call doubles them

@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_slices_second_call_doubles(form):
    b = generated(N_B)
    cfg = _cfg()
    db = run(engine(cfg), b, 3, form, calls=2)
    ho = b.oracle(cfg)
    A = b.cols.n_attrsets
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    np.testing.assert_array_equal(db.out_numpy("attrset_bytes", np.int64)[:A], 2 * ho.view("attrset_bytes", np.int64)[:A])
    assert int(db.out_numpy("accepted_spans", np.int64)[0]) == 2 * int(ho.view("accepted_spans", np.int64)[0])
    np.testing.assert_array_equal(db.out_numpy("keep")[:N_B], ho.view("keep", np.uint8)[:N_B])


# ---------------------------------------------------------------------------
# the option back at 0: a small call queues what it always did

def _launches(eng, b, calls=2):
    import torch
    eng.profile(True)
    eng.profile_read()
    db = DeviceBatch(b.cols)
    for _ in range(calls):
        eng.process_device(db, FUSED, native.GROUP_TRACE_ID, seed=SEED)
    torch.cuda.synchronize()
    out = {name: v["launches"] for name, v in eng.profile_read().items()}
    eng.profile(False)
    return out


@pytest.mark.gpu
def test_gpu_slices_option_off_queues_the_usual_launches():
    b = generated(N_B)
    eng = Engine(_cfg())
    run(eng, b, 4)                      # forced, then back at 0
    got = _launches(eng, b)
    fresh = _launches(Engine(_cfg()), b)
    assert got == fresh
    assert got["url_plan_kernel"] == 2 and got["url_plan_slow_kernel"] == 2 and got["url_copy_kernel"] == 2
    eng.set_option("url_tail_slices", 4)
    forced = _launches(eng, b)
    eng.set_option("url_tail_slices", 0)
    assert forced["url_plan_kernel"] == 8 and forced["url_copy_kernel"] == 8
