"""The size stage on hand-laid batches: one named layout per seam of
size_span_kernel, size_tail_kernel (size_tail_window) and size_fix_kernel,
and of the same spans pass fused into url_copy_kernel, each compared with the
oracle bit for bit (tests/size_layouts.py builds them).

The generator's batches have one scope per resource and 256 attribute sets,
so they never lay a resource run over two scopes, a scopeless resource or a
walk of size_fix_kernel.  Here every layout's census (computed from the built
columns alone) first proves that the batch holds its seam, the C oracle is
pinned against the Python restatement on it, and then the HIP stage must give
the oracle's res_bytes, attrset_bytes and accepted_spans.  The device outputs
are prefilled: res_bytes with 0xEE bytes (every entry is written on every
call), the counters with non-zero values (they are added to).

Layout                  guards (constant / code line)
----------------------  ---------------------------------------------------
run.ends                wave_seg_sum's DPP steps (row_shr 1/2/4/8, row_bcast
                        15/31): run tails on lanes 0, 1, 15, 16, 31, 32, 47,
                        48, 62, 63; 64 runs of one scope; keys changing at
                        every row edge; a run ending on lane 63 before a
                        resource starting on lane 0 (`after != rl`,
                        `before != r0`)
run.cross               the part slots and `fix`: lane 63 -> lane 0, lane 1
                        -> lane 62 of the next window, last run of a
                        multi-run window -> first of the next
run.long                size_fix_kernel's walk: 3, 4 and 6 windows visited;
                        stopping on the `whole_head` bit; `single &&
                        whole_tail`; a whole-window run without a flag
run.tiles               kSThreads / kTailTiles: runs over scope 255/256, over
                        one block's in-flight tiles, over 1024 scopes
gaps.1/2/300, gaps.S0   scopeless resources before the first scope, inside a
                        window, at lane 0 (`before`), after the last scope
                        (`s + 1 == S`); the `S == 0` loop and its grid-stride
ends.S                  `lastv < 63`, the `na` load on lane `lastv`, windows
                        with `vmask == 0`
removed                 `remove_empty && had && alive == 0` over part slots
attrsets.2048/2049      kLdsAttrsets: the LDS histogram and the global atomics
tail.stride             OSE_SIZE_TAIL_CAP: size_tail_kernel's second iteration
scope.runs              the spans pass's waves: tails on the same lanes, a
                        scope over waves and blocks, a dropped wave, a partial
                        last wave
span.stride.n           launch_size_spans' cap: the x1 tile and the second
                        iteration
varints                 sov / field_len at every level and byte boundary
*.paths                 the spans pass inside url_copy_kernel<true, false>
                        (packed) and <true, true> (refs), kept_partials
"""
import json

import numpy as np
import pytest

from odigos_amd import native
from odigos_amd.batch import HostOutputs
from tests import size_layouts as sl
from tests.oracle_lib import SamplingOracle, size_process
from tests.size_layouts import K, TAIL_LANES, TILE, WAVE, census, layout, tail_lanes

SIZE = native.STAGE_SIZE
APPLIED = native.STAGE_SIZE | native.STAGE_APPLY_KEEP | native.STAGE_APPLY_TEMPLATE
FUSED = native.STAGE_SIZE | native.STAGE_APPLY_KEEP | native.STAGE_TEMPLATE
REFS = FUSED | native.STAGE_TEMPLATE_REFS
TRAFFIC = {"res_attributes_keys": ["service.name"]}
SMALL, LARGE = list(sl.SMALL), list(sl.LARGE)


# ---------------------------------------------------------------------------
# constants

def test_constants_as_designed():
    # the layouts were drawn for these values: retuning one moves a seam, and
    # the layouts (and the table in this module's docstring) move with it
    got = {k: getattr(K, k) for k in sl.DESIGNED}
    assert got == sl.DESIGNED, "a size-stage constant changed: re-lay tests/size_layouts.py against it"
    assert sl.TAIL_STRIDE == 4_194_304 and sl.SPAN_STRIDE == 262_144
    assert sl.SPAN_STRIDE_NS == [262_144, 262_145, 524_288, 524_326]


def test_varint_lengths():
    for k in range(1, 9):
        for v in ((1 << 7 * k) - 1, 1 << 7 * k):
            assert int(sl.sov(v)) == sl.sov_int(v) == (k if v < (1 << 7 * k) else k + 1)
    assert int(sl.sov(0)) == sl.sov_int(0) == 1
    assert int(sl.field_len(127)) == 129 and int(sl.field_len(128)) == 131


# ---------------------------------------------------------------------------
# the two references

def _flags(stages, mode=native.GROUP_TRACE_ID):
    """(sampled, templated, remove_empty) of a device call (size_host.cpp prepare_size)."""
    applied = bool(stages & native.STAGE_APPLY_KEEP)
    sampled = bool(stages & native.STAGE_SAMPLE) or applied
    templated = bool(stages & (native.STAGE_TEMPLATE | native.STAGE_APPLY_TEMPLATE))
    return sampled, templated, applied or (sampled and mode == native.GROUP_TRACE_ID)


def oracle_mask(stages):
    """The mask oracle/size.c understands for a device call: it tests
    OSE_STAGE_TEMPLATE to apply url_out / tmpl, wherever they were written."""
    if stages & native.STAGE_APPLY_TEMPLATE:
        stages = (stages & ~native.STAGE_APPLY_TEMPLATE) | native.STAGE_TEMPLATE
    return stages & ~native.STAGE_TEMPLATE_REFS


def oracle(L, stages, inverse=1, ratio=1.0, u=0.0, mode=native.GROUP_TRACE_ID, sampling=None, seed=0):
    """(res_bytes[R], attrset_bytes[A], accepted_spans) oracle/size.c adds for one call."""
    ho = HostOutputs(L.cols)
    n = L.n
    ho.view("keep", np.uint8)[:n] = L.keep
    ho.view("url_out", np.uint8)[:n] = L.url_out
    ho.view("tmpl", np.uint32)[:2 * n] = L.tmpl.reshape(-1)
    if sampling is not None:
        assert SamplingOracle(sampling).process(L.cols, ho.outs, mode, seed) == 0
    assert size_process(L.cols, ho.outs, oracle_mask(stages), mode, ho.outs, inverse, ratio, u) == 0
    return (ho.view("res_bytes", np.uint64)[:L.R].copy(), ho.view("attrset_bytes", np.int64)[:L.A].copy(),
            int(ho.view("accepted_spans", np.int64)[0]))


def check_references(L, stages=(SIZE, APPLIED), inverse=1):
    for st in stages:
        sampled, templated, remove = _flags(st)
        want = sl.restate(L, sampled, templated, remove, inverse)
        got = oracle(L, st, inverse=inverse, ratio=1.0 / inverse)
        np.testing.assert_array_equal(got[0], want[0], err_msg=f"{L.name} res_bytes, stages {st:#x}")
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"{L.name} attrset_bytes, stages {st:#x}")
        assert got[2] == want[2], (L.name, st)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_is_the_restatement(name):
    check_references(layout(name))


@pytest.mark.parametrize("name", [f + ".paths" for f in sl.FUSED])
def test_oracle_is_the_restatement_fused(name):
    L = layout(name)
    assert (L.url_out != 0).sum() > L.n // 3 and len(set(L.tmpl_len[L.url_out != 0].tolist())) >= 4
    assert int(L.tmpl_len.max()) > 127                      # a template whose length varint takes two bytes
    assert {1, 2, 3} <= set(L.url_out.tolist())
    check_references(L, stages=(FUSED,))


def test_oracle_is_the_restatement_inverse():
    check_references(layout(f"attrsets.{K.kLdsAttrsets + 1}"), inverse=4)


@pytest.mark.parametrize("name", LARGE)
def test_oracle_is_the_restatement_large(name):
    L = layout(name)
    try:
        CENSUS[name.rsplit(".", 1)[0] if name.startswith("span") else name](L, census(L))
        check_references(L)
    finally:
        sl.drop(name)


# ---------------------------------------------------------------------------
# census: each layout holds its seam (from the built columns alone)

def _run_of(L, r):
    """(first scope, exclusive end) of resource r's run."""
    a = int(L.res_scopes[:r].sum())
    return a, a + int(L.res_scopes[r])


def _no_gaps(c):
    assert c.gap_first == c.gap_inner == c.gap_lane0 == c.gap_after == c.gap_s0 == 0


def census_run_ends(L, c):
    assert c.fix == 0 and c.cut_head == c.cut_tail == 0 and c.in_window == L.R and c.walks == []
    assert tail_lanes(c.tails, 0) == list(range(64))                       # 64 runs of one scope
    assert tail_lanes(c.tails, 1) == [15, 31, 47, 63]                      # keys change at every row edge
    assert tail_lanes(c.tails, 2) == TAIL_LANES
    assert L.scope_resource[3 * WAVE - 1] != L.scope_resource[3 * WAVE]    # lane 63 ends a run, lane 0 starts one
    assert tail_lanes(c.tails, 3) == [2, 63]
    assert L.S % WAVE == 10 and tail_lanes(c.tails, 4) == [3, 9]
    _no_gaps(c)


def census_run_cross(L, c):
    m = L.marks
    assert _run_of(L, m["A"]) == (63, 65)
    assert _run_of(L, m["B"]) == (WAVE + 1, 2 * WAVE + 63)
    assert _run_of(L, m["C"]) == (2 * WAVE + 63, 3 * WAVE + 10)
    assert c.fix_windows == [1, 2, 3] and c.walks == [1, 1, 1]
    assert c.cut_head == c.cut_tail == 3 and c.cut_both == 0 and c.in_window == L.R - 3
    assert len(tail_lanes(c.tails, 2)) == 2 and len(tail_lanes(c.tails, 3)) == 3      # multi-run windows
    _no_gaps(c)


def census_run_long(L, c):
    m = L.marks
    lane = lambda s: s % WAVE
    for name, whole in (("L2", 2), ("L3", 3), ("L5", 5)):
        a, e = _run_of(L, m[name])
        assert lane(a) == 40 and lane(e) == 21 and (e - 1) // WAVE - a // WAVE == whole + 1
    a, e = _run_of(L, m["H0"])
    assert lane(a) == 0 and lane(e) == 10 and e - a == 74
    a, e = _run_of(L, m["E63"])
    assert lane(a) == 30 and lane(e) == 0 and e - a == 98
    assert _run_of(L, m["ONE"]) == (17 * WAVE, 18 * WAVE) and _run_of(L, m["TWO"]) == (18 * WAVE, 20 * WAVE)
    # the windows holding each run's end, and what each walk visits
    assert c.fix_windows == [3, 7, 13, 15, 16, 19] and c.walks == [3, 4, 6, 1, 1, 1]
    assert c.in_window == 9 and c.cut_both == 2 + 3 + 5 + 0 + 0 + 0        # windows that are one cut run alone
    _no_gaps(c)


def census_run_tiles(L, c):
    m = L.marks
    a, e = _run_of(L, m["X"])
    assert a < TILE - 1 and e > TILE + 1                                   # over scope 255 / 256
    a, e = _run_of(L, m["BIG"])
    assert e - a > 4 * TILE and c.tail_blocks == 3 and c.tail_iters == 1
    gstride = c.tail_blocks * TILE
    assert a < gstride - 1 and e > gstride + TILE                          # block 0's second in-flight tile, whole
    assert max(c.walks) == (e - 1) // WAVE - a // WAVE == 19
    _no_gaps(c)


def census_gaps(g):
    def check(L, c):
        assert (c.gap_first, c.gap_inner, c.gap_lane0, c.gap_after, c.gap_s0) == (g, g, g, g, 0)
        assert c.gap_sizes == [g] and L.R == 6 + 4 * g
        a, e = _run_of(L, 2 * g + 2)
        assert e == WAVE                                                   # the run before the lane-0 gap ends on lane 63
    return check


def census_s0(R):
    def check(L, c):
        assert L.S == 0 and L.n == 0 and c.gap_s0 == R == L.R
        assert c.tail_blocks == min(-(-R // TILE), K.s0_cap)
        assert c.s0_second_iter == (R > K.s0_cap * TILE)
    return check


def census_ends(S):
    def check(L, c):
        assert L.S == S and int(L.scope_resource[-1]) == L.R - 1 and c.gap_after == 0
        tiles = -(-S // TILE)
        launched = -(-tiles // K.tail_tiles) * K.tail_tiles * (TILE // WAVE)
        assert c.empty_windows == launched - -(-S // WAVE)
        assert (S - 1) % WAVE in tail_lanes(c.tails, (S - 1) // WAVE)      # lastv ends the last run
        _no_gaps(c)
    return check


def census_removed(L, c):
    m = L.marks
    want = sl.restate(L, True, True, True)[0]
    stay = sl.restate(L, False, False, False)[0]
    a, e = _run_of(L, m["EMPTY"])
    assert (a % WAVE, e - a) == (60, 8) and want[m["EMPTY"]] == 0 and stay[m["EMPTY"]] > 0
    a, e = _run_of(L, m["STAYS"])
    assert a // WAVE + 1 == (e - 1) // WAVE and want[m["STAYS"]] > 0
    assert int((L.scope_spans[a:e] == 0).sum()) == 1
    a, e = _run_of(L, m["CARRY"])
    assert L.scope_spans[a] > 0 and not L.scope_spans[a + 1:e].any() and (e - 1) // WAVE - a // WAVE == 4
    assert want[m["LAST_EMPTY"]] == 0
    assert (want == 0).sum() == 2 and (stay == 0).sum() == 0
    assert c.walks == [1, 1, 4]
    _no_gaps(c)


def census_attrsets(A):
    def check(L, c):
        assert L.A == A and (A <= K.kLdsAttrsets) == (A == K.kLdsAttrsets)
        used = set(L.res_attrset.tolist())
        assert used == {7, 0, K.kLdsAttrsets - 1, A - 1}
        assert c.tail_blocks >= 3 and c.gap_inner == 30 and c.fix == 39
        blocks_of = {}
        for r in np.nonzero(L.res_attrset == 7)[0][::17]:
            blocks_of[_run_of(L, int(r))[0] // (K.tail_tiles * TILE)] = True
        assert len(blocks_of) >= 3                                         # one set, several blocks
        fixed = {int(L.scope_resource[w * WAVE]) for w in c.fix_windows}
        for a in L.marks["sets"]:
            rs = set(np.nonzero(L.res_attrset == a)[0].tolist())
            assert any(L.res_scopes[r] == 0 for r in rs) and rs & fixed
    return check


def census_tail_stride(L, c):
    assert L.S == sl.TAIL_STRIDE + TILE + 1 and c.tail_blocks == K.tail_cap
    assert c.tail_second_iter and c.tail_iters == 2
    a, e = _run_of(L, L.marks["X"])
    assert (a, e) == (sl.TAIL_STRIDE - 2, sl.TAIL_STRIDE + 2)              # over the first iteration's last scope
    assert int(L.res_scopes.max()) <= 4 and 2000 < L.n < 5000
    sc = L.scope
    assert (sc < TILE).any() and (sc >= L.S - TILE).any() and ((sc >= a) & (sc < e)).any()
    assert ((sc >= TILE) & (sc < a)).sum() == 0
    assert c.fix > 10_000 and set(c.walks) == {1}
    # the second iteration has two blocks: a whole tile and a tile of one scope, their other tile slots empty
    wpt = TILE // WAVE
    assert c.empty_windows == 2 * (K.tail_tiles - 1) * wpt + (wpt - 1)


def census_scope_runs(L, c):
    m = L.marks
    assert tail_lanes(c.span_tails, 0) == list(range(64))
    assert tail_lanes(c.span_tails, 1) == [15, 31, 47, 63]
    assert tail_lanes(c.span_tails, 2) == TAIL_LANES
    first = int(np.searchsorted(L.scope, m["LONG"]))
    assert first == 3 * WAVE + 10 and L.scope_spans[m["LONG"]] == 700
    assert c.max_scope_atomics == 12                                       # one per wave the scope reaches
    assert (first + 699) // TILE - first // TILE == 3                      # over four 256-span blocks
    d = int(np.searchsorted(L.scope, m["DROPPED"]))
    assert d % WAVE == 0 and not L.keep[d:d + WAVE].any() and c.dropped_waves == 1
    h = int(np.searchsorted(L.scope, m["HT"]))
    assert L.keep[h:h + 10].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    assert c.partial_wave == 27


def census_span_stride(L, c):
    n, edge = L.n, L.marks["edge"]
    assert c.span_blocks == K.span_cap
    assert c.span_x1 == (n > edge) and c.span_second_iter == (n > 2 * edge)
    if n > edge:
        assert L.scope[edge - 1] == L.scope[edge]                          # one scope over the x0 / x1 tile edge
    assert L.keep.min() == 0 and {0, 1, 2, 3} <= set(L.url_out[:64].tolist())


def census_varints(L, c):
    two = lambda k: {(1 << k) - 1, 1 << k}
    assert set(sl.VARINT_SPAN) <= set(L.span_size.tolist()) and (1 << 32) - 1 in sl.VARINT_SPAN
    kept = L.keep != 0
    framed = np.where(kept, sl.field_len(sl.span_sizes_after(L, True)), 0)
    body = sl._seg_sum(L.scope, framed, L.S)
    total = set((L.scope_size.astype(np.int64) + body).tolist())
    for k in sl.VARINT_SCOPE:
        assert two(k) <= total, k
    assert int(body.max()) < (1 << K.kSumBits) and int(body.max()) >= (1 << 35) - 8
    # the added KeyValue, its AnyValue and string, and the new name on both sides of 2^7 and 2^14
    tl = L.tmpl_len.astype(np.int64)
    for key, kind in ((12, L.kind == sl.CLIENT), (10, L.kind != sl.CLIENT)):
        kv = set((sl.field_len(key) + sl.field_len(sl.field_len(tl[kind & (L.url_out & 1 != 0)]))).tolist())
        for k in (7, 14):
            assert two(k) <= kv, (key, k)
    for old in (0, 3):
        names = set((old + 1 + tl[(L.name_len == old) & (L.url_out & 2 != 0)]).tolist())
        for k in (7, 14):
            assert two(k) <= names, (old, k)
    assert 0 in set(tl.tolist()) and {1, 2, 3} <= set(L.url_out.tolist())
    assert {sl.CLIENT, sl.SERVER, sl.INTERNAL} <= set(L.kind.tolist())


CENSUS = {"run.ends": census_run_ends, "run.cross": census_run_cross, "run.long": census_run_long,
          "run.tiles": census_run_tiles, "removed": census_removed, "scope.runs": census_scope_runs,
          "varints": census_varints, "tail.stride": census_tail_stride, "span.stride": census_span_stride,
          **{f"gaps.{g}": census_gaps(g) for g in (1, 2, 300)},
          **{f"gaps.S0.{R}": census_s0(R) for R in (1, 255, 257, K.s0_cap * TILE + 1)},
          **{f"ends.{S}": census_ends(S) for S in sl.ENDS},
          **{f"attrsets.{A}": census_attrsets(A) for A in (K.kLdsAttrsets, K.kLdsAttrsets + 1)}}


@pytest.mark.parametrize("name", SMALL)
def test_census(name):
    L = layout(name)
    CENSUS[name](L, census(L))


def test_census_reaches_every_path():
    """Every dispatch path of the stage is taken by some small layout (the two
    grid-stride ones by the large layouts, test_oracle_is_the_restatement_large)."""
    tot = {}
    for name in SMALL:
        for k, v in vars(census(layout(name))).items():
            if isinstance(v, (int, bool, np.integer)):
                tot[k] = tot.get(k, 0) + int(v)
    for k in ("fix", "in_window", "cut_head", "cut_tail", "cut_both", "gap_first", "gap_inner", "gap_lane0", "gap_after",
              "gap_s0", "s0_second_iter", "empty_windows", "dropped_waves", "partial_wave"):
        assert tot[k] > 0, k
    assert sl.TAIL_STRIDE + TILE + 1 > K.tail_tiles * K.tail_cap * TILE    # tail.stride: the second iteration
    assert sl.SPAN_STRIDE_NS[1] > K.span_cap * TILE and sl.SPAN_STRIDE_NS[3] > 2 * K.span_cap * TILE


# ---------------------------------------------------------------------------
# GPU: every layout against the oracle, in every call form

PRE_ACC = 77
_engines = {}


def _engine(cfg):
    from odigos_amd.batch import Engine
    key = json.dumps(cfg, sort_keys=True)
    if key not in _engines:
        _engines[key] = Engine(cfg)
    return _engines[key]


def _pre_attr(A):
    return 1000 + 3 * np.arange(A, dtype=np.int64)


def gpu_vs_oracle(L, stages, *, cfg=None, inverse=1, ratio=1.0, u=0.0, mode=native.GROUP_TRACE_ID, calls=1,
                  sampling=None, seed=0, tmpl_cap=None):
    """The device call on sentinel-filled outputs against the oracle's sums."""
    import torch
    from odigos_amd.batch import DeviceBatch
    cfg = cfg or {"odigostrafficmetrics": TRAFFIC}
    eng = _engine(cfg)
    db = DeviceBatch(L.cols, tmpl_cap=tmpl_cap)

    def put(name, a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
        db.o[name][:t.numel()].copy_(t)

    put("keep", L.keep)
    if stages & native.STAGE_APPLY_TEMPLATE:
        put("url_out", L.url_out)
        put("tmpl", L.tmpl)
    db.o["res_bytes"].fill_(0xEE)
    put("attrset_bytes", _pre_attr(L.A))
    put("accepted_spans", np.array([PRE_ACC], dtype=np.int64))
    for _ in range(calls):
        eng.process_device(db, stages, mode, seed=seed, traffic_u=u)
    torch.cuda.synchronize()
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    res, attr, acc = oracle(L, stages, inverse, ratio, u, mode, sampling, seed)
    got_res = db.out_numpy("res_bytes", np.uint64)
    np.testing.assert_array_equal(got_res[:L.R], res, err_msg=f"{L.name} res_bytes")
    assert (db.out_numpy("res_bytes")[8 * L.R:] == 0xEE).all(), "res_bytes written past n_resources"
    np.testing.assert_array_equal(db.out_numpy("attrset_bytes", np.int64)[:L.A], _pre_attr(L.A) + calls * attr,
                                  err_msg=f"{L.name} attrset_bytes")
    assert int(db.out_numpy("accepted_spans", np.int64)[0]) == PRE_ACC + calls * acc, L.name
    return db, (res, attr, acc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_gpu_layout(name):
    L = layout(name)
    gpu_vs_oracle(L, SIZE)
    gpu_vs_oracle(L, APPLIED)


@pytest.mark.gpu
def test_gpu_removed_forms_differ():
    # the same columns: emptied containers removed under APPLY_KEEP, kept under SIZE alone
    L = layout("removed")
    _, (gone, _, _) = gpu_vs_oracle(L, APPLIED)
    _, (kept, _, _) = gpu_vs_oracle(L, SIZE)
    assert gone[L.marks["EMPTY"]] == 0 < kept[L.marks["EMPTY"]] and gone[L.marks["STAYS"]] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("A", [K.kLdsAttrsets, K.kLdsAttrsets + 1])
def test_gpu_attrsets_inverse(A):
    cfg = {"odigostrafficmetrics": dict(TRAFFIC, sampling_ratio=0.25)}
    L = layout(f"attrsets.{A}")
    gpu_vs_oracle(L, APPLIED, cfg=cfg, inverse=4, ratio=0.25, u=0.1)
    _, (_, attr, _) = gpu_vs_oracle(L, SIZE, cfg=cfg, inverse=4, ratio=0.25, u=0.1)
    assert attr[0] > 0 and attr[K.kLdsAttrsets - 1] > 0 and attr[A - 1] > 0 and attr[7] % 4 == 0
    # rand.Float64() >= ratio: the call measures nothing and writes nothing
    import torch
    from odigos_amd.batch import DeviceBatch
    db = DeviceBatch(L.cols)
    db.o["res_bytes"].fill_(0xEE)
    _engine(cfg).process_device(db, SIZE, traffic_u=0.5)
    torch.cuda.synchronize()
    assert (db.out_numpy("res_bytes") == 0xEE).all() and not db.out_numpy("attrset_bytes").any()


@pytest.mark.gpu
def test_gpu_tail_stride():
    L = layout("tail.stride")
    try:
        gpu_vs_oracle(L, APPLIED)
        gpu_vs_oracle(L, SIZE)
    finally:
        sl.drop("tail.stride")


@pytest.mark.gpu
def test_gpu_span_stride():
    for n in sl.SPAN_STRIDE_NS:
        name = f"span.stride.{n}"
        try:
            L = layout(name)
            gpu_vs_oracle(L, APPLIED)
            if n == sl.SPAN_STRIDE_NS[-1]:
                gpu_vs_oracle(L, SIZE)
        finally:
            sl.drop(name)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["packed", "refs"])
@pytest.mark.parametrize("name", sl.FUSED)
def test_gpu_fused(name, form):
    """APPLY_KEEP | TEMPLATE | SIZE on real paths: the spans pass runs inside
    url_copy_kernel on the plan lengths, the surviving spans are counted per
    block (kept_partials) and summed by size_tail_kernel."""
    L = layout(name + ".paths")
    cfg = {"odigosurltemplate": {}, "odigostrafficmetrics": TRAFFIC}
    db, _ = gpu_vs_oracle(L, REFS if form == "refs" else FUSED, cfg=cfg, tmpl_cap=1 << 22)
    np.testing.assert_array_equal(db.out_numpy("url_out")[:L.n], L.url_out)
    lens = db.out_numpy("tmpl", np.uint32)[:2 * L.n].reshape(-1, 2)[:, 1]
    m = L.url_out != 0
    np.testing.assert_array_equal(lens[m], L.tmpl_len[m])


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.0, 100.0])
def test_gpu_batch_dropped(ratio):
    """SAMPLE | SIZE in OSE_GROUP_BATCH under a one-rule config whose decision
    does not depend on the uniform: dropped, every res_bytes entry is 0 (the
    sentinel overwritten) and the counters are unchanged; kept, nothing is
    removed."""
    L = layout("run.cross").with_sampling()
    sampling = sl.batch_config(ratio)
    cfg = {"odigossampling": sampling, "odigostrafficmetrics": TRAFFIC}
    stages = native.STAGE_SAMPLE | native.STAGE_SIZE
    for seed in (1, 2):
        _, (res, attr, acc) = gpu_vs_oracle(L, stages, cfg=cfg, mode=native.GROUP_BATCH, sampling=sampling, seed=seed)
        if ratio == 0.0:
            assert not res.any() and not attr.any() and acc == 0
        else:
            np.testing.assert_array_equal(res, sl.restate(L, False, False, False)[0])
            assert acc == L.n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["run.long", "scope.runs"])
def test_gpu_twice_doubles(name):
    # the reference test's property (processor_test.go): a second call doubles the counters
    gpu_vs_oracle(layout(name), APPLIED, calls=2)
