"""The trace stage on hand-laid batches: one named layout per seam of
trace_eval_kernel, the long-run kernels and the run-list path, each compared
with the oracle bit for bit (tests/trace_layouts.py builds them).

The generator workloads reach these seams by chance, if at all; here every
layout's census (computed from the built columns alone) first proves that the
batch holds its seam, the C oracle is pinned against the pure-Python
restatement on it, and then the HIP stage must give the oracle's keep, trace
order, level, ratio and decision.

Layout                         guards (constant / code line)
-----------------------------  ------------------------------------------------
step, step.ragged1/63          the 64-span step of trace_eval_kernel: a trace
                               ending at lane 63 / opening at lane 0, at lane
                               63, at lane 0 of a range's first and last window
                               (`w0`, `range_end`), traces of exactly 1, 2 and 5
                               steps (`cont_next`, `single`), a range whose
                               first windows hold no head (`!started`), n % 64
                               in {1, 63} (`valid`, `vmask`)
queue                          kQ (64): 1, 2, 31, 32, 33, 63, 64 closes in a
                               step; at W >= 2 the queue fills exactly and
                               overflows by one, without (`qn + nq > kQ`) and
                               with a carried trace closing (`qn == kQ`)
head                           kHeadQ (128): 64 + 64 heads fill it exactly; at
                               W >= 3 a third step overflows it by one
                               (`hn + nh > kHeadQ`), with and without a carried
                               trace closing there
stretch                        the latency stretches and `rep_slots`: A B A,
                               A B A B, A N A inside one step, in the carried
                               trace (`seg0_cont`) and in the trace left open
                               (`last_open`); zero starts (latency.go:69-73)
handoff.{first,last}.E         kLongSteps (4): `base >= range_end +
                               long_steps * 64`; a run from the first / last
                               lane of a range ending (exclusive) at range_end
                               + 255, 256 (not handed off), 257, 320 (handed);
                               one run decides on its last span, one on its
                               first (as L and M of the long.N layouts do)
long.2048 ... long.6145        kLongPiece (2048): runs of 1, 2, 2, 3 and 4
                               pieces (`np = ceil((end - pos) / kLongPiece)`)
long.last                      trace_long_plan_kernel's `end = a.n_spans` when
                               no head follows; the batch ends mid-window
long.17, long.33               kPlanWaves (16): a second and third plan /
                               decide workgroup
long.marks                     the piece partials (LongPart) combined in piece
                               order: zero starts and ERROR in the first / last
                               span of a piece and in the middle piece only
repeat.runs8 / runs9           kMaxRuns (8)
repeat.spans4096 / spans4097   kMaxFoldSpans (4096)
repeat.slots8 / slots9         kMaxFoldSlots (8) (latency services of the C3
                               rules; the chunked configs have more)
repeat.spread                  trace_fold_kernel's sort of the listed runs
repeat.first_long              the run-list path overwriting a long-run decision
dup.overflow                   kDupBucketCap (1024) and reserve_table's sizing:
                               5000 distinct single-span traces overflow the
                               buckets, *dup is set with nothing repeated
placed W = 2 / W = 16          win_per_wave = min(kWinPerWave, max(1, n_windows
                               / 4096)): the step, queue, head, stretch and
                               hand-off blocks in the first, a middle and the
                               last ranges of a batch of 524,225 spans (W = 2;
                               cut to 524,224: W = 1) and of 4,194,304 (W = 16)

kWinPerWaveBeside (64 windows per wave, taken only beside the forked URL
planning of a SAMPLE | TEMPLATE call of 2^20 spans or more, 64 of them from
16.7M spans up) is out of scope here.

The hand-off's witness: run_stages gates SAMPLE's tail on the host for every
call grouped by trace id (engine.cpp `gate_on_host`; a later stage only defers
it), so run_sampling_pass queues the long-run kernels only when the fast pass
listed a run, and `Engine.path_counts()["long_runs"]` is 1 or 0 accordingly
for the SAMPLE-only calls made here.  The witnesses are asserted for the
one-chunk configs; a chunked config counts a pass per chunk.
"""
import ctypes as C

import numpy as np
import pytest

from odigos_amd import native
from tests import trace_layouts as tl
from tests.oracle_lib import intern_services, lib as orc_lib
from tests.test_sampling_chunks import _attr_bits, _chunks
from tests.test_sampling_random import SEED, _arr, _group, _py_eval, fractional_config, gpu_vs_oracle, oracle_run
from tests.trace_layouts import A, B, K, N, WAVE
from tests.workloads import (c3_sampling_config, check_interning, wide_attr_config, wide_latency2_config,
                             wide_latency_config)

NAMES = list(tl.LAYOUTS)
N_W2 = tl.n_for(2)
N_W16 = 4_194_304
PLACED = ["step", "queue", "head", "stretch", "handoff"]
C3_LAT = sorted(tl.lat_services(c3_sampling_config()))


# ---------------------------------------------------------------------------
# constants and the W formula

def test_constants_as_designed():
    # the layouts were drawn for these values: retuning one moves a seam, and
    # the layouts (and the table in this module's docstring) move with it
    got = {k: getattr(K, k) for k in tl.DESIGNED}
    assert got == tl.DESIGNED, "a trace-stage constant changed: re-lay tests/trace_layouts.py against it"
    assert len(C3_LAT) == 11 and set(tl.LAT8 + [12]) <= set(C3_LAT)
    assert N not in C3_LAT and A in C3_LAT and B in C3_LAT


def test_win_per_wave_formula():
    assert tl.win_per_wave(8191 * WAVE) == 1
    assert tl.win_per_wave(8191 * WAVE + 1) == 2 and N_W2 == 8191 * WAVE + 1 == 524_225     # 8192 windows
    assert tl.win_per_wave(N_W2 - 1) == 1
    assert tl.win_per_wave(65535 * WAVE) == 15
    assert tl.win_per_wave(65535 * WAVE + 1) == 16 == tl.win_per_wave(N_W16)                 # 65536 windows
    assert tl.win_per_wave(1 << 30) == K.kWinPerWave
    for W in (2, 3, 16):
        assert tl.win_per_wave(tl.n_for(W)) == W and tl.win_per_wave(tl.n_for(W) - 1) == W - 1


# ---------------------------------------------------------------------------
# census: each layout holds its seam (from the built columns alone)

def _svc_rle(b, a, e):
    return tl._rle(b.svc[a:e])


def _one_run(b, label):
    r = b.runs_of(label)
    assert len(r) == 1, (label, r)
    return r[0]


def census_step(b, W, w_lo, sfx=""):
    R = WAVE * W
    base = w_lo * WAVE
    assert base % R == 0
    at = lambda label: tuple(x - base for x in _one_run(b, label + sfx))
    assert at("T1") == (0, 64) and at("T2") == (64, 192) and at("T5") == (192, 512)   # 1, 2 and 5 whole steps
    t63 = at("T63")
    assert t63[0] % WAVE == 63 and t63[1] - t63[0] == 10
    tL = at("TL")
    assert tL[0] % R == R - 64                     # lane 0 of a range's last window
    assert tL[1] == tL[0] + 64 + 64 * (W - 1) + 10  # ... through the next range's first W - 1 windows
    # heads: every whole-step trace is followed by a head at lane 0
    h = b.heads()
    for label in ("T1", "T2", "T5"):
        e = _one_run(b, label + sfx)[1]
        assert e % WAVE == 0 and h[e]
    _, _, headless = b.walk(W, w_lo, w_lo + 512 // WAVE)
    if W <= 2:
        assert headless, "T5 covers whole ranges"
    else:
        nxt = (base + tL[0]) // R * R + R
        assert not h[nxt:nxt + 64 * (W - 1) + 10].any() and h[nxt + 64 * (W - 1) + 10]


def census_queue(b, W, w_lo, sfx=""):
    k = len(tl.QUEUE_STEPS)
    assert b.closes_per_step(w_lo, w_lo + k).tolist() == tl.QUEUE_STEPS
    assert set(tl.QUEUE_STEPS) == {1, 2, 31, 32, 33, 63, 64}
    qc = _one_run(b, "QC" + sfx)
    assert qc[0] // WAVE == w_lo + k - 1 and (qc[1] - 1) // WAVE == w_lo + k     # carried into the next step
    ev, _, _ = b.walk(W, w_lo, w_lo + k + 1)
    assert ("q_exact",) in ev
    if W >= 2:
        assert ("q_over", 1, False) in ev and ("q_over", 1, True) in ev, ev


def census_head(b, W, w_lo, sfx=""):
    assert b.heads_per_step(w_lo, w_lo + 3).tolist() == [64, 64, 1]
    ev, _, _ = b.walk(W, w_lo, w_lo + max(W, 3) * 2)
    if W >= 2:
        assert ("h_exact",) in ev
    if W >= 3:
        assert ("h_over", 1, False) in ev and ("h_over", 1, True) in ev, ev
    hc = _one_run(b, "HC" + sfx)
    assert hc[0] % WAVE == 63 and hc[1] % WAVE == 10


def census_stretch(b, W, w_lo, sfx=""):
    base = w_lo * WAVE
    pats = {"aba": [A, B, A], "abab": [A, B, A, B], "ana": [A, N, A]}
    for name, want in pats.items():
        a, e = _one_run(b, f"S.{name}{sfx}")
        assert a // WAVE == (e - 1) // WAVE and _svc_rle(b, a, e) == want            # inside one step
        a, e = _one_run(b, f"C.{name}{sfx}")
        cut = (a // WAVE + 1) * WAVE
        assert a < cut < e and _svc_rle(b, cut, e) == want and _svc_rle(b, a, cut) == [N]   # the carried part
        a, e = _one_run(b, f"O.{name}{sfx}")
        cut = (a // WAVE + 1) * WAVE
        assert a < cut < e and _svc_rle(b, a, cut) == want and _svc_rle(b, cut, e) == [B]   # the opening step
    a, e = _one_run(b, "C.a|ba" + sfx)
    cut = (a // WAVE + 1) * WAVE
    assert _svc_rle(b, a, cut) == [A] and _svc_rle(b, cut, e) == [B, A]
    # zero starts: first stretch, second A stretch, first span of the carried part, first span of the trace
    for label, z in (("S.aba.z1", 1), ("S.aba.z1k", 1), ("S.aba.z2", 5), ("C.z.first", 0)):
        a, e = _one_run(b, label + sfx)
        assert np.nonzero(b.start[a:e] == 0)[0].tolist() == [z]
    a, e = _one_run(b, "C.z.part" + sfx)
    assert (a + int(np.nonzero(b.start[a:e] == 0)[0][0])) % WAVE == 0
    a, e = _one_run(b, "O.aba.z" + sfx)
    z = a + int(np.nonzero(b.start[a:e] == 0)[0][0])
    assert _svc_rle(b, a, z) == [A, N] and b.svc[z] == A and z // WAVE == a // WAVE
    assert base <= a


def census_handoff(b, W, w_lo, sfx=""):
    R = WAVE * W
    want = []
    for f in (1, 0):
        for e_off in tl.HANDOFF_ENDS:
            for mark in ("", "'"):
                a, e = _one_run(b, f"HO.{f}.{e_off}{mark}{sfx}")
                assert a % R == (0 if f else R - 1)
                rend = a // R * R + R
                assert e - rend == e_off
                if e_off > K.kLongSteps * WAVE:
                    want.append(a)
    assert sorted(tl.HANDOFF_ENDS) == [255, 256, 257, 320]
    _, handed, _ = b.walk(W, w_lo, _one_run(b, f"HO.0.{tl.HANDOFF_ENDS[-1]}'{sfx}")[1] // WAVE)
    assert sorted(handed) == sorted(want) and len(want) == 8


BLOCK_CENSUS = {"step": census_step, "queue": census_queue, "head": census_head, "stretch": census_stretch,
                "handoff": census_handoff}


def census(name, b):
    hp, ends, tr = b.runs()
    lens = ends - hp
    rep = b.repeated(C3_LAT)
    _, handed, _ = b.walk(1)
    assert (len(handed) > 0) == bool(b.expect["long_runs"]), name
    assert (len(rep) > 0) == (b.expect["run_list"] == 1 and name != "dup.overflow"), name
    over = any(r > K.kMaxRuns or s > K.kMaxFoldSpans or l > K.kMaxFoldSlots for r, s, l in rep)
    assert over == bool(b.expect["sort"]), (name, rep)
    assert (np.diff(b.resource.astype(np.int64)) >= 0).all() and b.resource[0] == 0
    assert len(np.unique(b.tid, axis=0)) == b.n_labels == len(np.unique(tr))       # distinct labels, distinct ids
    assert (b.res_svc[b.resource] == b.svc).all()
    fam = name.split(".")[0]
    if name.startswith("step") or name in ("queue", "head", "stretch"):
        BLOCK_CENSUS[fam](b, 1, b.block[0])
        if name.startswith("step.ragged"):
            assert b.n % WAVE == int(name[len("step.ragged"):])
    elif fam == "handoff":
        first, e_off = name.split(".")[1] == "first", int(name.split(".")[2])
        heads = []
        for label in ("HO", "HO'"):
            a, e = _one_run(b, label)
            assert a % WAVE == (0 if first else 63) and e - (a // WAVE + 1) * WAVE == e_off
            heads.append(a)
        assert handed == (heads if e_off > K.kLongSteps * WAVE else [])
    elif name in ("long.17", "long.33"):
        count = int(name[5:])
        assert len(handed) == count and count % K.kPlanWaves == 1 and count > K.kPlanWaves
        assert all(b.runs_of(f"L{k}")[0][0] in handed for k in range(count))
    elif name == "long.marks":
        P = K.kLongPiece
        assert len(handed) == 8
        marks = {"Zc": (None, None), "Zf": (P, None), "Zl": (P - 1, None), "Zo": (P - 1, None), "Zm": (P + 900, None),
                 "Ef": (None, P), "El": (None, P - 1), "Em": (None, P + 900)}
        for label, (z, er) in marks.items():
            a, e = _one_run(b, label)
            assert e - a == 2 * P + 1 and a in handed                      # three pieces
            assert np.nonzero(b.start[a:e] == 0)[0].tolist() == ([] if z is None else [z])
            assert np.nonzero(b.status[a:e] == native.STATUS_ERROR)[0].tolist() == ([] if er is None else [er])
    elif fam == "long":
        a, e = _one_run(b, "L")
        assert a % WAVE == 0 and b.start[e - 1] == 0
        if name == "long.last":
            assert handed == [a] and e == b.n and b.n % WAVE not in (0, 63) and e - a == K.kLongPiece + 1
        else:
            m = _one_run(b, "M")
            assert handed == [a, m[0]] and m[0] % WAVE == 0 and m[1] - m[0] == e - a
            assert e - a == int(name[5:]) and h_after(b, e) and h_after(b, m[1])
        pieces = -(-(e - a) // K.kLongPiece)
        assert pieces == {2048: 1, 2049: 2, 4096: 2, 4097: 3, 6145: 4}[e - a]
    elif name == "dup.overflow":
        assert (lens == 1).all() and len(hp) == b.n == 5000 and not rep
        assert tl.dup_bucket_slots(b.n) < b.n          # some bucket overflows whatever the fingerprints
    elif fam == "repeat":
        assert len(rep) == 1
        r, s, l = rep[0]
        want = {"runs8": (8, None, None), "runs9": (9, None, None), "spans4096": (2, 4096, None),
                "spans4097": (2, 4097, None), "slots8": (2, None, 8), "slots9": (2, None, 9),
                "spread": (6, None, None), "first_long": (2, None, None)}[name.split(".")[1]]
        assert r == want[0] and (want[1] is None or s == want[1]) and (want[2] is None or l == want[2]), rep
        x = b.runs_of("X")
        if name == "repeat.first_long":
            assert handed == [x[0][0]]
        if name == "repeat.spread":
            wins = [a // WAVE for a, _ in x]
            assert wins[-1] == (b.n - 1) // WAVE and min(np.diff(wins)) > 16
    else:
        raise AssertionError(f"layout {name} has no census")


def h_after(b, e):
    return e < b.n and bool(b.heads()[e])


@pytest.mark.parametrize("name", NAMES)
def test_census(name):
    census(name, tl.layout(name))


def _placed(W, n):
    L = sum(tl.BLOCKS[name](W)[1] for name in PLACED)
    R = WAVE * W
    # the last run of the batch: from the first lane of a range to the batch's end, handed off
    pt = (n - (R + (K.kLongSteps + 1) * WAVE)) // R * R
    where = [0, (n // 2) // R * R, pt - L]
    # (its decision hangs on the batch's last span: a zero start there)
    tail = tl.Seg("END", pt, n - pt, [(A, n - pt - 5), (B, 5)], early=0, zero=(n - pt - 1,))
    b, spans = tl.place(PLACED, W, n, seed=0x1AE0 + W, where=where, extra=[tail])
    return b, spans, pt


_placed_cache = {}


def placed(W):
    if W != 2:      # (the 4M-span batch is built where it is used and dropped after)
        return _placed(W, N_W16)
    if W not in _placed_cache:
        _placed_cache[W] = _placed(W, N_W2)
    return _placed_cache[W]


@pytest.mark.parametrize("W", [2, 16])
def test_census_placed(W):
    b, spans, pt = placed(W)
    assert tl.win_per_wave(b.n) == W
    assert spans[("step", 0)][0] == 0                                  # the batch's first range
    for (name, pk), (w_lo, w_hi) in spans.items():
        assert w_lo % W == 0
        BLOCK_CENSUS[name](b, W, w_lo, f"@{pk}")
    a, e = _one_run(b, "END")
    assert a == pt and e == b.n and a % (WAVE * W) == 0
    _, handed, _ = b.walk(W, a // WAVE)
    assert handed == [a]                                               # the last run, no head after it
    assert spans[("handoff", 2)][1] * WAVE == pt                       # the blocks end where the last range's run starts
    if W == 2:
        assert b.n % WAVE == 1
        c = b.cut(b.n - 1)
        assert tl.win_per_wave(c.n) == 1 and c.n == 524_224
        assert (np.diff(c.resource.astype(np.int64)) >= 0).all() and len(c.res_svc) == int(c.resource[-1]) + 1


# ---------------------------------------------------------------------------
# the reference itself on these shapes

@pytest.mark.parametrize("name", NAMES)
def test_oracle_vs_python(name):
    cfg = fractional_config()
    b = tl.layout(name)
    cols = b.cols
    ho = oracle_run(cols, native.GROUP_TRACE_ID, cfg=cfg)
    traces = _group(cols, False)
    assert int(ho.view("trace_count", np.uint32)[0]) == len(traces)
    svc_ids = intern_services(cfg)
    res = _arr(cols.resource, C.c_uint32, cols.n_spans)
    keep = ho.view("keep", np.uint8)
    first = ho.view("trace_first_span", np.uint32)
    levels = set()
    for t, spans in enumerate(traces):
        hi, lo = int(b.tid[spans[0], 0]), int(b.tid[spans[0], 1])
        u = orc_lib().orc_trace_uniform(hi, lo, SEED)
        k, lvl, ratio = _py_eval(cfg, svc_ids, cols, res, spans, False, u)
        assert first[t] == spans[0], t                                  # trace order
        assert ho.view("trace_level", np.uint8)[t] == lvl, t
        assert ho.view("trace_ratio", np.float64)[t] == ratio, t
        assert ho.view("trace_keep", np.uint8)[t] == int(k), t
        assert (keep[spans] == int(k)).all(), t
        levels.add(lvl)
    assert len(levels) >= 2, levels


def test_marked_traces_decide_as_laid():
    # the early / late starts make the endpoint level's outcome follow from
    # where minStart is reset: level 2 = a latency rule satisfied
    ho = {}
    lv = {}
    for name in ("long.marks", "stretch", "long.2049", "handoff.first.257"):
        b = tl.layout(name)
        ho[name] = oracle_run(b.cols, native.GROUP_TRACE_ID, cfg=c3_sampling_config())
        t = int(ho[name].view("trace_count", np.uint32)[0])
        first = ho[name].view("trace_first_span", np.uint32)[:t]
        level = ho[name].view("trace_level", np.uint8)[:t]
        for s in b.segs:
            lv[s.label] = int(level[np.searchsorted(first, s.at)])
    sat = {"Zc": 2, "Zf": 3, "Zl": 3, "Zo": 2, "Zm": 3, "Ef": 0, "El": 0, "Em": 0,
           "S.aba": 2, "S.abab": 2, "S.ana": 2, "S.aba.z1": 3, "S.aba.z1k": 2, "S.aba.z2": 3,
           "C.aba": 2, "C.abab": 2, "C.ana": 2, "C.a|ba": 2, "C.z.part": 3, "C.z.first": 2,
           "O.aba": 2, "O.abab": 2, "O.ana": 2, "O.aba.z": 3, "L": 2, "M": 2, "HO": 2, "HO'": 2}
    assert {k: lv[k] for k in sat} == sat


# ---------------------------------------------------------------------------
# GPU

def many_service_rules_config():
    # (the config of test_gpu_sampling_many_service_rules: lean, not narrow)
    cfg = c3_sampling_config()
    cfg["service_rules"] = [
        {"name": f"r{k}", "type": "service_name",
         "rule_details": {"service_name": f"svc-{k % 20:02d}", "sampling_ratio": float((k * 37) % 101),
                          "fallback_sampling_ratio": float(k % 7)}}
        for k in range(130)]
    return cfg


CONFIGS = {"c3": c3_sampling_config, "fractional": fractional_config, "many_rules": many_service_rules_config,
           "multi3": wide_latency_config, "multi2": wide_latency2_config, "chunks2": wide_attr_config}
ONE_CHUNK = ("c3", "fractional", "many_rules")


def test_layout_configs():
    for name, f in CONFIGS.items():
        check_interning(f())
        assert _chunks(f()) == {"multi3": 3, "multi2": 2, "chunks2": 2}.get(name, 1)
    assert sorted(tl.lat_services(many_service_rules_config())) == C3_LAT == sorted(tl.lat_services(fractional_config()))


def run_gpu(b, cname):
    cfg = CONFIGS[cname]()
    ran, paths = set(), {}
    keep_alive = None
    if cname == "chunks2":
        keep_alive = _attr_bits(b, 40, seed=17)
    try:
        gpu_vs_oracle(b, cfg=cfg, kernels=ran, paths=paths)
    finally:
        if keep_alive is not None:
            b.cols.attr_match = None
            b.cols.attr_match_words = 0
    return ran, paths


def check_witnesses(b, cname, ran, paths):
    dup = b.expect["run_list"]
    if cname in ONE_CHUNK:
        assert paths == b.expect, (paths, b.expect)
        assert "trace_eval_kernel" in ran and "trace_multi_kernel" not in ran
        assert ("trace_long_kernel" in ran) == bool(b.expect["long_runs"]), ran
    elif cname in ("multi2", "multi3"):
        # one pass over every chunk; a batch whose *dup is set is redone pass per chunk
        assert "trace_multi_kernel" in ran, ran
        assert ("trace_eval_kernel" in ran) == bool(dup), ran
    else:
        assert "trace_multi_kernel" not in ran and "trace_eval_kernel" in ran, ran
    assert ("trace_run_list" in ran) == bool(dup), ran


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_layouts_w1(cname, name):
    b = tl.layout(name)
    ran, paths = run_gpu(b, cname)
    check_witnesses(b, cname, ran, paths)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_layouts_w2(cname, cut):
    # the blocks in the first, a middle and the last ranges at two windows per
    # wave (524,225 spans), and the same columns cut to 524,224 (one window)
    b, _, _ = placed(2)
    if cut:
        b = b.cut(b.n - 1)
    ran, paths = run_gpu(b, cname)
    b.expect = dict(run_list=0, sort=0, long_runs=1)
    check_witnesses(b, cname, ran, paths)


@pytest.mark.gpu
def test_gpu_layouts_w16():
    # the same blocks at kWinPerWave windows per wave: 4,194,304 spans, C3 only
    b, _, _ = placed(16)
    ran, paths = run_gpu(b, "c3")
    b.expect = dict(run_list=0, sort=0, long_runs=1)
    check_witnesses(b, "c3", ran, paths)
