"""The trace stage where clamped and early loads can go wrong.

trace_eval_kernel and trace_multi_kernel load a step's columns one step ahead
with the span index clamped to n - 1 and the neighbour trace id through a
per-lane address; the lean instances load the resource index two steps ahead
and the service ids one.  Such loads can go wrong in three
places: at the batch's end, at a wave's first owned step after skipped ones,
and where a lane reads its neighbour's trace id.  Each layout here holds one
of those seams; a census proves it from the columns, the C oracle is pinned
against the Python restatement on the small ones, and `keep` on the GPU must
be the oracle's bit for bit.

Layout            guards
----------------  -------------------------------------------------------------
end.N             the batch's end: n in 1 .. 193 and 524,288 + {0, 1, 63, 65}
                  (two windows per wave: the last wave's last step is ragged).
                  Every column is a slice of a buffer 256 spans longer, and the
                  tail past n is poisoned with in-range values that flip the
                  last trace's decision if they reach it: its id continued,
                  ERROR statuses, zero starts, a latency-rule service's
                  resources, routes with a rule's prefix.
skip.K.R          one run of 64 K + R spans at the start of a batch of two
                  windows per wave; the next trace's head is lane R of window
                  K: for K = 3, 5 the wave that owns it has skipped a window
                  and leaves skip mode on exactly that step.
ids.singles,      one-span traces; traces of exactly 64 spans on the window
ids.aligned,      grid, and shifted by one span: every head at lane 0, every
ids.shifted       tail at lane 63, and `cont_next` both ways.
chain             the dependent chain: the resource changes on every span, every
                  service has a latency rule, routes of 0, 1, 15, 16 and 17
                  bytes at arena offsets 0 and 15 mod 16 (the head16 cases),
                  the last one ending on the arena's last byte.

The instances: `narrow` and `wide` are the lean ones (C3; 130 service rules),
`chunked` the lean pass per rule chunk (four chunks), `multi2`
trace_multi_kernel<2>, `general` the general instance (span_attribute bits).

The machine-code test compiles trace_kernel.hip to assembly and asserts that
no `s_waitcnt vmcnt(0)` lies between the prefetch and the loop's back edge of
the two lean instances outside the flush blocks (tools/vmcnt_report.py).
"""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import native
from tests import trace_layouts as tl
from tests.oracle_lib import intern_services, lib as orc_lib
from tests.test_sampling_random import SEED, _arr, _group, _py_eval, fractional_config, oracle_run
from tests.trace_layouts import A, B, N, WAVE, Seg
from tests.workloads import c3_sampling_config, wide_attr_config, wide_latency2_config, wide_mixed_config

ROOT = Path(__file__).resolve().parent.parent
TAIL = 256
N_W2 = 524_288
END_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 193] + [N_W2 + d for d in (0, 1, 63, 65)]
SKIPS = [(k, r) for k in (1, 3, 5) for r in (0, 1, 63)]


def many_service_rules_config():
    # lean, not narrow: more service-rule bits than one 32-bit word holds
    cfg = c3_sampling_config()
    cfg["service_rules"] = [
        {"name": f"r{k}", "type": "service_name",
         "rule_details": {"service_name": f"svc-{k % 20:02d}", "sampling_ratio": float((k * 37) % 101),
                          "fallback_sampling_ratio": float(k % 7)}}
        for k in range(130)]
    return cfg


CONFIGS = {"narrow": c3_sampling_config, "wide": many_service_rules_config, "chunked": wide_mixed_config,
           "multi2": wide_latency2_config, "general": wide_attr_config}
KERNEL = {"narrow": "trace_eval_kernel", "wide": "trace_eval_kernel", "chunked": "trace_eval_kernel",
          "multi2": "trace_multi_kernel", "general": "trace_eval_kernel"}


# ---------------------------------------------------------------------------
# layouts

class Sliced:
    """The first n spans of a batch laid out TAIL spans longer: `cols` sees n
    spans, every column pointer is the longer buffer's."""

    def __init__(self, full, n):
        self.full, self.n = full, n
        c = native.Columns()
        C.memmove(C.byref(c), C.byref(full.cols), C.sizeof(native.Columns))
        c.n_spans = n
        self.cols = c
        self.attr = None

    def with_attr(self, on):
        """attr_match for the span_attribute config: one 64-bit word per span
        (40 rules), the tail's all ones."""
        if on and self.attr is None:
            rng = np.random.default_rng(17)
            self.attr = np.zeros(self.full.n, dtype=np.uint64)
            for k in range(40):
                self.attr |= (rng.random(self.full.n) < 0.02).astype(np.uint64) << np.uint64(k)
            self.attr[self.n:] = np.uint64((1 << 40) - 1)
        for c in (self.cols, self.full.cols):
            c.attr_match = self.attr.ctypes.data if on else None
            c.attr_match_words = 1 if on else 0
        return self


_built = {}


def _once(key, f):
    if key not in _built:
        _built[key] = f()
    return _built[key]


def end_layout(n):
    def build():
        last = min(n, 3)
        segs = [Seg("LAST", n - last, last, svc=N, route=False, early=None),
                Seg("POISON", n, TAIL, svc=A, zero=range(TAIL), error=range(TAIL), route=True, early=None)]
        full = tl.Batch(segs, n + TAIL, seed=0x7F00 + n % 1009)
        full.tid[n:] = full.tid[n - 1]      # the last trace's id continued
        return Sliced(full, n)
    return _once(("end", n), build)


def skip_layout(k, r):
    def build():
        n = tl.n_for(2)
        run = 64 * k + r
        full = tl.Batch([Seg("RUN", 0, run, [(A, run - 7), (B, 7)], early=1),
                         Seg("NEXT", run, 3, [(B, 1), (A, 2)], early=1),
                         Seg("POISON", n, TAIL, svc=A, zero=range(TAIL), error=range(TAIL), route=True, early=None)],
                        n + TAIL, seed=0x7E00 + 64 * k + r)
        full.tid[n:] = full.tid[n - 1]
        return Sliced(full, n)
    return _once(("skip", k, r), build)


def ids_layout(kind):
    def build():
        if kind == "singles":
            n, segs, singles = 197, [], True
        else:
            sh = 1 if kind == "shifted" else 0
            n, singles = sh + 256 + 40, False
            segs = [Seg(f"T{j}", sh + 64 * j, 64, [(A, 30), (B, 34)], early=1 + j) for j in range(4)]
        segs.append(Seg("POISON", n, TAIL, svc=A, zero=range(TAIL), error=range(TAIL), route=True, early=None))
        full = tl.Batch(segs, n + TAIL, seed=0x7D00 + len(kind), singles=singles)
        full.tid[n:] = full.tid[n - 1]
        return Sliced(full, n)
    return _once(("ids", kind), build)


CHAIN_ROUTE = "/api/v2/orders/1234567"
CHAIN_KINDS = [(ln, al) for ln in (0, 1, 15, 16, 17) for al in (0, 15)]


def chain_layout():
    def build():
        n = 200
        segs = [Seg(f"D{t}", 4 * t, 4, [(A, 1), (B, 1), (A, 1), (B, 1)], early=2) for t in range(n // 4)]
        segs.append(Seg("POISON", n, TAIL, svc=A, zero=range(TAIL), error=range(TAIL), route=True, early=None))
        full = tl.Batch(segs, n + TAIL, seed=0x7C00)
        full.tid[n:] = full.tid[n - 1]
        # the routes: each kind once in the arena, the 17-byte one at 15 mod 16 last
        blob, offs = bytearray(), []
        for ln, al in CHAIN_KINDS:
            blob += b"\0" * ((al - len(blob)) % 16)
            offs.append(len(blob))
            blob += CHAIN_ROUTE[:ln].encode()
        full.arena_bytes = len(blob)                       # the last route ends on the arena's last byte
        full.arena = np.zeros((len(blob) + 15) // 16 * 16 + 32, dtype=np.uint8)
        full.arena[:len(blob)] = np.frombuffer(bytes(blob), dtype=np.uint8)
        q = np.arange(n + TAIL)
        kind = (q + q // len(CHAIN_KINDS)) % len(CHAIN_KINDS)      # (A on even spans, B on odd: each meets every kind)
        kind[n:] = CHAIN_KINDS.index((16, 0))              # (the tail: a route with a rule's prefix)
        full.route = np.ascontiguousarray(np.stack([np.array(offs, dtype=np.uint32)[kind],
                                                    np.array([ln for ln, _ in CHAIN_KINDS], dtype=np.uint32)[kind]], axis=1))
        full.route_kind = kind
        full._bind()
        return Sliced(full, n)
    return _once(("chain",), build)


SMALL = {**{f"end.{n}": (lambda n=n: end_layout(n)) for n in END_SIZES if n < 1000},
         **{f"ids.{k}": (lambda k=k: ids_layout(k)) for k in ("singles", "aligned", "shifted")},
         "chain": chain_layout}
LAYOUTS = {**SMALL,
           **{f"end.{n}": (lambda n=n: end_layout(n)) for n in END_SIZES if n >= 1000},
           **{f"skip.{k}.{r}": (lambda k=k, r=r: skip_layout(k, r)) for k, r in SKIPS}}


# ---------------------------------------------------------------------------
# census (CPU): each layout holds its seam, the poisoned tail included

def _poison_census(s):
    full, n = s.full, s.n
    t = slice(n, n + TAIL)
    assert full.n == n + TAIL
    assert (full.tid[t] == full.tid[n - 1]).all()                       # no head at n: the last trace goes on
    assert (full.status[t] == native.STATUS_ERROR).all() and (full.start[t] == 0).all()
    lat = tl.lat_services(c3_sampling_config())
    assert (full.svc[t] == A).all() and A in lat and B in lat
    # in range: a wrong read shows as a wrong keep, never as a fault
    assert int(full.resource.max()) < len(full.res_svc) == s.cols.n_resources
    assert (full.res_svc[full.resource[t]] == A).all()
    off, ln = full.route[:, 0].astype(np.int64), full.route[:, 1].astype(np.int64)
    assert (off + ln <= full.arena_bytes).all() and len(full.arena) >= (full.arena_bytes + 15) // 16 * 16 + 16
    for i in range(n, n + TAIL, 37):
        route = bytes(full.arena[off[i]:off[i] + ln[i]]).decode()
        assert any(route.startswith(p) for p in lat[A]), route
    for f in ("tid", "status", "start", "end", "resource", "route"):
        assert len(getattr(full, f)) == n + TAIL


def _last_trace_level(cols, cfg):
    ho = oracle_run(cols, native.GROUP_TRACE_ID, cfg=cfg)
    t = int(ho.view("trace_count", np.uint32)[0])
    return int(ho.view("trace_level", np.uint8)[t - 1]), t


@pytest.mark.parametrize("n", END_SIZES)
def test_census_end(n):
    s = end_layout(n)
    _poison_census(s)
    assert s.cols.n_spans == n and tl.win_per_wave(n) == (2 if n >= N_W2 else 1)
    if n >= N_W2:
        assert (n + 63) // 64 in (8192, 8193, 8194)
    h = s.full.heads()
    assert h[n - min(n, 3)] and not h[n - min(n, 3) + 1:n + TAIL].any()     # LAST, and no head after its own
    assert (s.full.svc[n - min(n, 3):n] == N).all() and not (s.full.status[:n][-min(n, 3):] == native.STATUS_ERROR).any()
    # the poison would flip the last trace: level 0 (the error rule) with it, not without
    cfg = c3_sampling_config()
    with_tail, t1 = _last_trace_level(s.full.cols, cfg)
    without, t0 = _last_trace_level(s.cols, cfg)
    assert t0 == t1 and with_tail == 0 and without != 0, (with_tail, without)


@pytest.mark.parametrize("k,r", SKIPS)
def test_census_skip(k, r):
    s = skip_layout(k, r)
    _poison_census(s)
    assert tl.win_per_wave(s.n) == 2 and s.n == tl.n_for(2)
    h = s.full.heads()[:s.n]
    run = 64 * k + r
    assert h[0] and not h[1:run].any() and h[run] and h[run + 3]
    assert run // WAVE == k and run % WAVE == r
    wave = k // 2                      # the wave owning windows 2 * wave, 2 * wave + 1
    heads_before = int(h[2 * wave * WAVE:run].sum())
    if k > 1:
        # the owner's first window holds no head: it skips it, then owns from lane r of window k
        assert k == 2 * wave + 1 and heads_before == 0
    else:
        assert heads_before == 1       # (the run's own head: wave 0 never skips)
    _, _, headless = s.full.walk(2, 0, 8)
    assert headless == [w for w in (2,) if k == 5]      # k = 5: wave 1 owns no head at all


@pytest.mark.parametrize("kind", ["singles", "aligned", "shifted"])
def test_census_ids(kind):
    s = ids_layout(kind)
    _poison_census(s)
    h = s.full.heads()[:s.n]
    hp, ends = np.nonzero(h)[0], np.append(np.nonzero(h)[0][1:], s.n)
    if kind == "singles":
        assert h.all() and s.n > 3 * WAVE                       # every lane a head and a tail
    elif kind == "aligned":
        assert all(h[64 * j] and not h[64 * j + 1:64 * j + 64].any() for j in range(4))
        assert set(range(0, 256, 64)) <= set(hp.tolist()) and {63, 127, 191, 255} <= set((ends - 1).tolist())
    else:
        assert all(h[64 * j + 1] and not h[64 * j + 2:64 * j + 65].any() for j in range(4))
        assert {64, 128, 192, 256} <= set((ends - 1).tolist())  # tails at lane 0: lane 63 continues into the next step


def test_census_chain():
    s = chain_layout()
    _poison_census(s)
    full, n = s.full, s.n
    assert (np.diff(full.resource[:n].astype(np.int64)) == 1).all()          # a new resource on every span
    lat = tl.lat_services(c3_sampling_config())
    assert set(full.svc[:n].tolist()) == {A, B} <= set(lat)
    for f in (many_service_rules_config, wide_mixed_config, wide_latency2_config, wide_attr_config):
        assert {A, B} <= set(tl.lat_services(f())), f.__name__
    off, ln = full.route[:n, 0], full.route[:n, 1]
    seen = {(int(l), int(o) % 16) for l, o in zip(ln, off) if l}
    assert seen == {(l, a) for l, a in CHAIN_KINDS if l} and (ln == 0).any()
    # both services meet every kind; the long ones carry a C3 prefix, the short ones none
    for v in (A, B):
        assert {int(k) for k in full.route_kind[:n][full.svc[:n] == v]} == set(range(len(CHAIN_KINDS)))
        for l in (15, 16, 17):
            assert any(CHAIN_ROUTE[:l].startswith(p) for p in lat[v])
        assert not any(CHAIN_ROUTE[:1].startswith(p) for p in lat[v])
    last = int(np.argmax(off.astype(np.int64) + ln))
    assert int(off[last]) + int(ln[last]) == full.arena_bytes and (int(ln[last]), int(off[last]) % 16) == (17, 15)
    assert len(full.arena) > full.arena_bytes                                # inside a larger allocation


# ---------------------------------------------------------------------------
# the reference itself on the small layouts

@pytest.mark.parametrize("name", list(SMALL))
def test_oracle_vs_python(name):
    cfg = fractional_config()
    s = SMALL[name]()
    cols = s.cols
    ho = oracle_run(cols, native.GROUP_TRACE_ID, cfg=cfg)
    traces = _group(cols, False)
    assert int(ho.view("trace_count", np.uint32)[0]) == len(traces)
    svc_ids = intern_services(cfg)
    res = _arr(cols.resource, C.c_uint32, cols.n_spans)
    keep = ho.view("keep", np.uint8)
    for t, spans in enumerate(traces):
        hi, lo = int(s.full.tid[spans[0], 0]), int(s.full.tid[spans[0], 1])
        u = orc_lib().orc_trace_uniform(hi, lo, SEED)
        k, lvl, ratio = _py_eval(cfg, svc_ids, cols, res, spans, False, u)
        assert ho.view("trace_first_span", np.uint32)[t] == spans[0], t
        assert ho.view("trace_level", np.uint8)[t] == lvl, t
        assert ho.view("trace_ratio", np.float64)[t] == ratio, t
        assert (keep[spans] == int(k)).all(), t


# ---------------------------------------------------------------------------
# GPU: keep is the oracle's, bit for bit

_oracle_keep = {}


def gpu_keep_vs_oracle(name, cname):
    import torch
    from odigos_amd.batch import DeviceBatch, Engine
    cfg = CONFIGS[cname]()
    s = LAYOUTS[name]().with_attr(cname == "general")
    n = s.n
    try:
        if (name, cname) not in _oracle_keep:
            _oracle_keep[(name, cname)] = oracle_run(s.cols, native.GROUP_TRACE_ID, cfg=cfg).view("keep", np.uint8)[:n].copy()
        eng = Engine({"odigossampling": cfg})
        db = DeviceBatch(s.full.cols)          # the device columns hold the poisoned tail too
        db.cols.n_spans = n
        eng.profile(True)
        eng.process_device(db, native.STAGE_SAMPLE, native.GROUP_TRACE_ID, seed=SEED)
        torch.cuda.synchronize()
        ran = set(eng.profile_read())
    finally:
        s.with_attr(False)
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    assert KERNEL[cname] in ran, ran
    np.testing.assert_array_equal(db.out_numpy("keep")[:n], _oracle_keep[(name, cname)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", END_SIZES)
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_batch_ends(cname, n):
    gpu_keep_vs_oracle(f"end.{n}", cname)


@pytest.mark.gpu
@pytest.mark.parametrize("k,r", SKIPS)
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_skip_then_own(cname, k, r):
    gpu_keep_vs_oracle(f"skip.{k}.{r}", cname)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["singles", "aligned", "shifted"])
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_neighbour_ids(cname, kind):
    gpu_keep_vs_oracle(f"ids.{kind}", cname)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", list(CONFIGS))
def test_gpu_dependent_chain(cname):
    gpu_keep_vs_oracle("chain", cname)


# ---------------------------------------------------------------------------
# the machine code: nothing drains the prefetch

def _vmcnt_report():
    spec = importlib.util.spec_from_file_location("vmcnt_report", ROOT / "tools" / "vmcnt_report.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_no_drain_between_prefetch_and_back_edge():
    vr = _vmcnt_report()
    if not vr.hipcc():
        pytest.skip("hipcc is not installed")
    asm, _ = vr.compile_asm()
    for name, mangled in vr.KERNELS[:2]:
        assert name in ("trace_eval_kernel<true, true, false>", "trace_eval_kernel<true, false, false>")
        fn = vr.function_lines(asm, mangled)
        found = vr.check_drain(fn)
        assert found is not None, f"{name}: the prefetch marker is gone from the machine code"
        assert found == [], f"{name}: s_waitcnt vmcnt(0) between the prefetch and the back edge: {found}"
        text = [l for _, l in fn]
        assert sum(vr.M_FBEGIN in l for l in text) >= 3 and sum(vr.M_PREFETCH in l for l in text) == 1
