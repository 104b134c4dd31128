"""SAMPLE | TEMPLATE | SIZE in the refs form against the oracle chain: the
order of the step's tail (engine.cpp run_stages: where the per-scope sums
are cleared, what the copy / size launches wait for) and size_tail_kernel's
several tiles per iteration (size_kernel.hip).

* 2^20 spans is the smallest batch whose URL front is forked onto the side
  stream: there the scope sums are cleared ahead of the trace stage.  Below
  it, and without SAMPLE or without TEMPLATE, the clear stays behind the
  stage whose scratch the size scratch overlaps.
* Scope counts around the tile (256 scopes) and around one iteration of a
  block (kTailTiles = 4 tiles of 256 scopes per block, so 4 * 256 * 4 scopes
  fill four blocks' iterations exactly): the generated batch has one scope
  per resource, so its scope and resource columns are rebuilt here with
  resources whose scopes cross tile edges, spanless scopes and resources
  without scopes.
"""
import numpy as np
import pytest

from odigos_amd import native
from odigos_amd.batch import COLUMN_LAYOUT, DeviceBatch, Engine, Generator, HostOutputs
from tests.oracle_lib import SamplingOracle, UrlOracle, size_process, span_template_bytes
from tests.workloads import c3_sampling_config

REFS = native.STAGE_TEMPLATE | native.STAGE_TEMPLATE_REFS
FUSED = native.STAGE_SAMPLE | REFS | native.STAGE_SIZE
RULES = {"templatization_rules": ["/users/{user}/orders/{order:\\d+}", "/api/v1/*", "/{a}/{b}/{c}/{d}/{e}/{f}"],
         "custom_ids": [{"regexp": "^inc_\\d+$", "template_name": "incident"}, {"regexp": "(?i)^PROCESS_"}]}
TAIL_TILES = 4   # size_kernel.hip kTailTiles


def _cfg(url=None):
    return {"odigossampling": c3_sampling_config(), "odigosurltemplate": url or {},
            "odigostrafficmetrics": {"res_attributes_keys": ["service.name"]}}


def _oracle(cols, stages, cfg, seed):
    ho = HostOutputs(cols)
    if stages & native.STAGE_SAMPLE:
        assert SamplingOracle(cfg["odigossampling"]).process(cols, ho.outs, native.GROUP_TRACE_ID, seed, 8) == 0
    if stages & native.STAGE_TEMPLATE:
        assert UrlOracle(cfg["odigosurltemplate"]).process(cols, ho.outs, 8) == 0
    assert size_process(cols, ho.outs, stages, native.GROUP_TRACE_ID, ho.outs, 1, 1.0, 0.0, 8) == 0
    return ho


def _check(db, ho, cols, stages):
    ns, A, R = cols.n_spans, cols.n_attrsets, cols.n_resources
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    if stages & native.STAGE_SAMPLE:
        np.testing.assert_array_equal(db.out_numpy("keep")[:ns], ho.view("keep", np.uint8)[:ns])
    if stages & native.STAGE_TEMPLATE:
        np.testing.assert_array_equal(db.out_numpy("url_out")[:ns], ho.view("url_out", np.uint8)[:ns])
        mask = ho.view("url_out", np.uint8)[:ns] != 0
        got = span_template_bytes(db.out_numpy("tmpl", np.uint32)[: 2 * ns], db.out_numpy("tmpl_arena")[: db.used()], mask)
        want = span_template_bytes(ho.view("tmpl", np.uint32)[: 2 * ns], ho.bufs["tmpl_arena"][: int(ho.used[0])], mask)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(db.out_numpy("attrset_bytes", np.int64)[:A], ho.view("attrset_bytes", np.int64)[:A])
    assert int(db.out_numpy("accepted_spans", np.int64)[0]) == int(ho.view("accepted_spans", np.int64)[0])
    np.testing.assert_array_equal(db.out_numpy("res_bytes", np.uint64)[:R], ho.view("res_bytes", np.uint64)[:R])


def _gpu_vs_oracle(cols, stages, cfg, seed=0x5EED, calls=1):
    import torch
    used = {k: v for k, v in cfg.items()
            if (k == "odigossampling" and stages & native.STAGE_SAMPLE) or
            (k == "odigosurltemplate" and stages & native.STAGE_TEMPLATE) or k == "odigostrafficmetrics"}
    eng = Engine(used)
    db = DeviceBatch(cols)
    ho = _oracle(cols, stages, cfg, seed)
    for _ in range(calls):   # the same engine and buffers: each call's results stand alone
        db.o["attrset_bytes"].zero_()
        db.o["accepted_spans"].zero_()
        eng.process_device(db, stages, native.GROUP_TRACE_ID, seed=seed)
        torch.cuda.synchronize()
        _check(db, ho, cols, stages)


@pytest.fixture(scope="module")
def forked_batch():
    return Generator("fused", seed=0x0D1600F0, n_spans=1 << 20, threads=8)


@pytest.mark.gpu
def test_gpu_tail_forked_default(forked_batch):
    _gpu_vs_oracle(forked_batch.cols, FUSED, _cfg())


@pytest.mark.gpu
def test_gpu_tail_forked_rules_twice(forked_batch):
    # templatization rules: the slow list is long; twice on the same engine
    # and buffers (the second call's front must not start into the first's tail)
    _gpu_vs_oracle(forked_batch.cols, FUSED, _cfg(RULES), calls=2)


@pytest.mark.gpu
@pytest.mark.parametrize("stages", [FUSED, REFS | native.STAGE_SIZE, native.STAGE_SAMPLE | native.STAGE_SIZE],
                         ids=["fused", "template_size", "sample_size"])
def test_gpu_tail_unforked(stages):
    g = Generator("fused", seed=0x0D1600F1, n_spans=5000)
    _gpu_vs_oracle(g.cols, stages, _cfg())


class _Recut:
    """The first spans of a generated batch with scope and resource columns
    rebuilt to n_scopes scopes: every resource with spans gets one scope or
    many (runs of 70, 130 and 300 scopes cross 64-scope windows and 256-scope
    tiles), every other scope of a run stays spanless, and resources without
    scopes are put between the runs and after the last scope."""
    EXTRA = (0, 2, 0, 299, 0, 69, 1, 0, 129, 0, 4)

    def __init__(self, g, n_scopes):
        c = g.cols
        res = g.array("resource").view(np.uint32)[: c.n_spans].copy()
        n_used = max(1, min(int(res[-1]) + 1, n_scopes // 3))        # old resources kept (each has spans)
        ns = int(np.searchsorted(res, n_used))                       # their spans
        res = res[:ns]
        k = np.ones(n_used, dtype=np.int64)                          # scopes per kept resource
        left, i = n_scopes - n_used, 0
        while left > 0:
            add = min(self.EXTRA[i % len(self.EXTRA)], left)
            k[i % n_used] += add
            left -= add
            i += 1
        # new resources: the kept ones, a scopeless copy after every 7th, two after the last
        src, new_of = [], np.zeros(n_used, dtype=np.uint32)
        for r in range(n_used):
            new_of[r] = len(src)
            src.append(r)
            if r % 7 == 6:
                src.append(r)
        src += [n_used - 1, 0]
        src = np.asarray(src, dtype=np.int64)
        first = np.concatenate(([0], np.cumsum(k)[:-1]))             # first scope of each kept resource
        j = np.arange(ns) - np.searchsorted(res, res)                # a span's index within its resource
        scope = (first[res] + np.minimum(2 * j, k[res] - 1)).astype(np.uint32)
        rng = np.random.default_rng(n_scopes)
        self.keep = {"resource": new_of[res], "scope": scope,
                     "scope_size": rng.integers(20, 60, n_scopes, dtype=np.uint32),
                     "scope_resource": np.repeat(new_of, k).astype(np.uint32)}
        for name, (dim, size) in COLUMN_LAYOUT.items():
            if dim == "res" and getattr(c, name):
                self.keep[name] = g.array(name).reshape(-1, size)[src].copy()
        self.g = g                                                   # the other columns stay the generator's
        self.cols = native.Columns.from_buffer_copy(c)
        self.cols.n_spans, self.cols.n_scopes, self.cols.n_resources = ns, n_scopes, len(src)
        for name, a in self.keep.items():
            setattr(self.cols, name, a.ctypes.data)
        assert np.all(np.diff(scope.astype(np.int64)) >= 0) and int(scope[-1]) < n_scopes


@pytest.fixture(scope="module")
def recut_source():
    return Generator("fused", seed=0x0D1600F2, n_spans=8000)


@pytest.mark.gpu
@pytest.mark.parametrize("n_scopes", [1, 255, 256, 257, 4 * 256 * TAIL_TILES - 1, 4 * 256 * TAIL_TILES,
                                      4 * 256 * TAIL_TILES + 1])
def test_gpu_tail_scope_counts(recut_source, n_scopes):
    b = _Recut(recut_source, n_scopes)
    _gpu_vs_oracle(b.cols, FUSED, _cfg())
    _gpu_vs_oracle(b.cols, native.STAGE_SIZE, _cfg())
