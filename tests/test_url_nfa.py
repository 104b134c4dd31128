"""The NFA route of the URL stage on the GPU: an odigosurltemplate regexp
whose DFA passes the device bounds is an NFA program (regex_nfa.hpp), and an
engine whose tables hold one plans and writes every group per lane
(url_nfa_fill_kernel, url_nfa_plan_kernel, url_nfa_emit_kernel), the regexp
call site dispatching on DFA / NFA.  Everything is compared with the oracle
(oracle/url.c) byte for byte; the engine option "url_regex_nfa" forces the
route on configs whose regexps also have DFAs, so both routes run on the same
batch.  Engine.path_counts()["url_nfa"] is the witness of the route.  The host
side of the matcher is tests/test_regex_nfa.py."""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

from odigos_amd import native
from tests import url_layouts as ul
from tests.oracle_lib import UrlOracle, span_template_bytes
from tests.test_regex_large import LARGE_URL_CFG
from tests.test_regex_nfa import CJK, CJK_ALT
from tests.test_unicode_regex import _cols_from_paths
from tests.url_layouts import Lane, Layout

pytestmark = pytest.mark.gpu

TEMPLATE = native.STAGE_TEMPLATE
REFS = native.STAGE_TEMPLATE | native.STAGE_TEMPLATE_REFS

# config A: one state-blowup custom id (its engine takes seconds to create:
# the subset construction runs into its cap first) and a class-count rule
CFG_A = {
    "custom_ids": [{"regexp": r"^(?:a|b)*a(?:a|b){20}$", "template_name": "ab"}],
    "templatization_rules": [r"/s/{seq:^" + CJK_ALT + r"+$}/{rest}"],
}
# free to create: the class-count custom id is an NFA program, the ids around it are DFAs
HAN = {"regexp": "^(?:" + "|".join(CJK) + "|yb|xa)+$", "template_name": "han"}
CFG_ORDER = {"custom_ids": [{"regexp": r"^xa$", "template_name": "pre"}, HAN, {"regexp": r"^(?:yb|zz)$", "template_name": "post"}]}
# an NFA custom id as the 16th name: id 18, outside the plan code's 4 bits
CFG_16TH = {"custom_ids": [{"regexp": "^\x01never%d\x01$" % k, "template_name": "n%d" % k} for k in range(15)] + [HAN]}
# regexps with DFAs, run under the forced option: assertions, (?m), UTF-8, rules that fall through
CFG_SEAMS = {
    "custom_ids": [
        {"regexp": r"^(?:a|b)*a(?:a|b){5}$", "template_name": "ab"},
        {"regexp": r"\bfoo\b", "template_name": "foo"},
        {"regexp": r"^\B-.*-\B$", "template_name": "dash"},
        {"regexp": r"(?m)^end$", "template_name": "ml"},
        {"regexp": r"^[α-ω]+$", "template_name": "gr"},
        {"regexp": r"^z.$", "template_name": "z1"},
        {"regexp": r"^z..$", "template_name": "z2"},
    ],
    "templatization_rules": [r"/r/{n:^[0-9]+x$}/{rest}", r"/r/{w:^w+$}/tail", r"/q/regex:^[ab]{3}$"],
}

_engines = {}


def _engine(cfg, extra=None):
    from odigos_amd.batch import Engine
    key = repr((cfg, extra))
    if key not in _engines:
        full = {"odigosurltemplate": cfg}
        full.update(extra or {})
        eng = Engine(full)
        eng.set_option("url_path_counts", 1)
        _engines[key] = eng
    return _engines[key]


def _oracle(cfg, cols, tmpl_cap=None):
    from odigos_amd.batch import HostOutputs
    ho = HostOutputs(cols, tmpl_cap=tmpl_cap)
    assert UrlOracle(cfg).process(cols, ho.outs, 8) == 0
    n, used = cols.n_spans, int(ho.used[0])
    return (ho.view("url_out", np.uint8)[:n].copy(), ho.view("tmpl", np.uint32)[:2 * n].copy(),
            ho.bufs["tmpl_arena"][:used].copy(), used)


def _gpu(cfg, cols, want, forced, nfa=True, stage=TEMPLATE, tmpl_cap=None):
    """One TEMPLATE call compared with the oracle's (url_out, refs, arena,
    used); nfa: whether the call must have taken the NFA route."""
    import torch
    from odigos_amd.batch import DeviceBatch
    eng = _engine(cfg)
    eng.set_option("url_regex_nfa", int(forced))
    db = DeviceBatch(cols, tmpl_cap=tmpl_cap)
    eng.process_device(db, stage)
    torch.cuda.synchronize()
    eng.set_option("url_regex_nfa", 0)
    n = cols.n_spans
    groups = (n + 63) // 64
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    url_out, refs, arena, used = want
    np.testing.assert_array_equal(db.out_numpy("url_out", n=n), url_out)
    mask = url_out != 0
    gt = db.out_numpy("tmpl", np.uint32)[:2 * n]
    if stage & native.STAGE_TEMPLATE_REFS:
        got = span_template_bytes(gt, db.out_numpy("tmpl_arena")[:db.used()], mask)
        for a, b in zip(got, span_template_bytes(refs, arena, mask)):
            np.testing.assert_array_equal(a, b)
    else:
        assert db.used() == used
        np.testing.assert_array_equal(db.out_numpy("tmpl_arena", n=used), arena)
        np.testing.assert_array_equal(gt.reshape(-1, 2)[mask], refs.reshape(-1, 2)[mask])
    c = eng.path_counts()
    if n:
        assert c["url_nfa"] == (groups if nfa else 0), c
        if nfa:
            assert c["url_unplanned"] == groups


def _both_routes(cfg, cols, tmpl_cap=None, stages=(TEMPLATE,)):
    """Option on equals option off equals the oracle.  (A config without a
    user regexp has no NFA program under the option either: it keeps its route.)"""
    from tests.test_regex_nfa import _blob
    want = _oracle(cfg, cols, tmpl_cap)
    for st in stages:
        _gpu(cfg, cols, want, forced=False, nfa=False, stage=st, tmpl_cap=tmpl_cap)
        _gpu(cfg, cols, want, forced=True, nfa=_blob(cfg, True)[2] > 0, stage=st, tmpl_cap=tmpl_cap)
    return want


def _paths_a(n, seed):
    rng = random.Random(seed)
    cjk = [c.encode() for c in CJK]
    near = [cjk[0] + b"a", chr(0x4E01).encode(), cjk[1] + chr(0x4E01).encode(), b"", b"s", cjk[2][:2], cjk[4] + b"\xff"]
    paths = []
    for _ in range(n):
        segs = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(1, 31))) for _ in range(rng.randrange(1, 5))]
        if rng.random() < 0.2:
            mid = b"".join(rng.choice(cjk) for _ in range(rng.randrange(1, 4))) if rng.random() < 0.6 else rng.choice(near)
            segs = [b"s", mid, segs[0]]
        paths.append(b"/" + b"/".join(segs))
    return paths


@pytest.fixture(scope="module")
def batch_a():
    paths = _paths_a(64 * 60 + 17, 0x0D1600F1)
    cols, keep = _cols_from_paths(paths)
    return cols, keep, _oracle(CFG_A, cols)


def test_parity_config_a(batch_a):
    cols, _keep, want = batch_a
    arena = want[2].tobytes()
    assert b"{ab}" in arena and b"{seq}" in arena   # both regexps decide something: parity is not vacuous
    _gpu(CFG_A, cols, want, forced=False)           # the tables hold NFA programs without the option
    _gpu(CFG_A, cols, want, forced=False, stage=REFS)


def test_config_a_through_ose_process(batch_a):
    from odigos_amd.batch import PinnedBatch, host_array
    cols, _keep, want = batch_a
    n = cols.n_spans
    pb = PinnedBatch(_engine(CFG_A), cols)
    pb.fill(cols)
    pb.process(TEMPLATE)
    np.testing.assert_array_equal(host_array(pb.outs.url_out, n), want[0])
    used = int(host_array(pb.outs.tmpl_arena_used, 8).view(np.uint64)[0])
    assert used == want[3]
    np.testing.assert_array_equal(host_array(pb.outs.tmpl_arena, used), want[2])
    pb.close()


def test_forced_option_large_dfa_config():
    rng = random.Random(0x0D1600E1)
    paths = []
    for _ in range(64 * 40 + 5):
        segs = ["".join(rng.choice("ab") for _ in range(rng.randrange(1, 30))) for _ in range(rng.randrange(1, 5))]
        if rng.random() < 0.2:
            segs = ["s"] + segs[:2]
        paths.append(("/" + "/".join(segs)).encode())
    cols, _keep = _cols_from_paths(paths)
    want = _both_routes(LARGE_URL_CFG, cols, stages=(TEMPLATE, REFS))
    assert b"{ab}" in want[2].tobytes() and b"{seq}" in want[2].tobytes()


GOLD = json.loads((Path(__file__).parent / "golden" / "url_kats.json").read_text())["rule_cases"]["cases"]


def _kat_cfgs():
    seen, out = set(), []
    for c in GOLD:
        cfg = {k2: c[k] for k, k2 in (("rules", "templatization_rules"), ("custom_ids", "custom_ids")) if k in c}
        if repr(cfg) not in seen:
            seen.add(repr(cfg))
            out.append(cfg)
    return out


@pytest.mark.parametrize("cfg", _kat_cfgs(), ids=["kat%d" % k for k in range(len(_kat_cfgs()))])
def test_forced_option_kat_rules_and_custom_ids(cfg):
    # every KAT path under every KAT config: the config's own paths and the others' as near misses
    cols, _keep = _cols_from_paths([c["path"].encode() for c in GOLD] * 4)
    _both_routes(cfg, cols)


def test_option_needs_the_url_section():
    from odigos_amd.batch import Engine
    eng = Engine({"odigostrafficmetrics": {"res_attributes_keys": ["service.name"]}})
    assert eng.L.ose_engine_set_option(eng.h, b"url_regex_nfa", 1) == native.OSE_EINVAL
    eng.close()


# ---------------------------------------------------------------------------
# hand-laid seams

def _pad(lanes, fill=b"/health"):
    return lanes + [Lane(fill) for _ in range(-len(lanes) % 64)]


def _layout(name, lanes, whole=True):
    groups = [lanes[k:k + 64] for k in range(0, len(lanes), 64)]
    if whole:
        groups[-1] = _pad(groups[-1])
    return Layout(name, groups, seed=len(name))


def _check_layout(L, cfg, forced, nfa=True, stages=(TEMPLATE, REFS)):
    url_out, refs, arena, used = L.oracle(cfg)
    for st in stages:
        _gpu(cfg, L.cols, (url_out, refs.reshape(-1), arena, used), forced, nfa=nfa, stage=st, tmpl_cap=ul.tmpl_cap(L))
    return arena.tobytes()


AB6 = b"bbabbbbb"   # an 'a' six from the end: {ab} under CFG_SEAMS


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_seam_group_edges(n):
    paths = [b"/x/" + AB6 + b"/%d" % k for k in range(n)]
    cols, _keep = _cols_from_paths(paths)
    want = _oracle(CFG_SEAMS, cols)
    _gpu(CFG_SEAMS, cols, want, forced=True)
    assert n == 0 or want[2].tobytes().count(b"{ab}") == n


def test_seam_group_without_a_path():
    # gates 0 and 1 only in the middle group: no span of it has a path to plan
    g1 = [Lane(b"/x/" + AB6) for _ in range(64)]
    g2 = [Lane(None, flags=0) if k % 2 else Lane(None, flags=ul.HAS | native.URL_TGT_STR_EMPTY | ul.EQ) for k in range(64)]
    L = Layout("nfa.nopath", [g1, g2, list(g1)], seed=3)
    assert set(ul.gate_of(int(f), int(k)) for f, k in zip(L.flags[64:128], L.kind[64:128])) == {0, 1}
    out = _check_layout(L, CFG_SEAMS, True)
    assert out.count(b"{ab}") == 128


def test_seam_empty_and_tiny_segments():
    lanes = [Lane(p) for p in (b"//", b"/a//" + AB6, b"/x/" + AB6 + b"/", b"/a", b"a", b"/", b"", b"/k/j/" + AB6, b"//" + AB6 + b"//",
                               b"/b/" + AB6 + b"/b")]
    out = _check_layout(_layout("nfa.tiny", lanes), CFG_SEAMS, True)
    assert out.count(b"{ab}") == 5


def test_seam_emitter_reclassifies():
    # a hit at segment index 16 and beyond: the plan is `slow`, url_nfa_emit_kernel classifies again
    lanes = [Lane(b"/" + b"/".join([b"k"] * k + [AB6] + [b"t"] * t)) for k in (14, 15, 16, 17, 30) for t in (0, 1, 3)]
    out = _check_layout(_layout("nfa.seg16", lanes), CFG_SEAMS, True)
    assert out.count(b"{ab}") == 15
    # an NFA custom id as the 16th name (id 18): no option, the class-count regexp has no DFA
    han = (CJK[3] + CJK[299]).encode()
    lanes = [Lane(b"/u/" + han), Lane(b"/" + han + b"/u/" + han), Lane(b"/u/" + han[:-1]), Lane(b"/yb/xa/zz")]
    out = _check_layout(_layout("nfa.16th", lanes), CFG_16TH, False)
    assert out.count(b"{han}") == 5


def test_seam_long_path():
    # over 3 KB and over 4 KB (the stage of the NFA kernels): LDS and HBM readers, hits at both ends
    lanes = []
    for n in (3100, 4200):
        body = ul.path_len(n, salt=n)
        lanes += [Lane(b"/" + AB6 + body + b"/" + AB6), Lane(body + b"/" + AB6 + b"/k")]
    lanes += [Lane(b"/x/" + AB6) for _ in range(6)]
    out = _check_layout(_layout("nfa.long", lanes), CFG_SEAMS, True)
    assert out.count(b"{ab}") == 12


def test_seam_question_mark_cut():
    # http.target: the '$' of the regexp is the cut, not the end of the attribute
    lanes = [Lane(b"/x/" + AB6 + b"?q=" + AB6, flags=ul.TARGET), Lane(b"/x/" + AB6 + b"b?", flags=ul.TARGET),
             Lane(b"/x/" + AB6 + b"?", flags=ul.TARGET), Lane(b"/x/" + AB6 + b"?q", flags=ul.RAW), Lane(b"?/" + AB6, flags=ul.TARGET),
             Lane(b"/r/12x/t?x/y", flags=ul.TARGET)]
    out = _check_layout(_layout("nfa.qm", lanes), CFG_SEAMS, True)
    assert out.count(b"{ab}") == 2 and b"/r/{n}/{rest}" in out


def test_seam_assertions_and_utf8():
    segs = [b"foo", b"foo-x", b"x-foo", b"xfoo", b"foox", b"a foo", b"-a-", b"-a", b"a-", b"--", b"x\nend", b"end\nx", b"xend", b"end",
            "αβγ".encode(), "αβc".encode(), "αβγ".encode()[:-1], b"z\xff", b"z\xe4\xb8", b"z\xe4\xb8\x80", b"z\xc3", b"z\xc3\xa9x",
            b"\xffz", b"z"]
    lanes = [Lane(b"/p/" + s) for s in segs] + [Lane(b"/" + s + b"/q") for s in segs]
    out = _check_layout(_layout("nfa.assert", lanes), CFG_SEAMS, True)
    for name in (b"{foo}", b"{dash}", b"{ml}", b"{gr}", b"{z1}", b"{z2}"):
        assert name in out, name


def test_seam_first_match_wins_across_routes():
    # a DFA custom id before and after an NFA one, no option: the tables hold both kinds
    lanes = [Lane(b"/xa"), Lane(b"/yb"), Lane(b"/zz"), Lane(b"/" + CJK[7].encode()), Lane(b"/xayb"), Lane(b"/zzz"), Lane(b"/xa/yb/zz")]
    out = _check_layout(_layout("nfa.order", lanes), CFG_ORDER, False)
    assert out.count(b"{pre}") == 2 and out.count(b"{han}") == 4 and out.count(b"{post}") == 2


def test_seam_rule_fallback():
    # the first rule's regexp segment fails: the next rule, then the default templatization decide
    lanes = [Lane(b"/r/12x/t"), Lane(b"/r/12/tail"), Lane(b"/r/www/tail"), Lane(b"/r/12/other"), Lane(b"/r/wx/tail"), Lane(b"/q/aba"),
             Lane(b"/q/abab"), Lane(b"/r/" + AB6 + b"/tail")]
    out = _check_layout(_layout("nfa.rules", lanes), CFG_SEAMS, True)
    assert b"/r/{n}/{rest}" in out and b"/r/{w}/tail" in out and b"/r/{id}/other" in out and b"/q/aba" in out and b"/r/{ab}/tail" in out


def test_seam_include_exclude():
    # res_url_ok 0 for one of two resources
    lanes = [Lane(b"/x/" + AB6 + b"/%d" % k) for k in range(70)]
    L = _layout("nfa.resok", lanes, whole=False)
    cols = native.Columns()
    C.memmove(C.byref(cols), C.byref(L.cols), C.sizeof(cols))
    res = (np.arange(L.n) % 2).astype(np.uint32)
    ok = np.array([1, 0], dtype=np.uint8)
    cols.n_resources, cols.resource, cols.res_url_ok = 2, res.ctypes.data, ok.ctypes.data
    want = _oracle(CFG_SEAMS, cols, ul.tmpl_cap(L))
    assert want[0][0] != 0 and want[0][1] == 0 and want[2].tobytes().count(b"{ab}") == 35
    _gpu(CFG_SEAMS, cols, want, forced=True, tmpl_cap=ul.tmpl_cap(L))


def test_fused_refs_form_with_sampling_and_traffic():
    # SAMPLE | TEMPLATE | SIZE, refs form, on an engine whose URL tables hold an NFA program beside a DFA
    import torch
    from odigos_amd.batch import DeviceBatch, Generator, HostOutputs
    from tests.oracle_lib import SamplingOracle, size_process
    from tests.workloads import c3_sampling_config
    url = {"custom_ids": [HAN, {"regexp": r"^[0-9]{2,}$", "template_name": "num"}]}
    cfg = {"odigossampling": c3_sampling_config(), "odigostrafficmetrics": {"res_attributes_keys": ["service.name"]}}
    g = Generator("fused", seed=0x0D1600F2, n_spans=64 * 50 + 9)
    eng = _engine(url, cfg)
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    db = DeviceBatch(g.cols)
    eng.process_device(db, st | native.STAGE_TEMPLATE_REFS, seed=13)
    torch.cuda.synchronize()
    assert int(db.out_numpy("device_status", np.uint32)[0]) == 0
    ns, A = g.cols.n_spans, g.cols.n_attrsets
    ho = HostOutputs(g.cols)
    assert SamplingOracle(cfg["odigossampling"]).process(g.cols, ho.outs, native.GROUP_TRACE_ID, 13, 8) == 0
    assert UrlOracle(url).process(g.cols, ho.outs, 8) == 0
    assert size_process(g.cols, ho.outs, st, native.GROUP_TRACE_ID, ho.outs, 1, 1.0, 0.0, 8) == 0
    np.testing.assert_array_equal(db.out_numpy("keep")[:ns], ho.view("keep", np.uint8)[:ns])
    np.testing.assert_array_equal(db.out_numpy("url_out")[:ns], ho.view("url_out", np.uint8)[:ns])
    np.testing.assert_array_equal(db.out_numpy("attrset_bytes", np.int64)[:A], ho.view("attrset_bytes", np.int64)[:A])
    assert int(db.out_numpy("accepted_spans", np.int64)[0]) == int(ho.view("accepted_spans", np.int64)[0])
    m = ho.view("url_out", np.uint8)[:ns] != 0
    want = span_template_bytes(ho.view("tmpl", np.uint32)[:2 * ns], ho.bufs["tmpl_arena"][:int(ho.used[0])], m)
    got = span_template_bytes(db.out_numpy("tmpl", np.uint32)[:2 * ns], db.out_numpy("tmpl_arena")[:db.used()], m)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert b"{num}" in ho.bufs["tmpl_arena"][:int(ho.used[0])].tobytes()
    assert eng.path_counts()["url_nfa"] == (ns + 63) // 64
