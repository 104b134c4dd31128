"""url.full / http.url parsed on the GPU (engine option otlp_url_full):
ose_otlp_decode computes the Path of net/url.Parse on the device
(otlp_url_full_kernel.hip, url_full.hpp) for every span whose chosen value is a
string_value, and unescapes the paths that hold escapes into the arena behind
the host pass's strings.

Expected columns come from the host columniser over the same traces
(host.Processor("pipeline", cfg).columnarize, whose url.Parse is urlparse.cpp's
go_url_parse_path), compared with tests/test_otlp._compare.  The messages are
written by tests/otlp_gogo.py (pdata's encoding) and by google.protobuf
(tests/test_otlp.py to_pb).  ose_otlp_url_full_counts is the witness that the
device route ran; on the parent commit set_option("otlp_url_full") is
OSE_EINVAL, so every GPU test here fails without the feature.
"""
import base64
import copy
import ctypes as C
import random
import threading

import numpy as np
import pytest

from odigos_amd import host, native
from tests import otlp_gogo as gg
from tests.test_otlp import CFG, SEED, _compare, to_pb
from tests.url_full_cases import HAND, kat_cases

MARSHAL = {"pdata": gg.marshal_traces, "protobuf": to_pb}
FULL, OLD = "url.full", "http.url"
RESOURCES = [{"service.name": "svc-a", "k8s.pod.name": "pod-0"}, {"service.name": "svc-b", "k8s.pod.name": "pod-1"},
             {"service.name": "svc-c", "k8s.pod.name": "pod-2"}]
# 4096 bytes whose Path holds escapes ("p%41th/" is 7 bytes: the cut falls after a whole escape)
LONG_URL = ("http://h/" + "p%41th/" * 600)[:4096]
ESCAPED = "https://example.com/caf%C3%A9/a%20b/%41?x=%zz#frag"   # decoded: 12 bytes


def _kv(key, value):
    """value: a Python scalar, or an AnyValue dict ({} = no value set)"""
    if isinstance(value, dict):
        return {"key": key, "value": value}
    return {"key": key, "value": host.attr_value(value)}


M = _kv("http.request.method", "GET")


def _cases():
    """Attribute lists (in wire order) of the spans: every case of the parse pass."""
    text = "http://h/user/%31/x"
    out = [[M, _kv(FULL, text[:k])] for k in (0, 1, 15, 16, 17)]
    out += [
        [M, _kv(FULL, LONG_URL)],
        [M, _kv(FULL, ESCAPED)],
        [_kv("http.method", "POST"), _kv(OLD, "http://example.com/orders/77?x=1")],
        # both keys, in either order: url.full is the source; each key twice: the first wins
        [M, _kv(OLD, "http://h/old/1"), _kv(FULL, "http://h/full/1")],
        [M, _kv(FULL, "http://h/full/2"), _kv(OLD, "http://h/old/2")],
        [M, _kv(FULL, "/%zz"), _kv(FULL, "http://h/second")],
        [M, _kv(FULL, "http://h/first%20one"), _kv(FULL, "/%zz")],
        [M, _kv(OLD, "http://h/old/first"), _kv(OLD, ":bad")],
        [M, _kv(OLD, ":bad"), _kv(OLD, "http://h/old/second")],
        # look-alike keys: another last byte, shorter, longer; alone, and before the real key
        [M, _kv("url.fulm", "http://h/a"), _kv("http.urk", "http://h/b"), _kv("url.ful", "http://h/c"),
         _kv("url.full2", "http://h/d")],
        [M, _kv("url.fulm", "http://h/a"), _kv("vrl.full", "http://h/b"), _kv(OLD, "http://h/real%2Fone")],
        # another path source beside it: url.full is ignored, whatever it holds
        [M, _kv("url.path", "/from/path"), _kv(FULL, "http://h/ignored")],
        [M, _kv(FULL, "/%zz"), _kv("http.target", "/from/target?q=1")],
        [M, _kv(FULL, {"intValue": "5"}), _kv("url.path", "/p")],
        # no method; a method that is not a string (AsString: the host pass)
        [_kv(FULL, "http://h/no/method")],
        [_kv("http.request.method", 7), _kv(FULL, "http://h/int/method")],
        # a chosen value that is not a string_value: AsString, the host pass
        [M, _kv(FULL, {"intValue": "42"})],
        [M, _kv(FULL, {"boolValue": True})],
        [M, _kv(FULL, {"doubleValue": 2.5})],
        [M, _kv(FULL, {"bytesValue": base64.b64encode(b"/bytes").decode()})],
        [M, _kv(FULL, {"arrayValue": {"values": [{"stringValue": "/a"}]}})],
        [M, _kv(FULL, {})],
        [M, _kv(OLD, {"intValue": "7"})],
        [M, _kv(FULL, {"intValue": "7"}), _kv(OLD, "http://h/string/behind")],   # url.full is chosen: the host pass
        [M, _kv(OLD, {"intValue": "7"}), _kv(FULL, "http://h/string%20chosen")],  # ... and here the string is
        # with a target attribute, a route for the sampling stage, another kind
        [M, _kv("url.template", "/t/{id}"), _kv(FULL, "http://h/users/12345")],
        [M, _kv("http.route", "/api"), _kv(FULL, "http://h/api/1234567")],
    ]
    out += [[M, _kv(FULL, s.decode())] for s in HAND]
    return out


def _chosen(at):
    """(reason the span takes the host pass or None, the url string the parse pass reads or None)"""
    def first(key):
        return next((kv["value"] for kv in at if kv["key"] == key), None)
    m = first("http.request.method") or first("http.method")
    if m is None:
        return None, None
    if "stringValue" not in m:
        return "method", None
    if first("url.path") is not None or first("http.target") is not None:
        return None, None
    v = first(FULL) if first(FULL) is not None else first(OLD)
    if v is None:
        return None, None
    if "stringValue" not in v:
        return "url", None
    return None, v["stringValue"]


def _counts(td):
    """(spans with a host-only reason, spans whose url the GPU parses) of a tree of _tree's spans"""
    host_only = parsed = 0
    for rs in td["resourceSpans"]:
        for ss in rs["scopeSpans"]:
            for sp in ss["spans"]:
                why, url = _chosen(sp["attributes"])
                host_only += why is not None
                parsed += url is not None
    return host_only, parsed


def _tree(attr_lists, seed=1):
    """One span per attribute list, over three resources, two scopes in the larger ones."""
    rng = random.Random(seed)
    spans = []
    for k, at in enumerate(attr_lists):
        sp = host.span(name=rng.choice(["GET", "op", ""]), kind=rng.choice([2, 3]), trace_id="%032x" % (1 + k % 7),
                       span_id="%016x" % (k + 1), start=1739000000000000000 + k, end=1739000000000000000 + k + 1000,
                       status=k % 3)
        sp["attributes"] = copy.deepcopy(at)
        spans.append(sp)
    n = len(spans)
    per = max(1, (n + len(RESOURCES) - 1) // len(RESOURCES))
    rss = []
    for r, res in enumerate(RESOURCES):
        part = spans[r * per:(r + 1) * per]
        if not part:
            continue
        if len(part) > 3:
            rss.append(host.resource_spans(res, scopes=[{"scope": {"name": "l0"}, "spans": part[:2]},
                                                        {"scope": {"name": "l1"}, "spans": part[2:]}]))
        else:
            rss.append(host.resource_spans(res, part))
    return host.traces(*rss)


def _cycle(n, seed=1):
    cases = _cases()
    return _tree([cases[k % len(cases)] for k in range(n)], seed)


def _engine(on=True, cfg=CFG):
    from odigos_amd.batch import Engine
    eng = Engine(cfg)
    eng.set_option("otlp_url_full", 1 if on else 0)
    return eng


def _paths(cols, got):
    """(url_flags, the path bytes where a source is set else None); every ref in bounds of arena_bytes"""
    n = cols.n_spans
    flags = got["url_flags"][:n]
    refs = got["path"].view(np.uint32).reshape(-1, 2)[:n]
    assert all(int(o) + int(l) <= cols.arena_bytes for o, l in refs)
    arena = got["arena"]
    return flags, [bytes(arena[o:o + l]) if f & native.URL_PATH_MASK else None for f, (o, l) in zip(flags, refs)]


def _expected(td, cfg=CFG):
    p = host.Processor("pipeline", cfg)
    return p, p.columnarize(td)


def _check(eng, msg, td, hb, parsed=None, host_only=None):
    """decode with the option on: all columns equal the columniser's, the refs in
    bounds, the counts exact; returns the open batch and its download"""
    from odigos_amd.batch import OtlpBatch
    ob = OtlpBatch(eng, msg) if isinstance(msg, bytes) else OtlpBatch(eng, msg.p, length=msg.n)
    got = ob.download()
    _compare(ob.cols, hb.cols, got)
    _paths(ob.cols, got)
    want_host, want_parsed = _counts(td)
    assert ob.host_spans == (want_host if host_only is None else host_only)
    assert ob.url_full_counts[0] == (want_parsed if parsed is None else parsed)
    return ob, got


def test_cases_cover_the_ground():
    """CPU: what the case table holds, by the columniser and the host seam."""
    from tests.test_url_full_option import DECODED, EMPTY, ERROR, IN_PLACE, parse
    cases = _cases()
    urls = [_chosen(at)[1] for at in cases]
    assert {0, 1, 15, 16, 17, 4096} <= {len(u) for u in urls if u is not None}
    outcomes = [parse(u.encode())[0] for u in urls if u is not None]
    assert {ERROR, EMPTY, IN_PLACE, DECODED} == set(outcomes) and outcomes.count(DECODED) >= 12
    reasons = [_chosen(at)[0] for at in cases]
    assert reasons.count("url") == 8 and reasons.count("method") == 1
    assert parse(ESCAPED.encode()) == (DECODED, 19, 20, b"/caf\xc3\xa9/a b/A")
    oc, off, ln, path = parse(LONG_URL.encode())
    assert (oc, off, ln) == (DECODED, 8, 4088) and len(path) == 4088 - 2 * 584
    td = _cycle(len(cases))
    p, hb = _expected(td)
    n = hb.cols.n_spans
    flags = np.ctypeslib.as_array((C.c_uint8 * n).from_address(hb.cols.url_flags))
    # url.full beside url.path / http.target is ignored; without a method there is no path at all
    k = cases.index([M, _kv("url.path", "/from/path"), _kv(FULL, "http://h/ignored")])
    assert flags[k] & native.URL_PATH_MASK == native.URL_PATH_RAW
    assert flags[k + 1] & native.URL_PATH_MASK == native.URL_PATH_TARGET
    assert flags[cases.index([_kv(FULL, "http://h/no/method")])] == 0
    p.close()


# ---------------------------------------------------------------------------
# 1. the reference's KATs

@pytest.mark.gpu
def test_gpu_kat_spans():
    import torch
    from odigos_amd.batch import OtlpBatch
    cases = kat_cases()
    assert len(cases) == 5
    spans = []
    for k, (_, c) in enumerate(cases):
        spans.append(host.span(name=c["span"], kind=c["kind"], attributes=c["attrs"], trace_id="%032x" % (k + 1),
                               span_id="%016x" % (k + 1), start=1, end=2))
    res = {"service.name": "GET", "k8s.namespace.name": "default", "k8s.deployment.name": "GET"}
    td = host.traces(host.resource_spans(res, spans))
    cfg = {"odigosurltemplate": {}, "odigostrafficmetrics": {}}
    eng = _engine(cfg=cfg)
    for enc in MARSHAL:
        ob = OtlpBatch(eng, MARSHAL[enc](td))
        assert ob.host_spans == 0 and ob.url_full_counts == (5, 0)
        eng.process_device(ob, native.STAGE_TEMPLATE)
        torch.cuda.synchronize()
        url_out = ob.out_numpy("url_out", n=5)
        out = gg.apply(td, url_out=url_out, tmpls=_templates(ob, 5))
        for sp, (_, c) in zip(out["resourceSpans"][0]["scopeSpans"][0]["spans"], cases):
            assert sp["name"] == c["expect_name"], c["name"]
            v = host.find_attr(sp, c["expect_key"])
            if c["expect_value"] is None:
                assert v is None, c["name"]
            else:
                assert v is not None and host.as_string(v) == c["expect_value"], c["name"]
        # the same through the host shim, whose columniser parses on the host
        p = host.Processor("odigosurltemplate", {})
        hb = p.columnarize(td)
        from tests.oracle_lib import UrlOracle
        assert UrlOracle({}).process(hb.cols, hb.outs) == 0
        np.testing.assert_array_equal(url_out, np.ctypeslib.as_array((C.c_uint8 * 5).from_address(hb.outs.url_out)))
        p.close()
        ob.close()
    eng.close()


def _templates(ob, n):
    """the spans' template strings (None where the span has none) from the TEMPLATE outputs"""
    refs = ob.out_numpy("tmpl", np.uint32, n=2 * n).reshape(-1, 2)
    arena = ob.out_numpy("tmpl_arena", n=ob.used()).tobytes()
    return [arena[o:o + l].decode() if l else None for o, l in refs]


# ---------------------------------------------------------------------------
# 2. the case table

@pytest.mark.gpu
@pytest.mark.parametrize("enc", ["pdata", "protobuf"])
def test_gpu_case_table(enc):
    from odigos_amd.batch import OtlpBatch
    n = 2 * len(_cases()) + 3
    td = _cycle(n, seed=3)
    msg = MARSHAL[enc](td)
    p, hb = _expected(td)
    want_host, want_parsed = _counts(td)
    assert want_host >= 18 and want_parsed >= 2 * len(HAND)
    eng = _engine()
    for _ in range(2):   # cold (resources resolved on the host), then from the device table
        ob, got = _check(eng, msg, td, hb)
        flags_on, paths_on = _paths(ob.cols, got)
        assert ob.url_full_counts[1] == sum(
            len(q) for q, u in zip(paths_on, _urls(td)) if u is not None and q is not None and b"%" in _path_part(u))
        ob.close()
    # the same message with the option off: equal column contents, the parsed spans on the host pass
    eng.set_option("otlp_url_full", 0)
    ob = OtlpBatch(eng, msg)
    got = ob.download()
    _compare(ob.cols, hb.cols, got)
    flags_off, paths_off = _paths(ob.cols, got)
    np.testing.assert_array_equal(flags_off, flags_on)
    assert paths_off == paths_on
    assert ob.url_full_counts == (0, 0)
    assert ob.host_spans == want_host + want_parsed
    ob.close()
    eng.close()
    p.close()


def _urls(td):
    return [_chosen(sp["attributes"])[1] for rs in td["resourceSpans"] for ss in rs["scopeSpans"] for sp in ss["spans"]]


def _path_part(url):
    """the raw sub-range the seam reports for a url (b"" where it has none)"""
    from tests.test_url_full_option import parse
    b = url.encode()
    oc, off, ln, _ = parse(b)
    return b[off:off + ln] if oc >= 2 else b""


def _message_ending_in_url(td, url):
    """td's bytes with one more resource whose only span carries `url` as its
    last attribute, the last field of the span: the string ends on the message's
    final byte.  Returns (bytes, the tree they encode)."""
    kvd = _kv(FULL, url)
    sp = host.span(name="last", kind=3, trace_id="%032x" % 9, span_id="%016x" % 9, start=5, end=6)
    res = {"service.name": "svc-a", "k8s.pod.name": "pod-9"}
    span_b = gg.span(sp) + gg._len(9, gg.key_value(M)) + gg._len(9, gg.key_value(kvd))
    rs_b = gg._len(1, gg._attrs(1, host.attrs(res))) + gg._len(2, gg._len(1, b"") + gg._len(2, span_b))
    msg = gg.marshal_traces(td) + gg._len(1, rs_b)
    assert msg.endswith(url.encode())
    sp["attributes"] = [M, kvd]
    full = host.traces(*(copy.deepcopy(td["resourceSpans"]) + [host.resource_spans(res, [sp])]))
    return msg, full


@pytest.mark.gpu
@pytest.mark.parametrize("url", ["http://h/a/1234", "http://h/x%20y", "/p%4", "http://h/" + "s" * 40 + "%41", "%"])
def test_gpu_url_at_message_end(url):
    import torch
    from odigos_amd.batch import PinnedBuffer
    msg, td = _message_ending_in_url(_cycle(20, seed=5), url)
    p, hb = _expected(td)
    eng = _engine()
    pin = PinnedBuffer(msg)
    for m in (msg, pin):
        ob, got = _check(eng, m, td, hb)
        # TEMPLATE reads the path in 16-byte windows: the arena's slack holds
        eng.process_device(ob, native.STAGE_TEMPLATE)
        torch.cuda.synchronize()
        assert int(ob.out_numpy("device_status", np.uint32)[0]) == 0
        ob.close()
    pin.close()
    eng.close()
    p.close()


# ---------------------------------------------------------------------------
# 3. seams

def _seam_lists(n, decoded):
    """n spans with url.full alone; `decoded`: which of them hold an escape"""
    pick = {"none": set(), "first": {0}, "last": {n - 1}, "all": set(range(n))}[decoded]
    return [[M, _kv(FULL, "http://h/seg%%20%d/x" % k if k in pick else "http://h/seg%d/x" % k)] for k in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("decoded", ["none", "first", "last", "all"])
@pytest.mark.parametrize("n", [63, 64, 65, 1024, 1025])
def test_gpu_seams_wave_and_scan_tile(n, decoded):
    td = _tree(_seam_lists(n, decoded), seed=n)
    p, hb = _expected(td)
    eng = _engine()
    ob, got = _check(eng, gg.marshal_traces(td), td, hb, parsed=n, host_only=0)
    flags, paths = _paths(ob.cols, got)
    want = [("/seg %d/x" if "%20" in at[1]["value"]["stringValue"] else "/seg%d/x") % k
            for k, at in enumerate(_seam_lists(n, decoded))]
    assert [q.decode() for q in paths] == want
    assert ob.url_full_counts[1] == sum(len(w) for w in want if " " in w)
    assert ob.walk_info["span_kernel"] == 1
    ob.close()
    eng.close()
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65536, 65537])
def test_gpu_seams_span_stage_max(n):
    """kSpanStageMax: the LDS-staged span kernel up to 65536 spans, the HBM one
    above.  The message is 64 copies of a 1024-span one (and one more span); so
    are the expected paths."""
    from odigos_amd.batch import OtlpBatch
    lists = _seam_lists(1024, "none")
    for k in range(0, 1024, 5):
        lists[k] = [M, _kv(FULL, "http://h/five%%2F%d" % k)]
    for k in range(3, 1024, 97):
        lists[k] = [M, _kv(FULL, {"intValue": "3"})]
    td = _tree(lists, seed=2)
    p, hb = _expected(td)
    f1 = np.ctypeslib.as_array((C.c_uint8 * 1024).from_address(hb.cols.url_flags)).copy()
    r1 = np.ctypeslib.as_array((C.c_uint32 * 2048).from_address(hb.cols.path)).reshape(-1, 2)
    a1 = bytes((C.c_uint8 * hb.cols.arena_bytes).from_address(hb.cols.arena))
    p1 = [a1[o:o + l] if f & native.URL_PATH_MASK else None for f, (o, l) in zip(f1, r1)]
    host1, parsed1 = _counts(td)
    msg = gg.marshal_traces(td) * 64
    extra = []
    if n == 65537:
        tail = _tree([[M, _kv(FULL, "http://h/the%20tail")]], seed=9)
        msg += gg.marshal_traces(tail)
        extra = [b"/the tail"]
    eng = _engine()
    ob = OtlpBatch(eng, msg)
    assert ob.cols.n_spans == n and ob.walk_info["span_kernel"] == (1 if n == 65536 else 2)
    flags, paths = _paths(ob.cols, ob.download())
    np.testing.assert_array_equal(flags[:65536], np.tile(f1, 64))
    assert paths == p1 * 64 + extra
    assert ob.host_spans == 64 * host1 and ob.url_full_counts[0] == 64 * parsed1 + len(extra)
    assert ob.url_full_counts[1] == 64 * sum(len(q) for q in p1 if q and q.startswith(b"/five/")) + sum(map(len, extra))
    ob.close()
    eng.close()
    p.close()


@pytest.mark.gpu
def test_gpu_decoded_and_host_pass_regions_are_disjoint():
    """A decoded span and a host-pass span in one batch: the host pass's strings
    and the unescaped paths both follow the message bytes, in that order."""
    lists = [[M, _kv(FULL, "http://h/a%20b")], [M, _kv(FULL, {"intValue": "12345"})],
             [M, _kv("url.path", 77)], [M, _kv(FULL, "http://h/c%2Fd/e")], [M, _kv(FULL, "http://h/plain")]]
    td = _tree(lists)
    p, hb = _expected(td)
    eng = _engine()
    msg = gg.marshal_traces(td)
    ob, got = _check(eng, msg, td, hb, parsed=3, host_only=2)
    refs = got["path"].view(np.uint32).reshape(-1, 2)[:5]
    flags, paths = _paths(ob.cols, got)
    assert paths == [b"/a b", b"12345", b"77", b"/c/d/e", b"/plain"]
    assert ob.url_full_counts == (3, 10)
    L = len(msg)
    in_msg = [k for k in range(5) if refs[k][0] + refs[k][1] <= L]
    assert in_msg == [4]
    host_rng = [(int(refs[k][0]), int(refs[k][0] + refs[k][1])) for k in (1, 2)]
    dec_rng = [(int(refs[k][0]), int(refs[k][0] + refs[k][1])) for k in (0, 3)]
    assert min(a for a, _ in host_rng) >= L + 16 and max(b for _, b in host_rng) + 16 <= min(a for a, _ in dec_rng)
    assert dec_rng[0][1] == dec_rng[1][0] and dec_rng[1][1] == ob.cols.arena_bytes   # span order, packed
    np.testing.assert_array_equal(got["arena"][:L], np.frombuffer(msg, dtype=np.uint8))
    ob.close()
    eng.close()
    p.close()


@pytest.mark.gpu
def test_gpu_unescape_regrows_the_arena():
    """More unescaped bytes than the arena's reserve: the arena is regrown, and
    the message bytes have moved with it."""
    n = 300
    lists = [[M, _kv(FULL, LONG_URL[:-4] + "%04d" % k)] for k in range(n)]
    lists[7] = [M, _kv(FULL, {"doubleValue": 1.5})]
    td = _tree(lists)
    p, hb = _expected(td)
    eng = _engine()
    msg = gg.marshal_traces(td)
    ob, got = _check(eng, msg, td, hb, parsed=n - 1, host_only=1)
    assert ob.walk_info["arena_regrown"] == 1
    assert ob.url_full_counts[1] == (n - 1) * (4088 - 2 * 584) > (1 << 20) - len(msg)
    np.testing.assert_array_equal(got["arena"][:len(msg)], np.frombuffer(msg, dtype=np.uint8))
    assert ob.cols.arena_bytes >= len(msg) + ob.url_full_counts[1]
    ob.close()
    eng.close()
    p.close()


@pytest.mark.gpu
def test_gpu_sentinels_past_the_columns():
    """Nothing is written past the end of path and url_flags, the output columns
    the new kernels write: a released batch's buffers are reused by the next
    decode, so sentinels laid into the 16 bytes behind both columns after one
    decode must stand after the next decode of the same message."""
    import torch
    from odigos_amd.batch import OtlpBatch
    L = native.lib()
    sh = torch.cuda.current_stream().cuda_stream
    bw = C.c_double()
    for n in (65, 1025):
        td = _tree(_seam_lists(n, "all"), seed=n)
        msg = gg.marshal_traces(td)
        eng = _engine()
        ob = OtlpBatch(eng, msg)
        at = {"path": ob.cols.path + (8 * n + 15) // 16 * 16, "url_flags": ob.cols.url_flags + (n + 15) // 16 * 16}
        where = (ob.cols.path, ob.cols.url_flags)
        mark = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
        for a in at.values():   # inside the slab's slack: every part is followed by >= 16 bytes, parts start on 256
            native.check(L.osehost_stream_copy(C.c_void_p(a), C.c_void_p(mark.data_ptr()), 16, 1, C.c_void_p(sh), C.byref(bw)))
        torch.cuda.synchronize()
        ob.close()
        ob = OtlpBatch(eng, msg)
        assert (ob.cols.path, ob.cols.url_flags) == where and ob.url_full_counts[0] == n
        for name, a in at.items():
            back = torch.zeros(16, dtype=torch.uint8, device="cuda")
            native.check(L.osehost_stream_copy(C.c_void_p(back.data_ptr()), C.c_void_p(a), 16, 1, C.c_void_p(sh), C.byref(bw)))
            torch.cuda.synchronize()
            assert back.cpu().tolist() == [0xA5] * 16, (n, name)
        ob.close()
        eng.close()


# ---------------------------------------------------------------------------
# 4. end to end

def _mix(n, share=1.0, seed=0x0D16F0A3):
    from odigos_amd.batch import Generator
    return Generator("fused", seed=seed, n_spans=n, threads=2).otlp(2, url_full=share)


def _bench_cfg():
    from bench import NODE_KEYS
    from tests.workloads import c3_sampling_config
    return {"odigossampling": c3_sampling_config(), "odigosurltemplate": {},
            "odigostrafficmetrics": {"res_attributes_keys": NODE_KEYS}}


@pytest.mark.gpu
def test_gpu_end_to_end_bytes_equal_option_off():
    """decode -> SAMPLE|TEMPLATE|SIZE -> ose_otlp_encode on a 2,000-span mix whose
    HTTP spans all carry url.full alone: the output bytes and the traffic
    counters with the option on equal those with it off."""
    import torch
    from odigos_amd.batch import OtlpBatch
    msg = _mix(2000)
    assert msg.count(b"url.full") > 500 and msg.count(b"%C3%A9%20menu") > 20 and b"url.path" not in msg
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    outs = {}
    for on in (False, True):
        eng = _engine(on, _bench_cfg())
        ob = OtlpBatch(eng, msg)
        n, R, A = ob.cols.n_spans, ob.cols.n_resources, ob.cols.n_attrsets
        eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=SEED)
        torch.cuda.synchronize()
        assert int(ob.out_numpy("device_status", np.uint32)[0]) == 0
        outs[on] = dict(enc=ob.encode(st), host_spans=ob.host_spans, counts=ob.url_full_counts,
                        keep=ob.out_numpy("keep", n=n), url_out=ob.out_numpy("url_out", n=n),
                        res_bytes=ob.out_numpy("res_bytes", np.uint64, n=R),
                        attrset_bytes=ob.out_numpy("attrset_bytes", np.int64, n=A),
                        accepted=int(ob.out_numpy("accepted_spans", np.int64)[0]))
        ob.close()
        eng.close()
    off, on = outs[False], outs[True]
    assert on["counts"][0] == msg.count(b"url.full") and on["counts"][1] > 0 and off["counts"] == (0, 0)
    assert on["host_spans"] == 0 and off["host_spans"] == on["counts"][0]
    assert on["enc"] == off["enc"] and len(on["enc"][0][1]) > 100000
    for k in ("keep", "url_out", "res_bytes", "attrset_bytes"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    assert on["accepted"] == off["accepted"] > 0
    assert (on["url_out"] != 0).sum() > 500   # templated from the parsed paths


@pytest.mark.gpu
def test_gpu_pipeline_two_concurrent_requests():
    """The same through ose_otlp_pipeline (it decodes through the same decode()):
    two concurrent requests, joined into one batch, option on against off."""
    from odigos_amd.batch import OtlpPipeline
    msgs = [_mix(1000, seed=0x0D16F0A4), _mix(1000, seed=0x0D16F0A5)]
    res = {}
    for on in (False, True):
        eng = _engine(on, _bench_cfg())
        pipe = OtlpPipeline(eng)
        pipe.hold(2)   # both requests in one batch
        got, errs = [None, None], []

        def call(k):
            try:
                got[k] = pipe.consume(msgs[k], seed=SEED)
            except Exception as ex:   # pragma: no cover
                errs.append(repr(ex))

        th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        cnt = pipe.counters()
        res[on] = (got, {k: v for k, v in cnt.items() if k not in ("batch_ms",)})
        pipe.close()
        eng.close()
    assert res[True][0] == res[False][0] and all(len(g[0][1]) > 50000 for g in res[True][0])
    assert res[True][1] == res[False][1] and res[True][1]["largest_batch"] == 2


# ---------------------------------------------------------------------------
# 5. groupbytrace

@pytest.mark.gpu
def test_gpu_groupbytrace_keeps_the_paths():
    """ose_gbt_add_otlp -> ose_gbt_release_otlp on a batch with in-place and
    decoded paths (and a host-pass one): the released batch's path bytes equal
    the added ones, span by span."""
    from odigos_amd.batch import GroupByTrace, OtlpBatch
    lists = _seam_lists(130, "none")
    for k in range(0, 130, 3):
        lists[k] = [M, _kv(FULL, "http://h/dec%%20oded/%d" % k)]
    lists[64] = [M, _kv(FULL, {"intValue": "64"})]
    lists[65] = [M, _kv(FULL, ":error")]
    td = _tree(lists, seed=6)
    eng = _engine()
    ob = OtlpBatch(eng, gg.marshal_traces(td))
    assert ob.host_spans == 1 and ob.url_full_counts[0] == 129 and ob.url_full_counts[1] > 0
    got = ob.download()
    flags, paths = _paths(ob.cols, got)
    added = dict(zip(got["start_ns"].view(np.uint64)[:130].tolist(), zip(flags.tolist(), paths)))
    assert len(added) == 130 and sum(q is not None and b" " in q for q in paths) == 44
    S = 1_000_000_000
    g = GroupByTrace(eng, {"wait_duration": "1s"}, 1 << 12, 1 << 20)
    g.add_otlp(ob, 0)
    ob.close()
    rb, ntr = g.release_otlp(4 * S)
    assert ntr == 7 and rb.cols.n_spans == 130
    rgot = rb.download()
    rflags, rpaths = _paths(rb.cols, rgot)
    released = dict(zip(rgot["start_ns"].view(np.uint64)[:130].tolist(), zip(rflags.tolist(), rpaths)))
    assert released == added
    g.close()
    eng.close()
