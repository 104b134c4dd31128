"""The engine option otlp_url_full and the host seam of its parser
(osehost_url_full_parse: url_full.hpp's host instantiation on one string).
The seam agrees with the reference's url.full / http.url KATs and with the
hand-written list's outcomes as go_url_parse_path gives them through the host
columniser; the option is accepted on an engine with the odigosurltemplate
section and OSE_EINVAL without it (an engine needs the device)."""
import ctypes as C

import pytest

from odigos_amd import host, native
from tests.url_full_cases import HAND, kat_cases

ERROR, EMPTY, IN_PLACE, DECODED = 0, 1, 2, 3


def parse(s: bytes):
    """(outcome, offset, length, the Path's bytes) of osehost_url_full_parse"""
    out = (C.c_uint32 * 4)()
    buf = C.create_string_buffer(len(s) + 1)
    native.check(native.lib().osehost_url_full_parse(s, len(s), out, C.cast(buf, C.c_void_p)))
    oc, off, ln, dec = list(out)
    path = {ERROR: None, EMPTY: b"", IN_PLACE: buf.raw[:ln], DECODED: buf.raw[:dec]}[oc]
    if oc == IN_PLACE:
        assert path == s[off:off + ln] and dec == 0
    if oc == DECODED:
        assert b"%" in s[off:off + ln] and dec == ln - 2 * s[off:off + ln].count(b"%")
    return oc, off, ln, path


def test_seam_agrees_with_the_kats():
    cases = kat_cases()
    assert [c["name"] for _, c in cases] == [
        "with url.full attribute", "with deprecated http.url attribute", "client span",
        "ignore client span with templated attribute", "invalid full url"]
    for _, case in cases:
        a = case["attrs"]
        oc, _, _, path = parse((a["url.full"] if "url.full" in a else a["http.url"]).encode())
        if case["name"] == "invalid full url":   # url.Parse fails: the span is left untouched
            assert oc == ERROR and case["expect_value"] is None
        else:
            assert (oc, path) == (IN_PLACE, b"/user/1234")


def test_seam_outcomes():
    assert parse(b"") == (EMPTY, 0, 0, b"")
    assert parse(b"*") == (IN_PLACE, 0, 1, b"*")
    assert parse(b"http://h") == (EMPTY, 8, 0, b"")
    assert parse(b"http:a")[0] == EMPTY                       # the opaque form
    assert parse(b"//u:p@h:80/a/b?q#f") == (IN_PLACE, 10, 4, b"/a/b")   # after "//u:p@h:80"
    assert parse(b"/a%20b") == (DECODED, 0, 6, b"/a b")
    assert parse(b"http://h/%e2%82%ac?x=%zz") == (DECODED, 8, 10, b"/\xe2\x82\xac")
    for bad in (b":a", b"1a:b", b"//h:80a", b"//[::1", b"/%zz", b"/p#%zz", b"/a\x7fb", b"//u^@h/", b"//h x/p"):
        assert parse(bad)[0] == ERROR, bad


def test_seam_agrees_with_the_columniser_on_the_hand_list():
    """The path the host columniser (go_url_parse_path) gives a span whose only
    source is url.full: the seam's Path, or no path where it reports an error."""
    spans = []
    for k, s in enumerate(HAND):
        sp = host.span(name="GET", kind=3, trace_id="%032x" % (k + 1), span_id="%016x" % (k + 1), start=1, end=2)
        sp["attributes"] = [{"key": "http.request.method", "value": {"stringValue": "GET"}},
                            {"key": "url.full", "value": {"stringValue": s.decode()}}]
        spans.append(sp)
    td = host.traces(host.resource_spans({"service.name": "svc-a"}, spans))
    p = host.Processor("pipeline", {"odigosurltemplate": {}, "odigostrafficmetrics": {}})
    hb = p.columnarize(td)
    n = hb.cols.n_spans
    assert n == len(HAND)
    flags = bytes((C.c_uint8 * n).from_address(hb.cols.url_flags))
    refs = list((C.c_uint32 * (2 * n)).from_address(hb.cols.path))
    arena = bytes((C.c_uint8 * max(1, hb.cols.arena_bytes)).from_address(hb.cols.arena))
    seen = set()
    for k, s in enumerate(HAND):
        oc, _, _, path = parse(s)
        seen.add(oc)
        if oc == ERROR:
            assert flags[k] & native.URL_PATH_MASK == 0, s
        else:
            assert flags[k] & native.URL_PATH_MASK == native.URL_PATH_RAW, s
            assert arena[refs[2 * k]:refs[2 * k] + refs[2 * k + 1]] == path, s
    assert seen == {ERROR, EMPTY, IN_PLACE, DECODED}
    p.close()


@pytest.mark.gpu
def test_gpu_option_needs_the_url_section():
    from odigos_amd.batch import Engine
    eng = Engine({"odigosurltemplate": {}, "odigostrafficmetrics": {}})
    for v in (1, 0, 1):
        eng.set_option("otlp_url_full", v)
    eng.close()
    plain = Engine({"odigostrafficmetrics": {}})
    for v in (1, 0):
        with pytest.raises(native.OseError) as e:
            plain.set_option("otlp_url_full", v)
        assert e.value.code == native.OSE_EINVAL and "odigosurltemplate" in str(e.value)
    plain.close()
