"""The hand-written url.full strings shared by the CPU check of the in-place
parser (tests/test_url_full_host.py, tests/url_full_check.cpp) and the GPU
case table (tests/test_otlp_url_full.py): at least one string for every
``return false`` of odigos_amd/csrc/urlparse.cpp and for every success branch."""
import json
from pathlib import Path

KATS = json.loads((Path(__file__).parent / "golden" / "url_kats.json").read_text())


def kat_cases():
    """The reference's URL KATs whose path source is url.full / http.url."""
    out = []
    for group in KATS["groups"]:
        for case in group["cases"]:
            a = case["attrs"]
            if ("url.full" in a or "http.url" in a) and "url.path" not in a and "http.target" not in a:
                out.append((group, case))
    return out


HAND = [
    # Parse: "*", empty forms, the '#' and '?' cuts
    b"*", b"", b"#", b"?", b"a?", b"a??", b"*#f", b"*?q", b"/p?q?r", b"/p?",
    # getScheme, the opaque form, the first segment's colon
    b"http:", b"http:a", b":a", b"1a:b", b"a:b/c", b"a/b:c", b"a+b-c.d:/p", b"http:/p", b"a_b:c", b"./a:b",
    # the authority rule
    b"//h", b"///p", b"http:///p", b"//h/p", b"http://h", b"http://h/", b"//h?q", b"http://h#f",
    # parseHost: ports, brackets, zones
    b"//h:80a", b"//h:", b"//h:80/p", b"//[::1]:9/p", b"//[::1", b"//[::1]x/p", b"//[::1]:9a/p", b"//[::1]/p",
    b"//[fe80::1%25en0]/p", b"//[fe80::1%25e%2fn]/p", b"//[fe80::1%25e%20n]/p", b"//[fe80::1%25e%41n]/p",
    b"//[fe80%3a:1%25en0]/p", b"//[fe80::1%25en0]:8%30/p", b"//[fe80::1%25e n]/p", b"//[a%25]/p", b"//[%2]/p",
    # host unescape
    b"//h%41/p", b"//h%25/p", b"//h x/p", b"//h%c3%a9/p", b"//h%zz/p", b"//h%4/p", b"//h\xc3\xa9/p", b"//h\"<>/p",
    b"//h^/p", b"//a:b:80/p",
    # userinfo
    b"//u:p@h/p", b"//u%4@h/", b"//u^@h/", b"//u@h/p", b"//u%41:p%42@h/p", b"//u:p%4@h/", b"//a@b@h/p", b"//u\xc3\xa9@h/p",
    b"//@h/p", b"//u:@h/p", b"//u%zz:p@h/p",
    # setPath
    b"/a%20b", b"/%zz", b"/a%4", b"/%", b"/a%4g", b"/%41%42%43", b"/a/%2F/b", b"/a%2fb?x=%zz", b"/%00", b"/%7F%ff",
    b"a%20b", b"http://h/a%20b?q#f", b"//h/%e2%82%ac",
    # setFragment
    b"/p#%zz", b"/p#a#b", b"/p#", b"/p#%41", b"/p#%4", b"#%", b"http:a#%zz",
    # control characters, UTF-8
    b"/a\x7fb", b"/a\x1fb", b"/a#\x1f", b"/a#\x7f", b"/\xe2\x82\xac/\xc3\xa9", b"/a\tb", b"http://h/\x00",
    # the reference's KAT strings
    b"http://example.com/user/1234?name=John", b"invalidurl/#@%@##%$@%@",
]
