"""The NFA route of odigosurltemplate regexps (regex_nfa.hpp,
regex_nfa_device.hpp): a regexp whose DFA passes the device bounds (about two
million states, 256 MiB of transitions, 255 rune classes) is held as an NFA
program and matched by a bit-set simulation.  osehost_regex_nfa_match builds
exactly the tables the URL blob gets and runs the step the kernels compile;
here it is checked against the oracle's Pike VM (tests.oracle_lib.Regex) and,
wherever a DFA exists, against the DFA route.  The GPU side is
tests/test_url_nfa.py."""
import ctypes as C
import json
import random
import subprocess
import sys
import zlib
from pathlib import Path

import pytest

from odigos_amd import native
from tests.oracle_lib import Regex
from tests.test_regex import NON_ASCII, PATTERNS, _case_id, _rand_strings
from tests.test_regex_large import BIG, LARGE_URL_CFG, _ab_strings
from tests.test_unicode_regex import UNI_PATTERNS, _strings

ROOT = Path(__file__).resolve().parent.parent

# 300 distinct CJK literals alternated: more than 255 rune classes
CJK = [chr(0x4E00 + 7 * k) for k in range(300)]
CJK_ALT = "(?:" + "|".join(CJK) + ")"


def _nfa(pattern, s: bytes):
    r = native.lib().osehost_regex_nfa_match(pattern.encode(), s, len(s))
    assert r >= 0, (pattern, r, native.lib().osehost_last_error())
    return bool(r)


def _check(pattern, strings, dfa=None):
    """dfa: how many of the strings also go to the DFA seam (all by default;
    it compiles the DFA on every call, which takes seconds where the subset
    construction runs into its cap)."""
    orc = Regex(pattern)
    L = native.lib()
    for k, s in enumerate(strings):
        got = _nfa(pattern, s)
        assert got == orc.match(s), (pattern, s)
        if dfa is None or k < dfa:
            d = L.osehost_regex_match(pattern.encode(), s, len(s))
            if d >= 0:
                assert got == bool(d), (pattern, s)


def _seed(pattern):
    return zlib.crc32(pattern.encode())


@pytest.mark.parametrize("pattern", PATTERNS + sorted({p for p, _, _ in NON_ASCII} - set(PATTERNS)), ids=_case_id)
def test_nfa_vs_oracle_ascii_corpus(pattern):
    strings = _rand_strings(random.Random(_seed(pattern)), 200) + [s for p, s, _ in NON_ASCII if p == pattern]
    _check(pattern, strings)


@pytest.mark.parametrize("pattern,s,expect", NON_ASCII)
def test_nfa_utf8_semantics(pattern, s, expect):
    assert _nfa(pattern, s) == expect


@pytest.mark.parametrize("pattern", UNI_PATTERNS)
def test_nfa_vs_oracle_unicode_corpus(pattern):
    strings = [s.encode() for s in _strings(random.Random(_seed(pattern)), 200)]
    strings += [b"\xff", b"a\xc3", b"\xe2\x82", b"\xce\xb1\xff"]
    _check(pattern, strings)


def _ab(k):
    return r"(a|b)*a(a|b){%d}" % k


OVERSIZE = BIG + [_ab(20), _ab(21), _ab(40), r"\b(a|b)*a(a|b){21}\b", "^" + CJK_ALT + "+$", CJK_ALT,
                  r"(?m)^(?:a|b)*a(?:a|b){21}$"]


@pytest.mark.parametrize("pattern", OVERSIZE, ids=lambda p: p if len(p) < 40 else p[:12] + "..." + p[-8:])
def test_nfa_vs_oracle_oversize(pattern):
    rng = random.Random(_seed(pattern))
    strings = [s.encode() for s in _ab_strings(rng, 200)]
    for _ in range(60):   # long enough to reach a{21} / a{40}, with the deciding 'a' at every distance
        k = rng.randrange(15, 48)
        body = "".join(rng.choice("ab") for _ in range(rng.randrange(0, 10))) + "a" + "".join(rng.choice("ab") for _ in range(k))
        strings.append((rng.choice(["", " ", "x ", "\n"]) + body + rng.choice(["", " ", " y", "\n", "\nab"])).encode())
    for _ in range(60):
        segs = [rng.choice(CJK + [chr(0x4E01), "a", "é"]) for _ in range(rng.randrange(0, 5))]
        strings.append("".join(segs).encode())
    strings += [CJK[0].encode()[:2], CJK[299].encode(), (CJK[299] * 3).encode(), CJK[5].encode() + b"\xe4\xb8"]
    _check(pattern, strings, dfa=40 if pattern in BIG else 0)


def test_nfa_go_largest_repeat():
    # 1000 is Go's largest repeat count: about 2,000 rune instructions, 63 state words
    pattern = r"^(?:a|b)*a(?:a|b){1000}$"
    assert native.lib().osehost_regex_nfa_size(pattern.encode()) == 2003
    rng = random.Random(1000)
    strings = []
    for lead in (0, 1, 37):
        tail = "".join(rng.choice("ab") for _ in range(1000))
        strings += [("b" * lead + "a" + tail).encode(), ("b" * lead + "b" + tail).encode(), ("b" * lead + "a" + tail[1:]).encode(),
                    ("b" * lead + "a" + tail + "c").encode()]
    _check(pattern, strings + [b"", b"a"], dfa=0)


@pytest.mark.parametrize("m", [31, 32, 33, 63, 64, 65])
def test_nfa_bit_set_word_edges(m):
    # the rune-instruction count from the compiler itself; the last instruction
    # (the closing 'c') is the bit at the word's edge
    L = native.lib()
    k = next(k for k in range(1, 80) if L.osehost_regex_nfa_size((r"^[ab]*a[ab]{%d}c$" % k).encode()) == m)
    pattern = r"^[ab]*a[ab]{%d}c$" % k
    strings = [b"a" + b"b" * k + b"c", b"a" + b"b" * (k - 1) + b"c", b"bab" + b"a" * k + b"c", b"a" + b"b" * k, b"a" + b"b" * k + b"cc",
               b"a" + b"b" * (k + 1) + b"c", b"b" * (k + 1) + b"c"]
    assert _nfa(pattern, strings[0]) and not _nfa(pattern, strings[1])
    _check(pattern, strings, dfa=0)   # (no DFA within the bounds from k = 21 on)
    un = r"[ab]*a[ab]{%d}c" % k   # unanchored: the start re-injected at every rune
    _check(un, [b"xx" + s + b"yy" for s in strings], dfa=0)


def _create(url_cfg):
    h = C.c_void_p()
    rc = native.lib().ose_engine_create(json.dumps({"odigosurltemplate": url_cfg}).encode(), C.byref(h))
    err = native.last_error()
    if rc == 0:
        native.lib().ose_engine_destroy(h)
    return rc, err


REFUSED_BEFORE = {
    "custom-id-states": {"custom_ids": [{"regexp": r"^(?:a|b)*a(?:a|b){21}$", "template_name": "ab"}]},
    "rule-states": {"templatization_rules": [r"/s/{seq:^[ab]*b[ab]{21}$}/{rest}"]},
    "custom-id-classes": {"custom_ids": [{"regexp": "^" + CJK_ALT + "$", "template_name": "han"}]},
}


@pytest.mark.parametrize("name", list(REFUSED_BEFORE))
def test_engine_accepts_regexps_past_the_dfa_bound(name):
    # (the two state-blowup configs take seconds: the subset construction runs into its cap first)
    rc, err = _create(REFUSED_BEFORE[name])
    assert rc in (0, native.OSE_EDEVICE), (rc, err)


def test_engine_still_refuses_past_the_nfa_bound():
    # more than 100,000 instructions: the parser's own bound, which the NFA route shares
    rc, err = _create({"custom_ids": [{"regexp": r"^(?:(?:(?:a?){40}){40}){40}$", "template_name": "x"}]})
    assert rc == native.OSE_ENOTSUP, (rc, err)
    assert "NFA bound" in str(err), err
    assert native.lib().osehost_regex_nfa_match(r"(?:(?:(?:a?){40}){40}){40}".encode(), b"", 0) == -2


def test_nfa_seam_syntax_errors():
    # (the DFA seam's own answers, -2 included, are pinned by tests/test_regex.py and tests/test_regex_large.py)
    L = native.lib()
    assert L.osehost_regex_nfa_match(b"(", b"", 0) == -1
    assert L.osehost_regex_nfa_size(b"a**") == -1


def _blob(url_cfg, force):
    h, nb, nn = C.c_uint64(), C.c_uint64(), C.c_uint32()
    rc = native.lib().osehost_url_blob_hash(json.dumps({"odigosurltemplate": url_cfg}).encode(), int(force), C.byref(h),
                                            C.byref(nb), C.byref(nn))
    assert rc == 0, native.last_error()
    return h.value, nb.value, nn.value


def test_blob_of_a_dfa_config_is_what_it_was():
    # FNV-1a and size of LARGE_URL_CFG's device tables as the build before the
    # NFA route made them: the two new header fields (n_nfa, nfa_off) lie in
    # what was the header's padding and are zero without an NFA program
    assert _blob(LARGE_URL_CFG, False) == (0x38385327AB6A6D99, 135984, 0)
    forced = _blob(LARGE_URL_CFG, True)
    assert forced[2] == 2 and forced[1] < 16384   # both regexps as NFA programs: a few KB
    assert _blob({}, False)[2] == 0 and _blob({}, True)[2] == 0
    assert _blob(REFUSED_BEFORE["custom-id-classes"], False)[2] == 1


def test_sanitizer_driver():
    # ASan + UBSan over table build + match in a stand-alone program (no Python in the process)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "fuzz" / "run_regex_nfa_san.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mismatches 0" in r.stdout
