#!/usr/bin/env python3
"""Builds tests/fuzz/regex_nfa_san.cpp with ASan + UBSan, together with the
product's regex sources (regex_dfa.cpp, regex_nfa.cpp, unicode_tables.cpp),
and runs it over the patterns of tests/test_regex_nfa.py with the oracle's
answers (tests.oracle_lib.Regex) as the expected results.  A stand-alone CPU
program: the sanitized code is not loaded into Python and no device is used.
tests/test_regex_nfa.py runs it; by hand:

    python tests/fuzz/run_regex_nfa_san.py
"""
from __future__ import annotations

import random
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
CSRC = ROOT / "odigos_amd" / "csrc"

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
         "-pthread", f"-I{ROOT / 'include'}"]
SOURCES = [CSRC / "regex_dfa.cpp", CSRC / "regex_nfa.cpp", CSRC / "unicode_tables.cpp", Path(__file__).with_name("regex_nfa_san.cpp")]


def cases():
    from tests import test_regex_nfa as t
    from tests.test_regex import NON_ASCII, PATTERNS, _rand_strings
    from tests.test_regex_large import _ab_strings
    from tests.test_unicode_regex import UNI_PATTERNS, _strings
    rng = random.Random(0x5A17)
    for p in PATTERNS + sorted({p for p, _, _ in NON_ASCII}):
        yield p, _rand_strings(rng, 30) + [s for q, s, _ in NON_ASCII if q == p]
    for p in UNI_PATTERNS:
        yield p, [s.encode() for s in _strings(rng, 30)] + [b"\xff", b"a\xc3", b"\xe2\x82"]
    for p in t.OVERSIZE + [r"^(?:a|b)*a(?:a|b){1000}$"] + [r"^[ab]*a[ab]{%d}c$" % k for k in (28, 29, 30, 60, 61, 62)]:
        ss = [s.encode() for s in _ab_strings(rng, 30)]
        ss += [b"a" + b"b" * k + b"c" for k in (27, 28, 29, 30, 31, 59, 60, 61, 62, 63)]
        ss += [b"b" * 7 + b"a" + b"b" * k for k in (20, 21, 40, 1000)]
        ss += ["".join(rng.choice(t.CJK) for _ in range(k)).encode() for k in (1, 2, 5)] + [t.CJK[7].encode()[:2]]
        yield p, ss


def main() -> int:
    from tests.oracle_lib import Regex
    with tempfile.TemporaryDirectory() as d:
        exe, inp = Path(d) / "regex_nfa_san", Path(d) / "cases.bin"
        with open(inp, "wb") as f:
            for p, strings in cases():
                orc = Regex(p)
                pb = p.encode()
                f.write(struct.pack("<I", len(pb)) + pb + struct.pack("<I", len(strings)))
                for s in strings:
                    f.write(struct.pack("<I", len(s)) + s + (b"\1" if orc.match(s) else b"\0"))
        subprocess.run(["g++", *FLAGS, "-o", str(exe), *map(str, SOURCES)], check=True, timeout=900)
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
