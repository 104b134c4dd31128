#!/usr/bin/env python3
"""Builds tests/fuzz/sqlop_san.cpp with ASan + UBSan and runs it over the
golden cases and 50,000 seeded random strings, each with the code the Python
restatement (tests/sqlop_ref.py) gives.  A stand-alone CPU program: nothing is
loaded into Python and no device is used.  Not collected by pytest; run it by
hand after changing odigos_amd/csrc/sqlop_device.hpp:

    python tests/fuzz/run_sqlop_san.py
"""
from __future__ import annotations

import random
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def main() -> int:
    from tests import sqlop_ref as ref
    from tests.test_sqlop import golden_queries, rand_query
    cases = [(q, ref.CODES[w]) for q, w in golden_queries()]
    rng = random.Random(0x5A17)
    for _ in range(50_000):
        q = rand_query(rng)
        cases.append((q, ref.code(q)))
    with tempfile.TemporaryDirectory() as d:
        exe, inp = Path(d) / "sqlop_san", Path(d) / "cases.txt"
        inp.write_text("".join(f"{q.hex() or '-'} {c}\n" for q, c in cases))
        subprocess.run(["g++", *FLAGS, "-o", str(exe), str(Path(__file__).with_name("sqlop_san.cpp"))], check=True, timeout=600)
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
