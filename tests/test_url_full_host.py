"""The in-place url.Parse (odigos_amd/csrc/url_full.hpp) against
go_url_parse_path (urlparse.cpp): tests/url_full_check.cpp, a plain host
program built with AddressSanitizer and UBSan, compares the two on the
reference's url.full / http.url KAT strings, the hand-written list
(tests/url_full_cases.py), every string of length 0-4 over "a/:?#%@[]2 ." and
100,000 seeded grammar strings, of which each of the four outcomes is at
least 5% (the program asserts it): the outcome class, the sub-range and the
decoded bytes of every string."""
import re
import subprocess
from pathlib import Path

from tests.url_full_cases import HAND, kat_cases

ROOT = Path(__file__).resolve().parents[1]


def test_in_place_parser_matches_go_url_parse_path(tmp_path):
    exe = tmp_path / "url_full_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(ROOT / "tests" / "url_full_check.cpp"),
                    str(ROOT / "odigos_amd" / "csrc" / "urlparse.cpp")], check=True, timeout=300)
    kats = []
    for _, case in kat_cases():
        a = case["attrs"]
        kats.append((a["url.full"] if "url.full" in a else a["http.url"]).encode())
    assert len(kats) == 5
    strings = kats + HAND
    listed = tmp_path / "strings.hex"
    listed.write_text("".join(s.hex() + "\n" for s in strings))
    r = subprocess.run([str(exe), str(listed)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    m = re.search(r"listed (\d+), exhaustive (\d+), grammar (\d+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(strings), 22621, 100000)
