#!/usr/bin/env python3
"""Builds tests/fuzz/condattr_san.cpp with ASan + UBSan and runs it over the
golden cases and seeded adversarial batches (tests/test_condattr.py), each
with the results of the Python restatement (tests/condattr_ref.py).  A
stand-alone CPU program: the sanitized code is not loaded into Python and no
device is used (the compiled config blob comes from the ordinary library's
osehost_condattr_blob).  Not collected by pytest; run it by hand after
changing odigos_amd/csrc/condattr_device.hpp:

    python tests/fuzz/run_condattr_san.py
"""
from __future__ import annotations

import ctypes as C
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def fnv(b: bytes) -> int:
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def blob_of(cfg) -> bytes:
    from odigos_amd import host, native
    from tests.condattr_ref import SECTION
    p, n = C.c_void_p(), C.c_size_t()
    native.check(native.lib().osehost_condattr_blob(host.dumps({SECTION: cfg}).encode(), C.byref(p), C.byref(n)))
    b = C.string_at(p.value, n.value)
    native.lib().osehost_free(p)
    return b


def write_batch(f, b, blob: bytes):
    from tests.test_condattr import _b
    want = b.want()
    n, U = b.n, len(b.targets)
    a = b.hb.arrays

    def blk(x: bytes):
        f.write(struct.pack("<Q", len(x)) + x)
    f.write(struct.pack("<4Q", n, b.R, b.S, b.arena_bytes))
    blk(blob)
    blk(b.arena)   # exactly arena_bytes: no slack
    blk(a["scope"][:n].tobytes())
    blk(a["scope_resource"][:b.S].tobytes())
    blk(a["scope_name"][:b.S].tobytes())
    for name, m in (("span_has", n), ("span_val", n), ("span_kv_size", n), ("scope_has", b.S), ("scope_val", b.S),
                    ("res_has", b.R), ("res_val", b.R)):
        blk(a[name][:b.K * m].tobytes())
    blk(a["span_size"][:n].tobytes())
    put = np.zeros(U * n, dtype=np.uint8)
    hs = np.zeros(U * n, dtype=np.uint32)
    ln = np.zeros(U * n, dtype=np.uint32)
    for u, t in enumerate(b.targets):
        for i in range(n):
            w = want[i][0].get(t)
            if w is not None:
                wb = _b(w)
                put[u * n + i], hs[u * n + i], ln[u * n + i] = 1, fnv(wb), len(wb)
    blk(put.tobytes())
    blk(hs.tobytes())
    blk(ln.tobytes())
    from tests import otlp_gogo as gg
    blk(np.array([len(gg.span(w[2])) for w in want], dtype=np.uint32).tobytes())


def main() -> int:
    from tests import test_condattr as tc
    with tempfile.TemporaryDirectory() as d:
        exe, inp = Path(d) / "condattr_san", Path(d) / "cases.bin"
        with open(inp, "wb") as f:
            for cfg, c in tc.kat_cases():
                write_batch(f, tc.Batch(cfg, tc.kat_tree(c)), blob_of(cfg))
            adv = blob_of(tc.adv_config())
            write_batch(f, tc.adversarial()[0], adv)
            for seed in range(4):
                write_batch(f, tc.Batch(tc.adv_config(), tc.adv_tree(0x5A0 + seed, 5000, 11 + seed, 90), align=bool(seed & 1)), adv)
            cfg, td = tc._size_tree()
            write_batch(f, tc.Batch(cfg, td), blob_of(cfg))
        subprocess.run(["g++", *FLAGS, "-o", str(exe), str(Path(__file__).with_name("condattr_san.cpp"))], check=True, timeout=600)
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
