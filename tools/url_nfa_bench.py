#!/usr/bin/env python3
"""The price of the URL stage's NFA route (url_nfa_plan_kernel /
url_nfa_emit_kernel: every span planned and written per lane, regexps run as
NFA programs) against the ordinary route, on one device batch.

Batch: --spans seeded paths of tests/test_regex_large.py's mix (1-4 segments
over {a, b} of 1-29 bytes, a fifth of the paths "/s/<seg>/<seg>").
  1. LARGE_URL_CFG (its regexps have DFAs): engine option "url_regex_nfa" off,
     then on, in one process: the median of --calls TEMPLATE calls between two
     device events after --warmup calls, their ratio, and the per-kernel times
     of the engine's own events (ose_profile_read) over further calls.
  2. config A of tests/test_url_nfa.py (a state-blowup custom id and a
     class-count rule: NFA programs without the option) on the same batch.
Both results are checked against each other (1) or the route witness (2)
before anything is timed.  Writes one JSON object to --out (merged into the
file when it exists).  A record, not a gate.
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def paths(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        segs = ["".join(rng.choice("ab") for _ in range(rng.randrange(1, 30))) for _ in range(rng.randrange(1, 5))]
        if rng.random() < 0.2:
            segs = ["s"] + segs[:2]
        out.append(("/" + "/".join(segs)).encode())
    return out


def timed(eng, db, stage, calls, warmup):
    import torch
    for _ in range(warmup):
        eng.process_device(db, stage)
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.process_device(db, stage)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    eng.profile(True)
    for _ in range(5):
        eng.process_device(db, stage)
    torch.cuda.synchronize()
    prof = {k: round(v["ms"] / v["launches"], 4) for k, v in eng.profile_read().items()}
    eng.profile(False)
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "kernels_ms": prof}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spans", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "url_nfa_bench.json"))
    args = ap.parse_args()
    import torch
    from odigos_amd import native
    from odigos_amd.batch import DeviceBatch, Engine
    from tests.test_regex_large import LARGE_URL_CFG
    from tests.test_unicode_regex import _cols_from_paths
    from tests.test_url_nfa import CFG_A

    cols, _keep = _cols_from_paths(paths(args.spans, 0x0D1600E1))
    n, groups = cols.n_spans, (cols.n_spans + 63) // 64
    st = native.STAGE_TEMPLATE
    res = {"spans": n, "arena_bytes": int(cols.arena_bytes), "calls": args.calls, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}

    eng = Engine({"odigosurltemplate": LARGE_URL_CFG})
    eng.set_option("url_path_counts", 1)
    db = DeviceBatch(cols)
    outs = {}
    for on in (0, 1):
        eng.set_option("url_regex_nfa", on)
        eng.process_device(db, st)
        torch.cuda.synchronize()
        assert eng.path_counts()["url_nfa"] == (groups if on else 0)
        used = db.used()
        outs[on] = (db.out_numpy("url_out", n=n).copy(), used, db.out_numpy("tmpl_arena", n=used).copy())
    assert outs[0][1] == outs[1][1] and np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][2], outs[1][2])
    eng.set_option("url_regex_nfa", 0)
    off = timed(eng, db, st, args.calls, args.warmup)
    eng.set_option("url_regex_nfa", 1)
    on = timed(eng, db, st, args.calls, args.warmup)
    res["large_url_cfg"] = {"dfa_route": off, "nfa_route": on, "nfa_over_dfa": round(on["ms_median"] / off["ms_median"], 2),
                            "nfa_spans_per_s": round(n / on["ms_median"] * 1e3), "dfa_spans_per_s": round(n / off["ms_median"] * 1e3)}
    eng.close()

    eng = Engine({"odigosurltemplate": CFG_A})
    eng.set_option("url_path_counts", 1)
    eng.process_device(db, st)
    torch.cuda.synchronize()
    assert eng.path_counts()["url_nfa"] == groups
    a = timed(eng, db, st, args.calls, args.warmup)
    a["spans_per_s"] = round(n / a["ms_median"] * 1e3)
    res["config_a"] = a
    eng.close()

    out = Path(args.out)
    doc = json.loads(out.read_text()) if out.exists() else {}
    doc["route_price"] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
