#!/usr/bin/env python3
"""Times the CONDATTR stage (odigosconditionalattributes: condattr_scope_kernel
+ condattr_span_kernel) alone, with the shipped category-attributes profile.

A seeded batch is built on the device: 10M spans by default in --scopes scopes
(50,000: 200 spans per scope, what a node collector's batches of a few hundred
spans per instrumentation library add up to) of --resources resources (5,000).
Three scopes in four carry one of the profile's 269 scope names, the rest a
name outside it; half the spans have http.request.method or http.method, a
few already carry odigos.category.  After a warm-up the stage is timed over
--calls calls of ose_condattr_process_device, each between two device events.

Prints one JSON line (and writes it to --out):
  ms_per_call          median of the per-call device times (mean, min, max beside it)
  spans_per_s          n_spans over the median
  algorithmic_bytes    from the shapes: per span scope (4) + the scratch word
                       of its scope (4) + per target the src byte written (1),
                       span_has (1) and, where the stage put, val (8); per
                       from_field key span_has (1) and span_val (8) where the
                       span has it; span_size (4) + span_kv_size of replaced
                       targets + span_size_out (4); per scope its name ref (8),
                       resource (4), the name's 16-byte arena chunks and the
                       scratch words written
  algorithmic_gbs      those bytes over the median time
  stream_copy_gbs      measured here with osehost_stream_copy (read + written bytes)
  frac_of_stream_copy  algorithmic_gbs over it
A sample of the results is checked against the host-compiled steps
(osehost_condattr_span) before anything is timed.  A record, not a gate.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

SECTION = "odigosconditionalattributes"


def profile_config() -> dict:
    p = json.loads((ROOT / "tests" / "golden" / "category_attributes_profile.json").read_text())
    rules = [{"field_to_check": r["field_to_check"],
              "new_attribute_value_configurations": {v: r["action_lists"][k] for v, k in r["values"].items()}}
             for r in p["rules"]]
    return {"global_default": p["global_default"], "rules": rules}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spans", type=int, default=10_000_000)
    ap.add_argument("--scopes", type=int, default=50_000)
    ap.add_argument("--resources", type=int, default=5_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0xCA7B)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from odigos_amd import host, native
    from odigos_amd.batch import Engine

    if not torch.cuda.is_available():
        print("condattr_bench: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = "cuda"
    cfg = profile_config()
    eng = Engine({SECTION: cfg})
    L = native.lib()
    keys = eng.condattr_keys()
    K, U = len(keys), eng.condattr_info().n_targets
    kidx = {k: i for i, (k, _) in enumerate(keys)}
    n, S, R = args.spans, args.scopes, args.resources
    rng = np.random.default_rng(args.seed)

    # the arena: the profile's scope names, 64 names outside it, the methods, "mine"
    names = [v.encode() for v in cfg["rules"][0]["new_attribute_value_configurations"]]
    outside = [b"unknown.library.%d" % k for k in range(64)]
    methods = [b"GET", b"POST", b"PUT", b"DELETE"]
    strs = names + outside + methods + [b"mine"]
    offs, buf = [], bytearray()
    for s in strs:
        offs.append(len(buf))
        buf += s
    arena_bytes = len(buf)
    arena = np.zeros((arena_bytes + 15) // 16 * 16 + 32, dtype=np.uint8)
    arena[:arena_bytes] = np.frombuffer(bytes(buf), dtype=np.uint8)
    ref_of = np.array([[o, len(s)] for o, s in zip(offs, strs)], dtype=np.uint32)

    in_profile = rng.random(S) < 0.75
    name_id = np.where(in_profile, rng.integers(0, len(names), S), len(names) + rng.integers(0, len(outside), S))
    scope_name = ref_of[name_id]
    scope_resource = (np.arange(S, dtype=np.uint64) * R // S).astype(np.uint32)
    scope = (np.arange(n, dtype=np.uint64) * S // n).astype(np.uint32)
    span_has = np.zeros((K, n), dtype=np.uint8)
    span_val = np.zeros((K, n, 2), dtype=np.uint32)
    span_kv = np.zeros((K, n), dtype=np.uint32)
    x = rng.random(n)
    m_id = len(names) + len(outside) + rng.integers(0, len(methods), n)
    for key, sel in ((b"http.request.method", x < 0.35), (b"http.method", (x >= 0.35) & (x < 0.5))):
        k = kidx[key]
        span_has[k] = sel
        span_val[k][sel] = ref_of[m_id[sel]]
    mine = rng.random(n) < 0.02
    kc = kidx[b"odigos.category"]
    span_has[kc] = mine
    span_val[kc][mine] = ref_of[len(strs) - 1]
    span_kv[kc][mine] = 2 + (2 + 15) + (2 + 2 + 4)   # framed KeyValue{"odigos.category": "mine"}
    span_size = rng.integers(180, 900, n).astype(np.uint32)
    zeros = lambda *shape: np.zeros(shape, dtype=np.uint8)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    t = {"arena": up(arena), "scope": up(scope), "scope_resource": up(scope_resource), "scope_name": up(scope_name),
         "span_has": up(span_has), "span_val": up(span_val), "span_kv_size": up(span_kv),
         "scope_has": up(zeros(K * S)), "scope_val": up(zeros(8 * K * S)), "res_has": up(zeros(K * R)),
         "res_val": up(zeros(8 * K * R)), "span_size": up(span_size)}
    cols = native.CondAttrColumns()
    cols.n_spans, cols.n_resources, cols.n_scopes, cols.arena_bytes = n, R, S, arena_bytes
    for k, v in t.items():
        setattr(cols, k, v.data_ptr())
    words = int(L.ose_condattr_scratch_words(eng.h, S))
    o = {"src": torch.zeros(U * n, dtype=torch.uint8, device=dev), "val": torch.zeros(8 * U * n, dtype=torch.uint8, device=dev),
         "span_size_out": torch.zeros(4 * n, dtype=torch.uint8, device=dev),
         "scratch": torch.zeros(4 * words, dtype=torch.uint8, device=dev)}
    outs = native.CondAttrOutputs()
    for k, v in o.items():
        setattr(outs, k, v.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        native.check(L.ose_condattr_process_device(eng.h, C.byref(cols), C.byref(outs), C.c_void_p(stream)))

    call()
    torch.cuda.synchronize()
    src = o["src"].cpu().numpy().reshape(U, n)
    val = o["val"].cpu().numpy().view(np.uint32).reshape(U, n, 2)
    size_out = o["span_size_out"].cpu().numpy().view(np.uint32)
    # a sample against the host-compiled steps: the first spans of 40 scopes
    pick = np.concatenate([np.arange(s * (n // S), min(n, s * (n // S) + 50)) for s in range(0, S, max(1, S // 40))])
    hc = native.CondAttrColumns()
    hc.n_spans, hc.n_resources, hc.n_scopes, hc.arena_bytes = len(pick), R, S, arena_bytes
    harr = {"arena": arena, "scope": scope[pick], "scope_resource": scope_resource, "scope_name": scope_name,
            "span_has": span_has[:, pick], "span_val": span_val[:, pick], "span_kv_size": span_kv[:, pick],
            "scope_has": zeros(K * S), "scope_val": zeros(8 * K * S), "res_has": zeros(K * R), "res_val": zeros(8 * K * R),
            "span_size": span_size[pick]}
    harr = {k: np.ascontiguousarray(v) for k, v in harr.items()}
    for k, v in harr.items():
        setattr(hc, k, v.ctypes.data)
    hs, hv, hz = np.zeros(U * len(pick), np.uint8), np.zeros((U * len(pick), 2), np.uint32), np.zeros(len(pick), np.uint32)
    ho = native.CondAttrOutputs()
    ho.src, ho.val, ho.span_size_out = hs.ctypes.data, hv.ctypes.data, hz.ctypes.data
    native.check(L.osehost_condattr_span(host.dumps({SECTION: cfg}).encode(), C.byref(hc), C.byref(ho)))
    if not np.array_equal(hs.reshape(U, -1), src[:, pick]) or not np.array_equal(hz, size_out[pick]):
        raise SystemExit("condattr_bench: the kernel and the host steps differ on the sample")
    put = hs.reshape(U, -1) != native.CA_KEEP
    if not np.array_equal(hv.reshape(U, -1, 2)[put], val[:, pick][put]):
        raise SystemExit("condattr_bench: the kernel and the host steps differ on the sample's values")
    hist = {name: int((src == code).sum()) for name, code in (("keep", 0), ("arena", 1), ("config", 2))}

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    med = float(np.median(ms))

    n_put = int((src != 0).sum())
    from_keys = [kidx[b"http.request.method"], kidx[b"http.method"]]
    n_from = int(span_has[from_keys].sum())
    name_chunks = int((((scope_name[:, 0] & 15) + scope_name[:, 1] + 15) // 16).sum())
    alg = (n * (4 + 4 + 4 + 4) + U * n * 2 + 8 * n_put + 2 * n + 8 * n_from + 4 * int(mine.sum())
           + S * (8 + 4 + 4 * (1 + U)) + 16 * name_chunks)
    bw = C.c_double()
    a_ = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    b_ = torch.empty_like(a_)
    native.check(L.osehost_stream_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), 10, C.c_void_p(stream), C.byref(bw)))
    gbs = alg / (med * 1e-3) / 1e9
    out = {
        "tool": "tools/condattr_bench.py", "kernels": ["condattr_scope_kernel", "condattr_span_kernel"],
        "device": torch.cuda.get_device_name(0), "config": "tests/golden/category_attributes_profile.json",
        "n_spans": n, "n_scopes": S, "n_resources": R, "n_keys": K, "n_targets": U,
        "scopes_in_profile": int(in_profile.sum()), "src_histogram": hist,
        "calls": args.calls, "warmup": args.warmup, "timing": "device events around each call",
        "ms_per_call": med, "ms_mean": float(ms.mean()), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
        "spans_per_s": n / (med * 1e-3), "algorithmic_bytes": alg, "algorithmic_gbs": gbs,
        "stream_copy_gbs": bw.value, "frac_of_stream_copy": gbs / bw.value if bw.value else None,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
