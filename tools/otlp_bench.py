"""OTLP protobuf ingest timed end to end on one GPU: a
serialized TracesData in host memory (the C4 mix as an HTTP instrumentation
would send it, odigos_amd/csrc/gen_otlp.cpp) → ose_otlp_decode (structural
walk on the host, H2D, the span decoder, the host pass) → the three stages
on the decoded columns.  PCIe-inclusive by construction: not a bench.py
`value`.  One JSON line on stdout and in --out.

Legs: decode from pinned memory (ose_host_alloc: a receiver reading into
engine buffers), decode from pageable memory, the stages after it, and the
output side (ose_otlp_encode: decisions D2H, routing to data-stream
pipelines, one TracesData per pipeline).
The span decoder's roofline: message bytes read + columns written per
launch over its HIP-event time, against 8 TB/s.

--sqlop: the query-operation-detector profile on the same path: the engine
has the odigossqldboperationprocessor section and the engine option
otlp_sqlop on, the stages include SQLOP, and a third of the spans carry a
db.query.text (as in tools/sqlop_bench.py).  The decoder's second pass
(otlp_sqlop_kernel) is reported as a row of its own, with its roofline.

--condattr: the node collector's pipeline instead: an engine
with the shipped category-attributes profile
(tests/golden/category_attributes_profile.json) and odigostrafficmetrics only,
engine option otlp_condattr on; the resources' scope names are drawn from the
profile's 269 values and 30 names outside them.  ose_otlp_decode ->
ose_condattr_process_device on the decoded columns -> SIZE with span_size_out
-> ose_otlp_encode_condattr, each leg timed; otlp_condattr_kernel by HIP
events, its bytes (the message read again, span_ref and the host flag read,
the hits' columns written) against osehost_stream_copy in the same process;
the same at 8192-span requests (one caller with each leg timed; 8 callers for
whole-job spans/s only: their legs overlap and are not reported).  Writes
profiles/otlp_condattr_bench.json unless --out names another file; an
"option_off_ab" entry already in that file (the parent-commit comparison,
made by a job of its own) is kept.  A record, not a gate.

--url-full SHARE: the engine option otlp_url_full off against on, on one
build and interleaved call by call.  That share of the mix's HTTP spans
carries url.full alone (a scheme, a host, the same path, a query; a tenth of
them with an escaped segment more), so with the option off they take the
decoder's host pass.  8192-span requests (decode -> stages -> encode) from 1
caller (each leg and the decode phases timed) and from 8 callers (whole-job
spans/s), and one --spans message (default 1M here).  The entry of this SHARE
in profiles/otlp_url_full_bench.json is replaced, the others and "parent_ab"
(the parent-commit comparison, made by a job of its own) are kept.  A record,
not a gate.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sqlop", action="store_true", help="odigossqldboperationprocessor through the OTLP path")
    ap.add_argument("--condattr", action="store_true", help="odigosconditionalattributes through the OTLP path")
    ap.add_argument("--url-full", type=float, default=None, metavar="SHARE",
                    help="otlp_url_full off against on; SHARE of the HTTP spans carries url.full alone")
    ap.add_argument("--out", default=str(ROOT / "gpurun_out" / "otlp.json"))
    args = ap.parse_args()
    if args.url_full is not None:
        if args.out == ap.get_default("out"):
            args.out = str(ROOT / "profiles" / "otlp_url_full_bench.json")
        if args.spans == ap.get_default("spans"):
            args.spans = 1_000_000
        return url_full_main(args)
    if args.condattr:
        if args.out == ap.get_default("out"):
            args.out = str(ROOT / "profiles" / "otlp_condattr_bench.json")
        return condattr_main(args)
    if args.sqlop and args.out == ap.get_default("out"):   # a file of its own beside the default
        args.out = str(Path(args.out).with_name("otlp_sqlop.json"))
    sql_every = 3 if args.sqlop else 0
    import torch
    from bench import NODE_KEYS, cpu_share
    from odigos_amd import native
    from odigos_amd.batch import Engine, Generator, OtlpBatch, PinnedBuffer, Router
    from tests.workloads import c3_sampling_config
    share, nproc, model = cpu_share()
    threads = max(1, min(16, share))
    t = time.perf_counter()
    g = Generator("fused", seed=0x0D16F0A1, n_spans=args.spans, threads=threads)
    pb = g.otlp(threads, sql_every)
    print(f"generated {len(pb) / 1e9:.2f} GB for {args.spans} spans in {time.perf_counter() - t:.1f}s", flush=True)
    cfg = {"odigossampling": c3_sampling_config(), "odigosurltemplate": {},
           "odigostrafficmetrics": {"res_attributes_keys": NODE_KEYS}}
    if args.sqlop:
        cfg["odigossqldboperationprocessor"] = {}
    eng = Engine(cfg)
    pin = PinnedBuffer(pb)
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    if args.sqlop:
        eng.set_option("otlp_sqlop", 1)
        st |= native.STAGE_SQLOP
    sh = torch.cuda.current_stream().cuda_stream

    # outputs allocated once (the shim keeps its buffers); template arena 64 B/span
    from odigos_amd.batch import device_outputs
    dims = native.Columns()
    dims.n_spans, dims.n_resources, dims.n_attrsets = g.cols.n_spans, g.cols.n_resources, 4096
    outs = device_outputs(dims, tmpl_cap=64 * args.spans)
    phases = []

    # data streams over the generated services (k8s.deployment.name = svc-NN in
    # namespace default): two pipelines, one of them fed twice, the rest default
    streams = [{"name": "ds-a", "sources": [{"namespace": "default", "kind": "Deployment", "name": "svc-%02d" % k}
                                            for k in range(0, 12)],
                "destinations": [{"destinationname": "d1", "configuredsignals": ["TRACES"]}]},
               {"name": "ds-b", "sources": [{"namespace": "default", "kind": "Deployment", "name": "svc-%02d" % k}
                                            for k in range(8, 20)],
                "destinations": [{"destinationname": "d2", "configuredsignals": ["TRACES", "LOGS"]}]}]
    router = Router({"datastreams": streams})
    enc = []

    def one(pinned: bool, stages: bool):
        a = time.perf_counter()
        ob = (OtlpBatch(eng, pin.p, stream=sh, length=pin.n, outputs=outs) if pinned
              else OtlpBatch(eng, pb, stream=sh, outputs=outs))
        phases.append(ob.timings_ms)
        torch.cuda.synchronize()
        b = time.perf_counter()
        if stages:
            eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=0x5EED, stream=sh)
            torch.cuda.synchronize()
        c = time.perf_counter()
        if stages:
            out = ob.encode(st, native.GROUP_TRACE_ID, router, stream=sh, copy=False)
            enc.append((time.perf_counter() - c, out, ob.encode_ms, ob.encode_path))
        info = (ob.cols.n_spans, ob.host_spans, int(ob.out_numpy("device_status", n=1)[0]) if stages else 0)
        ob.close()
        return b - a, c - b, info

    for _ in range(2):
        one(True, True)
    res = {"metric": "OTLP protobuf ingest: host TracesData bytes -> decoded columns -> SAMPLE|TEMPLATE|" +
                     ("SQLOP|SIZE" if args.sqlop else "SIZE"),
           "sqlop": bool(args.sqlop),
           "spans": args.spans, "message_bytes": len(pb), "bytes_per_span": len(pb) / args.spans,
           "host_cpu": model, "cpu_share": share, "nproc": nproc}
    eng.profile(True)
    dec, stg = [], []
    for _ in range(args.reps):
        d, s, info = one(True, True)
        dec.append(d)
        stg.append(s)
        assert info[2] == 0, "device status"
    prof = eng.profile_read()
    eng.profile(False)
    n_dec = prof.get("otlp_span_kernel", {"ms": 0.0, "launches": 1})
    k_ms = n_dec["ms"] / max(n_dec["launches"], 1)
    decode_kernels = ("otlp_span_kernel", "otlp_sqlop_kernel")
    stage_ms = sum(v["ms"] for k, v in prof.items() if k not in decode_kernels) / args.reps
    dp = min(dec)
    res["decode_pinned_ms"] = dp * 1e3
    best = phases[2 + dec.index(dp)]
    res["decode_phases_ms"] = best
    res["stages_ms"] = min(stg) * 1e3
    res["stages_kernel_ms"] = stage_ms
    res["end_to_end_spans_per_s"] = args.spans / (dp + min(stg))
    res["decode_spans_per_s"] = args.spans / dp
    res["host_pass_spans"] = info[1]
    res["span_kernel_ms"] = k_ms
    if args.sqlop:
        # the second pass: the span payloads again (the message bytes), span_ref and the
        # span kernel's host flag read, db_flags + db_query written
        q = prof.get("otlp_sqlop_kernel", {"ms": 0.0, "launches": 1})
        q_ms = q["ms"] / max(q["launches"], 1)
        q_alg = len(pb) + (8 + 1) * args.spans + (1 + 8) * args.spans
        res["sqlop_decode_kernel_ms"] = q_ms
        res["sqlop_decode_kernel_roofline"] = {"bound": "hbm", "achieved": q_alg / (q_ms * 1e-3) / 1e9 if q_ms else 0.0,
                                               "peak": 8000.0, "unit": "GB/s", "algorithmic_bytes": q_alg}
        res["sqlop_decode_kernel_roofline"]["frac"] = res["sqlop_decode_kernel_roofline"]["achieved"] / 8000.0
    e_best = min(enc[2:], key=lambda x: x[0])
    res["encode_ms"] = e_best[0] * 1e3
    res["encode_path"] = e_best[3]
    res["encode_phases_ms"] = dict(zip(("decisions_d2h", "sizing", "buffers", "writing"), e_best[2]))
    res["encode_outputs"] = [{"pipeline": p, "bytes": nb, "resources": nr} for p, nb, nr in e_best[1]]
    out_bytes = sum(x["bytes"] for x in res["encode_outputs"])
    res["encode_out_GBps"] = out_bytes / e_best[0] / 1e9
    res["end_to_end_with_encode_spans_per_s"] = args.spans / (dp + min(stg) + e_best[0])
    # decoder roofline: the message bytes it reads + 60 B/span of columns (and flags) written
    alg = len(pb) + 8 * args.spans + 60 * args.spans
    res["span_kernel_roofline"] = {"bound": "hbm", "achieved": alg / (k_ms * 1e-3) / 1e9 if k_ms else 0.0,
                                   "peak": 8000.0, "unit": "GB/s", "algorithmic_bytes": alg}
    res["span_kernel_roofline"]["frac"] = res["span_kernel_roofline"]["achieved"] / 8000.0
    d, _, _ = one(False, False)
    res["decode_pageable_ms"] = d * 1e3
    # per-call latency at the batch processor's 8192 spans
    smallpb = Generator("fused", seed=0x0D16F0A2, n_spans=8192, threads=threads).otlp(threads, sql_every)
    spin = PinnedBuffer(smallpb)
    sdims = native.Columns()
    sdims.n_spans, sdims.n_resources, sdims.n_attrsets = 8192, 8192, 4096
    souts = device_outputs(sdims, tmpl_cap=64 * 8192)
    lat, sph, leg = [], [], []
    for k in range(220):
        a = time.perf_counter()
        ob = OtlpBatch(eng, spin.p, stream=sh, length=spin.n, outputs=souts)
        sph.append(ob.timings_ms)
        b = time.perf_counter()
        eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=0x5EED, stream=sh)
        torch.cuda.synchronize()
        c = time.perf_counter()
        ob.encode(st, native.GROUP_TRACE_ID, router, stream=sh, copy=False)
        d = time.perf_counter()
        sph[-1].update({"enc_" + x: v for x, v in zip(("d2h", "sizing", "buffers", "writing"), ob.encode_ms)})
        ob.close()
        if k >= 20:
            lat.append(time.perf_counter() - a)
            leg.append(((b - a) * 1e3, (c - b) * 1e3, (d - c) * 1e3))
    lat.sort()
    res["batch8192_decode_stages_encode_us"] = {"p50": lat[len(lat) // 2] * 1e6, "p99": lat[int(len(lat) * 0.99)] * 1e6}
    res["batch8192_spans_per_s"] = 8192 / lat[len(lat) // 2]
    res["batch8192_legs_ms_median"] = {k: sorted(x[j] for x in leg)[len(leg) // 2]
                                       for j, k in enumerate(("decode", "stages", "encode"))}
    res["batch8192_decode_phases_ms_median"] = {k: sorted(x[k] for x in sph[20:])[len(sph[20:]) // 2] for k in sph[0]}
    # the same 8192-span request from several callers at once (a receiver's
    # concurrent export requests): one stream and one set of outputs per
    # caller, the engine and router shared; whole-job spans/s
    import threading
    for callers in (1, 4, 8, 16):
        per = 120
        ready = threading.Barrier(callers + 1)
        errs = []

        def caller(k):
            try:
                cs = torch.cuda.Stream()
                ch = cs.cuda_stream
                co = device_outputs(sdims, tmpl_cap=64 * 8192)
                ready.wait()
                for _ in range(per):
                    ob = OtlpBatch(eng, spin.p, stream=ch, length=spin.n, outputs=co)
                    eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=0x5EED, stream=ch)
                    ob.encode(st, native.GROUP_TRACE_ID, router, stream=ch, copy=False)
                    ob.close()
                cs.synchronize()
            except Exception as ex:   # pragma: no cover
                errs.append(repr(ex))

        th = [threading.Thread(target=caller, args=(k,)) for k in range(callers)]
        for t_ in th:
            t_.start()
        ready.wait()
        a = time.perf_counter()
        for t_ in th:
            t_.join()
        wall = time.perf_counter() - a
        assert not errs, errs
        res.setdefault("batch8192_callers", []).append(
            {"callers": callers, "calls": callers * per, "wall_s": wall,
             "spans_per_s": callers * per * 8192 / wall, "calls_per_s": callers * per / wall})
        print(f"otlp 8192-span calls, {callers} callers: {callers * per * 8192 / wall / 1e6:.1f} M spans/s", flush=True)
    # the same requests through ose_otlp_pipeline: concurrent callers'
    # requests coalesced into one device batch per wave of calls
    from odigos_amd.batch import OtlpPipeline
    pipe = OtlpPipeline(eng, router, st)
    import os
    if os.environ.get("OSE_PIPE_RUNNING"):   # diagnostics: the product defaults otherwise (4, 200 us, 8)
        pipe.tune(int(os.environ["OSE_PIPE_RUNNING"]), int(os.environ.get("OSE_PIPE_WINDOW_US", "200")),
                  int(os.environ.get("OSE_PIPE_TARGET", "8")))
    for callers in (1, 4, 8, 16):
        per = 150 if callers > 1 else 120
        ready = threading.Barrier(callers + 1)
        errs = []

        def pcaller(k):
            try:
                ready.wait()
                for _ in range(per):
                    pipe.consume(spin.p, spin.n, seed=0x5EED, copy=False)
            except Exception as ex:   # pragma: no cover
                errs.append(repr(ex))

        th = [threading.Thread(target=pcaller, args=(k,)) for k in range(callers)]
        for t_ in th:
            t_.start()
        pipe.counters()
        ready.wait()
        a = time.perf_counter()
        for t_ in th:
            t_.join()
        wall = time.perf_counter() - a
        assert not errs, errs
        cnt = pipe.counters()
        res.setdefault("pipeline8192_callers", []).append(
            {"callers": callers, "calls": callers * per, "wall_s": wall,
             "spans_per_s": callers * per * 8192 / wall, "calls_per_s": callers * per / wall,
             "batches": cnt["batches"], "largest_batch": cnt["largest_batch"], "alone": cnt["alone"],
             "batch_ms": cnt["batch_ms"]})
        print(f"otlp pipeline 8192-span requests, {callers} callers: {callers * per * 8192 / wall / 1e6:.1f} M spans/s "
              f"({cnt['batches']} batches, largest {cnt['largest_batch']}, alone {cnt['alone']}, ms {cnt['batch_ms']})", flush=True)
    pipe.close()
    spin.close()
    pin.close()
    line = json.dumps(res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line, flush=True)


def condattr_main(args):
    import ctypes as C

    import torch
    from bench import cpu_share
    from odigos_amd import native
    from odigos_amd.batch import Engine, Generator, OtlpBatch, PinnedBuffer, Router, device_outputs
    share, nproc, model = cpu_share()
    threads = max(1, min(16, share))
    # the shipped profile as the processor's config (action lists shared by name in the file)
    prof_json = json.loads((ROOT / "tests" / "golden" / "category_attributes_profile.json").read_text())
    cfg = {"global_default": prof_json["global_default"],
           "rules": [{"field_to_check": r["field_to_check"],
                      "new_attribute_value_configurations": {v: r["action_lists"][k] for v, k in r["values"].items()}}
                     for r in prof_json["rules"]]}
    SECTION, TRAFFIC = "odigosconditionalattributes", {"res_attributes_keys": ["service.name", "k8s.namespace.name"]}
    names = list(cfg["rules"][0]["new_attribute_value_configurations"]) + ["unknown.library.%d" % k for k in range(30)]
    eng = Engine({SECTION: cfg, "odigostrafficmetrics": TRAFFIC})
    eng.set_option("otlp_condattr", 1)
    L = eng.L
    info = eng.condattr_info()
    T, K = info.n_targets, info.n_keys
    sh = torch.cuda.current_stream().cuda_stream
    streams = [{"name": "ds-a", "sources": [{"namespace": "default", "kind": "Deployment", "name": "svc-%02d" % k}
                                            for k in range(0, 12)],
                "destinations": [{"destinationname": "d1", "configuredsignals": ["TRACES"]}]}]
    router = Router({"datastreams": streams})
    res = {"metric": "OTLP protobuf ingest: host TracesData bytes -> decoded columns -> CONDATTR -> SIZE -> "
                     "ose_otlp_encode_condattr (the category-attributes profile)",
           "condattr": True, "targets": T, "keys": K, "scope_names": len(names), "host_cpu": model, "cpu_share": share,
           "nproc": nproc}

    def setup(n_spans, seed):
        g = Generator("fused", seed=seed, n_spans=n_spans, threads=threads)
        pb = g.otlp(threads, scope_names=names)
        dims = native.Columns()
        dims.n_spans, dims.n_resources, dims.n_attrsets = n_spans, g.cols.n_resources, 4096
        outs = device_outputs(dims, tmpl_cap=16)
        words = int(L.ose_condattr_scratch_words(eng.h, g.cols.n_resources))
        z = lambda nb: torch.zeros(max(16, nb), dtype=torch.uint8, device="cuda")   # noqa: E731
        t = {"src": z(T * n_spans), "val": z(8 * T * n_spans), "span_size_out": z(4 * n_spans), "scratch": z(4 * words),
             "device_status": z(16)}
        o = native.CondAttrOutputs()
        for k, v in t.items():
            setattr(o, k, v.data_ptr())
        return pb, PinnedBuffer(pb), outs, o, t

    def one(pin, outs, o, stream):
        a = time.perf_counter()
        ob = OtlpBatch(eng, pin.p, stream=stream, length=pin.n, outputs=outs)
        b = time.perf_counter()
        native.check(L.ose_condattr_process_device(eng.h, C.byref(ob.condattr_cols), C.byref(o), C.c_void_p(stream)))
        ob.cols.span_size = o.span_size_out
        eng.process_device(ob, native.STAGE_SIZE, native.GROUP_TRACE_ID, stream=stream)
        torch.cuda.synchronize() if stream == sh else None
        c = time.perf_counter()
        path = {}
        out = eng.otlp_encode_condattr(ob, o, router, stream=stream, copy=False, path=path)
        d = time.perf_counter()
        r = {"decode": (b - a) * 1e3, "stages": (c - b) * 1e3, "encode": (d - c) * 1e3, "phases": ob.timings_ms,
             "host_spans": ob.host_spans, "path": path, "out": out, "arena_bytes": ob.cols.arena_bytes}
        ob.close()
        return r

    t0 = time.perf_counter()
    pb, pin, outs, o, keep = setup(args.spans, 0x0D16F0A1)
    print(f"generated {len(pb) / 1e9:.2f} GB for {args.spans} spans in {time.perf_counter() - t0:.1f}s", flush=True)
    res.update({"spans": args.spans, "message_bytes": len(pb), "bytes_per_span": len(pb) / args.spans})
    for _ in range(2):
        one(pin, outs, o, sh)
    eng.profile(True)
    runs = [one(pin, outs, o, sh) for _ in range(args.reps)]
    prof = eng.profile_read()
    eng.profile(False)
    best = min(runs, key=lambda r: r["decode"] + r["stages"] + r["encode"])
    puts = int((keep["src"][:T * args.spans] != 0).sum().item())
    res["decode_pinned_ms"] = best["decode"]
    res["decode_phases_ms"] = best["phases"]
    res["stages_ms"] = best["stages"]
    res["encode_ms"] = best["encode"]
    res["encode_path"] = best["path"]
    res["encode_outputs"] = [{"pipeline": p, "bytes": nb, "resources": nr} for p, nb, nr in best["out"]]
    res["host_pass_spans"] = best["host_spans"]
    res["puts"] = puts
    res["end_to_end_spans_per_s"] = args.spans / ((best["decode"] + best["stages"] + best["encode"]) * 1e-3)
    res["kernels_ms_per_call"] = {k: v["ms"] / max(v["launches"], 1) for k, v in prof.items()}
    # otlp_condattr_kernel: the message bytes read again, span_ref (8) and the host flag (1) per span read, and
    # per hit has (1) + val (8) + kv_size (4, target keys) written; the hits counted from the decoded columns
    ob = OtlpBatch(eng, pin.p, stream=sh, length=pin.n, outputs=outs)
    hits = int(np_sum_has(ob, K))
    ob.close()
    k_ms = res["kernels_ms_per_call"].get("otlp_condattr_kernel", 0.0)
    alg = len(pb) + 9 * args.spans + 13 * hits
    bw = C.c_double()
    a_ = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b_ = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    native.check(L.osehost_stream_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), 10, C.c_void_p(sh), C.byref(bw)))
    del a_, b_
    res["otlp_condattr_kernel"] = {"ms": k_ms, "span_has_hits": hits, "algorithmic_bytes": alg,
                                   "algorithmic_gbs": alg / (k_ms * 1e-3) / 1e9 if k_ms else 0.0, "stream_copy_gbs": bw.value}
    res["otlp_condattr_kernel"]["frac_of_stream_copy"] = (res["otlp_condattr_kernel"]["algorithmic_gbs"] / bw.value
                                                          if bw.value else 0.0)
    pin.close()
    # 8192-span requests: one caller's latency, then 8 callers
    spb, spin, souts, so, skeep = setup(8192, 0x0D16F0A2)
    lat = []
    for k in range(220):
        a = time.perf_counter()
        r = one(spin, souts, so, sh)
        if k >= 20:
            lat.append((time.perf_counter() - a, r["decode"], r["stages"], r["encode"]))
    lat.sort()
    med = lambda j: sorted(x[j] for x in lat)[len(lat) // 2]   # noqa: E731
    res["batch8192_us"] = {"p50": med(0) * 1e6, "p99": lat[int(len(lat) * 0.99)][0] * 1e6}
    res["batch8192_legs_ms_median"] = {"decode": med(1), "stages": med(2), "encode": med(3)}
    res["batch8192_spans_per_s"] = 8192 / med(0)
    res["batch8192_encode_path"] = r["path"]
    import threading
    callers, per = 8, 120
    ready = threading.Barrier(callers + 1)
    errs = []

    def caller(k):
        try:
            cs = torch.cuda.Stream()
            _, _, co, cobj, ckeep = setup(8192, 0x0D16F0A2)
            ready.wait()
            for _ in range(per):
                one(spin, co, cobj, cs.cuda_stream)
            cs.synchronize()
        except Exception as ex:   # pragma: no cover
            errs.append(repr(ex))
            ready.abort()

    th = [threading.Thread(target=caller, args=(k,)) for k in range(callers)]
    for t_ in th:
        t_.start()
    ready.wait()
    a = time.perf_counter()
    for t_ in th:
        t_.join()
    wall = time.perf_counter() - a
    assert not errs, errs
    res["batch8192_callers"] = {"callers": callers, "calls": callers * per, "wall_s": wall,
                                "spans_per_s": callers * per * 8192 / wall}
    spin.close()
    out = Path(args.out)
    if out.exists():
        try:
            old = json.loads(out.read_text())
            if "option_off_ab" in old:
                res["option_off_ab"] = old["option_off_ab"]
        except ValueError:
            pass
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


def url_full_main(args):
    import threading

    import torch
    from bench import NODE_KEYS, cpu_share
    from odigos_amd import native
    from odigos_amd.batch import Engine, Generator, OtlpBatch, PinnedBuffer, device_outputs
    from tests.workloads import c3_sampling_config
    share_cpu, nproc, model = cpu_share()
    threads = max(1, min(16, share_cpu))
    share = args.url_full
    cfg = {"odigossampling": c3_sampling_config(), "odigosurltemplate": {},
           "odigostrafficmetrics": {"res_attributes_keys": NODE_KEYS}}
    engs = {"off": Engine(cfg), "on": Engine(cfg)}
    engs["on"].set_option("otlp_url_full", 1)
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    sh = torch.cuda.current_stream().cuda_stream
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731

    def message(n, seed):
        pb = Generator("fused", seed=seed, n_spans=n, threads=threads).otlp(threads, url_full=share)
        dims = native.Columns()
        dims.n_spans, dims.n_resources, dims.n_attrsets = n, n, 4096
        return pb, PinnedBuffer(pb), dims

    def one(arm, pin, outs, stream, timed):
        eng = engs[arm]
        a = time.perf_counter()
        ob = OtlpBatch(eng, pin.p, stream=stream, length=pin.n, outputs=outs)
        b = time.perf_counter()
        eng.process_device(ob, st, native.GROUP_TRACE_ID, seed=0x5EED, stream=stream)
        if timed:
            torch.cuda.synchronize()
        c = time.perf_counter()
        ob.encode(st, native.GROUP_TRACE_ID, None, stream=stream, copy=False)
        d = time.perf_counter()
        r = {"decode": (b - a) * 1e3, "stages": (c - b) * 1e3, "encode": (d - c) * 1e3, "total": (d - a) * 1e3,
             "phases": ob.timings_ms, "host_spans": ob.host_spans, "counts": ob.url_full_counts}
        ob.close()
        return r

    def summary(runs):
        return {"decode_ms_median": med([r["decode"] for r in runs]), "decode_ms_min": min(r["decode"] for r in runs),
                "total_ms_median": med([r["total"] for r in runs]),
                "decode_phases_ms_median": {k: med([r["phases"][k] for r in runs]) for k in runs[0]["phases"]},
                "host_pass_spans": runs[-1]["host_spans"], "url_full_counts": list(runs[-1]["counts"]), "calls": len(runs)}

    res = {"metric": "ose_otlp_decode (and decode -> SAMPLE|TEMPLATE|SIZE -> ose_otlp_encode) with the engine option "
                     "otlp_url_full off against on, arms interleaved on one build",
           "url_full_share": share, "host_cpu": model, "cpu_share": share_cpu, "nproc": nproc}
    # 8192-span requests, one caller: the arms alternate call by call
    spb, spin, sdims = message(8192, 0x0D16F0A2)
    souts = device_outputs(sdims, tmpl_cap=64 * 8192)
    res["request8192_message_bytes"] = len(spb)
    res["request8192_url_full_spans"] = spb.count(b"url.full")
    runs = {"off": [], "on": []}
    for k in range(240):
        for arm in ("off", "on"):
            r = one(arm, spin, souts, sh, True)
            if k >= 40:
                runs[arm].append(r)
    res["request8192_1caller"] = {arm: summary(runs[arm]) for arm in runs}
    # ... eight callers: whole-job spans/s, the arms in alternating blocks
    callers, per = 8, 60
    blocks = {"off": [], "on": []}
    couts = [device_outputs(sdims, tmpl_cap=64 * 8192) for _ in range(callers)]
    cstreams = [torch.cuda.Stream() for _ in range(callers)]
    for blk in range(6):
        arm = ("off", "on")[blk % 2]
        ready = threading.Barrier(callers + 1)
        errs = []

        def caller(k):
            try:
                ready.wait()
                for _ in range(per):
                    one(arm, spin, couts[k], cstreams[k].cuda_stream, False)
                cstreams[k].synchronize()
            except Exception as ex:   # pragma: no cover
                errs.append(repr(ex))
                ready.abort()

        th = [threading.Thread(target=caller, args=(k,)) for k in range(callers)]
        for t_ in th:
            t_.start()
        ready.wait()
        a = time.perf_counter()
        for t_ in th:
            t_.join()
        wall = time.perf_counter() - a
        assert not errs, errs
        if blk >= 2:   # the first block of each arm warms the callers' buffers
            blocks[arm].append(callers * per * 8192 / wall)
    res["request8192_8callers_spans_per_s"] = {arm: {"blocks": v, "median": med(v)} for arm, v in blocks.items()}
    spin.close()
    # one large message: decode from pinned memory, the arms alternating
    pb, pin, dims = message(args.spans, 0x0D16F0A1)
    outs = device_outputs(dims, tmpl_cap=64 * args.spans)
    res["message_spans"] = args.spans
    res["message_bytes"] = len(pb)
    res["message_url_full_spans"] = pb.count(b"url.full")
    runs = {"off": [], "on": []}
    for k in range(args.reps + 1):
        for arm in ("off", "on"):
            r = one(arm, pin, outs, sh, True)
            if k >= 1:
                runs[arm].append(r)
    res["message"] = {arm: summary(runs[arm]) for arm in runs}
    pin.close()
    out = Path(args.out)
    doc = {}
    if out.exists():
        try:
            doc = json.loads(out.read_text())
        except ValueError:
            doc = {}
    doc["share_%g" % share] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(res), flush=True)


def np_sum_has(ob, K):
    """span_has entries set in a decoded batch's odigosconditionalattributes columns."""
    import ctypes as C

    import numpy as np
    from odigos_amd import native
    has = np.zeros(K * ob.cols.n_spans + 16, dtype=np.uint8)
    dst = native.CondAttrColumns()
    dst.span_has = has.ctypes.data
    native.check(ob.L.ose_otlp_condattr_download(ob.h, C.byref(dst)))
    return has.sum(dtype="uint64")


if __name__ == "__main__":
    main()
