"""groupbytrace on the OTLP path, end to end on one GPU: 8192-span requests of
the C4 mix in pdata's encoding go decode -> add_otlp -> release_otlp ->
SAMPLE | TEMPLATE | SIZE -> encode with the three-output router (two
pipelines and "default"), through one store, from 1 and 8 callers.

The clock is simulated: every step advances it by wait_duration, so the
release of step k hands back the traces step k-1 added (their ids return with
every request and start new traces, as ids do after their trace has left).
The store and the batch it releases belong to one caller at a time: callers
decode concurrently and take a lock from add to encode.

Reported: spans/s end to end and the median ms of each leg; the two wave
copies (gbt_msg_copy_kernel on the add, gbt_block_copy_kernel<true> on the
release) timed with HIP events (osehost_gbt_copy_times), as bytes read +
written over time against osehost_stream_copy in the same process.  One JSON
line on stdout and in --out.  Not a bench.py `value`.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "gbt_otlp.json"))
    args = ap.parse_args()
    import torch
    from bench import NODE_KEYS, cpu_share
    from odigos_amd import native
    from odigos_amd.batch import Engine, Generator, GroupByTrace, OtlpBatch, PinnedBuffer, Router, device_outputs
    from tests.gbt_otlp_ref import pieces_of
    from tests.workloads import c3_sampling_config
    share, nproc, model = cpu_share()
    threads = max(1, min(16, share))
    L = native.lib()
    pb = Generator("fused", seed=0x0D16F0A2, n_spans=args.spans, threads=threads).otlp(threads)
    msg_bytes = sum(ln for _, _, msgs in pieces_of(pb) for _, ln in msgs)
    pin = PinnedBuffer(pb)
    cfg = {"odigossampling": c3_sampling_config(), "odigosurltemplate": {},
           "odigostrafficmetrics": {"res_attributes_keys": NODE_KEYS}}
    eng = Engine(cfg)
    streams = [{"name": "ds-a", "sources": [{"namespace": "default", "kind": "Deployment", "name": "svc-%02d" % k}
                                            for k in range(0, 12)],
                "destinations": [{"destinationname": "d1", "configuredsignals": ["TRACES"]}]},
               {"name": "ds-b", "sources": [{"namespace": "default", "kind": "Deployment", "name": "svc-%02d" % k}
                                            for k in range(8, 20)],
                "destinations": [{"destinationname": "d2", "configuredsignals": ["TRACES", "LOGS"]}]}]
    router = Router({"datastreams": streams})
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    S = 1_000_000_000
    dims = native.Columns()
    dims.n_spans, dims.n_resources, dims.n_attrsets = args.spans, args.spans, 4096
    res = {"metric": "groupbytrace on the OTLP path: decode -> add_otlp -> release_otlp -> SAMPLE|TEMPLATE|SIZE -> "
                     "encode (3 outputs)", "spans_per_request": args.spans, "message_bytes": len(pb),
           "span_message_bytes": msg_bytes, "steps": args.steps, "warmup": args.warmup, "host_cpu": model,
           "cpu_share": share, "nproc": nproc, "runs": []}

    for callers in (1, 8):
        store = GroupByTrace(eng, {"wait_duration": "1s", "num_traces": 1_000_000}, 8 * args.spans, 8 * len(pb) + (1 << 20))
        native.check(L.osehost_gbt_copy_times(store.h, 1, None))
        lock = threading.Lock()
        clock = [0]
        legs, copies, errs, paths = [], [], [], []
        ready = threading.Barrier(callers + 1)
        per = (args.steps + args.warmup + callers - 1) // callers

        def caller(k):
            try:
                cs = torch.cuda.Stream()
                ch = cs.cuda_stream
                co = device_outputs(dims, tmpl_cap=64 * args.spans)
                ready.wait()
                for it in range(per):
                    t0 = time.perf_counter()
                    ob = OtlpBatch(eng, pin.p, stream=ch, length=pin.n, outputs=co)
                    t1 = time.perf_counter()
                    with lock:
                        clock[0] += S
                        now = clock[0]
                        t2 = time.perf_counter()
                        store.add_otlp(ob, now, stream=ch)
                        t3 = time.perf_counter()
                        out = C.c_void_p()
                        nt = C.c_uint32()
                        native.check(L.ose_gbt_release_otlp(store.h, now, C.c_void_p(ch), C.byref(out), C.byref(nt)))
                        t4 = time.perf_counter()
                        rcols = native.Columns.from_buffer_copy(L.ose_otlp_columns(out).contents)
                        n_rel = rcols.n_spans
                        t5 = t6 = t4
                        if n_rel:
                            rnd = native.Rand(0x5EED, 0.0)
                            native.check(L.ose_process_device(eng.h, C.byref(rcols), C.byref(co[0]), st,
                                                              native.GROUP_TRACE_ID, C.byref(rnd), C.c_void_p(ch)))
                            cs.synchronize()
                            t5 = time.perf_counter()
                            h = C.c_void_p()
                            native.check(L.ose_otlp_encode(eng.h, out, C.byref(co[0]), st, native.GROUP_TRACE_ID, router.h,
                                                           C.c_void_p(ch), C.byref(h)))
                            path = {}
                            from odigos_amd.batch import take_otlp_out
                            take_otlp_out(L, h, False, [], path)
                            t6 = time.perf_counter()
                            ms = (C.c_double * 2)()
                            native.check(L.osehost_gbt_copy_times(store.h, 1, ms))
                            if it * callers >= args.warmup:
                                copies.append((ms[0], ms[1], rcols.arena_bytes))
                                paths.append(path)
                    ob.close()
                    if it * callers >= args.warmup and n_rel:
                        legs.append({"decode": (t1 - t0) * 1e3, "wait_lock": (t2 - t1) * 1e3, "add": (t3 - t2) * 1e3,
                                     "release": (t4 - t3) * 1e3, "stages": (t5 - t4) * 1e3, "encode": (t6 - t5) * 1e3,
                                     "request": (time.perf_counter() - t0) * 1e3, "released_spans": n_rel})
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
        med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
        run = {"callers": callers, "requests": per * callers, "wall_s": wall,
               "spans_per_s": per * callers * args.spans / wall,   # the whole job, warm-up requests included
               "request_ms_median": med([x["request"] for x in legs]),
               "legs_ms_median": {k: med([x[k] for x in legs]) for k in legs[0] if k not in ("released_spans", "request")},
               "released_spans_median": med([x["released_spans"] for x in legs]),
               "gpu_encoder_calls": sum(1 for p in paths if p.get("gpu")), "encode_calls": len(paths),
               "stats": store.stats()}
        # the copies: bytes read + written over the kernel's time
        m_ms, b_ms, rel_bytes = med([c[0] for c in copies]), med([c[1] for c in copies]), med([c[2] for c in copies])
        run["copy_kernels"] = {"gbt_msg_copy_kernel": {"ms": m_ms, "bytes_moved": 2 * msg_bytes,
                                                       "gbs": 2 * msg_bytes / (m_ms * 1e-3) / 1e9 if m_ms else 0.0},
                               "gbt_block_copy_kernel<true>": {"ms": b_ms, "bytes_moved": 2 * rel_bytes,
                                                               "gbs": 2 * rel_bytes / (b_ms * 1e-3) / 1e9 if b_ms else 0.0}}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        store.close()

    # the stream-copy rate in the same process (read + written bytes), at a
    # size the GPU's caches do not hold and at the size these copies move
    for name, nbytes in (("stream_copy_gbs", 1 << 30), ("stream_copy_gbs_at_request_size", max(msg_bytes, 1 << 12) // 16 * 16)):
        a_ = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        b_ = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        bw = C.c_double()
        native.check(L.osehost_stream_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), 10,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(bw)))
        res[name] = bw.value
    for run in res["runs"]:
        for k in run["copy_kernels"].values():
            k["frac_of_stream_copy"] = k["gbs"] / res["stream_copy_gbs"] if res["stream_copy_gbs"] else 0.0
            k["frac_of_stream_copy_at_request_size"] = (k["gbs"] / res["stream_copy_gbs_at_request_size"]
                                                        if res["stream_copy_gbs_at_request_size"] else 0.0)
    line = json.dumps(res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
