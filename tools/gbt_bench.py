"""GPU-resident groupbytrace in steady state on one GPU:
a C4-mix batch of --spans spans arrives every simulated second (fresh trace
ids each time), wait_duration 30 s, so each call adds one batch and, after
the first 30, releases the traces of the batch added 30 s earlier; the
three processors then run on the release (OSE_GROUP_TRACE_ID).  Wall time
per leg with device syncs; one JSON line on stdout and in --out.  Not a
bench.py `value`.

--sqlop: the engine also has the odigossqldboperationprocessor section, a
third of the spans carry a db.query.text from tools/sqlop_bench.py's pool
(about 71 bytes on average; the bytes are appended to the batch's device
arena), the store carries db_flags / db_query through add and release, and
the stages on the release include OSE_STAGE_SQLOP.  The JSON then also has
the query bytes per batch.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def add_queries(db, n, seed):
    """db_flags / db_query on a DeviceBatch: a third of the spans get a query
    of sqlop_bench's pool, laid after the batch's own arena bytes (the
    existing refs stay valid).  Returns the query bytes added."""
    import random

    import torch
    from odigos_amd import native
    from tools.sqlop_bench import query_pool
    dev = db.t["arena"].device
    pool = query_pool(random.Random(seed), 4096)
    pool_len = torch.tensor([len(q) for q in pool], dtype=torch.int64, device=dev)
    pool_off = torch.cumsum(pool_len, 0) - pool_len
    pool_bytes = torch.frombuffer(bytearray(b"".join(pool)), dtype=torch.uint8).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    has_q = torch.rand(n, generator=g, device=dev) < 1 / 3
    idx = torch.randint(0, len(pool), (n,), generator=g, device=dev)
    lens = torch.where(has_q, pool_len[idx], torch.zeros_like(idx))
    base = int(db.cols.arena_bytes)
    offs = base + torch.cumsum(lens, 0) - lens
    qbytes = int(lens.sum().item())
    assert base + qbytes < 0xFFFFFFF0
    arena = torch.zeros((base + qbytes + 15) // 16 * 16 + 32, dtype=torch.uint8, device=dev)
    arena[:base] = db.t["arena"][:base]
    qi = torch.nonzero(has_q).squeeze(1)
    step = 1 << 20   # slices of 1M queries: bounded temporaries
    for a in range(0, qi.numel(), step):
        s = qi[a:a + step]
        ln, of = lens[s], offs[s]
        owner = torch.repeat_interleave(torch.arange(s.numel(), device=dev), ln)
        pos = torch.arange(owner.numel(), device=dev) - (of - of[0])[owner]
        arena[int(of[0]):int(of[0]) + owner.numel()] = pool_bytes[pool_off[idx[s]][owner] + pos]
    db.t["arena"] = arena
    db.t["db_flags"] = has_q.to(torch.uint8) * native.DB_HAS_QUERY
    db.t["db_query"] = (offs | (lens << 32)).contiguous()   # ose_strref {off, len} as one little-endian word
    db.cols.arena, db.cols.arena_bytes = arena.data_ptr(), base + qbytes
    db.cols.db_flags, db.cols.db_query = db.t["db_flags"].data_ptr(), db.t["db_query"].data_ptr()
    return qbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=str(ROOT / "gpurun_out" / "gbt.json"))
    ap.add_argument("--sqlop", action="store_true", help="carry db.query.text through the store and run OSE_STAGE_SQLOP")
    args = ap.parse_args()
    import torch
    from bench import NODE_KEYS, cpu_share
    from odigos_amd import native
    from odigos_amd.batch import DeviceBatch, DeviceView, Engine, Generator, GroupByTrace
    from tests.workloads import c3_sampling_config
    share, nproc, model = cpu_share()
    g = Generator("fused", seed=0x6B70001, n_spans=args.spans, threads=max(1, min(16, share)))
    cfg = {"odigossampling": c3_sampling_config(), "odigosurltemplate": {},
           "odigostrafficmetrics": {"res_attributes_keys": NODE_KEYS}}
    if args.sqlop:
        cfg["odigossqldboperationprocessor"] = {}
    eng = Engine(cfg)
    db = DeviceBatch(g.cols)
    query_bytes = add_queries(db, args.spans, 0x5A10B) if args.sqlop else 0
    tid = db.t["trace_id"][: 16 * args.spans].view(torch.int64)
    hold = 32 * args.spans
    # num_traces sized for the stream (contrib's default 1,000,000 would evict
    # traces at this rate: 30 s of batches hold ~6M traces)
    # (--sqlop: about 71 / 3 more bytes per span wait in the arena ring)
    store = GroupByTrace(eng, {"wait_duration": "30s", "num_traces": 16_000_000}, hold, hold * (80 if args.sqlop else 48))
    st = native.STAGE_SAMPLE | native.STAGE_TEMPLATE | native.STAGE_SIZE
    if args.sqlop:
        st |= native.STAGE_SQLOP
    legs = []
    S = 1_000_000_000
    for step in range(args.steps):
        tid.bitwise_xor_(step * 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF if step else 0)
        torch.cuda.synchronize()
        a = time.perf_counter()
        store.add(db.cols, step * S)
        torch.cuda.synchronize()
        b = time.perf_counter()
        rel, ntr = store.release(step * S)
        torch.cuda.synchronize()
        c = time.perf_counter()
        rel_ms = (c - b) * 1e3
        if rel.n_spans:
            view = DeviceView(rel)   # outputs for this release (allocation not timed)
            torch.cuda.synchronize()
            c = time.perf_counter()
            eng.process_device(view, st, native.GROUP_TRACE_ID, seed=step)
            torch.cuda.synchronize()
        d = time.perf_counter()
        legs.append({"step": step, "add_ms": (b - a) * 1e3, "release_ms": rel_ms, "stages_ms": (d - c) * 1e3,
                     "released_spans": rel.n_spans, "released_traces": ntr})
        print(json.dumps(legs[-1]), flush=True)
    steady = [x for x in legs if x["released_spans"]]
    med = lambda k: sorted(x[k] for x in steady)[len(steady) // 2]  # noqa: E731
    res = {"metric": "groupbytrace store: steady-state add + release (+ stages) per batch", "spans_per_batch": args.spans,
           "wait_duration_s": 30, "num_traces": 16_000_000, "held_spans": store.stats()["held_spans"], "steady_steps": len(steady),
           "add_ms": med("add_ms"), "release_ms": med("release_ms"), "stages_ms": med("stages_ms"),
           "store_spans_per_s": args.spans / ((med("add_ms") + med("release_ms")) * 1e-3),
           "with_stages_spans_per_s": args.spans / ((med("add_ms") + med("release_ms") + med("stages_ms")) * 1e-3),
           "stats": store.stats(), "host_cpu": model}
    if args.sqlop:
        res.update({"sqlop": True, "query_bytes_per_batch": query_bytes,
                    "arena_bytes_per_batch": int(db.cols.arena_bytes)})
    line = json.dumps(res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
