#!/usr/bin/env python3
"""Times the SQLOP stage (odigossqldboperationprocessor, sqlop_kernel) alone.

A seeded batch is built on the device at a size a gateway batch has: 10M
spans by default, about a third of them carrying a db.query.text of typical
length (statements of 5-165 bytes, about 72 on average, from a seeded pool, some with leading
blanks, lower case or a keyword the processor does not know), a few with
db.operation.name already set, and an exclude list that skips some resources.
After a warm-up the stage is timed over --calls calls of ose_process_device,
each between two device events.

Prints one JSON line (and writes it to --out):
  ms_per_call          median of the per-call device times (mean, min, max beside it)
  spans_per_s          n_spans over the median
  algorithmic_bytes    computed from the shapes: per span db_flags (1) + db_query (8)
                       + resource (4) + the sql_op byte written (1); res_sql_ok once;
                       per classified span the 16-byte arena chunks its first
                       16 bytes touch (the general path's further bytes are not counted)
  algorithmic_gbs      those bytes over the median time
  stream_copy_gbs      measured here with osehost_stream_copy (read + written bytes)
  frac_of_stream_copy  algorithmic_gbs over it
A sample of the results is checked against the host-compiled classifier
(osehost_sqlop_detect) before anything is timed.  A record, not a gate.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def query_pool(rng: random.Random, size: int) -> list[bytes]:
    tables = ["users", "orders", "order_items", "inventory", "sessions", "audit_log", "payments", "products"]
    cols = ["id", "user_id", "status", "created_at", "amount", "sku", "email", "updated_at", "quantity"]
    out = []
    for _ in range(size):
        t, c = rng.choice(tables), rng.sample(cols, 4)
        kind = rng.random()
        if kind < 0.45:
            q = f"SELECT {c[0]}, {c[1]}, {c[2]} FROM {t} WHERE {c[3]} = ?"
            if rng.random() < 0.5:
                q += f" AND {c[1]} IN (?, ?, ?) ORDER BY {c[0]} DESC LIMIT ?"
        elif kind < 0.62:
            q = f"INSERT INTO {t} ({', '.join(c)}) VALUES (?, ?, ?, ?)"
        elif kind < 0.78:
            q = f"UPDATE {t} SET {c[0]} = ?, {c[1]} = ? WHERE {c[2]} = ?"
        elif kind < 0.86:
            q = f"DELETE FROM {t} WHERE {c[0]} = ? AND {c[1]} < ?"
        elif kind < 0.90:
            q = rng.choice([f"CREATE TABLE IF NOT EXISTS {t}_tmp (id bigint)", f"DROP TABLE {t}_tmp",
                            f"ALTER TABLE {t} ADD COLUMN {c[0]}_x int"])
        else:
            q = rng.choice(["BEGIN", "COMMIT", f"WITH x AS (SELECT 1) SELECT * FROM x JOIN {t} USING ({c[0]})",
                            f"EXPLAIN SELECT * FROM {t}", "SET search_path TO app", f"(SELECT 1 FROM {t})"])
        x = rng.random()
        if x < 0.15:
            q = q.lower()
        if 0.15 <= x < 0.25:
            q = rng.choice(["\n    ", "  ", "\t", "\n"]) + q
        if 0.25 <= x < 0.28:
            q = " " * rng.randrange(17, 40) + q   # past the fast path's window
        if 0.28 <= x < 0.30:
            q = chr(0xA0) + q                # U+00A0, a non-ASCII space: the general path
        out.append(q.encode("utf-8"))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spans", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5A10B)
    ap.add_argument("--query-share", type=float, default=1 / 3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    from odigos_amd import native
    from odigos_amd.batch import Engine

    if not torch.cuda.is_available():
        print("sqlop_bench: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = "cuda"
    n = args.spans
    rng = random.Random(args.seed)
    pool = query_pool(rng, 4096)
    pool_len = torch.tensor([len(q) for q in pool], dtype=torch.int64, device=dev)
    pool_off = torch.cumsum(pool_len, 0) - pool_len
    pool_bytes = torch.frombuffer(bytearray(b"".join(pool)), dtype=torch.uint8).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    has_q = torch.rand(n, generator=g, device=dev) < args.query_share
    has_op = torch.rand(n, generator=g, device=dev) < 0.02
    idx = torch.randint(0, len(pool), (n,), generator=g, device=dev)
    lens = torch.where(has_q, pool_len[idx], torch.zeros_like(idx))
    offs = torch.cumsum(lens, 0) - lens
    arena_bytes = int(lens.sum().item())
    assert arena_bytes < 0xFFFFFFF0
    arena = torch.zeros((arena_bytes + 15) // 16 * 16 + 32, dtype=torch.uint8, device=dev)
    qi = torch.nonzero(has_q).squeeze(1)
    step = 1 << 20   # the arena in slices of 1M queries: bounded temporaries
    for a in range(0, qi.numel(), step):
        s = qi[a:a + step]
        ln, of = lens[s], offs[s]
        owner = torch.repeat_interleave(torch.arange(s.numel(), device=dev), ln)
        pos = torch.arange(owner.numel(), device=dev) - (of - of[0])[owner]
        arena[int(of[0]):int(of[0]) + owner.numel()] = pool_bytes[pool_off[idx[s]][owner] + pos]
    db_flags = (has_q.to(torch.uint8) * native.DB_HAS_QUERY) | (has_op.to(torch.uint8) * native.DB_HAS_OPNAME)
    db_query = (offs | (lens << 32)).contiguous()   # ose_strref {off, len} as one little-endian word
    R = max(1, n // 200)
    resource = (torch.arange(n, device=dev) // 200).clamp_(max=R - 1).to(torch.int32).contiguous()
    res_ok = (torch.rand(R, generator=g, device=dev) >= 0.05).to(torch.uint8)
    sql_op = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    status = torch.zeros(16, dtype=torch.uint8, device=dev)

    cols, outs = native.Columns(), native.Outputs()
    cols.n_spans, cols.n_resources, cols.arena_bytes = n, R, arena_bytes
    cols.arena, cols.db_flags, cols.db_query = arena.data_ptr(), db_flags.data_ptr(), db_query.data_ptr()
    cols.resource, cols.res_sql_ok = resource.data_ptr(), res_ok.data_ptr()
    outs.sql_op, outs.device_status = sql_op.data_ptr(), status.data_ptr()

    eng = Engine({"odigossqldboperationprocessor": {"exclude": {"language": ["python"]}}})
    L = native.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        native.check(L.ose_process_device(eng.h, C.byref(cols), C.byref(outs), native.STAGE_SQLOP, native.GROUP_TRACE_ID,
                                          None, C.c_void_p(stream)))

    call()
    torch.cuda.synchronize()
    # a sample against the host-compiled classifier
    active = has_q & ~has_op & res_ok[resource.long()].bool()
    sample = torch.nonzero(active).squeeze(1)
    sample = sample[:: max(1, sample.numel() // 2000)][:2000]
    offs_h, lens_h, got = offs[sample].cpu().numpy(), lens[sample].cpu().numpy(), sql_op[sample].cpu().numpy()
    arena_h = arena.cpu().numpy()
    for k in range(sample.numel()):
        q = arena_h[int(offs_h[k]):int(offs_h[k] + lens_h[k])].tobytes()
        if L.osehost_sqlop_detect(q, len(q)) != int(got[k]):
            raise SystemExit(f"sqlop_bench: span {int(sample[k])} {q!r}: kernel {int(got[k])}")
    assert not sql_op[:n][~active].any(), "a skipped span has an operation"
    hist = torch.bincount(sql_op[:n].long(), minlength=8).cpu().tolist()

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

    n_active = int(active.sum().item())
    al = active & (lens > 0)
    chunks = 1 + (((offs & 15) + torch.clamp(lens, max=16)) > 16).to(torch.int64)
    window_bytes = int((chunks[al] * 16).sum().item())
    alg = n * (1 + 8 + 4 + 1) + R + window_bytes
    bw = C.c_double()
    a_ = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    b_ = torch.empty_like(a_)
    native.check(L.osehost_stream_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), 10, C.c_void_p(stream), C.byref(bw)))
    gbs = alg / (med * 1e-3) / 1e9
    out = {
        "tool": "tools/sqlop_bench.py", "kernel": "sqlop_kernel", "device": torch.cuda.get_device_name(0),
        "n_spans": n, "n_resources": R, "spans_with_query": int(has_q.sum().item()), "spans_classified": n_active,
        "arena_bytes": arena_bytes, "mean_query_bytes": arena_bytes / max(1, int(has_q.sum().item())),
        "sql_op_histogram": hist, "calls": args.calls, "warmup": args.warmup, "timing": "device events around each call",
        "ms_per_call": med, "ms_mean": float(ms.mean()), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
        "spans_per_s": n / (med * 1e-3),
        "algorithmic_bytes": alg, "algorithmic_bytes_window_part": window_bytes, "algorithmic_gbs": gbs,
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
