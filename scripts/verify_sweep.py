#!/usr/bin/env python3
"""What seed verification costs behind the seed search (dev tool; not the
bench contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto
tables), four legs alternating in one session after a warm-up, each a
kfmi_search_seeds followed by a kfmi_verify_seeds on its handles:

  (a) exact reads, S = 1, max_occ = 1;
  (b) one substituted base per read, S = 4, max_occ = 8;
  (c) three substituted bases per read, S = 4, max_occ = 8;
  (d) (b) on both strands.

One JSON line per leg: every repeat's verify-kernel ms and the seed search's
LF-kernel ms before it (kfmi_last_timing), their medians and spreads
(max - min), the candidates scored, the tasks placed, and the line-request
model of DESIGN.md 5h: a scored candidate is one request for its sa entry plus
the 1 or 2 lines its window spans (counted here from the reported origins'
windows; candidates that lost are taken at the same mean), a candidate that
was skipped is its sa request alone.  The implied request rate stands beside
the text jump's 44.8 G/s (README, round 12).  After the timed region the
mismatch count of every reported origin among the first --check reads is
recounted on the host from the text.

  python scripts/verify_sweep.py --out profiles/r14/verify_r14.jsonl
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "k-step_fm-index_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import kstep_fmi as K  # noqa: E402
from kstep_fmi import synth  # noqa: E402
from seed_sweep import substituted  # noqa: E402

JUMP_REQUESTS_PER_S = 44.8e9     # the text jump's line requests per second, README round 12


def log(*a):
    print(f"[verify {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def code_of(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    b1, f2 = x & 4, x & 2
    return (b1 | np.where(b1 != 0, f2 ^ 2, f2)) >> 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--max-mism", type=int, default=5)
    p.add_argument("--check", type=int, default=100_000, help="reads whose reported origins are recounted on the host")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    exact = synth.gather_reads(text, synth.read_starts(len(text), a.queries, 100, 10), 100)
    n, m = exact.shape
    n_text = int(idx.header()["bwtsize"]) - 1
    reads = {"exact": exact, "sub1": substituted(exact, 1, 11), "sub3": substituted(exact, 3, 13)}
    log(f"inputs ready: {n} reads of {m} bases")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "m": m, "backend": a.backend, "text_bases": n_text, "max_mism": a.max_mism},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_reads": min(a.check, n)}]

    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    # leg -> (reads, S, strands, max_occ)
    legs = {"a: exact reads, S=1, max_occ=1": ("exact", 1, K.STRAND_FWD, 1),
            "b: one substitution, S=4, max_occ=8": ("sub1", 4, K.STRAND_FWD, 8),
            "c: three substitutions, S=4, max_occ=8": ("sub3", 4, K.STRAND_FWD, 8),
            "d: one substitution, S=4, max_occ=8, both strands": ("sub1", 4, K.STRAND_BOTH, 8)}
    handles = {}
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        handles[leg] = (K.Results.alloc(s * ns * n), K.Results.alloc(s * ns * n), K.Results.alloc(ns * n))
        for h in handles[leg]:
            K.transfer_to_gpu(idx, None, h)
    ver = {leg: [] for leg in legs}
    seed = {leg: [] for leg in legs}
    for it in range(a.warmup + a.steps):
        for leg, (name, s, strands, occ) in legs.items():
            iv, sp, hits = handles[leg]
            K.search_seeds(idx, Q[name], iv, sp, s, strands)
            t_seed = K.last_timing()["lf_ms"]
            K.verify_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, a.max_mism)
            if it >= a.warmup:
                seed[leg].append(t_seed)
                ver[leg].append(K.last_timing()["lf_ms"])
    log("timed region done; counting")

    c = min(a.check, n)
    tc = None
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv, sp, hits = handles[leg]
        K.transfer_to_cpu(hits)
        K.transfer_to_cpu(iv)
        origin, mism, multi, scored = K.decode_hits(hits.array())
        ivs = iv.array().reshape(ns * n, s, 2).astype(np.int64)
        listed = int(np.minimum(np.maximum(ivs[:, :, 1] - ivs[:, :, 0], 0), occ).sum())   # rows the slots list: sa requests
        placed = origin >= 0
        # the kernel loads ceil(m / 16) + 1 dwords from dword (n - o - m) / 16 of the stream, which starts at dword
        # 2 * rows of the allocation: the 128-byte lines (32 dwords) those span
        dw = 2 * (n_text + 1) + (n_text - origin[placed] - m) // 16
        lines_per_window = float(np.mean((dw + (m + 15) // 16) // 32 - dw // 32 + 1)) if placed.any() else 1.0
        n_scored = int(scored.sum())
        requests = listed + n_scored * lines_per_window
        med = statistics.median(ver[leg])
        row = {"leg": leg, "unit": "ms", "verify": [round(x, 3) for x in ver[leg]],
               "verify_median": round(med, 3), "verify_spread": round(max(ver[leg]) - min(ver[leg]), 3),
               "seeds_lf": [round(x, 3) for x in seed[leg]], "seeds_lf_median": round(statistics.median(seed[leg]), 3),
               "seeds_lf_spread": round(max(seed[leg]) - min(seed[leg]), 3),
               "tasks": ns * n, "candidates_listed": listed, "candidates_scored": n_scored,
               "tasks_placed": int(placed.sum()), "tasks_multi": int(multi.sum()),
               "mean_mism_of_placed": round(float(mism[placed].mean()), 4) if placed.any() else None,
               "lines_per_window": round(lines_per_window, 4),
               "line_requests_per_scored_candidate": round(requests / n_scored, 4) if n_scored else None,
               "line_requests": int(requests),
               "G_requests_per_s": round(requests / (med / 1e3) / 1e9, 2) if med > 0 else None,
               "text_jump_G_requests_per_s": JUMP_REQUESTS_PER_S / 1e9}
        # the reported origins of the first c reads, recounted from the text on the host
        if tc is None:
            tc = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
        tasks = reads[name][:c]
        if strands == K.STRAND_BOTH:
            both = np.empty((2 * c, m), np.uint8)
            both[0::2], both[1::2] = tasks, K.revcomp(np.ascontiguousarray(tasks))
            tasks = both
        o = origin[:tasks.shape[0]]
        ok = o >= 0
        win = tc[o[ok][:, None] + np.arange(m)[None, :]]
        recount = np.count_nonzero(code_of(win) != code_of(tasks[ok]), axis=1)
        row["recount_equal_on_sample"] = bool(np.array_equal(recount, mism[:tasks.shape[0]][ok]))
        row["sample_placed"] = int(ok.sum())
        rows.append(row)
        log(json.dumps(row))

    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
