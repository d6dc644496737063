#!/usr/bin/env python3
"""What the second placement costs behind the align (dev tool; not the bench
contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto tables),
legs alternating in one session after a warm-up, on the legs of
scripts/align_sweep.py.  Each leg is a kfmi_align_seeds followed by a
kfmi_align_second and a kfmi_map_quality on the same handles, so that every
figure of the second pass stands beside the align kernel's time of the same
session:

  (a) exact reads, S = 1, max_occ = 1, band 3: uniquely mapping reads, where the
      second pass should cost about the sa loads alone;
  (b) one substituted base per read, S = 4, max_occ = 8, band 3;
  (c) one 1-base indel per read, S = 4, max_occ = 8, band 3;
  (d) (c) on both strands;
  (e) the exact reads under piece seeds, 4 pieces, max_occ = 8, band 3: every
      piece leads to the read's own origin, so every candidate is near X.

One JSON line per leg: every repeat's kernel ms of the three calls, the medians
and spreads (max - min), second / align, the candidates counted, the tasks with
a second, the quality histogram.  After the timed region the first --check
records of every leg are recomputed on the host (kfmi_align_second_cpu and
kfmi_map_quality_cpu on the device's own records and the suffix array read
back from the device).

  python scripts/second_sweep.py --out profiles/r26/second_r26.jsonl
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
from align_sweep import with_indel  # noqa: E402
from seed_sweep import substituted  # noqa: E402


def log(*a):
    print(f"[second {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--max-edits", type=int, default=3)
    p.add_argument("--max-second", type=int, default=6)
    p.add_argument("--check", type=int, default=100_000, help="records recomputed on the host per leg")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    n_text = int(idx.header()["bwtsize"]) - 1
    m, n = 100, a.queries
    starts = synth.read_starts(len(text), n, m, 10 + m)
    reads = {"exact": synth.gather_reads(text, starts, m)}
    reads["sub1"] = substituted(reads["exact"], 1, 11)
    reads["indel"] = with_indel(text, np.minimum(np.asarray(starts), n_text - m - 1), m, 12)
    log(f"inputs ready: {n} reads per set")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "read_len": m, "backend": a.backend, "text_bases": n_text, "max_edits": a.max_edits,
                       "max_second": a.max_second},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_records": min(a.check, n)}]
    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    # leg -> (reads, S, strands, max_occ, band, piece seeds)
    legs = {"a: exact, S=1, occ=1, band 3": ("exact", 1, K.STRAND_FWD, 1, 3, False),
            "b: one substitution, S=4, occ=8, band 3": ("sub1", 4, K.STRAND_FWD, 8, 3, False),
            "c: one indel, S=4, occ=8, band 3": ("indel", 4, K.STRAND_FWD, 8, 3, False),
            "d: one indel, S=4, occ=8, band 3, both strands": ("indel", 4, K.STRAND_BOTH, 8, 3, False),
            "e: exact, 4 piece seeds, occ=8, band 3": ("exact", 4, K.STRAND_FWD, 8, 3, True)}
    H = {}
    for leg, (name, s, strands, occ, band, pieces) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        H[leg] = hs = [K.Results.alloc(s * ns * n), K.Results.alloc(s * ns * n)] + [K.Results.alloc(ns * n) for _ in range(3)]
        for h in hs:
            K.transfer_to_gpu(idx, None, h)
        if pieces:                                 # the seeds of a leg do not change between its repeats
            K.piece_seeds(idx, reads[name], s, strands, hs[0], hs[1])
        else:
            K.search_seeds(idx, Q[name], hs[0], hs[1], s, strands)
    ms = {leg: {"align": [], "second": [], "quality": []} for leg in legs}

    def run(leg):
        name, s, strands, occ, band, _ = legs[leg]
        iv, sp, hits, sec, ql = H[leg]
        out = {}
        K.align_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, band, a.max_edits)
        out["align"] = K.last_timing()["lf_ms"]
        K.align_second(idx, Q[name], iv, sp, hits, sec, s, strands, occ, band, a.max_second)
        out["second"] = K.last_timing()["lf_ms"]
        K.map_quality(idx, hits, sec, ql, strands, a.max_second)
        out["quality"] = K.last_timing()["lf_ms"]
        return out

    for it in range(a.warmup + a.steps):
        for leg in legs:
            t = run(leg)
            if it >= a.warmup:
                for k, v in t.items():
                    ms[leg][k].append(v)
    log("timed region done; counting and checking")
    sa = idx.jump_tables()[0]
    for leg, (name, s, strands, occ, band, pieces) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        hs = H[leg]
        run(leg)
        for h in hs:
            K.transfer_to_cpu(h)
        origin, edits, multi, scored = K.decode_hits(hs[2].array())
        begin, e2, multi2, trunc, counted = K.decode_second(hs[3].array())
        qual = hs[4].array().reshape(-1, 2)[:, 0]
        med = {k: statistics.median(v) for k, v in ms[leg].items()}
        row = {"leg": leg, "unit": "ms", "tasks": ns * n}
        for k, v in ms[leg].items():
            row[k + "_kernel"] = [round(x, 3) for x in v]
            row[k + "_median"] = round(med[k], 3)
            row[k + "_spread"] = round(max(v) - min(v), 3)
        row.update({"second_over_align": round(med["second"] / med["align"], 3) if med["align"] else None,
                    "candidates_scored": int(scored.sum()), "candidates_counted": int(counted.sum()),
                    "tasks_placed": int((origin >= 0).sum()), "tasks_with_second": int((begin >= 0).sum()),
                    "tasks_truncated": int(trunc.sum()),
                    "quality_histogram": {str(int(v)): int(c) for v, c in zip(*np.unique(qual, return_counts=True))}})
        c = min(a.check, n)
        qc = K.Queries.from_array(np.ascontiguousarray(reads[name][:c]))
        hc = [K.Results.alloc(s * ns * c), K.Results.alloc(s * ns * c)] + [K.Results.alloc(ns * c) for _ in range(3)]
        try:
            hc[0].array()[:] = hs[0].array()[:2 * s * ns * c]
            hc[1].array()[:] = hs[1].array()[:2 * s * ns * c]
            hc[2].array()[:] = hs[2].array()[:2 * ns * c]
            K.align_second_cpu(text, sa, qc, hc[0], hc[1], hc[2], hc[3], s, strands, occ, band, a.max_second)
            K.map_quality_cpu(hc[2], hc[3], hc[4], strands, a.max_second)
            row["host_equal_on_sample"] = bool(np.array_equal(hc[3].array(), hs[3].array()[:2 * ns * c]) and
                                               np.array_equal(hc[4].array(), hs[4].array()[:2 * ns * c]))
        finally:
            qc.close()
            for h in hc:
                h.close()
        rows.append(row)
        log(json.dumps(row))
    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
