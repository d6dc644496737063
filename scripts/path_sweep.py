#!/usr/bin/env python3
"""What the alignment paths cost behind seeds and align (dev tool; not the
bench contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto tables),
legs alternating in one session after a warm-up.  A leg is a kfmi_search_seeds,
a kfmi_align_seeds at band 3 on its handles and a kfmi_align_paths at band 3 on
the hits that leaves:

  exact reads (S = 1, max_occ = 1); one substituted base per read; one 1-base
  indel per read; the indel reads on both strands (S = 4, max_occ = 8); exact
  reads of 150 and of 256 bases (S = 1, max_occ = 1).

Beside each leg's paths kernel stands the align kernel at S = 1, max_occ = 1
and the same band on the same reads: one dynamic programme per task there and
here, so the difference is the row store and the walk.  The call's wall time
less its kernel time is what the workspace's allocation and release cost.

One JSON line per leg: every repeat's ms, the medians, the tasks with a path,
their edits and runs.  After the timed region the first --check records of
every leg are recomputed on the host (kfmi_align_paths_cpu on the device's own
hits).

  python scripts/path_sweep.py --out profiles/r22/paths_r22.jsonl
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
    print(f"[paths {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--band", type=int, default=3)
    p.add_argument("--max-edits", type=int, default=3)
    p.add_argument("--entries", type=int, default=4, help="cigar_entries: 2 * entries runs per task")
    p.add_argument("--check", type=int, default=100_000, help="records recomputed on the host per leg")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    log("text ready; building the index on the device")
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    n_text = int(idx.header()["bwtsize"]) - 1
    reads = {}
    for m in (100, 150, 256):
        starts = synth.read_starts(len(text), a.queries, m, 10 + m)
        reads["exact%d" % m] = synth.gather_reads(text, starts, m)
        if m == 100:
            reads["sub1"] = substituted(reads["exact100"], 1, 11)
            reads["indel"] = with_indel(text, np.minimum(np.asarray(starts), n_text - m - 1), m, 12)
    n, C = a.queries, a.entries
    log(f"inputs ready: {n} reads per set")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "backend": a.backend, "text_bases": n_text, "band": a.band, "max_edits": a.max_edits,
                       "cigar_entries": C},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_records": min(a.check, n)}]
    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    # leg -> (reads, S, strands, max_occ)
    legs = {"exact, S=1, occ=1": ("exact100", 1, K.STRAND_FWD, 1),
            "one substitution, S=4, occ=8": ("sub1", 4, K.STRAND_FWD, 8),
            "one indel, S=4, occ=8": ("indel", 4, K.STRAND_FWD, 8),
            "one indel, S=4, occ=8, both strands": ("indel", 4, K.STRAND_BOTH, 8),
            "150 bases, exact, S=1, occ=1": ("exact150", 1, K.STRAND_FWD, 1),
            "256 bases, exact, S=1, occ=1": ("exact256", 1, K.STRAND_FWD, 1)}
    # one set of handles per (S, ns), shared by the legs of that size, and one at S = 1 for the align kernel beside it
    shared = {}
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        for key, sizes in (((s, ns), (s * ns * n, s * ns * n, ns * n, ns * n, C * ns * n)), ((1, ns, "one"), (ns * n, ns * n, ns * n))):
            if key not in shared:
                shared[key] = hs = tuple(K.Results.alloc(x) for x in sizes)
                for h in hs:
                    K.transfer_to_gpu(idx, None, h)
    ms = {leg: {"align": [], "align_s1_occ1": [], "paths": [], "paths_call_wall": []} for leg in legs}

    def run(leg, out=None):
        name, s, strands, occ = legs[leg]
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv1, sp1, hits1 = shared[(1, ns, "one")]
        K.search_seeds(idx, Q[name], iv1, sp1, 1, strands)
        K.align_seeds(idx, Q[name], iv1, sp1, hits1, 1, strands, 1, a.band, a.max_edits)
        one = K.last_timing()["lf_ms"]
        iv, sp, hits, paths, cig = shared[(s, ns)]
        K.search_seeds(idx, Q[name], iv, sp, s, strands)
        K.align_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, a.band, a.max_edits)
        al = K.last_timing()["lf_ms"]
        t0 = time.perf_counter()
        K.align_paths(idx, Q[name], hits, paths, cig, strands, a.band, a.max_edits, C)
        wall = 1e3 * (time.perf_counter() - t0)
        pa = K.last_timing()["lf_ms"]
        if out is not None:
            out["align"].append(al)
            out["align_s1_occ1"].append(one)
            out["paths"].append(pa)
            out["paths_call_wall"].append(wall)

    for it in range(a.warmup + a.steps):
        for leg in legs:
            run(leg, ms[leg] if it >= a.warmup else None)
    log("timed region done; counting and checking")
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv, sp, hits, paths, cig = shared[(s, ns)]
        run(leg)
        for h in (hits, paths, cig):
            K.transfer_to_cpu(h)
        end, edits, runs, over = K.decode_paths(paths.array())
        has = end >= 0
        med = {k: statistics.median(v) for k, v in ms[leg].items()}
        row = {"leg": leg, "unit": "ms", "tasks": ns * n}
        for k, v in ms[leg].items():
            row[k] = [round(x, 3) for x in v]
            row[k + "_median"] = round(med[k], 3)
        row.update({"paths_minus_align_s1_occ1": round(med["paths"] - med["align_s1_occ1"], 3),
                    "paths_over_align_s1_occ1": round(med["paths"] / med["align_s1_occ1"], 3) if med["align_s1_occ1"] else None,
                    "allocation_share_of_call": round(1.0 - med["paths"] / med["paths_call_wall"], 4) if med["paths_call_wall"] else None,
                    "tasks_with_path": int(has.sum()), "share_with_path": round(float(has.mean()), 6),
                    "mean_edits": round(float(edits[has].mean()), 4) if has.any() else None,
                    "mean_runs": round(float(runs[has].mean()), 4) if has.any() else None, "overflowed": int(over.sum())})
        c = min(a.check, n)
        qc = K.Queries.from_array(np.ascontiguousarray(reads[name][:c]))
        hc = [K.Results.alloc(ns * c), K.Results.alloc(ns * c), K.Results.alloc(C * ns * c)]
        try:
            hc[0].array()[:] = hits.array()[:2 * ns * c]
            K.align_paths_cpu(text, qc, hc[0], hc[1], hc[2], strands, a.band, a.max_edits, C)
            row["host_equal_on_sample"] = bool(np.array_equal(hc[1].array(), paths.array()[:2 * ns * c]) and
                                               np.array_equal(hc[2].array(), cig.array()[:2 * C * ns * c]))
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
