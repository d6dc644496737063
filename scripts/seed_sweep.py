#!/usr/bin/env python3
"""What the seed search costs beside the forward search (dev tool; not the
bench contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto
tables), five legs alternating in one session after a warm-up:

  (a) kfmi_search on exact reads -- the comparison point;
  (b) kfmi_search_seeds, S = 1, on the same exact reads: what the extra state
      of the walk costs on the best case;
  (c) S = 4 on the reads with one substituted base each, uniformly placed;
  (d) S = 4 on the reads with three substituted bases each;
  (e) (c) on both strands.

One JSON line per leg: every repeat's LF-kernel and total device ms
(kfmi_last_timing), their medians and spreads (max - min), the mean number of
records per task, and whether the first --check reads' outputs equal
kfmi_search_seeds_cpu's (compared after the timed region).

  python scripts/seed_sweep.py --out profiles/r10/seeds_r10.jsonl
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
import kstep_fmi as K  # noqa: E402
from kstep_fmi import synth  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def log(*a):
    print(f"[seeds {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def substituted(q: np.ndarray, count: int, seed: int) -> np.ndarray:
    """`count` distinct positions of every read, uniformly drawn, get another base."""
    rng = np.random.default_rng(seed)
    n, m = q.shape
    out = q.copy()
    rows = np.arange(n)
    taken = []
    for j in range(count):
        p = rng.integers(0, m - j, size=n)
        for prev in (np.sort(np.stack(taken), axis=0) if taken else ()):   # skip the positions drawn before, in order
            p = p + (p >= prev)
        taken.append(p)
        out[rows, p] = ACGT[(np.searchsorted(ACGT, out[rows, p]) + rng.integers(1, 4, size=n)) % 4]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--check", type=int, default=100_000, help="reads compared with the host seed search")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    exact = synth.gather_reads(text, synth.read_starts(len(text), a.queries, 100, 10), 100)
    del text
    n, m = exact.shape
    reads = {"exact": exact, "sub1": substituted(exact, 1, 11), "sub3": substituted(exact, 3, 13)}
    log(f"inputs ready: {n} reads of {m} bases")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "m": m, "backend": a.backend, "text_bases": int(idx.header()["bwtsize"]) - 1},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_reads": min(a.check, n)}]

    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    R = K.Results.alloc(n)
    K.transfer_to_gpu(idx, Q["exact"], R)
    for name in ("sub1", "sub3"):
        K.transfer_to_gpu(idx, Q[name], None)
    # leg -> (reads, S, strands); S = 0: the forward search
    legs = {"a: kfmi_search, exact reads": ("exact", 0, K.STRAND_FWD),
            "b: seeds S=1, exact reads": ("exact", 1, K.STRAND_FWD),
            "c: seeds S=4, one substitution": ("sub1", 4, K.STRAND_FWD),
            "d: seeds S=4, three substitutions": ("sub3", 4, K.STRAND_FWD),
            "e: seeds S=4, one substitution, both strands": ("sub1", 4, K.STRAND_BOTH)}
    handles = {}
    for leg, (name, s, strands) in legs.items():
        if s:
            slots = s * (2 if strands == K.STRAND_BOTH else 1) * n
            handles[leg] = (K.Results.alloc(slots), K.Results.alloc(slots))
            for h in handles[leg]:
                K.transfer_to_gpu(idx, None, h)
    lf = {leg: [] for leg in legs}
    tot = {leg: [] for leg in legs}
    for it in range(a.warmup + a.steps):
        for leg, (name, s, strands) in legs.items():
            if s:
                K.search_seeds(idx, Q[name], handles[leg][0], handles[leg][1], s, strands)
            else:
                K.search(idx, Q[name], R)
            if it >= a.warmup:
                lt = K.last_timing()
                lf[leg].append(lt["lf_ms"])
                tot[leg].append(lt["total_ms"])
    log("timed region done; checking against the host")

    c = min(a.check, n)
    for leg, (name, s, strands) in legs.items():
        row = {"leg": leg, "unit": "ms", "lf": [round(x, 3) for x in lf[leg]], "total": [round(x, 3) for x in tot[leg]],
               "lf_median": round(statistics.median(lf[leg]), 3), "lf_spread": round(max(lf[leg]) - min(lf[leg]), 3),
               "total_median": round(statistics.median(tot[leg]), 3),
               "total_spread": round(max(tot[leg]) - min(tot[leg]), 3)}
        sample = np.ascontiguousarray(reads[name][:c])
        if s:
            ns = 2 if strands == K.STRAND_BOTH else 1
            for h in handles[leg]:
                K.transfer_to_cpu(h)
            iv, sp = (h.array().reshape(ns * n, s, 2) for h in handles[leg])
            row["records_per_task"] = round(float(np.count_nonzero(sp[:, :, 1])) / (ns * n), 4)
            row["tasks_with_one_whole_record"] = int(np.count_nonzero((sp[:, 0, 1] == m) & (sp[:, 0, 0] == 0)))
            hiv, hsp = K.search_seeds_array(idx, sample, max_seeds=s, strands=strands, cpu=True)
            row["equals_host_on_sample"] = bool(np.array_equal(iv[:ns * c], hiv) and np.array_equal(sp[:ns * c], hsp))
        else:
            K.transfer_to_cpu(R)
            got = R.array()
            row["nonempty"] = int(np.count_nonzero(got[1::2] > got[0::2]))
            row["equals_host_on_sample"] = bool(np.array_equal(got[:2 * c], K.search_cpu_array(idx, sample)))
        rows.append(row)
        log(json.dumps(row))
    base = rows[1]["lf_median"]
    for row in rows[2:]:
        row["lf_over_leg_a"] = round(row["lf_median"] / base, 4) if base > 0 else None

    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
