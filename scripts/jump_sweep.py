#!/usr/bin/env python3
"""The text jump over read lengths, and the index upload with and without its
tables (dev tool; DESIGN.md 5a'').

  python3 scripts/jump_sweep.py [--queries 5000000] [--lengths 32,40,48,...] [--uploads 2]

The 3 Gbase recipe text and its K = 2, d = 64 index on the device, task-mid.

Uploads: `--uploads` rounds of free_gpu + transfer_to_gpu of the index under
each setting (no tables; ftab; ftab + skip table; all three), wall time and the
tables' bytes.  One JSON line per (round, setting).

Lengths: per read length m, `queries` reads sampled like the bench's (seed
10); the mean HIP-event LF time of 12 searches after 12 warm-up ones under each
of: the skip walk (set_jump(0)), the jump at any remaining length (jump_min 1),
the jump at the default jump_min, the same from the flat tables
(set_jump_lines(0)) and from the lines with unsplit window loads
(set_jump_lines(2), DESIGN.md 5a'''), the skip walk again; results checked
equal to the first.  One JSON line per m.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "k-step_fm-index_amd"))
import kstep_fmi as K  # noqa: E402
from kstep_fmi import synth  # noqa: E402

LENGTHS = "32,40,48,64,72,80,88,96,100,112,128,144,150,160,240,256"
UPLOADS = (("no tables", 0, 0, 0), ("ftab", "auto", 0, 0), ("ftab, skip", "auto", "auto", 0),
           ("ftab, skip, jump", "auto", "auto", "auto"))


def defaults():
    K.set_ftab("auto")
    K.set_skip("auto")
    K.set_jump("auto")
    K.set_jump_min(K.JUMP_MIN_DEFAULT)
    K.set_jump_lines(1)


def upload_rows(idx, rounds: int):
    for rnd in range(rounds):
        for what, ftab, skip, jump in UPLOADS:
            K.set_ftab(ftab)
            K.set_skip(skip)
            K.set_jump(jump)
            idx.free_gpu()
            t0 = time.perf_counter()
            K.transfer_to_gpu(idx, None, None)
            wall = time.perf_counter() - t0
            print(json.dumps({"round": rnd, "what": what, "upload_s": round(wall, 4),
                              "index_bytes": idx.device_bytes(), "ftab_bytes": idx.ftab_bytes(),
                              "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes(),
                              "jump_line_bytes": idx.jump_line_bytes()}), flush=True)
    defaults()
    idx.free_gpu()
    K.transfer_to_gpu(idx, None, None)


def length_row(idx, text, m: int, nq: int) -> dict:
    reads = synth.gather_reads(text, synth.read_starts(len(text), nq, m, seed=10), m)
    q = K.Queries.from_array(reads)
    r = K.Results.alloc(nq)
    K.transfer_to_gpu(idx, q, r)
    row = {"m": m, "queries": nq, "jump_min_default": K.JUMP_MIN_DEFAULT}
    first = None
    settings = (("skip", 0, K.JUMP_MIN_DEFAULT, 1), ("jump_any", "auto", 1, 1),
                ("jump_default", "auto", K.JUMP_MIN_DEFAULT, 1), ("jump_lines0", "auto", K.JUMP_MIN_DEFAULT, 0),
                ("jump_lines_unsplit", "auto", K.JUMP_MIN_DEFAULT, 2), ("skip_again", 0, K.JUMP_MIN_DEFAULT, 1))
    for name, jump, jmin, lines in settings:
        K.set_jump(jump)
        K.set_jump_min(jmin)
        K.set_jump_lines(lines)
        lf = []
        for _ in range(24):
            K.search(idx, q, r)
            lf.append(K.last_timing()["lf_ms"])
        row[name + "_lf_ms"] = round(float(np.mean(lf[12:])), 4)
        K.transfer_to_cpu(r)
        res = r.array().copy()
        if first is None:
            first = res
        row[name + "_equal"] = bool(np.array_equal(res, first))
    defaults()
    q.close()
    r.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5_000_000)
    ap.add_argument("--lengths", default=LENGTHS)
    ap.add_argument("--uploads", type=int, default=2)
    a = ap.parse_args()
    K.load()
    K.set_device(0)
    K.set_backend("task-mid")
    defaults()
    text = synth.text_3g()
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    K.transfer_to_gpu(idx, None, None)
    upload_rows(idx, a.uploads)
    for m in [int(x) for x in a.lengths.split(",") if x]:
        print(json.dumps(length_row(idx, text, m, a.queries)), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
