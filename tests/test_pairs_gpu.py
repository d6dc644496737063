"""Pairs on the device (kfmi_mate_windows, kfmi_place_windows, kfmi_pair_hits,
map_pairs_array) against the chain of models and host forms of pair_chain.py,
bit for bit at every step: simulated pairs at fragment lengths min_frag,
max_frag and one inside, both orientations, clean mates, mates with a one-base
and with a 10-base indel (the seeds' band misses them, the rescue brings them
back: pair_chain.check asserts that on the models before the device is asked),
discordant pairs; the hand-made table of the pair order; modes 0 and 1."""
import re

import numpy as np
import pytest

import pair_chain as pc
import path_ref as pr
import seed_ref as sr
import window_ref as wr
from test_verify_gpu import defaults
from test_window_host import same

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def world(kfmi_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    chains = {(name, k): pc.chain(K, name, t, k) for name, t in pc.texts().items() for k in (1, 2)}   # the models first
    K.set_device(0)
    defaults(K)
    K.set_backend("task-mid")
    yield K, chains
    defaults(K)
    for c in chains.values():
        c["idx"].free_gpu()


class Handles:
    """n results handles of T entries on the index's device."""

    def __init__(self, K, idx, T, n):
        self.K, self.hs = K, [K.Results.alloc(T) for _ in range(n)]
        for h in self.hs:
            K.transfer_to_gpu(idx, None, h)

    def send(self, i, values):
        self.hs[i].array()[:] = values if np.isscalar(values) else np.asarray(values, np.uint32).reshape(-1)
        self.K.results_to_gpu(self.hs[i])

    def fetch(self, i):
        self.K.transfer_to_cpu(self.hs[i])
        return self.hs[i].array().copy().reshape(-1, 2)

    def close(self):
        for h in self.hs:
            h.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", ["r1003", "n1009"])
def test_every_step_equals_the_chain(world, text, k):
    """Seeds and align on the device, then per mode the windows, the rescued
    records and the paired records, each left on the device for the next call."""
    K, chains = world
    c = chains[text, k]
    idx, q = c["idx"], c["q"]
    T = 2 * q.shape[0]
    m, lo, hi = wr.PAIR_M, wr.PAIR_MIN, wr.PAIR_MAX
    Q = K.Queries.from_array(q)
    iv, sp = K.Results.alloc(pc.S * T), K.Results.alloc(pc.S * T)
    K.transfer_to_gpu(idx, Q, iv)
    K.transfer_to_gpu(idx, None, sp)
    h = Handles(K, idx, T, 4)                            # hits, windows, rescued, paired
    try:
        K.search_seeds(idx, Q, iv, sp, pc.S, sr.BOTH)
        K.align_seeds(idx, Q, iv, sp, h.hs[0], pc.S, sr.BOTH, pc.OCC, wr.PAIR_BAND, wr.PAIR_EDITS)
        same(h.fetch(0), c["hits"], (text, k, "the align step's hits"))
        for mode in (0, 1):
            x = c["modes"][mode]
            for i in (1, 2, 3):
                h.send(i, FILL)
            K.mate_windows(idx, h.hs[0], h.hs[1], m, lo, hi, mode)
            K.place_windows(idx, Q, h.hs[1], h.hs[2], sr.BOTH, wr.PAIR_EDITS)
            K.pair_hits(idx, h.hs[0], h.hs[2], h.hs[3], m, lo, hi)
            t = K.last_timing()
            assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
            same(h.fetch(1), x["win"], (text, k, mode, "windows"))
            same(h.fetch(2), x["resc"], (text, k, mode, "rescued"))
            same(h.fetch(3), x["paired"], (text, k, mode, "paired"))
            same(h.fetch(0), c["hits"], (text, k, mode, "the hits are read only"))
    finally:
        h.close()
        for r in (Q, iv, sp):
            r.close()


def test_pair_table(world):
    """One pair per key of the pair order, both orientations, every way to have no admissible combination."""
    K, chains = world
    idx = chains["r1003", 2]["idx"]
    hits, resc, names, want = wr.pair_table()
    h = Handles(K, idx, hits.shape[0], 3)
    try:
        h.send(0, hits)
        h.send(1, resc)
        h.send(2, FILL)
        K.pair_hits(idx, h.hs[0], h.hs[1], h.hs[2], 100, 200, 400)
        got = h.fetch(2)
        for p, name in enumerate(names):
            same(got[4 * p:4 * p + 4], want[4 * p:4 * p + 4], name)
    finally:
        h.close()


def test_pair_batches(world):
    """257 pairs (1,028 tasks, a block boundary inside) of shuffled table rows."""
    K, chains = world
    idx = chains["r1003", 2]["idx"]
    hits, resc, names, _ = wr.pair_table()
    pick = np.random.default_rng(85_000).integers(0, len(names), size=257)
    hits = hits.reshape(-1, 4, 2)[pick].reshape(-1, 2)
    resc = resc.reshape(-1, 4, 2)[pick].reshape(-1, 2)
    h = Handles(K, idx, hits.shape[0], 4)
    try:
        h.send(0, hits)
        h.send(1, resc)
        h.send(2, FILL)
        h.send(3, FILL)
        K.pair_hits(idx, h.hs[0], h.hs[1], h.hs[2], 100, 200, 400)
        same(h.fetch(2), wr.pair_hits(hits, resc, 100, 200, 400), "pairs")
        K.mate_windows(idx, h.hs[0], h.hs[3], 100, 200, 400, 1)
        same(h.fetch(3), wr.mate_windows(hits, 1_003, 100, 200, 400, 1), "windows")
    finally:
        h.close()


@pytest.mark.parametrize("text", ["r1003", "n1009"])
def test_map_pairs_array(world, text):
    """The whole chain in one call equals the chain of models and host forms, read by read."""
    K, chains = world
    c = chains[text, 2]
    try:
        begin, end, strand, edits, flags, cigar = K.map_pairs_array(
            c["idx"], c["q"], wr.PAIR_MIN, wr.PAIR_MAX, "task-mid", max_seeds=pc.S, max_occ=pc.OCC, band=wr.PAIR_BAND,
            max_edits=wr.PAIR_EDITS, cigar_entries=pc.C)
        wb, we, ws, wed, wf, t, has_path = pc.per_read(c)
        for got, want, what in ((begin, wb, "begin"), (end, we, "end"), (strand, ws, "strand"), (edits, wed, "edits"),
                                (flags, wf, "flags")):
            assert np.array_equal(got, want), (text, what, np.flatnonzero(got != want)[:8])
        code = {v: k for k, v in K.CIGAR_OPS.items()}
        for i in range(len(cigar)):
            if not has_path[i]:
                assert cigar[i] == "*", (i, cigar[i])
                continue
            runs = [int(a) << 4 | code[b] for a, b in re.findall(r"(\d+)([IDX=])", cigar[i])]
            n_runs = (int(c["paths"][t[i], 1]) >> pr.RUNS_SHIFT) & 0xFFF
            assert runs == [int(v) for v in c["cigars"][t[i], :n_runs]], (i, cigar[i])
        assert (flags & wr.PROPER).astype(bool).sum() > len(cigar) // 2 and (flags & wr.RESCUED).astype(bool).any()
        assert any("D" in s for s in cigar) and any("I" in s for s in cigar)
    finally:
        defaults(K)
        K.set_backend("task-mid")
