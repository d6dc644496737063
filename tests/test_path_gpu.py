"""Align paths on the device (kfmi_align_paths) against the model of
path_ref.py, bit for bit on `paths` and on every word of `cigars`, and against
the host form as a cross-check (not as the reference).

The hits the device walks from are the ones kfmi_align_seeds (band 0 also
kfmi_verify_seeds) leaves on the device -- test_align_gpu.py pins them to
align_ref.records, which is where the model's begin positions come from, and
every test here asserts that again before it uses them -- or caller-filled ones
sent up with kfmi_results_to_device.  `paths` and `cigars` hold 0xA5A5A5A5
when a call starts.  The non-vacuity conditions are asserted on the model
alone in path_ref.world, before any device call."""
import re

import numpy as np
import pytest

import align_ref as ar
import path_ref as pr
import seed_ref as sr
import verify_ref as vr
from test_align_gpu import Device as AlignDevice
from test_path_host import Host, cuts, same
from test_verify_gpu import defaults, fresh_upload

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
EDGE_SIZES = (1, 63, 64, 65, 257, 513)


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    w = pr.world(K, oracle_mod)       # the model and its conditions first
    K.set_device(0)
    defaults(K)
    K.set_path_chunk(0)
    yield K, w
    defaults(K)
    K.set_path_chunk(0)
    for x in w.values():
        for i in x["idx"].values():
            i.free_gpu()


class Device(AlignDevice):
    """test_align_gpu.Device with a paths handle and, per call, a cigars handle of C entries per task."""

    def __init__(self, K, idx, q, s, strands):
        super().__init__(K, idx, q, s, strands)
        self.P = K.Results.alloc(self.T)
        K.transfer_to_gpu(idx, None, self.P)

    def fill(self, h):
        h.array()[:] = FILL
        self.K.results_to_gpu(h)

    def set_hits(self, B):
        """Caller-filled hits: word x the begin positions, word y the fill."""
        a = self.hits.array().reshape(self.T, 2)
        a[:, 0], a[:, 1] = B, FILL
        self.K.results_to_gpu(self.hits)

    def paths(self, band, me, C, strands=None):
        G = self.K.Results.alloc(self.T * C)
        try:
            self.K.transfer_to_gpu(self.idx, None, G)
            self.fill(G)
            self.fill(self.P)
            self.K.align_paths(self.idx, self.Q, self.hits, self.P, G, self.strands if strands is None else strands, band, me, C)
            self.K.transfer_to_cpu(self.P)
            self.K.transfer_to_cpu(G)
            return self.P.array().copy().reshape(self.T, 2), G.array().copy().reshape(self.T, 2 * C)
        finally:
            G.close()

    def close(self):
        self.P.close()
        super().close()


def check_case(K, x, text, label, k, what, bands=pr.BANDS, strands=ar.STRANDS, kinds=("seed", "hand"), all_cuts=True, host=False):
    """Device against model on one case of the world: per strand mode one upload, the seed search, then per band the
    align step (its hits stay on the device) or caller-filled hits, and the paths under every cut."""
    m, q, both, per_k = x["cases"][label]
    idx = x["idx"][k]
    for st in strands:
        rows = vr.strand_rows(st)
        d = Device(K, idx, q, 8, st)
        try:
            d.seeds()
            for band in bands:
                for kind in kinds:
                    if st != sr.BOTH and kind == "hand":
                        continue
                    B, E, p = pr.walk_of(text, label, k, band, kind)
                    if kind == "seed":
                        got = d.align(8, band, m)
                        same(got, ar.records(per_k[k][2], 8, 8, band, m, rows), (what, label, st, band, "the align step's hits"))
                    else:
                        d.set_hits(B[rows])
                    for me, C in cuts(m) if all_cuts and st == sr.BOTH else ((m, 2),):
                        got_p, got_c = d.paths(band, me, C)
                        want_p, want_c = pr.records(p, me, C, rows)
                        same(got_p, want_p, (what, label, st, band, kind, me, C, "paths"))
                        same(got_c, want_c, (what, label, st, band, kind, me, C, "cigars"))
                        if host and me == m:
                            hp, hc = host_paths(K, x, q, st, B[rows], band, me, C)
                            same(got_p, hp, (what, label, st, band, kind, me, C, "host form, paths"))
                            same(got_c, hc, (what, label, st, band, kind, me, C, "host form, cigars"))
        finally:
            d.close()


def host_paths(K, x, q, st, B, band, me, C):
    h = Host(K, x["text"], q, st)
    try:
        return h.paths(B, band, me, C)
    finally:
        h.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", ["main", "n1005", "n1008", "n1009"])
def test_task_mid_every_length(world, text, k):
    """task-mid at K = 1, 2: both stagings at every length (the dword edges,
    the 8 | 16 word switch), bands 0, 1, 3, 8 and 15, every strand mode, the
    align step's hits and -- at K = 2 -- caller-filled ones with begin positions
    off either end of the text, C = 1, 2, 32 and max_edits 0, 1, m."""
    K, w = world
    x = w[text]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][k], "task-mid")
        for label in x["cases"]:
            check_case(K, x, text, label, k, (text, k), kinds=("seed", "hand") if k == 2 else ("seed",),
                       host=(text == "n1009" and label == 100))
    finally:
        defaults(K)


@pytest.mark.parametrize("text", list(pr.AW_TEXTS))
def test_low_complexity_texts(world, text):
    """allA and the text with tandem stretches: the walk's priority decides where a gap sits."""
    K, w = world
    x = w[text]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")
        for label in x["cases"]:
            check_case(K, x, text, label, 2, text)
    finally:
        defaults(K)


def test_band_zero_on_the_verify_hits(world):
    """Band 0 on the hits kfmi_verify_seeds leaves: m diagonal ops, D the Hamming count of the verify's record."""
    K, w = world
    K.set_backend("task-mid")
    x = w["n1009"]
    for label in (17, 100, 129, 256):
        m, q, both, per_k = x["cases"][label]
        d = Device(K, x["idx"][2], q, 8, sr.BOTH)
        try:
            d.seeds()
            hits = d.verify(8, m)
            B, E, p = pr.walk_of("n1009", label, 2, 0, "seed")
            assert np.array_equal(hits[:, 0], B.astype(np.uint32))
            got_p, got_c = d.paths(0, m, 32)
            want_p, want_c = pr.records(p, m, 32)
            same(got_p, want_p, (label, "paths"))
            same(got_c, want_c, (label, "cigars"))
            placed = hits[:, 0] != pr.NONE
            assert placed.any() and np.array_equal(got_p[placed, 1] & pr.EDITS_MASK, hits[placed, 1] & ar.EDIT_MASK)
            assert not ((got_c & 15) == pr.OP_I).any() and not ((got_c & 15) == pr.OP_D).any()
        finally:
            d.close()


def test_task_backend(world):
    """The reference's own layout (tag 101): the "task" backend at K = 2, one length."""
    K, w = world
    x = w["main"]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task")
        check_case(K, x, "main", 100, 2, "task", bands=(3, 15), all_cuts=False)
    finally:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")


def test_split_classes(world):
    """The loads under the 16-lane group mask (class 4), then the plain form (class 1) on the same upload."""
    K, w = world
    x = w["n1005"]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")
        for cls in (4, 1):
            K.set_split_class(cls)
            for label in (100, 101, 129, 256):
                check_case(K, x, "n1005", label, 2, ("class", cls), bands=(1, 15), all_cuts=False)
    finally:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")


@pytest.fixture(scope="module")
def edges(world):
    """513 shuffled reads of 100 bases of the main text: caller-filled hits at band 3, every third task without a
    path (NONE, B > n, B - c > w by turns), so path-less lanes stand next to lanes with paths in every wave."""
    _, w = world
    x = w["main"]
    m, q0, both0, per_k = x["cases"][100]
    B0, _ = pr.seed_hits(per_k[2][2], 3, m, vr.strand_rows(sr.FWD))
    pick = np.random.default_rng(100).permutation(np.arange(2 * q0.shape[0]) % q0.shape[0])[:513]
    q = np.ascontiguousarray(q0[pick])
    n = x["world"].n
    out = {}
    for st in ar.STRANDS:
        ns = 2 if st == sr.BOTH else 1
        tasks = sr.tasks_of(q, st)
        # the forward task's begin position on every strand: the reverse strand's tasks are placed where they do not lie
        B = np.repeat(B0[pick], ns)
        t = np.arange(B.size)
        B = np.where(t % 3 == 1, np.asarray([pr.NONE, n + 1, n - m + 4])[(t // 3) % 3], B)
        p = pr.Walk(x["world"], tasks, B, 3)
        assert p.ok[0::3].sum() > p.ok.size // 6 and not p.ok[1::3].any()
        out[st] = (tasks, B, p)
    return q, out


def test_batch_edges_and_chunks(world, edges):
    """Batches that end inside a wave, a staging round or a block, in all three
    strand modes, on handles pre-filled with 0xA5A5A5A5; then 257 tasks in
    chunks of 64 (kfmi_set_path_chunk), which must equal the single launch."""
    K, w = world
    q, per_st = edges
    idx = w["main"]["idx"][2]
    K.set_backend("task-mid")
    try:
        for num in EDGE_SIZES:
            for st in ar.STRANDS:
                tasks, B, p = per_st[st]
                T = (2 if st == sr.BOTH else 1) * num
                d = Device(K, idx, np.ascontiguousarray(q[:num]), 1, st)
                try:
                    d.set_hits(B[:T])
                    for me, C in ((100, 32), (3, 2)):
                        got_p, got_c = d.paths(3, me, C)
                        want_p, want_c = pr.records(p, me, C, slice(0, T))
                        same(got_p, want_p, (num, st, me, C, "paths"))
                        same(got_c, want_c, (num, st, me, C, "cigars"))
                    if num == 257:
                        K.set_path_chunk(64)
                        again_p, again_c = d.paths(3, 3, 2)
                        K.set_path_chunk(0)
                        same(again_p, got_p, (num, st, "chunks of 64, paths"))
                        same(again_c, got_c, (num, st, "chunks of 64, cigars"))
                finally:
                    d.close()
    finally:
        K.set_path_chunk(0)


def refused(K, idx, q, strands, band=3, C=2, sizes=None, call_strands=None):
    """(error code, whether anything on the device changed)."""
    d = Device(K, idx, q, 1, strands)
    T = d.T
    n_h, n_p, n_c = sizes or (T, T, T * C)
    hs = [K.Results.alloc(n) for n in (n_h, n_p, n_c)]
    try:
        for h in hs:
            K.transfer_to_gpu(idx, None, h)
        filled = FILL
        try:
            for h in hs:
                h.array()[:] = FILL
                K.results_to_gpu(h)
        except K.KfmiError as e:                  # device-group handles: the zeros of the transfer
            assert e.code == 19
            filled = 0
        code = 0
        try:
            K.align_paths(idx, d.Q, hs[0], hs[1], hs[2], strands if call_strands is None else call_strands, band, 3, C)
        except K.KfmiError as e:
            code = e.code
        for h in hs:
            K.transfer_to_cpu(h)
        return code, any(bool((h.array() != filled).any()) for h in hs)
    finally:
        for h in hs:
            h.close()
        d.close()


def test_refusals_write_nothing(world):
    K, w = world
    t = w["main"]["text"]
    q = w["main"]["cases"][100][1][:64]
    idx2 = w["main"]["idx"][2]
    idx4 = K.Index.build(t.tobytes(), k=4, d=64)
    try:
        defaults(K)
        K.set_backend("task-mid")
        assert refused(K, idx2, q, K.STRAND_BOTH) == (0, True)
        assert refused(K, idx2, q, K.STRAND_FWD, band=16) == (33, False)
        assert refused(K, idx2, q, K.STRAND_FWD, band=0xFFFFFFFF) == (33, False)
        assert refused(K, idx2, q, K.STRAND_FWD, C=33) == (33, False)
        for sizes in ((65, 64, 128), (64, 63, 128), (64, 64, 129), (64, 64, 64), (128, 128, 256)):
            assert refused(K, idx2, q, K.STRAND_FWD, sizes=sizes) == (33, False), sizes
        for cs in (0, 4, K.STRAND_BOTH):
            assert refused(K, idx2, q, K.STRAND_FWD, call_strands=cs) == (33, False), cs
        # C = 0: the cigars handle of the call has T * 1 entries, the argument says 0
        dd = Device(K, idx2, q, 1, K.STRAND_FWD)
        G = K.Results.alloc(dd.T)
        try:
            K.transfer_to_gpu(idx2, None, G)
            dd.fill(G)
            dd.fill(dd.P)
            with pytest.raises(K.KfmiError) as e:
                K.align_paths(idx2, dd.Q, dd.hits, dd.P, G, K.STRAND_FWD, 3, 3, 0)
            assert e.value.code == 33
            K.transfer_to_cpu(G)
            K.transfer_to_cpu(dd.P)
            assert (G.array() == FILL).all() and (dd.P.array() == FILL).all()
        finally:
            G.close()
            dd.close()
        for backend, idx in (("coop-mid", idx2), ("task-ac-mid", idx2), ("task-grp", idx4)):
            K.set_backend(backend)
            assert refused(K, idx, q, K.STRAND_FWD) == (19, False), backend
            assert refused(K, idx, q, K.STRAND_BOTH) == (19, False), backend
        K.set_backend("task-mid")
        K.set_devices([0, 0])
        assert refused(K, idx2, q, K.STRAND_FWD) == (19, False)
        K.set_devices([])
        long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
        assert refused(K, idx2, long, K.STRAND_FWD) == (33, False)
    finally:
        defaults(K)
        idx2.free_gpu()
        idx4.close()


def test_last_timing_reports_the_paths_kernel(world):
    K, w = world
    x = w["main"]
    K.set_backend("task-mid")
    m, q, both, per_k = x["cases"][100]
    d = Device(K, x["idx"][2], q, 8, sr.BOTH)
    try:
        d.seeds()
        d.align(8, 3, m)
        d.paths(3, m, 4)
        t = K.last_timing()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
    finally:
        d.close()


def test_map_paths_array(world):
    """End to end on reads with one indel each: every task that is placed replays, with at most one edit."""
    K, w = world
    x = w["main"]
    t, m = x["text"], 100
    extra = ar.indel_reads(t, m, 17_000 + m + 1)[:2 * len(ar.pinned(m))]      # one base deleted, one inserted, by turns
    try:
        defaults(K)
        begin, end, edits, cigar = K.map_paths_array(x["idx"][2], extra, "task-mid", max_seeds=4, max_occ=8, band=3,
                                                     max_edits=3, cigar_entries=4)
        fwd = slice(0, None, 2)
        assert (begin[fwd] >= 0).all() and (edits[fwd] <= 1).all() and (edits[fwd] == 1).any()
        assert any("D" in c for c in cigar[fwd]) and any("I" in c for c in cigar[fwd])
        tasks = sr.tasks_of(extra, sr.BOTH)
        placed = np.flatnonzero(begin >= 0)
        paths = np.zeros((begin.size, 2), np.uint32)
        paths[:, 0] = pr.NONE
        words = np.zeros((begin.size, 8), np.uint32)
        code = {v: k for k, v in K.CIGAR_OPS.items()}
        for i in placed:
            runs = [(int(a), code[b]) for a, b in re.findall(r"(\d+)([IDX=])", cigar[i])]
            words[i, :len(runs)] = [ln << 4 | op for ln, op in runs]
            paths[i] = (end[i], edits[i] | len(runs) << pr.RUNS_SHIFT)
        assert pr.check_properties(x["world"], tasks, np.where(begin < 0, pr.NONE, begin), 3, paths, words, "map_paths_array") == placed.size
    finally:
        defaults(K)
