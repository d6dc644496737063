"""Place windows on the device (kfmi_place_windows, kfmi_mate_windows) against
the model of window_ref.py, bit for bit on both words of every record, and
against the host form as a cross-check (not as the reference).

The windows are caller-filled and sent up with kfmi_results_to_device, or the
ones kfmi_mate_windows leaves on the device.  `hits` holds 0xA5A5A5A5 when a
call starts.  The non-vacuity conditions are asserted on the model alone in
window_ref.world, before any device call."""
import numpy as np
import pytest

import path_ref as pr
import seed_ref as sr
import verify_ref as vr
import window_ref as wr
from test_verify_gpu import defaults, fresh_upload
from test_window_host import clip_hits, host_place, same

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
EDGE_SIZES = (1, 63, 64, 65, 257, 513)
STRANDS = (sr.BOTH, sr.FWD, sr.REV)


@pytest.fixture(scope="module")
def world(kfmi_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    w = wr.world()                    # the model and its conditions first
    idx = {name: {k: K.Index.build(x["text"].tobytes(), k=k, d=64) for k in (1, 2)} for name, x in w.items()}
    K.set_device(0)
    defaults(K)
    yield K, w, idx
    defaults(K)
    for per_k in idx.values():
        for i in per_k.values():
            i.close()


class Device:
    """Reads, a windows handle and a hits handle on the device."""

    def __init__(self, K, idx, q, strands):
        self.K, self.idx, self.strands = K, idx, strands
        self.T = (2 if strands == sr.BOTH else 1) * q.shape[0]
        self.Q, self.W, self.H = K.Queries.from_array(q), K.Results.alloc(self.T), K.Results.alloc(self.T)
        K.transfer_to_gpu(idx, self.Q, self.W)
        K.transfer_to_gpu(idx, None, self.H)

    def send(self, h, values):
        h.array()[:] = np.asarray(values, np.uint32).reshape(-1) if not np.isscalar(values) else values
        self.K.results_to_gpu(h)

    def fetch(self, h):
        self.K.transfer_to_cpu(h)
        return h.array().copy().reshape(-1, 2)

    def place(self, me, win=None, strands=None):
        if win is not None:
            self.send(self.W, win)
        self.send(self.H, FILL)
        self.K.place_windows(self.idx, self.Q, self.W, self.H, self.strands if strands is None else strands, me)
        return self.fetch(self.H)

    def close(self):
        for h in (self.Q, self.W, self.H):
            h.close()


def check_case(K, x, idx, m, what, strands=STRANDS, all_bounds=True, host=False):
    q, tasks, win, tags, b = x["cases"][m]
    for st in strands:
        rows = vr.strand_rows(st)
        d = Device(K, idx, q, st)
        try:
            for me in wr.edit_bounds(m) if all_bounds and st == sr.BOTH else (8,):
                got = d.place(me, win[rows])
                same(got, wr.place(b, win[rows], me, rows), (what, m, st, me))
                if host and me == 8:
                    same(got, host_place(K, x["text"], q, st, win[rows], me), (what, "host form", m, st))
        finally:
            d.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", list(wr.texts()))
def test_task_mid_every_length(world, text, k):
    """task-mid at K = 1, 2: every word count (m = 1 .. 256 across the 32 / 64 /
    128 edges), both stagings, every strand mode, windows of 1, 33, 400 and
    KFMI_WINDOW_MAX_LEN bases, at both text ends, empty and past the text, reads
    with substitutions, short and long indels, max_edits 0, 1, 8 and m."""
    K, w, idx = world
    try:
        defaults(K)
        fresh_upload(K, idx[text][k], "task-mid")
        for m in wr.LENGTHS:
            check_case(K, w[text], idx[text][k], m, (text, k), host=(text == "n1009" and m in (33, 100)))
        assert idx[text][k].jump_bytes() != 0            # the call built the text jump's tables
    finally:
        defaults(K)


def test_task_backend(world):
    """The reference's own layout (tag 101): the "task" backend at K = 2."""
    K, w, idx = world
    try:
        defaults(K)
        fresh_upload(K, idx["n1005"][2], "task")
        for m in (33, 100, 256):
            check_case(K, w["n1005"], idx["n1005"][2], m, "task", all_bounds=False)
    finally:
        defaults(K)
        fresh_upload(K, idx["n1005"][2], "task-mid")


def test_split_classes(world):
    """The loads under the 16-lane group mask (class 4), then the plain form (class 1) on the same upload."""
    K, w, idx = world
    try:
        defaults(K)
        fresh_upload(K, idx["tandem"][2], "task-mid")
        for cls in (4, 1):
            K.set_split_class(cls)
            for m in (17, 64, 100, 256):
                check_case(K, w["tandem"], idx["tandem"][2], m, ("class", cls), all_bounds=False)
    finally:
        defaults(K)


def test_batch_edges(world):
    """Batches that end inside a wave, a staging round or a block, in all three
    strand modes: lanes with windows of 400 positions next to lanes with len = 0."""
    K, w, idx = world
    x = w["n1009"]
    q, tasks, win, b = wr.batch_case(x)
    assert (win[0::3, 1] == 400).all() and (win[1::3, 1] == 0).all()
    K.set_backend("task-mid")
    for num in EDGE_SIZES:
        for st in STRANDS:
            ns = 2 if st == sr.BOTH else 1
            rows = slice(0, 2 * num) if st == sr.BOTH else slice(0 if st == sr.FWD else 1, 2 * num, 2)
            d = Device(K, idx["n1009"][2], np.ascontiguousarray(q[:num]), st)
            try:
                assert d.T == ns * num
                for me in (3, 100):
                    same(d.place(me, win[rows]), wr.place(b, win[rows], me, rows), (num, st, me))
            finally:
                d.close()


def test_windows_left_by_mate_windows(world):
    """kfmi_mate_windows on the device equals the model, modes 0 and 1, windows
    clipped at 0 and at n among them; kfmi_place_windows then reads those
    windows where they lie."""
    K, w, idx = world
    x = w["n1009"]
    n = x["world"].n
    hits = clip_hits(n)
    K.set_backend("task-mid")
    reads = np.ascontiguousarray(x["cases"][100][0][:hits.shape[0] // 2])
    tasks = sr.tasks_of(reads, sr.BOTH)
    b = wr.Begins(x["world"], tasks)
    d = Device(K, idx["n1009"][2], reads, sr.BOTH)
    src = K.Results.alloc(d.T)
    try:
        K.transfer_to_gpu(idx["n1009"][2], None, src)
        d.send(src, hits)
        for mode in (0, 1):
            d.send(d.W, FILL)
            K.mate_windows(idx["n1009"][2], src, d.W, 100, 200, 400, mode)
            t = K.last_timing()
            assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
            want = wr.mate_windows(hits, n, 100, 200, 400, mode)
            same(d.fetch(d.W), want, ("mate windows", mode))
            same(d.fetch(src), hits, "the hits are read only")
            same(d.place(100), wr.place(b, want, 100), ("placed in the mate windows", mode))
        assert (want[:, 1] > 0).sum() >= 6
    finally:
        src.close()
        d.close()


def test_paths_of_placed_records(world):
    """kfmi_align_paths takes the records as they are: at band 15, D <= E
    whenever E <= 15 and B + m <= n (kstep_fmi.h, "align paths")."""
    K, w, idx = world
    x = w["n1008"]
    n = x["world"].n
    K.set_backend("task-mid")
    sure = 0
    for m in (33, 100, 256):
        q, tasks, win, tags, b = x["cases"][m]
        d = Device(K, idx["n1008"][2], q, sr.BOTH)
        P, G = K.Results.alloc(d.T), K.Results.alloc(d.T * 32)
        try:
            K.transfer_to_gpu(idx["n1008"][2], None, P)
            K.transfer_to_gpu(idx["n1008"][2], None, G)
            hits = d.place(m, win)
            same(hits, wr.place(b, win, m), (m, "placed"))
            K.align_paths(idx["n1008"][2], d.Q, d.H, P, G, sr.BOTH, 15, m, 32)
            paths = d.fetch(P)
            E, B = (hits[:, 1] & wr.EDITS).astype(np.int64), hits[:, 0].astype(np.int64)
            ok = (hits[:, 0] != wr.NONE) & (E <= 15) & (B + m <= n)
            assert (paths[ok, 0] != pr.NONE).all() and ((paths[ok, 1] & pr.EDITS_MASK) <= E[ok]).all(), m
            sure += int(ok.sum())
            long = [t for t, tag in enumerate(tags) if tag.split("/")[0] in ("del18", "ins17") and hits[t, 0] != wr.NONE]
            assert m < 64 or long                        # indels past the band: placed here, whatever the paths say
        finally:
            for h in (P, G):
                h.close()
            d.close()
    assert sure > 100


def refused(K, idx, q, strands, lens=33, sizes=None, call_strands=None):
    """(error code, whether anything on the device changed)."""
    d = Device(K, idx, q, strands)
    n_w, n_h = sizes or (d.T, d.T)
    hs = [K.Results.alloc(n) for n in (n_w, n_h)]
    try:
        for h in hs:
            K.transfer_to_gpu(idx, None, h)
        filled = FILL
        try:
            hs[0].array()[0::2] = 5
            hs[0].array()[1::2] = lens
            K.results_to_gpu(hs[0])
            hs[1].array()[:] = FILL
            K.results_to_gpu(hs[1])
        except K.KfmiError as e:                  # device-group handles: the zeros of the transfer
            assert e.code == 19
            filled = 0
        before = hs[0].array().copy()
        code = 0
        try:
            K.place_windows(idx, d.Q, hs[0], hs[1], strands if call_strands is None else call_strands, 3)
        except K.KfmiError as e:
            code = e.code
        for h in hs:
            K.transfer_to_cpu(h)
        changed = bool((hs[1].array() != filled).any()) or (filled != 0 and not np.array_equal(hs[0].array(), before))
        return code, changed
    finally:
        for h in hs:
            h.close()
        d.close()


def record_refused(K, idx, call, sizes, *args):
    hs = [K.Results.alloc(s) for s in sizes]
    try:
        filled = FILL
        for h in hs:
            K.transfer_to_gpu(idx, None, h)
        try:
            for h in hs:
                h.array()[:] = FILL
                K.results_to_gpu(h)
        except K.KfmiError as e:
            assert e.code == 19
            filled = 0
        code = 0
        try:
            call(idx, *hs, *args)
        except K.KfmiError as e:
            code = e.code
        for h in hs:
            K.transfer_to_cpu(h)
        return code, any(bool((h.array() != filled).any()) for h in hs)
    finally:
        for h in hs:
            h.close()


def test_refusals_write_nothing(world):
    K, w, idx = world
    x = w["n1005"]
    q = np.ascontiguousarray(np.tile(x["cases"][100][0], (3, 1))[:130])     # three waves
    nq = q.shape[0]
    idx2 = idx["n1005"][2]
    idx4 = K.Index.build(x["text"].tobytes(), k=4, d=64)
    try:
        defaults(K)
        K.set_backend("task-mid")
        assert refused(K, idx2, q, K.STRAND_BOTH) == (0, True)
        assert refused(K, idx2, q, K.STRAND_FWD, lens=wr.MAX_LEN) == (0, True)
        lens = np.full(nq, 33, np.int64)
        lens[nq - 1] = wr.MAX_LEN + 1                    # one entry too long, in the last wave
        assert refused(K, idx2, q, K.STRAND_FWD, lens=lens) == (33, False)
        lens[nq - 1], lens[0] = 33, 0xFFFFFFFF
        assert refused(K, idx2, q, K.STRAND_FWD, lens=lens) == (33, False)
        for sizes in ((nq + 1, nq), (nq, nq - 1), (2 * nq, 2 * nq)):
            assert refused(K, idx2, q, K.STRAND_FWD, sizes=sizes) == (33, False), sizes
        for cs in (0, 4, K.STRAND_BOTH):
            assert refused(K, idx2, q, K.STRAND_FWD, call_strands=cs) == (33, False), cs
        long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
        assert refused(K, idx2, long, K.STRAND_FWD) == (33, False)
        # the pair calls: odd num, min_frag < m, a range of fragments wider than a window, an unknown mode
        assert record_refused(K, idx2, K.mate_windows, (8, 8), 100, 200, 400, 0) == (0, True)
        assert record_refused(K, idx2, K.pair_hits, (8, 8, 8), 100, 200, 400) == (0, True)
        for args in ((100, 99, 400, 0), (100, 300, 299, 0), (100, 200, 200 + wr.MAX_LEN, 0), (100, 200, 400, 2)):
            assert record_refused(K, idx2, K.mate_windows, (8, 8), *args) == (33, False), args
            if args[3] == 0:
                assert record_refused(K, idx2, K.pair_hits, (8, 8, 8), *args[:3]) == (33, False), args
        assert record_refused(K, idx2, K.mate_windows, (6, 6), 100, 200, 400, 0) == (33, False)
        assert record_refused(K, idx2, K.mate_windows, (8, 12), 100, 200, 400, 0) == (33, False)
        assert record_refused(K, idx2, K.pair_hits, (6, 6, 6), 100, 200, 400) == (33, False)
        assert record_refused(K, idx2, K.pair_hits, (8, 8, 12), 100, 200, 400) == (33, False)
        for backend, i in (("coop-mid", idx2), ("task-ac-mid", idx2), ("task-grp", idx4)):
            K.set_backend(backend)
            assert refused(K, i, q, K.STRAND_FWD) == (19, False), backend
            assert refused(K, i, q, K.STRAND_BOTH) == (19, False), backend
            assert record_refused(K, i, K.mate_windows, (8, 8), 100, 200, 400, 0) == (19, False), backend
            assert record_refused(K, i, K.pair_hits, (8, 8, 8), 100, 200, 400) == (19, False), backend
        K.set_backend("task-mid")
        K.set_devices([0, 0])
        assert refused(K, idx2, q, K.STRAND_FWD) == (19, False)
        K.set_devices([])
    finally:
        defaults(K)
        idx2.free_gpu()
        idx4.close()


def test_last_timing_reports_the_window_kernel(world):
    K, w, idx = world
    x = w["n1005"]
    K.set_backend("task-mid")
    q, tasks, win, tags, b = x["cases"][100]
    d = Device(K, idx["n1005"][2], q, sr.BOTH)
    try:
        d.place(8, win)
        t = K.last_timing()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
    finally:
        d.close()
