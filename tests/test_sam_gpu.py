"""SAM lines on the device (kfmi_sam_lines) against the host form and the model
of sam_ref.py, byte for byte, offsets included.

The handles are those kfmi_align_paths leaves on the device from caller-filled
hits (sam_ref.World places each read); the path records are checked against
the host form's before they are used, and one task's words are rewritten on the
way to hold an X run before a D run (sam_ref.swap_first_dx), which the paths
kernel never produces.  The conditions of sam_ref.REQUIRED are asserted on the
model alone in sam_ref.world, before any device call."""
import ctypes

import numpy as np
import pytest

import sam_ref as sm
from test_verify_gpu import defaults, fresh_upload

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257)   # wave and block edges


@pytest.fixture(scope="module")
def world(kfmi_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ws = sm.world(K)                  # the model and its conditions first
    K.set_device(0)
    defaults(K)
    K.set_path_chunk(0)
    K.set_sam_form(0)
    idx = {m: K.Index.build(ws[m].text, k=2, d=64) for m in ws}
    for i in idx.values():
        fresh_upload(K, i, "task-mid")
    yield K, ws, idx
    defaults(K)
    K.set_path_chunk(0)
    K.set_sam_form(0)
    for i in idx.values():
        i.free_gpu()
        i.close()


class Chain:
    """One batch on both sides: sam_ref.HostChain, and the same handles on the device behind kfmi_align_paths."""

    def __init__(self, K, idx, w, num, strands, band, C):
        self.K, self.idx, self.w, self.strands, self.band, self.C = K, idx, w, strands, band, C
        self.host = sm.HostChain(K, w, num, strands, band, C, True)
        h = self.host
        self.Q = K.Queries.from_array(h.reads)
        self.H, self.P, self.G, self.U = (K.Results.alloc(h.T), K.Results.alloc(h.T), K.Results.alloc(h.T * C),
                                          K.Results.alloc(h.T))
        K.transfer_to_gpu(idx, self.Q, self.H)
        for r in (self.P, self.G, self.U):
            K.transfer_to_gpu(idx, None, r)
        a = self.H.array().reshape(h.T, 2)
        a[:, 0], a[:, 1] = h.B, 0xA5A5A5A5
        self.U.array()[:] = sm.task_quals(h.T)
        K.results_to_gpu(self.H)
        K.results_to_gpu(self.U)
        K.align_paths(idx, self.Q, self.H, self.P, self.G, strands, band, w.m, C)
        K.transfer_to_cpu(self.P)
        K.transfer_to_cpu(self.G)
        if sm.swap_first_dx(w.text, h.reads, strands, self.H.array(), self.P.array(), self.G.array(), C):
            K.results_to_gpu(self.G)
        _, hp, hg, _ = h.records()
        assert np.array_equal(self.P.array(), hp) and np.array_equal(self.G.array(), hg), "the path records differ"
        self.ct = K.Contigs.create(w.table.names, w.table.begins, w.table.lengths)

    def check(self, options, base, quals, what):
        """Device, host form and model agree; returns the model's lines."""
        K, h = self.K, self.host
        hits, paths, cig, u = h.records()
        want = sm.model_lines(self.w.text, self.w.table, h.reads, hits, paths, cig, u if quals else None, self.strands,
                              self.C, self.band, options, base)
        got = K.sam_lines(self.idx, self.Q, self.ct, self.H, self.P, self.G, self.U if quals else None, self.strands,
                          self.C, self.band, options, base)
        ref = K.sam_lines_cpu(self.w.text, h.Q, self.ct, h.H, h.P, h.G, h.U if quals else None, self.strands, self.C,
                              self.band, options, base)
        try:
            assert got.num == len(want) == ref.num, what
            assert np.array_equal(got.offsets(), sm.offsets_of(want)), what
            assert np.array_equal(got.offsets(), ref.offsets()), what
            text = got.text()
            assert text == ref.text(), what
            assert text == b"".join(want), what
        finally:
            got.close()
            ref.close()
        return want

    def close(self):
        for x in (self.Q, self.H, self.P, self.G, self.U, self.ct):
            x.close()
        self.host.close()


def replay_all(lines, w) -> int:
    done = 0
    for ln in lines:
        if ln.split(b"\t")[1] != b"4":
            sm.replay(ln, w.table, w.text)
            done += 1
    return done


@pytest.mark.parametrize("strands", [sm.FWD, sm.REV, sm.BOTH])
@pytest.mark.parametrize("m", [20, 100, 256])
def test_device_equals_host_and_model(world, m, strands):
    """Read counts at the wave and block edges; at m = 256 a wave's 64 lines exceed one 16 KB tile, so the rounds and
    the tile-edge decision run; both option values, quals given and NULL, name_base 0 and 10**19 (whose line offsets
    are no multiples of 16: asserted)."""
    K, ws, idx = world
    w, mapped, ragged = ws[m], 0, False
    for num in COUNTS:
        c = Chain(K, idx[m], w, num, strands, 3, 8)
        try:
            for options, base, quals in ((0, 0, True), (sm.CIGAR_M, 10**19, False)):
                want = c.check(options, base, quals, (m, strands, num, options, base, quals))
                mapped += replay_all(want, w)
                ragged = ragged or bool((sm.offsets_of(want)[1:4] % 16).any())
        finally:
            c.close()
    assert mapped >= 8 and ragged   # every batch of 63 reads and more holds a read of either strand that maps


def test_a_wave_takes_several_rounds(world):
    """m = 256, one strand: 64 lines of more than 256 bytes each are more than one tile."""
    K, ws, idx = world
    c = Chain(K, idx[256], ws[256], 65, sm.FWD, 15, 8)
    try:
        want = c.check(0, 10**19, True, "rounds")
        assert sum(len(x) for x in want[:64]) > 16384
    finally:
        c.close()


@pytest.mark.parametrize("form", [0, 1])
def test_knobs_change_no_byte(world, knobs, form):
    """Split classes 4 and 1, kfmi_set_path_chunk(64) upstream, and the lane-per-line form of the write pass."""
    K, ws, idx = world
    try:
        K.set_sam_form(form)
        for split in (4, 1):
            knobs.split(split)
            K.set_path_chunk(64)
            for m, band in ((100, 3), (256, 15)):
                c = Chain(K, idx[m], ws[m], 257, sm.BOTH, band, 8)
                try:
                    c.check(0, 12345, True, (form, split, m))
                    c.check(sm.CIGAR_M, 0, False, (form, split, m))
                finally:
                    c.close()
    finally:
        K.set_sam_form(0)
        K.set_path_chunk(0)


def test_small_c_and_band_0(world):
    """C = 1 (OVERFLOW lines) and band 0, every strand mode, m = 1 included."""
    K, ws, idx = world
    for m in (1, 100):
        for strands in (sm.FWD, sm.REV, sm.BOTH):
            for band, C in ((3, 1), (0, 8)):
                c = Chain(K, idx[m], ws[m], 65, strands, band, C)
                try:
                    c.check(0, 7, True, (m, strands, band, C))
                finally:
                    c.close()


def test_timing(world):
    K, ws, idx = world
    c = Chain(K, idx[100], ws[100], 257, sm.BOTH, 3, 8)
    try:
        s = K.sam_lines(idx[100], c.Q, c.ct, c.H, c.P, c.G, c.U, sm.BOTH, 8, 3)
        t, parts = K.last_timing(), K.sam_last_passes()
        s.close()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
        assert all(x > 0 for x in parts) and abs(sum(parts) - t["total_ms"]) < 1e-3
    finally:
        c.close()


def test_map_sam_array(world):
    """End to end on a task-mid K = 2 index: the device chain against the chain of host forms."""
    K, ws, idx = world
    w = ws[100]
    ct = K.Contigs.create(w.table.names, w.table.begins, w.table.lengths)
    host = K.Index.build(w.text, k=2, d=64, sa_rate=1)
    try:
        for mapq, options in ((True, 0), (False, sm.CIGAR_M)):
            kw = dict(max_seeds=4, strands=sm.BOTH, max_occ=8, band=3, max_edits=6, cigar_entries=8, mapq=mapq,
                      options=options, name_base=1000)
            got = K.map_sam_array(idx[100], w.reads, ct, "task-mid", **kw)
            want = K.map_sam_array(host, w.reads, ct, cpu=True, text=w.text, **kw)
            assert got == want
            head = w.table.header()
            assert got.startswith(head)
            assert replay_all(got[len(head):].splitlines(keepends=True), w) > 20
    finally:
        host.close()
        ct.close()


def test_refusals(world):
    """A host-only handle, wrong sizes, a table ending past n: nothing is created."""
    K, ws, idx = world
    w = ws[20]
    c = Chain(K, idx[20], w, 5, sm.BOTH, 3, 4)
    past = K.Contigs.create(["z"], [0], [sm.N_TEXT + 1])
    lone, odd = K.Results.alloc(c.host.T), K.Results.alloc(c.host.T + 1)
    K.transfer_to_gpu(idx[20], None, odd)
    L = K.load()

    def call(ct=c.ct, hits=c.H, paths=c.P, cig=c.G, quals=c.U, strands=sm.BOTH, C=4, band=3, options=0, base=0):
        out = ctypes.c_void_p(0x1234)
        code = L.kfmi_sam_lines(idx[20].ptr, c.Q.ptr, ct.ptr, hits.ptr, paths.ptr, cig.ptr, quals.ptr if quals else None,
                                strands, C, band, options, base, ctypes.byref(out))
        if code == 0:
            L.kfmi_sam_free(ctypes.byref(out))
        return code, out.value

    try:
        assert call()[0] == 0
        assert call(hits=lone) == (34, 0x1234) and call(quals=lone) == (34, 0x1234)
        for kw in (dict(ct=past), dict(hits=odd), dict(paths=odd), dict(quals=odd), dict(C=5), dict(strands=sm.FWD),
                   dict(options=2), dict(base=2**64 - 5), dict(band=16), dict(paths=c.H), dict(quals=c.G)):
            assert call(**kw) == (33, 0x1234), kw
    finally:
        for x in (past, lone, odd):
            x.close()
        c.close()
