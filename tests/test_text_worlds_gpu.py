"""The text kernels on the device over the random worlds of text_worlds.py, one
test per world: the index built at the world's K and d and uploaded afresh on
the world's backend, the world's split class and path chunk set, then the whole
chain with every intermediate handle left on the device --

    kfmi_search_seeds        its records must be the model's seeds
    kfmi_verify_seeds
    kfmi_align_seeds
    kfmi_align_paths         on the align step's hits, and on caller-filled ones
    kfmi_place_windows       on caller-filled windows
    kfmi_align_paths         on the placed records, at the world's band
    on pair worlds, modes 0 and 1:
    kfmi_mate_windows, kfmi_place_windows, kfmi_pair_hits, and kfmi_align_paths on `paired`

-- against the chain of models, bit for bit on both words of every entry.  Every
output handle holds 0xA5A5A5A5 when its call starts, and the handles a call
reads are fetched after it and must hold what they held.

Three worlds in four are uploaded under kfmi_set_jump(0), so the upload builds
no [sa | isa | text] tables and the seed search builds none either (both are
asserted); the first text-kernel call, kfmi_verify_seeds, then builds them
itself, at every d and K, on texts of one base and up (an index of two rows).
Every fourth world (i % 4 == 1) keeps the auto setting, under which the upload
builds the tables and the call finds them there.

The conditions of text_worlds.assert_not_vacuous are asserted on the models
alone before the first device call.  The host forms are held to the same
models by test_text_worlds_host.py and are not consulted here."""
import numpy as np
import pytest

import seed_ref as sr
import text_worlds as tw
from test_verify_gpu import defaults, fresh_upload
from test_window_host import same

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def worlds(kfmi_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    ws = tw.worlds()
    tw.assert_not_vacuous(ws)         # the models and their conditions first
    K.set_device(0)
    backend = K.get_backend()         # every world sets its own; the one in effect comes back after each
    defaults(K)
    K.set_path_chunk(0)
    yield K, ws, backend
    defaults(K)
    K.set_path_chunk(0)
    K.set_backend(backend)


class Handles:
    """Results handles on the index's device."""

    def __init__(self, K, idx):
        self.K, self.idx, self.all = K, idx, []

    def alloc(self, entries, values=FILL):
        h = self.K.Results.alloc(entries)
        self.all.append(h)
        self.K.transfer_to_gpu(self.idx, None, h)
        self.send(h, values)
        return h

    def send(self, h, values=FILL):
        h.array()[:] = values if np.isscalar(values) else np.asarray(values, np.uint32).reshape(-1)
        self.K.results_to_gpu(h)

    def fetch(self, h, shape=(-1, 2)):
        self.K.transfer_to_cpu(h)
        return h.array().copy().reshape(shape)

    def close(self):
        for h in self.all:
            h.close()


def hits_of(B):
    """Caller-filled hits: word x the begin positions, word y the fill (only x is read)."""
    out = np.full((B.size, 2), FILL, np.uint32)
    out[:, 0] = B
    return out


@pytest.mark.parametrize("i", range(tw.WORLDS))
def test_device_chain_equals_the_models(worlds, i):
    K, ws, backend = worlds
    x = ws[i]
    on_demand = i % 4 != 1            # the upload builds no tables: the first text-kernel call has to
    what = dict(world=i, n=x.n, m=x.m, K=x.K, d=x.d, N=x.N, S=x.S, occ=x.occ, band=x.band, strands=x.strands,
                max_mism=x.max_mism, max_edits=x.max_edits, C=x.C, chunk=x.chunk, split=x.split, backend=x.backend)
    T, S, C, m, st = x.T, x.S, x.C, x.m, x.strands
    idx = K.Index.build(x.text.tobytes(), k=x.K, d=x.d)
    Q = K.Queries.from_array(x.q)
    h = Handles(K, idx)
    try:
        defaults(K)
        if on_demand:
            K.set_jump(0)
        fresh_upload(K, idx, x.backend)
        assert (idx.jump_bytes() == 0) == on_demand, (what, "tables after the upload")
        K.set_split_class(x.split)
        K.set_path_chunk(x.chunk)
        K.transfer_to_gpu(idx, Q, None)
        iv, sp = h.alloc(T * S), h.alloc(T * S)

        def seeds_unchanged(after):
            assert np.array_equal(h.fetch(iv, (T, S, 2)), x.iv), (what, after, "seed intervals")
            assert np.array_equal(h.fetch(sp, (T, S, 2)), x.sp), (what, after, "seed spans")

        def paths(hits, B, kind):
            P, G = h.alloc(T), h.alloc(T * C)
            K.align_paths(idx, Q, hits, P, G, st, x.band, x.max_edits, C)
            want_p, want_c = x.paths[kind]
            same(h.fetch(P), want_p, (what, kind, "paths"))
            same(h.fetch(G, (T, 2 * C)), want_c, (what, kind, "cigars"))
            assert np.array_equal(h.fetch(hits)[:, 0], B.astype(np.uint32)), (what, kind, "the hits are read only")

        K.search_seeds(idx, Q, iv, sp, S, st)
        seeds_unchanged("search_seeds")
        assert (idx.jump_bytes() == 0) == on_demand, (what, "tables after the seed search")
        hv, ha = h.alloc(T), h.alloc(T)
        K.verify_seeds(idx, Q, iv, sp, hv, S, st, x.occ, x.max_mism)
        assert idx.jump_bytes() != 0, (what, "no tables after the first text-kernel call")
        same(h.fetch(hv), x.verify, (what, "verify"))
        seeds_unchanged("verify_seeds")
        K.align_seeds(idx, Q, iv, sp, ha, S, st, x.occ, x.band, x.max_edits)
        same(h.fetch(ha), x.align, (what, "align"))
        seeds_unchanged("align_seeds")
        paths(ha, x.B_align, "align")
        same(h.fetch(ha), x.align, (what, "align_paths", "the hits are read only"))
        paths(h.alloc(T, hits_of(x.B_hand)), x.B_hand, "hand")
        W, placed = h.alloc(T, x.windows), h.alloc(T)
        K.place_windows(idx, Q, W, placed, st, x.max_edits)
        same(h.fetch(placed), x.placed, (what, "placed"))
        same(h.fetch(W), x.windows, (what, "the windows are read only"))
        paths(placed, x.B_placed, "placed")
        same(h.fetch(placed), x.placed, (what, "align_paths", "the placed records are read only"))
        for mode in (1, 0) if x.pair else ():
            y = x.modes[mode]
            MW, resc, paired = h.alloc(T), h.alloc(T), h.alloc(T)
            K.mate_windows(idx, ha, MW, m, x.min_frag, x.max_frag, mode)
            same(h.fetch(MW), y.win, (what, "mate windows", mode))
            K.place_windows(idx, Q, MW, resc, sr.BOTH, x.max_edits)
            same(h.fetch(resc), y.resc, (what, "rescued", mode))
            same(h.fetch(MW), y.win, (what, "the mate windows are read only", mode))
            K.pair_hits(idx, ha, resc, paired, m, x.min_frag, x.max_frag)
            same(h.fetch(paired), y.paired, (what, "paired", mode))
            same(h.fetch(resc), y.resc, (what, "the rescued records are read only", mode))
            same(h.fetch(ha), x.align, (what, "the hits are read only", mode))
            if mode == 0:
                paths(paired, x.B_paired, "paired")
                same(h.fetch(paired), y.paired, (what, "align_paths", "the paired records are read only"))
    finally:
        defaults(K)
        K.set_path_chunk(0)
        K.set_backend(backend)
        h.close()
        Q.close()
        idx.close()
