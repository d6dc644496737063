"""The text kernels' host forms on the random worlds of text_worlds.py, no GPU
needed: over every world -- texts of one base and up, reads longer than the
text, every index geometry, every call parameter drawn together -- each host
form equals its model bit for bit, on fresh handles pre-filled with 0xA5A5A5A5:

* kfmi_search_seeds_cpu equals the model's seeds (seed_ref.reference on the
  brute-force suffix array);
* kfmi_verify_seeds_cpu, kfmi_align_seeds_cpu, kfmi_align_paths_cpu (from the
  align records' begin positions, from caller-filled ones, from the placed
  records' and from the paired records'), kfmi_place_windows_cpu,
  kfmi_mate_windows_cpu in modes 0 and 1 and kfmi_pair_hits_cpu equal their
  models; every fourth world verifies and aligns once more on a suffix array
  with rows that have no suffix and a hand-made slot over the whole array;
* path_ref.check_properties holds on every host record with a path.

The conditions of text_worlds.assert_not_vacuous are asserted on the models
alone before the first library call."""
import numpy as np
import pytest

import path_ref as pr
import text_worlds as tw
from test_align_host import host_hits as align_hits
from test_path_host import Host as PathHost
from test_verify_host import host_hits as verify_hits
from test_window_host import host_mate, host_pair, host_place, same

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def worlds():
    ws = tw.worlds()
    tw.assert_not_vacuous(ws)         # the models and their conditions first
    return ws


def host_seeds(K, x):
    """kfmi_search_seeds_cpu on the world's index and reads: (intervals, spans), uint32 [T, S, 2]."""
    idx = K.Index.build(x.text.tobytes(), k=x.K, d=x.d)
    Q, iv, sp = K.Queries.from_array(x.q), K.Results.alloc(x.T * x.S), K.Results.alloc(x.T * x.S)
    try:
        iv.array()[:] = FILL
        sp.array()[:] = FILL
        K.search_seeds_cpu(idx, Q, iv, sp, x.S, x.strands)
        return iv.array().copy().reshape(x.T, x.S, 2), sp.array().copy().reshape(x.T, x.S, 2)
    finally:
        for h in (Q, iv, sp, idx):
            h.close()


@pytest.mark.parametrize("i", range(tw.WORLDS))
def test_host_forms_equal_the_models(kfmi_mod, worlds, i):
    K, x = kfmi_mod, worlds[i]
    what = dict(world=i, n=x.n, m=x.m, K=x.K, d=x.d, N=x.N, S=x.S, occ=x.occ, band=x.band, strands=x.strands,
                max_mism=x.max_mism, max_edits=x.max_edits, C=x.C)
    iv, sp = host_seeds(K, x)
    assert np.array_equal(iv, x.iv), (what, "seed intervals")
    assert np.array_equal(sp, x.sp), (what, "seed spans")
    same(verify_hits(K, x.w, x.q, x.iv, x.sp, x.S, x.strands, x.occ, x.max_mism), x.verify, (what, "verify"))
    same(align_hits(K, x.w, x.q, x.iv, x.sp, x.S, x.strands, x.occ, x.band, x.max_edits), x.align, (what, "align"))
    if x.holes is not None:
        h = x.holes
        same(verify_hits(K, x.w, x.q, h.iv, h.sp, x.S, x.strands, x.occ, x.max_mism, sa=h.sa), h.verify, (what, "verify, holes"))
        same(align_hits(K, x.w, x.q, h.iv, h.sp, x.S, x.strands, x.occ, x.band, x.max_edits, sa=h.sa), h.align,
             (what, "align, holes"))
    same(host_place(K, x.text, x.q, x.strands, x.windows, x.max_edits), x.placed, (what, "placed"))
    for mode, y in x.modes.items():
        same(host_mate(K, x.n, x.align, x.m, x.min_frag, x.max_frag, mode), y.win, (what, "mate windows", mode))
        same(host_place(K, x.text, x.q, x.strands, y.win, x.max_edits), y.resc, (what, "rescued", mode))
        same(host_pair(K, x.align, y.resc, x.m, x.min_frag, x.max_frag), y.paired, (what, "paired", mode))
    ph = PathHost(K, x.text, x.q, x.strands)
    try:
        for kind, p in x.walks.items():
            got_p, got_c = ph.paths(p.B, x.band, x.max_edits, x.C)
            want_p, want_c = x.paths[kind]
            same(got_p, want_p, (what, kind, "paths"))
            same(got_c, want_c, (what, kind, "cigars"))
            pr.check_properties(x.w, x.tasks, p.B, x.band, got_p, got_c, (what, kind))
    finally:
        ph.close()
