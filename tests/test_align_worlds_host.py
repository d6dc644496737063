"""Align seeds on the host on the low-complexity worlds of align_worlds.py, no
GPU needed: kfmi_align_seeds_cpu equals the model of align_ref.py bit for bit
on both words of every record -- six texts (all-A, CG repeated, period 3, two
letters, runs, tandem repeats), lengths 17, 100, 129, 256, every band 0 .. 15,
max_edits in {0, 1, m}; the direct-origin handles (forward tasks), the real
seeds under FWD and BOTH with max_occ 1, 8 and 256, at
K = 1 where the world has them; the full text-end set at m = 100 and the batch
of 513 tasks.  The non-vacuity conditions hold on the model alone
(align_worlds.world asserts them before any library call)."""
import numpy as np
import pytest

import align_ref as ar
import align_worlds as aw
import seed_ref as sr
import verify_ref as vr
from test_align_host import Host
from test_verify_host import same


@pytest.fixture(scope="module")
def world(kfmi_mod):
    return aw.world(kfmi_mod)


@pytest.mark.parametrize("text", list(aw.texts()))
def test_host_equals_the_model(kfmi_mod, world, text):
    K, x = kfmi_mod, world[text]
    for m, c in x["cases"].items():
        q, iv, sp, a = c["direct"]
        h = Host(K, x["world"], q, iv, sp, 8, sr.FWD)
        try:
            for band in aw.BANDS:
                for me in ar.edit_bounds(m):
                    same(h.align(256, band, me), ar.records(a, 8, 256, band, me), (text, "direct", m, band, me))
        finally:
            h.close()
        rq, both, per_k = c["real"]
        for k, (riv, rsp, ra) in per_k.items():
            for strands in (sr.FWD, sr.BOTH):
                rows = vr.strand_rows(strands)
                h = Host(K, x["world"], rq, np.ascontiguousarray(riv[rows]), np.ascontiguousarray(rsp[rows]), 8, strands)
                try:
                    for band in aw.BANDS:
                        for occ in aw.OCCS:
                            for me in ar.edit_bounds(m):
                                same(h.align(occ, band, me), ar.records(ra, 8, occ, band, me, rows),
                                     (text, "real", k, m, strands, occ, band, me))
                finally:
                    h.close()


def test_every_text_end_origin(kfmi_mod, world):
    """The 16 first and 16 last origins x every pinned position x {deleted, inserted} at m = 100, every band."""
    x = world["two"]
    q, iv, sp, a = aw.ends_world(x["world"])
    h = Host(kfmi_mod, x["world"], q, iv, sp, 8, sr.FWD)
    try:
        for band in aw.BANDS:
            for me in (1, 100):
                same(h.align(8, band, me), ar.records(a, 8, 8, band, me), ("ends", band, me))
    finally:
        h.close()


def test_batch_of_513(kfmi_mod, world):
    x = world["cg"]
    q, iv, sp, a = aw.batch_world(x["world"], x["cases"][100]["direct"][0])
    h = Host(kfmi_mod, x["world"], q, iv, sp, 8, sr.FWD)
    try:
        same(h.align(256, aw.BATCH_BAND, 100), ar.records(a, 8, 256, aw.BATCH_BAND, 100), "batch")
    finally:
        h.close()
