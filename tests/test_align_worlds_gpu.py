"""Align seeds on the device (kfmi_align_seeds) on the low-complexity worlds of
align_worlds.py against the model of align_ref.py, bit for bit on both words
of every record: homopolymers, short tandem repeats and two-letter text, every
band 0 .. 15, placements on the band's edge, indels of w and w + 1 bases, paths
that leave the band, every text-end origin at m = 100.

Two kinds of handles per (text, length): direct origins (slots filled on the
host and transferred, one row each) and real seeds (kfmi_search_seeds' records
on the device, checked here against seed_ref.reference's, which is what the
model's candidates come from).  The non-vacuity conditions are asserted on the
model alone in align_worlds.world, before any device call.  The host form is
not consulted."""
import numpy as np
import pytest

import align_ref as ar
import align_worlds as aw
import seed_ref as sr
import verify_ref as vr
from test_align_gpu import Device, defaults, fresh_upload, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(kfmi_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    w = aw.world(K)                   # the model and its conditions first
    K.set_device(0)
    defaults(K)
    yield K, w
    defaults(K)
    for x in w.values():
        for i in x["idx"].values():
            i.free_gpu()


def direct_device(K, idx, q, iv, sp):
    """The reads and hand-filled slots on the device, forward tasks; the hits hold 0xA5A5A5A5."""
    d = Device(K, idx, q, 8, sr.FWD)
    d.iv.array()[:] = iv.reshape(-1)
    d.sp.array()[:] = sp.reshape(-1)
    K.results_to_gpu(d.iv)
    K.results_to_gpu(d.sp)
    return d


def seeded_device(K, idx, q, riv, rsp, strands, what):
    """The reads and the device's own seed records, which must be the reference's."""
    rows = vr.strand_rows(strands)
    d = Device(K, idx, q, 8, strands)
    try:
        d.seeds()
        K.transfer_to_cpu(d.iv)
        K.transfer_to_cpu(d.sp)
        assert np.array_equal(d.iv.array().reshape(d.T, 8, 2), riv[rows]), (what, "seed intervals")
        assert np.array_equal(d.sp.array().reshape(d.T, 8, 2), rsp[rows]), (what, "seed spans")
    except BaseException:
        d.close()
        raise
    return d


def check_direct(K, x, k, m, bands, what):
    q, iv, sp, a = x["cases"][m]["direct"]
    d = direct_device(K, x["idx"][k], q, iv, sp)
    try:
        for band in bands:
            occ = aw.OCCS[band % 3]               # one row per slot: max_occ cuts nothing
            for me in ar.edit_bounds(m):
                same(d.align(occ, band, me), ar.records(a, 8, 256, band, me), (what, "direct", m, occ, band, me))
    finally:
        d.close()


def check_real(K, x, k, m, bands, strands, what, occs=aw.OCCS):
    rq, both, per_k = x["cases"][m]["real"]
    riv, rsp, a = per_k[k]
    for st in strands:
        rows = vr.strand_rows(st)
        d = seeded_device(K, x["idx"][k], rq, riv, rsp, st, (what, m, st))
        try:
            for band in bands:
                for occ in occs:
                    for me in ar.edit_bounds(m):
                        same(d.align(occ, band, me), ar.records(a, 8, occ, band, me, rows), (what, "real", m, st, occ, band, me))
        finally:
            d.close()


@pytest.mark.parametrize("text", list(aw.texts()))
def test_task_mid_every_band(world, text):
    """task-mid at K = 2: every length, every band 0 .. 15, both kinds of
    handles, max_occ 1, 8, 256, max_edits 0, 1, m, FWD and BOTH (REV as well on
    the CG text, which is its own reverse complement)."""
    K, w = world
    x = w[text]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")
        for m in aw.LENGTHS:
            check_direct(K, x, 2, m, aw.BANDS, text)
            check_real(K, x, 2, m, aw.BANDS, (sr.FWD, sr.BOTH) + ((sr.REV,) if text == "cg" else ()), text)
    finally:
        defaults(K)


@pytest.mark.parametrize("text", aw.K1_TEXTS)
def test_k1_bands_4_to_14(world, text):
    """K = 1: the bands that no other device test runs."""
    K, w = world
    x = w[text]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][1], "task-mid")
        for m in aw.LENGTHS:
            check_direct(K, x, 1, m, range(4, 15), (text, "K = 1"))
            check_real(K, x, 1, m, range(4, 15), (sr.BOTH,), (text, "K = 1"))
    finally:
        defaults(K)


def test_split_classes(world):
    """The loads under the 16-lane group mask (class 4), then the plain form
    (class 1) on the same upload: two texts, lengths 100 and 256, bands 2, 7, 14."""
    K, w = world
    for text in ("runs", "tandem"):
        x = w[text]
        try:
            defaults(K)
            fresh_upload(K, x["idx"][2], "task-mid")
            for cls in (4, 1):
                K.set_split_class(cls)
                for m in (100, 256):
                    check_direct(K, x, 2, m, (2, 7, 14), (text, "class", cls))
                    check_real(K, x, 2, m, (2, 7, 14), (sr.BOTH,), (text, "class", cls), occs=(8, 256))
        finally:
            defaults(K)
            fresh_upload(K, x["idx"][2], "task-mid")


@pytest.mark.parametrize("text", list(aw.texts()))
def test_band_zero_is_the_verify(world, text):
    """Band 0 on the device equals kfmi_verify_seeds on the same device handles."""
    K, w = world
    x = w[text]
    K.set_backend("task-mid")
    for m in aw.LENGTHS:
        q, iv, sp, _ = x["cases"][m]["direct"]
        rq, _, per_k = x["cases"][m]["real"]
        ds = [direct_device(K, x["idx"][2], q, iv, sp)]
        try:
            ds.append(seeded_device(K, x["idx"][2], rq, per_k[2][0], per_k[2][1], sr.BOTH, (text, m)))
            for d in ds:
                for occ in aw.OCCS:
                    for mm in (0, 3, m):
                        want = d.verify(occ, mm)
                        same(d.align(occ, 0, mm), want, (text, m, occ, mm))
        finally:
            for d in ds:
                d.close()


def test_every_text_end_origin(world):
    """The 16 first and 16 last origins x every pinned read position x {one
    base deleted, one inserted} at m = 100, every band: 512 tasks, two blocks."""
    K, w = world
    x = w["two"]
    q, iv, sp, a = aw.ends_world(x["world"])
    K.set_backend("task-mid")
    d = direct_device(K, x["idx"][2], q, iv, sp)
    try:
        for band in aw.BANDS:
            for me in (1, 100):
                same(d.align(8, band, me), ar.records(a, 8, 8, band, me), ("ends", band, me))
    finally:
        d.close()


@pytest.mark.parametrize("num", [257, 513])
def test_batch_ends_inside_a_block(world, num):
    """257 and 513 tasks of one text: the last block holds one task, and lanes
    with 256 candidates stand next to lanes with none."""
    K, w = world
    x = w["cg"]
    q, iv, sp, a = aw.batch_world(x["world"], x["cases"][100]["direct"][0])
    K.set_backend("task-mid")
    d = direct_device(K, x["idx"][2], np.ascontiguousarray(q[:num]), iv[:num], sp[:num])
    try:
        for me in (0, 100):
            same(d.align(256, aw.BATCH_BAND, me), ar.records(a, 8, 256, aw.BATCH_BAND, me)[:num], ("batch", num, me))
    finally:
        d.close()
