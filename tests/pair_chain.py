"""The paired-end chain as models and host forms, shared by test_pairs_host.py
and test_pairs_gpu.py: seeds and the align step from the library's host forms
(test_seeds_host.py and test_align_host.py hold those to their own models), the
mate windows, the placements in them and the pair choice from window_ref.py,
the CIGARs from kfmi_align_paths_cpu (held to path_ref.py by test_path_host.py).

chain() asserts on its results on the text without repeats, before any device is asked:
  * every mate with a 10-base indel has no own hit on its strand -- the band of
    3 cannot place it -- and is brought back by the rescue: RESCUED, PROPER, at
    most 10 edits, at its true place;
  * every clean pair and every pair with a one-base indel is PROPER at its
    true places, in the orientation it was simulated in (a mate inside the
    text's 300-base copy has its own hit at the other copy and is rescued);
  * no discordant pair is PROPER;
  * modes 0 and 1 give the same paired records for the pairs whose own hits are
    concordant."""
import numpy as np

import seed_ref as sr
import verify_ref as vr
import window_ref as wr

S, OCC, C = 4, 8, 16


def own_hits(K, idx, text, q):
    """The align step's records of both strands on the host: uint32 [2N, 2]."""
    T = 2 * q.shape[0]
    Q = K.Queries.from_array(q)
    iv, sp, hits = K.Results.alloc(S * T), K.Results.alloc(S * T), K.Results.alloc(T)
    tmp = None
    try:
        rate, sa = idx.sa()
        if rate != 1:
            tmp = K.Index.build(bytes(text), k=1, d=64, sa_rate=1)
            rate, sa = tmp.sa()
        K.search_seeds_cpu(idx, Q, iv, sp, S, sr.BOTH)
        K.align_seeds_cpu(text, sa, Q, iv, sp, hits, S, sr.BOTH, OCC, wr.PAIR_BAND, wr.PAIR_EDITS)
        return hits.array().copy().reshape(T, 2)
    finally:
        if tmp is not None:
            tmp.close()
        for h in (Q, iv, sp, hits):
            h.close()


def host_paths(K, text, q, paired):
    T = 2 * q.shape[0]
    Q, H, P, G = K.Queries.from_array(q), K.Results.alloc(T), K.Results.alloc(T), K.Results.alloc(T * C)
    try:
        H.array()[:] = paired.reshape(-1)
        K.align_paths_cpu(text, Q, H, P, G, sr.BOTH, wr.PAIR_BAND, wr.PAIR_EDITS, C)
        return P.array().copy().reshape(T, 2), G.array().copy().reshape(T, 2 * C)
    finally:
        for h in (Q, H, P, G):
            h.close()


_cache = {}


def texts() -> dict:
    """r1003: random, no repeat -- the conditions are asserted on it.  n1009: one 300-base copy, so mates inside it
    have their own hit at the other copy; the records are compared all the same, the conditions are not asked."""
    return {"r1003": np.ascontiguousarray(wr.ACGT[np.random.default_rng(83_000).integers(0, 4, size=1_003)]),
            "n1009": vr.small_text(1_009)}


def chain(K, name: str, text: np.ndarray, k: int = 2) -> dict:
    if (name, k) in _cache:
        return _cache[name, k]
    w = vr.World(text)
    q, kinds, truth = wr.pair_reads(text, 81_000 + len(name))
    tasks = sr.tasks_of(q, sr.BOTH)
    idx = K.Index.build(text.tobytes(), k=k, d=64)
    hits = own_hits(K, idx, text, q)
    b = wr.Begins(w, tasks)
    m, lo, hi = wr.PAIR_M, wr.PAIR_MIN, wr.PAIR_MAX
    out = dict(world=w, text=text, idx=idx, q=q, tasks=tasks, kinds=kinds, truth=truth, hits=hits, begins=b, modes={})
    for mode in (0, 1):
        win = wr.mate_windows(hits, w.n, m, lo, hi, mode)
        resc = wr.place(b, win, wr.PAIR_EDITS)
        paired = wr.pair_hits(hits, resc, m, lo, hi)
        out["modes"][mode] = dict(win=win, resc=resc, paired=paired)
    out["paths"], out["cigars"] = host_paths(K, text, q, out["modes"][0]["paired"])
    if name == "r1003":
        check(out)
    _cache[name, k] = out
    return out


def check(c: dict) -> None:
    m, lo, hi = wr.PAIR_M, wr.PAIR_MIN, wr.PAIR_MAX
    hits = c["hits"].reshape(-1, 4, 2)
    p0, p1 = (c["modes"][mode]["paired"].reshape(-1, 4, 2) for mode in (0, 1))
    seen = dict.fromkeys(("rescued", "proper 0", "proper 1", "alone", "modes"), 0)
    for p, kind in enumerate(c["kinds"]):
        rec = p0[p]
        proper = (rec[:, 1] & wr.PROPER) != 0
        name = kind.split("/")[0]
        if name in ("far", "order", "same"):
            assert not proper.any(), (kind, rec)
            seen["alone"] += 1
            continue
        orient = int(kind.split("/")[2])
        f, r = (2, 1) if orient else (0, 3)
        ta, tb = (int(x) for x in c["truth"][p])                        # reads a and b
        bf, br = (tb, ta) if orient else (ta, tb)
        assert proper[f] and proper[r] and proper.sum() == 2, (kind, rec)
        if name in ("del10", "ins10", "del10-first"):
            side = f if name == "del10-first" else r
            want = bf if side == f else br
            assert hits[p, side, 0] == wr.NONE, (kind, "the band of 3 placed a 10-base indel", hits[p])
            assert rec[side, 1] & wr.RESCUED and (rec[side, 1] & wr.EDITS) <= 10 and rec[side, 0] == want, (kind, rec)
            seen["rescued"] += 1
        else:
            for side, want in ((f, bf), (r, br)):            # rescued only where the own hit lies elsewhere (the text's copy)
                assert rec[side, 0] == want and (not rec[side, 1] & wr.RESCUED or hits[p, side, 0] != want), (kind, rec, bf, br)
        seen["proper %d" % orient] += 1
        own_ok = any(int(hits[p, a, 0]) != wr.NONE and int(hits[p, b, 0]) != wr.NONE and
                     wr.concordant(int(hits[p, a, 0]), int(hits[p, b, 0]), m, lo, hi) for a, b in ((0, 3), (2, 1)))
        if own_ok:
            assert np.array_equal(p0[p], p1[p]), (kind, "modes 0 and 1 differ", p0[p], p1[p])
            seen["modes"] += 1
    assert all(v >= 6 for v in seen.values()), seen
    # mode 0 rescues only where it is needed, mode 1 everywhere a mate has a hit
    n0, n1 = ((c["modes"][mode]["win"][:, 1] > 0).sum() for mode in (0, 1))
    assert 0 < n0 < n1


def per_read(c: dict) -> tuple:
    """What map_pairs_array returns, from the chain's records of mode 0."""
    paired, paths, cig = c["modes"][0]["paired"], c["paths"], c["cigars"]
    n = c["q"].shape[0]
    x = paired[:, 0].astype(np.int64).reshape(n, 2)
    placed = x != wr.NONE
    strand = np.where(placed[:, 0], 0, np.where(placed[:, 1], 1, -1))
    k = np.maximum(strand, 0)
    r = np.arange(n)
    t = 2 * r + k
    ok = strand >= 0
    begin = np.where(ok, paired[t, 0].astype(np.int64), -1)
    has_path = ok & (paths[t, 0] != wr.NONE)
    end = np.where(has_path, paths[t, 0].astype(np.int64), -1)
    edits = np.where(ok, paired[t, 1] & wr.EDITS, 0).astype(np.int64)
    flags = np.where(ok, paired[t, 1] & (wr.PROPER | wr.RESCUED | wr.MULTI), 0).astype(np.int64)
    return begin, end, strand, edits, flags, t, has_path
