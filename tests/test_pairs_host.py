"""The paired-end chain on the host (kstep_fmi.h, "place windows / pairs"), no
GPU needed: on simulated pairs -- clean mates, one-base and 10-base indels, both
orientations, fragments at min_frag, inside and at max_frag, discordant pairs --
kfmi_mate_windows_cpu, kfmi_place_windows_cpu and kfmi_pair_hits_cpu equal the
models of window_ref.py bit for bit, modes 0 and 1.  pair_chain.chain asserts
what the inputs must show (the rescue brings back every mate the band cannot
place) on the models alone."""
import pytest

import pair_chain as pc
import seed_ref as sr
import window_ref as wr
from test_window_host import host_mate, host_pair, host_place, same

@pytest.mark.parametrize("text", ["r1003", "n1009"])
def test_host_forms_equal_the_models(kfmi_mod, text):
    K = kfmi_mod
    c = pc.chain(K, text, pc.texts()[text])
    m, lo, hi = wr.PAIR_M, wr.PAIR_MIN, wr.PAIR_MAX
    for mode in (0, 1):
        x = c["modes"][mode]
        win = host_mate(K, c["world"].n, c["hits"], m, lo, hi, mode)
        same(win, x["win"], (text, mode, "windows"))
        resc = host_place(K, c["text"], c["q"], sr.BOTH, win, wr.PAIR_EDITS)
        same(resc, x["resc"], (text, mode, "rescued"))
        same(host_pair(K, c["hits"], resc, m, lo, hi), x["paired"], (text, mode, "paired"))
