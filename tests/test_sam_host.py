"""SAM lines on the host (kstep_fmi.h, "SAM lines"), no GPU needed:

* kfmi_sam_lines_cpu equals the model of sam_ref.py byte for byte, offsets
  included, behind kfmi_align_paths_cpu at m in {1, 20, 100, 256}, every strand
  mode, both option values, bands 0, 3 and 15, C = 8 and 1, quals given and
  absent, name_base 0 and 10**19;
* the conditions of sam_ref.REQUIRED hold on the model alone (sam_ref.world
  asserts them before any SAM call);
* sam_ref.replay passes on every mapped line;
* the header text; every refusal creates nothing; fasta_contigs;
* tests/asan/sam_asan.c runs clean under AddressSanitizer + UBSan over the
  same world's records, written to a file here, and finds the expected bytes."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sam_ref as sm
import util


@pytest.fixture(scope="module")
def world(kfmi_mod):
    return kfmi_mod, sm.world(kfmi_mod)


def contigs_of(K, tab):
    return K.Contigs.create(tab.names, tab.begins, tab.lengths)


def replay_all(lines, tab, text) -> int:
    done = 0
    for ln in lines:
        if ln.split(b"\t")[1] != b"4":
            sm.replay(ln, tab, text)
            done += 1
    return done


@pytest.mark.parametrize("m", sm.LENGTHS)
def test_host_form_equals_the_model(world, m):
    K, ws = world
    w = ws[m]
    ct = contigs_of(K, w.table)
    mapped = 0
    try:
        for mm, strands, band, C, with_quals, options in sm.configs():
            if mm != m:
                continue
            h = sm.HostChain(K, w, w.reads.shape[0], strands, band, C, with_quals)
            try:
                for base in (0, 10**19):
                    want = h.model(options, base)
                    s = K.sam_lines_cpu(w.text, h.Q, ct, h.H, h.P, h.G, h.U, strands, C, band, options, base)
                    what = (m, strands, band, C, with_quals, options, base)
                    assert s.num == len(want), what
                    assert np.array_equal(s.offsets(), sm.offsets_of(want)), what
                    assert s.text() == b"".join(want), what
                    assert s.lines() == [x[:-1] for x in want], what
                    s.close()
                mapped += replay_all(want, w.table, w.text)
            finally:
                h.close()
    finally:
        ct.close()
    assert mapped > 100


def test_header_and_table_refusals(world):
    K, ws = world
    tab = ws[100].table
    ct = contigs_of(K, tab)
    want = tab.header()
    assert ct.header() == want
    assert want.startswith(b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:a\tLN:700\n@SQ\tSN:" + b"L" * 254 + b"\tLN:100\n")
    L = K.load()
    assert L.kfmi_sam_header(ct.ptr, None, 0) == len(want)
    small = ctypes.create_string_buffer(b"\x55" * len(want), len(want))
    assert L.kfmi_sam_header(ct.ptr, small, len(want) - 1) == len(want) and small.raw == b"\x55" * len(want)
    ct.close()
    bad = [
        ([], [], []),
        ([""], [0], [5]),
        (["x" * 255], [0], [5]),
        (["a b"], [0], [5]),
        (["a\x7f"], [0], [5]),
        (["ok"], [0], [0]),
        (["a", "b"], [0, 9], [10, 5]),        # overlap
        (["a", "b"], [20, 0], [5, 5]),        # descending
        (["a"], [0xFFFFFFF0], [0x20]),        # past 2^32 - 1
    ]
    for names, begins, lengths in bad:
        with pytest.raises(K.KfmiError) as e:
            K.Contigs.create(names, begins, lengths)
        assert e.value.args[0].endswith("(code 33)"), (names, e.value)
    ok = K.Contigs.create(["a", "b"], [0, 10], [10, 5])   # adjacent contigs are allowed
    ok.close()


def test_line_refusals_create_nothing(world):
    K, ws = world
    w = ws[20]
    ct = contigs_of(K, w.table)
    past = K.Contigs.create(["z"], [0], [sm.N_TEXT + 1])
    h = sm.HostChain(K, w, 5, sm.BOTH, 3, 4, True)
    odd = K.Results.alloc(h.T + 1)
    L = K.load()
    t = np.frombuffer(w.text, dtype=np.uint8)
    tp = t.ctypes.data_as(ctypes.c_void_p)

    def call(text=tp, n=t.size, q=h.Q, c=ct, hits=h.H, paths=h.P, cig=h.G, quals=h.U, strands=sm.BOTH, C=4, band=3,
             options=0, base=0):
        out = ctypes.c_void_p(0x1234)
        code = L.kfmi_sam_lines_cpu(text, n, q.ptr, c.ptr, hits.ptr, paths.ptr, cig.ptr, quals.ptr if quals else None,
                                    strands, C, band, options, base, 1, ctypes.byref(out))
        if code == 0:
            assert out.value not in (None, 0x1234)
            L.kfmi_sam_free(ctypes.byref(out))
        return code, out.value

    try:
        assert call()[0] == 0
        for kw in (dict(options=2), dict(options=0x80000001), dict(base=2**64 - 4), dict(base=2**64 - 5), dict(c=past), dict(strands=0),
                   dict(strands=4), dict(band=16), dict(C=0), dict(C=33), dict(C=5), dict(hits=odd), dict(paths=odd),
                   dict(quals=odd), dict(paths=h.H), dict(cig=h.P), dict(quals=h.G), dict(strands=sm.FWD), dict(n=2**32),
                   dict(text=None)):
            assert call(**kw) == (33, 0x1234), kw
        assert call(base=2**64 - 6)[0] == 0   # name_base + num = 2^64 - 1 still fits
    finally:
        for x in (odd, past, ct):
            x.close()
        h.close()


def test_fasta_contigs(kfmi_mod):
    K = kfmi_mod
    data = b">one first record\nACGTacgt\nNNnn\n>two\tx\nTTTT\n\n>three\nGATTACA\nga\n\n"
    text, ct = K.fasta_contigs(data)
    assert text == b"ACGTACGTGGGG" + b"TTTT" + b"GATTACAGA"
    assert ct.header() == b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:one\tLN:12\n@SQ\tSN:two\tLN:4\n@SQ\tSN:three\tLN:9\n"
    ct.close()
    with pytest.raises(K.KfmiError):
        K.fasta_contigs(b">empty\n>next\nACGT\n")


def test_map_sam_array_on_the_host(world):
    """The binding's chain with cpu=True: header plus lines, every mapped line replayed."""
    K, ws = world
    w = ws[100]
    ct = contigs_of(K, w.table)
    idx = K.Index.build(w.text, k=2, d=64, sa_rate=1)
    try:
        out = K.map_sam_array(idx, w.reads, ct, strands=sm.BOTH, band=3, max_edits=6, cigar_entries=8, mapq=True,
                              cpu=True, text=w.text, name_base=7)
        head = w.table.header()
        assert out.startswith(head)
        lines = out[len(head):].splitlines(keepends=True)
        assert len(lines) == w.reads.shape[0] and lines[0].startswith(b"7\t")
        assert replay_all(lines, w.table, w.text) > 20
    finally:
        idx.close()
        ct.close()


def test_symbols(kfmi_mod):
    K = kfmi_mod
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name in ("kfmi_contigs_create", "kfmi_contigs_free", "kfmi_sam_header", "kfmi_sam_lines", "kfmi_sam_lines_cpu",
                 "kfmi_sam_num", "kfmi_sam_bytes", "kfmi_sam_offsets", "kfmi_sam_text", "kfmi_sam_free"):
        assert name + "(" in header and hasattr(K.load(), name), name
    assert "#define KFMI_SAM_CIGAR_M 1u" in header and K.SAM_CIGAR_M == 1


def write_case(path, w, h, options, base, want):
    """One case for sam_asan.c: little-endian u32 / u64 fields, then the arrays."""
    tab = w.table
    hits, paths, cig, quals = h.records()
    names = b"".join(n.encode() + b"\0" for n in tab.names)
    blob = b"".join(want)
    with open(path, "wb") as f:
        f.write(struct.pack("<9IQ3Q", len(w.text), w.m, h.reads.shape[0], h.strands, h.band, h.C, options,
                            0 if quals is None else 1, len(tab.names), base, len(names), len(blob), h.T))
        f.write(w.text + h.reads.tobytes() + names)
        f.write(np.asarray(tab.begins, dtype="<u4").tobytes() + np.asarray(tab.lengths, dtype="<u4").tobytes())
        f.write(hits.astype("<u4").tobytes() + paths.astype("<u4").tobytes() + cig.astype("<u4").tobytes())
        if quals is not None:
            f.write(quals.astype("<u4").tobytes())
        f.write(sm.offsets_of(want).astype("<u8").tobytes() + blob)


def test_sam_clean_under_asan(world, tmp_path):
    """tests/asan/sam_asan.c with csrc/host/*.c under -fsanitize=address,undefined: a stand-alone program, the HIP
    layer stubbed, over records written here."""
    K, ws = world
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    files = []
    for m, strands, band, C, with_quals, options, base in ((100, sm.BOTH, 3, 8, True, 0, 0), (256, sm.REV, 15, 8, False, 1, 10**19),
                                                          (1, sm.FWD, 3, 1, True, 0, 5), (20, sm.BOTH, 0, 8, True, 1, 99)):
        h = sm.HostChain(K, ws[m], ws[m].reads.shape[0], strands, band, C, with_quals)
        try:
            fn = tmp_path / ("case_%d_%d.bin" % (m, strands))
            write_case(fn, ws[m], h, options, base, h.model(options, base))
            files.append(str(fn))
        finally:
            h.close()
    srcs = sorted(str(p) for p in (util.PKG / "csrc" / "host").glob("*.c"))
    exe = tmp_path / "sam_asan"
    cmd = ["gcc", "-g", "-O1", "-std=gnu11", "-fopenmp", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(exe), str(util.REPO / "tests" / "asan" / "sam_asan.c")] + srcs
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    p = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK"), p.stdout[-2000:] + p.stderr[-4000:]
    assert int(p.stdout.split()[1]) > 40
