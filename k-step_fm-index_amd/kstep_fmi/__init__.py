"""kstep_fmi -- Python host binding of libkstepfmi.so (include/kstep_fmi.h).

This is the ctypes form of the reference's link-time plugin interface
(/root/reference/common/interface.h:27-41): the same entry points, argument
meaning and error codes, over opaque handles.  It is plumbing for the test
suite, bench.py and multi-GPU runs; the engine itself is the C ABI library
(HIP kernels for gfx950 + C host code) and there is no Python or CPU fallback
for the search: if the library or a GPU is missing, calls fail loudly.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent          # k-step_fm-index_amd/
LIB_PATH = PKG_DIR / "lib" / "libkstepfmi.so"
BIN_DIR = PKG_DIR / "bin"

# (the packed and ac128 layouts were retired in round 6)
BACKENDS = ("task", "coop", "task-ac", "coop-ac", "task-mid", "coop-mid", "task-ac-mid", "coop-ac-mid",
            "task-grp", "coop-grp")
BACKEND_TAG = {"task": 101, "coop": 101, "task-ac": 201, "coop-ac": 201, "task-mid": 101, "coop-mid": 101,
               "task-ac-mid": 201, "coop-ac-mid": 201, "task-grp": 101, "coop-grp": 101}

_lib = None


class KfmiError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _lib.errorCommon(code).decode() if _lib is not None else f"error {code}"
        super().__init__(f"{what}: {msg} (code {code})" if what else f"{msg} (code {code})")


def build(jobs: int = 8) -> None:
    """Compile the HIP + C library and tools in-tree (hipcc --offload-arch=gfx950)."""
    subprocess.run(["make", "-C", str(PKG_DIR), f"-j{jobs}"], check=True)


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(f"{LIB_PATH} not built -- run kstep_fmi.build() / make -C {PKG_DIR}")
    L = ctypes.CDLL(str(LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    pvp = ctypes.POINTER(ctypes.c_void_p)
    sig = {
        "loadIndex": (i32, [ctypes.c_char_p, pvp]),
        "saveIndex": (i32, [ctypes.c_char_p, vp]),
        "initResults": (i32, [u32, pvp]),
        "searchIndexGPU": (None, [vp, vp, vp]),
        "freeIndex": (i32, [pvp]),
        "freeReference": (i32, [pvp, pvp]),
        "buildIndex": (i32, [vp, pvp]),
        "freeQueriesGPU": (i32, [pvp]),
        "freeResultsGPU": (i32, [pvp]),
        "freeIndexGPU": (i32, [pvp]),
        "transferGPUtoCPU": (i32, [vp]),
        "transferCPUtoGPU": (i32, [vp, vp, vp]),
        "sampleTime": (ctypes.c_double, []),
        "base2index": (u32, [u32]),
        "loadRef": (i32, [ctypes.c_char_p, u32, pvp]),
        "saveRef": (i32, [ctypes.c_char_p, vp]),
        "loadQueries": (i32, [ctypes.c_char_p, u32, u32, pvp]),
        "writeResults": (i32, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), u32]),
        "loadResults": (i32, [ctypes.c_char_p, pvp]),
        "freeQueries": (i32, [pvp]),
        "freeResults": (i32, [pvp]),
        "saveResults": (i32, [ctypes.c_char_p, vp, vp]),
        "errorCommon": (ctypes.c_char_p, [i32]),
        "kfmi_set_backend": (i32, [ctypes.c_char_p]),
        "kfmi_get_backend": (ctypes.c_char_p, []),
        "kfmi_set_device": (i32, [i32]),
        "kfmi_device_count": (i32, []),
        "kfmi_device_pci_bus_id": (i32, [i32, ctypes.c_char_p, i32]),
        "kfmi_last_error": (i32, []),
        "kfmi_search": (i32, [vp, vp, vp]),
        "searchIndexCPU": (None, [vp, vp, vp]),
        "kfmi_search_cpu": (i32, [vp, vp, vp, i32]),
        "kfmi_last_timing": (i32, [ctypes.POINTER(ctypes.c_double)] * 3),
        "kfmi_load_index_tag": (i32, [ctypes.c_char_p, u32, pvp]),
        "kfmi_index_from_image": (i32, [vp, u64, pvp]),
        "kfmi_index_image": (i32, [vp, pvp, ctypes.POINTER(ctypes.c_uint64)]),
        "kfmi_index_header": (i32, [vp, vp]),
        "kfmi_transform_interleave": (i32, [vp, pvp]),
        "kfmi_transform_ac": (i32, [vp, pvp, pvp]),
        "kfmi_transform_plain": (i32, [vp, pvp]),
        "kfmi_queries_from_buffer": (i32, [vp, u64, u32, pvp]),
        "kfmi_load_queries_gpu": (i32, [ctypes.c_char_p, u32, u64, pvp]),
        "kfmi_results_alloc": (i32, [u64, pvp]),
        "kfmi_results_host": (ctypes.POINTER(ctypes.c_uint32), [vp]),
        "kfmi_results_num": (u64, [vp]),
        "kfmi_build_index_cpu": (i32, [vp, u64, u32, u32, pvp]),
        "kfmi_build_index_gpu": (i32, [vp, u64, u32, u32, i32, pvp]),
        "kfmi_derive_index_gpu": (i32, [vp, u32, i32, pvp]),
        "kfmi_build_stats": (i32, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
        "kfmi_count_blocks": (i32, [vp, vp, ctypes.POINTER(ctypes.c_uint64)]),
        "kfmi_count_lines": (i32, [vp, vp, ctypes.POINTER(ctypes.c_uint64)]),
        "kfmi_probe_replay": (i32, [vp, vp, i32, i32, i32, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "kfmi_device_index_bytes": (u64, [vp]),
        "kfmi_search_stream": (i32, [vp, vp, u64, u32, vp, u64]),
        "kfmi_host_alloc": (i32, [u64, pvp]),
        "kfmi_host_threads": (i32, []),
        "kfmi_host_free": (i32, [vp]),
        "kfmi_stream_release": (i32, []),
        "kfmi_stream_hostpacked_fraction": (ctypes.c_double, []),
        "kfmi_pack_queries": (i32, [vp, u64, u32, vp]),
        "kfmi_pack_queries_k": (i32, [vp, u64, u32, u32, vp]),
        "kfmi_queries_upload_form": (i32, [vp]),
        "kfmi_set_devices": (i32, [ctypes.POINTER(ctypes.c_int32), i32]),
        "kfmi_get_devices": (i32, [ctypes.POINTER(ctypes.c_int32), i32]),
        "kfmi_build_index_ex": (i32, [vp, u64, u32, u32, u32, i32, pvp]),
        "kfmi_set_ftab": (i32, [u32]),
        "kfmi_ftab_auto_bases": (u32, [u64, u32, u64]),
        "kfmi_set_ftab_budget": (i32, [u64]),
        "kfmi_device_ftab_bytes": (u64, [vp]),        "kfmi_set_split_class": (i32, [u32]),
        "kfmi_set_skip": (i32, [u32]),
        "kfmi_skip_in_effect": (u32, []),
        "kfmi_skip_auto": (u32, [u64, u32, u64]),
        "kfmi_device_skip_bytes": (u64, [vp]),
        "kfmi_device_skip_table": (i32, [vp, vp, u64, ctypes.POINTER(u32)]),
        "kfmi_set_jump": (i32, [u32]),
        "kfmi_jump_in_effect": (u32, []),
        "kfmi_set_jump_min": (i32, [u32]),
        "kfmi_jump_min": (u32, []),
        "kfmi_jump_auto": (u32, [u64, u32, u64]),
        "kfmi_device_jump_bytes": (u64, [vp]),
        "kfmi_device_jump_tables": (i32, [vp, u32, vp, vp, u64, vp, u64]),
        "kfmi_set_jump_lines": (i32, [u32]),
        "kfmi_jump_lines": (u32, []),
        "kfmi_device_jump_line_bytes": (u64, [vp]),
        "kfmi_device_jump_lines": (i32, [vp, u32, vp, u64]),
        "kfmi_jump_line_geometry": (i32, [u64, u64, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "kfmi_set_ftab_fold": (i32, [u32]),
        "kfmi_ftab_fold": (u32, []),
        "kfmi_set_ftab_fold_bound": (i32, [u32]),
        "kfmi_ftab_fold_bound": (u32, [u64]),
        "kfmi_ftab_fold_fits": (u32, [u64, u64]),
        "kfmi_ftab_fold_encode": (i32, [u64, u32, u32, u32, ctypes.POINTER(u32)]),
        "kfmi_ftab_fold_decode": (i32, [u64, u32, u32, u32, ctypes.POINTER(u32)]),
        "kfmi_device_ftab_entries": (i32, [vp, u32, vp, u64, u64, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "kfmi_set_fused": (i32, [i32]),
        "kfmi_set_walk_check": (i32, [u32]),
        "kfmi_fail_index_uploads": (i32, [u32]),
        "kfmi_walk_check_last": (i32, []),
        "kfmi_set_alphabet": (i32, [ctypes.c_char_p]),
        "kfmi_index_sa": (i32, [vp, pvp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
        "kfmi_save_sa": (i32, [ctypes.c_char_p, vp]),
        "kfmi_load_sa": (i32, [ctypes.c_char_p, vp]),
        "kfmi_locate": (i32, [vp, vp, u32, pvp]),
        "kfmi_locations_total": (u64, [vp]),
        "kfmi_locations_offsets": (vp, [vp]),
        "kfmi_locations_positions": (vp, [vp]),
        "kfmi_locations_free": (i32, [pvp]),
        "kfmi_search_strands": (i32, [vp, vp, vp, u32]),
        "kfmi_search_stream_strands": (i32, [vp, vp, u64, u32, vp, u64, u32]),
        "kfmi_search_cpu_strands": (i32, [vp, vp, vp, u32, i32]),
        "kfmi_revcomp_queries": (i32, [vp, u64, u32, vp]),
        "kfmi_strand_words_host": (i32, [vp, u64, u32, u32, u32, vp]),
        "kfmi_reverse_stream_host": (i32, [vp, u64, u32, u32, vp]),
        "kfmi_search_seeds": (i32, [vp, vp, vp, vp, u32, u32]),
        "kfmi_search_seeds_cpu": (i32, [vp, vp, vp, vp, u32, u32, i32]),
        "kfmi_search_trace": (i32, [vp, vp, vp, vp]),
        "kfmi_search_strands_trace": (i32, [vp, vp, vp, u32, vp]),
        "kfmi_search_seeds_trace": (i32, [vp, vp, vp, vp, u32, u32, vp]),
        "kfmi_launch_plan": (i32, [ctypes.c_char_p] + [u32] * 11 + [vp]),
        "kfmi_results_to_device": (i32, [vp]),
        "kfmi_verify_seeds": (i32, [vp, vp, vp, vp, vp, u32, u32, u32, u32]),
        "kfmi_verify_seeds_cpu": (i32, [vp, u64, vp, u64, vp, vp, vp, vp, u32, u32, u32, u32, i32]),
        "kfmi_align_seeds": (i32, [vp, vp, vp, vp, vp, u32, u32, u32, u32, u32]),
        "kfmi_align_seeds_cpu": (i32, [vp, u64, vp, u64, vp, vp, vp, vp, u32, u32, u32, u32, u32, i32]),
        "kfmi_align_paths": (i32, [vp, vp, vp, vp, vp, u32, u32, u32, u32]),
        "kfmi_align_paths_cpu": (i32, [vp, u64, vp, vp, vp, vp, u32, u32, u32, u32, i32]),
        "kfmi_set_path_chunk": (i32, [u64]),
        "kfmi_place_windows": (i32, [vp, vp, vp, vp, u32, u32]),
        "kfmi_place_windows_cpu": (i32, [vp, u64, vp, vp, vp, u32, u32, i32]),
        "kfmi_mate_windows": (i32, [vp, vp, vp, u32, u32, u32, u32]),
        "kfmi_mate_windows_cpu": (i32, [u64, vp, vp, u32, u32, u32, u32]),
        "kfmi_pair_hits": (i32, [vp, vp, vp, vp, u32, u32, u32]),
        "kfmi_pair_hits_cpu": (i32, [vp, vp, vp, u32, u32, u32]),
        "kfmi_align_second": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, u32]),
        "kfmi_align_second_cpu": (i32, [vp, u64, vp, u64, vp, vp, vp, vp, vp, u32, u32, u32, u32, u32, i32]),
        "kfmi_map_quality": (i32, [vp, vp, vp, vp, u32, u32]),
        "kfmi_map_quality_cpu": (i32, [vp, vp, vp, u32, u32]),
        "kfmi_contigs_create": (i32, [vp, vp, vp, u32, pvp]),
        "kfmi_contigs_free": (i32, [pvp]),
        "kfmi_sam_header": (ctypes.c_int64, [vp, vp, u64]),
        "kfmi_sam_lines": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, u64, pvp]),
        "kfmi_sam_lines_cpu": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, u64, i32, pvp]),
        "kfmi_sam_num": (u64, [vp]),
        "kfmi_sam_bytes": (u64, [vp]),
        "kfmi_sam_offsets": (vp, [vp]),
        "kfmi_sam_text": (vp, [vp]),
        "kfmi_sam_free": (i32, [pvp]),
        "kfmi_set_sam_form": (i32, [u32]),
        "kfmi_sam_last_passes": (i32, [ctypes.POINTER(ctypes.c_double)] * 3),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def exported_symbols():
    """Names every C-ABI entry point the header declares (for the load test)."""
    load()
    return [n for n in _lib.__dict__ if not n.startswith("_")]


def _check(code: int, what: str) -> None:
    if code:
        raise KfmiError(code, what)


def set_backend(name: str) -> None:
    _check(load().kfmi_set_backend(name.encode()), f"set_backend({name})")


def get_backend() -> str:
    return load().kfmi_get_backend().decode()


FTAB_AUTO = 0xFFFFFFFF


def set_ftab(bases) -> None:
    """Jump-start table of `bases` bases (0 = off: the pure walk), or "auto"
    (the default): sized per index by ftab_auto_bases and built at upload."""
    n = FTAB_AUTO if bases == "auto" else int(bases)
    _check(load().kfmi_set_ftab(n), f"set_ftab({bases})")


def ftab_auto_bases(rows: int, k: int, budget_bytes: int) -> int:
    """The auto rule: table bases for an index of `rows` (n + 1) rows and K = k."""
    return int(load().kfmi_ftab_auto_bases(int(rows), int(k), int(budget_bytes)))


def set_ftab_budget(nbytes) -> None:
    """Byte budget of the auto rule (process-wide test knob); None = a quarter
    of the free device memory."""
    _check(load().kfmi_set_ftab_budget(0xFFFFFFFFFFFFFFFF if nbytes is None else int(nbytes)), "set_ftab_budget")


def set_ftab_fold(on) -> None:
    """Folded jump-start table (kstep_fmi.h): 1 (the default) = an upload that
    builds the auto table and the text jump's tables stores sa[L] in its
    one-row entries; 0 = every table stays {L, R}.  Process-wide
    (KFMI_FTAB_FOLD), read by an upload.  No setting changes a result."""
    _check(load().kfmi_set_ftab_fold(int(on)), f"set_ftab_fold({on})")


def ftab_fold() -> int:
    return int(load().kfmi_ftab_fold())


def set_ftab_fold_bound(bound) -> None:
    """Test knob: lowers the bound of the fold's fit rule (None or 0 = the
    rule's own, 0xFFFFFFFF - n), so a small index takes the "does not fit" branch."""
    _check(load().kfmi_set_ftab_fold_bound(0 if bound is None else int(bound)), f"set_ftab_fold_bound({bound})")


def ftab_fold_bound(n: int) -> int:
    """The fit rule: a table of an n-base text folds when every width other than 1 is below this."""
    return int(load().kfmi_ftab_fold_bound(int(n)))


def ftab_fold_fits(n: int, max_width: int) -> bool:
    return bool(load().kfmi_ftab_fold_fits(int(n), int(max_width)))


def ftab_fold_encode(n: int, L: int, R: int, p: int = 0):
    """The folded entry (x, y) of [L, R), p = sa[L] of a one-row entry; raises
    KfmiError when the width does not fit the rule or p > n."""
    out = (ctypes.c_uint32 * 2)()
    _check(load().kfmi_ftab_fold_encode(int(n), int(L), int(R), int(p), out), f"ftab_fold_encode({n}, {L}, {R}, {p})")
    return int(out[0]), int(out[1])


def ftab_fold_decode(n: int, x: int, y: int, folded: bool = True):
    """(L, R, p) of the entry (x, y) as every kernel decodes it; p = None when it carries no position."""
    out = (ctypes.c_uint32 * 3)()
    _check(load().kfmi_ftab_fold_decode(int(n), int(x), int(y), int(bool(folded)), out), "ftab_fold_decode")
    return int(out[0]), int(out[1]), (None if int(out[2]) == 0xFFFFFFFF else int(out[2]))


SKIP_AUTO = 0xFFFFFFFF


def set_skip(mode) -> None:
    """Skip table: 0 = off, 1 = on, "auto" (the default) = in effect exactly
    when the ftab setting is "auto" too; per calling thread."""
    n = SKIP_AUTO if mode == "auto" else int(mode)
    _check(load().kfmi_set_skip(n), f"set_skip({mode})")


def skip_in_effect() -> int:
    """The calling thread's skip setting resolved against its ftab setting:
    0 = off, 1 = on (explicit), 2 = auto and in effect."""
    return int(load().kfmi_skip_in_effect())


def skip_auto(rows: int, k: int, budget_bytes: int) -> bool:
    """The auto rule: whether an index of `rows` (n + 1) rows and K = k gets a
    skip table within `budget_bytes`."""
    return bool(load().kfmi_skip_auto(int(rows), int(k), int(budget_bytes)))


JUMP_AUTO = 0xFFFFFFFF
JUMP_MIN_DEFAULT = 8


def set_jump(mode) -> None:
    """Text jump: 0 = off, 1 = on, "auto" (the default) = in effect exactly
    when the skip setting is auto and in effect; per calling thread."""
    n = JUMP_AUTO if mode == "auto" else int(mode)
    _check(load().kfmi_set_jump(n), f"set_jump({mode})")


def jump_in_effect() -> int:
    """The calling thread's jump setting resolved against its skip setting:
    0 = off, 1 = on (explicit), 2 = auto and in effect."""
    return int(load().kfmi_jump_in_effect())


def set_jump_min(bases: int) -> None:
    """Fewest remaining bases a lane jumps with (process-wide; default 8)."""
    _check(load().kfmi_set_jump_min(int(bases)), f"set_jump_min({bases})")


def jump_min() -> int:
    return int(load().kfmi_jump_min())


def set_jump_lines(mode: int) -> None:
    """The text jump's line table: 0 = windows from the flat tables, 1 (the
    default) = from the lines, 2 = from the lines with the window's loads
    never split into 16-lane groups; process-wide (KFMI_JUMP_LINES).  Under
    1, on tables past the translation reach, reads longer than 192 bases take
    the flat tables' form (kstep_fmi.h).  No setting changes a result."""
    _check(load().kfmi_set_jump_lines(int(mode)), f"set_jump_lines({mode})")


def jump_lines() -> int:
    return int(load().kfmi_jump_lines())


def jump_line_geometry(n: int, p: int, nb: int):
    """(lines' first dword, line count, ISA dword, first window dword, bit
    shift, dwords read) of a jump with nb bases left at text position p."""
    out = (ctypes.c_uint64 * 6)()
    _check(load().kfmi_jump_line_geometry(int(n), int(p), int(nb), out), f"jump_line_geometry({n}, {p}, {nb})")
    return tuple(int(x) for x in out)


def jump_auto(rows: int, k: int, budget_bytes: int) -> bool:
    """The auto rule: whether an index of `rows` (n + 1) rows and K = k gets
    the text jump's tables within `budget_bytes`."""
    return bool(load().kfmi_jump_auto(int(rows), int(k), int(budget_bytes)))


def set_split_class(cls: int) -> None:
    """Fetch form of the task kernels by table-size class (0 = by the uploaded
    table's size, 1 / 2 / 4 = that class); process-wide test knob (KFMI_SPLIT)."""
    _check(load().kfmi_set_split_class(int(cls)), f"set_split_class({cls})")


def set_fused(on: bool) -> None:
    """In-kernel query packing where it fits (True, default) or always the
    separate pack launch (False); process-wide test knob (KFMI_FUSED)."""
    _check(load().kfmi_set_fused(1 if on else 0), f"set_fused({on})")


def fail_index_uploads(n: int) -> None:
    """Test knob: the next n index uploads fail for lack of device memory (0 = none)."""
    _check(load().kfmi_fail_index_uploads(int(n)), f"fail_index_uploads({n})")


def set_walk_check(mode: int) -> None:
    """Walk check of locate / derivation: 0 = by size (default), 1 = full
    pointer jumping, 2 = the sampled check; process-wide test knob."""
    _check(load().kfmi_set_walk_check(int(mode)), f"set_walk_check({mode})")


def walk_check_last() -> int:
    """How the last walk check decided: 0 none yet, 1 full, 2 sampled, 3 sampled then full."""
    return int(load().kfmi_walk_check_last())


def set_alphabet(mode: str | None) -> None:
    """Builders' alphabet: "acgt" (default), "map" (base2index every byte) or
    "ref" (byte-compatible with the reference builder); None = KFMI_ALPHABET."""
    _check(load().kfmi_set_alphabet(mode.encode() if mode else None), f"set_alphabet({mode})")


def set_device(dev: int) -> None:
    _check(load().kfmi_set_device(int(dev)), f"set_device({dev})")


def set_devices(devs) -> None:
    """Device group for the transfer/search/transfer trio (kfmi_set_devices):
    index replicated, queries sliced; [] returns to single-device mode."""
    devs = [int(d) for d in devs]
    arr = (ctypes.c_int32 * max(len(devs), 1))(*devs)
    _check(load().kfmi_set_devices(arr, len(devs)), f"set_devices({devs})")


def get_devices() -> list:
    arr = (ctypes.c_int32 * 16)()
    n = load().kfmi_get_devices(arr, 16)
    return [arr[i] for i in range(n)]


def build_stats() -> dict:
    """Tie diagnostics of the last GPU index build (kfmi_build_stats)."""
    t, r = ctypes.c_uint64(), ctypes.c_uint32()
    _check(load().kfmi_build_stats(ctypes.byref(t), ctypes.byref(r)), "build_stats")
    return {"ties": int(t.value), "rounds": int(r.value)}


def device_count() -> int:
    return int(load().kfmi_device_count())


def host_threads() -> int:
    """Threads of the library's parallel host paths (kfmi_host_threads)."""
    return int(load().kfmi_host_threads())


def device_pci_bus_id(dev: int) -> str:
    """PCI bus id of HIP device `dev` (the physical GPU, stable across processes)."""
    buf = ctypes.create_string_buffer(64)
    _check(load().kfmi_device_pci_bus_id(int(dev), buf, 64), f"device_pci_bus_id({dev})")
    return buf.value.decode()


def upload_form(queries) -> str:
    """How transfer_to_gpu left the reads (kfmi_queries_upload_form):
    "none", "ascii" or "packed" (packed to 2-bit words by the host)."""
    return ("none", "ascii", "packed")[load().kfmi_queries_upload_form(queries.ptr)]


def last_timing():
    t = [ctypes.c_double() for _ in range(3)]
    load().kfmi_last_timing(*[ctypes.byref(x) for x in t])
    return {"total_ms": t[0].value, "pack_ms": t[1].value, "lf_ms": t[2].value}


def _owned_view(addr: int, nbytes: int, dtype, owner) -> np.ndarray:
    """numpy view of library-owned memory that keeps `owner` (the handle) alive."""
    buf = (ctypes.c_uint8 * nbytes).from_address(addr)
    buf._kfmi_owner = owner
    return np.frombuffer(buf, dtype=dtype)


class _Handle:
    _free = ""

    def __init__(self, ptr):
        self._p = ctypes.c_void_p(ptr)

    @property
    def ptr(self):
        return self._p

    def close(self):
        if self._p and self._p.value:
            getattr(load(), self._free)(ctypes.byref(self._p))
            self._p = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index(_Handle):
    """An FM-index (any tag) -- the `fmi_t` handle of fmIndexCPUBaseline.c:54-69."""
    _free = "freeIndex"

    @classmethod
    def load(cls, path, required_tag: int = 0) -> "Index":
        L = load()
        p = ctypes.c_void_p()
        if required_tag:
            _check(L.kfmi_load_index_tag(str(path).encode(), required_tag, ctypes.byref(p)), f"load {path}")
        else:
            _check(L.loadIndex(str(path).encode(), ctypes.byref(p)), f"load {path}")
        return cls(p.value)

    @classmethod
    def from_image(cls, image) -> "Index":
        buf = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                                   else image).view(np.uint8)
        p = ctypes.c_void_p()
        _check(load().kfmi_index_from_image(buf.ctypes.data, buf.nbytes, ctypes.byref(p)), "index_from_image")
        return cls(p.value)

    @classmethod
    def build(cls, text: bytes, k: int = 2, d: int = 64, gpu: bool = False, host_image: bool = True,
              sa_rate: int = 0) -> "Index":
        """Tag-100 index of `text`; sa_rate > 0 also keeps SA[r] for rows r % sa_rate == 0 (locate)."""
        L = load()
        buf = np.frombuffer(text, dtype=np.uint8)
        p = ctypes.c_void_p()
        if sa_rate:
            err = L.kfmi_build_index_ex(buf.ctypes.data, buf.size, k, d, int(sa_rate), int(bool(gpu)),
                                        ctypes.byref(p))
        elif gpu:
            err = L.kfmi_build_index_gpu(buf.ctypes.data, buf.size, k, d, int(host_image), ctypes.byref(p))
        else:
            err = L.kfmi_build_index_cpu(buf.ctypes.data, buf.size, k, d, ctypes.byref(p))
        _check(err, "build_index")
        return cls(p.value)

    def header(self) -> dict:
        out = np.zeros(14, dtype=np.uint32)
        _check(load().kfmi_index_header(self._p, out.ctypes.data), "header")
        k = int(out[1])
        return dict(tag=int(out[0]), steps=k, bwtsize=int(out[2]), ncounters=int(out[3]),
                    nentries=int(out[4]), chunk=int(out[5]),
                    dollar_pos=[int(x) for x in out[6:6 + k]],
                    dollar_base=[int(x) for x in out[10:10 + k]])

    def image(self) -> np.ndarray:
        """Zero-copy view of the serialised file image (header + entries)."""
        p = ctypes.c_void_p()
        n = ctypes.c_uint64()
        _check(load().kfmi_index_image(self._p, ctypes.byref(p), ctypes.byref(n)), "image")
        return _owned_view(p.value, n.value, np.uint8, self)

    def save(self, fn) -> None:
        _check(load().saveIndex(str(fn).encode(), self._p), f"saveIndex {fn}")

    def derive(self, k: int, host_image: bool = False) -> "Index":
        """kfmi_derive_index_gpu: the 2K-step index of the same text, derived on
        the current device from this K-step one (K = 1 or 2, k = 2K)."""
        p = ctypes.c_void_p()
        _check(load().kfmi_derive_index_gpu(self._p, int(k), int(bool(host_image)), ctypes.byref(p)), "derive_index")
        return Index(p.value)

    def interleave(self) -> "Index":
        p = ctypes.c_void_p()
        _check(load().kfmi_transform_interleave(self._p, ctypes.byref(p)), "transform_interleave")
        return Index(p.value)

    def alt_counters(self):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(load().kfmi_transform_ac(self._p, ctypes.byref(a), ctypes.byref(b)), "transform_ac")
        return Index(a.value), Index(b.value)

    def plain(self) -> "Index":
        """The tag-100 index an AltCounters (tag 200/201) index was transformed from."""
        p = ctypes.c_void_p()
        _check(load().kfmi_transform_plain(self._p, ctypes.byref(p)), "transform_plain")
        return Index(p.value)

    def device_bytes(self) -> int:
        return int(load().kfmi_device_index_bytes(self._p))

    def ftab_bytes(self) -> int:
        """Bytes of the jump-start tables beside the device copies (not in device_bytes)."""
        return int(load().kfmi_device_ftab_bytes(self._p))

    def skip_bytes(self) -> int:
        """Bytes of the skip tables beside the device copies (not in device_bytes / ftab_bytes)."""
        return int(load().kfmi_device_skip_bytes(self._p))

    def jump_bytes(self) -> int:
        """Bytes of the text jump's tables beside the device copies (all members of a group)."""
        return int(load().kfmi_device_jump_bytes(self._p))

    def jump_tables(self, member: int = 0):
        """Test accessor: (sa, isa, text) of the single-device copy or of a
        group member: uint32 [rows], uint32 [rows], uint32 [n // 16 + 2] (base
        n - 1 - g of the text at bits 2g of the word stream)."""
        rows = int(self.header()["bwtsize"])
        words = (rows - 1) // 16 + 2
        sa = np.empty(rows, dtype=np.uint32)
        isa = np.empty(rows, dtype=np.uint32)
        text = np.empty(words, dtype=np.uint32)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _check(load().kfmi_device_jump_tables(self._p, int(member), as_p(sa), as_p(isa), rows, as_p(text), words),
               "jump_tables")
        return sa, isa, text

    def jump_line_bytes(self) -> int:
        """Bytes of the text jump's line tables (all members of a group; not in jump_bytes)."""
        return int(load().kfmi_device_jump_line_bytes(self._p))

    def jump_lines(self, member: int = 0):
        """Test accessor: the raw line table, uint32 [n // 16 + 2, 32]."""
        lines = (int(self.header()["bwtsize"]) - 1) // 16 + 2
        out = np.empty((lines, 32), dtype=np.uint32)
        _check(load().kfmi_device_jump_lines(self._p, int(member), out.ctypes.data_as(ctypes.c_void_p), lines),
               "jump_lines")
        return out

    def ftab_entries(self, first: int = 0, count=None, member: int = 0):
        """Test accessor: (bases, folded, uint32 [count, 2]) -- raw entries of the
        auto jump-start table of the single-device copy or of a group member,
        as stored: {L, R}, or the folded form when `folded`."""
        L = load()
        b, fo = ctypes.c_uint32(0), ctypes.c_uint32(0)
        if count is None:
            probe = np.empty((0, 2), dtype=np.uint32)
            _check(L.kfmi_device_ftab_entries(self._p, int(member), probe.ctypes.data_as(ctypes.c_void_p), 0, 0,
                                              ctypes.byref(b), ctypes.byref(fo)), "ftab_entries")
            count = (1 << (2 * int(b.value))) - int(first)
        out = np.empty((int(count), 2), dtype=np.uint32)
        _check(L.kfmi_device_ftab_entries(self._p, int(member), out.ctypes.data_as(ctypes.c_void_p), int(first),
                                          int(count), ctypes.byref(b), ctypes.byref(fo)), "ftab_entries")
        return int(b.value), bool(fo.value), out

    def skip_table(self):
        """Test accessor: (J, uint32 [rows, 2] of {row, code}) of the single-device copy's skip table."""
        rows = int(self.header()["bwtsize"])
        out = np.empty((rows, 2), dtype=np.uint32)
        j = ctypes.c_uint32(0)
        _check(load().kfmi_device_skip_table(self._p, out.ctypes.data_as(ctypes.c_void_p), rows, ctypes.byref(j)),
               "skip_table")
        return int(j.value), out

    def sa(self):
        """(rate, uint32 view of the row-sampled suffix array); (0, empty) when absent."""
        p = ctypes.c_void_p()
        n = ctypes.c_uint64()
        rate = ctypes.c_uint32()
        _check(load().kfmi_index_sa(self._p, ctypes.byref(p), ctypes.byref(n), ctypes.byref(rate)), "index_sa")
        if not n.value:
            return 0, np.zeros(0, dtype=np.uint32)
        return int(rate.value), _owned_view(p.value, 4 * n.value, np.uint32, self)

    def save_sa(self, fn) -> None:
        _check(load().kfmi_save_sa(str(fn).encode(), self._p), f"save_sa {fn}")

    def load_sa(self, fn) -> None:
        _check(load().kfmi_load_sa(str(fn).encode(), self._p), f"load_sa {fn}")

    def free_gpu(self) -> None:
        load().freeIndexGPU(ctypes.byref(self._p))


class Queries(_Handle):
    """`qrys_t` (common.h:64-69): num reads of `size` ASCII bases, plain layout."""
    _free = "freeQueries"

    @classmethod
    def from_array(cls, q: np.ndarray) -> "Queries":
        q = np.ascontiguousarray(q, dtype=np.uint8)
        n, m = q.shape
        p = ctypes.c_void_p()
        _check(load().kfmi_queries_from_buffer(q.ctypes.data, n, m, ctypes.byref(p)), "queries_from_buffer")
        return cls(p.value)

    @classmethod
    def load(cls, path, size: int, num: int) -> "Queries":
        p = ctypes.c_void_p()
        _check(load().loadQueries(str(path).encode(), size, num, ctypes.byref(p)), f"loadQueries {path}")
        return cls(p.value)

    @classmethod
    def load_gpu(cls, path, size: int, num: int = 0) -> "Queries":
        """FASTA parsed on the device (kfmi_load_queries_gpu); num = 0: every read."""
        p = ctypes.c_void_p()
        _check(load().kfmi_load_queries_gpu(str(path).encode(), size, num, ctypes.byref(p)),
               f"kfmi_load_queries_gpu {path}")
        return cls(p.value)

    def num(self) -> int:
        return int(ctypes.c_uint64.from_address(self._p.value).value)

    def free_gpu(self) -> None:
        load().freeQueriesGPU(ctypes.byref(self._p))


class Results(_Handle):
    """`res_t` (common.h:77-81): 2*num u32 [L0,R0,L1,R1,...]."""
    _free = "freeResults"

    @classmethod
    def alloc(cls, num: int) -> "Results":
        p = ctypes.c_void_p()
        _check(load().kfmi_results_alloc(num, ctypes.byref(p)), "results_alloc")
        return cls(p.value)

    def array(self) -> np.ndarray:
        L = load()
        n = int(L.kfmi_results_num(self._p))
        ptr = L.kfmi_results_host(self._p)
        if not n:
            return np.zeros(0, dtype=np.uint32)
        return _owned_view(ctypes.cast(ptr, ctypes.c_void_p).value, 8 * n, np.uint32, self)

    def save(self, fn) -> None:
        _check(load().saveResults(str(fn).encode(), self._p, None), f"saveResults {fn}")

    def free_gpu(self) -> None:
        load().freeResultsGPU(ctypes.byref(self._p))


def transfer_to_gpu(index: Index | None, queries: Queries | None, results: Results | None) -> None:
    _check(load().transferCPUtoGPU(index.ptr if index else None, queries.ptr if queries else None,
                                   results.ptr if results else None), "transferCPUtoGPU")


def search(index: Index, queries: Queries, results: Results) -> None:
    _check(load().kfmi_search(index.ptr, queries.ptr, results.ptr), "searchIndexGPU")


def transfer_to_cpu(results: Results) -> None:
    _check(load().transferGPUtoCPU(results.ptr), "transferGPUtoCPU")


def count_blocks(index: Index, queries: Queries) -> int:
    n = ctypes.c_uint64()
    _check(load().kfmi_count_blocks(index.ptr, queries.ptr, ctypes.byref(n)), "count_blocks")
    return int(n.value)


def count_lines(index: Index, queries: Queries) -> dict:
    """kfmi_count_lines: the 128-B lines the backend's fetches touch over the batch."""
    out = (ctypes.c_uint64 * 4)()
    _check(load().kfmi_count_lines(index.ptr, queries.ptr, out), "count_lines")
    return {"lines": int(out[0]), "counter_outside_planes_line": int(out[1]), "ends_fetched": int(out[2]),
            "line_local_ends": int(out[3])}


def probe_replay(index: Index, queries: Queries, unroll: int = 1, reps: int = 5, groups: int = 1) -> dict:
    """kfmi_probe_replay: the search's own line requests replayed without the
    LF dependence (MID layouts, K = 2); returns ms per launch, lines per
    launch, trace bytes and the line rate."""
    ms, lines, tb = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(load().kfmi_probe_replay(index.ptr, queries.ptr, int(unroll), int(groups), int(reps), ctypes.byref(ms),
                                    ctypes.byref(lines), ctypes.byref(tb)), "kfmi_probe_replay")
    return {"unroll": int(unroll), "groups": int(groups), "ms": ms.value, "lines": int(lines.value), "trace_bytes": int(tb.value),
            "G_lines_per_s": lines.value / (ms.value / 1e3) / 1e9 if ms.value > 0 else None}


class Locations(_Handle):
    """Output of kfmi_locate: offsets uint64[num+1], positions uint32[total]."""
    _free = "kfmi_locations_free"

    _num = 0

    def offsets(self) -> np.ndarray:
        return _owned_view(load().kfmi_locations_offsets(self._p), 8 * (self._num + 1), np.uint64, self)

    def positions(self) -> np.ndarray:
        L = load()
        t = self.total()
        if not t:
            return np.zeros(0, dtype=np.uint32)
        return _owned_view(L.kfmi_locations_positions(self._p), 4 * t, np.uint32, self)

    def total(self) -> int:
        return int(load().kfmi_locations_total(self._p))


def locate(index: Index, results: Results, max_occ: int = 0) -> Locations:
    """Text positions of every row of each query's [L, R) (results on the device)."""
    p = ctypes.c_void_p()
    _check(load().kfmi_locate(index.ptr, results.ptr, int(max_occ), ctypes.byref(p)), "kfmi_locate")
    loc = Locations(p.value)
    loc._num = int(load().kfmi_results_num(results.ptr))
    return loc


def locate_array(index: Index, queries: np.ndarray, backend: str | None = None, max_occ: int = 0):
    """Search + locate of uint8 [N, m] reads; returns (results uint32[2N],
    offsets uint64[N+1], positions uint32[total])."""
    if backend:
        set_backend(backend)
    q = Queries.from_array(queries)
    r = Results.alloc(queries.shape[0])
    transfer_to_gpu(index, q, r)
    search(index, q, r)
    loc = locate(index, r, max_occ)
    transfer_to_cpu(r)
    out = (r.array().copy(), loc.offsets().copy(), loc.positions().copy())
    loc.close()
    q.close()
    r.close()
    return out


class _Pinned:
    """Owner of a kfmi_host_alloc block (freed when the last view goes)."""

    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        _check(load().kfmi_host_alloc(int(nbytes), ctypes.byref(self.ptr)), "kfmi_host_alloc")
        self.nbytes = int(nbytes)

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.kfmi_host_free(self.ptr)
            self.ptr = ctypes.c_void_p()


def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """numpy array in pinned host memory (DMA'd directly by search_stream)."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    owner = _Pinned(max(n, 1))
    return _owned_view(owner.ptr.value, n, dt, owner).reshape(shape)


def pack_queries(reads: np.ndarray) -> np.ndarray:
    """Host 2-bit packing of uint8 [N, m] reads (kfmi_pack_queries): uint32
    [ceil(m/16), N], word-major, the words the search consumes."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, m = reads.shape
    out = np.empty(((m + 15) // 16, n), dtype=np.uint32)
    _check(load().kfmi_pack_queries(reads.ctypes.data, n, m, out.ctypes.data), "kfmi_pack_queries")
    return out


def pack_queries_k(reads: np.ndarray, k: int) -> np.ndarray:
    """Host packing for a K-step index and any read length (kfmi_pack_queries_k):
    uint32 [rows, N], the K-step stream of bases 0 .. m-r-1 plus, for r = m % K
    > 0, a row of remainder codes."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, m = reads.shape
    r = m % k
    out = np.empty(((m - r + 15) // 16 + (1 if r else 0), n), dtype=np.uint32)
    _check(load().kfmi_pack_queries_k(reads.ctypes.data, n, m, int(k), out.ctypes.data), "kfmi_pack_queries_k")
    return out


STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3


def _strand_count(strands: int) -> int:
    """Intervals per read of a strand mode (an invalid mode is left to the library's argument check)."""
    return 2 if int(strands) == STRAND_BOTH else 1


def revcomp(reads: np.ndarray) -> np.ndarray:
    """Reverse strand of uint8 [N, m] reads on the host (kfmi_revcomp_queries):
    P'[j] = "ACGT"[3 - base2index(P[m-1-j])]."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, m = reads.shape
    out = np.empty_like(reads)
    _check(load().kfmi_revcomp_queries(reads.ctypes.data, n, m, out.ctypes.data), "kfmi_revcomp_queries")
    return out


def strand_words_host(words: np.ndarray, m: int, k: int, strands: int) -> np.ndarray:
    """kfmi_strand_words_host: the task columns of `strands` (REV / BOTH) from
    pack_queries_k's uint32 [rows, N] forward words, by the device kernel's own
    code run on the host; uint32 [rows, ns * N]."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rows, n = words.shape
    out = np.empty((rows, _strand_count(strands) * n), dtype=np.uint32)
    _check(load().kfmi_strand_words_host(words.ctypes.data, n, int(m), int(k), int(strands), out.ctypes.data),
           "kfmi_strand_words_host")
    return out


def reverse_stream_host(words: np.ndarray, m: int, maxw: int) -> np.ndarray:
    """kfmi_reverse_stream_host: reverse_stream<maxw> (the register form the
    ASCII-fed strand kernels run) of every column of uint32 [maxw, N] forward
    code words, 16 bases per word, zero above base m-1; uint32 [maxw, N]."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rows, n = words.shape
    if rows != int(maxw):
        raise KfmiError(33, "kfmi_reverse_stream_host")
    out = np.empty((rows, n), dtype=np.uint32)
    _check(load().kfmi_reverse_stream_host(words.ctypes.data, n, int(m), int(maxw), out.ctypes.data),
           "kfmi_reverse_stream_host")
    return out


def search_strands(index: Index, queries: Queries, results: Results, strands: int) -> None:
    """kfmi_search_strands: the resident search of the reads as written (STRAND_FWD),
    of their reverse strands (STRAND_REV) or of both (STRAND_BOTH: results of
    2 * num intervals, 2q forward, 2q + 1 reverse)."""
    _check(load().kfmi_search_strands(index.ptr, queries.ptr, results.ptr, int(strands)), "kfmi_search_strands")


def search_stream(index: Index, reads: np.ndarray, out: np.ndarray | None = None, chunk: int = 0,
                  strands: int = STRAND_FWD) -> np.ndarray:
    """Streamed search of uint8 [N, m] host reads against an index already on the
    device (transfer_to_gpu(index, None, None)); returns uint32[2N], or
    uint32[4N] for strands=STRAND_BOTH (interval 2q forward, 2q + 1 reverse)."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, m = reads.shape
    ns = _strand_count(strands)
    if out is None:
        out = np.empty(2 * ns * n, dtype=np.uint32)
    assert out.dtype == np.uint32 and out.flags.c_contiguous and out.size >= 2 * ns * n
    if int(strands) == STRAND_FWD:
        _check(load().kfmi_search_stream(index.ptr, reads.ctypes.data, n, m, out.ctypes.data, int(chunk)),
               "kfmi_search_stream")
    else:
        _check(load().kfmi_search_stream_strands(index.ptr, reads.ctypes.data, n, m, out.ctypes.data, int(chunk),
                                                 int(strands)), "kfmi_search_stream_strands")
    return out


def search_cpu(index: Index, queries: Queries, results: Results, nthreads: int = 0) -> None:
    """searchIndexCPU in its own OpenMP region (kfmi_search_cpu): the host search."""
    _check(load().kfmi_search_cpu(index.ptr, queries.ptr, results.ptr, int(nthreads)), "searchIndexCPU")


def search_cpu_strands(index: Index, queries: Queries, results: Results, strands: int, nthreads: int = 0) -> None:
    """kfmi_search_cpu_strands: the host search of the strands' tasks."""
    _check(load().kfmi_search_cpu_strands(index.ptr, queries.ptr, results.ptr, int(strands), int(nthreads)),
           "kfmi_search_cpu_strands")


def search_cpu_array(index: Index, queries: np.ndarray, nthreads: int = 0, strands: int = STRAND_FWD) -> np.ndarray:
    """One-shot host search of uint8 [N, m] reads (searchIndexCPU); uint32[2N]
    (uint32[4N] for strands=STRAND_BOTH)."""
    q = Queries.from_array(queries)
    r = Results.alloc(_strand_count(strands) * queries.shape[0])
    try:
        if int(strands) == STRAND_FWD:
            search_cpu(index, q, r, nthreads)
        else:
            search_cpu_strands(index, q, r, strands, nthreads)
        return r.array().copy()
    finally:
        q.close()
        r.close()


def search_array(index: Index, queries: np.ndarray, backend: str | None = None,
                 strands: int = STRAND_FWD) -> np.ndarray:
    """One-shot GPU search of uint8 [N, m] reads; returns uint32[2N]
    (uint32[4N] for strands=STRAND_BOTH)."""
    if backend:
        set_backend(backend)
    q = Queries.from_array(queries)
    r = Results.alloc(_strand_count(strands) * queries.shape[0])
    try:
        transfer_to_gpu(index, q, r)
        if int(strands) == STRAND_FWD:
            search(index, q, r)
        else:
            search_strands(index, q, r, strands)
        transfer_to_cpu(r)
        return r.array().copy()
    finally:
        q.close()
        r.close()


TRACE_JUMP_OUTCOMES = ("taken", "refused", "differed", "bad_isa")
TRACE_FIELDS = ("steps", "skip_hits", "skip_misses", "jump_tried", "jump_pos", "jump_nb", "jump_line",
                "jump_outcome", "start_steps", "jump_split")


def decode_trace(records: np.ndarray) -> dict:
    """The named fields of kfmi_search_trace's records (uint32 [N, 4],
    kstep_fmi.h): int64 arrays of N per name in TRACE_FIELDS.  jump_outcome
    indexes TRACE_JUMP_OUTCOMES and is -1, like jump_pos / jump_nb / jump_line,
    for a read that never tried the jump."""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, 4).astype(np.int64)
    tried = r[:, 1] & 1
    no = tried == 0
    return {
        "steps": r[:, 0] & 0xFFFF,
        "skip_hits": (r[:, 0] >> 16) & 0xFF,
        "skip_misses": (r[:, 0] >> 24) & 0xFF,
        "jump_tried": tried,
        "jump_pos": np.where(no, -1, (r[:, 1] >> 4) & 0xFFF),
        "jump_nb": np.where(no, -1, (r[:, 1] >> 16) & 0xFFFF),
        "jump_line": np.where(no, -1, (r[:, 1] >> 1) & 1),
        "jump_outcome": np.where(no, -1, (r[:, 1] >> 2) & 3),
        "start_steps": r[:, 2] & 0x7FFFFFFF,
        "jump_split": r[:, 3],
    }


def trace_start_folded(records: np.ndarray) -> np.ndarray:
    """Bit 31 of word 2 of kfmi_search_trace's records (KFMI_TRACE_START_FOLDED):
    1 where the read's jump used the text position its jump-start entry carried
    (a folded table), so no SA load was issued; int64 [N]."""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, 4).astype(np.int64)
    return (r[:, 2] >> 31) & 1


def search_trace(index: Index, reads: np.ndarray, backend: str | None = None):
    """kfmi_search_trace, one shot: the search search_array runs on uint8
    [N, m] reads under the calling thread's settings, with the traced kernels.
    Returns (intervals uint32 [2N], records uint32 [N, 4]); decode_trace names
    the records' fields.  For tests and diagnosis; not timed."""
    if backend:
        set_backend(backend)
    q = Queries.from_array(reads)
    r = Results.alloc(reads.shape[0])
    rec = np.zeros((reads.shape[0], 4), dtype=np.uint32)
    try:
        transfer_to_gpu(index, q, r)
        _check(load().kfmi_search_trace(index.ptr, q.ptr, r.ptr, rec.ctypes.data_as(ctypes.c_void_p)),
               "kfmi_search_trace")
        transfer_to_cpu(r)
        return r.array().copy(), rec
    finally:
        q.close()
        r.close()


def search_seeds(index: Index, queries: Queries, intervals: Results, spans: Results, max_seeds: int,
                 strands: int = STRAND_FWD) -> None:
    """kfmi_search_seeds: every task's greedy right-to-left maximal exact
    segments, max_seeds slots per task: slot t * max_seeds + s of `intervals`
    holds (L, R) of record s of task t, of `spans` its (start, len); both handles
    have max_seeds * ns * num entries and are on the device."""
    _check(load().kfmi_search_seeds(index.ptr, queries.ptr, intervals.ptr, spans.ptr, int(max_seeds), int(strands)),
           "kfmi_search_seeds")


def search_seeds_cpu(index: Index, queries: Queries, intervals: Results, spans: Results, max_seeds: int,
                     strands: int = STRAND_FWD, nthreads: int = 0) -> None:
    """kfmi_search_seeds_cpu: the same tasks and slots on the host."""
    _check(load().kfmi_search_seeds_cpu(index.ptr, queries.ptr, intervals.ptr, spans.ptr, int(max_seeds),
                                        int(strands), int(nthreads)), "kfmi_search_seeds_cpu")


def search_seeds_array(index: Index, reads: np.ndarray, backend: str | None = None, max_seeds: int = 4,
                       strands: int = STRAND_FWD, cpu: bool = False):
    """One-shot seed search of uint8 [N, m] reads on the GPU (cpu=True: on the
    host); returns (intervals, spans), both uint32 [ns * N, max_seeds, 2]."""
    if backend and not cpu:
        set_backend(backend)
    n, s = reads.shape[0], int(max_seeds)
    slots = max(s, 0) * _strand_count(strands) * n
    q = Queries.from_array(reads)
    iv, sp = Results.alloc(slots), Results.alloc(slots)
    try:
        if cpu:
            search_seeds_cpu(index, q, iv, sp, s, strands)
        else:
            transfer_to_gpu(index, q, iv)
            transfer_to_gpu(index, None, sp)
            search_seeds(index, q, iv, sp, s, strands)
            transfer_to_cpu(iv)
            transfer_to_cpu(sp)
        shape = (_strand_count(strands) * n, s, 2)
        return iv.array().copy().reshape(shape), sp.array().copy().reshape(shape)
    finally:
        q.close()
        iv.close()
        sp.close()


SEED_TRACE_FIELDS = ("steps", "skip_hits", "skip_misses", "start_hits", "start_empty", "lone_units", "records")
TRACE_KERNELS = ("seed_kernel", "seed_strands_kernel", "seed_words_kernel", "task_strands_kernel",
                 "task_words_skip_kernel")
# launch_plan's kernels: those the trace records name, then the forward search's (KFMI_TRACE_KERNEL_TASK_FUSED ..)
PLAN_KERNELS = TRACE_KERNELS + ("task_kernel fused", "task_kernel tables", "task_kernel jump", "task_kernel words",
                                "coop_kernel")
PLAN_FIELDS = ("form", "maxw", "words_maxw", "pack", "kernel")
PLAN_PACKS = ("none", "forward", "strands from ascii", "strands from words")
LAUNCH_ID_FIELDS = ("form", "maxw", "kernel", "skip_split", "ftab_folded", "ftab_steps")


def decode_seed_trace(records: np.ndarray) -> dict:
    """The named fields of words 0 .. 2 of kfmi_search_seeds_trace's records
    (uint32 [T, 4], kstep_fmi.h): int64 arrays of T per name in
    SEED_TRACE_FIELDS.  decode_launch_id names word 3."""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, 4).astype(np.int64)
    return {
        "steps": r[:, 0] & 0xFFFF,
        "skip_hits": (r[:, 0] >> 16) & 0xFF,
        "skip_misses": (r[:, 0] >> 24) & 0xFF,
        "start_hits": r[:, 1] & 0xFFFF,
        "start_empty": (r[:, 1] >> 16) & 0xFFFF,
        "lone_units": r[:, 2] & 0xFFFF,
        "records": (r[:, 2] >> 16) & 0xFF,
    }


def decode_launch_id(records: np.ndarray) -> dict:
    """Word 3 of the records of kfmi_search_seeds_trace and
    kfmi_search_strands_trace, the launch identity: int64 arrays per name in
    LAUNCH_ID_FIELDS -- the fetch form (8, 7, 4, 1), the code registers (8, 16),
    the kernel (an index into TRACE_KERNELS), skip_split as the kernel received
    it, whether the jump-start table in use is folded and its step count."""
    w = np.asarray(records, dtype=np.uint32).reshape(-1, 4)[:, 3].astype(np.int64)
    return {
        "form": w & 0xF,
        "maxw": 8 * ((w >> 4) & 0xF),
        "kernel": (w >> 8) & 0xF,
        "skip_split": (w >> 12) & 0xF,
        "ftab_folded": (w >> 16) & 1,
        "ftab_steps": (w >> 24) & 0xFF,
    }


def launch_plan(backend: str, k: int, d: int, cls: int, m: int, *, seeds: bool = False, strands: int = 1,
                ascii: bool = True, fused: bool = True, skip: bool = False, jump: bool = False,
                traced: bool = False) -> dict:
    """kfmi_launch_plan: the library's launch plan of one search from values
    alone (no device, no handle) -- PLAN_FIELDS: the fetch form, maxw,
    words_maxw, the pack launch (an index into PLAN_PACKS) and the kernel (an
    index into PLAN_KERNELS).  A refused call raises KfmiError with its code."""
    out = (ctypes.c_int32 * 5)()
    _check(load().kfmi_launch_plan(backend.encode(), int(k), int(d), int(cls), int(m), int(bool(seeds)), int(strands),
                                   int(bool(ascii)), int(bool(fused)), int(bool(skip)), int(bool(jump)), int(bool(traced)),
                                   out), "kfmi_launch_plan")
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def search_strands_trace(index: Index, reads: np.ndarray, backend: str | None = None, strands: int = STRAND_BOTH):
    """kfmi_search_strands_trace, one shot: the search search_array(...,
    strands=) runs (STRAND_REV or STRAND_BOTH) with the traced strand kernels.
    Returns (intervals uint32 [2 * ns * N], records uint32 [ns * N, 4]);
    decode_trace names words 0 .. 2, decode_launch_id word 3."""
    if backend:
        set_backend(backend)
    tasks = _strand_count(strands) * reads.shape[0]
    q = Queries.from_array(reads)
    r = Results.alloc(tasks)
    rec = np.zeros((tasks, 4), dtype=np.uint32)
    try:
        transfer_to_gpu(index, q, r)
        _check(load().kfmi_search_strands_trace(index.ptr, q.ptr, r.ptr, int(strands),
                                                rec.ctypes.data_as(ctypes.c_void_p)), "kfmi_search_strands_trace")
        transfer_to_cpu(r)
        return r.array().copy(), rec
    finally:
        q.close()
        r.close()


def search_seeds_trace(index: Index, reads: np.ndarray, backend: str | None = None, max_seeds: int = 4,
                       strands: int = STRAND_FWD):
    """kfmi_search_seeds_trace, one shot: the search search_seeds_array runs with
    the traced seed kernels.  Returns (intervals, spans, records): the first two
    uint32 [ns * N, max_seeds, 2], records uint32 [ns * N, 4]; decode_seed_trace
    names words 0 .. 2, decode_launch_id word 3."""
    if backend:
        set_backend(backend)
    n, s = reads.shape[0], int(max_seeds)
    tasks = _strand_count(strands) * n
    q = Queries.from_array(reads)
    iv, sp = Results.alloc(max(s, 0) * tasks), Results.alloc(max(s, 0) * tasks)
    rec = np.zeros((tasks, 4), dtype=np.uint32)
    try:
        transfer_to_gpu(index, q, iv)
        transfer_to_gpu(index, None, sp)
        _check(load().kfmi_search_seeds_trace(index.ptr, q.ptr, iv.ptr, sp.ptr, s, int(strands),
                                              rec.ctypes.data_as(ctypes.c_void_p)), "kfmi_search_seeds_trace")
        transfer_to_cpu(iv)
        transfer_to_cpu(sp)
        return iv.array().copy().reshape(tasks, s, 2), sp.array().copy().reshape(tasks, s, 2), rec
    finally:
        q.close()
        iv.close()
        sp.close()


HIT_NONE = 0xFFFFFFFF
HIT_MISM_MASK = 0x0000FFFF
HIT_MULTI = 0x00010000
HIT_SCORED_SHIFT = 20
VERIFY_MAX_OCC = 256
ALIGN_MAX_BAND = 15


def results_to_gpu(results: Results) -> None:
    """kfmi_results_to_device: the handle's host array copied to its device
    array (transfer_to_gpu zeroes that array and copies nothing up)."""
    _check(load().kfmi_results_to_device(results.ptr), "kfmi_results_to_device")


def verify_seeds(index: Index, queries: Queries, intervals: Results, spans: Results, hits: Results, max_seeds: int,
                 strands: int, max_occ: int, max_mism: int) -> None:
    """kfmi_verify_seeds: the best Hamming placement of every task among the
    text positions its seed slots imply (`intervals` / `spans` as search_seeds
    leaves them on the device, at most max_occ rows per slot).  Entry t of
    `hits` (ns * num entries, on the device): x = the origin or HIT_NONE, y =
    mismatches | HIT_MULTI | scored << HIT_SCORED_SHIFT."""
    _check(load().kfmi_verify_seeds(index.ptr, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, int(max_seeds),
                                    int(strands), int(max_occ), int(max_mism)), "kfmi_verify_seeds")


def verify_seeds_cpu(text, sa: np.ndarray, queries: Queries, intervals: Results, spans: Results, hits: Results,
                     max_seeds: int, strands: int, max_occ: int, max_mism: int, nthreads: int = 0) -> None:
    """kfmi_verify_seeds_cpu: the same records on the host, from the text
    (bytes or uint8 array of n bases) and its full suffix array (uint32
    [n + 1], row 0 the '$' suffix) and the handles' host arrays."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    _check(load().kfmi_verify_seeds_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, sa.ctypes.data_as(ctypes.c_void_p),
                                        sa.size, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, int(max_seeds),
                                        int(strands), int(max_occ), int(max_mism), int(nthreads)),
           "kfmi_verify_seeds_cpu")


def align_seeds(index: Index, queries: Queries, intervals: Results, spans: Results, hits: Results, max_seeds: int,
                strands: int, max_occ: int, band: int, max_edits: int) -> None:
    """kfmi_align_seeds: verify_seeds with a banded edit distance (band 0 ..
    ALIGN_MAX_BAND cells either side of each seed's origin) in place of the
    Hamming count.  Entry t of `hits`: x = the smallest begin position of a
    best placement or HIT_NONE, y = edits | HIT_MULTI (best placements begin
    more than 2 * band apart) | scored << HIT_SCORED_SHIFT."""
    _check(load().kfmi_align_seeds(index.ptr, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, int(max_seeds),
                                   int(strands), int(max_occ), int(band), int(max_edits)), "kfmi_align_seeds")


def align_seeds_cpu(text, sa: np.ndarray, queries: Queries, intervals: Results, spans: Results, hits: Results,
                    max_seeds: int, strands: int, max_occ: int, band: int, max_edits: int, nthreads: int = 0) -> None:
    """kfmi_align_seeds_cpu: the same records on the host, with the arguments of verify_seeds_cpu."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    _check(load().kfmi_align_seeds_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, sa.ctypes.data_as(ctypes.c_void_p),
                                       sa.size, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, int(max_seeds),
                                       int(strands), int(max_occ), int(band), int(max_edits), int(nthreads)),
           "kfmi_align_seeds_cpu")


def decode_hits(hits: np.ndarray):
    """(origin int64 with -1 for none, mism, multi, scored) of uint32 [T, 2] hit records."""
    h = np.asarray(hits, dtype=np.uint32).reshape(-1, 2)
    x, y = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    none = x == HIT_NONE
    return (np.where(none, -1, x), np.where(none, 0, y & HIT_MISM_MASK), ((y & HIT_MULTI) != 0) & ~none,
            y >> HIT_SCORED_SHIFT)


SECOND_TRUNCATED = 0x00080000
MAPQ_MAX, MAPQ_PER_EDIT, MAPQ_TRUNCATED = 60, 10, 3


def align_second(index: Index, queries: Queries, intervals: Results, spans: Results, hits: Results, second: Results,
                 max_seeds: int, strands: int, max_occ: int, band: int, max_second: int) -> None:
    """kfmi_align_second: over the candidates of align_seeds, the best banded
    placement that begins more than 2 * band from word x of each task's hit.
    Entry t of `second` (ns * num entries, on the device): x = its smallest
    begin position or HIT_NONE, y = edits | HIT_MULTI | SECOND_TRUNCATED (a slot
    held more rows than max_occ) | counted << HIT_SCORED_SHIFT."""
    _check(load().kfmi_align_second(index.ptr, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, second.ptr,
                                    int(max_seeds), int(strands), int(max_occ), int(band), int(max_second)),
           "kfmi_align_second")


def align_second_cpu(text, sa: np.ndarray, queries: Queries, intervals: Results, spans: Results, hits: Results,
                     second: Results, max_seeds: int, strands: int, max_occ: int, band: int, max_second: int,
                     nthreads: int = 0) -> None:
    """kfmi_align_second_cpu: the same records on the host, with the arguments of align_seeds_cpu."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    _check(load().kfmi_align_second_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, sa.ctypes.data_as(ctypes.c_void_p),
                                        sa.size, queries.ptr, intervals.ptr, spans.ptr, hits.ptr, second.ptr,
                                        int(max_seeds), int(strands), int(max_occ), int(band), int(max_second),
                                        int(nthreads)), "kfmi_align_second_cpu")


def map_quality(index: Index, hits: Results, second: Results, quals: Results, strands: int, max_second: int) -> None:
    """kfmi_map_quality: entry t of `quals` is x = the quality min(MAPQ_MAX,
    MAPQ_PER_EDIT * gap), at most MAPQ_TRUNCATED under SECOND_TRUNCATED, and
    y = gap, the edits between the task's hit and the best of its second, its
    read's other strand (STRAND_BOTH) and max_second + 1."""
    _check(load().kfmi_map_quality(index.ptr, hits.ptr, second.ptr, quals.ptr, int(strands), int(max_second)),
           "kfmi_map_quality")


def map_quality_cpu(hits: Results, second: Results, quals: Results, strands: int, max_second: int) -> None:
    """kfmi_map_quality_cpu: the same records from the handles' host arrays."""
    _check(load().kfmi_map_quality_cpu(hits.ptr, second.ptr, quals.ptr, int(strands), int(max_second)),
           "kfmi_map_quality_cpu")


def decode_second(second: np.ndarray):
    """(begin int64 with -1 for none, edits, multi, truncated, counted) of uint32 [T, 2] second records."""
    h = np.asarray(second, dtype=np.uint32).reshape(-1, 2)
    x, y = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    none = x == HIT_NONE
    return (np.where(none, -1, x), np.where(none, 0, y & HIT_MISM_MASK), ((y & HIT_MULTI) != 0) & ~none,
            (y & SECOND_TRUNCATED) != 0, y >> HIT_SCORED_SHIFT)


def piece_bounds(m: int, pieces: int) -> list:
    """(start, len) of the `pieces` equal consecutive pieces of an m-base read; the last takes the remainder."""
    s, ln = int(pieces), int(m) // int(pieces)
    return [(j * ln, ln if j < s - 1 else int(m) - (s - 1) * ln) for j in range(s)]


def piece_seeds(index: Index, reads: np.ndarray, pieces: int, strands: int, intervals: Results | None = None,
                spans: Results | None = None, cpu: bool = False):
    """Fixed-length seeds: the S = `pieces` slots of every task hold the
    intervals of S equal consecutive pieces of the read (the last takes the
    remainder; a piece of no bases is an ignored slot), so that a near-copy of
    an exactly matching read's locus becomes a candidate -- the greedy seed
    search gives such a read one seed, the whole read.  Each piece is searched
    as a batch of its own with kfmi_search / kfmi_search_strands (cpu=True: the
    host searches) on the backend in effect; a REV task's pieces are those of
    P', piece (start, len) of P' being the reverse strand of P[m - start - len
    .. m - start).  Returns (intervals, spans), uint32 [ns * N, S, 2]; with
    `intervals` and `spans` handles of S * ns * N entries on the device the
    arrays are written to their host arrays and sent up (results_to_gpu)."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, m = reads.shape
    s, ns = int(pieces), _strand_count(strands)
    if s < 1 or s > 8:
        raise KfmiError(33, "piece_seeds")
    iv, sp = np.zeros((ns * n, s, 2), np.uint32), np.zeros((ns * n, s, 2), np.uint32)
    if cpu:
        find = lambda q, st: search_cpu_array(index, q, strands=st)   # noqa: E731
    else:
        find = lambda q, st: search_array(index, q, None, st)         # noqa: E731
    for j, (start, ln) in enumerate(piece_bounds(m, s)):
        if ln == 0 or n == 0:
            continue
        for strand in ((STRAND_FWD, STRAND_REV) if int(strands) == STRAND_BOTH else (int(strands),)):
            rows = slice(strand - 1, None, 2) if ns == 2 else slice(None)
            lo = start if strand == STRAND_FWD else m - start - ln
            iv[rows, j] = find(np.ascontiguousarray(reads[:, lo:lo + ln]), strand).reshape(n, 2)
            sp[rows, j] = (start, ln)
    if intervals is not None:
        intervals.array()[:] = iv.reshape(-1)
        spans.array()[:] = sp.reshape(-1)
        if not cpu:
            results_to_gpu(intervals)
            results_to_gpu(spans)
    return iv, sp


def map_reads_array(index: Index, reads: np.ndarray, backend: str | None = None, max_seeds: int = 4,
                    strands: int = STRAND_BOTH, max_occ: int = 8, max_mism: int | None = None, cpu: bool = False,
                    text=None, band: int | None = None, max_edits: int | None = None, mapq: bool = False,
                    max_second: int | None = None, pieces: int | None = None):
    """Upload, seed search and verify of uint8 [N, m] reads in one call: where
    each task maps and with how many differences.  Returns (origin, mism, multi,
    scored), arrays of ns * N tasks (BOTH: task 2q + strand): origin -1 and
    mism 0 where no scored candidate has at most max_mism mismatches (None:
    no bound).  cpu=True runs both steps on the host and needs `text`, the
    indexed text; the suffix array is the index's own at sampling rate 1, else
    that of a temporary index of `text`.
    band=None scores candidates by their Hamming count (verify_seeds).  An
    integer band takes align_seeds instead: origin is then the begin position
    of the best banded placement, mism its edits, bounded by max_edits (None:
    max_mism's value) -- reads with an indel of up to `band` bases map too.
    pieces=k takes piece_seeds' k fixed-length slots per task in place of the
    greedy seeds (max_seeds is then k).  mapq=True needs a band and returns two
    more arrays, (.., quality, gap): align_second and map_quality with
    max_second (None: max_edits' value) after the align."""
    n, s = reads.shape[0], int(max_seeds if pieces is None else pieces)
    ns = _strand_count(strands)
    mm = 0xFFFFFFFF if max_mism is None else int(max_mism)
    if band is not None and max_edits is not None:
        mm = int(max_edits)
    if mapq and band is None:
        raise ValueError("map_reads_array(mapq=True) needs a band")
    m2 = mm if max_second is None else int(max_second)
    if backend and not cpu:
        set_backend(backend)
    q = Queries.from_array(reads)
    iv, sp, hits = Results.alloc(max(s, 0) * ns * n), Results.alloc(max(s, 0) * ns * n), Results.alloc(ns * n)
    second, quals = (Results.alloc(ns * n), Results.alloc(ns * n)) if mapq else (None, None)
    tmp = None
    try:
        if cpu:
            if text is None:
                raise ValueError("map_reads_array(cpu=True) needs the indexed text")
            rate, sa = index.sa()
            if rate != 1:
                tmp = Index.build(bytes(text), k=1, d=64, sa_rate=1)
                rate, sa = tmp.sa()
            if pieces is None:
                search_seeds_cpu(index, q, iv, sp, s, strands)
            else:
                piece_seeds(index, reads, s, strands, iv, sp, cpu=True)
            if band is None:
                verify_seeds_cpu(text, sa, q, iv, sp, hits, s, strands, max_occ, mm)
            else:
                align_seeds_cpu(text, sa, q, iv, sp, hits, s, strands, max_occ, band, mm)
            if mapq:
                align_second_cpu(text, sa, q, iv, sp, hits, second, s, strands, max_occ, band, m2)
                map_quality_cpu(hits, second, quals, strands, m2)
        else:
            transfer_to_gpu(index, q, iv)
            transfer_to_gpu(index, None, sp)
            transfer_to_gpu(index, None, hits)
            if pieces is None:
                search_seeds(index, q, iv, sp, s, strands)
            else:
                piece_seeds(index, reads, s, strands, iv, sp)
            if band is None:
                verify_seeds(index, q, iv, sp, hits, s, strands, max_occ, mm)
            else:
                align_seeds(index, q, iv, sp, hits, s, strands, max_occ, band, mm)
            if mapq:
                transfer_to_gpu(index, None, second)
                transfer_to_gpu(index, None, quals)
                align_second(index, q, iv, sp, hits, second, s, strands, max_occ, band, m2)
                map_quality(index, hits, second, quals, strands, m2)
                transfer_to_cpu(quals)
            transfer_to_cpu(hits)
        out = decode_hits(hits.array().copy())
        if mapq:
            ql = quals.array().copy().reshape(-1, 2).astype(np.int64)
            out += (ql[:, 0], ql[:, 1])
        return out
    finally:
        if tmp is not None:
            tmp.close()
        for h in (q, iv, sp, hits, second, quals):
            if h is not None:
                h.close()


PATH_EDITS_MASK = 0x0000FFFF
PATH_RUNS_SHIFT = 16
PATH_RUNS_MASK = 0x00000FFF
PATH_OVERFLOW = 0x80000000
PATH_MAX_ENTRIES = 32
CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}


def align_paths(index: Index, queries: Queries, hits: Results, paths: Results, cigars: Results, strands: int, band: int,
                max_edits: int, cigar_entries: int) -> None:
    """kfmi_align_paths: the CIGAR and the end position of every task's
    placement at the begin position word x of its entry of `hits` holds (as
    align_seeds or verify_seeds leaves it on the device).  Entry t of `paths`
    (ns * num entries): x = the end position or HIT_NONE, y = edits | runs <<
    PATH_RUNS_SHIFT | PATH_OVERFLOW.  `cigars` (ns * num * cigar_entries
    entries): task t's 2 * cigar_entries words, run r = len << 4 | op with
    BAM's codes I 1, D 2, = 7, X 8."""
    _check(load().kfmi_align_paths(index.ptr, queries.ptr, hits.ptr, paths.ptr, cigars.ptr, int(strands), int(band),
                                   int(max_edits), int(cigar_entries)), "kfmi_align_paths")


def align_paths_cpu(text, queries: Queries, hits: Results, paths: Results, cigars: Results, strands: int, band: int,
                    max_edits: int, cigar_entries: int, nthreads: int = 0) -> None:
    """kfmi_align_paths_cpu: the same records on the host, from the text (bytes
    or uint8 array of n bases) and the handles' host arrays."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    _check(load().kfmi_align_paths_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, queries.ptr, hits.ptr, paths.ptr,
                                       cigars.ptr, int(strands), int(band), int(max_edits), int(cigar_entries),
                                       int(nthreads)), "kfmi_align_paths_cpu")


def set_path_chunk(tasks: int) -> None:
    """kfmi_set_path_chunk (process-wide test knob): align_paths launches chunks
    of `tasks` tasks, rounded up to a multiple of 64; 0 = by the workspace cap."""
    _check(load().kfmi_set_path_chunk(int(tasks)), "kfmi_set_path_chunk")


def decode_paths(paths: np.ndarray):
    """(end int64 with -1 for none, edits, runs, overflow) of uint32 [T, 2] path records."""
    p = np.asarray(paths, dtype=np.uint32).reshape(-1, 2)
    x, y = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    none = x == HIT_NONE
    return (np.where(none, -1, x), np.where(none, 0, y & PATH_EDITS_MASK),
            np.where(none, 0, (y >> PATH_RUNS_SHIFT) & PATH_RUNS_MASK), ((y & PATH_OVERFLOW) != 0) & ~none)


def cigar_strings(paths: np.ndarray, cigars: np.ndarray, cigar_entries: int) -> list:
    """One string per task, "57=1X42="-style, from the records of align_paths:
    "*" where the task has no path or its path overflowed its words."""
    _, _, runs, over = decode_paths(paths)
    words = np.asarray(cigars, dtype=np.uint32).reshape(runs.size, 2 * int(cigar_entries))
    out = []
    for t in range(runs.size):
        if runs[t] == 0 or over[t]:
            out.append("*")
        else:
            out.append("".join("%d%s" % (int(v) >> 4, CIGAR_OPS[int(v) & 15]) for v in words[t, :runs[t]]))
    return out


def map_paths_array(index: Index, reads: np.ndarray, backend: str | None = None, max_seeds: int = 4,
                    strands: int = STRAND_BOTH, max_occ: int = 8, band: int = 3, max_edits: int | None = None,
                    cigar_entries: int = 8):
    """Upload, seed search, align_seeds and align_paths of uint8 [N, m] reads
    in one call, all on the device: how each task lies on the text.  Returns
    (begin, end, edits, cigar): int64 arrays of ns * N tasks (BOTH: task 2q +
    strand) with -1 / -1 / 0 where the task is not placed, and a list of CIGAR
    strings ("*" where there is none).  edits are those of the path at the
    reported begin position, bounded by max_edits (None: no bound)."""
    n, s = reads.shape[0], int(max_seeds)
    ns = _strand_count(strands)
    me = 0xFFFFFFFF if max_edits is None else int(max_edits)
    c = int(cigar_entries)
    if backend:
        set_backend(backend)
    q = Queries.from_array(reads)
    iv, sp = Results.alloc(max(s, 0) * ns * n), Results.alloc(max(s, 0) * ns * n)
    hits, paths, cig = Results.alloc(ns * n), Results.alloc(ns * n), Results.alloc(max(c, 0) * ns * n)
    try:
        transfer_to_gpu(index, q, iv)
        for h in (sp, hits, paths, cig):
            transfer_to_gpu(index, None, h)
        search_seeds(index, q, iv, sp, s, strands)
        align_seeds(index, q, iv, sp, hits, s, strands, max_occ, band, me)
        align_paths(index, q, hits, paths, cig, strands, band, me, c)
        for h in (hits, paths, cig):
            transfer_to_cpu(h)
        end, edits, _, _ = decode_paths(paths.array())
        begin = np.where(end < 0, -1, hits.array().reshape(-1, 2)[:, 0].astype(np.int64))
        return begin, end, edits, cigar_strings(paths.array(), cig.array(), c)
    finally:
        for h in (q, iv, sp, hits, paths, cig):
            h.close()


SAM_CIGAR_M = 1
SAM_NONE, SAM_OVERFLOW, SAM_SPAN = 0, 1, 2


class Contigs(_Handle):
    """kfmi_contigs_create: the sequences of a concatenated text, contig i the
    text positions [begins[i], begins[i] + lengths[i]) under names[i]."""
    _free = "kfmi_contigs_free"

    @classmethod
    def create(cls, names, begins, lengths) -> "Contigs":
        raw = b"".join((n if isinstance(n, bytes) else str(n).encode()) + b"\0" for n in names)
        b = np.ascontiguousarray(begins, dtype=np.uint32)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        if b.size != len(names) or ln.size != len(names):
            raise KfmiError(33, "kfmi_contigs_create")
        out = ctypes.c_void_p()
        _check(load().kfmi_contigs_create(ctypes.c_char_p(raw), b.ctypes.data_as(ctypes.c_void_p),
                                          ln.ctypes.data_as(ctypes.c_void_p), len(names), ctypes.byref(out)),
               "kfmi_contigs_create")
        return cls(out.value)

    def header(self) -> bytes:
        """kfmi_sam_header: "@HD" and one "@SQ" line per contig."""
        need = load().kfmi_sam_header(self.ptr, None, 0)
        if need < 0:
            raise KfmiError(-need, "kfmi_sam_header")
        buf = ctypes.create_string_buffer(int(need) + 1)
        load().kfmi_sam_header(self.ptr, buf, need)
        return buf.raw[:need]


def fasta_contigs(data: bytes):
    """(text, Contigs) of a multi-record FASTA: the records' sequence bytes
    concatenated with no separator under the `map` alphabet's byte mapping
    ("ACGT"[base2index(byte)]: lowercase -> uppercase, N -> G), each record a
    contig named by its header line up to the first whitespace."""
    code = np.arange(256, dtype=np.uint32)
    f2, b1 = code & 2, code & 4
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)[(b1 | np.where(b1 != 0, f2 ^ 2, f2)) >> 1]
    names, begins, lengths, parts, pos = [], [], [], [], 0
    for line in bytes(data).splitlines():
        line = line.strip()
        if line.startswith(b">"):
            head = line[1:].split()
            names.append(head[0] if head else b"")
            begins.append(pos)
            lengths.append(0)
        elif line:
            if not names:
                raise ValueError("fasta_contigs: sequence before the first '>' line")
            parts.append(lut[np.frombuffer(line, dtype=np.uint8)])
            lengths[-1] += len(line)
            pos += len(line)
    text = np.concatenate(parts).tobytes() if parts else b""
    return text, Contigs.create(names, begins, lengths)


class Sam(_Handle):
    """A batch's SAM lines (kfmi_sam_lines / kfmi_sam_lines_cpu): one per read."""
    _free = "kfmi_sam_free"

    @property
    def num(self) -> int:
        return int(load().kfmi_sam_num(self.ptr))

    @property
    def nbytes(self) -> int:
        return int(load().kfmi_sam_bytes(self.ptr))

    def offsets(self) -> np.ndarray:
        """uint64 [num + 1]: where each read's line begins, and the total."""
        return _owned_view(load().kfmi_sam_offsets(self.ptr), 8 * (self.num + 1), np.uint64, self).copy()

    def text(self) -> bytes:
        """The lines' bytes; copied from the device at the first call."""
        addr = load().kfmi_sam_text(self.ptr)
        if not addr:
            raise KfmiError(32, "kfmi_sam_text")
        return ctypes.string_at(addr, self.nbytes)

    def lines(self) -> list:
        """One bytes object per read, without the newline."""
        t, off = self.text(), self.offsets()
        return [t[int(off[i]):int(off[i + 1]) - 1] for i in range(self.num)]


def sam_lines(index: Index, queries: Queries, contigs: Contigs, hits: Results, paths: Results, cigars: Results,
              quals: Results | None, strands: int, cigar_entries: int, band: int, options: int = 0,
              name_base: int = 0) -> Sam:
    """kfmi_sam_lines: one SAM line per read from the records align_seeds,
    align_paths (at `band`) and map_quality (or None: MAPQ 255) left on the
    device; QNAME is name_base + the read's number.  SAM_CIGAR_M in `options`
    merges adjacent = and X runs into M."""
    out = ctypes.c_void_p()
    _check(load().kfmi_sam_lines(index.ptr, queries.ptr, contigs.ptr, hits.ptr, paths.ptr, cigars.ptr,
                                 quals.ptr if quals is not None else None, int(strands), int(cigar_entries),
                                 int(band), int(options), int(name_base), ctypes.byref(out)), "kfmi_sam_lines")
    return Sam(out.value)


def sam_lines_cpu(text, queries: Queries, contigs: Contigs, hits: Results, paths: Results, cigars: Results,
                  quals: Results | None, strands: int, cigar_entries: int, band: int, options: int = 0,
                  name_base: int = 0, nthreads: int = 0) -> Sam:
    """kfmi_sam_lines_cpu: the same bytes on the host, from the text (bytes or
    uint8 array of n bases) and the handles' host arrays."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    out = ctypes.c_void_p()
    _check(load().kfmi_sam_lines_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, queries.ptr, contigs.ptr, hits.ptr,
                                     paths.ptr, cigars.ptr, quals.ptr if quals is not None else None, int(strands),
                                     int(cigar_entries), int(band), int(options), int(name_base), int(nthreads),
                                     ctypes.byref(out)), "kfmi_sam_lines_cpu")
    return Sam(out.value)


def set_sam_form(form: int) -> None:
    """kfmi_set_sam_form (process-wide test knob): 0 = a wave's lines go through
    its LDS tile, 1 = every lane writes its line straight to device memory."""
    _check(load().kfmi_set_sam_form(int(form)), "kfmi_set_sam_form")


def sam_last_passes():
    """(length pass, scan, write pass) of the calling thread's last sam_lines, ms."""
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    load().kfmi_sam_last_passes(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def map_sam_array(index: Index, reads: np.ndarray, contigs: Contigs, backend: str | None = None, max_seeds: int = 4,
                  strands: int = STRAND_BOTH, max_occ: int = 8, band: int = 3, max_edits: int | None = None,
                  cigar_entries: int = 8, mapq: bool = False, max_second: int | None = None, options: int = 0,
                  name_base: int = 0, cpu: bool = False, text=None) -> bytes:
    """Upload, seed search, align_seeds, (align_second and map_quality when
    mapq), align_paths and sam_lines of uint8 [N, m] reads in one call: the
    header and one line per read, as bytes.  cpu=True chains the host forms
    instead and needs `text`, the indexed text (see map_reads_array)."""
    n, s = reads.shape[0], int(max_seeds)
    ns = _strand_count(strands)
    me = 0xFFFFFFFF if max_edits is None else int(max_edits)
    m2 = me if max_second is None else int(max_second)
    c = int(cigar_entries)
    if backend and not cpu:
        set_backend(backend)
    q = Queries.from_array(reads)
    iv, sp = Results.alloc(max(s, 0) * ns * n), Results.alloc(max(s, 0) * ns * n)
    hits, paths, cig = Results.alloc(ns * n), Results.alloc(ns * n), Results.alloc(max(c, 0) * ns * n)
    second, quals = (Results.alloc(ns * n), Results.alloc(ns * n)) if mapq else (None, None)
    tmp = sam = None
    try:
        if cpu:
            if text is None:
                raise ValueError("map_sam_array(cpu=True) needs the indexed text")
            rate, sa = index.sa()
            if rate != 1:
                tmp = Index.build(bytes(text), k=1, d=64, sa_rate=1)
                rate, sa = tmp.sa()
            search_seeds_cpu(index, q, iv, sp, s, strands)
            align_seeds_cpu(text, sa, q, iv, sp, hits, s, strands, max_occ, band, me)
            if mapq:
                align_second_cpu(text, sa, q, iv, sp, hits, second, s, strands, max_occ, band, m2)
                map_quality_cpu(hits, second, quals, strands, m2)
            align_paths_cpu(text, q, hits, paths, cig, strands, band, me, c)
            sam = sam_lines_cpu(text, q, contigs, hits, paths, cig, quals, strands, c, band, options, name_base)
        else:
            transfer_to_gpu(index, q, iv)
            for h in (sp, hits, paths, cig, second, quals):
                if h is not None:
                    transfer_to_gpu(index, None, h)
            search_seeds(index, q, iv, sp, s, strands)
            align_seeds(index, q, iv, sp, hits, s, strands, max_occ, band, me)
            if mapq:
                align_second(index, q, iv, sp, hits, second, s, strands, max_occ, band, m2)
                map_quality(index, hits, second, quals, strands, m2)
            align_paths(index, q, hits, paths, cig, strands, band, me, c)
            sam = sam_lines(index, q, contigs, hits, paths, cig, quals, strands, c, band, options, name_base)
        return contigs.header() + sam.text()
    finally:
        if sam is not None:
            sam.close()
        if tmp is not None:
            tmp.close()
        for h in (q, iv, sp, hits, paths, cig, second, quals):
            if h is not None:
                h.close()


WINDOW_MAX_LEN = 4096
PAIR_PROPER = 0x00020000
PAIR_RESCUED = 0x00040000


def place_windows(index: Index, queries: Queries, windows: Results, hits: Results, strands: int, max_edits: int) -> None:
    """kfmi_place_windows: the best unbanded semi-global placement of every
    task among the begin positions lo .. lo + len - 1 of entry t = (lo, len) of
    `windows` (caller-filled and sent up with results_to_gpu, or as
    mate_windows leaves it on the device).  Entry t of `hits`: x = the smallest
    begin position of a best placement or HIT_NONE, y = edits | HIT_MULTI."""
    _check(load().kfmi_place_windows(index.ptr, queries.ptr, windows.ptr, hits.ptr, int(strands), int(max_edits)),
           "kfmi_place_windows")


def place_windows_cpu(text, queries: Queries, windows: Results, hits: Results, strands: int, max_edits: int,
                      nthreads: int = 0) -> None:
    """kfmi_place_windows_cpu: the same records on the host, from the text
    (bytes or uint8 array of n bases) and the handles' host arrays."""
    t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text,
                             dtype=np.uint8)
    _check(load().kfmi_place_windows_cpu(t.ctypes.data_as(ctypes.c_void_p), t.size, queries.ptr, windows.ptr, hits.ptr,
                                         int(strands), int(max_edits), int(nthreads)), "kfmi_place_windows_cpu")


def mate_windows(index: Index, hits: Results, windows: Results, read_len: int, min_frag: int, max_frag: int,
                 mode: int = 0) -> None:
    """kfmi_mate_windows: entry t of `windows` (2 * num entries, BOTH order,
    reads 2p and 2p + 1 mates) = the begin positions concordant with the hit of
    t's mate task t ^ 3, or (0, 0).  mode 0 leaves out tasks whose own hit is
    concordant already; mode 1 writes every window."""
    _check(load().kfmi_mate_windows(index.ptr, hits.ptr, windows.ptr, int(read_len), int(min_frag), int(max_frag),
                                    int(mode)), "kfmi_mate_windows")


def mate_windows_cpu(n: int, hits: Results, windows: Results, read_len: int, min_frag: int, max_frag: int,
                     mode: int = 0) -> None:
    """kfmi_mate_windows_cpu: the same windows on the host arrays, for a text of n bases."""
    _check(load().kfmi_mate_windows_cpu(int(n), hits.ptr, windows.ptr, int(read_len), int(min_frag), int(max_frag),
                                        int(mode)), "kfmi_mate_windows_cpu")


def pair_hits(index: Index, hits: Results, rescued: Results, paired: Results, read_len: int, min_frag: int,
              max_frag: int) -> None:
    """kfmi_pair_hits: per pair the concordant combination of own hits and
    rescued records with the fewest edits; `paired` holds one placement per
    read in the hits format, y | PAIR_PROPER | PAIR_RESCUED."""
    _check(load().kfmi_pair_hits(index.ptr, hits.ptr, rescued.ptr, paired.ptr, int(read_len), int(min_frag),
                                 int(max_frag)), "kfmi_pair_hits")


def pair_hits_cpu(hits: Results, rescued: Results, paired: Results, read_len: int, min_frag: int, max_frag: int) -> None:
    """kfmi_pair_hits_cpu: the same choice on the host arrays."""
    _check(load().kfmi_pair_hits_cpu(hits.ptr, rescued.ptr, paired.ptr, int(read_len), int(min_frag), int(max_frag)),
           "kfmi_pair_hits_cpu")


def decode_pairs(paired: np.ndarray):
    """(begin int64 with -1 for none, edits, multi, proper, rescued) of uint32 [T, 2] records of pair_hits."""
    h = np.asarray(paired, dtype=np.uint32).reshape(-1, 2)
    x, y = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    none = x == HIT_NONE
    return (np.where(none, -1, x), np.where(none, 0, y & HIT_MISM_MASK), ((y & HIT_MULTI) != 0) & ~none,
            ((y & PAIR_PROPER) != 0) & ~none, ((y & PAIR_RESCUED) != 0) & ~none)


def map_pairs_array(index: Index, reads: np.ndarray, min_frag: int, max_frag: int, backend: str | None = None,
                    max_seeds: int = 4, max_occ: int = 8, band: int = 3, max_edits: int | None = None,
                    cigar_entries: int = 8, mode: int = 0):
    """Upload, seed search, align_seeds, mate_windows, place_windows, pair_hits
    and align_paths of uint8 [N, m] interleaved mates (reads 2p and 2p + 1) in
    one call, all on the device.  Returns per read (begin, end, strand, edits,
    flags, cigar): int64 arrays of N entries -- begin / end -1, strand -1 and
    edits 0 where the read is not placed; strand 0 = as written, 1 = reverse
    complement; flags = the PAIR_PROPER / PAIR_RESCUED / HIT_MULTI bits of the
    chosen record -- and a list of CIGAR strings ("*" where the read is not
    placed, or where its rescued placement drifts out of `band`).  edits are
    those of the chosen placement, bounded by max_edits (None: no bound)."""
    n, s, m = reads.shape[0], int(max_seeds), reads.shape[1]
    me = 0xFFFFFFFF if max_edits is None else int(max_edits)
    c = int(cigar_entries)
    if backend:
        set_backend(backend)
    q = Queries.from_array(reads)
    iv, sp = Results.alloc(max(s, 0) * 2 * n), Results.alloc(max(s, 0) * 2 * n)
    hits, win, resc, paired, paths = (Results.alloc(2 * n) for _ in range(5))
    cig = Results.alloc(max(c, 0) * 2 * n)
    try:
        transfer_to_gpu(index, q, iv)
        for h in (sp, hits, win, resc, paired, paths, cig):
            transfer_to_gpu(index, None, h)
        search_seeds(index, q, iv, sp, s, STRAND_BOTH)
        align_seeds(index, q, iv, sp, hits, s, STRAND_BOTH, max_occ, band, me)
        mate_windows(index, hits, win, m, min_frag, max_frag, mode)
        place_windows(index, q, win, resc, STRAND_BOTH, me)
        pair_hits(index, hits, resc, paired, m, min_frag, max_frag)
        align_paths(index, q, paired, paths, cig, STRAND_BOTH, band, me, c)
        for h in (paired, paths, cig):
            transfer_to_cpu(h)
        b, e, multi, proper, rescued = decode_pairs(paired.array())
        end, _, _, _ = decode_paths(paths.array())
        cs = cigar_strings(paths.array(), cig.array(), c)
        b, e, end = b.reshape(n, 2), e.reshape(n, 2), end.reshape(n, 2)
        y = paired.array().reshape(n, 2, 2)[:, :, 1].astype(np.int64)
        strand = np.where(b[:, 0] >= 0, 0, np.where(b[:, 1] >= 0, 1, -1))
        k = np.maximum(strand, 0)
        r = np.arange(n)
        placed = strand >= 0
        flags = np.where(placed, y[r, k] & (PAIR_PROPER | PAIR_RESCUED | HIT_MULTI), 0)
        return (b[r, k], np.where(placed, end[r, k], -1), strand, e[r, k], flags,
                [cs[2 * i + int(k[i])] if placed[i] else "*" for i in range(n)])
    finally:
        for h in (q, iv, sp, hits, win, resc, paired, paths, cig):
            h.close()


def env_int(name: str, default: int) -> int:
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default
