#!/usr/bin/env python3
"""Kernel metadata of the gfx950 code objects in one or more object files:
one JSON line per kernel with its demangled name, VGPRs, SGPRs, scratch and LDS
bytes, kernarg bytes and code size.  With --against DIR it compares every
kernel whose name matches --match with the same object under DIR (names are
compared after removing the trace policy parameter) and exits 1 on a difference.
With --by-name the comparison is by kernel name across all the objects, for a
change that moves a kernel from one object to another.

  scripts/kernel_meta.py --match 'skip_walk|task_kernel' obj/hip_kfmi_inst_mid_k2.o --against ../parent/obj
  scripts/kernel_meta.py --by-name obj/hip_*.o --against ../parent/obj
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM", "/opt/rocm")) / "llvm" / "bin"


def kernels(obj: Path, arch: str):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = Path(tmp) / "dev.fatbin", Path(tmp) / "dev.co"
        cp = subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(obj)],
                            capture_output=True, text=True)
        if cp.returncode and "section '.hip_fatbin' not found" in cp.stderr:
            return []   # a host-only unit
        if cp.returncode:
            sys.exit(cp.stderr)
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--unbundle", f"--input={fat}",
                        f"--output={co}", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}"], check=True)
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-sW", str(co)], check=True, capture_output=True,
                              text=True).stdout
    size = {}
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    rows = []
    for chunk in notes.split("\n  - .agpr_count:")[1:]:   # one kernel each: its keys are indented by four
        k = dict(re.findall(r"^    (\.\w+):[ \t]+(\S.*)$", chunk, flags=re.M))
        name = k[".name"].strip("'")
        rows.append({"symbol": name, "vgpr": int(k[".vgpr_count"]), "sgpr": int(k[".sgpr_count"]),
                     "scratch": int(k[".private_segment_fixed_size"]), "lds": int(k[".group_segment_fixed_size"]),
                     "kernarg": int(k[".kernarg_segment_size"]), "code": size.get(name, -1)})
    if rows:
        dem = subprocess.run(["c++filt"], input="\n".join(r["symbol"] for r in rows), check=True,
                             capture_output=True, text=True).stdout.splitlines()
        for r, d in zip(rows, dem):
            r["name"] = d
    return rows


def plain(name: str) -> str:
    """The kernel's name without the trace policy: the parent's name."""
    name = re.sub(r"\(.*$", "", name)
    return name.replace(", kfmi::NoTrace>", ">")


FIELDS = ("vgpr", "sgpr", "scratch", "lds", "code", "kernarg")


def by_name(objects, arch: str, match: str):
    """name -> the sorted metadata rows of every kernel of that name in `objects`."""
    out = {}
    for obj in objects:
        for r in kernels(obj, arch):
            if re.search(match, r["name"]):
                out.setdefault(plain(r["name"]), []).append(tuple(r[f] for f in FIELDS))
    return {n: sorted(v) for n, v in out.items()}


def compare_by_name(a) -> int:
    """Every kernel of a.objects against the kernel of the same name in any
    hip_*.o under a.against: a kernel may move to another object.  Prints one
    summary line, then a line per kernel that differs or exists on one side."""
    mine = by_name(a.objects, a.arch, a.match)
    theirs = by_name(sorted(a.against.glob("hip_*.o")), a.arch, a.match)
    diff = sorted(n for n in set(mine) | set(theirs) if mine.get(n) != theirs.get(n))
    print(json.dumps({"kernels_here": sum(map(len, mine.values())), "kernels_there": sum(map(len, theirs.values())),
                      "names": len(mine), "differing": len(diff), "fields": FIELDS}))
    for n in diff:
        print(json.dumps({"kernel": n, "here": mine.get(n), "there": theirs.get(n)}))
    return len(diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("objects", nargs="+", type=Path)
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--match", default=".")
    ap.add_argument("--against", type=Path)
    ap.add_argument("--by-name", action="store_true",
                    help="with --against: compare by kernel name across all objects, not object by object")
    a = ap.parse_args()
    if a.by_name:
        if not a.against:
            ap.error("--by-name needs --against")
        sys.exit(1 if compare_by_name(a) else 0)
    bad = 0
    for obj in a.objects:
        mine = {plain(r["name"]): r for r in kernels(obj, a.arch) if re.search(a.match, r["name"])}
        theirs = None
        if a.against:
            theirs = {plain(r["name"]): r for r in kernels(a.against / obj.name, a.arch) if re.search(a.match, r["name"])}
            if set(mine) != set(theirs):
                bad += 1
                print(json.dumps({"object": obj.name, "only_here": sorted(set(mine) - set(theirs)),
                                  "only_there": sorted(set(theirs) - set(mine))}))
        for n, r in sorted(mine.items()):
            row = {"object": obj.name, "kernel": n, **{f: r[f] for f in ("vgpr", "sgpr", "scratch", "lds", "code", "kernarg")}}
            if theirs and n in theirs:
                t = theirs[n]
                row["parent"] = {f: t[f] for f in ("vgpr", "sgpr", "scratch", "lds", "code", "kernarg")}
                row["equal"] = all(r[f] == t[f] for f in ("vgpr", "sgpr", "scratch", "lds", "code"))
                bad += 0 if row["equal"] else 1
            print(json.dumps(row))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
