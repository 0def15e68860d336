"""Compare the gfx950 kernels of two builds, symbol by symbol (CPU only; nothing is loaded or run).

    python tools/isa_diff.py PARENT TREE [--show NAME_PART] [--vmem NAME_PART] [--rename OLD=NEW ...]

PARENT and TREE are two built libraries (``erasurehead_amd/_C*.so``), two fat objects (``build/objs/*.hip.o``)
or two bare gfx950 code objects.  Every mangled kernel name is disassembled with ``llvm-objdump -d
--no-show-raw-insn``; addresses, branch-target labels and comments are stripped, so two symbols compare equal
exactly when their instruction streams are the same text.  Printed:

* the number of kernel symbols in each build, the names only one has, the number identical;
* per differing symbol the instruction counts, the opcode-histogram delta, and vgpr_count, agpr_count,
  vgpr_spill_count, private_segment_fixed_size and group_segment_fixed_size (static LDS) from the metadata
  notes, parent against tree.

``--show PART`` also prints a unified diff of the differing symbols whose name contains PART; ``--vmem PART``
prints, for those, the sequence of vector-memory instructions, wait counts and barriers of each side, which is
what decides whether a row loop still waits for one row while the prefetched ones stay in flight.

``--rename OLD=NEW`` (repeatable) applies ``re.sub(OLD, NEW)`` to the demangled names of the parent's symbols the
tree lacks and compares each with the tree symbol of that name, so a renamed kernel is compared instead of being
listed on both sides, e.g. ``--rename 'old_reduce<(\w+)>=new_reduce<\1>'``.

This is the recipe docs/PERF_NOTES.md applies to every "nothing may move" refactor.  The exit status is 0
whether or not anything differs: the tool reports, the reader judges.
"""
from __future__ import annotations

import argparse
import collections
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")
NOTE_KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")
FLOW = re.compile(r"^(global_|buffer_|flat_|scratch_)|^s_waitcnt|^s_barrier")


def code_objects(path: str, work: str):
    """The gfx950 code objects inside a library / fat object (or the file itself if it is one)."""
    dst = os.path.join(work, os.path.basename(path))
    shutil.copy(path, dst)
    subprocess.run([OBJDUMP, "--offloading", dst], cwd=work, capture_output=True, check=True)
    found = sorted(glob.glob(dst + ".*gfx950*"))
    return found or [dst]


def functions(co: str):
    """{symbol: [instruction lines]} of one code object, addresses and comments stripped."""
    out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    funcs = {}
    for chunk in re.split(r"\n(?=[0-9a-f]+ <)", out):
        m = re.match(r"[0-9a-f]+ <([^>]+)>:", chunk)
        if not m:
            continue
        body = []
        for line in chunk.splitlines()[1:]:
            line = line.split("//")[0].strip()
            if not line or re.fullmatch(r"<[^>]+>:", line):  # blank, or a branch-target label
                continue
            if line == "...":  # zero padding up to the next symbol: the last symbol of a code object has none
                continue
            body.append(re.sub(r"\s+", " ", line))
        funcs[m.group(1)] = body
    return funcs


def notes(co: str):
    """{kernel name: {note key: int}} from the code object's metadata."""
    out = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        # a kernel's own keys stand at "  - .key:" (its first) and "    .key:"; its arguments' are indented deeper
        m = re.match(r"(  - |    )\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "name":
            res[m.group(3)] = cur
    return {n: {k: int(c.get(k, 0)) for k in NOTE_KEYS} for n, c in res.items()}


def load(path: str, work: str):
    funcs, meta = {}, {}
    for co in code_objects(path, work):
        funcs.update(functions(co))
        meta.update(notes(co))
    kernels = {n: b for n, b in funcs.items() if n in meta}  # kernels only: device functions are all inlined
    return kernels, meta


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if tool is None:
        sys.exit("--rename needs llvm-cxxfilt or c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def renamed(parent, tree, renames):
    """{parent symbol: tree symbol} for the parent's symbols that are the tree's once every OLD=NEW (a regular
    expression and its replacement) is applied to their demangled names."""
    da, db = demangle(sorted(set(parent) - set(tree))), demangle(sorted(set(tree) - set(parent)))
    by_name = {d: n for n, d in db.items()}
    res = {}
    for n, d in da.items():
        for r in renames:
            old, new = r.split("=", 1)
            d = re.sub(old, new, d)
        if d in by_name:
            res[n] = by_name[d]
    return res


def histogram_delta(a, b):
    ha = collections.Counter(l.split()[0] for l in a)
    hb = collections.Counter(l.split()[0] for l in b)
    return {op: hb[op] - ha[op] for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--show", default=None, help="print a unified diff of differing symbols containing this text")
    ap.add_argument("--vmem", default=None, help="print the vector-memory / wait / barrier sequence of those")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="compare a renamed kernel: re.sub(OLD, NEW) on the parent's demangled names (repeatable)")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
        ka, ma = load(a.parent, wa)
        kb, mb = load(a.tree, wb)
    ren = renamed(ka, kb, a.rename) if a.rename else {}
    print(f"kernel symbols: parent {len(ka)}, tree {len(kb)}")
    for title, names in (("only in parent", sorted(set(ka) - set(kb) - set(ren))),
                         ("only in tree", sorted(set(kb) - set(ka) - set(ren.values())))):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", n)
    if ren:
        print(f"renamed: {len(ren)} parent symbols compared with {len(set(ren.values()))} of the tree")
    pairs = [(n, n) for n in sorted(set(ka) & set(kb))] + sorted(ren.items())  # (parent symbol, tree symbol)
    differ = [(p, t) for p, t in pairs if ka[p] != kb[t] or ma[p] != mb[t]]
    print(f"identical: {len(pairs) - len(differ)} of {len(pairs)} common symbols; differing: {len(differ)}")
    for p, n in differ:
        print(f"\n{n}" if p == n else f"\n{p} -> {n}")
        print(f"    instructions {len(ka[p])} -> {len(kb[n])}")
        print("    " + ", ".join(f"{k} {ma[p][k]} -> {mb[n][k]}" for k in NOTE_KEYS))
        delta = histogram_delta(ka[p], kb[n])
        print("    opcodes: " + (", ".join(f"{op} {d:+d}" for op, d in delta.items()) or "same histogram, other order"))
        if a.vmem is not None and a.vmem in n:
            for side, body in (("parent", ka[p]), ("tree", kb[n])):
                print(f"    -- {side}: vector memory, waits, barriers")
                for l in body:
                    if FLOW.match(l):
                        print("      ", l)
        if a.show is not None and a.show in n:
            sys.stdout.writelines(l if l.endswith("\n") else l + "\n"
                                  for l in difflib.unified_diff(ka[p], kb[n], "parent", "tree", lineterm="", n=2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
