#!/usr/bin/env python3
"""Compiled-code identity of every gfx950 kernel, checked without a GPU: the proof a refactor of csrc/ has to give.

    python tools/kernel_isa.py dump  TREE  OUT.json [--ablation]
    python tools/kernel_isa.py compare A.json B.json

``dump`` compiles every csrc/*.hip of TREE (a checkout of this repository) device-only with that tree's own build.py
FLAGS, unbundles the gfx950 code object and records, per kernel symbol, a hash of its disassembly (address column and
the ``// addr: bytes <sym+off>`` trailers stripped; branch operands are pc-relative, so a kernel reads the same
wherever it sits in its code object; objdump's ``...`` for the zero padding behind a function, the ``s_nop 0`` padding
behind the last one and the pc-relative address of a constant table are dropped: they depend on what the linker placed next
to the kernel, not on the kernel) and its entry of the amdhsa.kernels note.  The key is the mangled kernel name,
not the file, so a kernel that moved between files compares against itself.  ``compare`` prints every kernel that is
missing, new or different and exits non-zero if there is one.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def _out(*cmd: str) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def _position_free(lines: list) -> list:
    """Drops what depends on where the kernel sits in its code object: the ``s_nop 0`` run that pads the end of the last function, and the
    literal of the ``s_add_u32`` / ``s_addc_u32`` pair behind an ``s_getpc_b64`` (the pc-relative address of a constant table)."""
    while lines and lines[-1] == "s_nop 0":
        lines.pop()
    for i, ln in enumerate(lines):
        if ln.startswith("s_getpc_b64"):
            for j in range(i + 1, min(i + 3, len(lines))):
                lines[j] = re.sub(r"^(s_addc?_u32 s\d+, s\d+), (0x[0-9a-f]+|-?\d+)$", r"\1, <pcrel>", lines[j])
    return lines


def _kernels_of(src: str, flags: list, hipcc: str, tmp: str) -> dict:
    base = os.path.join(tmp, os.path.basename(src)[:-4])
    _out(hipcc, *flags, "--offload-device-only", "-c", src, "-o", base + ".o")
    _out(os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + base + ".o",
         "--targets=" + TARGET, "--output=" + base + ".co")
    notes = {}
    for entry in re.split(r"\n  - ", _out(os.path.join(LLVM, "llvm-readelf"), "--notes", base + ".co"))[1:]:
        fields = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", entry, re.M))
        if "name" in fields:
            notes[fields["name"]] = {k: int(fields[k]) for k in NOTE_KEYS if k in fields}
    text = {}
    for head in re.split(r"\n(?=[0-9a-f]{16} <)", _out(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", base + ".co")):
        m = re.match(r"[0-9a-f]{16} <(.+)>:\n", head)
        if m and m.group(1) in notes:
            text[m.group(1)] = _position_free([ln.split("//")[0].strip() for ln in head[m.end():].splitlines() if ln.strip() not in ("", "...")])
    return {k: {"file": os.path.basename(src), "insns": len(text[k]), "isa_sha256": hashlib.sha256("\n".join(text[k]).encode()).hexdigest(),
                **notes[k]} for k in notes}


def dump(tree: str, out: str, ablation: bool) -> int:
    pkg = next(os.path.join(tree, d) for d in sorted(os.listdir(tree)) if os.path.isfile(os.path.join(tree, d, "build.py")))
    spec = importlib.util.spec_from_file_location("vatl_build_for_isa", os.path.join(pkg, "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    flags = bld.FLAGS + (["-DVATL_ABLATION"] if ablation else [])
    srcs = sorted(os.path.join(bld.CSRC, f) for f in os.listdir(bld.CSRC) if f.endswith(".hip"))
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for got in ex.map(lambda s: _kernels_of(s, flags, bld.HIPCC, tmp), srcs):
            dup = kernels.keys() & got.keys()
            assert not dup, f"kernel defined in two files: {sorted(dup)}"
            kernels.update(got)
    with open(out, "w") as f:
        json.dump(kernels, f, indent=1, sort_keys=True)
    print(f"{len(kernels)} kernels, {sum(k['insns'] for k in kernels.values())} instructions, {len(srcs)} files -> {out}")
    return 0


def compare(a_path: str, b_path: str) -> int:
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    bad = 0
    for k in sorted(a.keys() | b.keys()):
        if k not in a or k not in b:
            print(("NEW      " if k in b else "MISSING  ") + k)
        elif {**a[k], "file": ""} != {**b[k], "file": ""}:
            diff = {f: (a[k].get(f), b[k].get(f)) for f in a[k].keys() | b[k].keys() if f != "file" and a[k].get(f) != b[k].get(f)}
            print(f"DIFFERS  {k}  {diff}")
        else:
            continue
        bad += 1
    moved = sum(1 for k in a.keys() & b.keys() if a[k]["file"] != b[k]["file"])
    print(f"{len(a)} kernels vs {len(b)} kernels: {bad} missing, new or different; {moved} moved to another file")
    return 1 if bad else 0


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--ablation"]
    if len(argv) == 3 and argv[0] == "dump":
        sys.exit(dump(argv[1], argv[2], "--ablation" in sys.argv))
    if len(argv) == 3 and argv[0] == "compare":
        sys.exit(compare(argv[1], argv[2]))
    sys.exit(__doc__)
