"""Compare the gfx950 device code of two builds of libvf_hip.so kernel by kernel.

    python scripts/cmp_device_code.py OLD.so NEW.so [--match SUBSTRING] [--diff N]

Unbundles the device images of both libraries (llvm-objdump --offloading), disassembles them and compares every kernel
symbol's instruction text with addresses and encodings stripped.  Prints the number of kernels, how many bodies are
identical, and for every kernel that differs or exists on one side only: its registers, scratch and spills from the
code object's metadata, and the counts of the instructions a hand-scheduled K loop is made of (over the WHOLE kernel, not
its K loop alone: equal counts here are necessary for equal counts there, not sufficient).  --match keeps only the
kernels whose mangled name contains SUBSTRING (e.g. gemm); --diff N prints the first N differing lines of each.
Exit status 0 when every compared body is identical, 1 otherwise.  Needs no GPU.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ARCH = "gfx950"
COUNTED = ("v_mfma_", "global_load_lds_", "s_barrier", "s_waitcnt vmcnt", "ds_read", "ds_write")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def kernels_of(lib: str, tmp: str) -> dict:
    """{kernel symbol: {"body": [instruction text], "meta": {key: int}}} over every gfx950 image bundled in lib"""
    os.makedirs(tmp)
    shutil.copy(lib, os.path.join(tmp, "lib.so"))
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
    out = {}
    for img in sorted(f for f in os.listdir(tmp) if f.endswith(ARCH)):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", img], cwd=tmp, check=True, capture_output=True, text=True).stdout
        meta, entry = {}, {}
        for line in notes.splitlines() + ["  - "]:         # a kernel's entry: its "  - " line and the keys at that depth (deeper: .args)
            if line.startswith("  - "):
                if ".name" in entry:
                    meta.setdefault(entry[".name"], {}).update({k: int(v) for k, v in entry.items() if k in META})
                entry = {}
            m = re.match(r"(?:  - |    )(\.\w+):\s*(\S+)", line)
            if m:
                entry[m.group(1)] = m.group(2)
        kernel_names = {k for k, v in meta.items() if ".vgpr_count" in v}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", img], cwd=tmp, check=True,
                             capture_output=True, text=True).stdout
        name, ended = None, False
        for line in dis.splitlines():
            m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
            if m:
                if m.group(1) in kernel_names:
                    name, ended = m.group(1), False
                    out[name] = {"body": [], "meta": meta[name]}
                elif not m.group(1).startswith("L"):        # a local label inside the kernel keeps it; another symbol ends it
                    name = None
                continue
            if name and line.strip():
                text = re.sub(r"\s+", " ", line.split("//")[0].strip())
                if ended and text.startswith(("s_nop", "s_code_end")):     # alignment padding behind the last s_endpgm
                    continue
                if text:
                    out[name]["body"].append(text)
                    ended = text.startswith("s_endpgm")
    return out


def describe(k: dict) -> str:
    body = "\n".join(k["body"])
    return "  ".join(f"{key.lstrip('.')}={k['meta'].get(key, '?')}" for key in META) + "\n      " + \
           "  ".join(f"{ins}:{len(re.findall(re.escape(ins), body))}" for ins in COUNTED)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="")
    ap.add_argument("--diff", type=int, default=0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels_of(a.old, os.path.join(tmp, "old")), kernels_of(a.new, os.path.join(tmp, "new"))
    old = {k: v for k, v in old.items() if a.match in k}
    new = {k: v for k, v in new.items() if a.match in k}
    both = sorted(set(old) & set(new))
    same = [k for k in both if old[k]["body"] == new[k]["body"]]
    nonzero = [k for k in new if new[k]["meta"].get(".private_segment_fixed_size") or new[k]["meta"].get(".vgpr_spill_count")
               or new[k]["meta"].get(".sgpr_spill_count")]
    print(f"kernels: old {len(old)}, new {len(new)}, in both {len(both)}; identical bodies {len(same)}; "
          f"new kernels with scratch or spills {len(nonzero)}")
    for k in sorted(set(old) - set(new)):
        print(f"ONLY IN OLD {k}\n  old: {describe(old[k])}")
    for k in sorted(set(new) - set(old)):
        print(f"ONLY IN NEW {k}\n  new: {describe(new[k])}")
    for k in both:
        if k in same:
            continue
        print(f"DIFFERS {k}\n  old: {describe(old[k])}\n  new: {describe(new[k])}")
        if a.diff:
            lines = [d for d in difflib.unified_diff(old[k]["body"], new[k]["body"], lineterm="", n=0) if not d.startswith(("---", "+++"))]
            print("\n".join("    " + d for d in lines[:a.diff]))
    return 0 if len(same) == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
