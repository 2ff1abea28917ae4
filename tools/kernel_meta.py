#!/usr/bin/env python3
"""Resource figures of the kernels in a gfx950 code object, from its AMDGPU metadata note:
VGPRs, SGPRs, LDS bytes (group segment), scratch bytes (private segment), and each kernel's code
bytes from the symbol table.

  hipcc --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output -O3 -std=c++17 \\
        -I../include -Icsrc -c csrc/zh_decode.hip -o dec.co
  tools/kernel_meta.py dec.co [name-prefix]

Prints one JSON object {kernel: {"vgpr", "sgpr", "lds", "scratch", "code"}}.  Two builds (two commits) are
compared by comparing the two objects; nothing runs on a GPU."""
import json
import re
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
KEYS = {".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds", ".private_segment_fixed_size": "scratch"}


def kernel_meta(path, prefix=""):
    notes = subprocess.run([READELF, "--notes", path], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.groups()
        if k in KEYS:
            cur[KEYS[k]] = int(v)
        elif k == ".symbol":  # the kernel descriptor's symbol names the entry: NAME.kd
            name = v.strip("'\"")
            if name.endswith(".kd"):
                name = name[:-3]
            cur["name"] = name
        if len(cur) == 5:
            if cur["name"].startswith(prefix):
                out[cur.pop("name")] = cur
            cur = {}
    syms = subprocess.run([READELF, "--symbols", "--wide", path], check=True, capture_output=True, text=True).stdout
    for line in syms.splitlines():  # Num: Value Size Type Bind Vis Ndx Name
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in out:
            out[f[7]]["code"] = int(f[2], 0)
    return out


if __name__ == "__main__":
    print(json.dumps(kernel_meta(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""), indent=1, sort_keys=True))
