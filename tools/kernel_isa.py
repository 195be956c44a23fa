#!/usr/bin/env python3
"""usage: tools/kernel_isa.py <file.hip> <mangled-name substring> [--dump] [--against DIR]  -> instruction counts per basic
block of one kernel (VALU / SALU / LDS / VMEM), from hipcc -S for gfx950.  --dump prints the block bodies.  --against DIR:
the totals only, side by side with those of DIR/<file.hip> compiled against DIR's headers.  DIR holds a copy of another
commit's csrc only: include/ (disenlink_hip.h) is this tree's on both sides, so compare commits that share it."""
import collections
import os
import re
import subprocess
import sys

src, key = sys.argv[1], sys.argv[2]
against = sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else None


def kind(o):
    return ("wait" if o.startswith("s_waitcnt") else "smem" if o.startswith(("s_load", "s_buffer_load")) else "valu" if o.startswith("v_")
            else "salu" if o.startswith("s_") else "lds" if o.startswith("ds_")
            else "vmem" if o.startswith(("global_", "buffer_", "scratch_", "flat_")) else "other")


def blocks_of(path, inc):
    asm = "/tmp/kernel_isa.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-Iinclude", "-I" + inc,
                    "-S", "--cuda-device-only", path, "-o", asm], check=True, stderr=subprocess.DEVNULL)
    lines = open(asm).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % re.escape(key), l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    blocks, cur, name = [], [], "entry"
    for l in lines[start + 1:end + 1]:
        t = l.strip()
        if re.match(r"^\.LBB\S+:", t):
            blocks.append((name, cur))
            name, cur = t.split(":")[0], []
        elif t and not t.startswith((";", ".")):
            cur.append(t)
    blocks.append((name, cur))
    return blocks


blocks = blocks_of(src, "disenlink_amd/csrc")
tot = collections.Counter()
for name, ops in blocks:
    c = collections.Counter(kind(o) for o in ops)
    tot += c
    if against:
        continue
    if len(ops) >= 8:
        print(f"{name:12s} ops {len(ops):4d}  valu {c['valu']:4d}  salu {c['salu'] + c['wait'] + c['smem']:4d}  lds {c['lds']:3d}  vmem {c['vmem']:3d}")
    if "--dump" in sys.argv:
        for o in ops:
            print("      ", o.split(";")[0].rstrip())
print("total", dict(tot))
if against:
    other = collections.Counter(kind(o) for _, ops in blocks_of(os.path.join(against, os.path.basename(src)), against) for o in ops)
    print(f"total in {against}", dict(other))
    print("difference", {k: tot[k] - other[k] for k in sorted(set(tot) | set(other)) if tot[k] != other[k]} or "none")
