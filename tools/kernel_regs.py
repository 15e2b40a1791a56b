#!/usr/bin/env python3
"""Register / spill report of one object of the library: python tools/kernel_regs.py <object name> [substring ...] [-Dmacro ...]
(an instance of easykv_amd/csrc/ekv_instances.def by its object name, e.g. ekv_attn_decode_d128_plain_kv8, or a .hip file's base name)"""
import re, subprocess, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from easykv_amd import _build
name = os.path.basename(sys.argv[1])
name = name[:-4] if name.endswith(".hip") else name
defs = [a for a in sys.argv[2:] if a.startswith("-D")]
filt = [a for a in sys.argv[2:] if not a.startswith("-D")]
args = dict(_build.objects() + _build.added_objects() + _build.later_objects()).get(name)
if args is None:
    sys.exit(f"no object named {name}: see easykv_amd/csrc/ekv_instances.def")
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c"] + defs + args + ["-o", "/tmp/_regs.o",
       "-Rpass-analysis=kernel-resource-usage"]
out = subprocess.run(cmd, cwd=_build.CSRC, capture_output=True, text=True).stderr
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = re.sub(r"\(anonymous namespace\)::", "", cur).split("(")[0]
        rows[cur] = {}
        continue
    for key in ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]"):
        m = re.search(re.escape(key) + r": (\d+)", line)
        if m and cur and key not in rows[cur]:
            rows[cur][key] = int(m.group(1))
if "error" in out and not rows:
    print(out)
for name, r in rows.items():
    if filt and not all(f in name for f in filt):
        continue
    print(f"{name}: vgpr={r.get('VGPRs')} agpr={r.get('AGPRs')} occ={r.get('Occupancy [waves/SIMD]')} vspill={r.get('VGPRs Spill')} sspill={r.get('SGPRs Spill')} scratch={r.get('ScratchSize [bytes/lane]')}")
