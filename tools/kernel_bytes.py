#!/usr/bin/env python3
"""usage: tools/kernel_bytes.py device.elf [substring]  -> per kernel of the ELF (every function symbol that has a .kd companion, in name order;
with a substring: those whose demangled name contains it): SHA-256 of its code and of its kernel descriptor, and its resource row.
The ELF is a unit of csrc/ built with the Makefile's flags plus --cuda-device-only --no-gpu-bundle-output -c."""
import hashlib
import re
import shutil
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
CXXFILT = next((p for p in map(shutil.which, ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt")) if p), None)      # none: mangled names
elf = sys.argv[1]
only = sys.argv[2] if len(sys.argv) > 2 else ""
data = open(elf, "rb").read()
run = lambda *a: subprocess.run([READELF, *a, elf], capture_output=True, text=True, check=True).stdout
secs = {}                                                    # index -> (address, file offset)
for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+[0-9a-f]+", run("-S", "-W"), re.M):
    secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
syms = {}                                                    # name -> (value, size, section, type)
for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(\S+)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", run("-s", "-W"), re.M):
    syms[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(3))
notes = run("--notes")
kernels = [n for n in syms if syms[n][3] == "FUNC" and n + ".kd" in syms]
shown = subprocess.run([CXXFILT, *kernels], capture_output=True, text=True, check=True).stdout.split("\n") if CXXFILT else kernels
# k_viterbi<0>, not void dsr::k_viterbi<0>(dsr::VitArgs); k_mcc_cost<1>, not void (anonymous namespace)::k_mcc_cost<1>(...)
shown = {n: re.sub(r"^void |\bdsr::|\(anonymous namespace\)::", "", d).split("(")[0] for n, d in zip(kernels, shown)}
for name in sorted(kernels, key=lambda n: shown[n]):
    if only not in shown[name]:
        continue
    digests = []
    for s, want in ((name, None), (name + ".kd", 64)):
        value, size, sec = syms[s][:3]
        assert want is None or size == want, (s, size)
        off = secs[sec][1] + value - secs[sec][0]
        digests.append(hashlib.sha256(data[off:off + size]).hexdigest())
    block = [b for b in notes.split("  - .agpr_count") if re.search(r"\.name:\s+%s\n" % re.escape(name), b)][0]      # this kernel's entry of amdhsa.kernels
    row = " ".join("%s=%s" % (k, re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                   for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    print("%s code %s kd %s %s" % (shown[name], digests[0], digests[1], row))
