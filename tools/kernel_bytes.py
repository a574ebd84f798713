#!/usr/bin/env python3
"""usage: tools/kernel_bytes.py device.elf  -> per k_viterbi<0..7>: SHA-256 of its code and of its kernel descriptor, and its resource row.
The ELF is csrc/k_viterbi.hip built with the Makefile's flags plus --cuda-device-only --no-gpu-bundle-output -c."""
import hashlib
import re
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
elf = sys.argv[1]
data = open(elf, "rb").read()
run = lambda *a: subprocess.run([READELF, *a, elf], capture_output=True, text=True, check=True).stdout
secs = {}                                                    # index -> (address, file offset)
for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+[0-9a-f]+", run("-S", "-W"), re.M):
    secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
syms = {}                                                    # name -> (value, size, section)
for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+\S+\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", run("-s", "-W"), re.M):
    syms[m.group(4)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(3)))
notes = run("--notes")
for mode in range(8):
    name = "_ZN3dsr9k_viterbiILi%dEEEvNS_7VitArgsE" % mode
    digests = []
    for s, want in ((name, None), (name + ".kd", 64)):
        value, size, sec = syms[s]
        assert want is None or size == want, (s, size)
        off = secs[sec][1] + value - secs[sec][0]
        digests.append(hashlib.sha256(data[off:off + size]).hexdigest())
    block = [b for b in notes.split("  - .agpr_count") if re.search(r"\.name:\s+%s\n" % name, b)][0]      # this kernel's entry of amdhsa.kernels
    row = " ".join("%s=%s" % (k, re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                   for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    print("k_viterbi<%d> code %s kd %s %s" % (mode, digests[0], digests[1], row))
