#!/usr/bin/env python3
"""Register / LDS / scratch table of the kernels in an ISA listing made by `make asm`: tools/kernel_resources.py [--full] [csrc/wavefront.s ...]
--full: the whole mangled name, and the code length in bytes and the occupancy (waves per SIMD) the listing states for the kernel."""
import re, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
full = "--full" in sys.argv[1:]
files = [a for a in sys.argv[1:] if a != "--full"] or [os.path.join(ROOT, "distributed-path-tracer_amd", "csrc", f) for f in ("wavefront.s", "kernels.s")]
for f in files:
    txt = open(f).read()
    # the listing's own figures follow each kernel's descriptor: "; codeLenInByte = n" ... "; Occupancy: n"
    extra = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n.*?; codeLenInByte = (\d+)\n.*?; Occupancy: (\d+)\n", txt, re.S)}
    for blk in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        name = g("name")
        short = re.sub(r"^_ZN3ptx\d+", "", name)[:60]
        line = f"vgpr {g('vgpr_count'):>4s} sgpr {g('sgpr_count'):>4s} spill v{g('vgpr_spill_count')}/s{g('sgpr_spill_count')} lds {g('group_segment_fixed_size'):>6s} scratch {g('private_segment_fixed_size'):>5s}"
        if full:
            agpr = blk.split()[0]
            print(f"{name} agpr {agpr:>4s} {line} code {extra[name][0]:>7s} occupancy {extra[name][1]}")
        else:
            print(f"{short:62s} {line}")
