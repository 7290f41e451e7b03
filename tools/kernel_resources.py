#!/usr/bin/env python3
"""Register / LDS budget of every kernel of a csrc file, from hipcc's own remarks (no GPU needed):

    python tools/kernel_resources.py conv_igemm [gemm1x1_ring conv_streamk conv_wgrad winograd_deconv43 winograd_s2_43 stem_pool_w1d ...]
(names of csrc/*.hip files; the persistent 1x1 kernels are part of conv_igemm) prints scalar registers, arch VGPRs, accumulator VGPRs, spills, scratch bytes per lane, waves per SIMD, static
LDS bytes per block (the Winograd kernels' LDS is dynamic: see their launchers) and the number of instructions in the kernel's gfx950 assembly.  A kernel whose waves leave part of the
SIMD's 512 registers free lets a small element-wise wave of another stream share the CU (profiles/r05_notes.md)."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vatl4pose-wacv2024_amd", "csrc")
OCC, LDS, SCR = r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]", r"ScratchSize \[bytes/lane\]"
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
for name in sys.argv[1:]:
    src = os.path.join(CSRC, name + ".hip")
    r = subprocess.run(HIPCC + ["-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    asm = subprocess.run(HIPCC + ["-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True).stdout
    print("==", name)
    for blk in r.stderr.split("Function Name: ")[1:]:
        mangled = blk.split("\n")[0].split()[0]            # the remark's own "[-Rpass-analysis=...]" tag follows the name
        def g(k):
            m = re.search(k + r": (\d+)", blk)
            return m.group(1) if m else "?"
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(mangled), asm, re.S | re.M)       # instructions: indented lines that are neither directives nor comments
        insts = len(re.findall(r"^\t[a-z]\w*\b", body.group(1), re.M)) if body else "?"
        dn = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()[:120]
        print("S%4s V%4s A%4s spill%4s scratch%5s occ%2s LDS%7s inst%6s  %s" % (g("SGPRs"), g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g(SCR), g(OCC), g(LDS), insts, dn))
