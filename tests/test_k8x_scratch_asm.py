"""K8x's scratch use, read from the compiled assembly: a ceiling per 8-bin instance so that the spills taken out of the
layer loop (undefined spline state carried across layers, the table index held from the kernel's entry, 64-bit LDS
pointers, vector loads of the uniform scales) cannot creep back unnoticed.  The figures are bytes per lane as hipcc
reports them for this source (`.amdhsa_private_segment_fixed_size`); they were 204 .. 216 before.  Lower is welcome:
lower the ceiling with it.
"""
import re

import pytest

from test_host_logic import kernel_assembly

# rqs_resnet_f16x3_kernel<INVERSE, INIT_KS, DBG = false, KB = 8>
CEILING = {(0, 2): 68, (0, 4): 68, (1, 2): 80, (1, 4): 80}


def _scratch_per_kernel(asm):
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        size = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        out[m.group(1)] = int(size.group(1))
    return out


@pytest.mark.asm
def test_k8x_eight_bin_scratch_ceiling():
    (asm,) = kernel_assembly(["rqs_resnet_f16x3.hip"])
    sizes = _scratch_per_kernel(asm)
    for (inverse, init_ks), ceiling in CEILING.items():
        name = "_ZN3nfa3k8x23rqs_resnet_f16x3_kernelILb%dELi%dELb0ELi8EEEvNS0_4ArgsE" % (inverse, init_ks)
        assert name in sizes, sorted(sizes)
        assert sizes[name] <= ceiling, (name, sizes[name], ceiling)
