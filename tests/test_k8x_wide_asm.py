"""The four instances of K8x's wide form (eight waves on one ring: rqs_resnet_f16x3_kernel.hpp, WAVES = 8), read from the
compiled assembly: nothing in scratch, at most 256 registers (two waves per SIMD), the narrow instances' ceilings on the
conversion VALU (tests/test_k8x_valu_asm.py) -- each wave runs the narrow form's program --, and no more per-lane global
loads or stream drains than the narrow instances have (tests/test_k8x_vmem_asm.py: none of either in the layer loop).
"""
import re

import pytest

from test_host_logic import kernel_assembly
from test_k8x_valu_asm import CEILING, CNDMASK, _figures, _opcodes
from test_k8x_vmem_asm import GLOBAL_LOAD_CEILING, _body

NARROW = "_ZN3nfa3k8x23rqs_resnet_f16x3_kernelILb%dELi%dELb0ELi8EEEvNS0_4ArgsE"
WIDE = "_ZN3nfa3k8x28rqs_resnet_f16x3_kernel_wideILb%dELi%dEEEvNS0_4ArgsE"


def _descriptor(asm, name):
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, name
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\n", m.group(1))}


def _count(lines, pattern):
    return sum(bool(re.match(pattern, line)) for line in lines)


@pytest.mark.asm
def test_k8x_wide_instances():
    (asm,) = kernel_assembly(["rqs_resnet_f16x3.hip"])
    for inverse in (0, 1):
        for init_ks in (2, 4):
            name = WIDE % (inverse, init_ks)
            d = _descriptor(asm, name)
            assert d["private_segment_fixed_size"] == 0, (name, d)
            # (gfx950: architectural and accumulation registers share one file of 512 per SIMD lane)
            assert d["next_free_vgpr"] <= 256, (name, d["next_free_vgpr"])
            m = re.search(r"\.max_flat_workgroup_size: (\d+)\s+\.name:\s+" + re.escape(name) + r"\n", asm)
            assert m and int(m.group(1)) == 512, name
            got = _figures(_opcodes(asm, name))
            assert got["pk_f32"] == 0 and got["v_maximum3_f32"] > 0, (name, got)
            for key, limit in dict(CEILING[init_ks], v_cndmask_b32=CNDMASK[(inverse, init_ks)]).items():
                if key in ("v_fma_mix_f32", "v_fma_mixlo_f16", "v_fma_mixhi_f16", "v_perm_b32", "v_cndmask_b32"):
                    assert got[key] <= limit, (name, key, got[key], limit)
            wide, narrow = _body(asm, name), _body(asm, NARROW % (inverse, init_ks))
            loads = _count(wide, r"\s+global_load_dword")
            assert loads <= min(GLOBAL_LOAD_CEILING, _count(narrow, r"\s+global_load_dword")), (name, loads)
            drain = r"\s+s_waitcnt\b.*vmcnt\(0\)"
            assert _count(wide, drain) <= _count(narrow, drain), (name, _count(wide, drain), _count(narrow, drain))
            # one barrier per PAIR of stages, the requests of a pair where a stage's were
            assert 2 * _count(wide, r"\s+s_barrier") <= _count(narrow, r"\s+s_barrier") + 4, name
