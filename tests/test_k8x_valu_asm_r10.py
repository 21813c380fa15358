"""K8x's transcendental and piece-split instructions after round 10, read from the compiled assembly: static counts per
8-bin instance, narrow and wide, held as ceilings (tests/test_k8x_valu_asm.py holds the older, higher ones and stays).
Round 10 made the activations' last piece as bf8 directly -- per pair of values one v_cvt_scalef32_pk_bf8_f32 where two
v_fma_mixlo/hi_f16 made an f16 piece and half a v_perm_b32 picked its high byte out -- and took the reciprocal out of the
softplus correction (two v_rcp_f32 per evaluation, three evaluation sites per instance); the skip connection of a
residual block is written in place on the tiles the block loop carries (rqs_resnet_f16x3_kernel.hpp: skip_half), which
took out the 32 v_mov_b64 that copied the second Linear's accumulators back to them.

The parent's counts, same flags (forward / inverse; INIT_KS 2 and 4 where they differ; narrow and wide alike):
    v_exp_f32 46 / 46      v_log_f32 9 / 12      v_rcp_f32 18 / 24      v_add_f32 + v_fma_f32 + v_fmac_f32 317 / 365
    v_fma_mixlo_f16 = v_fma_mixhi_f16 312 (INIT_KS 2), 336 (4)      v_perm_b32 104, 112      v_mov_b64 42
    v_cvt_scalef32_pk_bf8_f32 0
Not taken out: the knots from prefix sums and the shared softmax reciprocal, so v_exp_f32,
v_log_f32 and the add / fma count stand where they stood (the 64 in-place v_fma_f32 of the skip connection were 64 v_fma_f32
/ v_fmac_f32 before).
Lower is welcome: lower the ceiling with it.
"""
import re

import pytest

from test_host_logic import kernel_assembly
from test_k8x_valu_asm import _opcodes

# per direction (0 forward, 1 inverse)
SPLINE = {0: {"v_exp_f32": 46, "v_log_f32": 9, "v_rcp_f32": 12, "add_fma_f32": 317},
          1: {"v_exp_f32": 46, "v_log_f32": 12, "v_rcp_f32": 18, "add_fma_f32": 365}}
# per INIT_KS
SPLIT = {2: {"v_fma_mixlo_f16": 208, "v_fma_mixhi_f16": 208, "v_perm_b32": 52, "v_cvt_scalef32_pk_bf8_f32": 104},
         4: {"v_fma_mixlo_f16": 224, "v_fma_mixhi_f16": 224, "v_perm_b32": 56, "v_cvt_scalef32_pk_bf8_f32": 112}}
MOV_B64 = 10
NAMES = {"narrow": "_ZN3nfa3k8x23rqs_resnet_f16x3_kernelILb%dELi%dELb0ELi8EEEvNS0_4ArgsE",
         "wide": "_ZN3nfa3k8x28rqs_resnet_f16x3_kernel_wideILb%dELi%dEEEvNS0_4ArgsE"}


def _figures(ops):
    def total(pattern):
        return sum(n for op, n in ops.items() if re.fullmatch(pattern, op))
    enc = r"(_e32|_e64|_sdwa|_dpp)?"
    return {"v_exp_f32": total(r"v_exp_f32" + enc), "v_log_f32": total(r"v_log_f32" + enc), "v_rcp_f32": total(r"v_rcp_f32" + enc),
            "add_fma_f32": total(r"v_(add|fma|fmac)_f32" + enc), "v_fma_mixlo_f16": total(r"v_fma_mixlo_f16"),
            "v_fma_mixhi_f16": total(r"v_fma_mixhi_f16"), "v_perm_b32": total(r"v_perm_b32"),
            "v_cvt_scalef32_pk_bf8_f32": total(r"v_cvt_scalef32_pk_bf8_f32"), "v_mov_b64": total(r"v_mov_b64" + enc)}


@pytest.mark.asm
@pytest.mark.parametrize("form", ["narrow", "wide"])
def test_k8x_eight_bin_round10_ceilings(form):
    (asm,) = kernel_assembly(["rqs_resnet_f16x3.hip"])
    for inverse in (0, 1):
        for init_ks in (2, 4):
            name = NAMES[form] % (inverse, init_ks)
            got = _figures(_opcodes(asm, name))
            print(name, got)
            for key, limit in dict(SPLINE[inverse], v_mov_b64=MOV_B64, **SPLIT[init_ks]).items():
                assert got[key] <= limit, (name, key, got[key], limit)
            # the last piece of every pair of values comes from the conversion: as many as the f16 lo halves
            assert got["v_cvt_scalef32_pk_bf8_f32"] * 2 == got["v_fma_mixlo_f16"], (name, got)
