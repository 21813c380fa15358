"""K8x's layer loop holds no stream drain and no per-lane global load, read from the compiled assembly of the four
non-diagnostic 8-bin instances: biases and tables reach LDS as LDS-DMA pieces behind the weight stream's own counted waits
(rqs_resnet_f16x3_kernel.hpp: bias_area_piece), so
  * `global_load_dword*` is left only outside the layer loop -- the table entries at the kernel's head, the row block's input
    rows, the log-determinant read of an accumulating launch: 7 (was 61, 52 of them `global_load_dwordx4`: twenty hidden
    bias tiles per layer and wave, the final layer's bias copy, the table prefetch);
  * nothing is in scratch;
  * no `s_waitcnt vmcnt(0)` between the layer loop's header and the branch that closes it (was seven).

How the layer loop is found: hipcc comments every loop header block with its depth and its parents.  The kernel's loops
are `for (quad ...)` (Depth=1) and, inside it at Depth=2, the input read, the layer loop and the two output loops; the layer
loop is the one Depth=2 loop that CONTAINS Depth=3 loops (the blocks, the final layer's groups, the pieces), i.e. the
Depth=2 header label that the Depth=3 headers name as a parent.  Its body runs from the header label to the last branch
back to that label.  If a later compiler lays the loops out differently, look for `s_setprio` (the first statement of the
layer loop's body) and the `Parent Loop` comments around it.
"""
import re

import pytest

from test_host_logic import kernel_assembly

GLOBAL_LOAD_CEILING = 7


def _body(asm, name):
    m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\.Lfunc_end", asm, re.S)
    assert m, name
    return m.group(1).splitlines()


def _layer_loop(lines, name):
    """(first, last) line index of the layer loop: see the module's docstring"""
    parents = set()
    for i, line in enumerate(lines):
        if re.search(r"This (Inner )?Loop Header: Depth=3", line):
            # the comment block in front: `.LBBn_m: ; Parent Loop BBn_a Depth=1` / `; Parent Loop BBn_b Depth=2`
            j = i - 1
            while j >= 0 and "Parent Loop" in lines[j]:
                m = re.search(r"Parent Loop (BB\d+_\d+) Depth=2", lines[j])
                if m:
                    parents.add(m.group(1))
                j -= 1
    assert len(parents) == 1, (name, parents)
    label = ".L" + parents.pop()
    first = next(i for i, line in enumerate(lines) if line.startswith(label + ":"))
    assert "Depth=2" in lines[first + 1], (name, lines[first:first + 2])
    back = [i for i, line in enumerate(lines) if re.match(r"\s+s_cbranch_\w+\s+" + re.escape(label) + r"\s*$", line)
            or re.match(r"\s+s_branch\s+" + re.escape(label) + r"\s*$", line)]
    assert back and back[-1] > first, (name, label, back)
    return first, back[-1]


@pytest.mark.asm
def test_k8x_layer_loop_has_no_drain_and_no_global_load():
    (asm,) = kernel_assembly(["rqs_resnet_f16x3.hip"])
    for inverse in (0, 1):
        for init_ks in (2, 4):
            name = "_ZN3nfa3k8x23rqs_resnet_f16x3_kernelILb%dELi%dELb0ELi8EEEvNS0_4ArgsE" % (inverse, init_ks)
            lines = _body(asm, name)
            loads = [i for i, line in enumerate(lines) if re.match(r"\s+global_load_dword", line)]
            assert len(loads) <= GLOBAL_LOAD_CEILING, (name, len(loads))
            m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
            assert m, name
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1)) == 0, name
            first, last = _layer_loop(lines, name)
            inside = lines[first:last + 1]
            assert sum("s_setprio" in line for line in inside) == 2, name   # (it IS the layer loop)
            assert sum("s_barrier" in line for line in inside) >= 20, name
            drains = [line.strip() for line in inside if re.search(r"s_waitcnt\b.*vmcnt\(0\)", line)]
            assert not drains, (name, drains)
            assert not [i for i in loads if first <= i <= last], name
            # the pieces are there: LDS-DMA loads beside the weight stream's twelve-per-stage dwordx4 requests
            assert sum(bool(re.match(r"\s+buffer_load_dword\s.*\blds\b", line)) for line in inside) >= 2, name
