"""The launch switch of K8x's form (NFA_FLAG_K8X_FORM, bits 16-17 of `flags`: 0 the launcher's choice, 1 narrow, 2 wide),
CPU only: K8x's two entry points take the three codes and reject the fourth, every other whole-layer entry point rejects
the bits as unknown flags, and the binding's tri-state holds the header's codes.  (Argument errors come first: batch 0
answers without reaching the device.)"""
import os
import re

from nflows_amd import _native as N
from nflows_amd import ops
from test_whole_layer_abi import ENTRIES, base


def form(code):
    return code << N.FLAG_K8X_FORM_SHIFT


def test_form_codes_of_the_entry_points():
    lib = N.load()
    for name, (engine, call) in ENTRIES.items():
        for code in (1, 2, 3):
            rc = call(lib, base(batch=0, flags=form(code)))
            if engine == "k8x" and code < 3:
                assert rc == N.OK, (name, code, rc)
            else:
                assert rc == N.ERR_INVALID_ARGUMENT, (name, code, rc)


def test_binding_matches_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nflows_amd.h")).read()
    consts = dict(re.findall(r"#define (NFA_\w+) (\w+)", header))
    assert int(consts["NFA_FLAG_K8X_FORM_SHIFT"]) == N.FLAG_K8X_FORM_SHIFT
    assert int(consts["NFA_FLAG_K8X_FORM_MASK"], 16) == 3 << N.FLAG_K8X_FORM_SHIFT
    assert ops.K8X_FORMS == {"auto": int(consts["NFA_K8X_FORM_AUTO"]), "narrow": int(consts["NFA_K8X_FORM_NARROW"]),
                             "wide": int(consts["NFA_K8X_FORM_WIDE"])}
    assert ops.K8X_FORM in ops.K8X_FORMS.values()
