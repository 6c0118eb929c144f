"""apz_wgrad_wino_f16x2 is declared in the C header, listed in the symbol table and bound with its nine arguments;
hipconv.conv3x3_wgrad_f16x2 exists.  (No GPU: nothing is launched.)"""
import os
import re

from alphapig_amd import _native, hipconv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_symbol_table_agree():
    text = open(os.path.join(REPO, "include", "alphapig_hip.h")).read()
    m = re.search(r"int\s+apz_wgrad_wino_f16x2\s*\(([^)]*)\)", text)
    assert m, "apz_wgrad_wino_f16x2 is not declared in include/alphapig_hip.h"
    assert len(m.group(1).split(",")) == 9
    assert "apz_wgrad_wino_f16x2" in _native.HIP_SYMBOLS


def test_python_entry_exists():
    assert callable(getattr(hipconv, "conv3x3_wgrad_f16x2", None))
