"""apz_set_trunk_uniform is declared in the C header with two parameters and listed in the symbol table;
PolicyValueNet takes uniform_trunk (default False) and TrainPipeline reads the conf key of that name.  (No GPU: nothing is
launched.)"""
import inspect
import os
import re

from alphapig_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_symbol_table_agree():
    text = open(os.path.join(REPO, "include", "alphapig_hip.h")).read()
    m = re.search(r"int\s+apz_set_trunk_uniform\s*\(([^)]*)\)", text)
    assert m, "apz_set_trunk_uniform is not declared in include/alphapig_hip.h"
    assert len(m.group(1).split(",")) == 2
    assert "apz_set_trunk_uniform" in _native.HIP_SYMBOLS
    assert hasattr(_native.hip(), "apz_set_trunk_uniform")


def test_policy_value_net_takes_uniform_trunk():
    from alphapig_amd.policy_value_net import PolicyValueNet
    p = inspect.signature(PolicyValueNet.__init__).parameters
    assert "uniform_trunk" in p and p["uniform_trunk"].default is False


def test_train_pipeline_reads_the_conf_key():
    from alphapig_amd import pipeline
    src = inspect.getsource(pipeline.TrainPipeline.__init__)
    assert re.search(r"conf\.get\(\s*[\"']uniform_trunk[\"']\s*,\s*False\s*\)", src)
    assert len(re.findall(r"uniform_trunk=self\.uniform_trunk", inspect.getsource(pipeline.TrainPipeline))) == 2
