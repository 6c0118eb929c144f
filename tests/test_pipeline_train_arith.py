"""TrainPipeline's train_arith key (HipTrainer's trunk_arith): an unknown value is rejected when the pipeline is built,
before anything touches a GPU."""
import pytest

from alphapig_amd.pipeline import TrainPipeline


@pytest.mark.parametrize("value", ["bf16", "F16X2", "", None])
def test_unknown_train_arith_is_rejected(value):
    with pytest.raises(ValueError, match="train_arith"):
        TrainPipeline({"train_arith": value}, policy_value_net=object(), trainer=object())
