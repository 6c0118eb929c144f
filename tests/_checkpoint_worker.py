"""Worker for tests/test_pipeline_checkpoint.py: the lock-step TrainPipeline on CPU ranks (gloo) with the stand-in
evaluator and trainer of tests/_pipeline_worker.py, stopped at a checkpoint or resumed from one.
argv: out_dir game_batch_num checkpoint_every [resume path]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from alphapig_amd import dist  # noqa: E402
from alphapig_amd.pipeline import TrainPipeline  # noqa: E402
from _pipeline_worker import TiltNet, TiltTrainer  # noqa: E402


class StatefulTiltTrainer(TiltTrainer):
    def state(self):
        return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

    def load_state(self, state):
        self._p = {"w": np.array(state["p/w"], np.float32), "b": np.array(state["p/b"], np.float32)}
        self.t = int(state["meta"]["t"])


def main():
    out_dir, batches, every = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    resume = sys.argv[4] if len(sys.argv) > 4 else None
    rank, world, _ = dist.init(backend="gloo")
    conf = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
            "n_playout": 8, "c_puct": 5, "buffer_size": 100000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
            "check_freq": 1000, "game_batch_num": batches, "play_batch_size": 2, "pure_mcts_playout_num": 10,
            "async_update": False, "concurrent_games": 4, "replay": "compact", "checkpoint_every": every,
            "model_dir": os.path.join(out_dir, "models%d" % rank), "checkpoint_dir": os.path.join(out_dir, "checkpoints")}
    net = TiltNet(64)
    trainer = StatefulTiltTrainer(net) if rank == 0 else None
    pipe = TrainPipeline(conf, policy_value_net=net, seed=77, trainer=trainer, resume=resume)
    assert pipe.distributed and (pipe.rank, pipe.world) == (rank, world)
    hist = pipe.run()
    res = {"rank": rank, "history": hist, "buffer": len(pipe.data_buffer), "lr_multiplier": pipe.lr_multiplier,
           "w": net.params()["w"].tolist(), "trainer_w": trainer.get_params()["w"].tolist() if trainer else None,
           "next_index": pipe.engine.next_index}
    with open(os.path.join(out_dir, "pipe%d.json" % rank), "w") as f:
        json.dump(res, f)
    dist.barrier()
    pipe.engine.close()
    dist.shutdown()


if __name__ == "__main__":
    main()
