"""The nets of the generic convolution route (csrc/conv3x3_mfma.h: every 15x15 net that is not the 128-filter residual net)
and that route's launch rule restated -- TEST HELPER ONLY (tests/test_generic_bounds.py on the CPU, tests/test_gpu_generic_nets.py,
tests/test_gpu_generic_train.py and the operator cases of tests/test_gpu_train.py on the GPU).

  GEN                        the three nets: (kind, side, residual blocks, filters)
  params / positions         weights.init_params(style="bench") and test_gpu_net.random_positions with fixed seeds
  layer_channels(...)        (C_in, C_out, residual) of every 3x3 layer in apz_layer_io order
  conv_lds_bytes(...)        ConvGeo<H, W>::lds_bytes of the channel chunk launch_conv_r chooses
  evaluator_form(...)        launch_conv_t + launch_conv_r: which template form and grid a layer of n boards takes
  operator_form(...)         apz_conv3x3_fwd's `groups` rule + launch_conv_r, for hipconv.conv3x3_fwd / conv3x3_dgrad

The rule is restated from csrc/apz_engine.hip, not read from the library: a test asserts the form its case depends on, so on a
device whose CU count gives another form the case fails instead of silently testing something else."""
import collections
import json
import os

import numpy as np

from alphapig_amd import weights
from oracle import net_ref

GEN = (("simple", 15, 0, 128), ("resnet", 15, 1, 64), ("resnet", 15, 1, 256))
GEN_IDS = ("simple15", "resnet15x64", "resnet15x256")
PARAM_SEED = {"simple15": 61, "resnet15x64": 62, "resnet15x256": 63}
LDS_BUDGET = 160 * 1024


def gen_id(kind, side, blocks, nf):
    return GEN_IDS[GEN.index((kind, side, blocks, nf))]


def params(kind, side, blocks, nf, seed=None):
    seed = PARAM_SEED[gen_id(kind, side, blocks, nf)] if seed is None else seed
    return weights.init_params(kind, side, side, 9, blocks, nf, seed=seed, style="bench")


_positions = {}


def positions(n, side=15, seed=2500):
    """-> (codes uint8 [n, stride], planes float32 [n, 9, side, side]); cached, read-only."""
    key = (n, side, seed)
    if key not in _positions:
        from test_gpu_net import random_positions
        codes, planes = random_positions(n, side, seed=seed)
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        codes.setflags(write=False)
        planes.setflags(write=False)
        _positions[key] = (codes, planes)
    return _positions[key]


def layer_channels(kind, blocks, nf, c_in=9):
    if kind == "resnet":
        return [(c_in, nf, False)] + [(nf, nf, False), (nf, nf, True)] * blocks
    out, prev = [], c_in
    for _, co in net_ref.SIMPLE_LAYERS:
        out.append((prev, co, False))
        prev = co
    return out


# ---- csrc/conv3x3_mfma.h ConvGeo and csrc/apz_engine.hip launch_conv_r / launch_conv_t / apz_conv3x3_fwd, restated --------
def _plane_stride(side):
    plane = (side + 2) * (side + 1)
    return ((plane + 15) // 32) * 32 + 16


def conv_chunk(cin, side):
    """Channels resident in LDS at once: C_in padded to 4, halved (to a multiple of 4) until the tile fits 160 KiB."""
    ps = _plane_stride(side)
    max_chunk = ((LDS_BUDGET // 4 - 64) // ps) & ~3
    chunk = (cin + 3) // 4 * 4
    while chunk > max_chunk:
        chunk = ((chunk // 2) + 3) & ~3
    return chunk


def conv_lds_bytes(cin, side):
    return (conv_chunk(cin, side) * _plane_stride(side) + 64) * 4


Form = collections.namedtuple("Form", "ct groups split per_cu grid chunks second_board")


def _grid(n, cin, side, num_cu):
    per_cu = max(1, min(4, LDS_BUDGET // conv_lds_bytes(cin, side)))
    return per_cu, min(n, num_cu * per_cu)


def evaluator_form(n, cin, cout, side, num_cu):
    """launch_conv_t: CT = cout / 64 tiles per workgroup, or CT workgroups of one tile per board while n * CT <= 2 * num_cu."""
    tiles = cout // 64
    split = tiles > 1 and n * tiles <= 2 * num_cu
    per_cu, grid = _grid(n, cin, side, num_cu)
    chunks = -(-((cin + 3) // 4 * 4) // conv_chunk(cin, side))
    return Form(1 if split else tiles, tiles if split else 1, split, per_cu, grid, chunks, grid < n)


def operator_form(n, cin, cout, side, num_cu):
    """apz_conv3x3_fwd: `groups` doubles while it leaves tiles to split and boards x groups stays below the CU count."""
    groups = 1
    while groups * 64 < cout and n * groups * 2 <= num_cu * 2 and n * groups < num_cu:
        groups *= 2
    per_cu, grid = _grid(n, cin, side, num_cu)
    chunks = -(-((cin + 3) // 4 * 4) // conv_chunk(cin, side))
    return Form(cout // 64 // groups, groups, groups > 1, per_cu, grid, chunks, grid < n)


def form_name(f):
    return "CT=%d x %d groups, per_cu %d, grid %d%s%s" % (f.ct, f.groups, f.per_cu, f.grid, ", %d chunks" % f.chunks if f.chunks > 1
                                                        else "", ", second board" if f.second_board else "")


# ---- the measured table (profiles/r25_generic_route.md is written from it) ---------------------------------------------------
class Table(object):
    """Rows the tests measured, saved as <APZ_TABLE_DIR>/<name>.json after every row; without the variable nothing is written."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def add(self, **row):
        self.rows.append(row)
        out = os.environ.get("APZ_TABLE_DIR")
        if out:
            out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), out)   # (an absolute one stays)
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, self.name + ".json"), "w") as f:
                json.dump(self.rows, f, indent=1)
