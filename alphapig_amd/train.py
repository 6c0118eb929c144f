"""Training step on the HIP kernels: the consumer of the self-play path's tuples.

Everything the reference defines around the optimiser step (policy_value_net_mxnet.py:173-212, :282-299 and
train_mxnet.py:194-240) restated as an explicit forward pass, an explicit backward pass over the saved activations
and one Adam launch -- each operator a hand-written HIP kernel behind include/alphapig_hip.h (alphapig_amd/hipconv.py
holds the one-line wrappers).  No autograd and no PyTorch arithmetic: torch tensors are device buffers here, as in
the self-play path.  The module needs the HIP library and a GPU; without them construction raises.

  graph     training-mode BatchNorm (batch statistics, eps 1e-3, momentum 0.9, gamma frozen at 1 where the
            reference leaves fix_gamma at MXNet's default), Dropout(0.5) on both flattened head inputs (the training
            graph shares create_backbone_resnet), softmax / tanh heads
  loss      mean((z - v)^2) + mean(-sum(pi * log p, axis=1)); entropy monitor mean(sum(-p log p))
  update    MXNet Adam as Module.init_optimizer configures it: g = grad / batch_size + wd * w (rescale_grad =
            1/batch_size on top of the mean loss; wd = 1e-4 on *_weight and *_gamma only), m/v moments,
            lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), eps 1e-8
  policy_update   epochs x train_step with the KL-adaptive learning-rate multiplier and the 4 * kl_targ early stop
  guard     opt-in (step_guard / clip_norm; csrc/grad_guard.h): the global gradient norm taken on the device in front of
            Adam, global-norm clipping inside Adam's rescale factor, and a step whose gradients or losses are not finite
            skipped on the device -- weights, moments, moving statistics and t as if it had not been asked for
  legal     opt-in (legal_policy): softmax, cross-entropy and entropy over the empty cells of every position
  average   opt-in (ema_decay; csrc/ema.h): an exponential moving average of every parameter and statistic in a shadow copy
            on the device, moved by one launch behind every Adam launch under that launch's skip rule -- what self-play, the
            arena and the saved models of TrainPipeline read while the raw weights go on being trained

The 10-block / 128-filter / 15x15 network keeps its trunk activations in the self-play kernels' padded-row layout
[n][128][15][16] from the stem's BatchNorm to the heads (forward and data gradient on the fused Winograd kernel of
the self-play path, weight gradient through the Winograd domain); other shapes (the 8x8 simple net, other filter
counts) run dense on the direct MFMA kernel.

PARITY UNPINNED like the forward's numbers (MXNet absent, no recorded training runs).  Checked on the GPU against
tests/torch_trainer.py (the same graph in PyTorch float64 / float32 autograd), which tests/test_train.py in turn
checks against oracle/train_ref.py (NumPy float64 loss + finite differences, NumPy Adam).
"""
import collections

import numpy as np

BN_EPS = 1e-3
BN_MOMENTUM = 0.9
SIMPLE_CONVS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv_final")
DeviceBatch = collections.namedtuple("DeviceBatch", "states pis zs")     # HipTrainer.upload()
# what the forward pass leaves on the tape for the backward pass: one conv_act layer (x -> Convolution y -> BatchNorm,
# relu a), and one residual block (x -> convA ya -> bnA, relu ha -> convB yb -> bnB + x, relu out; m / i: the batch mean
# and 1 / std of each BatchNorm, k: its ReLU decisions as a bit mask, padded rows only; layout: the convolution's, blay /
# side: its BatchNorm's -- side only where that runs behind to_rows16 with the board mask, the stem of a framed board)
ConvAct = collections.namedtuple("ConvAct", "name x y a mean invstd layout blay side")
Block = collections.namedtuple("Block", "x ya ha ma ia yb out mb ib ka kb")


def check_ema_decay(ema_decay):
    """-> None or a float; ValueError unless ema_decay is None or a finite number with 0 < d < 1.  Needs no GPU."""
    if ema_decay is None:
        return None
    try:
        d = float(ema_decay)
    except (TypeError, ValueError):
        d = float("nan")
    if not (np.isfinite(d) and 0.0 < d < 1.0):
        raise ValueError("ema_decay must be None or a finite number with 0 < ema_decay < 1, not %r" % (ema_decay,))
    return d


def ema_coefficient(decay, n, warmup):
    """The coefficient c of the averaged weights' step s = s + c * (w - s) (csrc/ema.h) after n steps have been applied ->
    np.float32.  warmup: the decay rises as (1 + n) / (10 + n) until it reaches `decay` (0.1, 0.18, 0.25, ...: the first
    steps move the average most of the way, so it does not sit on the initial weights for 1 / (1 - decay) steps).  Computed
    in Python floats and rounded once."""
    decay_t = min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)
    return np.float32(1.0 - decay_t)


TRAINABLE_SIDES = (15, 8)
FRAMED_SIDES = (6, 7, 9, 11, 12, 13, 14)      # Frame15::framed_side (csrc/frame15.h)


def check_trainable_board(params, framed=False, net_kind="resnet", trunk_arith="f32"):
    """ValueError unless the policy head of `params` (fc_3_1_1_bias: one output per cell) belongs to a board the training
    step runs on.  15x15 and 8x8 have training kernels of their own and pass whatever `framed` says.  The other square
    boards from 6x6 to 14x14 except 10x10 -- the evaluator's "framed" boards, the S x S window of the 15x15 trunk kernels'
    frame (csrc/frame15.h) -- pass with framed=True only: the step then runs the 15x15 trunk kernels with the board mask
    in its BatchNorm passes (csrc/bn_frame.h; DESIGN.md, "Boards smaller than 15x15"), for the residual net of 128
    filters (net_kind, and the shape of res_conv1_weight / convA1_weight when `params` holds them) in trunk_arith "f32":
    the f16x2 trunk's statistics epilogue and device-chosen scales see off-board cells.  Without the switch the plain
    padded-row kernels would take their BatchNorm statistics over all 225 cells of the frame, so the call is refused.
    Needs no GPU."""
    hw = int(np.asarray(params["fc_3_1_1_bias"]).shape[0])
    side = int(round(hw ** 0.5))
    if side * side != hw or side in TRAINABLE_SIDES:
        return
    if not framed:
        raise ValueError("HipTrainer supports 15x15 and 8x8 boards, not %dx%d: the evaluator runs the other 6x6 .. 14x14 boards (not 10x10) framed "
                         "on the 15x15 kernels, the training step on them does not exist without framed=True (SxS: 6, 7, 9, "
                         "11 .. 14, residual net of 128 filters)" % (side, side))
    if side not in FRAMED_SIDES:
        raise ValueError("framed training runs boards of side %s (and 15x15 and 8x8 on their own kernels), not %dx%d" %
                         (", ".join(str(s) for s in FRAMED_SIDES), side, side))
    if net_kind != "resnet":
        raise ValueError("framed training runs the residual net only, not net_kind %r on a %dx%d board" % (net_kind, side, side))
    for k in ("res_conv1_weight", "convA1_weight"):
        if k in params and int(np.shape(params[k])[0]) != 128:
            raise ValueError("framed training runs the residual net of 128 filters, not %d (%dx%d board)" %
                             (int(np.shape(params[k])[0]), side, side))
    if trunk_arith != "f32":
        raise ValueError("framed training has no trunk_arith=%r form: the f16x2 trunk's statistics epilogue and its "
                         "device-chosen scales see off-board cells (%dx%d board)" % (trunk_arith, side, side))


def f16x2_route(params, net_kind="resnet", n_blocks=10):
    """Which form trunk_arith="f16x2" takes on the net of `params` -> "rows16" (the 15x15 residual trunk of 128 filters: the
    padded-row Winograd kernels, trunk15_wino3h16.h) or "dense" (every other 15x15 net: conv15h_kernel, conv15_split.h, for
    its 3x3 layers whose channel counts are multiples of 64).  ValueError for everything else: 8x8 and framed boards, and a
    15x15 net without such a layer (check_trainable_board has refused the framed boards with its own words by then).  Needs
    no GPU."""
    hw = int(np.shape(params["fc_3_1_1_bias"])[0])
    side = int(round(hw ** 0.5))
    if side * side != hw or side != 15:
        raise ValueError("trunk_arith='f16x2' needs the 15x15 residual trunk of 128 filters (net_kind %r, %dx%d)" %
                         (net_kind, side, side))
    if net_kind == "resnet" and n_blocks > 0 and tuple(np.shape(params["convA1_weight"])) == (128, 128, 3, 3):
        return "rows16"
    if not f16x2_dense_layers(params, net_kind, n_blocks):
        raise ValueError("trunk_arith='f16x2' needs a 3x3 layer whose C_in and C_out are multiples of 64 (net_kind %r, %d blocks)" %
                         (net_kind, n_blocks))
    return "dense"


def f16x2_dense_layers(params, net_kind, n_blocks):
    """The parameter prefixes of the 3x3 layers that the dense f16x2 route runs on conv15h_kernel: C_in and C_out multiples
    of 64 (the kernel's contraction splits over four waves of 16-channel chunks, in both orientations).  The first layer
    (C_in = 9) never is one."""
    if net_kind == "resnet":
        names = ["conv%s%d" % (ab, i) for i in range(1, n_blocks + 1) for ab in "AB"]
    else:
        names = list(SIMPLE_CONVS)
    out = []
    for k in names:
        shape = tuple(np.shape(params[k + "_weight"]))
        if len(shape) == 4 and shape[2:] == (3, 3) and shape[0] % 64 == 0 and shape[1] % 64 == 0:
            out.append(k)
    return out


class HipTrainer(object):
    def __init__(self, params, net_kind="resnet", n_blocks=10, batch_size=512, wd=1e-4, device_index=0, dropout=0.5,
                 seed=0, height=None, width=None, dropout_step0=0, trunk_arith="f32", framed=False, step_guard=False,
                 clip_norm=None, ema_decay=None, ema_warmup=True, legal_policy=False):
        """params: name -> array, in any order.  height / width: the board (default: square, from the policy head's size).
        seed / dropout_step0: the dropout masks are a stateless hash of (seed, dropout_step0 + step, element) -- a trainer
        that is re-created (set_params, a resumed checkpoint) or one of several ranks passes its own seed / the steps
        already taken, or it replays the mask sequence of a fresh trainer.
        trunk_arith: "f32" (default) runs the padded-row trunk's forward and data gradient on the exact fp32 Winograd
        kernel; "f16x2" on the two-term fp16 kernel of the self-play path (trunk15_wino3h16.h: the forward with the
        BatchNorm statistics in its epilogue, the data gradient with a power-of-two input scale chosen on the device),
        at every batch size -- the weight gradient, the stem and the heads stay as they are.  A step in which an f16x2
        launch leaves the fp16 range is taken again on the exact kernels (trunk_overflows counts them) and ends
        bit-identical to the "f32" trainer's step.  (profiles/r07_train_f16x2.md: 0.86 of the "f32" step time at batch
        512, but only 0.98 at the reference's batch of 128, where the kernel has 128 work items for 256 CUs.)
        Every other 15x15 net (rows16 False: the simple net, the residual nets of other filter counts) takes "f16x2" on
        dense tensors (f16x2_route -> "dense"): every 3x3 layer whose C_in and C_out are multiples of 64 runs its forward and
        its data gradient on conv15h_kernel (csrc/conv15_split.h; the data gradient with the same device-chosen input
        scale, from the dense bn_bwd's dxmax), weights packed by one launch per step; the first layer (C_in = 9), the
        weight gradient, BatchNorm, heads, loss and Adam stay on their exact kernels; overflow is handled the same way
        (profiles/r32_generic_train_f16x2.md).  8x8 and framed boards have no f16x2 form: ValueError.
        framed: opt in to the training step on the framed boards (6x6, 7x7, 9x9, 11x11 .. 14x14; check_trainable_board):
        the residual net of 128 filters on the 15x15 trunk kernels, the board mask in the BatchNorm passes.  Without it
        those boards raise ValueError as they always did; 15x15 and 8x8 train as they always did whatever it says.
        step_guard: opt in to the guarded optimiser step (csrc/grad_guard.h): two reduction launches in front of Adam take
        the global norm of the step's gradients (last_grad_norm: of grad / batch_size, what Adam sees before weight decay)
        and look for non-finite values in the gradients and the three losses; a step that has one is SKIPPED on the device
        -- weights, moments, moving statistics, t and with it the next dropout masks are as if it had not been asked for
        (skipped_steps, last_skip_reason) -- and train_step still returns that step's (non-finite) loss.  The verdict
        travels in the step's one read-back: no second synchronisation.  A step that is not skipped has the unguarded
        step's bits.  On "f16x2" the overflow word is one more reason to skip: the step is repeated on the exact kernels as
        always, and the repeat is guarded in turn.
        clip_norm: None, or a finite positive number -- global-norm clipping (implies step_guard): a step whose gradient
        norm exceeds it has its gradient scaled to that norm (clipped_steps), inside Adam's rescale factor.
        ema_decay: None (default: nothing is allocated and nothing launched), or a finite number in (0, 1) -- the averaged
        weights (csrc/ema.h): ema_p, a shadow of every tensor of p (statistics and pinned gammas included), starts as a copy
        of p and follows it by ema_p += c * (p - ema_p), c = ema_coefficient(ema_decay, ema_updates, ema_warmup), in one
        launch queued directly behind every Adam launch of train_step with that launch's skip condition: a step that was
        skipped (the guard's verdict) or repeated (an f16x2 overflow) moves the average exactly as often as it moved the
        weights.  ema_updates counts the steps applied, from the read-back the step makes anyway.  The raw weights, the
        moments and the losses are those of a trainer without it, bit for bit: the launch only reads them.
        ema_params() / sync_evaluator(net, ema=True) hand the average out.
        legal_policy: opt in to the legal-move policy: the loss takes its log-softmax, cross-entropy and
        entropy over the EMPTY cells of every position (hipconv.pv_loss(occ=...)), so no gradient is spent on pushing
        occupied cells down; the occupancy is made on the device once per uploaded batch, from the planes.  The internal
        evaluator of the KL monitor is created with the same switch.  Off: the reference's loss, today's launches."""
        if trunk_arith not in ("f32", "f16x2"):
            raise ValueError("trunk_arith must be 'f32' or 'f16x2', not %r" % (trunk_arith,))
        if clip_norm is not None:
            clip_norm = float(clip_norm)
            if not (np.isfinite(clip_norm) and clip_norm > 0):
                raise ValueError("clip_norm must be None or a finite positive number, not %r" % (clip_norm,))
        ema_decay = check_ema_decay(ema_decay)
        if "fc_3_1_1_bias" in params:
            # before anything touches the GPU: today's failure would come from the first step
            check_trainable_board(params, framed, net_kind, trunk_arith)
            if trunk_arith == "f16x2":
                f16x2_route(params, net_kind, n_blocks)
        import torch
        from . import _native, hipconv
        if not torch.cuda.is_available():
            raise RuntimeError("HipTrainer needs a GPU: the training step has no CPU path")
        _native.hip()                          # raises when libalphapig_hip.so is missing
        self.torch, self.ops = torch, hipconv
        self.kind, self.n_blocks = net_kind, n_blocks
        self.batch_size, self.wd, self.dropout, self.seed = batch_size, wd, dropout, seed
        self.device = torch.device("cuda", device_index)
        self.p = collections.OrderedDict()
        for k, v in params.items():
            self.p[k] = torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device=self.device)
        stem = "res_conv1_weight" if net_kind == "resnet" else "conv1_weight"
        if stem not in self.p:
            raise ValueError("parameter %s missing (net_kind %r)" % (stem, net_kind))
        self.c_in = int(self.p[stem].shape[1])
        self.hw = int(self.p["fc_3_1_1_bias"].shape[0])
        self.side = int(round(self.hw ** 0.5))
        if (height is None) != (width is None):
            raise ValueError("pass both height and width, or neither")
        if height is not None and (int(height) * int(width) != self.hw or int(height) != int(width)):
            raise ValueError("the HIP training kernels take square boards whose size matches the policy head (%d cells)" % self.hw)
        if self.side * self.side != self.hw:
            raise ValueError("policy head of %d cells is not a square board" % self.hw)
        self.dropout_step0 = int(dropout_step0)
        self.stat_names = [k for k in self.p if k.endswith(("_mean", "_var", "_moving_mean", "_moving_var"))]
        # gammas of the fix_gamma BatchNorm layers (every conv_act layer: res_conv1, the two 1x1 heads, and all of the
        # simple net; policy_value_loss.json nodes 9 / 208 / 226 carry no fix_gamma=False) never enter the graph.
        # MXNet rewrites them to 1 on every forward, so they are pinned to 1 here and kept out of the optimiser --
        # left in, weight decay + Adam move them by ~lr per step for ever and the drift lands in saved checkpoints.
        self.fixed_gamma_names = [k for k in self.p if k.endswith("_gamma") and not k.startswith(("bnA", "bnB"))]
        for k in self.fixed_gamma_names:
            self.p[k].fill_(1.0)
        self.train_names = [k for k in self.p if k not in self.stat_names and k not in self.fixed_gamma_names]
        self.m = {k: torch.zeros_like(self.p[k]) for k in self.train_names}
        self.v = {k: torch.zeros_like(self.p[k]) for k in self.train_names}
        self.t = 0
        self.grad = {}
        # the self-play kernels' padded-row layout for the trunk when the net has their shape
        # framed boards (check_trainable_board has seen the net): the board's side, the `side` of every trunk-side operator;
        # None on 15x15 and 8x8, where nothing changes
        self.framed = bool(framed)
        self.frame_side = self.side if (self.framed and self.side in FRAMED_SIDES) else None
        if self.frame_side and (n_blocks < 1 or tuple(self.p["convA1_weight"].shape) != (128, 128, 3, 3)):
            raise ValueError("framed training needs the residual trunk of 128 filters (at least one block)")
        self.rows16 = (net_kind == "resnet" and n_blocks > 0 and (self.side == 15 or self.frame_side is not None) and
                       tuple(self.p["convA1_weight"].shape) == (128, 128, 3, 3))
        # ... whose 2 n_blocks weight tensors then live back to back in one buffer (self.p holds views): one launch packs
        # all of them for the Winograd kernel in both orientations at the start of a step (hipconv.wino_pack_many)
        self._trunk_names = []
        self._trunk_w = self._upk = None
        if self.rows16:
            self._trunk_names = ["conv%s%d_weight" % (ab, i) for i in range(1, n_blocks + 1) for ab in "AB"]
            self._trunk_w = self._flat(self._trunk_names, self.p).view(-1, 128, 128, 3, 3)
        self.trunk_arith = trunk_arith
        self.trunk_overflows = 0       # f16x2: steps (and loss_and_grads calls) repeated on the exact kernels
        self._fast = False             # the pass being queued runs its trunk on the f16x2 kernel
        # f16x2 on the dense route: the eligible layers by parameter prefix -> their packed (forward, data gradient) pairs of
        # the pass being queued (hipconv.conv15h_pack_many: one launch at the start of a fast pass)
        self._gen_names, self._gen, self._gen_out = [], {}, None
        if trunk_arith == "f16x2" and not self.rows16:
            f16x2_route(self.p, net_kind, n_blocks)      # (raises for 8x8 and for a net without an eligible layer)
            self._gen_names = f16x2_dense_layers(self.p, net_kind, n_blocks)
        if trunk_arith == "f16x2" and self.rows16:
            # the trunk biases back to back as well (wino3h_pack_many packs them with the weights), the moving statistics in
            # one buffer (one copy snapshots them at the start of a step: a repeated step must not move them twice), and
            # a word after the step's three losses: the overflow word, read with the losses in ONE device -> host copy
            self._trunk_b = self._flat([k[:-len("_weight")] + "_bias" for k in self._trunk_names], self.p).view(-1, 128)
            self._u16 = None
        # the guarded step (csrc/grad_guard.h) skips on the device; what it must not move either lives in the same
        # arrangement, for every net kind and arithmetic: the statistics in one buffer with a snapshot, and the guard's
        # 16-byte record behind the overflow word (16 bytes in: aligned), all in the step's ONE device -> host copy
        self.clip_norm = clip_norm
        self.step_guard = bool(step_guard) or clip_norm is not None
        self.last_grad_norm = None     # of the last guarded train_step (grad / batch_size, before weight decay)
        self.skipped_steps = 0         # guarded steps that left everything as it was
        self.clipped_steps = 0         # guarded steps taken with the gradient scaled to clip_norm
        self.last_skip_reason = None   # of the last guarded train_step: None (taken), or the record's why bits in words
        self.last_rescale_eff = None   # of the last guarded train_step: the `rescale` Adam ran with (float32)
        self._word = None              # (a plain f32 trainer has none: its read-back is loss3)
        if trunk_arith == "f16x2" or self.step_guard:
            self._stat_buf = self._flat(self.stat_names, self.p)
            self._stat_snap = torch.empty_like(self._stat_buf)
            # [loss3][overflow word] (+ [record]): _attempt says which of them a read-back holds
            self._word = torch.zeros((8 if self.step_guard else 4,), dtype=torch.float32, device=self.device)
            self._flag = self._word[3:4]
            self._record = self._word[4:8] if self.step_guard else None
        # the averaged weights (csrc/ema.h): a shadow of every tensor of p, in p's order, as views of ONE flat buffer (a
        # broadcast sends one piece) -- allocated last, when every tensor of p has moved to where it stays
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema_updates = 0           # averaging steps applied (a skipped step is none)
        self.ema_p = None
        if ema_decay is not None:
            self.ema_p = collections.OrderedDict()
            self._ema_buf = self._flat(list(self.p), self.ema_p)
            # (the launch's table, once: from here on the tensors of p and ema_p are only ever written INTO)
            self._ema_tab = hipconv.ema_table([(self.ema_p[k], self.p[k]) for k in self.p])
        self.legal_policy = bool(legal_policy)
        self._occ = (None, None, None)  # legal_policy: the states tensor the occupancy was made of, its version, the occupancy
        self._eval = None
        self._eval_t = -1
        self.tape = None

    def _occupancy(self, states):
        """legal_policy: the occupancy [n][H*W] u8 of a batch's planes, made once per uploaded batch: policy_update hands the
        same DeviceBatch to every epoch, and a tensor that was written to since (its version moved) is read again"""
        held, version, occ = self._occ
        if held is not states or version != states._version:
            occ = self.ops.occupancy_planes(states)
            self._occ = (states, states._version, occ)
        return occ

    def _flat(self, names, into):
        """The tensors of p named `names`, copied back to back into ONE new contiguous buffer -> the buffer, flat;
        into[name] = the tensor's view of it (into = self.p: the tensor lives there from now on)"""
        torch, src = self.torch, [self.p[k] for k in names]
        buf = torch.empty((sum(t.numel() for t in src),), dtype=torch.float32, device=self.device)
        off = 0
        for k, t in zip(names, src):
            into[k] = buf[off:off + t.numel()].view(t.shape)
            into[k].copy_(t)
            off += t.numel()
        return buf

    # ---- forward: every activation the backward pass reads goes on the tape -----------------------------------------
    def _conv_act_fwd(self, x, name, layout, frame=False):
        """conv_act of the reference (policy_value_net_mxnet.py:28-39): Convolution -> BatchNorm(fix_gamma) -> relu
        -> (a, ConvAct).  On a framed board a 1x1 convolution (a head) reads the S x S window of its padded-row input and
        everything behind it is dense S x S.  frame (the stem of a framed board): the planes go into the 15x15 frame first,
        and the BatchNorm runs BEHIND to_rows16 (the dense convolution leaves bias-and-neighbour values off the board; the
        framed BatchNorm is the mask): x = the framed planes, y / a padded rows."""
        o, p = self.ops, self.p
        w = p[name + "_weight"]
        if frame:
            x = o.frame_planes(x)
        if w.shape[2] == 1:
            y, blay = o.conv1x1_fwd(x, w, p[name + "_bias"], layout, side=self.frame_side), o.DENSE
        elif name in self._gen:          # (a fast pass on the dense route)
            y, blay = o.conv3x3_fwd_f16x2_dense_packed(x, self._gen[name][0], flag=self._flag), layout
        else:
            y, blay = o.conv3x3_fwd(x, w, p[name + "_bias"], layout), layout
        side = self.frame_side if frame else None
        if frame:
            y, blay = o.to_rows16(y), o.ROWS16
        a, mean, invstd = o.bn_fwd(y, None, p[name + "_beta"], p[name + "_mean"], p[name + "_var"], None, True, blay,
                                   1.0 - BN_MOMENTUM, BN_EPS, side=side)
        return a, ConvAct(name, x, y, a, mean, invstd, layout, blay, side)

    def _act_bwd(self, da, rec, dymax=None):
        """conv_act's BatchNorm and relu backwards -> dy in the layout its convolution wrote (framed stem: off-board cells
        zero, so the dense 15x15 gradients behind it are the S x S board's); dymax: receives bn_bwd's dxmax"""
        o = self.ops
        dy, _, _, self.grad[rec.name + "_beta"] = o.bn_bwd(da, rec.y, rec.a, None, rec.mean, rec.invstd, True, False, rec.blay,
                                                         dxmax=dymax, side=rec.side)
        return o.from_rows16(dy) if rec.side else dy

    def _conv_act_bwd(self, da, rec, need_dx):
        """conv_act backwards, 3x3 (the two 1x1 heads share their input: _backward runs them as a pair)"""
        o, g = self.ops, self.grad
        # a fast pass on the dense route: the BatchNorm leaves max |dy| for the f16x2 data gradient right behind it
        fast = need_dx and rec.name in self._gen
        dymax = o._empty((o.bn_bwd_splits(rec.y, rec.blay), int(rec.y.shape[1])), da) if fast else None
        dy = self._act_bwd(da, rec, dymax)
        g[rec.name + "_weight"] = o.conv3x3_wgrad(rec.x, dy, rec.layout)
        g[rec.name + "_bias"] = o.bias_grad(dy, rec.layout)
        if fast:
            return o.conv3x3_dgrad_f16x2_dense(dy, self._gen[rec.name][1], dymax, self._flag)
        return o.conv3x3_dgrad(dy, self.p[rec.name + "_weight"], rec.layout) if need_dx else None

    def _trunk_conv(self, j):
        """Trunk convolution j = 2 i - 2 (A of block i) or 2 i - 1 (B): its parameter prefix"""
        return "conv%s%d" % ("AB"[j % 2], j // 2 + 1)

    def _trunk_conv_fwd(self, x, j):
        """Trunk convolution j on x -> (y, stats): stats = the per-board sums bn_fwd(stats=...) takes, or None.  Padded rows:
        on the f16x2 kernel in a fast pass, else on the Winograd kernel, whose epilogue leaves the BatchNorm's sums (no
        statistics pass; apz_wino_conv_stats is one launch: up to 16384 boards); other nets plain."""
        o = self.ops
        if self._fast and self.rows16:
            return o.conv3x3_fwd_stats_f16x2(x, self._u16[0][j, 0], self._u16[1][j, 0], self._flag)
        if self._trunk_conv(j) in self._gen:       # (a fast pass on the dense route)
            return o.conv3x3_fwd_f16x2_dense_packed(x, self._gen[self._trunk_conv(j)][0], flag=self._flag), None
        w, b = self.p[self._trunk_conv(j) + "_weight"], self.p[self._trunk_conv(j) + "_bias"]
        if not self.rows16:
            return o.conv3x3_fwd(x, w, b, o.DENSE), None
        if self.frame_side is None and int(x.shape[0]) <= 16384:      # (the epilogue's sums cover all 225 cells)
            return o.conv3x3_fwd_stats(x, w, b, upk=self._upk[j, 0])
        return o.conv3x3_fwd(x, w, b, o.ROWS16, upk=self._upk[j, 0]), None

    def _trunk_conv_dgrad(self, dy, j, skip=None, dymax=None):
        """The data gradient of trunk convolution j (+ skip: the skip connection's gradient of the same tensor) on the
        kernel of the pass; dymax: bn_bwd's dxmax for dy (the f16x2 launch's input scale)."""
        o = self.ops
        if self._fast and self.rows16:
            return o.conv3x3_dgrad_f16x2(dy, self._u16[0][j, 1], self._u16[1][j, 1], dymax, self._flag, add=skip)
        if self._trunk_conv(j) in self._gen:
            return o.conv3x3_dgrad_f16x2_dense(dy, self._gen[self._trunk_conv(j)][1], dymax, self._flag, add=skip)
        w = self.p[self._trunk_conv(j) + "_weight"]
        if not self.rows16:
            return o.conv3x3_dgrad(dy, w, o.DENSE, add=skip)
        return o.conv3x3_dgrad(dy, w, o.ROWS16, add=skip, upk=self._upk[j, 1])

    def _forward(self, states, step):
        o, p = self.ops, self.p
        tape = {"blocks": [], "stack": []}
        if self._fast and self._gen_names:     # the dense route's weights, both orientations, one launch (it zeroes the overflow word)
            self._gen_out = o.conv15h_pack_many([(p[k + "_weight"], p[k + "_bias"]) for k in self._gen_names], self._gen_out,
                                                self._flag)
            self._gen = dict(zip(self._gen_names, self._gen_out))
        if self.kind == "resnet":
            S = self.frame_side
            x, tape["stem"] = self._conv_act_fwd(states, "res_conv1", o.DENSE, frame=bool(S))
            lay = o.ROWS16 if self.rows16 else o.DENSE
            if self.rows16:             # every trunk layer's weights packed for this pass's kernel, both orientations, one launch
                if not S:
                    x = o.to_rows16(x)
                if self._fast:          # (the pack launch zeroes the step's overflow word)
                    self._u16 = o.wino3h_pack_many(self._trunk_w, self._trunk_b, self._u16, self._flag)
                else:
                    self._upk = o.wino_pack_many(self._trunk_w, self._upk)
            wm = self.rows16            # padded rows: the ReLU decisions as a byte per four elements for the backward pass
            for i in range(1, self.n_blocks + 1):
                A, B = "bnA%d" % i, "bnB%d" % i
                ya, sa = self._trunk_conv_fwd(x, 2 * i - 2)
                ha, ma, ia, *ka = o.bn_fwd(ya, p[A + "_gamma"], p[A + "_beta"], p[A + "_moving_mean"], p[A + "_moving_var"], None,
                                           True, lay, 1.0 - BN_MOMENTUM, BN_EPS, stats=sa, want_mask=wm, side=S)
                yb, sb = self._trunk_conv_fwd(ha, 2 * i - 1)
                out, mb, ib, *kb = o.bn_fwd(yb, p[B + "_gamma"], p[B + "_beta"], p[B + "_moving_mean"], p[B + "_moving_var"], x,
                                            True, lay, 1.0 - BN_MOMENTUM, BN_EPS, stats=sb, want_mask=wm, side=S)
                tape["blocks"].append(Block(x, ya, ha, ma, ia, yb, out, mb, ib, ka[0] if ka else None, kb[0] if kb else None))
                x = out
        else:
            lay = o.DENSE
            x = states
            for name in SIMPLE_CONVS:
                x, rec = self._conv_act_fwd(x, name, lay)
                tape["stack"].append(rec)
        tape["layout"] = lay
        n = int(x.shape[0])
        pol, tape["pol"] = self._conv_act_fwd(x, "conv3_1_1", lay)
        val, tape["val"] = self._conv_act_fwd(x, "conv3_2_1", lay)
        pol, val = pol.view(n, -1), val.view(n, -1)
        if self.dropout > 0:
            keep = 1.0 - self.dropout
            pol = o.dropout(pol, keep, self.seed, 2 * (self.dropout_step0 + step))
            val = o.dropout(val, keep, self.seed, 2 * (self.dropout_step0 + step) + 1)
        tape["pol_in"], tape["val_in"] = pol, val
        logits = o.fc_fwd(pol, p["fc_3_1_1_weight"], p["fc_3_1_1_bias"])
        vlogit = o.fc_fwd(val, p["fc_3_2_1_weight"], p["fc_3_2_1_bias"]).view(n)
        return logits, vlogit, tape

    # ---- backward ---------------------------------------------------------------------------------------------------
    def _backward(self, tape, dlogits, dvlogit):
        o, p, g = self.ops, self.p, self.grad
        n = int(dlogits.shape[0])
        lay = tape["layout"]
        dpol, g["fc_3_1_1_weight"], g["fc_3_1_1_bias"] = o.fc_bwd(tape["pol_in"], p["fc_3_1_1_weight"], dlogits)
        dval, g["fc_3_2_1_weight"], g["fc_3_2_1_bias"] = o.fc_bwd(tape["val_in"], p["fc_3_2_1_weight"], dvlogit.view(n, 1))
        if self.dropout > 0:
            keep = 1.0 - self.dropout
            dpol = o.dropout(dpol, keep, self.seed, 2 * (self.dropout_step0 + tape["step"]))
            dval = o.dropout(dval, keep, self.seed, 2 * (self.dropout_step0 + tape["step"]) + 1)
        # the two heads share their input: both BatchNorm backward passes, then ONE pass over the trunk output for dx
        dys = [self._act_bwd(dpol.view(n, 4, self.side, self.side), tape["pol"]),
               self._act_bwd(dval.view(n, 2, self.side, self.side), tape["val"])]
        dx, g["conv3_1_1_weight"], g["conv3_1_1_bias"], g["conv3_2_1_weight"], g["conv3_2_1_bias"] = o.conv1x1_bwd_pair(
            tape["pol"].x, p["conv3_1_1_weight"], dys[0], p["conv3_2_1_weight"], dys[1], tape["pol"].layout, side=self.frame_side)
        if self.kind == "resnet":
            # the trunk convolutions' bias gradients = column sums of the dx their BatchNorms hand back: every bn_bwd
            # leaves its per-split sums in its own columns of ONE matrix, added after the loop in one launch
            nb, S = self.n_blocks, self.frame_side
            nf = int(tape["blocks"][0].ya.shape[1]) if nb else 0
            parts = o._empty((o.bn_bwd_splits(tape["blocks"][0].ya, lay), 2 * nb * nf), dx) if nb else None
            # f16x2: each bn_bwd also leaves max |dx| per split and channel, which the data-gradient launch right behind it
            # folds into its input scale (one buffer: every pair runs in stream order)
            dmax = o._empty((parts.shape[0], nf), dx) if (self._fast and nb) else None
            for i in range(nb, 0, -1):
                A, B = "A%d" % i, "B%d" % i
                blk = tape["blocks"][i - 1]
                ca, cb = (2 * i - 2) * nf, (2 * i - 1) * nf
                dyb, dskip, g["bn" + B + "_gamma"], g["bn" + B + "_beta"] = o.bn_bwd(
                    dx, blk.yb, blk.out, p["bn" + B + "_gamma"], blk.mb, blk.ib, True, True, lay, dxsum=parts[:, cb:cb + nf],
                    mask=blk.kb, dxmax=dmax, side=S)
                g["conv" + B + "_weight"] = o.conv3x3_wgrad(blk.ha, dyb, lay)
                dha = self._trunk_conv_dgrad(dyb, 2 * i - 1, None, dmax)
                dya, _, g["bn" + A + "_gamma"], g["bn" + A + "_beta"] = o.bn_bwd(
                    dha, blk.ya, blk.ha, p["bn" + A + "_gamma"], blk.ma, blk.ia, True, False, lay, dxsum=parts[:, ca:ca + nf],
                    mask=blk.ka, dxmax=dmax, side=S)
                g["conv" + A + "_weight"] = o.conv3x3_wgrad(blk.x, dya, lay)
                dx = self._trunk_conv_dgrad(dya, 2 * i - 2, dskip, dmax)       # trunk + skip gradients meet
            db = o.colsum(parts) if nb else None
            for i in range(1, nb + 1):
                g["convA%d_bias" % i] = db[(2 * i - 2) * nf:(2 * i - 1) * nf]
                g["convB%d_bias" % i] = db[(2 * i - 1) * nf:2 * i * nf]
            if self.rows16 and not S:      # (the framed stem's BatchNorm takes padded rows)
                dx = o.from_rows16(dx)
            self._conv_act_bwd(dx, tape["stem"], False)
        else:
            for j in range(len(SIMPLE_CONVS) - 1, -1, -1):
                dx = self._conv_act_bwd(dx, tape["stack"][j], j > 0)

    # ---- one optimiser step (policy_value_net_mxnet.py:282-299) -----------------------------------------------------
    def _to(self, a, shape):
        t = self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).reshape(shape)
        return t.to(self.device).contiguous()

    def upload(self, state_batch, mcts_probs, winner_batch):
        """-> a DeviceBatch that train_step / loss_and_grads take in place of the three host arrays: a policy_update feeds
        the SAME mini-batch to every epoch (train_mxnet.py:201-207), so it goes to the device once (4.6 MB at batch 512:
        0.26 ms of an idle GPU in front of every step otherwise)."""
        return DeviceBatch(self._to(state_batch, (-1, self.c_in, self.side, self.side)), self._to(mcts_probs, (-1, self.hw)),
                           self._to(winner_batch, (-1,)))

    def loss_and_grads(self, state_batch, mcts_probs=None, winner_batch=None, keep_tape=False):
        """Forward + backward in training mode (moving statistics are updated).  -> (loss3 device tensor =
        (value loss, policy loss, entropy)); the gradients of the MEAN loss land in self.grad.  keep_tape: hold on to
        the saved activations afterwards (relu_masks(); tests).  state_batch: host array, or upload()'s DeviceBatch.
        trunk_arith "f16x2": the call reads the overflow word (a synchronisation) and repeats itself on the exact kernels
        when it is set (train_step does the same without the extra synchronisation)."""
        return self._attempts(state_batch, mcts_probs, winner_batch, None, keep_tape)[0]

    def _pass(self, batch, fast, keep_tape, loss3):
        """Forward and backward of one DeviceBatch, the trunk on the f16x2 kernels if `fast` -> loss3 (given, or new)"""
        self.grad = {}
        self._fast = fast
        try:
            logits, vlogit, tape = self._forward(batch.states, self.t)
            tape["step"] = self.t
            out = self.ops.pv_loss(logits, vlogit, batch.pis, batch.zs, grads=True, loss3=loss3,
                                   occ=self._occupancy(batch.states) if self.legal_policy else None)
            self._backward(tape, out["dlogits"], out["dvlogit"])
        finally:
            self._fast = False
            self._gen = {}
        self.tape = tape if keep_tape else None
        return out["loss3"]

    def _attempt(self, batch, fast, learning_rate, keep_tape, snapshot=True):
        """One attempt at a step, queued: the pass (fast: on the f16x2 kernels) and, with a learning rate (None:
        loss_and_grads), t += 1, Adam and the average's launch -> (loss3 on the device, the read-back).  The rules of the
        step's words live here and nowhere else:
          snapshot   of the moving statistics, where something may refuse the attempt: an f16x2 pass or a guarded step
                     (snapshot=False: the repeat of a pass, the snapshot still holds the statistics at the start of the step)
          skip word  of Adam: the overflow word on a fast attempt (the guard counts it among its reasons); of the average: the
                     guard record's skip word under the guard, else Adam's
          read-back  ONE device -> host copy, the attempt's only synchronisation: the word buffer [loss3][overflow word]
                     (+ [record]: guarded) where the trainer has one, else loss3; none for an exact pass without a step.
                     loss3 means something after a step, word 3 after a fast attempt, the record after a guarded step."""
        step = learning_rate is not None
        guarded = step and self.step_guard
        if snapshot and (fast or guarded):
            self._stat_snap.copy_(self._stat_buf)
        loss3 = self._pass(batch, fast, keep_tape, self._word[:3] if (step and self._word is not None) else None)
        if step:
            self.t += 1
            overflow = self._flag if fast else None
            self._adam(learning_rate, skip=overflow, guarded=guarded)
            self._ema(skip=self._record[2:3] if guarded else overflow)
        back = self._word if (self._word is not None and (step or fast)) else loss3 if step else None
        return loss3, (None if back is None else back.cpu().numpy())

    def _attempts(self, state_batch, mcts_probs, winner_batch, learning_rate, keep_tape):
        """The attempt on the trainer's arithmetic and, when an f16x2 launch of it left the fp16 range (nothing reached Adam
        or the average: the overflow word skipped them), everything taken back and the exact attempt -> what that returns;
        its word 3 is still set and says nothing"""
        batch = state_batch if isinstance(state_batch, DeviceBatch) else self.upload(state_batch, mcts_probs, winner_batch)
        fast = self.trunk_arith == "f16x2"
        loss3, w = self._attempt(batch, fast, learning_rate, keep_tape)
        if fast and w[3:4].view(np.uint32)[0] != 0:
            self.trunk_overflows += 1
            self._take_back(learning_rate is not None)
            loss3, w = self._attempt(batch, False, learning_rate, keep_tape, snapshot=False)
        return loss3, w

    def _take_back(self, stepped=True):
        """A refused attempt: the moving statistics as at its start, and t (the next attempt draws the same dropout masks; the
        internal evaluator is not stale)"""
        self._stat_buf.copy_(self._stat_snap)
        if stepped:
            self.t -= 1

    def relu_masks(self):
        """{layer: [n][C][H][W] bool} -- which activations of the kept forward pass were positive.  (A comparator that
        takes its ReLU decisions from here differs from this trainer by rounding only: an activation within rounding
        distance of zero otherwise lands on different sides in different arithmetic and moves whole gradient rows.)"""
        S = self.frame_side
        cut = (lambda t: t[..., :S, :S]) if S else (lambda t: t[..., :15]) if self.rows16 else (lambda t: t)
        tape, out = self.tape, {}
        recs = [tape["pol"], tape["val"]] + tape["stack"] + ([tape["stem"]] if "stem" in tape else [])
        for rec in recs:
            out[rec.name] = (cut(rec.a) if (S and rec.name == "res_conv1") else rec.a) > 0
        for i, blk in enumerate(tape["blocks"], 1):
            out["bnA%d" % i] = cut(blk.ha) > 0
            out["block%d" % i] = cut(blk.out) > 0
        return out

    def train_step(self, state_batch, mcts_probs, winner_batch, learning_rate, keep_tape=False):
        """One optimiser step -> (loss, entropy).  state_batch may be upload()'s DeviceBatch (mcts_probs / winner_batch are
        then ignored).  step_guard: see __init__ -- a skipped step returns its own losses, NaN included."""
        _, w = self._attempts(state_batch, mcts_probs, winner_batch, learning_rate, keep_tape)
        self._verdict(w)
        return float(w[0] + w[1]), float(w[2])

    def _verdict(self, w):
        """What the step's last read-back says of it.  Guarded: the record -- a skip takes the step back; a rescale other than
        1 / batch_size is a clip.  A step that stands has moved the average."""
        if self.step_guard:
            norm, eff, skip, why = self.ops.read_guard_record(w[4:8])
            self.last_grad_norm, self.last_rescale_eff = norm, eff
            self.last_skip_reason = self.ops.guard_reason(why)
            if skip:
                self._take_back()
                self.skipped_steps += 1
                return
            if eff != np.float32(1.0 / self.batch_size):
                self.clipped_steps += 1
        if self.ema_p is not None:
            self.ema_updates += 1

    def _entries(self):
        return [(self.p[k], self.grad[k], self.m[k], self.v[k], self.wd if k.endswith(("_weight", "_gamma")) else 0.0)
                for k in self.train_names]

    def _adam(self, learning_rate, skip=None, guarded=False):
        b1, b2, eps = 0.9, 0.999, 1e-8
        lr_t = learning_rate * (1.0 - b2 ** self.t) ** 0.5 / (1.0 - b1 ** self.t)
        if guarded:
            self.ops.adam_step_guarded(self._entries(), lr_t, b1, b2, eps, 1.0 / self.batch_size, self.clip_norm, self.device,
                                       loss3=self._word[:3], skip=skip, record=self._record)
        else:
            self.ops.adam_step(self._entries(), lr_t, b1, b2, eps, 1.0 / self.batch_size, self.device, skip=skip)

    def _ema(self, skip=None):
        """The averaged weights' launch behind an Adam launch (nothing without ema_decay).  skip: that Adam launch's skip
        word.  The coefficient belongs to ema_updates as it stands: a launch that skips on the device is followed by one
        with the same coefficient."""
        if self.ema_p is None:
            return
        c = ema_coefficient(self.ema_decay, self.ema_updates, self.ema_warmup)
        self.ops.ema_update(self._ema_tab, c, self.device, skip=skip)

    def ema_params(self):
        """The averaged weights as host arrays, in get_params()'s order (ValueError without ema_decay)"""
        if self.ema_p is None:
            raise ValueError("this trainer keeps no averaged weights (ema_decay=None)")
        return collections.OrderedDict((k, v.cpu().numpy()) for k, v in self.ema_p.items())

    def grad_norm(self):
        """The global norm of self.grad after a loss_and_grads, as the guard measures it: of grad / batch_size, the gradient
        Adam sees before weight decay -- the scale clip_norm is compared with.  Two launches and a read-back (a
        synchronisation); works with the guard off as well."""
        if not self.grad:
            raise RuntimeError("grad_norm() needs the gradients of a loss_and_grads or train_step")
        rec = self.ops.grad_norm(self._entries(), 1.0 / self.batch_size, None, self.device)
        return self.ops.read_guard_record(rec.cpu().numpy())[0]

    def sync_evaluator(self, net, ema=False):
        """Give `net` (a PolicyValueNet of the same architecture) this trainer's current weights, device to device:
        folding and packing run as kernels behind the optimiser step on the same stream (apz_load_weights_dev).
        ema=True: the averaged weights instead (ValueError without ema_decay)."""
        if ema and self.ema_p is None:
            raise ValueError("this trainer keeps no averaged weights (ema_decay=None)")
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        net.load_device_params(self.ema_p if ema else self.p, stream)

    def policy_value(self, state_batch):
        """Inference-mode (moving statistics) probabilities and values for the KL monitor: the self-play path's own
        evaluator (PolicyValueNet) on the current weights."""
        return self._evaluator().policy_value(state_batch)

    def policy_value_dev(self, planes):
        """policy_value on a device tensor of planes (PolicyValueNet.policy_value_dev): same bits, no upload"""
        return self._evaluator().policy_value_dev(planes)

    def _evaluator(self):
        from .policy_value_net import PolicyValueNet
        if self._eval is None:
            nf = int(next(iter(self.p.values())).shape[0]) if self.kind == "resnet" else 128
            self._eval = PolicyValueNet(self.side, self.side, batch_size=self.batch_size, n_blocks=self.n_blocks, n_filter=nf,
                                        model_params=self.get_params(), net_kind=self.kind, c_in=self.c_in,
                                        device=self.device.index or 0, legal_policy=self.legal_policy)
            self._eval_t = self.t
        elif self._eval_t != self.t:
            self.sync_evaluator(self._eval)
            self._eval_t = self.t
        return self._eval

    def get_params(self):
        return collections.OrderedDict((k, v.cpu().numpy()) for k, v in self.p.items())

    # ---- checkpoint -----------------------------------------------------------------------------------------------
    def _groups(self, ema):
        """The tensor groups of a state by their key prefix; ema: the averaged weights among them"""
        return [("p", self.p), ("m", self.m), ("v", self.v)] + ([("e", self.ema_p)] if ema else [])

    def state(self):
        """Everything the next train_step reads, as host values: {"meta": t, dropout_step0, seed, trunk_overflows, the guard's
        two settings and two counters and the net's kind (the dropout masks are keyed by seed and dropout_step0 + t),
        "p/<name>": every parameter and BatchNorm statistic, "m/<name>" / "v/<name>": Adam's moments} -- what load_state
        takes.  With ema_decay: "e/<name>", the averaged weights, and meta's ema_decay, ema_warmup and ema_updates."""
        out = {"meta": {"t": int(self.t), "dropout_step0": int(self.dropout_step0), "seed": int(self.seed),
                        "trunk_overflows": int(self.trunk_overflows), "net_kind": self.kind, "n_blocks": int(self.n_blocks),
                        "trunk_arith": self.trunk_arith, "framed": self.framed, "step_guard": self.step_guard,
                        "clip_norm": self.clip_norm, "skipped_steps": int(self.skipped_steps),
                        "clipped_steps": int(self.clipped_steps)}}
        if self.legal_policy:          # (a trainer without the switch writes what it always wrote)
            out["meta"]["legal_policy"] = True
        if self.ema_p is not None:
            out["meta"].update(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_updates=int(self.ema_updates))
        for tag, group in self._groups(self.ema_p is not None):
            for k, t in group.items():
                out["%s/%s" % (tag, k)] = t.cpu().numpy()
        return out

    def load_state(self, state):
        """Continue where the trainer that returned `state` stood (same net: names and shapes are checked before anything
        is written).  The values are copied INTO the existing tensors: the trunk weights, biases and statistics are views
        into the packed buffers the kernels read.  The internal evaluator is stale afterwards and re-synchronises on its
        next use.  The averaged weights: a state that holds them ("e/<name>") continues them in a trainer built with
        ema_decay and is read without them by one built without; a state that holds none starts the average of a trainer
        built with ema_decay at the loaded weights, ema_updates = 0."""
        meta = state["meta"]
        if meta["net_kind"] != self.kind or int(meta["n_blocks"]) != self.n_blocks:
            raise ValueError("this trainer state belongs to a %s net of %s blocks" % (meta["net_kind"], meta["n_blocks"]))
        if bool(meta.get("framed", False)) != self.framed:
            raise ValueError("this trainer state was written with framed=%s, the trainer was built with framed=%s" %
                             (bool(meta.get("framed", False)), self.framed))
        if bool(meta.get("legal_policy", False)) != self.legal_policy:      # (a state from before the switch: off)
            raise ValueError("this trainer state was written with legal_policy=%s, the trainer was built with legal_policy=%s" %
                             (bool(meta.get("legal_policy", False)), self.legal_policy))
        todo = []
        with_ema = self.ema_p is not None and any(k.startswith("e/") for k in state)
        for tag, group in self._groups(with_ema):
            for k, t in group.items():
                a = state.get("%s/%s" % (tag, k))
                if a is None or tuple(np.shape(a)) != tuple(t.shape):
                    raise ValueError("this trainer state has no %s/%s of shape %s" % (tag, k, tuple(t.shape)))
                todo.append((t, np.ascontiguousarray(a, dtype=np.float32)))
        for t, a in todo:
            t.copy_(self.torch.from_numpy(a))
        if self.ema_p is not None and not with_ema:
            for k, t in self.ema_p.items():
                t.copy_(self.p[k])
        self.torch.cuda.current_stream(self.device).synchronize()
        self.t = int(meta["t"])
        self.dropout_step0 = int(meta["dropout_step0"])
        self.seed = int(meta["seed"])
        self.trunk_overflows = int(meta["trunk_overflows"])
        # (a state from before the guard: zeros.  Whether THIS trainer guards and clips is its constructor's word; the
        # state's own step_guard / clip_norm say what the run that wrote it did.)
        self.skipped_steps = int(meta.get("skipped_steps", 0))
        self.clipped_steps = int(meta.get("clipped_steps", 0))
        if self.ema_p is not None:
            self.ema_updates = int(meta.get("ema_updates", 0)) if with_ema else 0
        self._eval_t = -1
        self.tape = None

    def get_grads(self):
        return collections.OrderedDict((k, self.grad[k].cpu().numpy()) for k in self.train_names)

    def close(self):
        if self._eval is not None:
            self._eval.close()
            self._eval = None


def explained_variance(winner_z, value):
    """train_mxnet.py:222-227: 1 - Var(z - v) / Var(z) (NumPy semantics: a constant z gives nan / -inf, as there)."""
    z = np.asarray(winner_z, dtype=np.float64)
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(1.0 - np.var(z - v) / np.var(z))


# ---- the weight hand-off: a trainer's weights into an evaluator, device to device where both sides can, else through the host.
# Trainers and evaluators are duck-typed (HipTrainer / PolicyValueNet / LanedEvaluator, the tests' stand-ins): what an object
# can do is asked here and nowhere else.
def _host_array(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def trainer_weights(trainer, averaged=False, host=False):
    """{name: weight} of `trainer` (averaged: of its averaged weights): the device tensors themselves where the trainer keeps
    them (`p` / `ema_p` beside `torch`) and host=False, else host arrays (get_params() / ema_params() / ema_p)."""
    if not host and hasattr(trainer, "torch") and hasattr(trainer, "ema_p" if averaged else "p"):
        return trainer.ema_p if averaged else trainer.p
    if not averaged:
        return trainer.get_params()
    if hasattr(trainer, "ema_params"):
        return trainer.ema_params()
    return {k: _host_array(v) for k, v in trainer.ema_p.items()}


def load_weights(net, weights, keep_trainer, stream=None):
    """The mapping `weights` into evaluator `net`: load_device_params where the values are device tensors and the evaluator
    has it -- it packs from them asynchronously, so the caller keeps what this returns alive -- else set_params with host
    arrays (-> None).  keep_trainer: set_params must not drop the evaluator's own trainer (PolicyValueNet's _keep_trainer)."""
    if getattr(next(iter(weights.values())), "is_cuda", False) and hasattr(net, "load_device_params"):
        net.load_device_params(weights, *(() if stream is None else (stream,)))
        return weights
    net.set_params({k: _host_array(v) for k, v in weights.items()}, **({"_keep_trainer": True} if keep_trainer else {}))
    return None


def sync_weights(trainer, net, averaged=False, keep_trainer=False):
    """The trainer's current (averaged: averaged) weights into evaluator `net`: HipTrainer.sync_evaluator, on torch's current
    stream, where the trainer has it and the evaluator takes device tensors, else through the host."""
    if hasattr(trainer, "sync_evaluator") and hasattr(net, "load_device_params") and (not averaged or hasattr(trainer, "ema_p")):
        trainer.sync_evaluator(net, **({"ema": True} if averaged else {}))
    else:
        load_weights(net, trainer_weights(trainer, averaged, host=True), keep_trainer)


def policy_update(trainer, mini_batch, learn_rate=1e-3, lr_multiplier=1.0, epochs=8, kl_targ=0.02, evaluator=None, monitors=None):
    """train_mxnet.py:194-240: epochs x train_step with KL early stop and the adaptive LR multiplier.
    mini_batch: list of (state, mcts_prob, winner_z).  `evaluator.policy_value(states)` (the HIP
    PolicyValueNet) supplies old/new predictions when given, else the trainer's own inference
    graph.  -> (loss, entropy, kl, lr_multiplier); `monitors` (a dict, optional) receives the reference's value-head
    monitors explained_var_old / explained_var_new (train_mxnet.py:222-227) and the learning rate used.
    A trainer with the guard's counters (HipTrainer: skipped_steps, clipped_steps, last_grad_norm) also gets grad_norm (of
    the update's last step), skipped_steps and clipped_steps (of this update) into `monitors`, and an update whose every
    step was skipped leaves lr_multiplier alone: it changed nothing, so its KL is 0 and would otherwise raise it.
    mini_batch may also be the DeviceBatch a code replay buffer draws (alphapig_amd/replay.py), already stacked.  NumPy
    arrays (CompactReplayBuffer): uploaded once, like the list's.  Device tensors (DeviceReplayBuffer): no stacking and no
    upload; the KL monitor's forwards read the planes where they are (`policy_value_dev`; an evaluator without it gets them
    on the host, once) and zs come to the host once for the explained-variance monitors.  The KL stays the NumPy expression
    on the probabilities copied back: it decides the early stop and the learning-rate multiplier, so its bits must not
    depend on the buffer kind."""
    pv = (evaluator.policy_value if evaluator is not None else trainer.policy_value)
    if isinstance(mini_batch, DeviceBatch) and not isinstance(mini_batch.states, np.ndarray):
        batch, (states, pis, zs) = mini_batch, mini_batch
        pv_dev = getattr(evaluator if evaluator is not None else trainer, "policy_value_dev", None)
        if pv_dev is not None:
            pv = pv_dev
        else:
            states = states.cpu().numpy()
        pis, zs = None, zs.cpu().numpy()           # (train_step ignores them beside a DeviceBatch)
    else:
        if isinstance(mini_batch, DeviceBatch):
            states, pis, zs = (np.ascontiguousarray(a, dtype=np.float32) for a in mini_batch)
        else:
            states = np.stack([np.ascontiguousarray(d[0]) for d in mini_batch]).astype(np.float32)
            pis = np.stack([d[1] for d in mini_batch]).astype(np.float32)
            zs = np.array([d[2] for d in mini_batch], dtype=np.float32)
        batch = trainer.upload(states, pis, zs) if hasattr(trainer, "upload") else states     # once for all epochs
    old_probs, old_v = pv(states)
    new_v = old_v
    loss = entropy = kl = 0.0
    lr_used = lr_multiplier                               # (the reference logs learn_rate * the multiplier the epochs ran with)
    # a guarded trainer (HipTrainer(step_guard=True)) counts the steps it refused; one without the guard or the counters
    # behaves as before
    guarded = bool(getattr(trainer, "step_guard", hasattr(trainer, "skipped_steps")))
    skipped0, clipped0 = (int(trainer.skipped_steps), int(getattr(trainer, "clipped_steps", 0))) if guarded else (0, 0)
    steps = 0
    for _ in range(epochs):
        loss, entropy = trainer.train_step(batch, pis, zs, learn_rate * lr_multiplier)
        steps += 1
        if evaluator is not None:
            sync_weights(trainer, evaluator)
        new_probs, new_v = pv(states)
        kl = float(np.mean(np.sum(old_probs * (np.log(old_probs + 1e-10) - np.log(new_probs + 1e-10)), axis=1)))
        if kl > kl_targ * 4:
            break
    skipped = int(trainer.skipped_steps) - skipped0 if guarded else 0
    if steps > 0 and skipped == steps:
        pass            # every step was skipped: nothing changed, the KL is 0 and says nothing about the learning rate
    elif kl > kl_targ * 2 and lr_multiplier > 0.05:        # train_mxnet.py:215-218
        lr_multiplier /= 1.5
    elif kl < kl_targ / 2 and lr_multiplier < 20:
        lr_multiplier *= 1.5
    if monitors is not None and guarded:
        monitors["grad_norm"] = getattr(trainer, "last_grad_norm", None)       # of the update's last step
        monitors["skipped_steps"] = skipped                                      # in this update
        monitors["clipped_steps"] = int(getattr(trainer, "clipped_steps", 0)) - clipped0
    if monitors is not None:
        monitors["explained_var_old"] = explained_variance(zs, old_v)
        monitors["explained_var_new"] = explained_variance(zs, new_v)
        monitors["learn_rate"] = float(learn_rate * lr_used)
    return loss, entropy, kl, lr_multiplier
