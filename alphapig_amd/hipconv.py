"""The training graph's operators on the hand-written HIP kernels, one thin function per
C-ABI entry point of include/alphapig_hip.h: 3x3 convolution forward / data gradient / weight gradient (direct MFMA
kernel, or the self-play path's fused Winograd kernel for the 128 -> 128 trunk shape), bias gradient, training-mode
BatchNorm (+ residual) (+ ReLU) forward and backward, the 1x1 head convolutions, FullyConnected, Dropout, the
policy-value loss, layout copies and Adam.

There is no autograd here and no PyTorch arithmetic: alphapig_amd/train.py calls these functions in the order of the
reference's graph (policy_value_net_mxnet.py:41-102, :173-212) and then in reverse.  Tensors are torch CUDA float32
tensors used as device buffers (allocation + data pointers) on torch's current stream; without the HIP library every
function raises.
"""
import ctypes as C

from . import _native
from ._native import ApzConfig

_ENGINES = {}

DENSE, ROWS16 = 0, 1       # APZ_LAYOUT_*: dense NCHW / the trunk's padded rows [n][C][15][16] (pad column zero)


def _engine(h, w, device_index):
    key = (h, w, device_index)
    if key not in _ENGINES:
        L = _native.hip()
        cfg = ApzConfig(h, w, 9, 128, 0, 0, 1, device_index)
        hnd = L.apz_create(C.byref(cfg))
        if not hnd:
            raise RuntimeError("apz_create failed: %s" % L.apz_last_error().decode())
        _ENGINES[key] = hnd
    return _ENGINES[key]


_TORCH = _F32 = None


def _torch():
    global _TORCH, _F32
    if _TORCH is None:
        import torch
        _TORCH, _F32 = torch, torch.float32
    return _TORCH


def _ck(L, rc):
    if rc < 0:
        raise RuntimeError("%s (code %d)" % (L.apz_last_error().decode(), rc))


def _any_engine(device_index):
    """Operators that do not depend on the board (FullyConnected, Dropout, Adam) run on whichever engine this device
    already has (the net's own board size), else on a 15x15 one."""
    for (h, w, d), hnd in _ENGINES.items():
        if d == device_index:
            return hnd
    return _engine(15, 15, device_index)


def _check(t, what, dtype=None, shape=None):
    """ValueError(what) unless t is a contiguous device tensor of `dtype` (default float32) -- and of `shape`, if given"""
    if not (t.is_cuda and t.dtype == (dtype or _F32 or _torch().float32) and t.is_contiguous() and
            (shape is None or tuple(t.shape) == shape)):
        raise ValueError(what)


def _ctx(x, board=None):
    """-> (library, engine handle, stream pointer) for every operator.  x: a tensor (checked: contiguous float32 on a
    device) or a torch.device; board: (height, width) of the engine, None = whichever the device has (_any_engine).  The
    stream is torch's current one on that device."""
    torch = _torch()
    if isinstance(x, torch.device):
        dev = x
    else:
        _check(x, "HIP operators take contiguous float32 device tensors")
        dev = x.device
    hnd = _any_engine(dev.index or 0) if board is None else _engine(board[0], board[1], dev.index or 0)
    return _native.hip(), hnd, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _board(x, layout=DENSE):
    """(height, width) of the board a tensor [n][C][H][W] in `layout` holds"""
    h, w = int(x.shape[2]), int(x.shape[3])
    if layout == ROWS16:
        if (h, w) != (15, 16):
            raise ValueError("padded-row tensors are [n][C][15][16]")
        w = 15
    return h, w


def _ptr(t):
    return None if t is None else t.data_ptr()


def _empty(shape, like):
    torch = _torch()
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def is_trunk_shape(weight, x, layout):
    """128 -> 128 channels on 15x15 boards: the shape of the self-play path's fused Winograd kernel."""
    board = (15, 16) if layout == ROWS16 else (15, 15)
    return tuple(weight.shape) == (128, 128, 3, 3) and tuple(x.shape[2:]) == board


# ---- 3x3 convolution ------------------------------------------------------------------------------------------------
def wino_pack_many(weights, out=None):
    """weights [count][128][128][3][3] (one contiguous tensor) -> [count][2][apz_wino_packed_size()]: every layer's
    transformed weights for the forward convolution ([:, 0]) and the data-gradient convolution ([:, 1]), one launch."""
    _check(weights, "wino_pack_many takes a contiguous float32 device tensor [count][128][128][3][3]", None,
           tuple(weights.shape[:1]) + (128, 128, 3, 3))
    L, hnd, stream = _ctx(weights, (15, 15))
    count = int(weights.shape[0])
    if out is None:
        out = _empty((count, 2, L.apz_wino_packed_size()), weights)
    _ck(L, L.apz_wino_pack_many(hnd, weights.data_ptr(), count, out.data_ptr(), stream))
    return out


def wino3h_pack_many(weights, biases=None, out=None, flag=None):
    """The training step's trunk weights for the f16x2 kernel: weights [count][128][128][3][3] and biases [count][128] (None:
    zero), one contiguous float32 device tensor each -> (upk [count][2][apz_wino3h_packed_size()], bias [count][2][256])
    for the forward ([:, 0]) and the data gradient ([:, 1]), one launch.  out: such a pair to fill again; flag: a device
    int32 word the launch zeroes (the overflow word of the step that follows)."""
    _check(weights, "wino3h_pack_many takes a contiguous float32 device tensor [count][128][128][3][3]", None,
           tuple(weights.shape[:1]) + (128, 128, 3, 3))
    count = int(weights.shape[0])
    if biases is not None and not (biases.is_contiguous() and biases.dtype == _torch().float32 and
                                   tuple(biases.shape) == (count, 128)):
        raise ValueError("biases: a contiguous float32 [count][128] tensor")
    L, hnd, stream = _ctx(weights, (15, 15))
    if out is None:
        out = (_empty((count, 2, L.apz_wino3h_packed_size()), weights), _empty((count, 2, 256), weights))
    _ck(L, L.apz_wino3h_pack_many(hnd, weights.data_ptr(), _ptr(biases), count, out[0].data_ptr(), out[1].data_ptr(), _ptr(flag),
                                  stream))
    return out


def conv3x3_fwd_stats_f16x2(x, upk, bias, flag):
    """conv3x3_fwd_stats on the f16x2 kernel: upk / bias = one layer's forward pair of wino3h_pack_many.  -> (y, stats);
    a non-finite output sets the int32 device word `flag` to 1."""
    L, hnd, stream = _ctx(x, _board(x, ROWS16))
    if tuple(x.shape[1:]) != (128, 15, 16):
        raise ValueError("conv3x3_fwd_stats_f16x2: the 128-channel trunk in the padded-row layout")
    n = int(x.shape[0])
    y = _empty(tuple(x.shape), x)
    stats = _torch().empty((128, n, 2), dtype=_torch().float64, device=x.device)
    _ck(L, L.apz_wino3h_conv_stats(hnd, x.data_ptr(), upk.data_ptr(), bias.data_ptr(), y.data_ptr(), stats.data_ptr(), n,
                                   flag.data_ptr(), stream))
    return y, stats


def conv3x3_dgrad_f16x2(dy, upk, bias, dymax, flag, add=None):
    """conv3x3_dgrad on the f16x2 kernel (padded rows): upk / bias = one layer's data-gradient pair of wino3h_pack_many;
    dymax = bn_bwd's dxmax for this dy (partial maxima of |dy|: the launch's power-of-two input scale; NaN entries are
    ignored, a +inf entry sets `flag`); (+ add)."""
    L, hnd, stream = _ctx(dy, _board(dy, ROWS16))
    if tuple(dy.shape[1:]) != (128, 15, 16) or (add is not None and add.shape != dy.shape):
        raise ValueError("conv3x3_dgrad_f16x2: the 128-channel trunk in the padded-row layout")
    n = int(dy.shape[0])
    dx = _empty(tuple(dy.shape), dy)
    _ck(L, L.apz_wino3h_conv_dgrad(hnd, dy.data_ptr(), upk.data_ptr(), bias.data_ptr(), _ptr(add), dx.data_ptr(), n,
                                   dymax.data_ptr(), int(dymax.numel()), flag.data_ptr(), stream))
    return dx


def conv3x3_wgrad_f16x2(x, dy, dymax, flag):
    """conv3x3_wgrad of the trunk shape on the f16x2 kernel (csrc/wgrad_wino3h.h; padded rows [n][128][15][16] only):
    dymax = bn_bwd's dxmax for this dy (partial maxima of |dy|: the launch's power-of-two scale of dy); flag = the int32
    overflow word, set -- never cleared -- when the transformed activations leave the fp16 range, a partial result is not
    finite or dymax holds +inf."""
    L, hnd, stream = _ctx(x, _board(x, ROWS16))
    if x.dim() != 4 or tuple(x.shape[1:]) != (128, 15, 16) or dy.shape != x.shape:
        raise ValueError("conv3x3_wgrad_f16x2: the 128 -> 128 trunk shape in the padded-row layout")
    if int(dymax.numel()) < 1:
        raise ValueError("conv3x3_wgrad_f16x2: dymax is empty")
    dw = _empty((128, 128, 3, 3), x)
    _ck(L, L.apz_wgrad_wino_f16x2(hnd, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), int(x.shape[0]), dymax.data_ptr(),
                                  int(dymax.numel()), flag.data_ptr(), stream))
    return dw


def conv3x3_fwd_f16x2_dense(x, weight, bias=None, resid=None, relu=False, flag=None):
    """y = act(conv2d(x, weight, bias, padding=1) (+ resid)) on the fp16 matrix pipe with two-term operands
    (csrc/conv15_split.h, apz_conv15h_fwd): dense x [n][C_in][15][15], raw weight [C_out][C_in][3][3], C_in a multiple of 64,
    C_out a multiple of 16, inputs up to 65 504 in magnitude.  A board's bits do not depend on the batch.  flag: a device
    int32 word (one element) that the launch sets to 1 -- never clears -- when a sum in front of the ReLU is not finite;
    None: a word of the call's own, which nobody reads."""
    if x.dim() != 4 or tuple(x.shape[2:]) != (15, 15):
        raise ValueError("conv3x3_fwd_f16x2_dense: dense [n][C_in][15][15] tensors only, not %s" % (tuple(x.shape),))
    L, hnd, stream = _ctx(x, (15, 15))
    torch = _torch()
    n, cin = int(x.shape[0]), int(x.shape[1])
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (cin, 3, 3):
        raise ValueError("conv3x3_fwd_f16x2_dense: weight must be [C_out][%d][3][3], not %s" % (cin, tuple(weight.shape)))
    cout = int(weight.shape[0])
    if n < 1 or cin % 64 or cout % 16:
        raise ValueError("conv3x3_fwd_f16x2_dense: C_in must be a multiple of 64, C_out a multiple of 16 and the batch not "
                         "empty, not %d boards of %d -> %d channels" % (n, cin, cout))
    _check(weight, "conv3x3_fwd_f16x2_dense: weight must be a contiguous float32 device tensor")
    if bias is not None:
        _check(bias, "conv3x3_fwd_f16x2_dense: bias must be a contiguous float32 device tensor [C_out]", None, (cout,))
    if resid is not None:
        _check(resid, "conv3x3_fwd_f16x2_dense: resid must be a contiguous float32 device tensor of y's shape", None,
               (n, cout, 15, 15))
    if flag is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=x.device)
    else:
        _check(flag, "conv3x3_fwd_f16x2_dense: flag must be an int32 device tensor of one element", torch.int32, (1,))
    y = _empty((n, cout, 15, 15), x)
    _ck(L, L.apz_conv15h_fwd(hnd, x.data_ptr(), weight.data_ptr(), _ptr(bias), _ptr(resid), y.data_ptr(), n, cin, cout,
                             int(bool(relu)), flag.data_ptr(), stream))
    return y


_CONV15H_ENTRY = [("w", "u8"), ("bias", "u8"), ("pk0", "u8"), ("pk1", "u8"), ("b0", "u8"), ("b1", "u8"), ("cin", "i4"),
                  ("cout", "i4")]     # apz_conv15h_pack_entry, 56 bytes


def _flag_word(flag, who, like):
    """The int32 overflow word of an f16x2 launch: the caller's (one element; a float32 view of a word buffer passes as
    well), or a word of the call's own, which nobody reads"""
    torch = _torch()
    if flag is None:
        return torch.zeros((1,), dtype=torch.int32, device=like.device)
    if not (flag.is_cuda and flag.is_contiguous() and flag.numel() == 1 and flag.dtype in (torch.int32, torch.float32)):
        raise ValueError("%s: flag must be a 32-bit device tensor of one element" % who)
    return flag


def conv15h_pack_many(layers, out=None, flag=None):
    """The training step's weights of the generic 15x15 nets for the f16x2 kernel (csrc/conv15_split.h), one launch for all
    of them.  layers: [(weight [C_out][C_in][3][3], bias [C_out] or None)] of contiguous float32 device tensors, C_in and
    C_out multiples of 64 -> [((pk, bias8h) of the forward, (pk, bias8h) of the data gradient)] per layer: pk float32
    [9 C_in C_out] words (two fp16 terms of w S), bias8h [2][channels] = (bias -- zero for the data gradient --, 1 / S).  The
    forward pair holds bit for bit what conv3x3_fwd_f16x2_dense packs per call.  out: such a list to fill again (the tensors
    of `layers` must be the ones it was made for); flag: a 32-bit device word the launch zeroes (the overflow word of the step
    that follows)."""
    import numpy as np
    layers = list(layers)
    if not layers:
        raise ValueError("conv15h_pack_many: no layers")
    L, hnd, stream = _ctx(layers[0][0], (15, 15))
    tab = np.zeros(len(layers), dtype=_CONV15H_ENTRY)
    made = []
    for i, (w, b) in enumerate(layers):
        _check(w, "conv15h_pack_many: weight %d must be a contiguous float32 device tensor [C_out][C_in][3][3]" % i)
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
            raise ValueError("conv15h_pack_many: weight %d must be [C_out][C_in][3][3], not %s" % (i, tuple(w.shape)))
        cout, cin = int(w.shape[0]), int(w.shape[1])
        if cin % 64 or cout % 64:
            raise ValueError("conv15h_pack_many: C_in and C_out must be multiples of 64, not %d -> %d (layer %d)" % (cin, cout, i))
        if b is not None:
            _check(b, "conv15h_pack_many: bias %d must be a contiguous float32 device tensor [C_out]" % i, None, (cout,))
        if out is None:
            words = int(L.apz_conv15h_packed_size(cin, cout))
            pair = ((_empty((words,), w), _empty((2, cout), w)), (_empty((words,), w), _empty((2, cin), w)))
        else:
            pair = out[i]
            if tuple(pair[0][1].shape) != (2, cout) or tuple(pair[1][1].shape) != (2, cin):
                raise ValueError("conv15h_pack_many: out[%d] was made for another layer" % i)
        made.append(pair)
        tab[i] = (w.data_ptr(), 0 if b is None else b.data_ptr(), pair[0][0].data_ptr(), pair[1][0].data_ptr(),
                  pair[0][1].data_ptr(), pair[1][1].data_ptr(), cin, cout)
    if flag is not None:
        flag = _flag_word(flag, "conv15h_pack_many", layers[0][0])
    _ck(L, L.apz_conv15h_pack_many(hnd, tab.ctypes.data_as(C.c_void_p), len(tab), _ptr(flag), stream))
    return made


def _conv15h_packed(who, x, packed, resid, what):
    """The shared argument checks of the two packed operators -> (n, C of x, C of the result)"""
    if x.dim() != 4 or tuple(x.shape[2:]) != (15, 15):
        raise ValueError("%s: dense [n][C][15][15] tensors only, not %s" % (who, tuple(x.shape)))
    _check(x, "%s: contiguous float32 device tensors" % who)
    pk, b8 = packed
    n, cin = int(x.shape[0]), int(x.shape[1])
    _check(pk, "%s: packed weights of conv15h_pack_many" % who)
    _check(b8, "%s: bias8h of conv15h_pack_many" % who)
    if b8.dim() != 2 or int(b8.shape[0]) != 2:
        raise ValueError("%s: bias8h must be [2][C]" % who)
    cout = int(b8.shape[1])
    if n < 1 or cin % 64 or cout % 16 or int(pk.numel()) != 9 * cin * cout:
        raise ValueError("%s: %d boards of %d channels do not fit packed weights of %d words for %d output channels" %
                         (who, n, cin, int(pk.numel()), cout))
    if resid is not None:
        _check(resid, "%s: %s must be a contiguous float32 device tensor of the result's shape" % (who, what), None,
               (n, cout, 15, 15))
    return n, cin, cout


def conv3x3_fwd_f16x2_dense_packed(x, packed, resid=None, flag=None):
    """y = conv2d(x, weight, bias, padding=1) (+ resid) as conv3x3_fwd_f16x2_dense(relu=False) computes it, bit for bit, on
    weights packed once per step: packed = a layer's forward pair of conv15h_pack_many.  flag as there."""
    n, cin, cout = _conv15h_packed("conv3x3_fwd_f16x2_dense_packed", x, packed, resid, "resid")
    L, hnd, stream = _ctx(x, (15, 15))
    flag = _flag_word(flag, "conv3x3_fwd_f16x2_dense_packed", x)
    y = _empty((n, cout, 15, 15), x)
    _ck(L, L.apz_conv15h_fwd_packed(hnd, x.data_ptr(), packed[0].data_ptr(), packed[1].data_ptr(), _ptr(resid), y.data_ptr(), n,
                                    cin, cout, flag.data_ptr(), stream))
    return y


def conv3x3_dgrad_f16x2_dense(dy, packed, dymax, flag=None, add=None):
    """dx = conv2d_input(dy, weight) (+ add) on the f16x2 kernel, dense tensors: packed = a layer's data-gradient pair of
    conv15h_pack_many; dymax = bn_bwd's dxmax for this dy (partial maxima of |dy|: the launch's power-of-two input scale; NaN
    entries are ignored, a +inf entry sets `flag`, an all-zero dymax gives exactly `add`, or +0)."""
    who = "conv3x3_dgrad_f16x2_dense"
    n, c_dy, c_dx = _conv15h_packed(who, dy, packed, add, "add")
    _check(dymax, "%s: dymax must be a contiguous float32 device tensor" % who)
    if int(dymax.numel()) < 1:
        raise ValueError("%s: dymax is empty" % who)
    L, hnd, stream = _ctx(dy, (15, 15))
    flag = _flag_word(flag, who, dy)
    dx = _empty((n, c_dx, 15, 15), dy)
    _ck(L, L.apz_conv15h_dgrad(hnd, dy.data_ptr(), packed[0].data_ptr(), packed[1].data_ptr(), _ptr(add), dx.data_ptr(), n, c_dy,
                               c_dx, dymax.data_ptr(), int(dymax.numel()), flag.data_ptr(), stream))
    return dx


def _conv3x3_run(x, weight, bias, layout, flip, resid, relu, upk=None):
    """conv(x, W) (flip: the data-gradient convolution with W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]) + bias + resid.
    upk: the layer's transformed weights in that orientation when the caller packed them already (wino_pack_many)."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    co, ci = int(weight.shape[0]), int(weight.shape[1])
    cin_p, cout_p = (co, ci) if flip else (ci, co)
    n = int(x.shape[0])
    if int(x.shape[1]) != cin_p:
        raise ValueError("channel mismatch")
    if relu and resid is not None and layout != ROWS16:     # (a dense residual is added by a launch of its own: add_)
        raise ValueError("relu after a dense residual is not provided")
    y = _empty((n, cout_p) + tuple(x.shape[2:]), x)
    # the Winograd kernel works on board pairs x channel halves: from 192 boards on it fills the chip and beats the
    # direct kernel (measured round 1: 24.2 vs 31.0 ms per training step at batch 512, 12.3 vs 11.8 ms at 128);
    # padded-row tensors are its native layout and always take it
    if is_trunk_shape(weight, x, layout) and (layout == ROWS16 or n >= 192):
        if upk is None:
            upk = _empty((L.apz_wino_packed_size(),), x)
            _ck(L, L.apz_wino_pack(hnd, weight.data_ptr(), int(flip), upk.data_ptr(), stream))
        if resid is not None and layout != ROWS16:
            _ck(L, L.apz_wino_conv_add(hnd, x.data_ptr(), upk.data_ptr(), _ptr(bias), None, y.data_ptr(), n, 0, layout, stream))
            add_(y, resid)
        else:
            _ck(L, L.apz_wino_conv_add(hnd, x.data_ptr(), upk.data_ptr(), _ptr(bias), _ptr(resid), y.data_ptr(), n, int(relu),
                                       layout, stream))
        return y
    if layout != DENSE:
        raise ValueError("padded-row layout: the 128 -> 128 trunk shape only")
    wpk = _empty((L.apz_conv3x3_packed_size(cin_p, cout_p),), x)
    _ck(L, L.apz_conv3x3_pack(hnd, weight.data_ptr(), ci, co, int(flip), wpk.data_ptr(), stream))
    _ck(L, L.apz_conv3x3_fwd(hnd, x.data_ptr(), wpk.data_ptr(), _ptr(bias), y.data_ptr(), n, cin_p, cout_p,
                             int(relu and resid is None), stream))
    if resid is not None:
        add_(y, resid)
    return y


def conv3x3_fwd(x, weight, bias=None, layout=DENSE, relu=False, upk=None):
    """y = conv2d(x, weight, bias, padding=1).  Dense: boards 15x15 or 8x8, C_out in {64, 128, 256}."""
    return _conv3x3_run(x, weight, bias, layout, False, None, relu, upk)


def conv3x3_fwd_stats(x, weight, bias, upk=None):
    """The trunk shape in the padded-row layout, for a BatchNorm that follows: -> (y, stats); stats [128][n][2] float64 =
    per (channel, board) the sum and the sum of squares of y, taken in the convolution's epilogue (bn_fwd(stats=...)
    then makes no pass of its own over y for them)."""
    L, hnd, stream = _ctx(x, _board(x, ROWS16))
    if not is_trunk_shape(weight, x, ROWS16):
        raise ValueError("conv3x3_fwd_stats: the 128 -> 128 trunk shape in the padded-row layout")
    n = int(x.shape[0])
    if upk is None:
        upk = _empty((L.apz_wino_packed_size(),), x)
        _ck(L, L.apz_wino_pack(hnd, weight.data_ptr(), 0, upk.data_ptr(), stream))
    y = _empty(tuple(x.shape), x)
    stats = _torch().empty((128, n, 2), dtype=_torch().float64, device=x.device)
    _ck(L, L.apz_wino_conv_stats(hnd, x.data_ptr(), upk.data_ptr(), _ptr(bias), y.data_ptr(), stats.data_ptr(), n, stream))
    return y, stats


def conv3x3_dgrad(dy, weight, layout=DENSE, add=None, upk=None):
    """dx = conv2d_input(dy, weight) (+ add: another gradient of the same tensor, e.g. the skip connection's).
    Needs C_in in {64, 128, 256} (the first layer's input gradient is never wanted)."""
    return _conv3x3_run(dy, weight, None, layout, True, add, False, upk)


def conv3x3_wgrad(x, dy, layout=DENSE):
    """dw [C_out][C_in][3][3] = sum over boards of x (*) dy."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, ci, co = int(x.shape[0]), int(x.shape[1]), int(dy.shape[1])
    dw = _empty((co, ci, 3, 3), x)
    # through the Winograd domain (3.6x fewer MFMAs; wgrad_wino3_kernel beats the direct kernel from 8 boards on: 14 against
    # 35 us at 8 boards, 22 against 48 at 32 -- round 3's kernel needed 64 boards to cover its per-slice partial sums)
    if layout == ROWS16 and (ci, co) == (128, 128):
        _ck(L, L.apz_wgrad_wino(hnd, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), n, stream))
    else:
        _ck(L, L.apz_conv3x3_wgrad(hnd, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), n, ci, co, layout, stream))
    return dw


def bias_grad(dy, layout=DENSE):
    """db[c] = sum over boards and cells of dy (pad cells of a padded-row gradient are zero)."""
    L, hnd, stream = _ctx(dy, _board(dy, layout))
    db = _empty((int(dy.shape[1]),), dy)
    _ck(L, L.apz_bias_grad(hnd, dy.data_ptr(), db.data_ptr(), int(dy.shape[0]), int(dy.shape[1]), layout, stream))
    return db


def add_(y, x):
    """y += x"""
    L, hnd, stream = _ctx(y, _board(y, DENSE if y.shape[3] != 16 else ROWS16))
    if y.shape != x.shape:
        raise ValueError("shape mismatch")
    _ck(L, L.apz_add(hnd, y.data_ptr(), x.data_ptr(), y.numel(), stream))
    return y


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
def _frame_side(side, layout, stats=None):
    """The `side` argument of the framed BatchNorm operators, checked before the library sees it"""
    side = int(side)
    if layout != ROWS16 or stats is not None:
        raise ValueError("side: padded-row tensors only, and no statistics from a convolution's epilogue (they cover all 225 cells)")
    return side


def bn_fwd(x, gamma, beta, run_mean, run_var, resid=None, relu=True, layout=DENSE, momentum=0.1, eps=1e-3, stats=None,
           want_mask=False, side=None):
    """y = act(batch_norm(x) (+ resid)) with batch statistics; gamma None = fixed at 1 (the reference's fix_gamma layers).
    run_mean / run_var are updated in place (momentum = weight of the new batch value).  -> (y, mean, invstd)
    stats: conv3x3_fwd_stats' second result for this x.  want_mask (padded rows): -> (y, mean, invstd, mask), mask = the
    ReLU decisions as uint8 [n][C][60] (4 bits per byte), for bn_bwd(mask=...).
    side (padded rows; None: the 15x15 board): the framed board's side S (csrc/bn_frame.h) -- statistics over the S x S
    window only (count n S S), whatever the off-board cells of x and resid hold; off-board y exactly +0, mask bits 0."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, c = int(x.shape[0]), int(x.shape[1])
    y = _empty(tuple(x.shape), x)
    mean, invstd = _empty((c,), x), _empty((c,), x)
    if stats is not None and (tuple(stats.shape) != (c, n, 2) or stats.dtype != _torch().float64 or not stats.is_contiguous()):
        raise ValueError("stats: contiguous float64 [C][n][2]")
    mask = _torch().empty((n, c, 60), dtype=_torch().uint8, device=x.device) if want_mask else None
    if side is not None:
        _ck(L, L.apz_bn_fwd_frame(hnd, x.data_ptr(), _ptr(resid), _ptr(gamma), beta.data_ptr(), _ptr(run_mean), _ptr(run_var),
                                  y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(mask), n, c, layout, int(relu), momentum,
                                  eps, _frame_side(side, layout, stats), stream))
    else:
        _ck(L, L.apz_bn_fwd_stats(hnd, x.data_ptr(), _ptr(resid), _ptr(gamma), beta.data_ptr(), _ptr(run_mean), _ptr(run_var),
                                  y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(stats), _ptr(mask), n, c, layout,
                                  int(relu), momentum, eps, stream))
    return (y, mean, invstd, mask) if want_mask else (y, mean, invstd)


def bn_bwd(dy, x, y, gamma, mean, invstd, relu=True, want_dres=False, layout=DENSE, dxsum=None, mask=None, dxmax=None,
           side=None):
    """-> (dx, dres or None, dgamma, dbeta); y is the forward output (the ReLU mask) -- or None when mask (bn_fwd's
    want_mask result) carries the ReLU decisions.
    dxsum: a [bn_bwd_splits(x, layout)][C] view (row stride >= C) of a float32 matrix that receives the per-split column
    sums of dx -- colsum() of it is the bias gradient of the convolution in front (bias_parts() hands such views out).
    dxmax (padded rows, or dense 15x15 tensors): a contiguous float32 [bn_bwd_splits(x, layout)][C] tensor that receives max |dx| per split and
    channel (the dymax of conv3x3_dgrad_f16x2 / conv3x3_dgrad_f16x2_dense); without it: the same dx, sums and bits.
    side (padded rows; None: the 15x15 board): the framed board's side, as in bn_fwd -- off-board dy and x may hold
    anything; off-board dx and dres are exactly +0."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, c = int(x.shape[0]), int(x.shape[1])
    dx = _empty(tuple(x.shape), x)
    dres = _empty(tuple(x.shape), x) if want_dres else None
    dgamma, dbeta = _empty((c,), x), _empty((c,), x)
    ld = 0
    if dxsum is not None:
        if tuple(dxsum.shape) != (bn_bwd_splits(x, layout), c) or dxsum.stride(1) != 1:
            raise ValueError("dxsum: a [splits][C] view with unit column stride")
        ld = int(dxsum.stride(0))
    if mask is not None and (tuple(mask.shape) != (n, c, 60) or mask.dtype != _torch().uint8 or not mask.is_contiguous()):
        raise ValueError("mask: contiguous uint8 [n][C][60]")
    if dxmax is not None and (tuple(dxmax.shape) != (bn_bwd_splits(x, layout), c) or not dxmax.is_contiguous() or
                              dxmax.dtype != _torch().float32):
        raise ValueError("dxmax: a contiguous float32 [splits][C] tensor")
    if side is not None:
        _ck(L, L.apz_bn_bwd_frame(hnd, dy.data_ptr(), x.data_ptr(), _ptr(y), _ptr(mask), _ptr(gamma), mean.data_ptr(),
                                  invstd.data_ptr(), dx.data_ptr(), _ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dxsum), ld,
                                  _ptr(dxmax), n, c, layout, int(relu), _frame_side(side, layout), stream))
    else:
        _ck(L, L.apz_bn_bwd_max(hnd, dy.data_ptr(), x.data_ptr(), _ptr(y), _ptr(mask), _ptr(gamma), mean.data_ptr(),
                                invstd.data_ptr(), dx.data_ptr(), _ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dxsum), ld,
                                _ptr(dxmax), n, c, layout, int(relu), stream))
    return dx, dres, dgamma, dbeta


def bn_bwd_splits(x, layout=DENSE, side=None):
    """rows of bn_bwd's dxsum matrix for tensors of x's shape (side: as in bn_bwd -- the framed kernels keep the grid)"""
    if side is not None:
        _frame_side(side, layout)
    L, hnd, _ = _ctx(x, _board(x, layout))
    s = L.apz_bn_bwd_splits(hnd, int(x.shape[0]), int(x.shape[1]), layout)
    _ck(L, s)
    return int(s)


def colsum(m, scale=1.0):
    """out[j] = scale * sum_i m[i][j] (fixed order, double accumulation); m: contiguous [rows][cols] float32"""
    if m.dim() != 2:
        raise ValueError("colsum takes a contiguous float32 device matrix")
    _check(m, "colsum takes a contiguous float32 device matrix")
    L, hnd, stream = _ctx(m)
    out = _empty((int(m.shape[1]),), m)
    _ck(L, L.apz_colsum(hnd, m.data_ptr(), out.data_ptr(), int(m.shape[0]), int(m.shape[1]), scale, stream))
    return out


# ---- heads ----------------------------------------------------------------------------------------------------------
def conv1x1_fwd(x, weight, bias=None, layout=DENSE, side=None):
    """y [n][CO][H][W] (dense) = W x + b, CO <= 8.  side (padded rows): the framed board's side S -- y [n][CO][S][S] from
    the S x S window of x, whatever its off-board cells hold."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, c, co = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
    if side is not None:
        side = _frame_side(side, layout)
        y = _empty((n, co, side, side), x)
        _ck(L, L.apz_conv1x1_fwd_frame(hnd, x.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), n, c, co, side, stream))
        return y
    h, w = int(x.shape[2]), (15 if layout == ROWS16 else int(x.shape[3]))
    y = _empty((n, co, h, w), x)
    _ck(L, L.apz_conv1x1_fwd(hnd, x.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), n, c, co, layout, stream))
    return y


def conv1x1_bwd(x, weight, dy, layout=DENSE, dx=None):
    """-> (dx, dw, db).  dx given: the gradient is ADDED to it (the second head); else a new tensor in x's layout."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, c, co = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
    acc = dx is not None
    if dx is None:
        dx = _empty(tuple(x.shape), x)
    dw, db = _empty(tuple(weight.shape), x), _empty((co,), x)
    _ck(L, L.apz_conv1x1_bwd(hnd, x.data_ptr(), weight.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                             n, c, co, layout, int(acc), stream))
    return dx, dw, db


def conv1x1_bwd_pair(x, w1, dy1, w2, dy2, layout=DENSE, side=None):
    """Two 1x1 convolutions of the same input (the two heads): -> (dx, dw1, db1, dw2, db2), dx = both heads' input
    gradients added, in one pass over x.  side (padded rows): the framed board's side S, dy1 / dy2 dense [n][CO][S][S];
    rows S .. 14 of dx are NOT written (bn_bwd(side=S), which reads dx next, masks them)."""
    L, hnd, stream = _ctx(x, _board(x, layout))
    n, c, co1, co2 = int(x.shape[0]), int(x.shape[1]), int(w1.shape[0]), int(w2.shape[0])
    dx = _empty(tuple(x.shape), x)
    dw = _empty((co1 + co2, c), x)
    if side is not None:
        side = _frame_side(side, layout)
        for dy, co in ((dy1, co1), (dy2, co2)):
            _check(dy, "conv1x1_bwd_pair: dy dense [n][CO][side][side]", None, (n, co, side, side))
        _ck(L, L.apz_conv1x1_bwd2_frame(hnd, x.data_ptr(), w1.data_ptr(), dy1.data_ptr(), co1, w2.data_ptr(), dy2.data_ptr(), co2,
                                        dx.data_ptr(), dw.data_ptr(), n, c, side, 0, stream))
    else:
        _ck(L, L.apz_conv1x1_bwd2(hnd, x.data_ptr(), w1.data_ptr(), dy1.data_ptr(), co1, w2.data_ptr(), dy2.data_ptr(), co2,
                                   dx.data_ptr(), dw.data_ptr(), n, c, layout, 0, stream))
    return dx, dw[:co1].view(w1.shape), bias_grad(dy1, DENSE), dw[co1:].view(w2.shape), bias_grad(dy2, DENSE)


def fc_fwd(x, weight, bias=None):
    """y [n][N] = x [n][K] W[N][K]^T + b"""
    L, hnd, stream = _ctx(x)
    n, k, nn = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
    y = _empty((n, nn), x)
    _ck(L, L.apz_fc_fwd(hnd, x.data_ptr(), weight.data_ptr(), _ptr(bias), y.data_ptr(), n, k, nn, stream))
    return y


def fc_bwd(x, weight, dy):
    """-> (dx, dw, db)"""
    L, hnd, stream = _ctx(x)
    n, k, nn = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
    dx, dw, db = _empty((n, k), x), _empty((nn, k), x), _empty((nn,), x)
    _ck(L, L.apz_fc_bwd(hnd, x.data_ptr(), weight.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                        n, k, nn, stream))
    return dx, dw, db


def dropout(x, keep, seed, step):
    """y = x * mask / keep, mask = [hash(seed, step, element) < keep]; the same call on dy is the backward pass."""
    L, hnd, stream = _ctx(x)
    y = _empty(tuple(x.shape), x)
    _ck(L, L.apz_dropout(hnd, x.data_ptr(), y.data_ptr(), x.numel(), keep, seed, step, stream))
    return y


def pv_loss(logits, vlogit, pi=None, z=None, grads=True, outputs=False, loss3=None, occ=None):
    """The reference's loss head (policy_value_net_mxnet.py:180-193) on [n][H*W] logits and [n] value logits.
    -> dict with loss3 = (value loss, policy loss, entropy) [device, 3 floats], dlogits, dvlogit (grads),
    probs, values (outputs).  loss3: a contiguous float32 device tensor of 3 to write the losses into.
    occ (default None: the reference's softmax over all cells): a contiguous uint8 device tensor [n][H*W] in move order,
    non-zero where the move is occupied (occupancy_planes) -- softmax, cross-entropy and entropy then run over the empty
    cells only and probs / dlogits are exactly +0 on the occupied ones (apz_pv_loss_legal)."""
    n, hw = int(logits.shape[0]), int(logits.shape[1])
    side = int(round(hw ** 0.5))
    L, hnd, stream = _ctx(logits, (side, side))
    out = {}
    if pi is not None:
        out["loss3"] = _empty((3,), logits) if loss3 is None else loss3
        if grads:
            out["dlogits"], out["dvlogit"] = _empty((n, hw), logits), _empty((n,), logits)
    if outputs:
        out["probs"], out["values"] = _empty((n, hw), logits), _empty((n,), logits)
    outs = [_ptr(out.get(k)) for k in ("loss3", "dlogits", "dvlogit", "probs", "values")]
    if occ is None:
        _ck(L, L.apz_pv_loss(hnd, logits.data_ptr(), vlogit.data_ptr(), _ptr(pi), _ptr(z), n, *outs, stream))
    else:
        if occ.device != logits.device:
            raise ValueError("occ: a contiguous uint8 tensor [%d][%d] on the device of logits" % (n, hw))
        _check(occ, "occ: a contiguous uint8 tensor [%d][%d] on the device of logits" % (n, hw), _torch().uint8, (n, hw))
        _ck(L, L.apz_pv_loss_legal(hnd, logits.data_ptr(), vlogit.data_ptr(), _ptr(pi), _ptr(z), occ.data_ptr(), n, *outs, stream))
    return out


def occupancy_planes(planes):
    """planes [n][c_in][H][W] (c_in 9 or 4, top row first: Board.current_state) -> uint8 [n][H*W] in move order (m = h*W + w,
    bottom row first, the order of pi): 1 where the "all own stones" or the "all opponent stones" plane is non-zero at the
    move's cell (apz_occupancy_planes)."""
    torch = _torch()
    if planes.dim() != 4 or int(planes.shape[1]) not in (9, 4):
        raise ValueError("occupancy_planes takes [n][9 or 4][H][W]")
    L, hnd, stream = _ctx(planes)
    n, c_in, h, w = (int(v) for v in planes.shape)
    occ = torch.empty((n, h * w), dtype=torch.uint8, device=planes.device)
    _ck(L, L.apz_occupancy_planes(hnd, planes.data_ptr(), n, c_in, h, w, occ.data_ptr(), stream))
    return occ


# ---- layout ---------------------------------------------------------------------------------------------------------
def to_rows16(x):
    """dense [n][C][15][15] -> padded rows [n][C][15][16] (pad column zero)"""
    L, hnd, stream = _ctx(x, _board(x, DENSE))
    y = _empty((int(x.shape[0]), int(x.shape[1]), 15, 16), x)
    _ck(L, L.apz_layout_convert(hnd, x.data_ptr(), y.data_ptr(), int(x.shape[0]) * int(x.shape[1]), 1, stream))
    return y


def frame_planes(x):
    """dense [n][C][S][S] (S = 6, 7, 9, 11 .. 14) -> dense [n][C][15][15]: the board in the top-left window of the 15x15
    frame, every off-board cell zero (csrc/frame15.h)"""
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError("frame_planes takes [n][C][S][S]")
    L, hnd, stream = _ctx(x, (15, 15))
    y = _empty((int(x.shape[0]), int(x.shape[1]), 15, 15), x)
    _ck(L, L.apz_frame_planes_dev(hnd, x.data_ptr(), y.data_ptr(), int(x.shape[0]) * int(x.shape[1]), int(x.shape[2]), stream))
    return y


def from_rows16(x):
    L, hnd, stream = _ctx(x, _board(x, ROWS16))
    y = _empty((int(x.shape[0]), int(x.shape[1]), 15, 15), x)
    _ck(L, L.apz_layout_convert(hnd, x.data_ptr(), y.data_ptr(), int(x.shape[0]) * int(x.shape[1]), 0, stream))
    return y


# ---- device replay buffer -------------------------------------------------------------------------------------------
def replay_gather(codes, pi, z, entries, height, width, n_planes=9):
    """The mini-batch of a device replay ring (apz_replay_gather, csrc/replay.h).  codes u8 [cap][code stride], pi f32
    [cap][HW], z f32 [cap]: contiguous device tensors; entries: k entry words slot * 8 + symmetry (any integer sequence).
    -> (states [k][n_planes][H][W], pis [k][HW], zs [k]) on the same device, queued on torch's current stream.  Entries
    outside [0, 8 * cap) raise ValueError here, before the library is called."""
    import numpy as np
    torch = _torch()
    h, w, n_planes = int(height), int(width), int(n_planes)
    hw = h * w
    stride = (hw + 1 + 15) // 16 * 16
    if h != w:
        raise ValueError("replay_gather rotates boards: it needs a square board")
    if n_planes not in (9, 4):
        raise ValueError("n_planes must be 9 or 4")
    cap = int(codes.shape[0])
    _check(codes, "codes: a contiguous uint8 device tensor [cap][%d]" % stride, torch.uint8, (cap, stride))
    for t, shape, what in ((pi, (cap, hw), "pi"), (z, (cap,), "z")):
        msg = "%s: a contiguous float32 tensor %s on the device of codes" % (what, list(shape))
        if t.device != codes.device:
            raise ValueError(msg)
        _check(t, msg, None, shape)
    ent = np.asarray(entries).reshape(-1)
    if ent.size and not np.issubdtype(ent.dtype, np.integer):
        raise ValueError("entries must be integers")
    if ent.size and (int(ent.min()) < 0 or int(ent.max()) >= 8 * cap):
        raise ValueError("replay_gather: entries must lie in [0, 8 * capacity = %d), got %d ... %d" %
                         (8 * cap, int(ent.min()), int(ent.max())))
    ent = np.ascontiguousarray(ent, dtype=np.int32)
    k = int(ent.size)
    states = torch.empty((k, n_planes, h, w), dtype=torch.float32, device=codes.device)
    pis, zs = _empty((k, hw), states), _empty((k,), states)
    if k == 0:
        return states, pis, zs
    L, hnd, stream = _ctx(codes.device, (h, w))
    _ck(L, L.apz_replay_gather(hnd, codes.data_ptr(), pi.data_ptr(), z.data_ptr(), cap, _native.as_ptr(ent, C.c_int32), k,
                               n_planes, states.data_ptr(), pis.data_ptr(), zs.data_ptr(), stream))
    return states, pis, zs


# ---- Adam -----------------------------------------------------------------------------------------------------------
def adam_step(entries, lr_t, b1, b2, eps, rescale, device, skip=None):
    """One launch over all tensors.  entries: [(w, grad, m, v, wd)] of float32 device tensors (apz_adam_step).  skip: a
    device int32 word; when it is not zero at the time the launch runs, nothing is updated (apz_adam_step_unless)."""
    tab = _adam_table(entries)
    L, hnd, stream = _ctx(device)
    _ck(L, L.apz_adam_step_unless(hnd, tab.ctypes.data_as(C.c_void_p), len(tab), lr_t, b1, b2, eps, rescale, _ptr(skip), stream))


def _adam_table(entries):
    """[(w, grad, m, v, wd)] -> the host table of apz_adam_step (48-byte entries)"""
    import numpy as np
    tab = np.zeros(len(entries), dtype=[("w", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("n", "i8"), ("wd", "f4"),
                                        ("pad", "i4")])
    for i, (w, g, m, v, wd) in enumerate(entries):
        if g.shape != w.shape or not g.is_contiguous():
            raise ValueError("gradient %d: shape / layout mismatch" % i)
        tab[i] = (w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), wd, 0)
    return tab


def ema_update(entries, c, device, skip=None, skip2=None):
    """The averaged weights' step, one launch over all tensors (apz_ema_update; csrc/ema.h): entries [(shadow, weight)] of
    float32 device tensors, shadow = shadow + c * (weight - shadow) in three separately rounded float32 operations.  skip /
    skip2: device int32 words; when either is not zero at the time the launch runs, nothing is written.  entries may also be
    the table ema_table(entries) returned: a caller whose tensors stay where they are (HipTrainer) builds it once."""
    import numpy as np
    if isinstance(entries, np.ndarray):
        tab = entries
        if tab.dtype != _EMA_ENTRY or tab.ndim != 1 or not tab.flags.c_contiguous:
            raise ValueError("ema_update takes [(shadow, weight)] or the table ema_table() built, not an array of dtype %s" % tab.dtype)
    else:
        tab = ema_table(entries)
    L, hnd, stream = _ctx(device)
    _ck(L, L.apz_ema_update(hnd, tab.ctypes.data_as(C.c_void_p), len(tab), float(c), _ptr(skip), _ptr(skip2), stream))


_EMA_ENTRY = [("s", "u8"), ("w", "u8"), ("n", "i8")]     # apz_ema_update's 24-byte entry


def ema_table(entries):
    """[(shadow, weight)] -> the host table of apz_ema_update (24-byte entries), shapes and layouts checked.  It holds
    addresses: the tensors must stay alive and in place for as long as it is used."""
    import numpy as np
    tab = np.zeros(len(entries), dtype=_EMA_ENTRY)
    f32 = _torch().float32
    for i, (s, w) in enumerate(entries):
        if not (s.is_cuda and w.is_cuda and s.dtype == f32 and w.dtype == f32):
            raise ValueError("shadow %d: float32 device tensors" % i)
        if s.shape != w.shape or not s.is_contiguous() or not w.is_contiguous():
            raise ValueError("shadow %d: shape / layout mismatch" % i)
        tab[i] = (s.data_ptr(), w.data_ptr(), w.numel())
    return tab


# why bits of the guard record (csrc/grad_guard.h)
GUARD_GRAD, GUARD_LOSS, GUARD_SKIP_IN, GUARD_NORM = 1, 2, 4, 8


def _guard_record(record, device):
    torch = _torch()
    if record is None:
        return torch.zeros((4,), dtype=torch.float32, device=device)
    _check(record, "record: a contiguous float32 device tensor of 4 elements", None, (4,))
    if record.data_ptr() % 16:
        raise ValueError("record: 16-byte aligned storage")
    return record


def grad_norm(entries, rescale, clip, device, loss3=None, skip=None, record=None):
    """The global norm of the gradients in entries ([(w, grad, m, v, wd)] as adam_step takes them; only grad is read), two
    launches (apz_grad_norm) -> record, a float32 device tensor of 4 words {norm, rescale_eff, skip, why} (the last two are
    uint32: record.view(torch.int32)); read_guard_record() brings it to the host.  norm = sqrt(sum grad^2) * rescale; clip
    (None or <= 0: off): the norm above which rescale_eff = rescale * clip / norm; loss3: three device floats, skip: a device
    int32 word -- a non-finite gradient element (why bit 1), a non-finite loss3 (2), a skip word that is not zero (4) or a norm
    beyond float32 under clipping (8) set skip.  record: such a tensor to fill (16-byte aligned), else a new one."""
    tab = _adam_table(entries)
    L, hnd, stream = _ctx(device)
    record = _guard_record(record, device)
    _ck(L, L.apz_grad_norm(hnd, tab.ctypes.data_as(C.c_void_p), len(tab), rescale, clip or 0.0, _ptr(loss3), _ptr(skip),
                           record.data_ptr(), stream))
    return record


def adam_step_guarded(entries, lr_t, b1, b2, eps, rescale, clip, device, loss3=None, skip=None, record=None):
    """grad_norm's two launches and then adam_step with the record's rescale_eff in place of rescale, skipped on the device
    when the record says skip (apz_adam_step_guarded) -> record.  Without a clip and without a skip: adam_step's bits."""
    tab = _adam_table(entries)
    L, hnd, stream = _ctx(device)
    record = _guard_record(record, device)
    _ck(L, L.apz_adam_step_guarded(hnd, tab.ctypes.data_as(C.c_void_p), len(tab), lr_t, b1, b2, eps, rescale, clip or 0.0,
                                   _ptr(loss3), _ptr(skip), record.data_ptr(), stream))
    return record


def read_guard_record(words):
    """Four float32 words as a host array (a record copied back) -> (norm, rescale_eff, skip, why)"""
    import numpy as np
    w = np.ascontiguousarray(words, dtype=np.float32).reshape(4)
    u = w.view(np.uint32)
    return float(w[0]), np.float32(w[1]), bool(u[2]), int(u[3])


def guard_reason(why):
    """The why bits in words"""
    names = ((GUARD_GRAD, "non-finite gradient"), (GUARD_LOSS, "non-finite loss"), (GUARD_SKIP_IN, "f16x2 overflow"),
             (GUARD_NORM, "gradient norm beyond float32"))
    return ", ".join(n for b, n in names if why & b) or None
