"""The error envelopes of everything behind the trunk: the inference softmax / tanh (head_softmax_value_kernel on 15x15
boards, head8_kernel on 8x8 boards; head_fc_kernel<1>'s fused tail has the split kernel's form), the training loss
(pv_loss_kernel) and the pi half of the GPU root sampler (root_sample_kernel), at saturated inputs.

This module holds the bars as functions of the inputs, a numpy float32 restatement of each kernel's operation order, the
input builders, and CPU tests that every restatement stays inside its bar against float64 with at least 4x room
(ROOM).  tests/test_gpu_loss_edges.py, tests/test_gpu_head_edges.py and tests/test_gpu_sampler.py assert the same bars of
the kernels.

Units: u = 2^-24, the unit roundoff of float32 (one rounding moves a value by at most u relative).  The device expf,
logf, log1pf and tanhf are taken as 2 ulp = 4 u relative (FN): the HIP documentation that ships with the toolkit gives no
figures, so this is an assumption, and the 4x room of the restatement (numpy's functions are within 1 ulp) is what absorbs
the difference.  The library is built with -ffp-contract=off (alphapig_amd/build.py): a * b + c rounds twice on the
device as it does in the restatements.

The bounds below are first-order (products of two errors dropped), derived once from the order of operations.  Where one
rounding dominates, the restatement attains most of such a bound (lp = t - logs at |lp| = 20 is rounded by up to 16 u of
the 20 u it is allowed), so a BAR is ROOM = 4 times its bound: that factor is the room the restatement must keep, and it
is what the device functions get on top of FN.

softmax tail (l: the float32 logits, t_j = l_j - max l, p = softmax(l), H = sum_k p_k |t_k|):
    t_j          one rounding                                            u |t_j|          (absolute)
    e_j = expf   argument error + the function                           u |t_j| + FN u   (relative)
    s = sum e    <= 3 additions in the lane + 6 in the shuffle tree, all terms positive; the e_k's own errors weigh
                 in with p_k                                             9 u + u (H + FN) (relative)
    p_j = e_j * (1 / s)   two roundings (head8_kernel: e_j / s, one)     2 u
  => |d p_j| <= u p_j (|t_j| + H + 2 FN + 11)   (+ TINY: results below 2^-126 may be flushed)
  and |sum_j p_j - 1| <= sum_j of that.
tanh:  |d v| <= FN u |v| (+ TINY).

pv_loss_kernel (lp_j = (l_j - m) - logf(s), logs = log s):
    logs         the relative error of s + the function                  u (9 + H + FN) + FN u |logs|   (absolute)
    lp_j         t_j's rounding, logs, one rounding                      u LAM_j,  LAM_j = |t_j| + |lp_j| + 9 + H + FN + FN |logs|
    p_j = expf(lp_j)                                                     u p_j (LAM_j + FN)
    ce  = -sum pi_j lp_j   product + <= 9 additions                      u sum_j pi_j (LAM_j + 10 |lp_j|)
    ent = -sum p_j lp_j                                                  u sum_j p_j (|lp_j| (LAM_j + FN + 10) + LAM_j)
    v = tanhf(u'), d = z - v, d * d                                      u (2 |d| FN |v| + 3 d^2)
    loss3        double sum over the samples, * (float) 1/n, rounded     mean of the terms' bars + 3 u |loss|
    dlogits_j = (p_j spi - pi_j) g,  spi = sum pi (9 additions), g = (float) 1/n
                                                                          g u (p_j spi (LAM_j + FN + 10) + 3 |p_j spi - pi_j|)
    dvlogit = 2 (v - z) (1 - v v) g: 1 - v v cancels, its absolute error is 2 |v| FN u |v| + u v^2 + u |1 - v^2|
                                                                          g u (2 |v - z| ((2 FN + 1) v^2 + |1 - v^2|) + 3 |dv / g|)
  Every bar is then cut at what the suite asked of the same quantity before (CAPS): no bar here is looser.

root_sample_kernel, pi (v: visit counts < 2^24, T = 1 / temp, y_k = T log(v_k / v_max) <= 0, pi_k = exp(y_k) / sum):
    v - v_max    exact in integers; (float) of it and of v_max exact
    L_k = log1pf((v - v_max) / v_max) for a ratio >= 1/2: the quotient's rounding moves L by u |d| / (1 + d) <= 2 u |L|;
          logf(v / v_max) below 1/2: the quotient's rounding moves L by u <= 1.45 u |L|;  the function: FN u |L|
    y_k = T L_k  one rounding, T = 1.0f / (float) temp: two more         u |y_k| (FN + 5)
    (the reference adds 1e-10 to both counts: T 1e-10 |1 / v_k - 1 / v_max|, carried in the bar; a child without visits
     beside a visited one is T (logf(1e-10f) - logf(v_max)), the same form)
    e_k = expf(y_k), s (3 + 6 additions), 1 / s, e_k * inv               as the softmax tail
  => |d pi_k| <= pi_k (u (W_k + FN + 11 + sum_j pi_j (W_j + FN)) + R_k + sum_j pi_j R_j),  W_k = |y_k| (FN + 5),
     cut at 1e-6, the figure csrc/sampler.h documents."""
import numpy as np
import pytest

U = 2.0 ** -24
FN = 4.0                      # device expf / logf / log1pf / tanhf: 2 ulp assumed (see above)
TINY = 2.0 ** -125            # flushed / denormal results
ROOM = 4.0                    # the restatements must be this far inside the bars
F32 = np.float32

# what the suite asked before this module: tests/test_gpu_train.py::test_policy_value_loss_head (1e-5 (1 + loss), 1e-6 on
# probs / values, 1e-4 max |grad| + 1e-6 on the gradients), tests/test_gpu_net.py (2e-5 on inference probs / values), and
# the sampler's documented 1e-6
CAP_LOSS_REL, CAP_LOSS_OUT, CAP_GRAD_REL, CAP_INFER, CAP_PI = 1e-5, 1e-6, 1e-4, 2e-5, 1e-6


# ---- the kernels' reductions ----------------------------------------------------------------------------------------
def wave_tree(lanes):
    """[..., 64] float32 -> what every lane holds after `for o in 32, 16, .. 1: v += shfl_xor(v, o)`"""
    s = np.asarray(lanes, dtype=F32)
    for half in (32, 16, 8, 4, 2, 1):
        s = s[..., :half] + s[..., half:2 * half]
    assert s.dtype == F32
    return s[..., 0]


def _pad256(x):
    out = np.zeros(x.shape[:-1] + (256,), dtype=F32)         # x + 0 is exact: absent cells do not change a lane's sum
    out[..., :x.shape[-1]] = x
    return out


def strided_lanes(x):
    """lane l adds the cells l, l + 64, l + 128, l + 192 in that order (pv_loss_kernel, the head kernels)"""
    q = _pad256(np.asarray(x, dtype=F32)).reshape(x.shape[:-1] + (4, 64))
    return ((q[..., 0, :] + q[..., 1, :]) + q[..., 2, :]) + q[..., 3, :]


def contiguous_lanes(x):
    """lane l adds the cells 4 l .. 4 l + 3 in that order (root_sample_kernel)"""
    q = _pad256(np.asarray(x, dtype=F32)).reshape(x.shape[:-1] + (64, 4))
    return ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]


# ---- float32 restatements -------------------------------------------------------------------------------------------
def softmax_tail_f32(logits, form):
    """form "mul": expf(l - m) * (1 / s)  (head_softmax_value_kernel, head_fc_kernel<1>);  "div": expf(l - m) / s
    (head8_kernel)"""
    l = np.asarray(logits, dtype=F32)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    s = wave_tree(strided_lanes(e))[:, None]
    p = e * (F32(1) / s) if form == "mul" else e / s
    assert p.dtype == F32
    return p


def tanh_f32(u):
    return np.tanh(np.asarray(u, dtype=F32))


def pv_loss_f32(logits, u, pi, z):
    """pv_loss_kernel + colsum_kernel -> dict like alphapig_amd.hipconv.pv_loss"""
    l, u, pi, z = (np.asarray(a, dtype=F32) for a in (logits, u, pi, z))
    n = l.shape[0]
    t = l - l.max(axis=1, keepdims=True)
    logs = np.log(wave_tree(strided_lanes(np.exp(t))))[:, None]
    lp = t - logs
    p = np.exp(lp)
    ce = -wave_tree(strided_lanes(pi * lp))
    ent = -wave_tree(strided_lanes(p * lp))
    spi = wave_tree(strided_lanes(pi))[:, None]
    g = F32(1) / F32(n)
    v = np.tanh(u)
    d = z - v
    terms = np.stack([d * d, ce, ent], axis=1)
    assert terms.dtype == F32 and p.dtype == F32
    return {"loss3": (terms.astype(np.float64).sum(axis=0) * np.float64(g)).astype(F32),
            "dlogits": (p * spi - pi) * g, "dvlogit": F32(2) * (v - z) * (F32(1) - v * v) * g, "probs": p, "values": v}


def sampler_pi_f32(visits, temp, form="log1p"):
    """the pi half of root_sample_kernel.  form "old": the kernel before the integer-maximum form,
    expf(T logf(v + 1e-10f) - max) (kept to show what the near-tie rows catch)"""
    v = np.asarray(visits, dtype=np.int64)
    has = v >= 0
    T = F32(1) / F32(temp)
    with np.errstate(divide="ignore", invalid="ignore"):
        if form == "old":
            x = np.where(has, T * np.log(v.astype(F32) + F32(1e-10)), F32(-np.inf)).astype(F32)
            e = np.where(has, np.exp(x - x.max(axis=1, keepdims=True)), F32(0)).astype(F32)
        else:
            vmax = v.max(axis=1, keepdims=True)
            fmax = vmax.astype(F32)
            d = (v - vmax).astype(F32) / fmax
            mid = T * np.where(d >= F32(-0.5), np.log1p(d), np.log(v.astype(F32) / fmax))
            unvisited = T * (np.log(F32(1e-10)) - np.log(fmax))
            xm = np.where((v > 0) & (v < vmax), mid, np.where((v == 0) & (vmax > 0), unvisited, F32(0))).astype(F32)
            e = np.where(has, np.exp(xm), F32(0)).astype(F32)
        s = wave_tree(contiguous_lanes(e))[:, None]
        pi = e * (F32(1) / s)
    pi[~has.any(axis=1)] = 0                      # a row without a child: pi = 0 (the kernel returns before the sum)
    assert pi.dtype == F32
    return pi


# ---- float64 references ---------------------------------------------------------------------------------------------
def softmax64(l):
    t = np.asarray(l, dtype=np.float64)
    t = t - t.max(axis=1, keepdims=True)
    e = np.exp(t)
    return e / e.sum(axis=1, keepdims=True), t


def pv_loss64(logits, u, pi, z):
    """float64 log_softmax / tanh and the analytic gradients of mean((z - v)^2) + mean(-sum pi log p) on the float32
    inputs (tests/test_gpu_loss_edges.py holds them against torch autograd once)"""
    l, u, pi, z = (np.asarray(a, dtype=np.float64) for a in (logits, u, pi, z))
    n = l.shape[0]
    t = l - l.max(axis=1, keepdims=True)
    logs = np.log(np.exp(t).sum(axis=1, keepdims=True))
    lp = t - logs
    p = np.exp(lp)
    v = np.tanh(u)
    # 1 - tanh^2 = sech^2 without the cancellation
    sech2 = 1.0 / np.cosh(np.minimum(np.abs(u), 300.0)) ** 2
    return {"loss3": np.array([((z - v) ** 2).mean(), (-(pi * lp).sum(axis=1)).mean(), (-(p * lp).sum(axis=1)).mean()]),
            "dlogits": (p * pi.sum(axis=1, keepdims=True) - pi) / n, "dvlogit": 2 * (v - z) * sech2 / n, "probs": p, "values": v,
            "t": t, "logs": logs, "lp": lp}


def sampler_pi64(visits, temp):
    """softmax(1 / temp * log(visits + 1e-10)) over the children (mcts_alphaZero.py:13-16, :152-155); rows without a child: 0"""
    v = np.asarray(visits, dtype=np.int64)
    out = np.zeros(v.shape)
    for i, row in enumerate(v):
        acts = np.flatnonzero(row >= 0)
        if len(acts):
            x = 1.0 / temp * np.log(row[acts].astype(np.float64) + 1e-10)
            e = np.exp(x - x.max())
            out[i, acts] = e / e.sum()
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------
def softmax_bar(logits):
    """-> (bar of every probability, bar of |row sum - 1|) for the inference softmax of these float32 logits"""
    p, t = softmax64(logits)
    H = (p * np.abs(t)).sum(axis=1, keepdims=True)
    bar = ROOM * U * p * (np.abs(t) + H + 2 * FN + 11) + TINY
    return np.minimum(bar, CAP_INFER), np.minimum(bar.sum(axis=1), CAP_INFER)


def tanh_bar(u, cap=CAP_INFER):
    return np.minimum(ROOM * FN * U * np.abs(np.tanh(np.asarray(u, dtype=np.float64))) + TINY, cap)


def pv_loss_bars(logits, u, pi, z):
    r = pv_loss64(logits, u, pi, z)
    pi, z = np.asarray(pi, dtype=np.float64), np.asarray(z, dtype=np.float64)
    n = pi.shape[0]
    t, lp, logs, p, v = np.abs(r["t"]), np.abs(r["lp"]), np.abs(r["logs"]), r["probs"], r["values"]
    H = (p * t).sum(axis=1, keepdims=True)
    lam = t + lp + 9 + H + FN + FN * logs
    d = np.abs(z - v)
    UR = ROOM * U
    terms = np.stack([UR * (2 * d * FN * np.abs(v) + 3 * d * d) + TINY,
                      UR * (pi * (lam + 10 * lp)).sum(axis=1),
                      UR * (p * (lp * (lam + FN + 10) + lam)).sum(axis=1)], axis=1)
    loss = terms.mean(axis=0) + 3 * UR * np.abs(r["loss3"])
    spi = pi.sum(axis=1, keepdims=True)
    dl = (UR * (p * spi * (lam + FN + 10) + 3 * np.abs(p * spi - pi)) + TINY) / n
    dv = (UR * (2 * d * ((2 * FN + 1) * v * v + np.abs(1 - v * v)) + 3 * n * np.abs(r["dvlogit"])) + TINY) / n
    return {"loss3": np.minimum(loss, CAP_LOSS_REL * (1 + np.abs(r["loss3"]))),
            "dlogits": np.minimum(dl, CAP_GRAD_REL * np.abs(r["dlogits"]).max() + 1e-6),
            "dvlogit": np.minimum(dv, CAP_GRAD_REL * np.abs(r["dvlogit"]).max() + 1e-6),
            "probs": np.minimum(UR * p * (lam + FN) + TINY, CAP_LOSS_OUT), "values": tanh_bar(u, CAP_LOSS_OUT)}, r


def sampler_pi_bar(visits, temp):
    v = np.asarray(visits, dtype=np.int64)
    assert v.max() < 2 ** 24                                   # the condition of the bar: counts convert exactly
    pi = sampler_pi64(v, temp)
    has = v >= 0
    vmax = np.maximum(v.max(axis=1, keepdims=True), 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(has & (v < vmax), 1.0 / temp * (np.log(v + 1e-10) - np.log(vmax + 1e-10)), 0.0)
        R = np.where(has & (v > 0) & (v < vmax), 1e-10 / temp * np.abs(1.0 / v - 1.0 / vmax), 0.0)
    W = np.abs(y) * (FN + 5)
    rel = ROOM * U * (W + FN + 11 + (pi * (W + FN)).sum(axis=1, keepdims=True)) + R + (pi * R).sum(axis=1, keepdims=True)
    return np.minimum(pi * rel + TINY * has, CAP_PI)


# ---- inputs ---------------------------------------------------------------------------------------------------------
LOGIT_FAMILIES = ("randn3", "randn30", "randn300", "randn3e4", "offset+1e4", "offset-1e4", "equal", "twomax")
TARGET_FAMILIES = ("dirichlet", "onehot_argmax", "onehot_underflow", "zero")
VALUE_LOGITS = (0.0, 1e-20, -1e-20, 0.5, -0.5, 9.0, -9.0, 20.0, -20.0, 88.0, -88.0)
OUTCOMES = (-1.0, 0.0, 1.0)
ONE_HOT_GAP = 104.0                 # exp(-104) < 2^-150: the float32 softmax of such a row is exactly one-hot


def logit_row(rs, family, hw):
    x = rs.standard_normal(hw)
    if family.startswith("randn"):
        return x * float(family[5:])
    if family.startswith("offset"):
        return x * 3 + float(family[6:])
    if family == "equal":
        return np.full(hw, 3.0 * x[0])
    a, b = rs.permutation(hw)[:2]                              # two equal maxima far above the rest
    x = x * 3
    x[[a, b]] = np.abs(x).max() + 200.0
    return x


def target_row(rs, family, logits32):
    hw = len(logits32)
    if family == "dirichlet":
        return rs.dirichlet(np.ones(hw) * 0.3)
    out = np.zeros(hw)
    if family == "onehot_argmax":
        out[int(np.argmax(logits32))] = 1.0
    elif family == "onehot_underflow":                         # the least likely cell: its probability is 0 in float32
        out[int(np.argmin(logits32))] = 1.0                    # wherever the row's spread exceeds ONE_HOT_GAP
    return out


def loss_batch(logit_family, target_family, n, hw, combo):
    """-> float32 (logits [n][hw], value logits [n], pi [n][hw], z [n]).  The rows 0, n // 2 and n - 1 are of the two named
    families, the others cycle through all of them; (value logit, outcome) pairs walk through all 33 combinations,
    starting at `combo`."""
    rs = np.random.RandomState(1000 * hw + 37 * n + combo)
    marked = {0, n // 2, n - 1}
    logits = np.empty((n, hw), dtype=F32)
    pi = np.empty((n, hw), dtype=F32)
    u = np.empty(n, dtype=F32)
    z = np.empty(n, dtype=F32)
    for i in range(n):
        lf = logit_family if i in marked else LOGIT_FAMILIES[(i + combo) % len(LOGIT_FAMILIES)]
        tf = target_family if i in marked else TARGET_FAMILIES[(i // 2 + combo) % len(TARGET_FAMILIES)]
        logits[i] = logit_row(rs, lf, hw)
        pi[i] = target_row(rs, tf, logits[i])
        k = (combo + i) % (len(VALUE_LOGITS) * len(OUTCOMES))   # 11 and 3 are coprime: k <-> (value logit, outcome)
        u[i] = VALUE_LOGITS[k % len(VALUE_LOGITS)]
        z[i] = OUTCOMES[k % len(OUTCOMES)]
    return logits, u, pi, z


def loss_combos():
    return [(c, lf, tf) for c, (lf, tf) in enumerate((lf, tf) for lf in LOGIT_FAMILIES for tf in TARGET_FAMILIES)]


def one_hot_batch(n, hw):
    """every row's float32 softmax is exactly one-hot (top-two gap > ONE_HOT_GAP): the entropy term must be exactly 0"""
    rs = np.random.RandomState(77 + n + hw)
    logits = (rs.standard_normal((n, hw)) * 3).astype(F32)
    logits[np.arange(n), rs.randint(0, hw, n)] += F32(400.0)
    top = np.sort(logits.astype(np.float64), axis=1)
    assert (top[:, -1] - top[:, -2] > ONE_HOT_GAP).all()
    pi = np.stack([target_row(rs, TARGET_FAMILIES[i % 4], logits[i]) for i in range(n)]).astype(F32)
    k = np.arange(n)
    return logits, np.array(VALUE_LOGITS, dtype=F32)[k % 11], pi, np.array(OUTCOMES, dtype=F32)[k % 3]


SAMPLER_TEMPS = (1e-3, 0.5, 1.0)
TABLE_ROWS = ((1600, 1599, 3), (800, 799, 798, 1), (399, 398), (100000, 99990, 5))   # two leaders one visit apart


def near_tie_rows(hw):
    """-> (names, visits int32 [rows][hw]): the near-tie rows and the degenerate ones, children scattered over the board
    with the first and the last cell among them"""
    rows = [("table %s" % (r,), r) for r in TABLE_ROWS]
    rows += [("five in a row", (1600, 1599, 1598, 1597, 1596)),
             ("all cells equal", (7,) * hw),
             ("unvisited children only", (0,) * 5),
             ("unvisited beside one visited", (0, 50, 0, 0)),
             ("unvisited beside one visit", (0, 1, 0)),
             ("single child", (13,)),
             ("single unvisited child", (0,)),
             ("counts to 1e6", (1000000, 999999, 999000, 500001, 500000, 499999, 1, 0))]
    v = np.full((len(rows), hw), -1, dtype=np.int32)
    for i, (_, counts) in enumerate(rows):
        k = len(counts)
        cells = np.arange(hw) if k == hw else np.unique(np.round(np.linspace(0, hw - 1, k)).astype(int))
        assert len(cells) == k
        v[i, cells] = counts
    return [name for name, _ in rows], v


def ratio(got, ref, bar):
    """worst |got - ref| / bar; a zero bar asks for the exact value"""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bar = np.broadcast_to(bar, e.shape)
    return float(np.max(np.where(e == 0, 0.0, e / np.maximum(bar, 1e-300)))) if e.size else 0.0


# ---- the restatements against float64, with room ----------------------------------------------------------------------
@pytest.mark.parametrize("hw", [225, 64])
@pytest.mark.parametrize("n", [1, 3, 5, 37])
def test_the_loss_restatement_stays_inside_its_bars(n, hw):
    worst = {}
    for combo, lf, tf in loss_combos():
        args = loss_batch(lf, tf, n, hw, combo)
        bars, ref = pv_loss_bars(*args)
        got = pv_loss_f32(*args)
        for k in bars:
            assert np.isfinite(got[k]).all(), (lf, tf, k)
            q = ratio(got[k], ref[k], bars[k])
            worst[(lf, k)] = max(worst.get((lf, k), 0.0), q)
            assert q * ROOM <= 1.0, (lf, tf, k, q)
        assert got["loss3"][2] >= 0 and (np.abs(got["values"]) <= 1).all()
        assert (got["dvlogit"][np.abs(got["values"]) == 1] == 0).all()
        zero = ~args[2].any(axis=1)
        assert (got["dlogits"][zero] == 0).all()
        # the caps are in force: nothing here is looser than what the suite asked before
        assert (bars["probs"] <= CAP_LOSS_OUT).all() and (bars["values"] <= CAP_LOSS_OUT).all()
        assert (bars["loss3"] <= CAP_LOSS_REL * (1 + np.abs(ref["loss3"]))).all()
    for lf in LOGIT_FAMILIES:
        print("n %d hw %d %-10s restatement / bar: %s" % (n, hw, lf, "  ".join(
            "%s %.3f" % (k, worst[(lf, k)]) for k in ("loss3", "dlogits", "dvlogit", "probs", "values"))))


@pytest.mark.parametrize("hw", [225, 64])
def test_one_hot_rows_have_exactly_zero_entropy_in_the_restatement(hw):
    args = one_hot_batch(37, hw)
    got = pv_loss_f32(*args)
    assert got["loss3"][2] == 0 and np.isfinite(got["loss3"]).all()
    assert ((got["probs"] == 1).sum(axis=1) == 1).all() and ((got["probs"] == 0).sum(axis=1) == hw - 1).all()


@pytest.mark.parametrize("form,hw", [("mul", 225), ("mul", 64), ("div", 64)])
def test_the_softmax_tail_restatement_stays_inside_its_bar(form, hw):
    for lf in LOGIT_FAMILIES:
        rs = np.random.RandomState(len(lf) + hw)
        logits = np.stack([logit_row(rs, lf, hw) for _ in range(37)]).astype(F32)
        bar, sum_bar = softmax_bar(logits)
        p = softmax_tail_f32(logits, form)
        q = ratio(p, softmax64(logits)[0], bar)
        qs = ratio(p.astype(np.float64).sum(axis=1), 1.0, sum_bar)
        print("%s hw %d %-10s restatement / bar: probs %.3f  row sum %.3f" % (form, hw, lf, q, qs))
        assert np.isfinite(p).all() and q * ROOM <= 1.0 and qs * ROOM <= 1.0, (lf, q, qs)
        assert (bar <= CAP_INFER).all()
    u = np.array(VALUE_LOGITS + (3.0, -7.5, 1e-3), dtype=F32)
    q = ratio(tanh_f32(u), np.tanh(u.astype(np.float64)), tanh_bar(u))
    assert q * ROOM <= 1.0, q


@pytest.mark.parametrize("hw", [225, 64])
@pytest.mark.parametrize("temp", SAMPLER_TEMPS)
def test_the_sampler_pi_restatement_stays_inside_its_bar(temp, hw):
    names, v = near_tie_rows(hw)
    rs = np.random.RandomState(hw)
    for _ in range(64):                                       # ordinary rows and rows of 1600 playouts as well
        k = int(rs.randint(1, hw + 1))
        row = np.full(hw, -1, dtype=np.int32)
        row[np.sort(rs.permutation(hw)[:k])] = rs.multinomial(rs.choice([399, 1600]), rs.dirichlet(np.ones(k) * 0.3))
        v = np.vstack([v, row[None]])
        names.append("multinomial")
    ref, bar = sampler_pi64(v, temp), sampler_pi_bar(v, temp)
    assert (bar <= CAP_PI).all()
    new, old = sampler_pi_f32(v, temp), sampler_pi_f32(v, temp, "old")
    for i, name in enumerate(names[:12]):
        print("temp %g hw %d %-32s error / bar: restatement %.3f (%.1e)  old form %.1f (%.1e)" % (
            temp, hw, name, ratio(new[i], ref[i], bar[i]), np.abs(new[i] - ref[i]).max(),
            ratio(old[i], ref[i], bar[i]), np.abs(old[i] - ref[i]).max()))
    assert ratio(new, ref, bar) * ROOM <= 1.0
    assert np.isfinite(new).all()
    single = (v >= 0).sum(axis=1) == 1
    assert (new[single].max(axis=1) == 1).all()
    if temp == 1e-3:                                          # what the near-tie rows are for: the form before misses the bar
        for i in range(len(TABLE_ROWS)):
            assert ratio(old[i], ref[i], bar[i]) > 5.0, names[i]


def test_a_row_without_a_child_is_all_zero_in_the_restatement():
    v = np.full((3, 225), -1, dtype=np.int32)
    v[0, 5], v[2, 7:9] = 4, (3, 1)
    pi = sampler_pi_f32(v, 1.0)
    assert np.isfinite(pi).all() and not pi[1].any()
    np.testing.assert_allclose(pi[[0, 2]], sampler_pi64(v, 1.0)[[0, 2]], rtol=0, atol=CAP_PI)
