"""The error envelopes of the legal-move forms of the heads and of the loss (head_softmax_value_kernel<true>,
head8_kernel<true>, pv_loss_kernel<true>): the bars of tests/test_head_loss_bounds.py with t_j, H and
LAM_j taken over the EMPTY cells E of a row -- t_j = l_j - max_E l, H = sum_E p_k |t_k|, every sum over cells a sum over E
-- the same ROOM and the same cuts; a float32 NumPy restatement of each masked kernel's operation order; and CPU tests that
every restatement stays inside its bar against float64 with ROOM to spare.  tests/test_gpu_legal_policy.py asserts the same
bars of the kernels.

The derivation is the unmasked one: an occupied cell takes part in no operation (the kernels leave it out by selection),
a lane adds at most its 4 cells and the shuffle tree has 6 levels whatever E is, so the counts of roundings that the unmasked
bounds carry (<= 3 additions in the lane + 6 in the tree) bound the masked kernels too.  On an occupied cell the bar is 0:
probs and dlogits are exactly 0 there.  A row without an empty cell: everything about the policy is exactly 0.

Inputs: the logit families of tests/test_head_loss_bounds.py (randn x 3 .. 3e4, offsets of +-1e4, equal, two maxima) under
the occupancy families (no stone, one stone, random half, all but one cell, all cells), and "max on a stone": the row's
largest logit, 1e4 above the rest, on an occupied cell -- a maximum taken over all cells would leave every empty cell at
exp(-1e4) = 0 and the row at 0 / 0."""
import numpy as np
import pytest

import test_head_loss_bounds as hb
from test_head_loss_bounds import CAP_GRAD_REL, CAP_INFER, CAP_LOSS_OUT, CAP_LOSS_REL, F32, FN, ROOM, TINY, U

OCC_FAMILIES = ("none", "one", "half", "all_but_one", "all")
HWS = (225, 81, 64)
NS = (1, 3, 5, 37)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def occupancy_row(rs, family, hw):
    occ = np.zeros(hw, dtype=np.uint8)
    if family == "one":
        occ[rs.randint(hw)] = 1
    elif family == "half":
        occ[rs.permutation(hw)[:hw // 2]] = 1
    elif family == "all_but_one":
        occ[:] = 1
        occ[rs.randint(hw)] = 0
    elif family == "all":
        occ[:] = 1
    return occ


def occupancy_batch(family, n, hw, seed=0):
    """-> uint8 [n][hw]: rows 0, n // 2 and n - 1 of `family`, the others cycle through all families"""
    rs = np.random.RandomState(7000 + 31 * hw + n + seed)
    marked = {0, n // 2, n - 1}
    return np.stack([occupancy_row(rs, family if i in marked else OCC_FAMILIES[(i + seed) % len(OCC_FAMILIES)], hw)
                     for i in range(n)])


def max_on_a_stone(logits, occ, seed=0):
    """a copy of the float32 logits in which every row with a stone has its largest logit, 1e4 above the rest, on one"""
    rs = np.random.RandomState(99 + seed)
    out = np.array(logits, dtype=F32)
    for i in range(len(out)):
        stones = np.flatnonzero(occ[i])
        if len(stones):
            out[i, stones[rs.randint(len(stones))]] = F32(np.abs(out[i]).max() + 1e4)
    return out


def legal_loss_batch(logit_family, target_family, occ_family, n, hw, combo):
    """hb.loss_batch with an occupancy; pi is zero on occupied cells, as the search's visit counts are"""
    logits, u, pi, z = hb.loss_batch(logit_family, target_family, n, hw, combo)
    occ = occupancy_batch(occ_family, n, hw, combo)
    return logits, u, np.where(occ != 0, F32(0), pi).astype(F32), z, occ


# ---- float32 restatements of the masked kernels -----------------------------------------------------------------------
def _masked_max(l, emp):
    return np.where(emp, l, F32(-np.inf)).astype(F32).max(axis=1, keepdims=True)


def legal_softmax_tail_f32(logits, occ, form, max_over="empty"):
    """form "mul": head_softmax_value_kernel<true>;  "div": head8_kernel<true>.  max_over "all": what a kernel that took its
    maximum over every cell would compute (kept to show what "max on a stone" catches)"""
    l, emp = np.asarray(logits, dtype=F32), np.asarray(occ) == 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = _masked_max(l, emp) if max_over == "empty" else l.max(axis=1, keepdims=True)
        e = np.where(emp, np.exp(l - m), F32(0)).astype(F32)
        s = hb.wave_tree(hb.strided_lanes(e))[:, None]
        p = np.where(emp, e * (F32(1) / s) if form == "mul" else e / s, F32(0))
    assert p.dtype == F32
    return p


def legal_pv_loss_f32(logits, u, pi, z, occ):
    """pv_loss_kernel<true> + colsum_kernel -> dict like alphapig_amd.hipconv.pv_loss(occ=...)"""
    l, u, pi, z = (np.asarray(a, dtype=F32) for a in (logits, u, pi, z))
    emp = np.asarray(occ) == 0
    n = l.shape[0]
    zero = F32(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = l - _masked_max(l, emp)
        logs = np.log(hb.wave_tree(hb.strided_lanes(np.where(emp, np.exp(t), zero).astype(F32))))[:, None]
        lp = t - logs
        p = np.where(emp, np.exp(lp), zero).astype(F32)
        ce = -hb.wave_tree(hb.strided_lanes(np.where(emp, pi * lp, zero).astype(F32)))
        ent = -hb.wave_tree(hb.strided_lanes(np.where(emp, p * lp, zero).astype(F32)))
        spi = hb.wave_tree(hb.strided_lanes(np.where(emp, pi, zero).astype(F32)))[:, None]
        g = F32(1) / F32(n)
        dl = np.where(emp, (p * spi - pi) * g, zero).astype(F32)
    v = np.tanh(u)
    d = z - v
    terms = np.stack([d * d, ce, ent], axis=1)
    assert terms.dtype == F32 and p.dtype == F32
    return {"loss3": (terms.astype(np.float64).sum(axis=0) * np.float64(g)).astype(F32), "dlogits": dl,
            "dvlogit": F32(2) * (v - z) * (F32(1) - v * v) * g, "probs": p, "values": v}


# ---- float64 references over the empty cells --------------------------------------------------------------------------
def legal_softmax64(logits, occ):
    """-> (p, t): softmax over the empty cells of the float32 logits in float64, 0 on occupied cells and on rows without an
    empty cell; t = l - max_E l on E, 0 elsewhere"""
    l, emp = np.asarray(logits, dtype=np.float64), np.asarray(occ) == 0
    m = np.where(emp, l, -np.inf).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        t = np.where(emp, l - np.where(np.isfinite(m), m, 0.0), 0.0)
    e = np.where(emp, np.exp(t), 0.0)
    s = e.sum(axis=1, keepdims=True)
    return e / np.where(s > 0, s, 1.0), t


def legal_pv_loss64(logits, u, pi, z, occ):
    """hb.pv_loss64 over the empty cells: log-softmax, cross-entropy, entropy and sum pi over E"""
    u, pi, z = (np.asarray(a, dtype=np.float64) for a in (u, pi, z))
    emp = np.asarray(occ) == 0
    n = pi.shape[0]
    _, t = legal_softmax64(logits, occ)
    s = np.where(emp, np.exp(t), 0.0).sum(axis=1, keepdims=True)
    logs = np.log(np.where(s > 0, s, 1.0))
    lp = np.where(emp, t - logs, 0.0)
    p = np.where(emp, np.exp(lp), 0.0)
    pe = np.where(emp, pi, 0.0)
    v = np.tanh(u)
    sech2 = 1.0 / np.cosh(np.minimum(np.abs(u), 300.0)) ** 2
    return {"loss3": np.array([((z - v) ** 2).mean(), (-(pe * lp).sum(axis=1)).mean(), (-(p * lp).sum(axis=1)).mean()]),
            "dlogits": np.where(emp, p * pe.sum(axis=1, keepdims=True) - pe, 0.0) / n, "dvlogit": 2 * (v - z) * sech2 / n,
            "probs": p, "values": v, "t": t, "logs": logs, "lp": lp, "pi": pe}


# ---- bars: hb's, every sum over the empty cells -----------------------------------------------------------------------
def legal_softmax_bar(logits, occ):
    """hb.softmax_bar over E -> (bar of every probability: 0 on occupied cells, bar of |row sum - 1|)"""
    emp = np.asarray(occ) == 0
    p, t = legal_softmax64(logits, occ)
    H = (p * np.abs(t)).sum(axis=1, keepdims=True)
    bar = np.where(emp, ROOM * U * p * (np.abs(t) + H + 2 * FN + 11) + TINY, 0.0)
    return np.minimum(bar, CAP_INFER), np.minimum(bar.sum(axis=1), CAP_INFER)


def legal_pv_loss_bars(logits, u, pi, z, occ):
    """hb.pv_loss_bars over E; 0 on the occupied cells of probs and dlogits"""
    r = legal_pv_loss64(logits, u, pi, z, occ)
    emp = np.asarray(occ) == 0
    z = np.asarray(z, dtype=np.float64)
    pi = r["pi"]
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
            "dlogits": np.where(emp, np.minimum(dl, CAP_GRAD_REL * np.abs(r["dlogits"]).max() + 1e-6), 0.0),
            "dvlogit": np.minimum(dv, CAP_GRAD_REL * np.abs(r["dvlogit"]).max() + 1e-6),
            "probs": np.where(emp, np.minimum(UR * p * (lam + FN) + TINY, CAP_LOSS_OUT), 0.0),
            "values": hb.tanh_bar(u, CAP_LOSS_OUT)}, r


def positive_zero(a):
    """every element is +0 by bit pattern"""
    return not np.asarray(a, dtype=F32).view(np.uint32).any()


# ---- the restatements against float64, with room ----------------------------------------------------------------------
def _check_loss(args, tag, worst):
    bars, ref = legal_pv_loss_bars(*args)
    got = legal_pv_loss_f32(*args)
    occ = args[4] != 0
    for k in bars:
        assert np.isfinite(got[k]).all(), (tag, k)
        q = hb.ratio(got[k], ref[k], bars[k])
        worst[k] = max(worst.get(k, 0.0), q)
        assert q * ROOM <= 1.0, (tag, k, q)
    assert positive_zero(got["probs"][occ]) and positive_zero(got["dlogits"][occ])
    assert (bars["probs"] <= CAP_LOSS_OUT).all() and (bars["loss3"] <= CAP_LOSS_REL * (1 + np.abs(ref["loss3"]))).all()
    return got


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("n", NS)
def test_the_masked_loss_restatement_stays_inside_its_bars(n, hw):
    worst = {}
    for combo, lf, tf in hb.loss_combos():
        of = OCC_FAMILIES[combo % len(OCC_FAMILIES)]
        args = legal_loss_batch(lf, tf, of, n, hw, combo)
        _check_loss(args, (lf, tf, of), worst)
        # the row's largest logit on a stone, 1e4 above the rest: the maximum is taken over the empty cells only
        hot = (max_on_a_stone(args[0], args[4], combo),) + args[1:]
        got = _check_loss(hot, (lf, tf, of, "max on a stone"), worst)
        free = (args[4] == 0).any(axis=1)
        assert np.abs(got["probs"].astype(np.float64).sum(axis=1)[free] - 1).max(initial=0) <= 225 * CAP_LOSS_OUT
    print("n %d hw %d masked loss restatement / bar: %s" % (n, hw, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("form,hw", [("mul", 225), ("mul", 81), ("mul", 36), ("div", 64)])
def test_the_masked_softmax_tail_restatement_stays_inside_its_bar(form, hw):
    for i, lf in enumerate(hb.LOGIT_FAMILIES):
        for of in OCC_FAMILIES:
            rs = np.random.RandomState(len(lf) + hw)
            logits = np.stack([hb.logit_row(rs, lf, hw) for _ in range(37)]).astype(F32)
            occ = occupancy_batch(of, 37, hw, i)
            for l in (logits, max_on_a_stone(logits, occ, i)):
                bar, sum_bar = legal_softmax_bar(l, occ)
                p = legal_softmax_tail_f32(l, occ, form)
                ref = legal_softmax64(l, occ)[0]
                free = (occ == 0).any(axis=1)
                q = hb.ratio(p, ref, bar)
                qs = hb.ratio(p.astype(np.float64).sum(axis=1)[free], 1.0, sum_bar[free])
                assert np.isfinite(p).all() and q * ROOM <= 1.0 and qs * ROOM <= 1.0, (lf, of, q, qs)
                assert positive_zero(p[occ != 0]) and positive_zero(p[~free]) and (bar <= CAP_INFER).all()
            # what the family is for: with the maximum over all cells every empty cell is exp(-1e4) = 0 and the row 0 / 0
            both = free & (occ != 0).any(axis=1)
            wrong = legal_softmax_tail_f32(max_on_a_stone(logits, occ, i), occ, form, max_over="all")
            assert np.isnan(wrong[both][occ[both] == 0]).all()


@pytest.mark.parametrize("hw", HWS)
def test_degenerate_rows_are_exact_in_the_restatement(hw):
    logits, u, pi, z = hb.loss_batch("randn30", "dirichlet", 5, hw, 3)
    # a single empty cell: p = 1, ce = ent = 0 whatever pi holds there
    occ = np.stack([occupancy_row(np.random.RandomState(i), "all_but_one", hw) for i in range(5)])
    pi1 = np.where(occ != 0, F32(0), F32(1)).astype(F32)
    got = legal_pv_loss_f32(logits, u, pi1, z, occ)
    assert (got["probs"][occ == 0] == 1).all() and got["loss3"][1] == 0 and got["loss3"][2] == 0
    assert positive_zero(got["probs"][occ != 0]) and not got["dlogits"].any()
    for form in ("mul", "div"):
        assert (legal_softmax_tail_f32(logits, occ, form)[occ == 0] == 1).all()
    # no empty cell: all zeros, finite
    full = np.ones_like(occ)
    got = legal_pv_loss_f32(logits, u, pi, z, full)
    assert all(np.isfinite(v).all() for v in got.values())
    assert positive_zero(got["probs"]) and positive_zero(got["dlogits"]) and got["loss3"][1] == 0 and got["loss3"][2] == 0
    # no stone: the unmasked restatement's bits
    none = np.zeros_like(occ)
    a, b = legal_pv_loss_f32(logits, u, pi, z, none), hb.pv_loss_f32(logits, u, pi, z)
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    for form in ("mul", "div"):
        np.testing.assert_array_equal(legal_softmax_tail_f32(logits, none, form), hb.softmax_tail_f32(logits, form))
