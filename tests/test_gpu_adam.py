"""hipconv.adam_step / adam_step(skip=...) (adam_step_kernel, adam_step_unless_kernel: one launch over a table of tensors,
32 x 256 threads per tensor) against the same recurrence in float64, step by step from the kernel's own float32 state.

Bars per step (u = 2^-24), from the roundings of
    g = grad * rescale + wd * w;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= lr_t m / (sqrt(v) + eps):
at most 4 roundings on the way to each of m and v and 8 on the way to the update.  m and v: 8 u relative -- relative to the
sum of the magnitudes of their terms, which is |m| (v) itself unless b1 m and (1 - b1) g cancel (a fresh random gradient per
step does that to a few elements; a bar relative to the cancelled |m| would ask more than the arithmetic can give);
w: |dw| <= 2 (u |w| + 8 u lr_t |m| / (sqrt(v) + eps)), |m| read the same way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24
SIZES = (1, 3, 255, 256, 257, 8193, 100003)
B1, B2, EPS, RESCALE = 0.9, 0.999, 1e-8, 1.0 / 64


def _f32(v):
    return float(np.float32(v))


def _table(seed):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(k, generator=g).cuda() for k in SIZES]
    ms = [torch.zeros(k).cuda() for k in SIZES]
    vs = [torch.zeros(k).cuda() for k in SIZES]
    wds = [0.0 if i % 2 == 0 else 1e-4 for i in range(len(SIZES))]
    return g, ws, ms, vs, wds


def _grads(g):
    return [(torch.randn(k, generator=g) * 3.0).cuda() for k in SIZES]


def _lr_t(lr, t):
    return lr * (1.0 - B2 ** t) ** 0.5 / (1.0 - B1 ** t)


def _clone(ts):
    return [t.clone() for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_three_steps_against_float64():
    from alphapig_amd import hipconv
    g, ws, ms, vs, wds = _table(1)
    dev = ws[0].device
    b1, b2, eps, rs = _f32(B1), _f32(B2), _f32(EPS), _f32(RESCALE)
    worst = [0.0, 0.0, 0.0]
    for t in (1, 2, 3):
        gs = _grads(g)
        lr_t = _lr_t(1e-3, t)
        before = [[x.double().cpu().numpy() for x in ts] for ts in (ws, ms, vs)]
        hipconv.adam_step([(w, gr, m, v, wd) for w, gr, m, v, wd in zip(ws, gs, ms, vs, wds)], lr_t, B1, B2, EPS, RESCALE, dev)
        torch.cuda.synchronize()
        lr = _f32(lr_t)
        for i, wd in enumerate(wds):
            w0, m0, v0 = before[0][i], before[1][i], before[2][i]
            g0 = gs[i].double().cpu().numpy()
            wd = _f32(wd)
            gg = g0 * rs + wd * w0
            gabs = np.abs(g0 * rs) + np.abs(wd * w0)
            m64 = m0 * b1 + (1.0 - b1) * gg
            v64 = v0 * b2 + (1.0 - b2) * gg * gg
            w64 = w0 - lr * m64 / (np.sqrt(v64) + eps)
            mabs = np.abs(m0) * b1 + (1.0 - b1) * gabs
            vabs = v0 * b2 + (1.0 - b2) * gabs * gabs
            w1, m1, v1 = (x[i].double().cpu().numpy() for x in (ws, ms, vs))
            bar_m, bar_v = 8 * U * mabs, 8 * U * vabs
            bar_w = 2 * (U * np.abs(w0) + 8 * U * lr * mabs / (np.sqrt(v64) + eps))
            q = [float((np.abs(a - b) / bar).max()) for a, b, bar in ((m1, m64, bar_m), (v1, v64, bar_v), (w1, w64, bar_w))]
            worst = [max(a, b) for a, b in zip(worst, q)]
            assert q[0] <= 1.0 and q[1] <= 1.0 and q[2] <= 1.0, (t, SIZES[i], q)
    print("worst error / bar: m %.3f  v %.3f  w %.3f" % tuple(worst))


def test_zero_gradient_on_zero_moments_leaves_the_weights():
    from alphapig_amd import hipconv
    g, ws, ms, vs, _ = _table(2)
    w0 = _clone(ws)
    zeros = [torch.zeros_like(w) for w in ws]
    hipconv.adam_step([(w, z, m, v, 0.0) for w, z, m, v in zip(ws, zeros, ms, vs)], _lr_t(1e-3, 1), B1, B2, EPS, RESCALE,
                      ws[0].device)
    torch.cuda.synchronize()
    assert _same(ws, w0)
    assert all(float(m.abs().max()) == 0.0 for m in ms) and all(float(v.abs().max()) == 0.0 for v in vs)


def test_the_skip_word():
    """word 0: adam_step's bits; word not zero: weights and moments untouched"""
    from alphapig_amd import hipconv
    g, ws, ms, vs, wds = _table(3)
    dev = ws[0].device
    gs = _grads(g)
    lr_t = _lr_t(1e-3, 1)
    hipconv.adam_step([(w, gr, m, v, wd) for w, gr, m, v, wd in zip(ws, gs, ms, vs, wds)], lr_t, B1, B2, EPS, RESCALE, dev)  # moments != 0
    a = [_clone(ts) for ts in (ws, ms, vs)]
    b = [_clone(ts) for ts in (ws, ms, vs)]
    c = [_clone(ts) for ts in (ws, ms, vs)]
    start = [_clone(ts) for ts in (ws, ms, vs)]
    gs = _grads(g)
    lr_t = _lr_t(1e-3, 2)
    entries = lambda s: [(w, gr, m, v, wd) for w, gr, m, v, wd in zip(s[0], gs, s[1], s[2], wds)]
    clear = torch.zeros(1, dtype=torch.int32, device=dev)
    for word in (1, -1, 1 << 20):
        setw = torch.full((1,), word, dtype=torch.int32, device=dev)
        hipconv.adam_step(entries(c), lr_t, B1, B2, EPS, RESCALE, dev, skip=setw)
        torch.cuda.synchronize()
        assert int(setw.item()) == word
        for got, ref in zip(c, start):
            assert _same(got, ref), word
    hipconv.adam_step(entries(a), lr_t, B1, B2, EPS, RESCALE, dev)
    hipconv.adam_step(entries(b), lr_t, B1, B2, EPS, RESCALE, dev, skip=clear)
    torch.cuda.synchronize()
    assert int(clear.item()) == 0
    for got, ref in zip(b, a):
        assert _same(got, ref)
    assert not _same(a[0], start[0])


def test_table_size_limit():
    from alphapig_amd import hipconv
    w, gr, m, v = (torch.zeros(4097, device="cuda") for _ in range(4))
    entries = [(w[i:i + 1], gr[i:i + 1], m[i:i + 1], v[i:i + 1], 0.0) for i in range(4097)]
    with pytest.raises(RuntimeError):
        hipconv.adam_step(entries, 1e-3, B1, B2, EPS, RESCALE, w.device)
    torch.cuda.synchronize()
    assert float(w.abs().max()) == 0.0
    hipconv.adam_step(entries[:4096], 1e-3, B1, B2, EPS, RESCALE, w.device)      # the largest table is taken
    torch.cuda.synchronize()
