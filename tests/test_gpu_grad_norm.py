"""hipconv.grad_norm / adam_step_guarded (csrc/grad_guard.h: grad_sumsq_kernel over the Adam table, grid 32 x ntensors;
grad_guard_fold_kernel, one workgroup; adam_step_guarded_kernel) against NumPy float64 and against the existing adam_step.

Bars, derived, not measured:
  norm         every float32 squared is exact in double; the at most 3.2 M double additions of one table lose at most
               3.2e6 * 2^-53 = 4e-10 relative (far less in the kernels' tree order), the square root and the product with
               rescale 2^-52 each: the record's norm is the float64 value rounded to float32 once -- within 1 float32 ulp of
               NumPy's float64 norm rounded to float32 (they differ only where the two doubles straddle a rounding boundary).
  rescale_eff  under a clip: (float)(clip / norm) is one rounding of a double that is right to 4e-10, the fp32 product with
               rescale a second: within 2 float32 ulp of the float64 value rescale * clip / norm.
  everything else is bit equality.
The tensors: lengths 1, 3, 255, 256, 257, 8193 and 128 * 128 * 9 (one element, less than one 16-byte quad, around 256
elements, one quad more than the grid's 8192 threads take in one trip, the trunk weight), tables of 1 to 5, storage that
starts 0, 4, 8 and 12 bytes past a 16-byte boundary, values randn times 1e-20 .. 1e18."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRUNK = 128 * 128 * 9
# (lengths, offsets in floats past a 16-byte boundary, scales)
CASES = [
    ((1,), (0,), (1.0,)),
    ((3, 255), (1, 0), (1e-20, 1e-20)),
    ((256, 257, 8193), (2, 3, 1), (1.0, 1e3, 1e-3)),
    ((TRUNK, 8193, 1, 3), (0, 3, 2, 1), (1e18, 1e18, 1e18, 1e18)),
    ((TRUNK, 257, 256, 255, 8193), (1, 0, 2, 3, 0), (1e-2, 1.0, 1e-20, 1e18, 1e-3)),
]
RESCALES = (1.0 / 64, 1.0 / 3)
B1, B2, EPS = 0.9, 0.999, 1e-8


def _f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _host(case):
    """The case's host tensors and their float64 sum of squares: computed once, never written"""
    lengths, _, scales = CASES[case]
    rs = np.random.RandomState(100 + case)
    arrs = [(rs.randn(n) * s).astype(np.float32) for n, s in zip(lengths, scales)]
    for a in arrs:
        a.setflags(write=False)
    total = sum(float(np.sum(a.astype(np.float64) ** 2)) for a in arrs)
    return arrs, total


def _place(a, off):
    """a (host float32) on the device in storage that starts `off` floats past a 16-byte boundary"""
    base = torch.empty(a.size + 8, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[off:off + a.size]
    v.copy_(torch.from_numpy(np.array(a)))
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def _entries(gs):
    return [(g, g, g, g, 0.0) for g in gs]          # the norm reads the gradients only


def _read(rec):
    from alphapig_amd import hipconv
    return hipconv.read_guard_record(rec.cpu().numpy())


def _bits(rec):
    return rec.view(torch.int32).cpu().numpy().copy()


def _ulps(a, b):
    """distance between two positive finite float32 in units in the last place"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_norm_against_float64_and_reproducible(case):
    from alphapig_amd import hipconv
    arrs, total = _host(case)
    offs = CASES[case][1]
    dev = torch.device("cuda", 0)
    shifted = [_place(a, o) for a, o in zip(arrs, offs)]
    aligned = [_place(a, 0) for a in arrs]
    rotated = [_place(a, (o + 1 + i) % 4) for i, (a, o) in enumerate(zip(arrs, offs))]
    for rescale in RESCALES:
        ref = np.sqrt(total) * float(np.float32(rescale))
        recs = [hipconv.grad_norm(_entries(gs), rescale, None, dev) for gs in (shifted, shifted, aligned, rotated)]
        norm, eff, skip, why = _read(recs[0])
        print("case %d rescale %.4g: norm %.9g float64 %.17g (%d ulp)" % (case, rescale, norm, ref, _ulps(norm, ref)))
        assert _ulps(norm, ref) <= 1
        assert eff == np.float32(rescale) and not skip and why == 0
        b = [_bits(r) for r in recs]
        assert np.array_equal(b[0], b[1])                                   # two runs
        assert np.array_equal(b[0], b[2]) and np.array_equal(b[0], b[3])    # the same values, other alignments


@pytest.mark.parametrize("case", [2, 4])
def test_clip_scales_to_the_norm(case):
    from alphapig_amd import hipconv
    arrs, total = _host(case)
    gs = [_place(a, o) for a, o in zip(arrs, CASES[case][1])]
    dev = gs[0].device
    rescale = RESCALES[1]
    rs32 = float(np.float32(rescale))
    norm = _read(hipconv.grad_norm(_entries(gs), rescale, None, dev))[0]
    clip = _f32(norm / 2)
    n2, eff, skip, why = _read(hipconv.grad_norm(_entries(gs), rescale, clip, dev))
    ref = rs32 * clip / (np.sqrt(total) * rs32)
    print("case %d: rescale_eff %.9g float64 %.17g (%d ulp)" % (case, eff, ref, _ulps(eff, ref)))
    assert n2 == norm and not skip and why == 0
    assert _ulps(eff, ref) <= 2
    # above the norm (the next float32: the record's norm is the double rounded, which may have rounded down), and with the
    # clip off: rescale itself
    for c in (float(np.nextafter(np.float32(norm), np.float32(np.inf))), _f32(norm * 2), 0.0, None, -1.0):
        n3, eff, skip, why = _read(hipconv.grad_norm(_entries(gs), rescale, c, dev))
        assert n3 == norm and eff == np.float32(rescale) and not skip and why == 0


def test_non_finite_gradient_elements_set_bit_1():
    from alphapig_amd import hipconv
    rs = np.random.RandomState(7)
    lengths, offs = (257, 8193, 1000), (1, 2, 3)
    arrs = [rs.randn(n).astype(np.float32) for n in lengths]
    gs = [_place(a, o) for a, o in zip(arrs, offs)]
    dev = gs[0].device
    rec = torch.zeros(4, device=dev)
    assert _read(hipconv.grad_norm(_entries(gs), 1.0, 1.0, dev, record=rec))[2:] == (False, 0)
    for ti in (0, len(gs) - 1):
        n = lengths[ti]
        for pos in (0, n // 2, n - 1):
            for bad in (float("nan"), float("inf"), -float("inf")):
                keep = float(gs[ti][pos])
                gs[ti][pos] = bad
                norm, eff, skip, why = _read(hipconv.grad_norm(_entries(gs), 1.0, 1.0, dev, record=rec))
                gs[ti][pos] = keep
                assert skip and why == hipconv.GUARD_GRAD, (ti, pos, bad, why)
                assert not np.isfinite(norm)
    assert _read(hipconv.grad_norm(_entries(gs), 1.0, 1.0, dev, record=rec))[2:] == (False, 0)


def test_loss_and_skip_word_set_bits_2_and_4():
    from alphapig_amd import hipconv
    arrs, _ = _host(2)
    gs = [_place(a, o) for a, o in zip(arrs, CASES[2][1])]
    dev = gs[0].device
    clear = torch.zeros(1, dtype=torch.int32, device=dev)
    setw = torch.full((1,), 1, dtype=torch.int32, device=dev)
    high = torch.full((1,), -2 ** 31, dtype=torch.int32, device=dev)
    good = torch.tensor([0.5, 2.0, 3.0], device=dev)
    rec = hipconv.grad_norm(_entries(gs), 1.0 / 64, None, dev)
    plain, plain_norm = _bits(rec), _read(rec)[0]
    assert np.array_equal(_bits(hipconv.grad_norm(_entries(gs), 1.0 / 64, None, dev, loss3=good, skip=clear)), plain)
    for i in range(3):
        for bad in (float("nan"), float("inf"), -float("inf")):
            l3 = good.clone()
            l3[i] = bad
            norm, eff, skip, why = _read(hipconv.grad_norm(_entries(gs), 1.0 / 64, None, dev, loss3=l3))
            assert skip and why == hipconv.GUARD_LOSS and norm == plain_norm
    for w in (setw, high):
        assert _read(hipconv.grad_norm(_entries(gs), 1.0 / 64, None, dev, skip=w))[2:] == (True, hipconv.GUARD_SKIP_IN)
    l3 = good.clone()
    l3[1] = float("nan")
    gs[0][5] = float("inf")
    assert _read(hipconv.grad_norm(_entries(gs), 1.0 / 64, None, dev, loss3=l3, skip=setw))[2:] == (True, 7)


def test_norm_beyond_float32_sets_bit_8_under_a_clip_only():
    from alphapig_amd import hipconv
    g = torch.full((8193,), 3e38, device="cuda")         # finite elements, sum of squares 7e80: fine in double
    norm, eff, skip, why = _read(hipconv.grad_norm(_entries([g]), 1.0, 1.0, g.device))
    assert skip and why == hipconv.GUARD_NORM and np.isinf(norm)
    norm, eff, skip, why = _read(hipconv.grad_norm(_entries([g]), 1.0, None, g.device))
    assert not skip and why == 0 and np.isinf(norm) and eff == np.float32(1.0)
    norm, eff, skip, why = _read(hipconv.grad_norm(_entries([g]), 2.0 ** -20, 1.0, g.device))    # the RESCALED norm counts
    assert not skip and why == 0 and _ulps(norm, float(np.float32(3e38)) * np.sqrt(8193.0) * 2.0 ** -20) <= 1


def _adam_state(seed):
    """A table with moments that are not zero: (ws, gs, ms, vs, wds), gradients in shifted storage"""
    from alphapig_amd import hipconv
    g = torch.Generator().manual_seed(seed)
    sizes, offs = (1, 3, 255, 256, 257, 8193), (1, 2, 3, 0, 1, 2)
    ws = [torch.randn(k, generator=g).cuda() for k in sizes]
    ms = [torch.zeros(k).cuda() for k in sizes]
    vs = [torch.zeros(k).cuda() for k in sizes]
    wds = [0.0 if i % 2 == 0 else 1e-4 for i in range(len(sizes))]
    g0 = [(torch.randn(k, generator=g) * 2.0).cuda() for k in sizes]
    hipconv.adam_step(list(zip(ws, g0, ms, vs, wds)), 1e-3, B1, B2, EPS, 1.0 / 64, ws[0].device)
    gs = [_place((torch.randn(k, generator=g) * 3.0).numpy(), o) for k, o in zip(sizes, offs)]
    return ws, gs, ms, vs, wds


def _clone(ts):
    return [t.clone() for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_guarded_adam_is_adam_step_with_the_records_rescale():
    from alphapig_amd import hipconv
    ws, gs, ms, vs, wds = _adam_state(11)
    dev = ws[0].device
    lr_t, rescale = 2e-3, 1.0 / 64
    norm = _read(hipconv.grad_norm(list(zip(ws, gs, ms, vs, wds)), rescale, None, dev))[0]

    def run(clip, **kw):
        a = [_clone(ws), _clone(ms), _clone(vs)]
        rec = hipconv.adam_step_guarded(list(zip(a[0], gs, a[1], a[2], wds)), lr_t, B1, B2, EPS, rescale, clip, dev, **kw)
        return a, _read(rec)

    def plain(rs):
        b = [_clone(ws), _clone(ms), _clone(vs)]
        hipconv.adam_step(list(zip(b[0], gs, b[1], b[2], wds)), lr_t, B1, B2, EPS, rs, dev)
        return b
    # clipped: the existing kernel with rescale_eff
    a, (n, eff, skip, why) = run(_f32(norm / 2))
    assert n == norm and not skip and abs(float(eff) / rescale - 0.5) < 1e-6
    b = plain(float(eff))
    assert all(_same(x, y) for x, y in zip(a, b))
    assert not _same(a[0], plain(rescale)[0])                 # (and the clip did change the step)
    # clip above the norm, and no clip: the plain step's bits
    for clip in (_f32(norm * 2), None):
        a, (n, eff, skip, why) = run(clip)
        assert not skip and eff == np.float32(rescale)
        assert all(_same(x, y) for x, y in zip(a, plain(rescale)))
    # skip: nothing moves, whatever the reason
    setw = torch.full((1,), 1, dtype=torch.int32, device=dev)
    nanloss = torch.tensor([0.1, float("nan"), 0.2], device=dev)
    for kw, bit in (({"skip": setw}, hipconv.GUARD_SKIP_IN), ({"loss3": nanloss}, hipconv.GUARD_LOSS)):
        a, (n, eff, skip, why) = run(_f32(norm / 2), **kw)
        assert skip and why == bit
        assert all(_same(x, y) for x, y in zip(a, (ws, ms, vs)))
    keep = float(gs[-1][8192])
    gs[-1][8192] = float("nan")
    a, (n, eff, skip, why) = run(None)
    gs[-1][8192] = keep
    assert skip and why == hipconv.GUARD_GRAD
    assert all(_same(x, y) for x, y in zip(a, (ws, ms, vs)))
    assert all(bool(torch.isfinite(x).all()) for x in a[0])


def test_arguments_are_checked():
    from alphapig_amd import hipconv
    g = torch.randn(64).cuda()
    with pytest.raises(ValueError, match="16-byte"):
        hipconv.grad_norm(_entries([g]), 1.0, None, g.device, record=torch.zeros(8, device=g.device)[1:5])
    with pytest.raises(ValueError, match="record"):
        hipconv.grad_norm(_entries([g]), 1.0, None, g.device, record=torch.zeros(3, device=g.device))
    with pytest.raises(RuntimeError, match="bad argument"):
        hipconv.grad_norm([], 1.0, None, g.device)
