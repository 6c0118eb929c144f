"""The training entry points' per-engine scratch (csrc/apz_engine.hip): the buffers that grow on demand and the ordering
between streams that use them.  Two properties no operator test targets:

  growth keeps results   calls in ascending size on an engine that has never run (every call reallocates its buffer), then
                         the same calls again when nothing grows: each result bit-equal to its twin
  two streams, one scratch   the same two operators alternating on two streams: every output equals the single-stream
                         result (StreamScope orders a stream behind the previous user of the scratch)

Nothing here provokes anything: every call is one the trainer makes, at the smallest sizes that step a capacity."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _rows16(t):
    return F.pad(t, (0, 1)).contiguous()


@pytest.fixture
def hipconv(monkeypatch):
    """alphapig_amd.hipconv with no engine yet: every scratch buffer of the engines this test creates starts empty, whatever
    ran before in the process.  The engines are destroyed afterwards."""
    from alphapig_amd import _native, hipconv as ops
    fresh = {}
    monkeypatch.setattr(ops, "_ENGINES", fresh)
    yield ops
    torch.cuda.synchronize()
    for hnd in fresh.values():
        _native.hip().apz_destroy(hnd)


def _twice(calls):
    """Every call in order (growing), then every call again (nothing grows): the pairs of results"""
    first = [c() for c in calls]
    second = [c() for c in calls]
    torch.cuda.synchronize()
    return list(zip(first, second))


def _assert_twins(pairs):
    for k, (a, b) in enumerate(pairs):
        a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.data_ptr() != y.data_ptr()
            assert bool(torch.isfinite(x).all()), k
            assert torch.equal(x, y), k


def test_weight_gradient_partials_grow(hipconv):
    x8, dy8 = _randn(1, 1, 4, 8, 8), _randn(2, 1, 32, 8, 8)
    x1, dy1 = _rows16(_randn(3, 1, 128, 15, 15)), _rows16(_randn(4, 1, 128, 15, 15))
    x9, dy9 = _rows16(_randn(5, 9, 128, 15, 15)), _rows16(_randn(6, 9, 128, 15, 15))
    dymax = dy9.abs().amax(dim=(0, 2, 3)).reshape(1, 128).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    pairs = _twice([
        lambda: hipconv.conv3x3_wgrad(x8, dy8),                         # dense 8x8, 4 -> 32 channels, one slice
        lambda: hipconv.conv3x3_wgrad(x1, dy1, hipconv.ROWS16),         # 8 slices
        lambda: hipconv.conv3x3_wgrad(x9, dy9, hipconv.ROWS16),         # 16 slices
        lambda: hipconv.conv3x3_wgrad_f16x2(x9, dy9, dymax, flag),
    ])
    _assert_twins(pairs)
    assert int(flag.item()) == 0
    assert tuple(pairs[0][0].shape) == (32, 4, 3, 3) and tuple(pairs[3][0].shape) == (128, 128, 3, 3)


def test_head_scratch_grows(hipconv):
    logits, vlogit = _randn(10, 1, 64), _randn(11, 1)
    pi, z = torch.softmax(_randn(12, 1, 64), dim=1), torch.ones(1, device="cuda")
    dy = _randn(13, 2, 128, 8, 8)
    x, w1, w2 = _randn(14, 3, 128, 8, 8), _randn(15, 4, 128, 1, 1), _randn(16, 2, 128, 1, 1)
    d1, d2 = _randn(17, 3, 4, 8, 8), _randn(18, 3, 2, 8, 8)

    def loss():
        out = hipconv.pv_loss(logits, vlogit, pi, z, grads=True)
        return out["loss3"], out["dlogits"], out["dvlogit"]
    _assert_twins(_twice([
        loss,                                                           # 3 floats
        lambda: hipconv.bias_grad(dy),                                  # 2 slices x 128
        lambda: hipconv.conv1x1_bwd_pair(x, w1, d1, w2, d2),            # 3 boards x 6 x 128
    ]))


def test_rows16_copies_grow(hipconv):
    """apz_wino_conv_add on DENSE tensors through the library handle (hipconv routes dense tensors there from 192 boards on)"""
    from alphapig_amd import _native
    L, hnd = _native.hip(), hipconv._engine(15, 15, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w, bias = _randn(20, 128, 128, 3, 3) * 0.05, _randn(21, 128)
    upk = torch.empty((L.apz_wino_packed_size(),), dtype=torch.float32, device="cuda")
    assert L.apz_wino_pack(hnd, w.data_ptr(), 0, upk.data_ptr(), stream) == 0
    xs = {n: _randn(22 + n, n, 128, 15, 15) for n in (1, 3)}

    def conv(n):
        y = torch.empty_like(xs[n])
        rc = L.apz_wino_conv_add(hnd, xs[n].data_ptr(), upk.data_ptr(), bias.data_ptr(), None, y.data_ptr(), n, 1,
                                 hipconv.DENSE, stream)
        assert rc == 0, L.apz_last_error()
        return y
    pairs = _twice([lambda: conv(1), lambda: conv(3)])
    _assert_twins(pairs)
    # (the operator itself, loosely: the copies went through the buffers they were meant to)
    ref = torch.relu(F.conv2d(xs[3].double(), w.double(), bias.double(), padding=1))
    assert float((pairs[1][0].double() - ref).abs().max()) < 1e-3 * float(ref.abs().max())


def test_adam_table_grows(hipconv):
    dev = torch.device("cuda", 0)

    def step(sizes, seed):
        ts = [[_randn(seed + 4 * i + j, s) for j in range(4)] for i, s in enumerate(sizes)]
        for t in ts:
            t[3].abs_()                                                 # v >= 0
        hipconv.adam_step([(w, g, m, v, 1e-4) for w, g, m, v in ts], 1e-3, 0.9, 0.999, 1e-8, 1.0 / 64, dev)
        return tuple(t[j] for t in ts for j in (0, 2, 3))
    _assert_twins(_twice([lambda: step([8], 30), lambda: step([8, 5, 3, 2, 1], 40)]))


def test_gather_entries_grow(hipconv):
    cap, hw, stride = 4, 64, 80
    rs = np.random.RandomState(50)
    codes = torch.tensor(rs.randint(0, 9, size=(cap, stride)).astype(np.uint8), device="cuda")
    pi, z = _randn(51, cap, hw), _randn(52, cap)
    words = [[13], [0, 31, 8, 9, 17, 26, 3, 12, 30]]
    pairs = _twice([lambda: hipconv.replay_gather(codes, pi, z, words[0], 8, 8, 9),
                    lambda: hipconv.replay_gather(codes, pi, z, words[1], 8, 8, 9)])
    _assert_twins(pairs)
    for (states, p, zz), ent in zip((a for a, _ in pairs), words):
        assert tuple(states.shape) == (len(ent), 9, 8, 8) and tuple(p.shape) == (len(ent), hw)
        assert torch.equal(zz, z[[e >> 3 for e in ent]])


def test_two_streams_never_share_the_scratch(hipconv):
    """bias_grad on stream A and pv_loss on stream B, both through the head scratch of the 8x8 engine, alternating 20 times:
    every output equals the single-stream result of the same call."""
    dy = _randn(60, 2, 128, 8, 8)
    logits, vlogit = _randn(61, 3, 64), _randn(62, 3)
    pi, z = torch.softmax(_randn(63, 3, 64), dim=1), torch.tensor([1.0, -1.0, 1.0], device="cuda")
    db_ref = hipconv.bias_grad(dy)
    ref = hipconv.pv_loss(logits, vlogit, pi, z, grads=True)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    dbs, losses = [], []
    for _ in range(20):
        with torch.cuda.stream(sa):
            dbs.append(hipconv.bias_grad(dy))
        with torch.cuda.stream(sb):
            losses.append(hipconv.pv_loss(logits, vlogit, pi, z, grads=True))
    sa.synchronize()
    sb.synchronize()
    assert bool(torch.isfinite(db_ref).all()) and bool(torch.isfinite(ref["loss3"]).all())
    for k in range(20):
        assert torch.equal(dbs[k], db_ref), k
        for key in ("loss3", "dlogits", "dvlogit"):
            assert torch.equal(losses[k][key], ref[key]), (k, key)
