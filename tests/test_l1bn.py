"""nn.L1BatchNorm2d (csrc/l1bn.hip) against the reference MODULE: tests/golden/l1bn_ops.pt holds what the reference's
L1BatchNorm2d (models/modules/lp_norm.py:238-291, float64, CPU) returned at these shapes (tools/make_golden_l1bn.py), with
the rel-L2 bounds test_ops.py::test_batchnorm_train_fwd_bwd applies to BatchNorm2d (forward fp32 1e-5 / bf16 1e-2 / f16
2e-3; dy, dres 1e-4 / 1.5e-2; dgamma, dbeta the larger of that and 2e-4; running buffers 1e-4).
  * emul: the same kernel sources through the TEST-ONLY SIMT emulator
  * gpu : libconvnet_hip.so on a real MI355X
The fixture stores seeds, not inputs, and up to 2048 samples of every returned tensor (make_golden.sample_tensor); the
whole tensors are checked here against a float64 closed form that the same samples pin to the reference."""
import math
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import GOLDEN, int_tensor, rel_l2, sample_index

MODES = ['emul', pytest.param('gpu', marks=pytest.mark.gpu)]
K = math.sqrt(math.pi / 2)
_FIX = {}


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    import convnet_amd as ca
    assert ca._lib.is_emulated() == (mode == 'emul')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _fixture():
    if not _FIX:
        _FIX.update(torch.load(os.path.join(GOLDEN, 'l1bn_ops.pt')))
    return _FIX


def _inputs(shape, has_res, seed):
    """tools/make_golden_l1bn.py:op_inputs restated: NCHW float64 values that are exact in bf16, f16 and fp32."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(seed)

    def draw(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).bfloat16().double()
    y = (draw(N, C, H, W, scale=1.5) + draw(1, C, 1, 1, scale=0.5)).bfloat16().double()
    gamma = (torch.rand(C, generator=g) + 0.5).bfloat16().double()
    beta = draw(C, scale=0.3)
    res = draw(N, C, H, W) if has_res else None
    dz = draw(N, C, H, W)
    return y, gamma, beta, res, dz


def closed_form(y, gamma, beta, res, dz, relu, eps=1e-5, momentum=0.1):
    """The reference's semantics in float64 on NCHW tensors, sign(0) = 0."""
    C = y.shape[1]
    v = lambda t: t.view(1, C, 1, 1)
    M = y.numel() // C
    mu = y.mean((0, 2, 3))
    d = y - v(mu)
    V = d.abs().mean((0, 2, 3))
    s = 1.0 / (V * K + eps)
    xhat = d * v(s)
    z = xhat * v(gamma) + v(beta)
    if res is not None:
        z = z + res
    g = dz * (z > 0) if relu else dz
    if relu:
        z = z.clamp_min(0)
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xhat).sum((0, 2, 3))
    sg = torch.sign(d)
    dy = v(gamma * s) * ((g - v(dbeta / M)) - K * v(dgamma / M) * (sg - v(sg.mean((0, 2, 3)))))
    return {'z': z, 'dy': dy, 'dres': g if res is not None else None, 'dgamma': dgamma, 'dbeta': dbeta,
            'running_mean': mu * (1 - momentum), 'running_var': s * (1 - momentum), 'mu': mu, 's': s}


def _nhwc(t, dtype, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def _nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


def _module(C, gamma, beta, dtype, dev):
    import convnet_amd as ca
    bn = ca.nn.L1BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(gamma.float())
        bn.bias.copy_(beta.float())
    ca.engine.prepare(torch.nn.Sequential(bn), dev, dtype)
    return bn


def _train_call(bn, y, res, dz, relu, dtype, dev):
    """One training-mode forward + backward of the module; returns NCHW fp32 copies."""
    bn.train()
    bn.grad_view('weight').zero_()
    bn.grad_view('bias').zero_()
    yh = _nhwc(y, dtype, dev).requires_grad_(True)
    rh = _nhwc(res, dtype, dev).requires_grad_(True) if res is not None else None
    z = bn(yh, residual=rh, relu=bool(relu))
    z.backward(_nhwc(dz, dtype, dev))
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return {'z': _nchw(z), 'dy': _nchw(yh.grad), 'dres': _nchw(rh.grad) if rh is not None else None,
            'dgamma': bn.grad_view('weight').detach().float().cpu().clone(),
            'dbeta': bn.grad_view('bias').detach().float().cpu().clone(),
            'running_mean': bn.running_mean.detach().float().cpu().clone(),
            'running_var': bn.running_var.detach().float().cpu().clone()}


def _tols(dtype):
    fwd = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype]
    grad = 1e-4 if dtype == torch.float32 else 1.5e-2
    return fwd, grad, max(grad, 2e-4)


def _sampled(t, name):
    t = t.contiguous().flatten()
    return t[sample_index(name, t.numel())]


def _check_record(rec, dtype, dev):
    shape = tuple(rec['shape'])
    N, H, W, C = shape
    y, gamma, beta, res, dz = _inputs(shape, rec['has_res'], rec['seed'])
    sums = [float(t.sum()) for t in (y, gamma, beta, dz)] + ([float(res.sum())] if res is not None else [])
    assert sums == pytest.approx(rec['input_sums'], rel=1e-12, abs=1e-12)      # the seeded generator reproduces the inputs
    ref = closed_form(y, gamma, beta, res, dz, rec['relu'])
    # the closed form IS the reference module (float64 against float64: rounding only)
    for k in ('z', 'dy', 'dres'):
        if rec[k] is not None:
            assert rel_l2(_sampled(ref[k], k), rec[k]['val']) < 1e-6, k
            assert float(ref[k].norm()) == pytest.approx(rec[k]['norm'], rel=1e-6), k
    for k in ('dgamma', 'dbeta', 'running_mean', 'running_var'):
        assert rel_l2(ref[k], rec[k]) < 1e-6, k
    # both sides see the inputs rounded to the compute dtype: bf16 and fp32 hold them exactly, f16 all but the few of
    # magnitude below 2^-14
    rounded = [t.to(dtype).double() if t is not None else None for t in (y, gamma, beta, res, dz)]
    if any(t is not None and not torch.equal(t, r) for t, r in zip((y, gamma, beta, res, dz), rounded)):
        assert dtype == torch.float16
        y, gamma, beta, res, dz = rounded
        ref = closed_form(y, gamma, beta, res, dz, rec['relu'])
    bn = _module(C, gamma, beta, dtype, dev)
    assert list(bn.state_dict().keys()) == _fixture()['state_dict_keys']
    assert not any('num_batches_tracked' in k for k in bn.state_dict())
    out = _train_call(bn, y, res, dz, rec['relu'], dtype, dev)
    fwd, grad, pgrad = _tols(dtype)
    what = (shape, rec['relu'], rec['has_res'], dtype)
    errs = {'z': (rel_l2(out['z'], ref['z']), fwd), 'dy': (rel_l2(out['dy'], ref['dy']), grad),
            'dgamma': (rel_l2(out['dgamma'], ref['dgamma']), pgrad), 'dbeta': (rel_l2(out['dbeta'], ref['dbeta']), pgrad),
            'running_mean': (rel_l2(out['running_mean'], rec['running_mean']), 1e-4),
            'running_var': (rel_l2(out['running_var'], rec['running_var']), 1e-4),
            'z vs fixture': (rel_l2(_sampled(out['z'], 'z'), rec['z']['val']), fwd),
            'dy vs fixture': (rel_l2(_sampled(out['dy'], 'dy'), rec['dy']['val']), grad),
            'dgamma vs fixture': (rel_l2(out['dgamma'], rec['dgamma']), pgrad),
            'dbeta vs fixture': (rel_l2(out['dbeta'], rec['dbeta']), pgrad)}
    if res is not None:
        errs['dres'] = (rel_l2(out['dres'], ref['dres']), grad)
        errs['dres vs fixture'] = (rel_l2(_sampled(out['dres'], 'dres'), rec['dres']['val']), grad)
    # eval mode from the running buffers the training call left (0.9 x the batch statistics: buffers start at 0)
    bn.eval()
    with torch.no_grad():
        ze = bn(_nhwc(y, dtype, dev), residual=_nhwc(res, dtype, dev) if res is not None else None, relu=bool(rec['relu']))
    errs['z_eval'] = (rel_l2(_sampled(_nchw(ze), 'z_eval'), rec['z_eval']['val']), fwd)
    print('l1bn %s: %s' % (what, {k: '%.2e' % e for k, (e, _) in errs.items()}))
    missed = [(what, k, e, tol) for k, (e, tol) in errs.items() if not e < tol]
    # a second identical call: bit-identical z, dy, dgamma (fixed-order reductions, no atomics)
    bn2 = _module(C, gamma, beta, dtype, dev)
    out2 = _train_call(bn2, y, res, dz, rec['relu'], dtype, dev)
    for k in ('z', 'dy', 'dgamma'):
        assert torch.equal(out[k], out2[k]), (what, k)
    return missed


def _records(shape):
    recs = [r for r in _fixture()['records'] if tuple(r['shape']) == tuple(shape)]
    assert recs, shape
    return recs


# (N, H, W, C): the smallest shapes that reach each code path
SHAPES = [
    (2, 1, 1, 8),        # M = 2: less than one pass
    (3, 7, 5, 24),       # three bf16 chunks in a four-lane row slice (one lane column idle), M = 105: a ragged last pass
    (2, 9, 9, 64),
    (1, 37, 1, 1040),    # fp32: 260 chunks, a second column group
    (4, 28, 28, 16),     # M = 3136: the four-deep unrolled loop and its tail over several row blocks
    (2, 56, 56, 8),      # one chunk column, many row blocks
]
_ID = lambda s: 'x'.join(map(str, s))


def test_fixture_covers_the_shapes():
    fix = _fixture()
    assert fix['state_dict_keys'] == ['bias', 'weight', 'running_mean', 'running_var']
    for shape in SHAPES:
        combos = sorted((r['relu'], r['has_res']) for r in _records(shape))
        if shape[0] * shape[1] * shape[2] * shape[3] <= 4096:
            assert combos == [(0, 0), (1, 0), (1, 1)], (shape, combos)
        else:
            assert len(combos) == 1, (shape, combos)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ID)
def test_against_reference_module(mode, dtype, shape):
    """(2, 1, 1, 8) runs on the float64 path of csrc/l1bn.hip (M <= 32 values per channel): with two values per channel the
    two terms of dy cancel to eps*s (~1e-5) of their size, and fp32 sums and coefficients leave dy 6e-4 .. 2e-3 off."""
    dev = _dev(mode)
    if mode == 'emul' and dtype == torch.float16 and shape not in ((3, 7, 5, 24), (2, 9, 9, 64)):
        pytest.skip('f16 on the emulator: a subset, as in test_ops.py')
    if shape[3] == 1040 and dtype != torch.float32:
        pytest.skip('260 chunks: the fp32 case (130 chunks in 16 bits stay in one column group)')
    missed = []
    for rec in _records(shape):      # (every record is run and printed before the bounds are asserted)
        missed += _check_record(rec, dtype, dev)
    assert not missed, missed


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(1, 1, 3, 8), (2, 4, 4, 16), (1, 3, 11, 8)], ids=_ID)
def test_few_values_per_channel(mode, dtype, shape):
    """Both sides of the M = 32 threshold between the float64 path and the streaming kernels (M = 3, 32, 33), every (relu,
    residual) combination, against the float64 closed form with the bounds of the reference-module test."""
    dev = _dev(mode)
    N, H, W, C = shape
    fwd, grad, pgrad = _tols(dtype)
    for i, (relu, has_res) in enumerate([(0, 0), (1, 0), (1, 1)]):
        y, gamma, beta, res, dz = _inputs(shape, has_res, 900 + i)
        ref = closed_form(y, gamma, beta, res, dz, relu)
        out = _train_call(_module(C, gamma, beta, dtype, dev), y, res, dz, relu, dtype, dev)
        errs = {'z': (rel_l2(out['z'], ref['z']), fwd), 'dy': (rel_l2(out['dy'], ref['dy']), grad),
                'dgamma': (rel_l2(out['dgamma'], ref['dgamma']), pgrad), 'dbeta': (rel_l2(out['dbeta'], ref['dbeta']), pgrad),
                'running_mean': (rel_l2(out['running_mean'], ref['running_mean']), 1e-4),
                'running_var': (rel_l2(out['running_var'], ref['running_var']), 1e-4)}
        if has_res:
            errs['dres'] = (rel_l2(out['dres'], ref['dres']), grad)
        print('l1bn small %s: %s' % ((shape, relu, has_res, dtype), {k: '%.2e' % e for k, (e, _) in errs.items()}))
        for k, (e, tol) in errs.items():
            assert e < tol, (shape, relu, has_res, dtype, k, e, tol)


@pytest.mark.parametrize('mode', MODES)
def test_exact_integer_data(mode):
    """Integers in [-3, 3], half of them zero, M = 64 (a power of two): mu and every sum are exact in fp32.  Channel 0 is
    symmetric (mu = 0 exactly, its zeros sit ON the mean), channel 1 is constant 0.5 (V = 0)."""
    dev = _dev(mode)
    N, H, W, C = 2, 4, 8, 8
    M = N * H * W
    gen = torch.Generator().manual_seed(7)
    y = int_tensor((N, C, H, W), gen)                 # float64 integers, density 0.5
    half = int_tensor((M // 2,), gen)
    y[:, 0] = torch.cat([half, -half])[torch.randperm(M, generator=gen)].view(N, H, W)
    y[:, 1] = 0.5
    assert float(y[:, 0].sum()) == 0.0
    on_mean = int((y[:, 0] == 0).sum())
    assert 4 * on_mean >= M, 'premise: at least a quarter of the symmetric channel sits exactly on its mean (%d of %d)' % (on_mean, M)
    gamma = (torch.rand(C, generator=gen) + 0.5).double()
    gamma = gamma.float().double()
    beta = (torch.randn(C, generator=gen) * 0.3).float().double()
    dz = int_tensor((N, C, H, W), gen, density=1.0)
    ref = closed_form(y, gamma, beta, None, dz, relu=0)
    bn = _module(C, gamma, beta, torch.float32, dev)
    out = _train_call(bn, y, None, dz, 0, torch.float32, dev)
    mu32 = ref['mu'].float()
    assert torch.equal(mu32.double(), ref['mu'])      # k / 64: exact
    assert torch.equal(out['running_mean'], mu32 * torch.tensor(0.9, dtype=torch.float32)), (out['running_mean'], mu32)
    assert float(out['running_mean'][0]) == 0.0
    # the constant channel: z == beta exactly, finite gradients
    assert torch.equal(out['z'][:, 1], beta[1].float().expand(N, H, W)), (out['z'][:, 1].flatten()[:4], beta[1])
    for k in ('z', 'dy', 'dgamma', 'dbeta', 'running_var'):
        assert bool(torch.isfinite(out[k]).all()), k
    # the symmetric channel: sign(0) = 0 (a kernel that takes y >= mu as +1 is off by ~1/sqrt(M) here)
    e = rel_l2(out['dy'][:, 0], ref['dy'][:, 0])
    print('exact data: dy rel-L2 on the symmetric channel %.2e, whole tensor %.2e' % (e, rel_l2(out['dy'][:, [0] + list(range(2, C))], ref['dy'][:, [0] + list(range(2, C))])))
    assert e < 1e-4
    wrong = closed_form(y, gamma, beta, None, dz, relu=0)
    sg = torch.where(y[:, 0] >= 0, 1.0, -1.0).double()
    s0, g0 = wrong['s'][0], dz[:, 0]
    dy_wrong = gamma[0] * s0 * ((g0 - g0.mean()) - K * (wrong['dgamma'][0] / M) * (sg - sg.mean()))
    assert rel_l2(dy_wrong, ref['dy'][:, 0]) > 1e-2      # ... and this data tells the two apart
    keep = [c for c in range(C) if c != 1]
    assert rel_l2(out['z'][:, keep], ref['z'][:, keep]) < 1e-5
    assert rel_l2(out['dy'][:, keep], ref['dy'][:, keep]) < 1e-4


@pytest.mark.parametrize('mode', MODES)
def test_statistics_only_and_c_abi_refusals(mode):
    """z == NULL: the statistics call writes stats and both running buffers and touches nothing else; bad shapes and a
    short workspace are refused before any launch."""
    dev = _dev(mode)
    import convnet_amd as ca
    from convnet_amd import ops
    lib = ca._lib
    L = lib.load()
    N, H, W, C = 3, 7, 5, 24
    M = N * H * W
    y, gamma, beta, _, dz = _inputs((N, H, W, C), False, 5)
    ref = closed_form(y, gamma, beta, None, dz, 0)
    yh = _nhwc(y, torch.float32, dev)
    g32, b32 = gamma.float().to(dev), beta.float().to(dev)
    rm, rv = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    stats = torch.zeros(7 * C, device=dev)
    ws = ops.workspace(L.cn_l1bn_workspace(M, C, 0), dev)
    L.cn_l1bn_fwd_train(lib.ptr(yh), None, None, None, lib.ptr(g32), lib.ptr(b32), lib.ptr(rm), lib.ptr(rv), 0.1, 1e-5,
                        lib.ptr(stats), M, C, 0, 0, lib.ptr(ws), ws.numel() * 4, lib.stream_of(yh))
    st = stats.cpu().double().view(7, C)
    assert rel_l2(st[0], ref['mu']) < 1e-5 and rel_l2(st[1], ref['s']) < 1e-5
    assert rel_l2(st[2], gamma * ref['s']) < 1e-5 and torch.equal(st[3], beta)
    assert rel_l2(rv.cpu(), ref['running_var']) < 1e-4
    with pytest.raises(lib.ConvNetHipError):
        L.cn_l1bn_fwd_train(lib.ptr(yh), None, None, None, lib.ptr(g32), lib.ptr(b32), None, None, 0.1, 1e-5,
                            lib.ptr(stats), M, C + 1, 0, 0, lib.ptr(ws), ws.numel() * 4, lib.stream_of(yh))
    with pytest.raises(lib.ConvNetHipError):
        L.cn_l1bn_fwd_train(lib.ptr(yh), None, None, None, lib.ptr(g32), lib.ptr(b32), None, None, 0.1, 1e-5,
                            lib.ptr(stats), M, C, 0, 0, lib.ptr(ws), 16, lib.stream_of(yh))
    assert L.cn_l1bn_workspace(M, C + 1, 0) == 0


def test_module_refuses_what_is_not_built():
    import convnet_amd as ca
    for kw in (dict(noise=True), dict(normalized=False)):
        with pytest.raises(NotImplementedError):
            ca.nn.L1BatchNorm2d(8, **kw)
    bn = ca.nn.L1BatchNorm2d(8, momentum=0.1, eps=1e-5)
    assert not isinstance(bn, ca.nn.BatchNorm2d)
    assert float(bn.running_var.sum()) == 0.0 and float(bn.weight.detach().sum()) == 8.0
