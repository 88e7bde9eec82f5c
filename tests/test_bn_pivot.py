"""nn.BatchNorm2d.batch_pivot (fp32 storage) -> cn_bn_fwd_train_pivot (csrc/bn.hip): the one-pass fp32 statistics centred on an
estimate of the batch mean (bn_pivot_kernel: the mean of up to 256 rows spread over the tensor) instead of the running
mean, which is 0 at a cold start.  The data here has channel means of up to 30 standard deviations - sums centred on 0
would lose a factor 1 + 30^2 of the variance's precision - and the module is fresh (running mean 0).

Bounds (float64 oracle on inputs rounded to the compute dtype):
  * batch variance, read back through running_var (0.9 + 0.1 * unbiased): rel 2e-5.  A lane adds <= 64 terms, the workgroup
    <= 8 more, the rest is float64: <= 72 * 2^-24 = 4.3e-6, times 1 + (pivot - mean)^2 / var <= 2, plus the fp32 rounding of
    running_var itself (1.2e-6 of a variance near 1);
  * batch mean through running_mean: 2^-22 relative + 1e-6;
  * z: rel-L2 1e-5 in fp32 (tests/test_ops.py's bound), 4e-3 in bf16 / f16 storage; dy (fp32): 1e-4 (tests/test_gconv.py's
    gradient bound).
The module takes this path for fp32 tensors only (behind the rounding of a 16-bit tensor the gain cannot be seen); the
library call is checked for all three storage types."""
import pytest
import torch
import torch.nn.functional as F

from conftest import HAS_GPU
from helpers import rel_l2

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
# (N, H, W, C): fewer rows than the pivot sample; more, and no multiple of it; more than 256 fp32 chunk columns (two
# column groups) on 18 rows
SHAPES = [(2, 5, 7, 8), (3, 17, 19, 24), (2, 3, 3, 1032)]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _case(shape, dtype):
    """Inputs rounded to the storage type (NCHW) and the float64 result: z, dy, running mean / variance after one step."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(C + N * H * W)
    offs = torch.linspace(-30.0, 30.0, C).view(1, C, 1, 1)
    y0 = (torch.randn(N, C, H, W, generator=g) + offs).to(dtype).float()
    gamma0, beta0 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dz0 = torch.randn(N, C, H, W, generator=g).to(dtype).float()
    yr = y0.double().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    zr = F.relu(F.batch_norm(yr, rm, rv, gamma0.double(), beta0.double(), True, 0.1, 1e-5))
    zr.backward(dz0.double())
    return y0, gamma0, beta0, dz0, zr.detach(), yr.grad, rm, rv


def _stat_errors(running_mean, running_var, rm, rv):
    var, var_ref = (running_var.cpu().double() - 0.9) / 0.1, (rv - 0.9) / 0.1
    return (((var - var_ref).abs() / var_ref).max().item(),
            ((running_mean.cpu().double() - rm).abs() - rm.abs() * 2.0 ** -22).max().item())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_module_cold_start_statistics_of_an_offset_tensor(mode, shape):
    dev = _dev(mode)
    import convnet_amd as ca
    dtype = torch.float32
    N, H, W, C = shape
    y0, gamma0, beta0, dz0, zr, dyr, rm, rv = _case(shape, dtype)
    calls = []
    L = ca.ops._L()
    real = L.cn_bn_fwd_train_pivot

    bn = ca.nn.BatchNorm2d(C)
    assert bn.batch_pivot is False
    bn.batch_pivot = True
    model = torch.nn.Sequential(bn)
    ca.engine.prepare(model, dev, dtype)
    bn.weight.data.copy_(gamma0.to(dev))
    bn.bias.data.copy_(beta0.to(dev))
    bn.train()
    L.cn_bn_fwd_train_pivot = lambda *a: (calls.append(1), real(*a))[1]
    try:
        z, y = _fwd_bwd(bn, model, y0, dz0, dtype, dev)
    finally:
        L.cn_bn_fwd_train_pivot = real
    assert calls == [1]
    e_var, e_mean = _stat_errors(bn.running_mean, bn.running_var, rm, rv)
    e_z = rel_l2(z.detach().float().cpu().permute(0, 3, 1, 2), zr.float())
    e_dy = rel_l2(y.grad.float().cpu().permute(0, 3, 1, 2), dyr.float())
    print('module', shape, 'var', e_var, 'mean', e_mean, 'z', e_z, 'dy', e_dy)
    assert e_var < 2e-5 and e_mean < 1e-6 and e_z < 1e-5 and e_dy < 1e-4
    assert int(bn.num_batches_tracked) == 1
    # 16-bit storage: the module keeps the plain statistics pass
    bn16 = ca.nn.BatchNorm2d(C)
    bn16.batch_pivot = True
    m16 = torch.nn.Sequential(bn16)
    ca.engine.prepare(m16, dev, torch.bfloat16)
    bn16.train()
    L.cn_bn_fwd_train_pivot = lambda *a: (calls.append(1), real(*a))[1]
    try:
        _fwd_bwd(bn16, m16, y0, dz0, torch.bfloat16, dev)
    finally:
        L.cn_bn_fwd_train_pivot = real
    assert calls == [1]


def _fwd_bwd(bn, model, y0, dz0, dtype, dev):
    y = y0.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev).requires_grad_(True)
    z = bn(y, relu=True)
    model._cn_arena.zero_grad()
    z.backward(dz0.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev))
    return z, y


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_library_call_in_every_storage_type(mode, dtype, shape):
    dev = _dev(mode)
    import convnet_amd as ca
    from convnet_amd._lib import dtype_code, ptr, stream_of
    L = ca.ops._L()
    N, H, W, C = shape
    M = N * H * W
    y0, gamma0, beta0, dz0, zr, dyr, rm, rv = _case(shape, dtype)
    y = y0.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    z = torch.empty_like(y)
    f32 = dict(dtype=torch.float32, device=dev)
    gamma, beta = gamma0.to(dev), beta0.to(dev)
    running_mean, running_var = torch.zeros(C, **f32), torch.ones(C, **f32)
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    stats, pivot = torch.empty(4 * C, **f32), torch.full((C,), float('nan'), **f32)
    code = dtype_code(dtype)
    ws = torch.empty(L.cn_bn_workspace(M, C, code) // 4 + 1, **f32)
    L.cn_bn_fwd_train_pivot(ptr(y), None, ptr(z), None, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(nbt),
                            0.1, 1e-5, ptr(stats), ptr(pivot), M, C, 1, code, ptr(ws), ws.numel() * 4, stream_of(y))
    e_var, e_mean = _stat_errors(running_mean, running_var, rm, rv)
    e_z = rel_l2(z.float().cpu().permute(0, 3, 1, 2), zr.float())
    # the pivot is an estimate of the mean, not the mean: within one deviation (sigma = 1 here) for every channel
    e_piv = (pivot.cpu().double() - rm / 0.1).abs().max().item()
    print('call', shape, dtype, 'var', e_var, 'mean', e_mean, 'z', e_z, 'pivot', e_piv)
    assert e_var < 2e-5 and e_mean < 1e-6 and e_piv < 1.0
    assert e_z < (1e-5 if dtype == torch.float32 else 4e-3)
    assert int(nbt) == 1


def test_mobilenet_turns_it_on_and_nothing_else_does():
    import convnet_amd as ca
    m = ca.models.mobilenet(width=0.25, shallow=True, num_classes=16)
    bns = [x for x in m.modules() if isinstance(x, ca.nn.BatchNorm2d)]
    assert len(bns) == 17 and all(x.batch_pivot for x in bns)
    r = ca.models.resnet(depth=18, num_classes=16)
    assert not any(getattr(x, 'batch_pivot', False) for x in r.modules())
