"""Grouped 3x3 convolution kernels (csrc/gconv.hip) against F.conv2d(..., groups=g) on fp32 inputs rounded to the compute
dtype, with the rel-L2 bounds of test_ops.py (bf16 1e-2, f16 2e-3, fp32 1e-5 forward / 1e-4 gradients).
  * emul: the same kernel sources through the TEST-ONLY SIMT emulator, small shapes
  * gpu : libconvnet_hip.so on a real MI355X, every ResNeXt-50 / ResNeXt-18 grouped shape"""
import pytest
import torch
import torch.nn.functional as F

from conftest import HAS_GPU
from helpers import assert_within_forward_bound, rel_l2

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    import convnet_amd as ca
    assert ca._lib.is_emulated() == (mode == 'emul')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _tol(dtype, grad=False):
    if dtype == torch.bfloat16:
        return 1e-2
    if dtype == torch.float16:
        return 2e-3
    return 1e-4 if grad else 1e-5


def _case(N, H, W, C, K, g, st, dtype, dev, seed=0):
    """Inputs rounded to the compute dtype; returns (x_nhwc, w_krsc, dy_nhwc, references fwd / dgrad / wgrad)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen).to(dtype).float()
    w = (torch.randn(K, C // g, 3, 3, generator=gen) / (9 * C // g) ** 0.5).to(dtype).float()
    P, Q = (H - 1) // st + 1, (W - 1) // st + 1
    dy = torch.randn(N, K, P, Q, generator=gen).to(dtype).float()
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=st, padding=1, groups=g)
    y.backward(dy.double())
    xh = x.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    wh = w.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    dyh = dy.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    return xh, wh, dyh, y.detach(), xr.grad, wr.grad


def _run(N, H, W, C, K, g, st, dtype, dev, beta_check=False):
    from convnet_amd import ops
    xh, wh, dyh, y_ref, dx_ref, dw_ref = _case(N, H, W, C, K, g, st, dtype, dev)
    y = ops.gconv2d_fwd(xh, wh, K, g, st)
    assert rel_l2(y.float().cpu().permute(0, 3, 1, 2), y_ref) < _tol(dtype), ('fwd', N, H, W, C, K, g, st, dtype)
    dx = ops.gconv2d_dgrad(dyh, wh, xh.shape, K, g, st)
    assert rel_l2(dx.float().cpu().permute(0, 3, 1, 2), dx_ref) < _tol(dtype, True), ('dgrad', N, H, W, C, K, g, st, dtype)
    dw = torch.full((K * 9 * (C // g),), float('nan'), device=dev)     # beta = 0 must not read the old contents
    ops.gconv2d_wgrad(xh, dyh, dw, K, g, st, beta=0.0)
    dw_k = dw.cpu().view(K, 3, 3, C // g).permute(0, 3, 1, 2)
    assert rel_l2(dw_k, dw_ref) < _tol(dtype, True), ('wgrad', N, H, W, C, K, g, st, dtype)
    # beside the norms: every element within the forward error bound of an fp32 dot product plus one output rounding,
    # against the fp64 reference and its magnitude sums (the same operation on the absolute values)
    xa, wa, da = [t.double().cpu().permute(0, 3, 1, 2).abs() for t in (xh, wh, dyh)]
    what = str((N, H, W, C, K, g, st, dtype))
    ratios = (assert_within_forward_bound(y.cpu().permute(0, 3, 1, 2), y_ref, F.conv2d(xa, wa, stride=st, padding=1, groups=g),
                                          9 * (C // g), dtype, 'gconv fwd ' + what),
              assert_within_forward_bound(dx.cpu().permute(0, 3, 1, 2), dx_ref,
                                          torch.nn.grad.conv2d_input(xa.shape, wa, da, stride=st, padding=1, groups=g),
                                          9 * (K // g), dtype, 'gconv dgrad ' + what),
              assert_within_forward_bound(dw_k, dw_ref,
                                          torch.nn.grad.conv2d_weight(xa, wa.shape, da, stride=st, padding=1, groups=g),
                                          dyh.numel() // K, torch.float32, 'gconv wgrad ' + what))
    print('gconv max |err| / bound (fwd, dgrad, wgrad) %s: %.3g %.3g %.3g' % ((what,) + ratios))
    if beta_check:
        dw2 = dw.clone()
        ops.gconv2d_wgrad(xh, dyh, dw2, K, g, st, beta=1.0, scale=0.5)
        assert rel_l2(dw2.cpu(), 1.5 * dw.cpu()) < 1e-6
    return xh, wh, dyh, y, dx, dw


# (N, H, W, C, K, groups, stride): C/g, K/g in {1, 2, 4, 8, ...}, unequal widths, odd maps, partial pixel tiles
EMUL_CASES = [
    (1, 5, 7, 8, 8, 2, 1),       # (4, 4)
    (2, 7, 5, 16, 16, 4, 2),     # (4, 4) stride 2, odd map
    (1, 6, 6, 8, 16, 4, 1),      # (2, 4): K/g != C/g
    (1, 5, 5, 16, 8, 4, 2),      # (4, 2)
    (1, 4, 5, 8, 8, 8, 1),       # depthwise (1, 1)
    (1, 3, 3, 16, 32, 8, 1),     # (2, 4), several groups per block
    (1, 5, 3, 64, 64, 2, 2),     # (32, 32) stride 2
]


@pytest.mark.parametrize('case', EMUL_CASES, ids=lambda c: 'N%d_%dx%d_C%d_K%d_g%d_s%d' % c)
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_gconv_emul(case, dtype):
    dev = _dev('emul')
    _run(*case, dtype, dev, beta_check=case == EMUL_CASES[0])


def test_gconv_emul_wide_groups():
    """64 rows per group: a group spans two row blocks (C/g = K/g = 64), and (64, 32) / (32, 64) unequal widths."""
    dev = _dev('emul')
    _run(1, 3, 4, 128, 128, 2, 1, torch.bfloat16, dev)
    _run(1, 3, 3, 128, 64, 2, 2, torch.bfloat16, dev)
    _run(1, 3, 3, 64, 128, 2, 1, torch.float32, dev)


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_gconv_unaligned_group_rows(mode, dtype):
    """34 rows per group: the second row block of a group starts at g*34 + 32, not a multiple of 4 (element stores)."""
    dev = _dev(mode)
    _run(1, 3, 5, 272, 272, 8, 1, dtype, dev)
    _run(1, 4, 3, 272, 272, 8, 2, dtype, dev)


def _shapes_resnext(N, big=False):
    """Every grouped 3x3 of ResNeXt-50 32x4d (H, C=K, groups=32, stride: the first block of a stage strides) and of
    ResNeXt-18 (BasicBlock, expansion 2: (C, K) per group from (2, 4) up to (64, 32) / (32, 64)) at N images."""
    rx50 = [(56, 128, 128, 32, 1), (56, 256, 256, 32, 2), (28, 256, 256, 32, 1), (28, 512, 512, 32, 2),
            (14, 512, 512, 32, 1), (14, 1024, 1024, 32, 2), (7, 1024, 1024, 32, 1)]
    rx18 = [(56, 64, 128, 32, 1), (56, 256, 128, 32, 1), (56, 256, 256, 32, 2), (28, 256, 512, 32, 1),
            (28, 512, 512, 32, 2), (14, 512, 1024, 32, 1), (14, 1024, 1024, 32, 2), (7, 1024, 2048, 32, 1),
            (7, 2048, 1024, 32, 1)]
    return [(N, H, H, C, K, g, st) for H, C, K, g, st in rx50 + rx18]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_gconv_gpu_resnext_shapes(dtype):
    dev = _dev('gpu')
    for case in _shapes_resnext(2):
        _run(*case, dtype, dev, beta_check=case[1] == 56 and case[6] == 1)
    for case in EMUL_CASES:
        _run(*case, dtype, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_gconv_gpu_b256(dtype):
    """The three 56x56 / 28x28 ResNeXt-50 grouped shapes at the training batch."""
    dev = _dev('gpu')
    for H, C, st in ((56, 128, 1), (56, 256, 2), (28, 256, 1)):
        _run(256, H, H, C, C, 32, st, dtype, dev)


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_gconv_deterministic(mode):
    """Two identical calls give identical bytes (the weight gradient's split reduction has a fixed order)."""
    dev = _dev(mode)
    N, H = (1, 6) if mode == 'emul' else (32, 56)
    a = _run(N, H, H, 32, 32, 8, 2, torch.bfloat16, dev)
    b = _run(N, H, H, 32, 32, 8, 2, torch.bfloat16, dev)
    for t, u in zip(a[3:], b[3:]):
        assert torch.equal(t.cpu().view(torch.uint8) if t.dtype != torch.float32 else t.cpu(),
                           u.cpu().view(torch.uint8) if u.dtype != torch.float32 else u.cpu())


def test_gconv_refuses_unsupported():
    import convnet_amd as ca
    from convnet_amd import _lib, ops
    f32, bf = torch.float32, torch.bfloat16
    ok = ops.gconv2d_ok
    assert ok(128, 128, 32, (3, 3), (1, 1), (1, 1), bf) and ok(256, 256, 32, (3, 3), (2, 2), (1, 1), f32)
    assert not ok(128, 128, 32, (1, 1), (1, 1), (0, 0), bf)          # not 3x3
    assert not ok(128, 128, 32, (3, 3), (3, 3), (1, 1), bf)          # stride 3
    assert not ok(128, 128, 32, (3, 3), (1, 1), (0, 0), bf)          # padding 0
    assert not ok(128, 128, 32, (3, 3), (1, 2), (1, 1), bf)          # unequal strides
    assert not ok(130, 128, 32, (3, 3), (1, 1), (1, 1), bf)          # groups do not divide C
    assert not ok(256, 256, 2, (3, 3), (1, 1), (1, 1), bf)           # 128 channels per group
    assert not ok(12, 12, 3, (3, 3), (1, 1), (1, 1), bf)             # C not a multiple of the 16-bit chunk
    assert ok(12, 12, 3, (3, 3), (1, 1), (1, 1), f32)
    dev = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
    x = torch.zeros(1, 4, 4, 256, dtype=bf, device=dev)
    w = torch.zeros(256 * 9 * 128, dtype=bf, device=dev)
    with pytest.raises(_lib.ConvNetHipError):
        ops.gconv2d_fwd(x, w, 256, 2, 1)
    # module level: every grouped configuration but ResNeXt's 3x3 is refused at construction
    for kw in (dict(kernel_size=1), dict(kernel_size=3, padding=0), dict(kernel_size=3, padding=1, stride=3),
               dict(kernel_size=3, padding=1, bias=True), dict(kernel_size=3, padding=1, dilation=2)):
        kw.setdefault('bias', False)
        with pytest.raises(NotImplementedError):
            ca.nn.Conv2d(64, 64, groups=8, **kw)
    with pytest.raises(NotImplementedError):
        ca.nn.Conv2d(256, 256, 3, padding=1, groups=2, bias=False)     # 128 channels per group


def test_grouped_conv2d_module_matches_torch_init_and_shape():
    """Weight shape [K, C/g, 3, 3] and the RNG use of torch.nn.Conv2d (seeded construction gives the same weights)."""
    import convnet_amd as ca
    torch.manual_seed(7)
    ours = ca.nn.Conv2d(64, 128, 3, stride=2, padding=1, groups=16, bias=False)
    torch.manual_seed(7)
    ref = torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, groups=16, bias=False)
    assert ours.weight.shape == (128, 4, 3, 3)
    assert torch.equal(ours.weight.data, ref.weight.data)
    torch.manual_seed(7)
    ca.nn.Conv2d(64, 128, 3, stride=2, padding=1, groups=16, bias=False)
    a = torch.rand(4)
    torch.manual_seed(7)
    torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, groups=16, bias=False)
    assert torch.equal(a, torch.rand(4))
