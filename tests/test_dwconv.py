"""Depthwise 3x3 convolution kernels (csrc/dwconv.hip) against F.conv2d(..., groups=C) in float64 on inputs rounded to the
compute dtype.
  * emul: the same kernel sources through the TEST-ONLY SIMT emulator, small shapes
  * gpu : libconvnet_hip.so on a real MI355X, the small shapes and every depthwise shape of MobileNet-1.0 at 224
Integer data (|x| <= 4, |w| <= 2, |dy| <= 4, |bias| <= 3): every sum is exact in fp32 and every forward / data-gradient
result is a bf16-representable integer (|y| <= 9*4*2 + 3 = 75, |dx| <= 72 < 256), so the results EQUAL the float64 ones in
all three dtypes.  Random data: the rel-L2 bounds of test_gconv.py (bf16 1e-2, f16 2e-3, fp32 1e-5 forward / 1e-4
gradients) and helpers.assert_within_forward_bound per element with reduction lengths 9, 9 and N*P*Q."""
import pytest
import torch
import torch.nn.functional as F

from conftest import HAS_GPU
from helpers import assert_same_values, assert_within_forward_bound, rel_l2

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
MODES = ['emul', pytest.param('gpu', marks=pytest.mark.gpu)]

# (N, H, W, C, stride)
SMALL = [
    (1, 1, 1, 8, 1),
    (1, 2, 2, 8, 2),
    (3, 5, 9, 24, 1),
    (3, 5, 9, 24, 2),       # odd map, 3 chunks
    (2, 7, 7, 40, 2),
    (1, 4, 13, 16, 1),      # W not a multiple of any run length
    (3, 17, 19, 8, 1),      # more than one weight-gradient partial, ragged last slab
]
# the 13 depthwise layers of MobileNet-1.0 at 224 (the 14 x 14 / 512 / stride-1 shape occurs five times): (H, C, stride)
MOBILENET = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2),
             (7, 1024, 1)]


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


def _reference(x, w, b, dy, st):
    """float64 forward / gradients of F.conv2d(groups=C); x, dy NCHW, w [C,1,3,3], b [C] or None."""
    C = x.shape[1]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if b is not None else None
    y = F.conv2d(xr, wr, br, stride=st, padding=1, groups=C)
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad, (br.grad if b is not None else None)


def _to_dev(x, w, dy, dtype, dev):
    C = x.shape[1]
    xh = x.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    wh = w.reshape(C, 9).t().contiguous().to(dtype).to(dev)      # tap-major [3][3][C]
    dyh = dy.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    return xh, wh, dyh


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


def _int_case(N, H, W, C, st, seed=0):
    g = torch.Generator().manual_seed(seed)
    P, Q = (H - 1) // st + 1, (W - 1) // st + 1
    x = torch.randint(-4, 5, (N, C, H, W), generator=g).float()
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).float()
    b = torch.randint(-3, 4, (C,), generator=g).float()
    dy = torch.randint(-4, 5, (N, C, P, Q), generator=g).float()
    return x, w, b, dy


def _exact(case, dtype, dev):
    from convnet_amd import ops
    N, H, W, C, st = case
    x, w, b, dy = _int_case(*case)
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, dy, st)
    assert float(dw_ref.abs().max()) < 2 ** 24
    xh, wh, dyh = _to_dev(x, w, dy, dtype, dev)
    what = '%s %s' % (case, dtype)
    y = ops.dwconv_fwd(xh, wh, b.to(dev), st)
    assert_same_values(_nchw(y), y_ref, dtype, 'dwconv fwd ' + what)
    dx = ops.dwconv_dgrad(dyh, wh, xh.shape, st)
    assert_same_values(_nchw(dx), dx_ref, dtype, 'dwconv dgrad ' + what)
    dw = torch.full((C * 9,), float('nan'), device=dev)       # beta = 0 must not read the old contents
    db = torch.full((C,), float('nan'), device=dev)
    ops.dwconv_wgrad(xh, dyh, dw, db, st, beta=0.0)
    assert_same_values(dw.cpu().view(C, 1, 3, 3), dw_ref, torch.float32, 'dwconv wgrad ' + what)
    assert_same_values(db.cpu(), db_ref, torch.float32, 'dwconv bias grad ' + what)
    # without a bias: the same forward minus b, and the weight gradient alone
    y0 = ops.dwconv_fwd(xh, wh, None, st)
    assert_same_values(_nchw(y0), y_ref - b.double().view(1, C, 1, 1), dtype, 'dwconv fwd (no bias) ' + what)
    dw0 = torch.full((C * 9,), float('nan'), device=dev)
    ops.dwconv_wgrad(xh, dyh, dw0, None, st, beta=0.0)
    assert torch.equal(dw0.cpu(), dw.cpu())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', SMALL, ids=lambda c: 'N%d_%dx%d_C%d_s%d' % c)
def test_dwconv_exact_on_integer_data(mode, dtype, case):
    dev = _dev(mode)
    _exact(case, dtype, dev)


def test_dwconv_wgrad_split_of_the_ragged_case():
    """(3, 17, 19, 8, 1): 51 output rows in slabs of 16 -> 4 partials, the last of 3 rows; one slab for the tiny shapes."""
    from convnet_amd import ops
    assert ops.dwconv_wgrad_split((3, 17, 19, 8), 1, torch.bfloat16) == 4
    assert ops.dwconv_wgrad_split((3, 17, 19, 8), 1, torch.float32) > 1
    assert ops.dwconv_wgrad_split((1, 4, 13, 16), 1, torch.bfloat16) == 1


def _random_case(N, H, W, C, st, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    P, Q = (H - 1) // st + 1, (W - 1) // st + 1
    x = torch.randn(N, C, H, W, generator=g).to(dtype).float()
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3.0).to(dtype).float()
    b = torch.randn(C, generator=g)
    dy = torch.randn(N, C, P, Q, generator=g).to(dtype).float()
    return x, w, b, dy


def _bound(out, ref64, A, n, out_dtype, what):
    """helpers.assert_within_forward_bound per element.  Its output-rounding term u_out*|ref| is the bound of a NORMAL
    number; an f16 result below 2^-14 is subnormal, where round-to-nearest is off by up to half the fixed spacing 2^-24
    whatever |ref| is.  Those elements (f16 only; bf16 and fp32 share fp32's exponent range) are held to
    2^-25 + 2*n*2^-24*A here and handed to the helper with the reference's own value."""
    out = out.detach().cpu().double()
    ref64, A = ref64.detach().cpu().double(), A.detach().cpu().double()
    if out_dtype == torch.float16:
        sub = ref64.abs() < 2.0 ** -14
        err = (out - ref64).abs()[sub]
        assert bool((err <= 2.0 ** -25 + 2.0 * n * 2.0 ** -24 * A[sub]).all()), what + ': f16 subnormal range'
        out = torch.where(sub, ref64, out)
    return assert_within_forward_bound(out, ref64, A, n, out_dtype, what)


def _random(case, dtype, dev, semantics=False):
    from convnet_amd import ops
    N, H, W, C, st = case
    x, w, b, dy = _random_case(N, H, W, C, st, dtype)
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, dy, st)
    xh, wh, dyh = _to_dev(x, w, dy, dtype, dev)
    what = '%s %s' % (case, dtype)
    y = ops.dwconv_fwd(xh, wh, b.to(dev), st)
    assert rel_l2(_nchw(y.float()), y_ref) < _tol(dtype), ('fwd', what)
    dx = ops.dwconv_dgrad(dyh, wh, xh.shape, st)
    assert rel_l2(_nchw(dx.float()), dx_ref) < _tol(dtype, True), ('dgrad', what)
    dw = torch.full((C * 9,), float('nan'), device=dev)
    db = torch.full((C,), float('nan'), device=dev)
    ops.dwconv_wgrad(xh, dyh, dw, db, st, beta=0.0)
    dw_k = dw.cpu().view(C, 1, 3, 3)
    assert rel_l2(dw_k, dw_ref) < _tol(dtype, True), ('wgrad', what)
    assert rel_l2(db.cpu(), db_ref) < _tol(dtype, True), ('bias grad', what)
    # per element: the forward error bound of an fp32 dot product plus one output rounding, against the float64
    # reference and its magnitude sums (the same operation on the absolute values)
    xa, wa, da, ba = x.double().abs(), w.double().abs(), dy.double().abs(), b.double().abs()
    npq = dy.numel() // C
    ratios = (_bound(_nchw(y), y_ref, F.conv2d(xa, wa, ba, stride=st, padding=1, groups=C), 9, dtype,
                                          'dwconv fwd ' + what),
              _bound(_nchw(dx), dx_ref,
                                          torch.nn.grad.conv2d_input(xa.shape, wa, da, stride=st, padding=1, groups=C), 9,
                                          dtype, 'dwconv dgrad ' + what),
              _bound(dw_k, dw_ref,
                                          torch.nn.grad.conv2d_weight(xa, wa.shape, da, stride=st, padding=1, groups=C), npq,
                                          torch.float32, 'dwconv wgrad ' + what),
              _bound(db.cpu(), db_ref, da.sum((0, 2, 3)), npq, torch.float32, 'dwconv bias grad ' + what))
    print('dwconv max |err| / bound (fwd, dgrad, wgrad, bias) %s: %.3g %.3g %.3g %.3g' % ((what,) + ratios))
    if semantics:
        dw2, db2 = dw.clone(), db.clone()
        ops.dwconv_wgrad(xh, dyh, dw2, db2, st, beta=1.0, scale=0.5)
        assert rel_l2(dw2.cpu(), 1.5 * dw.cpu()) < 1e-6 and rel_l2(db2.cpu(), 1.5 * db.cpu()) < 1e-6
        dw3, db3 = torch.full_like(dw, float('nan')), torch.full_like(db, float('nan'))
        ops.dwconv_wgrad(xh, dyh, dw3, db3, st, beta=0.0)                 # run twice: bit-identical
        assert torch.equal(dw3.cpu(), dw.cpu()) and torch.equal(db3.cpu(), db.cpu())
    return xh, wh, dyh, y, dx, dw


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dwconv_random_data(mode, dtype):
    dev = _dev(mode)
    for case in SMALL:
        _random(case, dtype, dev, semantics=case in (SMALL[3], SMALL[6]))


@pytest.mark.parametrize('mode', MODES)
def test_dwconv_matches_the_grouped_kernels(mode):
    """The parent's route for a bias-free depthwise layer, ops.gconv2d_* with groups = C, on one bf16 shape: rel-L2 within
    the bf16 bound (not equality: the MFMA product sums in another order and the weight gradient splits differently)."""
    from convnet_amd import ops
    dev = _dev(mode)
    N, H, W, C, st = SMALL[3]
    x, w, b, dy = _random_case(N, H, W, C, st, torch.bfloat16)
    xh, wh, dyh = _to_dev(x, w, dy, torch.bfloat16, dev)
    wk = w.reshape(C, 9).contiguous().to(torch.bfloat16).to(dev)          # [K][3][3][1]
    tol = _tol(torch.bfloat16)
    assert rel_l2(ops.dwconv_fwd(xh, wh, None, st).float().cpu(), ops.gconv2d_fwd(xh, wk, C, C, st).float().cpu()) < tol
    assert rel_l2(ops.dwconv_dgrad(dyh, wh, xh.shape, st).float().cpu(),
                  ops.gconv2d_dgrad(dyh, wk, xh.shape, C, C, st).float().cpu()) < tol
    a, g = torch.zeros(C * 9, device=dev), torch.zeros(C * 9, device=dev)
    ops.dwconv_wgrad(xh, dyh, a, None, st, beta=0.0)
    ops.gconv2d_wgrad(xh, dyh, g, C, C, st, beta=0.0)
    assert rel_l2(a.cpu(), g.cpu()) < tol


def test_dwconv_shape_contract():
    from convnet_amd import _lib, ops
    f32, bf, f16 = torch.float32, torch.bfloat16, torch.float16
    ok = ops.dwconv_ok
    assert ok(32, (3, 3), (1, 1), (1, 1), bf) and ok(1024, (3, 3), (2, 2), (1, 1), f16) and ok(12, (3, 3), (1, 1), (1, 1), f32)
    assert not ok(12, (3, 3), (1, 1), (1, 1), bf)            # C not a multiple of the 16-bit chunk
    assert not ok(6, (3, 3), (1, 1), (1, 1), f32)            # ... of the fp32 chunk
    assert not ok(32, (1, 1), (1, 1), (0, 0), bf)            # not 3x3
    assert not ok(32, (5, 5), (1, 1), (2, 2), bf)
    assert not ok(32, (3, 3), (3, 3), (1, 1), bf)            # stride 3
    assert not ok(32, (3, 3), (1, 2), (1, 1), bf)            # unequal strides
    assert not ok(32, (3, 3), (1, 1), (0, 0), bf)            # padding 0
    assert not ok(32, (3, 3), (1, 1), (1, 0), bf)
    assert not ok(0, (3, 3), (1, 1), (1, 1), bf)
    assert not _lib.load().cn_dwconv3x3_ok(32, 3, 3, 1, 1, 1, 1, 7)     # unknown dtype code
    dev = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
    x = torch.zeros(1, 4, 4, 12, dtype=bf, device=dev)
    w = torch.zeros(9 * 12, dtype=bf, device=dev)
    with pytest.raises(_lib.ConvNetHipError) as e:
        ops.dwconv_fwd(x, w, None, 1)
    assert '(rc=-2)' in str(e.value)         # CN_ESHAPE
    with pytest.raises(_lib.ConvNetHipError):
        ops.dwconv_dgrad(x, w, (1, 4, 4, 12), 1)
    with pytest.raises(_lib.ConvNetHipError):
        ops.dwconv_fwd(torch.zeros(1, 4, 4, 16, dtype=bf, device=dev), torch.zeros(9 * 16, dtype=bf, device=dev), None, 3)
    assert _lib.load().cn_dwconv3x3_wgrad_workspace(1, 4, 4, 12, 1, _lib.dtype_code(bf)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_dwconv_gpu_mobilenet_shapes(dtype):
    """Every distinct depthwise shape of MobileNet-1.0 at 224, N = 2: integer data exact, random data within the bounds."""
    dev = _dev('gpu')
    for H, C, st in MOBILENET:
        _exact((2, H, H, C, st), dtype, dev)
        _random((2, H, H, C, st), dtype, dev)


# ---------------------------------------------------------------------------------------------- module
def test_depthwise_module_matches_torch_init_and_shape():
    """Weight [C, 1, 3, 3], bias [C] and the RNG use of torch.nn.Conv2d(groups=C) (seeded construction: the same tensors,
    the same generator state afterwards)."""
    import convnet_amd as ca
    torch.manual_seed(7)
    ours = ca.nn.Conv2d(16, 16, 3, padding=1, groups=16)
    a = torch.rand(4)
    torch.manual_seed(7)
    ref = torch.nn.Conv2d(16, 16, 3, padding=1, groups=16)
    assert ours.depthwise and ours.weight.shape == (16, 1, 3, 3) and ours.bias.shape == (16,)
    assert torch.equal(ours.weight.data, ref.weight.data) and torch.equal(ours.bias.data, ref.bias.data)
    assert torch.equal(a, torch.rand(4))
    assert ca.nn.Conv2d(16, 16, 3, stride=2, padding=1, groups=16, bias=False).bias is None
    # every other grouped configuration behaves as before
    assert not ca.nn.Conv2d(64, 64, 3, padding=1, groups=8, bias=False).depthwise
    for kw in (dict(groups=8, bias=True), dict(groups=16, padding=0), dict(groups=16, stride=3)):
        kw.setdefault('padding', 1)
        with pytest.raises(NotImplementedError):
            ca.nn.Conv2d(16 if kw['groups'] == 16 else 64, 16 if kw['groups'] == 16 else 64, 3, **kw)


class _Net(torch.nn.Module):
    def __init__(self, C, stride, bias):
        super().__init__()
        import convnet_amd as ca
        self.conv = ca.nn.Conv2d(C, C, 3, stride=stride, padding=1, groups=C, bias=bias)

    def forward(self, x):
        return self.conv(x)


def _module_run(stride, bias, dev, seed=11):
    """One forward + backward of the module through autograd on an NHWC fp32 input; returns y, dx (NCHW) and the gradients
    in the parameters' own shapes, with torch's results on the same tensors."""
    import convnet_amd as ca
    C = 16
    torch.manual_seed(seed)
    net = _Net(C, stride, bias)
    w0 = net.conv.weight.detach().clone()
    b0 = net.conv.bias.detach().clone() if bias else None
    ca.engine.prepare(net, dev, torch.float32)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, C, 6, 7, generator=g)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    y = net(xh)
    dy = torch.randn(y.shape, generator=g)
    ca.ops.fill_f32_(net.conv._arena.grads, 0.0)
    y.backward(dy.to(dev))
    if dev.type == 'cuda':
        ca.ops.SIDE.join(dev)
        torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    wr = w0.double().requires_grad_(True)
    br = b0.double().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br, stride=stride, padding=1, groups=C)
    yr.backward(dy.permute(0, 3, 1, 2).double())
    ours = (_nchw(y.detach()), _nchw(xh.grad), net.conv.weight.grad.cpu(), net.conv.bias.grad.cpu() if bias else None)
    return ours, (yr.detach(), xr.grad, wr.grad, br.grad if bias else None)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('stride', [1, 2])
def test_depthwise_module_autograd_matches_torch(mode, stride):
    dev = _dev(mode)
    ours, ref = _module_run(stride, True, dev)
    for name, a, b, tol in zip(('y', 'dx', 'dw', 'db'), ours, ref, (1e-5, 1e-4, 1e-4, 1e-4)):
        assert tuple(a.shape) == tuple(b.shape), name
        assert rel_l2(a, b) < tol, (name, rel_l2(a, b))


@pytest.mark.parametrize('mode', MODES)
def test_flag_dwconv_off_takes_the_grouped_route(mode, monkeypatch):
    """flags dwconv=0: the bias-free layer runs on the grouped kernels and agrees with the depthwise ones (fp32: 1e-5 /
    1e-4); a layer with a bias raises NotImplementedError at forward."""
    import convnet_amd as ca
    dev = _dev(mode)
    on, _ = _module_run(2, False, dev)
    c0 = ca.ops.COUNTERS.get('gconv', 0)
    monkeypatch.setattr(ca.ops, 'DWCONV', False)
    off, _ = _module_run(2, False, dev)
    assert ca.ops.COUNTERS.get('gconv', 0) == c0 + 1
    for name, a, b, tol in zip(('y', 'dx', 'dw'), on, off, (1e-5, 1e-4, 1e-4)):
        assert rel_l2(a, b) < tol, name
    with pytest.raises(NotImplementedError):
        _module_run(1, True, dev)
