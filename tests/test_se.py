"""nn.SEBlock (csrc/se.hip) against the reference MODULE: tests/golden/se_ops.pt holds what the reference's SEBlock
(models/modules/se.py:6-25, float64, CPU) returned at these shapes (tools/make_golden_se.py), with the rel-L2 bounds
test_l1bn.py takes from test_ops.py (forward fp32 1e-5 / bf16 1e-2 / f16 2e-3; dr 1e-4 / 1.5e-2; parameter gradients the
larger of that and 2e-4).
  * emul: the same kernel sources through the TEST-ONLY SIMT emulator
  * gpu : libconvnet_hip.so on a real MI355X
The fixture stores seeds, not inputs, and up to 2048 samples of every returned tensor (make_golden.sample_tensor); the
whole tensors are checked here against a float64 closed form that the same samples pin to the reference."""
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import GOLDEN, rel_l2, sample_index

MODES = ['emul', pytest.param('gpu', marks=pytest.mark.gpu)]
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
        _FIX.update(torch.load(os.path.join(GOLDEN, 'se_ops.pt')))
    return _FIX


def _inputs(shape, signed, seed):
    """tools/make_golden_se.py:op_inputs restated: float64 values that are exact in bf16 and fp32 (and in f16 but for the
    few below 2^-14); r NCHW, signed (a shortcut BatchNorm's output) or post-ReLU (an identity block's input)."""
    N, H, W, C, Cr = shape
    g = torch.Generator().manual_seed(seed)

    def draw(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).bfloat16().double()
    r = (draw(N, C, H, W) + draw(N, C, 1, 1, scale=0.7) + draw(1, C, 1, 1, scale=0.5)).bfloat16().double()
    if not signed:
        r = r.clamp_min(0)
    w1, b1 = draw(Cr, C, scale=2.0 / C ** 0.5), draw(Cr, scale=0.3)
    w2, b2 = draw(C, Cr, scale=1.5 / Cr ** 0.5), draw(C, scale=0.5)
    dout = draw(N, C, H, W)
    return r, w1, b1, w2, b2, dout


def closed_form(r, w1, b1, w2, b2, dout):
    """The reference's semantics in float64 on NCHW tensors."""
    HW = r.shape[2] * r.shape[3]
    s = r.mean((2, 3))
    a1 = s @ w1.t() + b1
    h = a1.clamp_min(0)
    m = torch.sigmoid(h @ w2.t() + b2)
    out = r * m[:, :, None, None]
    dm = (dout * r).sum((2, 3))
    dz2 = dm * m * (1 - m)
    dh = (dz2 @ w2) * (a1 > 0)
    ds = dh @ w1
    dr = dout * m[:, :, None, None] + ds[:, :, None, None] / HW
    return {'out': out, 'dr': dr, 'm': m, 'dw1': dh.t() @ s, 'db1': dh.sum(0), 'dw2': dz2.t() @ h, 'db2': dz2.sum(0),
            's': s, 'h': h, 'ds': ds}


def _nhwc(t, dtype, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def _nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


def _module(C, Cr, w1, b1, w2, b2, dtype, dev):
    import convnet_amd as ca
    se = ca.nn.SEBlock(C, ratio=C // Cr)
    assert se.hidden_channels == Cr
    with torch.no_grad():
        se.transform[0].weight.copy_(w1.float())
        se.transform[0].bias.copy_(b1.float())
        se.transform[2].weight.copy_(w2.float())
        se.transform[2].bias.copy_(b2.float())
    arena = ca.engine.prepare(torch.nn.Sequential(se), dev, dtype)
    assert len(arena.slots) == 4
    return se


_PARAMS = (('dw1', 0, 'weight'), ('db1', 0, 'bias'), ('dw2', 2, 'weight'), ('db2', 2, 'bias'))


def _grads(se):
    return {k: se.transform[i].grad_view(p).detach().float().cpu().clone().view(se.transform[i]._slots[p].param.shape)
            for k, i, p in _PARAMS}


def _call(se, r, dout, dtype, dev, zero=True):
    """One forward + backward of the module; NCHW fp32 copies of out / dr and the four gradient segments."""
    if zero:
        for _, i, p in _PARAMS:
            se.transform[i].grad_view(p).zero_()
    rh = _nhwc(r, dtype, dev).requires_grad_(True)
    out = se(rh)
    out.backward(_nhwc(dout, dtype, dev))
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    res = {'out': _nchw(out), 'dr': _nchw(rh.grad)}
    res.update(_grads(se))
    return res


def _tols(dtype):
    fwd = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype]
    grad = 1e-4 if dtype == torch.float32 else 1.5e-2
    return fwd, grad, max(grad, 2e-4)


def _sampled(t, name):
    t = t.contiguous().flatten()
    return t[sample_index(name, t.numel())]


def _check_record(rec, dtype, dev):
    from convnet_amd import ops
    shape = tuple(rec['shape'])
    N, H, W, C, Cr = shape
    ins = _inputs(shape, rec['signed'], rec['seed'])
    assert [float(t.sum()) for t in ins] == pytest.approx(rec['input_sums'], rel=1e-12, abs=1e-12)
    assert bool((ins[0] < 0).any()) == bool(rec['signed'])
    ref = closed_form(*ins)
    # the closed form IS the reference module (float64 against float64: rounding only)
    for k in ('out', 'dr', 'm', 'dw1', 'db1', 'dw2', 'db2'):
        assert rel_l2(_sampled(ref[k], k), rec[k]['val']) < 1e-6, k
        assert float(ref[k].norm()) == pytest.approx(rec[k]['norm'], rel=1e-6), k
    # both sides see the activations rounded to the compute dtype: bf16 and fp32 hold them exactly, f16 all but the few of
    # magnitude below 2^-14 (the weights stay fp32 masters)
    r, w1, b1, w2, b2, dout = ins
    r16, d16 = r.to(dtype).double(), dout.to(dtype).double()
    if not (torch.equal(r16, r) and torch.equal(d16, dout)):
        assert dtype == torch.float16
        r, dout = r16, d16
        ref = closed_form(r, w1, b1, w2, b2, dout)
    se = _module(C, Cr, w1, b1, w2, b2, dtype, dev)
    assert list(se.state_dict().keys()) == _fixture()['state_dict_keys']
    out = _call(se, r, dout, dtype, dev)
    with torch.no_grad():
        s, h, m = ops._se_gate(_nhwc(r, dtype, dev), se, N, H * W, C, Cr)
        ev = se.eval()(_nhwc(r, dtype, dev))     # the same operator in eval mode
    se.train()
    assert s.dtype == h.dtype == m.dtype == torch.float32
    fwd, grad, pgrad = _tols(dtype)
    what = (shape, rec['signed'], dtype)
    errs = {'out': (rel_l2(out['out'], ref['out']), fwd), 'dr': (rel_l2(out['dr'], ref['dr']), grad),
            'm': (rel_l2(m.cpu(), ref['m']), 1e-5), 's': (rel_l2(s.cpu(), ref['s']), 1e-5),
            'out vs fixture': (rel_l2(_sampled(out['out'], 'out'), rec['out']['val']), fwd),
            'dr vs fixture': (rel_l2(_sampled(out['dr'], 'dr'), rec['dr']['val']), grad),
            'm vs fixture': (rel_l2(_sampled(m.cpu(), 'm'), rec['m']['val']), 1e-5)}
    for k, _, _ in _PARAMS:
        errs[k] = (rel_l2(out[k], ref[k]), pgrad)
        errs[k + ' vs fixture'] = (rel_l2(_sampled(out[k], k), rec[k]['val']), pgrad)
    print('se %s: %s' % (what, {k: '%.2e' % e for k, (e, _) in errs.items()}))
    missed = [(what, k, e, tol) for k, (e, tol) in errs.items() if not e < tol]
    assert torch.equal(_nchw(ev), out['out']), what
    # a second identical call: bit-identical outputs and gradients (fixed-order reductions, no atomics)
    out2 = _call(se, r, dout, dtype, dev)
    for k in out:
        assert torch.equal(out[k], out2[k]), (what, k)
    return missed


def _records(shape):
    recs = [r for r in _fixture()['records'] if tuple(r['shape']) == tuple(shape)]
    assert recs, shape
    return recs


# (N, H, W, C, C // ratio): the smallest shapes that reach each code path
SHAPES = [
    (2, 1, 1, 16, 1),        # HW = 1, one hidden unit
    (3, 7, 5, 32, 2),        # odd HW
    (2, 9, 9, 64, 4),
    (1, 37, 1, 1040, 65),    # many chunk columns (several column groups in fp32), C no power of two, 65 hidden units
    (4, 28, 28, 16, 1),      # several pixel slices per sample: partial rows + the finalize launch
    (2, 56, 56, 8, 2),       # ratio 4, one (16-bit) / two (fp32) chunk columns, 256 row lanes
]
GPU_SHAPES = [(2, 56, 56, 256, 16), (2, 7, 7, 2048, 128)]      # the real widths of the first and the last stage
_ID = lambda s: 'x'.join(map(str, s))


def test_fixture_covers_the_shapes():
    fix = _fixture()
    assert fix['state_dict_keys'] == ['transform.0.weight', 'transform.0.bias', 'transform.2.weight', 'transform.2.bias']
    for shape in SHAPES:
        signs = sorted(r['signed'] for r in _records(shape))
        if shape[0] * shape[1] * shape[2] * shape[3] <= 16384:
            assert signs == [0, 1], (shape, signs)
        else:
            assert len(signs) == 1, (shape, signs)
    # the first-block case (signed shortcut) and the post-ReLU case are both among the records
    assert {r['signed'] for r in fix['records']} == {0, 1}
    assert {r['signed'] for s in GPU_SHAPES for r in _records(s)} == {0, 1}


def _run_records(mode, dtype, shape):
    dev = _dev(mode)
    missed = []
    for rec in _records(shape):      # (every record is run and printed before the bounds are asserted)
        missed += _check_record(rec, dtype, dev)
    assert not missed, missed


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ID)
def test_against_reference_module(mode, dtype, shape):
    if mode == 'emul' and dtype == torch.float16 and shape not in ((3, 7, 5, 32, 2), (2, 9, 9, 64, 4)):
        pytest.skip('f16 on the emulator: a subset, as in test_ops.py')
    _run_records(mode, dtype, shape)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', GPU_SHAPES, ids=_ID)
def test_against_reference_module_real_widths(dtype, shape):
    _run_records('gpu', dtype, shape)


@pytest.mark.parametrize('mode', MODES)
def test_two_backward_calls_accumulate_bit_for_bit(mode):
    """The stage-sharing path: a second backward into the same gradient segments adds to what the first one left; in fp32
    the result is the fp32 sum of the two separate results, bit for bit."""
    dev = _dev(mode)
    shape = (3, 7, 5, 32, 2)
    N, H, W, C, Cr = shape
    r1, w1, b1, w2, b2, d1 = _inputs(shape, 1, 11)
    r2, _, _, _, _, d2 = _inputs(shape, 0, 12)
    se = _module(C, Cr, w1, b1, w2, b2, torch.float32, dev)
    a = _call(se, r1, d1, torch.float32, dev)
    b = _call(se, r2, d2, torch.float32, dev)
    _call(se, r1, d1, torch.float32, dev)
    both = _call(se, r2, d2, torch.float32, dev, zero=False)
    for k, _, _ in _PARAMS:
        assert float(a[k].abs().sum()) > 0 and float(b[k].abs().sum()) > 0, k
        assert torch.equal(both[k], a[k] + b[k]), k
    assert torch.equal(both['dr'], b['dr']) and torch.equal(both['out'], b['out'])
    assert se._pending_bwd == 0


@pytest.mark.parametrize('mode', MODES)
def test_apply_addend_scaled_gradients_and_c_abi_refusals(mode):
    """The optional addend of the backward apply pass, dst = beta*dst + scale*(...) of the parameter gradients, and the
    refusals of bad shapes / a short workspace before any launch."""
    dev = _dev(mode)
    import convnet_amd as ca
    from convnet_amd import ops
    lib = ca._lib
    L = lib.load()
    shape = (3, 7, 5, 32, 2)
    N, H, W, C, Cr = shape
    HW = H * W
    r, w1, b1, w2, b2, dout = _inputs(shape, 1, 21)
    ref = closed_form(r, w1, b1, w2, b2, dout)
    add = _inputs(shape, 1, 22)[5]
    f32 = lambda t: t.float().contiguous().to(dev)
    g, m, ds = _nhwc(dout, torch.float32, dev), f32(ref['m']), f32(ref['ds'])
    dr = torch.empty_like(g)
    st = lib.stream_of(g)
    addh = _nhwc(add, torch.float32, dev)
    L.cn_se_scale_bwd_apply(lib.ptr(g), lib.ptr(m), lib.ptr(ds), lib.ptr(addh), lib.ptr(dr), N, HW, C, 0, st)
    assert rel_l2(_nchw(dr), ref['dr'] + add) < 1e-6
    # parameter gradients with beta = 0.5, scale = 2 on top of a known content
    nbytes = L.cn_se_workspace(N, HW, C, Cr, 0)
    assert nbytes >= 4 * N * (C + Cr)
    ws = ops.workspace(nbytes, dev)
    dm = f32((dout * r).sum((2, 3)))
    dst = {k: torch.full(tuple(ref[k].shape), 3.0, device=dev) for k, _, _ in _PARAMS}
    sh, hh, w1h, w2h = f32(ref['s']), f32(ref['h']), f32(w1), f32(w2)      # (held: the call reads them)
    ds.zero_()
    L.cn_se_excite_bwd(lib.ptr(dm), lib.ptr(sh), lib.ptr(hh), lib.ptr(m), lib.ptr(w1h), lib.ptr(w2h), lib.ptr(ds),
                       lib.ptr(dst['dw1']), lib.ptr(dst['db1']), lib.ptr(dst['dw2']), lib.ptr(dst['db2']), 0.5, 2.0, N, C, Cr,
                       lib.ptr(ws), ws.numel() * 4, st)
    for k, _, _ in _PARAMS:
        assert rel_l2(dst[k].cpu(), 1.5 + 2.0 * ref[k]) < 1e-6, k
    assert rel_l2(ds.cpu(), ref['ds']) < 1e-5
    with pytest.raises(lib.ConvNetHipError):      # C not a multiple of the chunk
        L.cn_se_scale_fwd(lib.ptr(g), lib.ptr(m), lib.ptr(dr), N, HW, C + 1, 0, st)
    with pytest.raises(lib.ConvNetHipError):      # more channels than the excite kernels hold
        L.cn_se_excite_fwd(lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), N, 4096,
                           Cr, st)
    with pytest.raises(lib.ConvNetHipError):      # no hidden unit
        L.cn_se_excite_fwd(lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), N, C, 0,
                           st)
    with pytest.raises(lib.ConvNetHipError):      # short workspace
        L.cn_se_excite_bwd(lib.ptr(dm), lib.ptr(dm), lib.ptr(dm), lib.ptr(m), lib.ptr(dm), lib.ptr(dm), lib.ptr(ds),
                           lib.ptr(dst['dw1']), lib.ptr(dst['db1']), lib.ptr(dst['dw2']), lib.ptr(dst['db2']), 1.0, 1.0, N, C,
                           Cr, lib.ptr(ws), 16, st)
    big = (4, 28, 28, 16, 1)
    x = torch.zeros(big[0], big[1], big[2], big[3], device=dev)
    with pytest.raises(lib.ConvNetHipError):      # several slices per sample need the partial rows
        L.cn_se_squeeze(lib.ptr(x), lib.ptr(dm), big[0], big[1] * big[2], big[3], 0, None, 0, st)
    assert L.cn_se_workspace(N, HW, C + 1, Cr, 0) == 0


def test_module_refuses_what_is_not_built():
    import convnet_amd as ca
    with pytest.raises(NotImplementedError):
        ca.nn.SEBlock(8)                      # 8 // 16 == 0 hidden units
    with pytest.raises(NotImplementedError):
        ca.nn.SEBlock(32, out_channels=64)
    with pytest.raises(NotImplementedError):
        ca.nn.SEBlock(4096)
    se = ca.nn.SEBlock(32, ratio=4)
    assert [k for k, _ in se.named_children()] == ['relu', 'global_pool', 'transform']
    assert tuple(se.transform[0].weight.shape) == (8, 32) and tuple(se.transform[2].weight.shape) == (32, 8)
    with pytest.raises(ca._lib.ConvNetHipError):
        se(torch.zeros(1, 2, 2, 32))          # used before engine.prepare
