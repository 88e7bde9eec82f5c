"""Junction pair that recomputes the BatchNorm input (csrc/wgrad.hip: jbwd_kernel_ry, cn_conv2d_bwd1x1_lazy_ry): where
the lazy dy's y is the output of the very convolution whose gradients are formed, the kernel does not read y but forms it
per tile from x and w with the forward kernel's instructions.  Same operands, same splits, same summation order as the
kernel that reads y (jbwd_kernel), so dx and dW are bit-identical to it - provided the forward bits really are
recomputable, which is checked on its own."""
import os
import sys

import pytest
import torch

from conftest import HAS_GPU
from helpers import ROOT, load_traj, rel_l2, run_engine_trajectory

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
C, K = 64, 256
# (N, H, W): 9 pixels, less than one stage of 128; 130, two stages with a tail of 2; 512, whole stages; 765
SHAPES = [(1, 3, 3), (1, 10, 13), (2, 16, 16), (5, 17, 9)]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    import convnet_amd as ca
    assert ca._lib.is_emulated() == (mode == 'emul')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _operands(N, H, W, dtype, dev):
    """x, w, g, coef drawn as tests/test_ops.py's junction-pair test draws them (y is NOT drawn: the forward makes it)."""
    g_ = torch.Generator().manual_seed(N * H + W)
    gq = (torch.randn(N, H, W, K, generator=g_) * 0.5).to(dtype).to(dev)
    torch.randn(N, H, W, K, generator=g_)      # (that test's y draw: keeps the later draws the same)
    x = torch.randn(N, H, W, C, generator=g_).to(dtype).to(dev)
    coef = torch.cat([torch.rand(K, generator=g_) + 0.5, torch.randn(K, generator=g_) * 0.05,
                      torch.randn(K, generator=g_) * 0.01]).to(dev)
    w = (torch.randn(K, 1, 1, C, generator=g_) * (2.0 / C) ** 0.5).to(dtype).to(dev)
    return x, w, gq, coef


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_recomputing_pair_equals_the_pair_that_reads_y(mode, dtype):
    """cn_conv2d_bwd1x1_lazy_ry(x, g, w) against cn_conv2d_bwd1x1_lazy(x, g, y = ops.conv2d_fwd(x, w)) with the same
    jbwd_splits: 3 (several stages per workgroup: prefetch and both g buffers in use) and 256 (workgroups of a single
    partial stage), overwrite and accumulate (beta = 1, scale = 0.5 onto a non-zero dW).  bf16, and fp16 under the
    emulator: bit for bit.  fp16 on the GPU: two compilations of the same arithmetic, relative L2 below 2e-4 (the rule of
    the existing pair test)."""
    dev = _dev(mode)
    import convnet_amd as ca
    ops = ca.ops
    L = ca._lib.load()
    exact = dtype == torch.bfloat16 or mode == 'emul'
    for (N, H, W) in SHAPES:
        x, w, gq, coef = _operands(N, H, W, dtype, dev)
        wc = w.permute(3, 1, 2, 0).contiguous()
        y = ops.conv2d_fwd(x, w, None, K, 1, 1, (1, 1), (0, 0))
        assert float(y.float().abs().sum()) > 0
        dw0 = torch.randn(K, 1, 1, C, generator=torch.Generator().manual_seed(7)).to(dev)
        for splits in (3, 256):
            for beta, scale in ((0.0, 1.0), (1.0, 0.5)):
                L.cn_set_option(b'jbwd_splits', splits)
                try:
                    dw_ref = dw0.clone()
                    dx_ref = ops.conv2d_bwd1x1_lazy(x, gq, y, coef, wc, dw_ref, K, beta=beta, scale=scale)
                    L.cn_kernel_log(1)
                    dw = dw0.clone()
                    with ops.bn_y_is_output_of(w):
                        dx = ops.conv2d_bwd1x1_lazy(x, gq, y, coef, wc, dw, K, beta=beta, scale=scale)
                    names = L.cn_kernel_log(0).decode()
                finally:
                    L.cn_set_option(b'jbwd_splits', 256)
                case = (N, H, W, splits, beta)
                assert 'jbwd_kernel_ry<' in names and 'jbwd_kernel<' not in names, names
                if exact:
                    assert torch.equal(dx.cpu(), dx_ref.cpu()), case
                    assert torch.equal(dw.cpu(), dw_ref.cpu()), case
                else:
                    assert rel_l2(dx.float().cpu(), dx_ref.float().cpu()) < 2e-4, case
                    assert rel_l2(dw.cpu(), dw_ref.cpu()) < 2e-4, case
                assert float(dx.float().abs().sum()) > 0 and not torch.equal(dw.cpu(), dw0.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_every_forward_kernel_of_this_convolution_gives_the_same_bits(dtype):
    """What the recomputation rests on: y of a 64 -> 256 channel 1x1 convolution has the same bits whichever forward
    kernel stored it - the streaming kernel (jfwd_kernel), its "lazy a" form (how conv3's y is made in the step) and the
    tiled kernel in both operand paths (knob igemm_variant)."""
    dev = _dev('gpu')
    import convnet_amd as ca
    ops, lib = ca.ops, ca._lib
    L = lib.load()
    code = lib.dtype_code(dtype)
    for (N, H, W) in SHAPES:
        g_ = torch.Generator().manual_seed(N * H + W)
        y2 = (torch.randn(N, H, W, C, generator=g_) * 1.5 + 0.3).to(dtype).to(dev)
        w = (torch.randn(K, 1, 1, C, generator=g_) * (2.0 / C) ** 0.5).to(dtype).to(dev)
        gamma, beta = (torch.rand(C, generator=g_) + 0.5).to(dev), (torch.randn(C, generator=g_) * 0.3).to(dev)
        stats = torch.empty(4 * C, dtype=torch.float32, device=dev)
        M = N * H * W
        x = torch.empty_like(y2)      # x = relu(bn(y2)): conv3's input
        ws = ops.workspace(L.cn_bn_workspace(M, C, code), dev)
        lib.check(L.cn_bn_fwd_train(lib.ptr(y2), None, lib.ptr(x), None, lib.ptr(gamma), lib.ptr(beta), None, None, None,
                                    0.1, 1e-5, lib.ptr(stats), M, C, 1, code, lib.ptr(ws), ws.numel() * 4,
                                    lib.stream_of(y2)), 'cn_bn_fwd_train')
        y = ops.conv2d_fwd(x, w, None, K, 1, 1, (1, 1), (0, 0))
        assert 'jfwd_kernel' in L.cn_last_kernel_name().decode()
        assert float(y.float().abs().sum()) > 0
        a = torch.empty_like(y2)
        y_la = ops.conv2d_fwd_lazya((y2, stats, a, True), w, K)
        assert L.cn_last_kernel_name().decode().endswith(', true>')
        assert torch.equal(a.cpu().view(torch.int16), x.cpu().view(torch.int16)), (N, H, W)
        assert torch.equal(y_la.cpu().view(torch.int16), y.cpu().view(torch.int16)), (N, H, W)
        saved = ops.CONV1X1_STREAM
        try:
            ops.CONV1X1_STREAM = False
            for variant in (1, 3):      # register-staged and LDS-DMA operand paths of the tiled kernel
                L.cn_set_option(b'igemm_variant', variant)
                y_t = ops.conv2d_fwd(x, w, None, K, 1, 1, (1, 1), (0, 0))
                assert 'igemm_kernel' in L.cn_last_kernel_name().decode()
                assert torch.equal(y_t.cpu().view(torch.int16), y.cpu().view(torch.int16)), (N, H, W, variant)
        finally:
            ops.CONV1X1_STREAM = saved
            L.cn_set_option(b'igemm_variant', 0)


@pytest.mark.gpu
def test_training_with_the_recomputing_pair_is_bit_identical():
    """Full-size ResNet-50, bf16, B = 4, two steps, with jpair_recompute off and on: the pair runs at the same eight
    places, the new kernel only in the second run, and every record and every tensor of the final state is equal."""
    dev = _dev('gpu')
    import convnet_amd as ca
    L = ca._lib.load()
    meta, _ = load_traj('r50_full')
    res = {}
    saved = (ca.ops.JPAIR_RECOMPUTE, ca.ops.LAZY_DY_MIN_MB, ca.ops.conv2d_bwd1x1_lazy)
    seen = []

    def logged(*args, **kw):      # (the library's kernel log is short and per thread: read it around each pair call)
        L.cn_kernel_log(1)
        out = saved[2](*args, **kw)
        seen.append(L.cn_kernel_log(0).decode())
        return out
    try:
        ca.ops.conv2d_bwd1x1_lazy = logged
        for ry in (False, True):
            ca.ops.JPAIR_RECOMPUTE, ca.ops.LAZY_DY_MIN_MB = ry, 0.0
            ca.ops.COUNTERS['jpair'] = 0
            del seen[:]
            recs, tr, model, data = run_engine_trajectory(meta, torch.bfloat16, dev, 2, graph=False)
            res[ry] = (recs, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                       ca.ops.COUNTERS['jpair'], ';'.join(seen))
    finally:
        ca.ops.JPAIR_RECOMPUTE, ca.ops.LAZY_DY_MIN_MB, ca.ops.conv2d_bwd1x1_lazy = saved
    assert res[False][2] == 2 * 4 and res[True][2] == 2 * 4, (res[False][2], res[True][2])
    assert 'jbwd_kernel<' in res[False][3] and 'jbwd_kernel_ry<' not in res[False][3]
    assert 'jbwd_kernel_ry<' in res[True][3] and 'jbwd_kernel<' not in res[True][3]
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    for k, v in res[False][1].items():
        assert torch.equal(v, res[True][1][k]), k


def test_recomputing_pair_fits_the_compute_unit():
    """The code object: LDS within the CU's 160 KB, no scratch beyond the 16 bytes per lane allowed every bf16 kernel,
    MFMA and LDS transpose reads present."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_check
    lib = os.path.join(ROOT, 'convnet.pytorch_amd', 'libconvnet_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    res = {k: v for k, v in isa_check.kernel_resources(lib).items() if 'jbwd_kernel_ry<' in k}
    tab = {k: v for k, v in isa_check.kernel_table(lib).items() if 'jbwd_kernel_ry<' in k}
    assert len(res) == 2 and len(tab) == 2, (sorted(res), sorted(tab))      # bf16 and fp16
    for k, v in res.items():
        assert v['lds'] <= 160 * 1024 and v['scratch'] <= 16, (k, v)
    for k, c in tab.items():
        assert c['mfma'] >= 2 and c['tr_read'] >= 4, (k, c)
