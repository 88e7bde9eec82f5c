"""Shared helpers for the parity tests (test infrastructure)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_traj(tag):
    with open(os.path.join(GOLDEN, 'traj_%s.json' % tag)) as f:
        meta = json.load(f)
    final = torch.load(os.path.join(GOLDEN, 'traj_%s_final.pt' % tag))
    return meta, final


def golden_batches(meta):
    g = torch.Generator().manual_seed(meta['seed'])
    data = [(torch.randn(meta['B'], 3, meta['size'], meta['size'], generator=g),
             torch.randint(0, meta['classes'], (meta['B'],), generator=g)) for _ in range(meta['steps'])]
    for (x, t), (sx, st) in zip(data, meta['input_sums']):   # the seeded generator reproduces the inputs
        assert abs(float(x.double().sum()) - sx) < 1e-6 * max(1.0, abs(sx)) and float(t.sum()) == st
    return data


def tensor_sums(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items()
            if v.dtype.is_floating_point}


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


WARM_SAMPLE = 2048     # == oracle/make_golden.py


def warm_bn_state(model, seed, bn_type=None, last_gamma=(0.03, 0.1)):
    """The recipe of oracle/make_golden.py:warm_bn_state applied to OUR model (same module names and order):
    seeded non-trivial gamma / beta / running statistics for every BatchNorm, so that the inner blocks' weight
    and data gradients are non-zero from step 0 (init_model zeroes the last gamma of every block).  The last
    BatchNorm of every block draws gamma from `last_gamma` (conditioning: see the generator), the others from
    [0.5, 1.5)."""
    if bn_type is None:
        import convnet_amd as ca
        bn_type = ca.nn.BatchNorm2d
    g = torch.Generator().manual_seed(seed)
    names = set(n for n, _ in model.named_modules())
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, bn_type):
                C = m.num_features
                last = name.endswith('.bn3') or (name.endswith('.bn2') and (name[:-4] + '.bn3') not in names)
                lo, hi = last_gamma if last else (0.5, 1.5)
                m.weight.copy_(torch.rand(C, generator=g) * (hi - lo) + lo)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) + 0.5)


def sample_index(name, n):
    if n <= WARM_SAMPLE:
        return torch.arange(n)
    gi = torch.Generator().manual_seed(sum(map(ord, name)) + n)
    return torch.randperm(n, generator=gi)[:WARM_SAMPLE].sort().values


def sample_tensor(v, name):
    """(norm, sampled values) of a tensor in its logical (reference-shape, row-major) element order."""
    v = v.detach().float().cpu().contiguous().flatten()
    return float(v.double().norm()), v[sample_index(name, v.numel())]


def load_warm(tag):
    with open(os.path.join(GOLDEN, 'traj_%s.json' % tag)) as f:
        meta = json.load(f)
    return meta, torch.load(os.path.join(GOLDEN, 'traj_%s_tensors.pt' % tag))


def run_engine_trajectory(meta, dtype, device, steps=None, graph=True, grads_after_step0=None):
    """Train our engine exactly as oracle/make_golden.py trained the reference; returns
    (per-step records, validate dict, model).  `meta['warm_seed']` (warm-start goldens): the BatchNorm state is
    overwritten by the seeded recipe first.  grads_after_step0: dict filled with {name: (norm, sample)} of the
    named parameters' gradients after the first step."""
    import convnet_amd as ca
    torch.manual_seed(123)
    kw = dict(meta['model_kw'])
    model = ca.models.resnet(dataset='imagenet', **kw)
    if meta.get('warm_seed') is not None:
        warm_bn_state(model, meta['warm_seed'], last_gamma=tuple(meta['warm_last_gamma']))
    crit = ca.CrossEntropyLoss(smooth_eps=meta['smooth_eps']) if meta['smooth_eps'] else ca.CrossEntropyLoss()
    opt = ca.OptimRegime(model, model.regime)
    tr = ca.Trainer(model, crit, opt, device=str(device), dtype=dtype, loss_scale=meta['loss_scale'],
                    grad_clip=meta['grad_clip'], print_freq=10 ** 9)
    if not graph:
        tr._use_graph = False     # eager launches only (tests that count Python-side fusion decisions per step)
    data = golden_batches(meta)
    if steps is not None:
        data = data[:steps]
    recs = []
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)], chunk_batch=meta['chunk_batch'])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0 and grads_after_step0 is not None:   # zero_grad runs at the START of a step: these are step 0's
            params = dict(model.named_parameters())
            for k in list(grads_after_step0):
                grads_after_step0[k] = sample_tensor(params[k].grad, k)
    return recs, tr, model, data


# ---- the 2-rank data-parallel workers and their oracle-side checks (tests/test_cli_and_dp.py: gloo, CPU emulator or
# one shared GPU; tests/test_rccl_gpu.py: direct RCCL, one GPU per rank)
DP_WORKER = r'''
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import convnet_amd as ca
DEV = %(dev)r
rank = int(os.environ['RANK'])
if DEV != 'cpu':
    DEV = DEV %% rank if '%%d' in DEV else DEV        # 'cuda:%%d': one device per rank (direct RCCL); 'cuda:0': shared
    torch.cuda.set_device(torch.device(DEV))
    assert not ca._lib.is_emulated()
dist.init_process_group(%(backend)r, init_method='env://')
torch.manual_seed(123 + 7 * rank)          # different initial weights per rank: the broadcast must fix that
model = ca.models.resnet(depth=18, width=(8, 16, 32, 64), inplanes=8, num_classes=16)
tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=DEV,
                dtype=torch.float32, distributed=True, local_rank=rank, grad_clip=1e9, print_freq=10**9,
                bucket_mb=0.05)
g = torch.Generator().manual_seed(77)
data = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 16, (8,), generator=g)) for _ in range(2)]
recs = []
for x, t in data:
    r = tr.train([(x[rank * 4:(rank + 1) * 4], t[rank * 4:(rank + 1) * 4])])
    recs.append({k: float(r[k]) for k in ('loss', 'grad')})
sd = {k: v.float().cpu() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
torch.save({'recs': recs, 'sd': sd, 'nbuckets': len(tr.arena.buckets), 'transport': tr.reducer.describe()}, %(out)r %% rank)
ca.comm.destroy_default()
dist.destroy_process_group()
'''


def check_dp_against_oracle(outs):
    """Oracle-side DDP semantics (/root/reference/trainer.py:79-82): rank-0 initial weights everywhere, per-rank BN
    statistics, gradients averaged over the 2 ranks, one SGD step per iteration."""
    import pytest
    from oracle import convnet_oracle as O
    torch.manual_seed(123)
    replicas = [O.OracleResNet(18, 16, 8, (8, 16, 32, 64)) for _ in range(2)]
    replicas[1].load_state_dict(replicas[0].state_dict())
    opts = [O.OracleSGD(m) for m in replicas]
    g = torch.Generator().manual_seed(77)
    data = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 16, (8,), generator=g)) for _ in range(2)]
    for step, (x, t) in enumerate(data):
        losses = []
        for r, m in enumerate(replicas):
            m.train()
            opts[r].zero_grad()
            loss = O.oracle_cross_entropy(m(x[r * 4:(r + 1) * 4]), t[r * 4:(r + 1) * 4])
            loss.backward()
            losses.append(float(loss))
        for p0, p1 in zip(replicas[0].parameters(), replicas[1].parameters()):
            avg = (p0.grad + p1.grad) / 2
            p0.grad.copy_(avg)
            p1.grad.copy_(avg)
        gnorm = torch.norm(torch.stack([p.grad.norm(2) for p in replicas[0].parameters()]), 2).item()
        for o in opts:
            o.step()
        for r in range(2):
            assert outs[r]['recs'][step]['loss'] == pytest.approx(losses[r], abs=1e-4)
            assert outs[r]['recs'][step]['grad'] == pytest.approx(gnorm, rel=1e-3)
    ref_sd = replicas[0].state_dict()
    for k in ('conv1.weight', 'layer2.0.downsample.0.weight', 'fc.weight', 'layer4.1.bn2.bias'):
        assert rel_l2(outs[0]['sd'][k], ref_sd[k]) < 1e-4, k


def check_syncbn_against_oracle(outs):
    """--sync-bn: 2 ranks x 4 samples with synchronised statistics == one process on the 8-sample batch."""
    import pytest
    from oracle import convnet_oracle as O
    torch.manual_seed(123)
    model = O.OracleResNet(18, 16, 8, (8, 16, 32, 64))
    opt = O.OracleSGD(model)
    g = torch.Generator().manual_seed(77)
    data = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 16, (8,), generator=g)) for _ in range(2)]
    for step, (x, t) in enumerate(data):
        model.train()
        opt.zero_grad()
        loss = O.oracle_cross_entropy(model(x), t)
        loss.backward()
        gnorm = torch.norm(torch.stack([p.grad.norm(2) for p in model.parameters()]), 2).item()
        opt.step()
        rank_mean = 0.5 * (outs[0]['recs'][step]['loss'] + outs[1]['recs'][step]['loss'])
        assert rank_mean == pytest.approx(float(loss), abs=1e-4)
        assert outs[0]['recs'][step]['grad'] == pytest.approx(gnorm, rel=1e-3)
    ref_sd = model.state_dict()
    for k in ('conv1.weight', 'layer2.0.downsample.0.weight', 'fc.weight', 'layer4.1.bn2.bias',
              'bn1.running_mean', 'layer3.0.bn1.running_var', 'layer1.1.bn2.weight'):
        assert rel_l2(outs[0]['sd'][k], ref_sd[k]) < 1e-4, k


# ---- exact-arithmetic helpers (tests/test_exact.py and the per-element bounds beside the rel-L2 checks).
# With small-integer data every product and every partial sum of a convolution is an integer below 2^24, so an fp32
# accumulation is exact in ANY summation order, tile shape or split count, and the correct result is one fixed bit
# pattern: the integer itself in fp32, its round-to-nearest-even in bf16 / fp16.
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


def int_tensor(shape, gen, lo=-3, hi=3, density=0.5):
    """Seeded integer-valued fp64 tensor with values in [lo, hi]; a share `density` of the elements is non-zero."""
    assert lo <= hi and (lo != 0 or hi != 0)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen)
    while True:                                   # redraw the zeros: the density is decided by the mask alone
        z = v == 0
        if not bool(z.any()):
            break
        v = torch.where(z, torch.randint(lo, hi + 1, tuple(shape), generator=gen), v)
    keep = torch.rand(tuple(shape), generator=gen) < density
    return torch.where(keep, v, torch.zeros_like(v)).double()


def assert_exact_domain(abs_result, n_bits=24):
    """abs_result: the operation under test evaluated in fp64 on |inputs| (the magnitude sum A of every output
    element).  A < 2^n_bits bounds every partial sum of every summation order, so no fp32 addition can round."""
    a = float(abs_result.double().abs().max())
    assert a < 2.0 ** n_bits, 'left the exact-integer domain: max magnitude sum %g >= 2^%d' % (a, n_bits)
    return a


def assert_not_degenerate(ref):
    """A reference that is mostly zero, or holds a handful of values, would let a wrong kernel pass."""
    r = ref.double().flatten()
    nz = int((r != 0).sum())
    assert 2 * nz >= r.numel(), 'degenerate reference: only %d of %d elements are non-zero' % (nz, r.numel())
    sample = r if r.numel() <= (1 << 22) else r[:: r.numel() // (1 << 22)]
    nd = int(torch.unique(sample).numel())
    assert nd >= 16, 'degenerate reference: only %d distinct values' % nd


def _mismatch_report(bad, out, want, what):
    """Count, first indices with got / want, and histograms by leading index (image), border / interior pixel (4-D
    n, h, w, c tensors) and 8-channel chunk of the last dimension."""
    idx = bad.nonzero()
    n = idx.shape[0]
    lines = ['%s: %d of %d elements differ' % (what, n, bad.numel())]
    names = 'nhwc' if bad.dim() == 4 else ''.join('d%d,' % i for i in range(bad.dim())).rstrip(',')
    for row in idx[:6].tolist():
        lines.append('  (%s) = %s: got %r want %r' % (','.join(names) if bad.dim() == 4 else names, tuple(row),
                                                    float(out[tuple(row)]), float(want[tuple(row)])))
    lead = torch.bincount(idx[:, 0], minlength=bad.shape[0])
    top = [(int(i), int(lead[i])) for i in lead.argsort(descending=True)[:8].tolist() if int(lead[i])]
    lines.append('  by leading index (image / filter): %d of %d touched, largest %s' % (int((lead > 0).sum()),
                                                                                      bad.shape[0], top))
    if bad.dim() == 4:
        H, W = bad.shape[1], bad.shape[2]
        h, w = idx[:, 1], idx[:, 2]
        border = (h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)
        lines.append('  by pixel: %d on the border, %d interior; rows %s cols %s' % (
            int(border.sum()), int((~border).sum()), sorted(set(h.tolist()))[:12], sorted(set(w.tolist()))[:12]))
    chunk = torch.bincount(idx[:, -1] // 8, minlength=(bad.shape[-1] + 7) // 8)
    lines.append('  by 8-channel chunk of the last dimension: %s' % chunk.tolist()[:64])
    return '\n'.join(lines)


def assert_same_values(out, ref_exact, dtype, what):
    """out == ref_exact.to(dtype) by VALUE on every element (-0.0 == 0.0), and no NaN anywhere in out."""
    out = out.detach().cpu()
    assert out.dtype == dtype, (what, out.dtype, dtype)
    want = ref_exact.detach().cpu().to(dtype)
    assert tuple(out.shape) == tuple(want.shape), (what, tuple(out.shape), tuple(want.shape))
    assert not bool(torch.isnan(out).any()), '%s: NaN in the output' % what
    if torch.equal(out, want):
        return
    bad = out != want
    raise AssertionError(_mismatch_report(bad, out, want, what))


def assert_within_forward_bound(out, ref64, A, n, out_dtype, what=''):
    """Per element: |out - ref| <= u_out*|ref| + 2*n*2^-24*A.  ref64: the fp64 reference, A: the fp64 magnitude sum
    (the same operation on |inputs|), n: the reduction length.  The textbook forward error bound of an fp32 dot
    product in any order (gamma_n <= n*u; the factor 2 covers an internal adder that does not round to nearest) plus one
    rounding to the output format.  Returns the largest |err| / bound."""
    out = out.detach().cpu().double()
    ref64, A = ref64.detach().cpu().double(), A.detach().cpu().double()
    assert tuple(out.shape) == tuple(ref64.shape) == tuple(A.shape), (what, out.shape, ref64.shape, A.shape)
    assert not bool(torch.isnan(out).any()), '%s: NaN in the output' % what
    bound = U_OUT[out_dtype] * ref64.abs() + 2.0 * n * 2.0 ** -24 * A
    err = (out - ref64).abs()
    bad = err > bound
    if bool(bad.any()):
        raise AssertionError(_mismatch_report(bad, out, ref64, '%s: per-element forward bound (n=%d)' % (what, n)))
    ratio = err / bound.clamp_min(1e-300)
    return float(ratio.max())
