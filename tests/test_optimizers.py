"""Adam, AdamW, RMSprop and Nesterov SGD as fused flat-arena optimizers: the kernels of csrc/optim.hip and
OptimRegime's handling of them against torch.optim on the CPU (single-tensor arithmetic), in the two modes of
tests/test_ops.py (emul: the same kernel sources through the CPU emulator; gpu: libconvnet_hip.so on an MI355X).
Both sides always get the SAME gradients: what is compared is the optimizer arithmetic, not a training run.
Bound: rel-L2 < 1e-6 for the parameters and every state buffer, the bound of test_sgd_momentum_weight_decay_clip."""
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import rel_l2

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
BOUND = 1e-6
LR, WD_L2, WD_DEC = 1e-2, 1e-4, 1e-2

# name -> (torch factory, torch state keys in the order of the kernel's state buffers)
KERNEL_CASES = {
    'Adam': (lambda p: torch.optim.Adam(p, lr=LR, betas=(0.9, 0.999), eps=1e-8), ('exp_avg', 'exp_avg_sq')),
    'AdamW': (lambda p: torch.optim.AdamW(p, lr=LR, betas=(0.8, 0.99), eps=1e-6, weight_decay=WD_DEC),
              ('exp_avg', 'exp_avg_sq')),
    'RMSprop': (lambda p: torch.optim.RMSprop(p, lr=LR, alpha=0.99, eps=1e-8), ('square_avg',)),
    'RMSprop_momentum': (lambda p: torch.optim.RMSprop(p, lr=LR, alpha=0.9, eps=1e-8, momentum=0.9),
                         ('square_avg', 'momentum_buffer')),
    'Nesterov': (lambda p: torch.optim.SGD(p, lr=LR, momentum=0.9, nesterov=True), ('momentum_buffer',)),
}
# 1, 3: tail only; 4: no tail; 1003: both; (gpu) 4096*256*4 + 1027: second trip of the grid-stride loop + ragged tail
LENGTHS = [(1, MODES), (3, MODES), (4, MODES), (1003, MODES), (4096 * 256 * 4 + 1027, MODES[1:])]
KERNEL_PARAMS = [pytest.param(m.values[0], n, marks=m.marks) for n, modes in LENGTHS for m in modes]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    import convnet_amd as ca
    assert ca._lib.is_emulated() == (mode == 'emul')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _stream(dev):
    return None if dev.type == 'cpu' else torch.cuda.current_stream().cuda_stream


def _kernel_call(L, name, ptr, opt, p, g, bufs, n, lr_arg, mu_arg, clip, hyp, corr, stream):
    grp = opt.param_groups[0]
    if name in ('Adam', 'AdamW'):
        b1, b2 = grp['betas']
        L.cn_adam(ptr(p), ptr(g), ptr(bufs[0]), ptr(bufs[1]), n, lr_arg, 1.0 - b1, b2, 1.0 - b2, grp['eps'], WD_L2,
                  WD_DEC if name == 'AdamW' else 0.0, 1.0 / 8.0, ptr(clip), ptr(hyp), ptr(corr), stream)
    elif name.startswith('RMSprop'):
        L.cn_rmsprop(ptr(p), ptr(g), ptr(bufs[0]), ptr(bufs[1]) if len(bufs) > 1 else None, n, lr_arg, mu_arg,
                     grp['alpha'], 1.0 - grp['alpha'], grp['eps'], WD_L2, 1.0 / 8.0, ptr(clip), ptr(hyp), stream)
    else:
        L.cn_sgd_nesterov(ptr(p), ptr(g), ptr(bufs[0]), n, lr_arg, mu_arg, WD_L2, 1.0 / 8.0, ptr(clip), ptr(hyp), stream)


def _clip_grad_norm(pr, max_norm):
    """torch.nn.utils.clip_grad_norm_ with the norm taken in float64.  torch's own fp32 CPU norm is fine for the short
    lengths and 8.3e-5 low at 4096*256*4 + 1027 elements (255.94827 against 255.96946 in float64 for the gradient of
    step 0) - an error of the reference that every state buffer would inherit through the clip coefficient, 80 times the
    bound.  The coefficient itself is torch's: max_norm / (norm + 1e-6), clamped to 1, applied in fp32."""
    total = pr.grad.double().norm()
    pr.grad.mul_(float(torch.clamp(max_norm / (total + 1e-6), max=1.0)))


@pytest.mark.parametrize('mode,n', KERNEL_PARAMS)
@pytest.mark.parametrize('name', list(KERNEL_CASES))
def test_kernels_against_torch_optim(mode, n, name):
    """5 steps, gradients that change sign and size, loss scale 8, clip 5.0 through cn_grad_norm_clip, a regulariser
    decay (and AdamW's decoupled one), a learning rate that moves, lr / momentum alternately by value and from the
    device buffer (with poisoned by-value arguments); t is read back from the device."""
    dev = _dev(mode)
    from convnet_amd._lib import load, ptr
    L = load()
    factory, keys = KERNEL_CASES[name]
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    pr = p0.clone().requires_grad_(True)
    opt = factory([pr])
    mu = opt.param_groups[0].get('momentum', 0.0)
    npad = (n + 3) // 4 * 4
    p = torch.zeros(npad, device=dev); p[:n] = p0.to(dev)
    gr = torch.zeros(npad, device=dev)
    bufs = [torch.zeros(npad, device=dev) for _ in keys]
    norm_out = torch.zeros(2, device=dev)
    ws = torch.zeros(L.cn_grad_norm_workspace() // 4, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    corr = torch.zeros(2, device=dev)
    stream = _stream(dev)
    steps = 5
    for step, (scale, lr) in enumerate(zip((1.0, -3.0, 0.25, -40.0, 7.0), (LR, LR, LR / 2, LR / 2, LR / 4))):
        gs = torch.randn(n, generator=gen) * scale
        opt.param_groups[0]['lr'] = lr
        pr.grad = (gs / 8.0).clone()                        # reference: p.grad.div_(loss_scale)
        _clip_grad_norm(pr, 5.0)                            # then clip
        pr.grad.add_(pr.detach(), alpha=WD_L2)              # WeightDecay regulariser, then the optimizer
        opt.step()
        gr[:n] = gs.to(dev)
        L.cn_grad_norm_clip(ptr(gr), npad, 1.0 / 8.0, 5.0, ptr(norm_out), None, 0.0, ptr(ws), stream)
        hyp = torch.tensor([lr, mu], device=dev) if step % 2 else None
        if name != 'Nesterov':
            b1, b2 = opt.param_groups[0].get('betas', (0.0, 0.0))
            L.cn_optim_advance(ptr(step_dev), ptr(corr), 1.0 - b1, 1.0 - b2, stream)
        _kernel_call(L, name, ptr, opt, p, gr, bufs, n, lr if hyp is None else 7.0, mu if hyp is None else 0.5,
                     norm_out[1:], hyp, corr, stream)
        err = {'p': rel_l2(p[:n].cpu(), pr.detach())}
        for key, buf in zip(keys, bufs):
            err[key] = rel_l2(buf[:n].cpu(), opt.state[pr][key])
        print(name, n, 'step', step, err)
        assert all(e < BOUND for e in err.values()), (step, err)
        assert float(p[n:].abs().sum()) == 0.0 and all(float(b[n:].abs().sum()) == 0.0 for b in bufs)
    if name != 'Nesterov':
        assert int(step_dev.item()) == steps
        assert int(float(opt.state[pr]['step'])) == steps


@pytest.mark.parametrize('mode', MODES)
def test_misaligned_pointer_is_refused_before_any_launch(mode):
    dev = _dev(mode)
    import convnet_amd as ca
    from convnet_amd._lib import load, ptr
    L = load()
    t = [torch.ones(16, device=dev) for _ in range(4)]
    corr = torch.ones(2, device=dev)
    s = _stream(dev)
    calls = [
        lambda a, b, c, d: L.cn_adam(a, b, c, d, 8, 0.1, 0.1, 0.999, 0.001, 1e-8, 0.0, 0.0, 1.0, None, None, ptr(corr), s),
        lambda a, b, c, d: L.cn_rmsprop(a, b, c, d, 8, 0.1, 0.9, 0.99, 0.01, 1e-8, 0.0, 1.0, None, None, s),
        lambda a, b, c, d: L.cn_sgd_nesterov(a, b, c, 8, 0.1, 0.9, 0.0, 1.0, None, None, s),
    ]
    for call in calls:
        for bad in range(4 if call is not calls[2] else 3):
            args = [ptr(x[1:]) if i == bad else ptr(x) for i, x in enumerate(t)]
            with pytest.raises(ca._lib.ConvNetHipError) as e:
                call(*args)
            assert '(rc=-1)' in str(e.value) and '16-byte aligned' in str(e.value)     # CN_EINVAL
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert all(torch.equal(x.cpu(), torch.ones(16)) for x in t)     # nothing ran


# ---- OptimRegime ---------------------------------------------------------------------------------------------------
KW = dict(depth=18, width=(8, 16, 32, 64), inplanes=8, num_classes=16)
REGIME_CASES = {
    'Adam': {'optimizer': 'Adam', 'lr': 1e-3},
    'AdamW': {'optimizer': 'AdamW', 'lr': 1e-3, 'weight_decay': 1e-2, 'betas': (0.8, 0.99)},
    'RMSprop': {'optimizer': 'RMSprop', 'lr': 1e-3, 'alpha': 0.9},
    'RMSprop_momentum': {'optimizer': 'RMSprop', 'lr': 1e-3, 'alpha': 0.9, 'momentum': 0.9},
    'Nesterov': {'optimizer': 'SGD', 'lr': 0.1, 'momentum': 0.9, 'nesterov': True},
}


def _wd_regularizer():
    from convnet_amd.models.resnet import weight_decay_config
    return weight_decay_config(1e-4)


def _model(dev, seed=1):
    import convnet_amd as ca
    torch.manual_seed(seed)
    model = ca.models.resnet(**KW)
    ca.engine.prepare(model, dev, torch.float32)
    return model


def _set_grads(model, step, seed=0):
    """Seeded gradients written through the parameters' gradient views (kernel order underneath); returns them by name
    in the reference layout.  Sign and size change from step to step."""
    gen = torch.Generator().manual_seed(1000 * seed + step)
    out = {}
    scale = (1.0, -2.0, 0.3, 5.0, -0.7, 1.5, -3.0)[step % 7]
    for n, p in model.named_parameters():
        g = torch.randn(p.shape, generator=gen) * scale
        p.grad.copy_(g.to(p.grad.device))
        out[n] = g
    return out


def _state_buffers(opt):
    return [b for b in (opt.momentum_buf, opt.exp_avg, opt.exp_avg_sq, opt.square_avg) if b is not None]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(REGIME_CASES))
def test_arena_padding_stays_zero(mode, name):
    """The slots of this model carry alignment padding (BatchNorm vectors of 8..64 channels in 64-float slots): after 3
    steps the padding of params and of every state buffer is exactly 0."""
    dev = _dev(mode)
    import convnet_amd as ca
    model = _model(dev)
    opt = ca.OptimRegime(model, [dict(REGIME_CASES[name], epoch=0, regularizer=_wd_regularizer())])
    opt.update(0, 0)
    opt._bind()
    a = opt.arena
    pad = torch.ones(a.params.numel(), dtype=torch.bool)
    for s in a.slots:
        pad[s.offset:s.offset + s.numel] = False
    assert int(pad.sum()) > 0
    for step in range(3):
        _set_grads(model, step)
        opt.step()
    bufs = _state_buffers(opt)
    assert len(bufs) == {'Adam': 2, 'AdamW': 2, 'RMSprop': 1, 'RMSprop_momentum': 2, 'Nesterov': 1}[name]
    for t in [a.params] + bufs:
        t = t.cpu()
        assert torch.isfinite(t).all() and float(t[~pad].abs().sum()) > 0
        assert float(t[pad].abs().max()) == 0.0


def _torch_twin(model, factory):
    """Leaf copies of the model's parameters in the reference layout + a torch optimizer over them."""
    ref = {n: p.detach().cpu().clone().contiguous().requires_grad_(True) for n, p in model.named_parameters()}
    return ref, factory(list(ref.values()))


def _decayed(name):
    return not (name.endswith('bias') or 'bn' in name or 'downsample.1' in name)


@pytest.mark.parametrize('mode', MODES)
def test_regime_with_lr_change_and_switch_to_adam_follows_torch(mode):
    """The googlenet shape: SGD, an lr change, then 'optimizer': Adam at a later boundary, an lr change under Adam.
    torch.optim is driven by hand on the same named tensors with the same gradients; the switch constructs the new
    optimizer from the old param groups (zero state, lr / weight_decay carried over) as the reference does."""
    dev = _dev(mode)
    import convnet_amd as ca
    model = _model(dev)
    regime = [{'epoch': 0, 'optimizer': 'SGD', 'lr': 0.1, 'momentum': 0.9, 'regularizer': _wd_regularizer()},
              {'epoch': 2, 'lr': 0.01},
              {'epoch': 3, 'optimizer': 'Adam', 'lr': 1e-3},
              {'epoch': 5, 'lr': 5e-4}]
    opt = ca.OptimRegime(model, regime)
    ref, topt = _torch_twin(model, lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9))
    names = list(ref)
    assert any(_decayed(n) for n in names) and sum(not _decayed(n) for n in names) > 10
    sigs = []
    for step in range(7):
        opt.update(step, step)
        sigs.append(opt.runs_signature())
        if step == 2:
            topt.param_groups[0]['lr'] = 0.01
        if step == 3:
            topt = torch.optim.Adam(topt.param_groups)
            topt.param_groups[0]['lr'] = 1e-3
        if step == 5:
            topt.param_groups[0]['lr'] = 5e-4
        grads = _set_grads(model, step)
        opt.grad_scale, opt.clip_coef = 1.0, None
        opt.step()
        for n in names:
            g = grads[n].clone()
            if _decayed(n):                     # the WeightDecay filter: BatchNorm weights and every bias are not decayed
                g.add_(ref[n].detach(), alpha=1e-4)
            ref[n].grad = g
        topt.step()
        if step == 3:       # the switch started Adam from zero state: after one step m = (1 - b1) g', t = 1
            sd = opt.state_dict()
            assert sd['optimizer'] == 'Adam' and all(e['step'] == 1 for e in sd['state'].values())
            assert opt.momentum_buf is None
        worst = max(rel_l2(p.detach().cpu(), ref[n].detach()) for n, p in model.named_parameters())
        print('step', step, 'worst rel-L2', worst)
        assert worst < BOUND, (step, worst)
    assert sigs[0] == sigs[2] and sigs[3] != sigs[2] and sigs[3] == sigs[6]   # lr moves nothing, the switch re-keys
    # state_dict: torch's key names and shapes, values within the bound of torch's
    sd = opt.state_dict()
    assert sorted(sd) == ['hyper', 'optimizer', 'regime_phase', 'state'] and sorted(sd['state']) == sorted(names)
    tsd = topt.state_dict()
    for i, n in enumerate(names):
        assert sorted(sd['state'][n]) == ['exp_avg', 'exp_avg_sq', 'step'] and sd['state'][n]['step'] == 4
        for key in ('exp_avg', 'exp_avg_sq'):
            assert sd['state'][n][key].shape == tsd['state'][i][key].shape == ref[n].shape
            assert rel_l2(sd['state'][n][key], tsd['state'][i][key]) < BOUND
    # import of torch's own state_dict: bit for bit, bare and under 'optimizer_state'
    for wrap in (lambda s: s, lambda s: {'optimizer_state': s, 'regime': []}):
        opt.load_state_dict(wrap(tsd))
        opt.update(6, 6)
        mine = opt.state_dict()['state']
        for i, n in enumerate(names):
            assert mine[n]['step'] == 4
            for key in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(mine[n][key], tsd['state'][i][key]), (n, key)


@pytest.mark.parametrize('mode', MODES)
def test_rmsprop_state_dict_imports_torch_state_bit_for_bit(mode):
    dev = _dev(mode)
    import convnet_amd as ca
    model = _model(dev)
    opt = ca.OptimRegime(model, [dict(REGIME_CASES['RMSprop_momentum'], epoch=0)])
    opt.update(0, 0)
    ref, topt = _torch_twin(model, lambda ps: torch.optim.RMSprop(ps, lr=1e-3, alpha=0.9, momentum=0.9))
    for step in range(2):
        grads = _set_grads(model, step)
        for n in ref:
            ref[n].grad = grads[n].clone()
        topt.step()
    tsd = topt.state_dict()
    opt.load_state_dict(tsd)
    opt.update(0, 2)
    mine = opt.state_dict()
    assert mine['optimizer'] == 'RMSprop'
    for i, n in enumerate(ref):
        assert sorted(mine['state'][n]) == ['momentum_buffer', 'square_avg', 'step'] and mine['state'][n]['step'] == 2
        for key in ('square_avg', 'momentum_buffer'):
            assert torch.equal(mine['state'][n][key], tsd['state'][i][key]), (n, key)


@pytest.mark.parametrize('mode', MODES)
def test_refusals(mode):
    dev = _dev(mode)
    import convnet_amd as ca
    Err = ca._lib.ConvNetHipError
    model = _model(dev)

    def regime(**kw):
        o = ca.OptimRegime(model, [dict(kw, epoch=0)])
        o.update(0, 0)
        return o
    with pytest.raises(NotImplementedError) as e:
        regime(optimizer='Adagrad', lr=0.1)
    assert all(n in str(e.value) for n in ('SGD', 'Adam', 'AdamW', 'RMSprop'))
    for kw in (dict(optimizer='Adam', amsgrad=True), dict(optimizer='RMSprop', centered=True),
               dict(optimizer='SGD', momentum=0.9, dampening=0.1), dict(optimizer='SGD', momentum=0.9, nesterov=True,
                                                                        dampening=0.5)):
        with pytest.raises(NotImplementedError):
            regime(lr=0.1, **kw)
    assert regime(optimizer=torch.optim.AdamW, lr=0.1).opt_name == 'AdamW'       # the torch class, as for SGD today
    # hyper-parameters: torch's defaults for what the regime never set; what it set survives a switch
    o = ca.OptimRegime(model, [{'epoch': 0, 'optimizer': 'SGD', 'lr': 0.1, 'momentum': 0.9, 'weight_decay': 5e-4, 'eps': 1e-3},
                               {'epoch': 1, 'optimizer': 'Adam'}])
    o.update(0, 0)
    sig_sgd = o.runs_signature()
    o.update(1, 1)
    assert o.opt_name == 'Adam' and o.hyper['betas'] == (0.9, 0.999) and o.hyper['eps'] == 1e-3
    assert (o.hyper['lr'], o.hyper['momentum'], o.hyper['weight_decay']) == (0.1, 0.9, 5e-4)
    assert o.runs_signature() != sig_sgd
    assert {wd for _, _, wd in o._runs} == {5e-4} and o._decoupled == 0.0          # coupled for Adam
    sig = o.runs_signature()
    o.adjust(dict(o.setting, eps=1e-4))
    assert o.runs_signature() != sig                  # a by-value scalar moved: a new capture key
    o.adjust(dict(o.setting, optimizer='AdamW'))
    o.runs_signature()
    assert {wd for _, _, wd in o._runs} == {0.0} and o._decoupled == 5e-4          # decoupled for AdamW

    # load_state_dict
    adam = regime(optimizer='Adam', lr=1e-3)
    _set_grads(model, 0)
    adam.step()
    good = adam.state_dict()
    names = list(good['state'])
    bad = {'optimizer': 'Adam', 'state': {n: dict(e) for n, e in good['state'].items()}, 'hyper': {}}
    bad['state'][names[3]]['step'] = 2
    with pytest.raises(Err):                           # per-parameter steps differ
        adam.load_state_dict(bad)
    with pytest.raises(Err):                           # unknown layouts
        adam.load_state_dict({'something': 'else'})
    with pytest.raises(Err):
        adam.load_state_dict({'optimizer': 'Adam', 'state': {n: {'step': 1, 'max_exp_avg_sq': torch.zeros(1)} for n in names}})
    with pytest.raises(Err):
        adam.load_state_dict({'state': {}, 'param_groups': []})
    # a state for another optimizer than the one the replayed regime puts in force
    rms = regime(optimizer='RMSprop', lr=1e-3)
    rms.load_state_dict(good)
    with pytest.raises(Err):
        rms.update(0, 1)
    sgd = regime(optimizer='SGD', lr=0.1, momentum=0.9)
    sgd.load_state_dict(good)
    with pytest.raises(Err):
        sgd.step()
    adam2 = regime(optimizer='Adam', lr=1e-3)
    adam2.load_state_dict(regime(optimizer='SGD', lr=0.1, momentum=0.9).state_dict())
    with pytest.raises(Err):
        adam2.update(0, 1)
    # RMSprop: a state without the momentum buffer the regime needs
    with pytest.raises(Err):
        regime(optimizer='RMSprop', lr=1e-3, momentum=0.9).load_state_dict(regime(optimizer='RMSprop', lr=1e-3).state_dict())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['Adam', 'RMSprop_momentum'])
def test_resume_is_bit_identical_to_an_uninterrupted_run(mode, name):
    """3 steps, state_dict, a fresh model + OptimRegime (whose optimizer comes into force only when the regime is
    replayed, after load_state_dict), 3 more steps: the parameters equal those of 6 uninterrupted steps bit for bit."""
    dev = _dev(mode)
    import convnet_amd as ca
    regime = [dict(REGIME_CASES[name], epoch=0, regularizer=_wd_regularizer()), {'epoch': 4, 'lr': 5e-4}]

    def steps(model, opt, rng):
        for step in rng:
            opt.update(step, step)
            _set_grads(model, step)
            opt.step()
    m_all = _model(dev)
    o_all = ca.OptimRegime(m_all, regime)
    steps(m_all, o_all, range(6))
    m1 = _model(dev)
    o1 = ca.OptimRegime(m1, regime)
    steps(m1, o1, range(3))
    saved = {'model': {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}, 'optim': o1.state_dict()}
    assert all(e['step'] == 3 for e in saved['optim']['state'].values())
    m2 = _model(dev, seed=77)
    m2.load_state_dict(saved['model'])
    o2 = ca.OptimRegime(m2, regime)
    o2.load_state_dict(saved['optim'])
    steps(m2, o2, range(3, 6))
    assert all(e['step'] == 6 for e in o2.state_dict()['state'].values())
    for (n, a), (_, b) in zip(m_all.named_parameters(), m2.named_parameters()):
        assert torch.equal(a.detach().cpu(), b.detach().cpu()), n
    for a, b in zip(_state_buffers(o_all), _state_buffers(o2)):
        assert torch.equal(a.cpu(), b.cpu())


# ---- command line --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_cli_mnist_adam_trains_and_resumes(mode, tmp_path):
    """Config 0 from the command line: models/mnist.py attaches no regime, so --optimizer / --lr make it."""
    _dev(mode)
    import math
    from convnet_amd.main import main
    common = ['--model', 'mnist', '--dataset', 'synthetic', '--optimizer', 'Adam', '--lr', '1e-3', '--batch-size', '2',
              '--input-size', '10',
              '--steps-per-epoch', '3', '--val-steps', '1', '--results-dir', str(tmp_path), '--print-freq', '1000',
              '--device', 'cuda' if mode == 'gpu' else 'cpu']
    res = main(common + ['--epochs', '1', '--save', 'first'])
    assert math.isfinite(res['train']['loss']) and math.isfinite(res['val']['loss'])
    ckpt = os.path.join(str(tmp_path), 'first', 'checkpoint.pth.tar')
    state = torch.load(ckpt, map_location='cpu', weights_only=False)['optim_state_dict']
    assert state['optimizer'] == 'Adam' and {e['step'] for e in state['state'].values()} == {3}
    res2 = main(common + ['--epochs', '2', '--save', 'second', '--resume', ckpt])
    assert math.isfinite(res2['train']['loss']) and math.isfinite(res2['val']['loss'])
    state2 = torch.load(os.path.join(str(tmp_path), 'second', 'checkpoint.pth.tar'), map_location='cpu',
                        weights_only=False)['optim_state_dict']
    assert {e['step'] for e in state2['state'].values()} == {6}      # continued, not restarted
