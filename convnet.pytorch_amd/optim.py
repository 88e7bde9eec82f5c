"""Regime / OptimRegime: the optimizer object Trainer drives (duck-typed API at /root/reference
trainer.py:111-112,121,157,173,258 and main.py:243-253: zero_grad, update(epoch, steps),
pre_forward, pre_backward, step, get_lr, state_dict / load_state_dict).

The classes live in the reference's un-vendored utils submodule; they are re-stated here from the
call sites and from the regime dictionaries the models attach (models/resnet.py:250-256):
a regime is a list of dicts keyed by 'epoch' (or 'step') whose later entries override earlier ones,
optionally with `step_lambda` / `epoch_lambda` strings that evaluate to a dict of overrides.

The step itself is a fused flat-arena kernel: cn_sgd_momentum for SGD, cn_sgd_nesterov, cn_adam (Adam and
AdamW) and cn_rmsprop for the other values of 'optimizer'.  Weight decay is the reference's WeightDecay
regulariser (g += wd * p for the filtered parameters, applied right before the update, i.e. after gradient
clipping); the plain `weight_decay` hyper-parameter is the same coupled term for SGD, Adam and RMSprop and the
decoupled p *= 1 - lr*wd for AdamW.  State buffers are fp32, master weights are fp32 (the reference's
use_float_copy for half precision is therefore always on).  The step count of Adam / AdamW / RMSprop lives in
device memory (`step_dev`) and is advanced by a launch that is part of the step, so a replayed capture - which
never calls step() on the host - counts too; the host keeps no copy.
"""
from copy import deepcopy

import torch

from . import _lib, engine, ops
from ._lib import ptr, stream_of


OPTIMIZERS = ('SGD', 'Adam', 'AdamW', 'RMSprop')
# torch's state key names -> the attribute holding the flat buffer
_STATE_ATTR = {'momentum_buffer': 'momentum_buf', 'exp_avg': 'exp_avg', 'exp_avg_sq': 'exp_avg_sq',
               'square_avg': 'square_avg'}


def eval_func(f, x):
    if isinstance(f, str):
        f = eval(f)  # regime lambdas are strings in the reference (models/resnet.py:70-72)
    return f(x)


class Regime(object):
    """Epoch/step keyed settings with cumulative override semantics."""

    def __init__(self, regime, defaults=None):
        self.regime = regime
        self.defaults = dict(defaults or {})
        self.reset()

    def reset(self):
        self.current_regime_phase = None
        self.setting = dict(self.defaults)

    def update(self, epoch=None, train_steps=None):
        if self.regime is None:
            return False
        epoch = -1 if epoch is None else epoch
        train_steps = -1 if train_steps is None else train_steps
        setting = deepcopy(self.setting)
        if self.current_regime_phase is None:
            for phase, phase_setting in enumerate(self.regime):
                start_epoch = phase_setting.get('epoch', 0)
                start_step = phase_setting.get('step', 0)
                if epoch >= start_epoch or train_steps >= start_step:
                    self.current_regime_phase = phase
                    break
                setting.update(phase_setting)
            if self.current_regime_phase is None:
                self.current_regime_phase = 0
        while len(self.regime) > self.current_regime_phase + 1:
            nxt = self.regime[self.current_regime_phase + 1]
            if epoch >= nxt.get('epoch', float('inf')) or train_steps >= nxt.get('step', float('inf')):
                setting.update(self.regime[self.current_regime_phase])
                self.current_regime_phase += 1
            else:
                break
        setting.update(self.regime[self.current_regime_phase])
        if 'lr_decay_rate' in setting and 'lr' in setting:
            decay_steps = setting.pop('lr_decay_steps', 100)
            if train_steps % decay_steps == 0:
                setting['lr'] *= setting.pop('lr_decay_rate') ** (train_steps / decay_steps)
        elif 'step_lambda' in setting:
            setting.update(eval_func(setting.pop('step_lambda'), train_steps))
        elif 'epoch_lambda' in setting:
            setting.update(eval_func(setting.pop('epoch_lambda'), epoch))
        if 'execute' in setting:
            setting.pop('execute')()
        if _comparable(setting) == _comparable(self.setting):
            return False
        self.setting = setting
        return True

    def __repr__(self):
        return 'Current: %s\n Regime:%s' % (self.setting, self.regime)


def _comparable(setting):
    return {k: (v if not callable(v) else id(v)) for k, v in setting.items() if k != 'regularizer'} | \
        {'regularizer': repr(setting.get('regularizer'))}


class OptimRegime(Regime):
    def __init__(self, model, regime, defaults=None, filter=None, use_float_copy=False, log=True):
        super().__init__(regime, defaults)
        if filter is not None:
            raise NotImplementedError('OptimRegime(filter=...) is outside the hot path')
        self.model = model
        self.use_float_copy = use_float_copy
        # keys the regime never sets keep torch's defaults (the same for every optimizer that reads them)
        self.hyper = {'lr': 0.0, 'momentum': 0.0, 'weight_decay': 0.0, 'dampening': 0.0, 'nesterov': False,
                      'betas': (0.9, 0.999), 'eps': 1e-8, 'alpha': 0.99, 'centered': False, 'amsgrad': False}
        self.opt_name = 'SGD'
        self.regularizer_cfg = []
        self.arena = None
        self.momentum_buf = None  # SGD / Nesterov momentum; RMSprop's momentum buffer when momentum > 0
        self.exp_avg = None       # Adam / AdamW
        self.exp_avg_sq = None
        self.square_avg = None    # RMSprop
        self.step_dev = None      # int64[1] on the device: steps taken by Adam / AdamW / RMSprop since they came into force
        self._generation = 0      # bumped whenever state buffers are re-allocated: captured pointers are stale then
        self._pending = None      # (optimizer name or family, {key: {param name: tensor}}, t) loaded before its optimizer is in force
        self._loaded = None       # name / family of the state last loaded, until the replayed regime confirmed it
        self._runs = None
        self._decoupled = 0.0     # AdamW's decay, carried beside the (start, end, wd) runs
        # set by Trainer each step
        self.grad_scale = 1.0     # 1/loss_scale (and 1/world_size for data parallel)
        self.clip_coef = None     # device scalar written by cn_grad_norm_clip, or None
        self.hyper_dev = None     # device copy of (lr, momentum) + Adam's two bias corrections: read by the kernels, so a captured step
        self._hyper_pushed = None  # (HIP graph) follows the schedule; refreshed by push_hyper() when it changes

    # -- binding to the device arena ------------------------------------------------------
    def _bind(self):
        if self.arena is not None:
            return
        arena = getattr(self.model, '_cn_arena', None)
        if arena is None:
            raise _lib.ConvNetHipError('OptimRegime: call engine.prepare(model, device, dtype) before stepping')
        self.arena = arena
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=arena.device)
        self._ensure_state(first=True)
        self._runs = None

    def _needed_state(self):
        if self.opt_name in ('Adam', 'AdamW'):
            return ('exp_avg', 'exp_avg_sq')
        if self.opt_name == 'RMSprop':
            return ('square_avg', 'momentum_buf') if float(self.hyper['momentum']) > 0 else ('square_avg',)
        return ('momentum_buf',)

    def _ensure_state(self, first=False):
        """Allocate (zeroed) what the optimizer in force needs and free the rest.  Called from _bind and adjust, i.e. on
        the host side of a step: never inside a capture."""
        if self.arena is None:
            return
        need = self._needed_state()
        changed = False
        for attr in ('momentum_buf', 'exp_avg', 'exp_avg_sq', 'square_avg'):
            have = getattr(self, attr) is not None
            if attr in need and not have:
                setattr(self, attr, torch.zeros_like(self.arena.params))
                changed = True
            elif attr not in need and have:
                setattr(self, attr, None)
                changed = True
        if changed and not first:      # a capture may hold the old pointers
            self._generation += 1

    def _switch(self, opt):
        """Another optimizer comes into force: zero state and t = 0, which is what the reference does by constructing
        torch.optim.X(old.param_groups) - lr, momentum, weight_decay carry over in the param groups, the per-parameter
        state does not.  (That code lives in the reference's un-vendored utils submodule: recalled, not read.)"""
        self.opt_name = opt
        for attr in ('momentum_buf', 'exp_avg', 'exp_avg_sq', 'square_avg'):
            setattr(self, attr, None)       # (_ensure_state allocates the new optimizer's, zeroed)
        if self.step_dev is not None:
            self.step_dev.zero_()
        self._runs = None

    def _build_runs(self):
        """Contiguous arena ranges sharing one weight-decay value -> one optimizer launch each."""
        wd_default = float(self.hyper.get('weight_decay', 0.0) or 0.0)
        self._decoupled = 0.0
        if self.opt_name == 'AdamW':      # the hyper-parameter is the decoupled decay; the regulariser stays coupled L2
            self._decoupled, wd_default = wd_default, 0.0
        per_slot = []
        for s in self.arena.slots:
            wd = wd_default
            for reg in self.regularizer_cfg:
                if reg.get('name') != 'WeightDecay':
                    raise NotImplementedError('regularizer %r is outside the hot path' % reg.get('name'))
                flt = reg.get('filter') or {}
                ok = True
                if 'parameter_name' in flt and not flt['parameter_name'](s.name):
                    ok = False
                if 'module' in flt and not flt['module'](s.module):
                    ok = False
                if ok:
                    wd += float(reg.get('value', 0.0))
            per_slot.append(wd)
        runs = []
        for s, wd in zip(self.arena.slots, per_slot):
            end = s.offset + engine._round_up(s.numel, engine._ALIGN)
            if runs and runs[-1][2] == wd and runs[-1][1] == s.offset:
                runs[-1][1] = end
            else:
                runs.append([s.offset, end, wd])
        self._runs = [(a, b, wd) for a, b, wd in runs]

    # -- regime handling ------------------------------------------------------------------
    def update(self, epoch=None, train_steps=None, metrics=None):
        if super().update(epoch, train_steps):
            self.adjust(self.setting)
            return True
        return False

    def adjust(self, setting):
        opt = setting.get('optimizer', 'SGD')
        if not isinstance(opt, str):
            opt = getattr(opt, '__name__', str(opt))
        if opt not in OPTIMIZERS:
            raise NotImplementedError('optimizer %r: the MI355X hot path implements %s' % (opt, ', '.join(OPTIMIZERS)))
        for key in self.hyper:
            if key in setting and setting[key] != self.hyper[key]:
                if key == 'weight_decay':
                    self._runs = None
                self.hyper[key] = tuple(setting[key]) if key == 'betas' else setting[key]
        if self.hyper.get('dampening'):
            raise NotImplementedError('dampening != 0: torch treats the first step specially, which nothing else needs')
        if self.hyper.get('amsgrad') or self.hyper.get('centered'):
            raise NotImplementedError('amsgrad / centered are not built (Adam, AdamW, RMSprop run their default forms)')
        if opt == 'SGD' and self.hyper.get('nesterov') and not float(self.hyper['momentum']) > 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if opt != self.opt_name:
            self._switch(opt)
        self._ensure_state()
        if 'regularizer' in setting:
            reg = deepcopy_regularizer(setting['regularizer'])
            self.regularizer_cfg = reg
            self._runs = None
        if self._pending is not None and self.arena is not None:
            self._apply_loaded(*self._pending)
        self._confirm_loaded()

    # -- the API Trainer calls ------------------------------------------------------------
    def zero_grad(self):
        self._bind()
        self.arena.zero_grad()

    def pre_forward(self):
        pass

    def pre_backward(self):
        pass

    def step(self, *args, **kwargs):
        self._bind()
        if self._runs is None:
            self._build_runs()
        self._confirm_loaded()
        L = _lib.load()
        a = self.arena
        lr, mu = float(self.hyper['lr']), float(self.hyper['momentum'])
        self.push_hyper()
        gs, clip, hyp, st = float(self.grad_scale), ptr(self.clip_coef), ptr(self.hyper_dev), stream_of(a.params)
        kind, sc = self._kind(), self._scalars()
        if kind in ('Adam', 'AdamW', 'RMSprop'):
            # t += 1 on the device and, for Adam, the bias corrections of this t beside (lr, momentum); the
            # complements are rounded from double here (1.f - 0.999f in the kernel would be 1e-5 off)
            om1, om2 = (1.0 - sc[0], 1.0 - sc[1]) if kind != 'RMSprop' else (1.0, 1.0)
            ops.PROFILER.run('optim_advance', 1, 0.0, 16.0,
                             lambda: L.cn_optim_advance(ptr(self.step_dev), ptr(self.hyper_dev[2:]), om1, om2, st),
                             a.device)
        for start, end, wd in self._runs:
            n = end - start
            p, g = ptr(a.params[start:]), ptr(a.grads[start:])
            if kind == 'SGD':
                ops.PROFILER.run('sgd_momentum', 1, 0.0, 20.0 * n,
                                 lambda: L.cn_sgd_momentum(p, g, ptr(self.momentum_buf[start:]), n, lr, mu, float(wd),
                                                           gs, clip, hyp, st),
                                 a.device)
            elif kind == 'Nesterov':
                ops.PROFILER.run('sgd_nesterov', 1, 0.0, 20.0 * n,
                                 lambda: L.cn_sgd_nesterov(p, g, ptr(self.momentum_buf[start:]), n, lr, mu, float(wd),
                                                           gs, clip, hyp, st),
                                 a.device)
            elif kind == 'RMSprop':
                alpha, eps = sc
                buf = ptr(self.momentum_buf[start:]) if self.momentum_buf is not None else None
                ops.PROFILER.run('rmsprop', 1, 0.0, (28.0 if buf else 20.0) * n,
                                 lambda: L.cn_rmsprop(p, g, ptr(self.square_avg[start:]), buf, n, lr, mu, alpha,
                                                      1.0 - alpha, eps, float(wd), gs, clip, hyp, st),
                                 a.device)
            else:
                b1, b2, eps = sc
                ops.PROFILER.run('adam', 1, 0.0, 28.0 * n,
                                 lambda: L.cn_adam(p, g, ptr(self.exp_avg[start:]), ptr(self.exp_avg_sq[start:]), n, lr,
                                                   1.0 - b1, b2, 1.0 - b2, eps, float(wd), float(self._decoupled), gs,
                                                   clip, hyp, ptr(self.hyper_dev[2:]), st),
                                 a.device)
        a.bump_version()

    def _kind(self):
        if self.opt_name == 'SGD':
            return 'Nesterov' if self.hyper.get('nesterov') else 'SGD'
        return self.opt_name

    def _scalars(self):
        """The hyper-parameters the kernel in force takes BY VALUE (lr and momentum come from hyper_dev)."""
        kind = self._kind()
        if kind in ('Adam', 'AdamW'):
            b1, b2 = self.hyper['betas']
            return (float(b1), float(b2), float(self.hyper['eps']))
        if kind == 'RMSprop':
            return (float(self.hyper['alpha']), float(self.hyper['eps']))
        return ()

    def push_hyper(self):
        """Device copy of (lr, momentum) for the optimizer kernels; one tiny H2D copy whenever the schedule moves.
        (Floats 2 and 3 of the buffer are Adam's bias corrections, written on the device by cn_optim_advance.)"""
        self._bind()
        cur = (float(self.hyper['lr']), float(self.hyper['momentum']))
        if self.hyper_dev is None:
            self.hyper_dev = torch.zeros(4, dtype=torch.float32, device=self.arena.device)
            self._hyper_pushed = None
        if cur != self._hyper_pushed:
            self.hyper_dev[:2].copy_(torch.tensor(cur, dtype=torch.float32), non_blocking=False)
            self._hyper_pushed = cur

    def runs_signature(self):
        """What a captured step bakes in besides lr / momentum: the weight-decay runs and, for every optimizer but
        plain SGD, the kernel in force, the scalars it takes by value, the decoupled decay and the generation of the
        state buffers (a switch of optimizer allocates new ones: a capture of the old ones must not be replayed)."""
        self._bind()
        if self._runs is None:
            self._build_runs()
        if self._kind() == 'SGD' and self._generation == 0:
            return tuple(self._runs)
        return (self._kind(), self._generation, self._scalars(), self._decoupled,
                self.momentum_buf is not None) + tuple(self._runs)

    def get_value(self, key):
        return [self.hyper.get(key)]

    def get_lr(self):
        return self.get_value('lr')

    # -- checkpoint -----------------------------------------------------------------------
    def _export(self, flat):
        """Flat arena-shaped buffer -> {parameter name: CPU tensor in the reference's shape (filters OIHW)}."""
        out = {}
        for s in self.arena.slots:
            seg = flat[s.offset:s.offset + s.numel]
            p = s.param
            if s.is_filter and p.dim() == 4:
                O, I, R, S_ = p.shape
                out[s.name] = seg.view(O, R, S_, I).permute(0, 3, 1, 2).contiguous().cpu()
            else:
                out[s.name] = seg.view(p.shape).clone().cpu()
        return out

    def _import(self, flat, named, what):
        missing = [s.name for s in self.arena.slots if s.name not in named]
        if missing:
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: %s missing for %s%s'
                                       % (what, missing[:4], ' ...' if len(missing) > 4 else ''))
        for s in self.arena.slots:
            src = named[s.name].to(self.arena.device, torch.float32)
            seg = flat[s.offset:s.offset + s.numel]
            p = s.param
            if s.is_filter and p.dim() == 4:
                O, I, R, S_ = p.shape
                seg.view(O, R, S_, I).permute(0, 3, 1, 2).copy_(src)
            else:
                seg.view(p.shape).copy_(src)

    def state_dict(self):
        """SGD (plain and Nesterov): {'momentum_buffer': {name: tensor}, 'hyper', 'regime_phase'}.  The others:
        {'optimizer': name, 'state': {name: {'step': t, <torch's key>: tensor}}, 'hyper', 'regime_phase'} with torch's key
        names (exp_avg, exp_avg_sq, square_avg, momentum_buffer) and the reference's OIHW shapes; t is read back from
        the device."""
        self._bind()
        self._confirm_loaded()
        if self.opt_name == 'SGD':
            return {'momentum_buffer': self._export(self.momentum_buf), 'hyper': dict(self.hyper),
                    'regime_phase': self.current_regime_phase}
        t = int(self.step_dev.item())
        state = {s.name: {'step': t} for s in self.arena.slots}
        for key, attr in _STATE_ATTR.items():
            if attr in self._needed_state():
                for name, ten in self._export(getattr(self, attr)).items():
                    state[name][key] = ten
        return {'optimizer': self.opt_name, 'state': state, 'hyper': dict(self.hyper),
                'regime_phase': self.current_regime_phase}

    def load_state_dict(self, state):
        """Restores the state buffers and the step count (and the hyper-parameters as a starting point).  The regime
        position is deliberately NOT restored: `setting` is cumulative over all phases passed so far
        (e.g. the WeightDecay regulariser only appears in phase 0 of the ResNet regime,
        models/resnet.py:250-256), so the first `update(epoch, steps)` after a resume replays the
        regime from the start exactly as a fresh OptimRegime at that epoch would.
        Two formats are understood: this engine's own (state_dict() above) and the
        reference's, i.e. what its OptimRegime.state_dict() hands to torch.save (utils.pytorch optim.py: the
        torch.optim state_dict, bare or under 'optimizer_state'): {'state': {i: {'momentum_buffer': t}},
        'param_groups': [{'params': [i...]}]} with i enumerating model.parameters() - so a checkpoint written by
        the reference resumes WITH its state.  A state for another optimizer than the one in force is kept until the
        replayed regime brings its optimizer into force; if it does not, the next adjust / step / state_dict raises.
        Anything else is refused loudly (never a silent restart from zero state)."""
        self._bind()
        name, bufs, t = self._parse_state(state)
        self._pending = self._loaded = None
        if self.opt_name in name.split('/'):
            self._apply_loaded(name, bufs, t)
        else:
            self._pending = (name, bufs, t)
        self.hyper.update(state.get('hyper', {}))
        self.reset()          # current_regime_phase = None, setting = defaults: next update() replays the regime
        self._runs = None

    def _parse_state(self, state):
        """-> (optimizer name, or 'Adam/AdamW' for a torch state that fits both; {torch key: {param name: tensor}}; t)."""
        if isinstance(state, dict) and state.get('momentum_buffer') is not None:
            return 'SGD', {'momentum_buffer': state['momentum_buffer']}, 0
        if isinstance(state, dict) and 'optimizer' in state and isinstance(state.get('state'), dict) \
                and 'param_groups' not in state:
            name = state['optimizer']
            if name not in OPTIMIZERS or name == 'SGD':
                raise _lib.ConvNetHipError('OptimRegime.load_state_dict: unknown optimizer %r in the state' % (name,))
            named = state['state']
        else:
            st = state.get('optimizer_state', state) if isinstance(state, dict) else None
            named = _torch_state_by_name(self.model, st)
            if named is None:
                raise _lib.ConvNetHipError(
                    "OptimRegime.load_state_dict: neither this engine's format ('momentum_buffer', or 'optimizer' + "
                    "'state') nor a torch.optim state_dict ('state' + 'param_groups'): refusing to resume from zero "
                    "state (main.py --drop-optim-state skips the optimizer state on purpose)")
            name = None
        keys = set()
        for ent in named.values():
            keys |= set(ent) - {'step'}
        unknown = keys - set(_STATE_ATTR)
        if unknown:
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: unknown state entries %s' % sorted(unknown))
        family = ('Adam/AdamW' if keys == {'exp_avg', 'exp_avg_sq'} else
                  'RMSprop' if keys in ({'square_avg'}, {'square_avg', 'momentum_buffer'}) else
                  'SGD' if keys <= {'momentum_buffer'} else None)
        if family is None or (name is not None and name not in family.split('/')):
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: state entries %s fit %s'
                                       % (sorted(keys), 'no optimizer built here' if name is None else 'not ' + name))
        steps = {int(float(ent['step'])) for ent in named.values() if 'step' in ent}
        if len(steps) > 1:
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: per-parameter step counts differ (%s): the flat '
                                       'arena keeps one' % sorted(steps)[:4])
        if family != 'SGD' and not steps:
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: the state carries no step count')
        params = dict(self.model.named_parameters())
        bufs = {}
        for key in (keys or {'momentum_buffer'}):
            # a parameter that never received a gradient has no entry yet: zero is exactly its state
            bufs[key] = {n: (ent[key] if key in ent else torch.zeros_like(params[n], device='cpu'))
                         for n, ent in named.items()}
        return name or family, bufs, (steps.pop() if steps else 0)

    def _apply_loaded(self, name, bufs, t):
        need = {key for key, attr in _STATE_ATTR.items() if attr in self._needed_state()}
        if set(bufs) != need:
            raise _lib.ConvNetHipError('OptimRegime.load_state_dict: the state holds %s, %s in force keeps %s'
                                       % (sorted(bufs), self._kind(), sorted(need)))
        for key, named in bufs.items():
            self._import(getattr(self, _STATE_ATTR[key]), named, 'momentum buffers' if key == 'momentum_buffer' else key)
        self.step_dev.fill_(t)
        self._pending, self._loaded = None, name

    def _confirm_loaded(self):
        """A loaded state must belong to the optimizer the replayed regime puts in force."""
        name = self._pending[0] if self._pending is not None else self._loaded
        if name is None:
            return
        if self._pending is not None or self.opt_name not in name.split('/'):
            self._pending = self._loaded = None
            raise _lib.ConvNetHipError('OptimRegime: the loaded optimizer state is for %s, the regime puts %s in force'
                                       % (name, self.opt_name))
        self._loaded = None


def _torch_state_by_name(model, st):
    """torch.optim state_dict -> {parameter name: its state entry ({} where torch has none yet)} or None."""
    if not (isinstance(st, dict) and 'state' in st and 'param_groups' in st):
        return None
    order = [i for grp in st['param_groups'] for i in grp['params']]
    names = [n for n, _ in model.named_parameters()]
    if len(order) != len(names):
        raise _lib.ConvNetHipError('OptimRegime.load_state_dict: optimizer state covers %d parameters, the model '
                                   'has %d' % (len(order), len(names)))
    out = {}
    for name, idx in zip(names, order):
        ent = st['state'].get(idx, st['state'].get(str(idx)))
        out[name] = {k: v for k, v in ent.items() if v is not None} if isinstance(ent, dict) else {}
    return out


def deepcopy_regularizer(reg):
    if isinstance(reg, dict):
        reg = [reg]
    return [dict(r) for r in reg]
