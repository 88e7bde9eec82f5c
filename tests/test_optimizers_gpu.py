"""The adaptive optimizers inside a captured step (`-m gpu`): the step count lives on the device and is advanced by a
launch that is part of the step, so a replayed HIP graph or launch plan - which never calls optimizer.step() on the
host - must give bit for bit what the eager launches give, across a learning-rate change (no re-capture) and across a
switch of optimizer between regime phases (a new capture key).  Each case runs in a fresh child process with its own
time limit, in the manner of tests/test_graph_gpu.py, on that file's small ResNet-50."""
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

WORKER = r'''
import sys, torch
sys.path.insert(0, %(root)r)
import convnet_amd as ca
from convnet_amd.models.resnet import weight_decay_config
torch.cuda.set_device(0)
CASE = %(case)r
kw = dict(depth=50, width=(16, 32, 64, 128), inplanes=16, num_classes=32)
g = torch.Generator().manual_seed(9)
data = [(torch.randn(16, 3, 64, 64, generator=g).cuda(), torch.randint(0, 32, (16,), generator=g).cuda())
        for _ in range(7)]
REGIMES = {
    'Adam': [{'epoch': 0, 'optimizer': 'Adam', 'lr': 1e-3, 'regularizer': weight_decay_config(1e-4)},
             {'epoch': 30, 'lr': 1e-4}],
    'RMSprop': [{'epoch': 0, 'optimizer': 'RMSprop', 'lr': 1e-3, 'alpha': 0.9, 'momentum': 0.9,
                 'regularizer': weight_decay_config(1e-4)},
                {'epoch': 30, 'lr': 1e-4}],
    'switch': [{'epoch': 0, 'optimizer': 'SGD', 'lr': 0.1, 'momentum': 0.9, 'regularizer': weight_decay_config(1e-4)},
               {'epoch': 30, 'optimizer': 'Adam', 'lr': 1e-3}],
}

def run(mode, dtype):
    torch.manual_seed(123)
    model = ca.models.resnet(**kw)
    tr = ca.Trainer(model, ca.CrossEntropyLoss(smooth_eps=0.1), ca.OptimRegime(model, REGIMES[CASE]),
                    device='cuda:0', dtype=dtype, grad_clip=5.0, loss_scale=4.0, print_freq=10**9)
    tr._use_graph = mode != 'eager'
    tr._graph_mode = '0' if mode == 'eager' else '1'     # force the capture ('auto' decides by host vs device time)
    tr._plan = mode == 'plan'
    recs = []
    for i, b in enumerate(data):
        if i == 4:
            tr.epoch = 30            # the lr change / the switch of optimizer
        r = tr.train([b])
        recs.append((r['loss'], r['prec1'], r.get('grad')))
    torch.cuda.synchronize()
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    return recs, sd, tr.optimizer.state_dict(), tr

for dtype in (torch.float32, torch.bfloat16):
    e_recs, e_sd, e_opt, _ = run('eager', dtype)
    steps = 3 if CASE == 'switch' else 7           # (the switch starts Adam at t = 0 in step 4)
    assert e_opt['optimizer'] == ('RMSprop' if CASE == 'RMSprop' else 'Adam')
    assert {e['step'] for e in e_opt['state'].values()} == {steps}, 'eager t'
    for mode in ('graph', 'plan'):
        recs, sd, opt, tr = run(mode, dtype)
        sts = [g['graph'] for g in tr._gstates.values() if g['graph'] is not None]
        assert len(sts) == (2 if CASE == 'switch' else 1), (mode, len(sts), 'captures')    # the switch re-keyed, lr did not
        assert all((st.get('plan') is not None) == (mode == 'plan') for st in sts), mode
        assert recs == e_recs, (mode, dtype, e_recs, recs)
        for k in e_sd:
            assert torch.equal(e_sd[k], sd[k]), (mode, dtype, k)
        assert opt['optimizer'] == e_opt['optimizer'] and sorted(opt['state']) == sorted(e_opt['state'])
        for n, ent in e_opt['state'].items():
            assert opt['state'][n]['step'] == steps, (mode, dtype, n, opt['state'][n]['step'])
            for key, val in ent.items():
                if key != 'step':
                    assert torch.equal(val, opt['state'][n][key]), (mode, dtype, n, key)
print('OPTIM_CAPTURE_OK', CASE)
'''


@pytest.mark.parametrize('case', ['Adam', 'RMSprop', 'switch'])
def test_captured_step_is_bit_identical_to_eager(tmp_path, case):
    """Adam / RMSprop with momentum: eager, forced HIP graph (plan off) and launch plan, fp32 and bf16, 7 steps with the
    lr change at step 4: results per step, the model's and the optimizer's state_dict (t == 7 read back from the device)
    equal the eager run's bit for bit, and a capture / plan was in fact what ran.  'switch': SGD -> Adam at step 4."""
    script = tmp_path / 'optim_capture_worker.py'
    script.write_text(WORKER % {'root': ROOT, 'case': case})
    env = dict(os.environ, CONVNET_AMD_EMULATE='0')
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'OPTIM_CAPTURE_OK ' + case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
