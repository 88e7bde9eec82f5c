"""Golden fixtures for duplicates / batch augmentation (tests/test_duplicates.py) from the unmodified reference Trainer on
CPU fp32, with the recipe of oracle/make_golden.py:trajectory: the loader hands over B x D x C x H x W inputs, the
reference flattens them (trainer.py:17-29,214-216: sample-major for chunk_batch == 1, view-major for chunk_batch > 1).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dup.py

Writes under tests/golden/ (data only):
  traj_r18s_dup          make_golden.SMALL depth 18, B = 4, D = 2, 32 x 32, 3 steps, chunk_batch = 1
  traj_r18s_dup_chunk2   the same with chunk_batch = 2 (every accumulation chunk holds one view of every sample)
Both with the grad_clip / loss_scale of traj_r18s.  Recorded: per-step loss / prec1 / prec5 / grad, the final tensors,
`validate` on the first two 5-D batches with average_output False ('validate') and True ('validate_avg'), and the smallest
gap between neighbours among the six largest averaged logits of any validation sample ('avg_top_gap': the averaged prec
values are not decided by a tie when it is well above rounding - asserted > 1e-4 here)."""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402


def dup_batches(n, B, D, size, classes, seed):
    """tests/test_duplicates.py restates this."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, D, 3, size, size, generator=g), torch.randint(0, classes, (B,), generator=g)) for _ in range(n)]


def avg_top_gap(model, data):
    """Smallest difference between neighbours among the six largest duplicate-averaged logits, over every sample."""
    model.eval()
    gap = float('inf')
    with torch.no_grad():
        for x, _ in data:
            B, D = x.shape[:2]
            out = model(x.flatten(0, 1)).view(B, D, -1).mean(1)
            top = out.sort(dim=1, descending=True).values[:, :6]
            gap = min(gap, float((top[:, :-1] - top[:, 1:]).min()))
    return gap


def trajectory(tag, model_kw, B, D, size, classes, steps, seed, chunk_batch):
    torch.manual_seed(123)
    model = mg.ref_models.resnet(dataset='imagenet', **model_kw)
    init_sums = mg.tensor_sums({k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=torch.float,
                       distributed=False, loss_scale=1.0, grad_clip=1e9, print_freq=10 ** 9)
    data = dup_batches(steps, B, D, size, classes, seed)
    recs = []
    for x, t in data:
        r = tr.train([(x, t)], chunk_batch=chunk_batch)
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
    val = tr.validate(data[:2])
    val_avg = tr.validate(data[:2], average_output=True)
    gap = avg_top_gap(model, data[:2])
    assert gap > 1e-4, 'averaged validation logits at a tie (%g): pick another seed' % gap
    sd = model.state_dict()
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'D': D, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': chunk_batch, 'smooth_eps': 0.0, 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
           'validate_avg': {k: float(val_avg[k]) for k in ('loss', 'prec1', 'prec5')},
           'avg_top_gap': gap,
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'init_sums': init_sums,
           'final_sums': mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point}),
           'num_batches_tracked': int(sd['bn1.num_batches_tracked'])}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    keep = ['conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'layer1.0.conv1.weight',
            'layer2.0.downsample.0.weight', 'layer4.1.bn2.weight', 'fc.weight', 'fc.bias']
    torch.save({k: sd[k].clone() for k in keep if k in sd}, os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    print(tag, recs, 'val', out['validate'], 'val avg', out['validate_avg'], 'gap', gap)


if __name__ == '__main__':
    kw = dict(depth=18, **mg.SMALL)
    trajectory('r18s_dup', kw, B=4, D=2, size=32, classes=16, steps=3, seed=61, chunk_batch=1)
    trajectory('r18s_dup_chunk2', kw, B=4, D=2, size=32, classes=16, steps=3, seed=62, chunk_batch=2)
    mg.assert_no_new_bytecode()
