"""CIFAR ResNet training rate on one GPU, bf16, three input paths alternated in one process:

  (i)   synthetic   resident synthetic batches in the loader layout (fp32 NCHW on the device): the step alone
  (ii)  resident    data.DeviceCifarLoader on generated CIFAR-10 pickle files (50 000 images, 150 MB in device memory):
                    csrc/augment.hip cuts every batch, with cutout
  (iii) workers     the reference's worker pipeline (data.DataRegime without device_normalize: PIL RandomCrop / flip /
                    ToTensor / Normalize in `--workers` DataLoader processes, pinned fp32 batches, trainer.DevicePrefetcher)

    python tools/bench_cifar.py [--batches 128,256] [--depth 44] [--rounds 3] [--seconds 1.5] [--workers 16] [--only synthetic]

Per batch size one model and Trainer serve all variants (each input form has its own recorded plan).  Per variant: warm-up
steps, then chunks of `--chunk` steps are timed until `--seconds` have passed, with one synchronise at the end; the
variants alternate inside every round, so the spread between rounds of one variant stands beside the difference between
variants.  The last line printed is one JSON object: img/s of every round.  `--only synthetic --rounds 1` is the short run a
`rocprofv3 --kernel-trace --stats` pass wraps (tracing slows the host: its rates are not comparable)."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import convnet_amd as ca  # noqa: E402
from convnet_amd import data as cdata  # noqa: E402
from convnet_amd.main import SyntheticLoader  # noqa: E402


def make_pickles(root, n=50000):
    d = os.path.join(root, 'cifar10', 'cifar-10-batches-py')
    os.makedirs(d)
    rs = np.random.RandomState(0)
    for name, m in [('data_batch_%d' % i, n // 5) for i in range(1, 6)] + [('test_batch', 1000)]:
        with open(os.path.join(d, name), 'wb') as f:
            pickle.dump({'data': rs.randint(0, 256, size=(m, 3072), dtype=np.uint8), 'labels': rs.randint(0, 10, m).tolist()}, f)


class Stream(object):
    """An endless stream of batches over a loader's epochs, handed out `n` at a time (an epoch of 50 000 images is 390 steps:
    the timed chunks are shorter, and the worker pool is never torn down between them)."""

    def __init__(self, loader, n):
        self.loader, self.n, self.it = loader, n, None

    def __len__(self):
        return self.n

    def __iter__(self):
        for _ in range(self.n):
            try:
                if self.it is None:
                    raise StopIteration
                yield next(self.it)
            except StopIteration:
                self.it = iter(self.loader)
                yield next(self.it)


def rate(tr, stream, batch, seconds, warm):
    stream.n, n_timed = warm, stream.n
    tr.train(stream)
    stream.n = n_timed
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        tr.train(stream)
        n += len(stream) * batch
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,256')
    ap.add_argument('--depth', type=int, default=44)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=1.5)
    ap.add_argument('--chunk', type=int, default=40, help='steps per timed train() call')
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--images', type=int, default=50000)
    ap.add_argument('--only', default='synthetic,resident,workers')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cifar.py measures on a GPU: none is visible')
    dev = torch.device('cuda', 0)
    only = args.only.split(',')
    out = {'depth': args.depth, 'dtype': 'bf16', 'device': torch.cuda.get_device_name(0), 'build': ca._lib.build_hash(),
           'images': args.images, 'workers': args.workers, 'unit': 'img/s per round'}
    with tempfile.TemporaryDirectory() as root:
        make_pickles(root, args.images)
        ds = cdata.get_dataset('cifar10', 'train', datasets_path=root)
        for batch in [int(b) for b in args.batches.split(',')]:
            torch.manual_seed(1)
            model = ca.models.resnet(dataset='cifar10', depth=args.depth)
            tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device='cuda:0',
                            dtype=torch.bfloat16, print_freq=10 ** 9)
            loaders = {}
            if 'synthetic' in only:
                loaders['synthetic'] = SyntheticLoader(args.chunk, batch, 32, 10, 3, 5, device=dev)
            if 'resident' in only:
                loaders['resident'] = cdata.DeviceCifarLoader(ds, batch, dev, torch.bfloat16, augment=True,
                                                              cutout={'holes': 1, 'length': 16})
            regime = None
            if 'workers' in only:
                regime = cdata.DataRegime(None, defaults={
                    'datasets_path': root, 'name': 'cifar10', 'split': 'train', 'augment': True, 'batch_size': batch,
                    'shuffle': True, 'num_workers': args.workers, 'pin_memory': True, 'drop_last': True,
                    'cutout': {'holes': 1, 'length': 16}, 'device_normalize': False})
                loaders['workers'] = regime.get_loader()
            streams = {k: Stream(ld, args.chunk) for k, ld in loaders.items()}
            res = {k: [] for k in streams}
            for r in range(args.rounds):
                for k, st in streams.items():
                    res[k].append(round(rate(tr, st, batch, args.seconds, 8 if r == 0 else 2)))
            res['final_loss_finite'] = bool(all(torch.isfinite(p).all() for p in model.parameters()))
            res['plans'] = sum(1 for s in tr._gstates.values() if s['graph'] is not None and s['graph'].get('plan') is not None)
            out['b%d' % batch] = res
            print('b=%d' % batch, res, flush=True)
            for st in streams.values():
                st.it = None          # (shuts the worker pool of this batch size down)
            del streams, loaders, regime
    print(json.dumps(out))


if __name__ == '__main__':
    main()
