"""MobileNet v1 (the reference's models/mobilenet.py) on the HIP operator modules: a 3x3 / stride-2 stem and 13
depthwise-separable blocks (8 with shallow=True), plain ReLU, no residuals, global average pool, Linear head.  Same module
tree and registration order as the reference - state_dict keys ``features.N.*``, ``features.N.components.{0,1,3,4}.*``,
``fc.*`` - so a seeded construction draws the reference's initial tensors and its checkpoints load strictly.

The depthwise 3x3 convolutions (bias included: the reference keeps nn.Conv2d's default) run on csrc/dwconv.hip
(ops.DepthwiseConv2dFunction); they take no fusion, every BatchNorm runs its plain passes with the ReLU folded into its
apply.  The reference defines an init_model() for this family but never calls it: every tensor keeps its constructor draw,
and so it does here."""
import torch
import torch.nn as tnn

from .. import data as cdata
from .. import nn as cnn

__all__ = ['mobilenet']

_IMAGENET_STATS = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}


def nearby_int(n):
    return int(round(n))


def weight_decay_config(value=1e-4, log=True):
    """models/mobilenet.py:25-36: decay Linear and non-depthwise convolution weights only, never a `bias`.  (`log` is kept
    for the reference's call shape; the regulariser here does not log.)"""
    def regularize_layer(m):
        non_depthwise_conv = isinstance(m, cnn.Conv2d) and m.groups != m.in_channels
        return isinstance(m, cnn.Linear) or non_depthwise_conv

    return {'name': 'WeightDecay', 'value': value, 'log': log,
            'filter': {'parameter_name': lambda n: not n.endswith('bias'), 'module': regularize_layer}}


class DepthwiseSeparableFusedConv2d(tnn.Module):
    """depthwise 3x3 (+ bias) -> BN -> ReLU -> 1x1 -> BN -> ReLU; the parameterless ReLUs keep the Sequential indices of
    the reference, the forward folds them into the BatchNorm apply passes."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.components = tnn.Sequential(
            cnn.Conv2d(in_channels, in_channels, kernel_size, stride=stride, padding=padding, groups=in_channels),
            cnn.BatchNorm2d(in_channels),
            cnn.ReLU(True),
            cnn.Conv2d(in_channels, out_channels, 1, bias=False),
            cnn.BatchNorm2d(out_channels),
            cnn.ReLU(True))

    def forward(self, x):
        c = self.components
        x = c[1](c[0](x), relu=True)
        return c[4](c[3](x), relu=True)


class MobileNet(tnn.Module):

    def __init__(self, width=1., shallow=False, regime=None, num_classes=1000):
        super().__init__()
        num_classes = num_classes or 1000
        width = width or 1.
        w = lambda c: nearby_int(width * c)     # noqa: E731
        layers = [cnn.Conv2d(3, w(32), kernel_size=3, stride=2, padding=1, bias=False), cnn.BatchNorm2d(w(32)),
                  cnn.ReLU(True)]
        plan = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2)]
        if not shallow:
            plan += [(512, 512, 1)] * 5
        plan += [(512, 1024, 2), (1024, 1024, 1)]   # (the reference's stride-1 reading of the paper's last block)
        for cin, cout, stride in plan:
            layers.append(DepthwiseSeparableFusedConv2d(w(cin), w(cout), kernel_size=3, stride=stride, padding=1))
        self.features = tnn.Sequential(*layers)
        self.features[0].needs_dgrad = False
        # biased depthwise outputs and post-ReLU 1x1 products have means of the size of their deviations, and this
        # family amplifies a 1e-5 error of the first step's statistics a hundredfold by the second (NOTES.md):
        # centre every BatchNorm's sums on the batch itself
        for m in self.modules():
            if isinstance(m, cnn.BatchNorm2d):
                m.batch_pivot = True
        self.avg_pool = cnn.AdaptiveAvgPool2d(1)
        self.fc = cnn.Linear(w(1024), num_classes)

        self.data_regime = [{
            'transform': cdata.Compose([cdata.Resize(256), cdata.RandomCrop(224), cdata.RandomHorizontalFlip(),
                                        cdata.ToTensor(), cdata.Normalize(**_IMAGENET_STATS)])
        }]
        if regime == 'small':
            scale_lr = 4
            self.regime = [
                {'epoch': 0, 'optimizer': 'SGD', 'momentum': 0.9, 'lr': scale_lr * 1e-1,
                 'regularizer': weight_decay_config(1e-4)},
                {'epoch': 30, 'lr': scale_lr * 1e-2},
                {'epoch': 60, 'lr': scale_lr * 1e-3},
                {'epoch': 80, 'lr': scale_lr * 1e-4}
            ]
            self.data_regime = [
                {'epoch': 0, 'input_size': 128, 'batch_size': 512},
                {'epoch': 80, 'input_size': 224, 'batch_size': 128},
            ]
            self.data_eval_regime = [
                {'epoch': 0, 'input_size': 128, 'batch_size': 1024},
                {'epoch': 80, 'input_size': 224, 'batch_size': 512},
            ]
        else:
            self.regime = [
                {'epoch': 0, 'optimizer': 'SGD', 'lr': 1e-1, 'momentum': 0.9, 'regularizer': weight_decay_config(1e-4)},
                {'epoch': 30, 'lr': 1e-2},
                {'epoch': 60, 'lr': 1e-3},
                {'epoch': 80, 'lr': 1e-4}
            ]

    def forward(self, x):
        """x: fp32 NCHW (the loader layout) or an already-converted NHWC compute tensor."""
        f = self.features
        stem = f[0]
        if x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != stem.padded_in_channels():
            x = stem.forward_from_nchw(x)
        else:
            x = stem(x)
        x = f[1](x, relu=True)
        for block in list(f)[3:]:
            x = block(x)
        x = self.avg_pool(x)
        return self.fc(x.view(x.size(0), -1))


def mobilenet(**config):
    """Factory with the reference's call shape (models/mobilenet.py:168-178): ImageNet only ('imagenet-synthetic' is this
    package's data-free stand-in for it, main.py's default)."""
    dataset = config.pop('dataset', 'imagenet')
    if dataset not in ('imagenet', 'imagenet-synthetic'):
        raise NotImplementedError("mobilenet is defined for dataset='imagenet' only (got %r; the reference asserts)" % dataset)
    return MobileNet(**config)
