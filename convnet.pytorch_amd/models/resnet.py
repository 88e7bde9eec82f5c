"""ResNet family (ImageNet and CIFAR variants) on the HIP operator modules.

Same factory surface, module tree / ``state_dict`` keys, initialisation and optimisation regimes
as /root/reference models/resnet.py (factory :385-431, ResNet_imagenet :216-317, blocks :81-165,
init_model :16-31, weight-decay filter :34-40), re-expressed as a declarative stage table instead
of hand-written block classes.  ``quantize=True`` (BASELINE config 5; the reference rebinds torch.nn's
Conv2d / Linear / BatchNorm2d to its simulated-8-bit classes, :387-391) builds the same tree from
``convnet.pytorch_amd.quant``'s QConv2d / QLinear / RangeBN.
``bn_norm='L1'`` (the reference rebinds torch.nn's BatchNorm2d to models/modules/lp_norm.py's L1BatchNorm2d, :393-399)
builds the same tree with ``nn.L1BatchNorm2d`` (csrc/l1bn.hip) for the stem, branch and shortcut norms; such a norm takes
part in no convolution-epilogue fusion.  ``resnet_se`` (:434-436 there: resnet(residual_block=SEBlock)) constructs ONE
``nn.SEBlock`` (csrc/se.hip) per stage, hands that same module to every block of the stage and applies it to the SHORTCUT
(z = relu(bn_last(y) + se(r)), r the block input or the shortcut BatchNorm's output); every fusion that rests on the
junction reading the untouched block input is off in such a model.  ``resnet(dataset='cifar10' | 'cifar100')`` is the
reference's ResNet_cifar (:320-383, factory :423-431): a 3x3 / stride 1 stem without max-pool, three stages of basic blocks
(depth = 6n + 2, default 44) at widths 16 / 32 / 64, its two regimes, and ``dropout=p`` behind the first ReLU of every
block; it is built for the default operators only (no quantize / bn_norm / residual_block / groups, no mixup, no "sampled"
regime).  Out of scope here: mixed-size "sampled" regimes, mixup layers, checkpoint_segments, bn_norm='TopK'.

Module construction order and registration order deliberately match the reference, so seeding
torch's RNG and building ``resnet(depth=50)`` yields bit-identical initial weights.
"""
import math

import torch
import torch.nn as tnn

from .. import nn as cnn
from ..ops import ResGradHolder

__all__ = ['resnet', 'resnet_se']

# depth -> (block kind, blocks per stage)      (reference models/resnet.py:403-419)
_IMAGENET_DEPTHS = {
    18: ('basic', (2, 2, 2, 2)),
    34: ('basic', (3, 4, 6, 3)),
    50: ('bottleneck', (3, 4, 6, 3)),
    101: ('bottleneck', (3, 4, 23, 3)),
    152: ('bottleneck', (3, 8, 36, 3)),
    200: ('bottleneck', (3, 24, 36, 3)),
}

# conv plan of a residual branch: (kernel, width multiplier key, takes the block stride?)
_BRANCH = {
    'basic': ((3, 'planes', True), (3, 'out', False)),
    'bottleneck': ((1, 'planes', False), (3, 'planes', True), (1, 'out', False)),
}


def weight_decay_config(value=1e-4, log=False):
    """Regulariser spec of the reference regime (models/resnet.py:34-40): decay every parameter
    whose name does not end in 'bias' and whose module is not a BatchNorm2d (with bn_norm='L1' the reference's
    nn.BatchNorm2d IS its L1BatchNorm2d by then, so that class is exempt in the same way)."""
    return {'name': 'WeightDecay', 'value': value, 'log': log,
            'filter': {'parameter_name': lambda n: not n.endswith('bias'),
                       'module': lambda m: not isinstance(m, (cnn.BatchNorm2d, cnn.L1BatchNorm2d))}}


def linear_scale(lr0, lrT, T, t0=0):
    rate = (lrT - lr0) / T
    return "lambda t: {'lr': max(%s + (t - %s) * %s, 0)}" % (lr0, t0, rate)


def _link_stats(conv, bn):
    """`bn` behind `conv` with every fusion: its statistics come out of the conv epilogue, centred on its running mean, and its
    backward apply can be left to the conv (ops.LAZY_DY).  (Instance dict: neither becomes a sub-module of the other.)"""
    conv.feeds_batchnorm = True
    conv.__dict__['stats_bn'] = bn
    bn.__dict__['producer_conv'] = conv


class ResidualBlock(tnn.Module):
    """BasicBlock / Bottleneck of the reference (models/resnet.py:81-165) built from a branch plan.
    The last BN of the branch fuses `+ residual` and the final ReLU; inner BNs fuse their ReLU."""

    def __init__(self, kind, inplanes, planes, stride, expansion, downsample, op_classes=None, groups=1, norm=None,
                 residual_block=None, dropout=None):
        super().__init__()
        self.kind = kind
        # dropout = p > 0 (ResNet_cifar's blocks): Dropout(p) sits between relu(bn_i(.)) and conv_{i+1}, so that BatchNorm
        # applies its ReLU itself and hands over a materialised tensor, and conv_{i+1} - which reads the dropped tensor, not
        # the BatchNorm's output - does none of that BatchNorm's work: no input_bn, no inner_consumer_conv in this block
        self.drop_p = float(dropout or 0)
        if self.drop_p and (op_classes is not None or kind != 'basic'):
            raise NotImplementedError('dropout inside a residual block is built for the basic block of the default operators')
        # residual_block (resnet_se: the stage's shared nn.SEBlock) gates the shortcut before the junction.  The junction
        # then no longer reads the untouched block input, so everything resting on that is off: no ResGradHolder (the
        # fork adds the two block-input gradients), no junction_conv1, no input_bn / consumer_conv across the block
        # boundary (set_input_bn), no dual apply of the shortcut BatchNorm (its output is pooled first).  The fusions
        # INSIDE the branch and the projection's statistics epilogue do not see the shortcut and stay.
        self.gated = residual_block is not None
        if self.gated and (op_classes is not None or norm is not None):
            raise NotImplementedError('residual_block together with quantize / bn_norm')
        self.quantized = op_classes is not None
        Conv, Norm = op_classes[:2] if self.quantized else (cnn.Conv2d, norm or cnn.BatchNorm2d)
        widths = {'planes': planes, 'out': planes * expansion}
        cin = inplanes
        self.n_convs = len(_BRANCH[kind])
        # groups > 1 (ResNeXt): every 3x3 convolution of the branch is grouped (the reference's conv3x3(..., groups)).
        # A grouped convolution takes part in no fusion: the BatchNorm it feeds runs its standalone passes, and no
        # BatchNorm parks a lazy operand (or its backward reduction) on it; everything else keeps its fusions.
        self.grouped = [k == 3 and groups > 1 for k, _, _ in _BRANCH[kind]]
        # norm (bn_norm='L1'): that norm class runs its standalone passes behind EVERY convolution - the same no-fusion
        # rule, for all of the block's convolutions and its shortcut
        self.unfused_norm = norm is not None
        self.nofuse = [g or self.unfused_norm for g in self.grouped]
        for i, (k, wkey, strided) in enumerate(_BRANCH[kind], start=1):
            cout = widths[wkey]
            gkw = {'groups': groups} if self.grouped[i - 1] else {}
            setattr(self, 'conv%d' % i, Conv(cin, cout, kernel_size=k, stride=stride if strided else 1,
                                             padding=k // 2, bias=False, **gkw))
            setattr(self, 'bn%d' % i, Norm(cout))
            if not self.quantized and not self.nofuse[i - 1]:
                _link_stats(getattr(self, 'conv%d' % i), getattr(self, 'bn%d' % i))
            if i > 1 and not self.quantized and not self.nofuse[i - 1] and not self.nofuse[i - 2] and not self.drop_p:   # this conv reads relu(bn_{i-1}(.)): its dgrad epilogue does that BN's backward reduction
                # (instance dict, not setattr: the BN must not become a registered sub-module of the conv)
                getattr(self, 'conv%d' % i).__dict__['input_bn'] = getattr(self, 'bn%d' % (i - 1))
            if i == 1 and kind == 'basic':
                self.relu = cnn.ReLU(inplace=True)  # registration order of the reference BasicBlock
            cin = cout
        if kind == 'bottleneck':
            self.relu = cnn.ReLU(inplace=True)
            self.dropout = cnn.Dropout(0)
        self.downsample = downsample
        self.residual_block = residual_block    # (registered behind downsample, as in the reference's blocks)
        if kind == 'basic':
            self.dropout = cnn.Dropout(self.drop_p)
        self.stride = stride
        self.expansion = expansion
        if self.quantized:   # the reference's operator chain; what is shared / fused is listed in quant.py
            # the two gradients meeting at the block input are summed in the later data gradient's epilogue
            # (quant.JUNCTION_ADD): conv1 + the identity shortcut's gradient (parked by quant.add_relu), or conv1 + the
            # projection convolution
            self._holder = ResGradHolder()
            self.conv1._res_holder = self._holder
            if downsample is not None:
                downsample[0]._res_holder = self._holder
            if downsample is not None and hasattr(downsample[0], 'quantize_input'):
                # conv1 and the projection read the same block input: one min / max + quantise pass for both
                self.conv1.__dict__['share_q_out'] = True
                downsample[0].__dict__['share_q_from'] = self.conv1
            return
        if self.nofuse[0] or self.gated:
            # conv1 is grouped (ResNeXt BasicBlock), the norms are unfused or the shortcut is gated: the two gradients
            # meeting at the block input are added by the fork
            self._holder = None
            if downsample is not None and not self.unfused_norm:
                _link_stats(downsample[0], downsample[1])
            return
        # the two gradients meeting at the block input are summed inside a dgrad epilogue
        self._holder = ResGradHolder()
        self.conv1._res_holder = self._holder
        self.conv1.__dict__['junction_conv1'] = True   # (never a lazy-dy consumer: ops._lazy_dy_ok)
        if downsample is None:
            self.last_bn()._res_holder = self._holder     # identity: last BN's dres + conv1 dgrad
        else:
            downsample[0]._res_holder = self._holder      # downsample conv dgrad + conv1 dgrad
            _link_stats(downsample[0], downsample[1])

    def last_bn(self):
        return getattr(self, 'bn%d' % self.n_convs)

    def link_inner_consumers(self):
        """bn_i -> relu -> conv_{i+1} run back to back in forward(): a 1x1 convolution on the streaming kernel / a 3x3
        convolution on the 64-channel halo kernel applies that BatchNorm on its operand path (ops.LAZY_A)."""
        if not self.quantized and not self.drop_p:
            for i in range(1, self.n_convs):
                if self.nofuse[i - 1] or self.nofuse[i]:
                    continue
                getattr(self, 'bn%d' % i).__dict__['inner_consumer_conv'] = getattr(self, 'conv%d' % (i + 1))

    def set_input_bn(self, bn):
        """The block input is the output of `bn` (the previous block's last BN, ReLU and residual fused):
        whichever of conv1 / downsample conv completes the input gradient reduces it for that BN."""
        if self.quantized or self.unfused_norm or self.gated:
            return
        if self.downsample is not None:
            self.downsample[0].__dict__['input_bn'] = bn
        if self.grouped[0]:
            return
        self.conv1.__dict__['input_bn'] = bn
        bn.__dict__['consumer_conv'] = self.conv1   # (lazy z: conv1 can apply that junction on its operand load, ops.LAZY_Z)

    def forward(self, x):
        xa, xb = cnn.fork(x, self._holder)
        out = xa
        for i in range(1, self.n_convs):
            out = getattr(self, 'conv%d' % i)(out)
            out = getattr(self, 'bn%d' % i)(out, relu=True)
            if self.drop_p:
                out = self.dropout(out)
        out = getattr(self, 'conv%d' % self.n_convs)(out)
        residual = xb
        if self.quantized:   # bn -> (downsample) -> add -> relu as separate operators, in the reference's order
            out = self.last_bn()(out)
            if self.downsample is not None:
                residual = self.downsample[1](self.downsample[0](xb))
            from ..quant import add_relu
            return add_relu(out, residual, self._holder if self.downsample is None else None)
        if self.downsample is not None:
            ds_conv, ds_bn = self.downsample[0], self.downsample[1]
            from .. import ops
            if ops.DUAL_BN and not self.gated and ds_bn.training and self.last_bn().training and isinstance(ds_bn, cnn.BatchNorm2d) \
                    and ops._sync_group(ds_bn) is None and ops._sync_group(self.last_bn()) is None:
                # the shortcut BatchNorm finalises its statistics only; the junction's apply pass applies both
                residual = ds_bn(ds_conv(xb), defer_apply=True)
                return self.last_bn()(out, residual=residual, relu=True, residual_bn=ds_bn)
            residual = ds_bn(ds_conv(xb))
        if self.gated:
            residual = self.residual_block(residual)
        return self.last_bn()(out, residual=residual, relu=True)


def init_model(model):
    """models/resnet.py:16-31: fan-out normal for convs, BN (1, 0), zero gamma on the last BN of every
    residual block, N(0, 0.01) classifier with zero bias - same draw order as the reference."""
    for m in model.modules():
        if isinstance(m, cnn.Conv2d):
            n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            m.weight.data.normal_(0, math.sqrt(2. / n))
        elif isinstance(m, (cnn.BatchNorm2d, cnn.L1BatchNorm2d)):   # (the reference's rebound nn.BatchNorm2d under bn_norm)
            m.weight.data.fill_(1)
            m.bias.data.zero_()
    for m in model.modules():
        if isinstance(m, ResidualBlock):
            tnn.init.constant_(m.last_bn().weight, 0)
    model.fc.weight.data.normal_(0, 0.01)
    model.fc.bias.data.zero_()


class _ResNetBase(tnn.Module):
    """What the ImageNet and the CIFAR model share: the operator classes in force, the stage builder and forward()."""

    def __init__(self, op_classes=None, norm=None):
        super().__init__()
        self.op_classes = op_classes     # (QConv2d, RangeBN, QLinear) under quantize, else None
        self.norm = norm                 # nn.L1BatchNorm2d under bn_norm='L1'; None: nn.BatchNorm2d with every fusion

    def _link_blocks(self, first_input_bn=None):
        """Registration order = execution order of the residual blocks: each block learns which BatchNorm made its input."""
        prev_bn = first_input_bn
        for m in self.modules():
            if isinstance(m, ResidualBlock):
                if prev_bn is not None:
                    m.set_input_bn(prev_bn)
                m.link_inner_consumers()
                prev_bn = m.last_bn()

    def forward(self, x):
        return self.fc(self.features(x))

    def _make_layer(self, kind, planes, blocks, expansion, stride, groups=1, residual_block=None, dropout=None):
        out_planes = planes * expansion
        downsample = None
        if stride != 1 or self.inplanes != out_planes:  # models/resnet.py:176-181
            Conv, Norm = (self.op_classes or (cnn.Conv2d, self.norm or cnn.BatchNorm2d))[:2]
            downsample = tnn.Sequential(
                Conv(self.inplanes, out_planes, kernel_size=1, stride=stride, bias=False),
                Norm(out_planes))
        if residual_block is not None:
            # models/resnet.py:182-183: ONE module per stage, constructed (its initial weights drawn) behind the stage's
            # downsample and before its blocks, and handed to every block
            residual_block = residual_block(out_planes)
        stage = [ResidualBlock(kind, self.inplanes, planes, stride, expansion, downsample, self.op_classes, groups, self.norm,
                               residual_block, dropout)]
        self.inplanes = out_planes
        for _ in range(1, blocks):
            stage.append(ResidualBlock(kind, self.inplanes, planes, 1, expansion, None, self.op_classes, groups, self.norm,
                                       residual_block, dropout))
        return tnn.Sequential(*stage)


class ResNetImagenet(_ResNetBase):
    num_train_images = 1281167

    def __init__(self, num_classes=1000, inplanes=64, block='bottleneck', layers=(3, 4, 23, 3),
                 width=(64, 128, 256, 512), expansion=4, regime='normal', scale_lr=1, ramp_up_lr=True,
                 ramp_up_epochs=5, epochs=90, base_devices=4, base_device_batch=64, quantize=False,
                 groups=(1, 1, 1, 1), bn_norm=None, residual_block=None):
        super().__init__()
        if residual_block is not None and (quantize or bn_norm is not None):
            raise NotImplementedError('residual_block (resnet_se) together with quantize=True or bn_norm=%r: the gated '
                                      'shortcut is built for the default operators only' % (bn_norm,))
        groups = [int(g) for g in groups]
        if len(groups) != len(layers) or min(groups) < 1:
            raise ValueError('groups must give one positive group count per stage, got %r' % (groups,))
        if quantize and max(groups) > 1:
            raise NotImplementedError('quantize=True with grouped convolutions (groups=%r): the quantised operators are '
                                      'dense-only' % (groups,))
        if bn_norm not in (None, 'L1'):
            raise NotImplementedError("bn_norm=%r: 'L1' (nn.L1BatchNorm2d) is the norm option built natively" % (bn_norm,))
        if quantize and bn_norm is not None:
            raise NotImplementedError('quantize=True together with bn_norm=%r: the quantised model keeps its RangeBN' % (bn_norm,))
        self.norm = cnn.L1BatchNorm2d if bn_norm == 'L1' else None   # None: nn.BatchNorm2d with every fusion
        self.inplanes = inplanes
        self.op_classes = None
        if quantize:
            from .. import quant
            self.op_classes = (quant.QConv2d, quant.RangeBN, quant.QLinear)
        Conv, Norm, Dense = self.op_classes or (cnn.Conv2d, self.norm or cnn.BatchNorm2d, cnn.Linear)
        self.conv1 = Conv(3, inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.conv1.needs_dgrad = False  # network input needs no gradient
        self.conv1.feeds_batchnorm = not quantize and self.norm is None
        self.bn1 = Norm(inplanes)
        if not quantize and self.norm is None:
            self.conv1.__dict__['stats_bn'] = self.bn1   # the stem's statistics partials are centred on bn1.running_mean
        self.relu = cnn.ReLU(inplace=True)
        self.maxpool = cnn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for i, nblocks in enumerate(layers):
            setattr(self, 'layer%d' % (i + 1),
                    self._make_layer(block, width[i], nblocks, expansion, stride=1 if i == 0 else 2, groups=groups[i],
                                     residual_block=residual_block))
        self._link_blocks()
        self.avgpool = cnn.AdaptiveAvgPool2d(1)
        self.fc = Dense(width[-1] * expansion, num_classes)
        init_model(self)

        batch_size = base_devices * base_device_batch
        num_steps_epoch = math.floor(self.num_train_images / batch_size)
        ramp_up_steps = num_steps_epoch * ramp_up_epochs
        self.regime = [
            {'epoch': 0, 'optimizer': 'SGD', 'lr': scale_lr * 1e-1, 'momentum': 0.9,
             'regularizer': weight_decay_config(1e-4)},
            {'epoch': 30, 'lr': scale_lr * 1e-2},
            {'epoch': 60, 'lr': scale_lr * 1e-3},
            {'epoch': 80, 'lr': scale_lr * 1e-4},
        ]
        if 'cutmix' in regime:
            self.regime = [
                {'epoch': 0, 'optimizer': 'SGD', 'lr': scale_lr * 1e-1, 'momentum': 0.9,
                 'regularizer': weight_decay_config(1e-4)},
                {'epoch': 75, 'lr': scale_lr * 1e-2},
                {'epoch': 150, 'lr': scale_lr * 1e-3},
                {'epoch': 225, 'lr': scale_lr * 1e-4},
            ]
        if 'linear' in regime:
            self.regime = [
                {'epoch': 0, 'optimizer': 'SGD', 'lr': scale_lr * 1e-1, 'momentum': 0.9,
                 'regularizer': weight_decay_config(1e-4),
                 'step_lambda': linear_scale(scale_lr * 1e-1, 0, num_steps_epoch * epochs)},
            ]
            if ramp_up_lr:
                # the reference (models/resnet.py:269-276) would start this regime at lr 0 and append a ramp-up
                # phase, but crashes on `self.regime['step_lambda']` (a list indexed by a string); here the
                # linear decay runs without warm-up, and says so
                import logging
                logging.warning("resnet(regime='linear'): ramp_up_lr is ignored (linear decay from %g without "
                                "warm-up; the reference raises a TypeError for this combination)", scale_lr * 1e-1)
            ramp_up_lr = False
        if ramp_up_lr and scale_lr > 1:  # learning-rate ramp-up (models/resnet.py:313-317)
            self.regime[0]['step_lambda'] = linear_scale(0.1, 0.1 * scale_lr, ramp_up_steps)
            self.regime.insert(1, {'epoch': ramp_up_epochs, 'lr': scale_lr * 1e-1})

    def features(self, x):
        """x: fp32 NCHW (the loader layout) or an already-converted NHWC compute tensor."""
        if self.op_classes is not None and self.training:
            from .. import quant
            quant.tick(x.device)    # fresh stochastic-rounding noise for this step's gradient quantisers
        if x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != self.conv1.padded_in_channels():
            x = self.conv1.forward_from_nchw(x)
        else:
            x = self.conv1(x)
        x = cnn.bn_relu_maxpool(self.bn1, self.maxpool, x)
        from .. import ops
        ops.LAZY_Z_SCOPE[0] += 1    # block b's junction may be left to block b+1's conv1: it runs next, by construction
        try:
            x = self.layer1(x)
            x = self.layer2(x)
            x = self.layer3(x)
            x = self.layer4(x)
        finally:
            ops.LAZY_Z_SCOPE[0] -= 1
        x = self.avgpool(x)
        return x.view(x.size(0), -1)


class ResNetCifar(_ResNetBase):
    """ResNet_cifar of the reference (models/resnet.py:320-383): conv3x3(3, inplanes) / stride 1 -> bn1 + ReLU, no max-pool,
    three stages of n = (depth - 2) // 6 basic blocks (strides 1, 2, 2; a projection shortcut where the stride is not 1 or the
    width changes), global average pool, Linear(width[-1], num_classes).  Same construction / registration order, so a seeded
    build draws the reference's initial tensors."""

    def __init__(self, num_classes=10, inplanes=16, depth=18, width=(16, 32, 64), regime='normal', dropout=None):
        super().__init__()
        if 'sampled' in regime:
            raise NotImplementedError("resnet(dataset='cifar...', regime=%r): mixed-size \"sampled\" data regimes (and their "
                                      "GradSmooth regulariser) are not built" % (regime,))
        if len(width) != 3:
            raise ValueError('a CIFAR ResNet has three stages: width must give three values, got %r' % (width,))
        n = int((depth - 2) / 6)
        if n < 1:
            raise ValueError('unsupported CIFAR ResNet depth %r (depth = 6n + 2, n >= 1)' % (depth,))
        self.inplanes = inplanes
        self.conv1 = cnn.Conv2d(3, inplanes, kernel_size=3, stride=1, padding=1, bias=False)
        self.conv1.needs_dgrad = False  # network input needs no gradient
        self.bn1 = cnn.BatchNorm2d(inplanes)
        _link_stats(self.conv1, self.bn1)
        self.relu = cnn.ReLU(inplace=True)
        for i in range(3):
            setattr(self, 'layer%d' % (i + 1),
                    self._make_layer('basic', width[i], n, 1, stride=1 if i == 0 else 2, dropout=dropout))
        # (the first block reads relu(bn1(.)) of the stem: a BatchNorm output like any block junction's)
        self._link_blocks(first_input_bn=self.bn1)
        self.avgpool = cnn.AdaptiveAvgPool2d(1)
        self.fc = cnn.Linear(width[-1], num_classes)
        init_model(self)
        self.regime = [
            {'epoch': 0, 'optimizer': 'SGD', 'lr': 1e-1, 'momentum': 0.9, 'regularizer': weight_decay_config(1e-4)},
            {'epoch': 81, 'lr': 1e-2},
            {'epoch': 122, 'lr': 1e-3},
            {'epoch': 164, 'lr': 1e-4},
        ]
        if 'wide-resnet' in regime:
            self.regime = [
                {'epoch': 0, 'optimizer': 'SGD', 'lr': 1e-1, 'momentum': 0.9, 'regularizer': weight_decay_config(5e-4)},
                {'epoch': 60, 'lr': 2e-2},
                {'epoch': 120, 'lr': 4e-3},
                {'epoch': 160, 'lr': 8e-4},
            ]

    def features(self, x):
        """x: fp32 NCHW (the loader layout) or an already-converted NHWC compute tensor (data.DeviceCifarLoader's)."""
        if x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != self.conv1.padded_in_channels():
            x = self.conv1.forward_from_nchw(x)
        else:
            x = self.conv1(x)
        x = self.bn1(x, relu=True)
        from .. import ops
        ops.LAZY_Z_SCOPE[0] += 1
        try:
            x = self.layer1(x)
            x = self.layer2(x)
            x = self.layer3(x)
        finally:
            ops.LAZY_Z_SCOPE[0] -= 1
        x = self.avgpool(x)
        return x.view(x.size(0), -1)


def resnet(**config):
    """Factory with the reference's call shape: resnet(dataset=..., depth=..., **kw); groups=[g1, g2, g3, g4] makes
    every 3x3 convolution of stage i grouped (the reference's ResNet_imagenet(groups=...), ResNeXt's building block);
    bn_norm='L1' puts nn.L1BatchNorm2d in the place of every BatchNorm2d (the reference's models/resnet.py:393-399)."""
    dataset = config.pop('dataset', 'imagenet')
    bn_norm = config.pop('bn_norm', None) or None
    if bn_norm == 'TopK':
        raise NotImplementedError("resnet(bn_norm='TopK') needs a per-channel top-k selection kernel that is not built; "
                                  "bn_norm='L1' is")
    if bn_norm is not None and bn_norm != 'L1':
        raise ValueError("bn_norm must be None or 'L1', got %r" % (bn_norm,))
    config['bn_norm'] = bn_norm
    config['quantize'] = bool(config.pop('quantize', False))
    if 'cifar10' in dataset:       # ('cifar100' contains 'cifar10'; 'cifar10-synthetic' names the same model)
        return _resnet_cifar(dataset, config)
    if 'imagenet' not in dataset:
        raise NotImplementedError("the ImageNet and CIFAR ResNet variants are built natively (dataset=%r)" % dataset)
    config.setdefault('num_classes', 1000)
    depth = config.pop('depth', 50)
    if depth not in _IMAGENET_DEPTHS:
        raise ValueError('unsupported ResNet depth %r' % depth)
    kind, layers = _IMAGENET_DEPTHS[depth]
    config.update(block=kind, layers=layers)
    if kind == 'basic':
        config['expansion'] = 1
    return ResNetImagenet(**config)


def _resnet_cifar(dataset, config):
    """models/resnet.py:423-431: 10 / 100 classes, depth 44.  What the reference would build from the remaining options is
    refused by name: none of them has CIFAR-sized kernels or a fixture here."""
    for key, why in (('quantize', 'the quantised operators are built and measured for the ImageNet model only'),
                     ('bn_norm', 'the L1 norm is wired into the ImageNet model only'),
                     ('residual_block', 'the gated shortcut (resnet_se) is built for the ImageNet model only'),
                     ('mixup', "the reference's MixUp layers are not built")):
        if config.pop(key, None):
            raise NotImplementedError("resnet(dataset=%r, %s=...): %s" % (dataset, key, why))
    groups = config.pop('groups', None)
    if groups is not None and any(int(g) != 1 for g in groups):
        raise NotImplementedError('resnet(dataset=%r, groups=%r): grouped convolutions are built for the ImageNet model '
                                  '(ResNeXt) only' % (dataset, groups))
    config.setdefault('num_classes', 100 if 'cifar100' in dataset else 10)
    config.setdefault('depth', 44)
    return ResNetCifar(**config)


def resnet_se(**config):
    """The reference's resnet_se (models/resnet.py:434-436): resnet(residual_block=SEBlock, **config).  depth and groups as
    for resnet; quantize=True, bn_norm=... and a non-ImageNet dataset are refused."""
    if config.get('quantize'):
        raise NotImplementedError('resnet_se(quantize=True): the gated shortcut is built for the default operators only')
    if config.get('bn_norm'):
        raise NotImplementedError('resnet_se(bn_norm=%r): the gated shortcut is built for nn.BatchNorm2d only'
                                  % (config['bn_norm'],))
    config['residual_block'] = cnn.SEBlock
    return resnet(**config)
