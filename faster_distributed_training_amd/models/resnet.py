"""ResNet family with the CIFAR stem and the FusedConvBN "module fusion" trick.

Architecture and parameter names follow the reference exactly so checkpoints are
interchangeable (``resnet.py:147-313``; key schema in survey §2.8):

* ``conv1 = Sequential(FusedConvBN(3, 64, 3, padding=1), CELU(0.075))`` (``resnet.py:237-240``)
* stages ``conv2_x..conv5_x`` with strides 1, 2, 2, 2 (``resnet.py:243-246``)
* BottleNeck stride-1: 3 x FusedConvBN (1x1, 3x3, 1x1) with ReLU between
  (``resnet.py:210-216``); stride-2: FusedConvBN 1x1 -> Conv2d 3x3 s2 + BatchNorm2d + ReLU
  -> FusedConvBN 1x1 (``resnet.py:201-208``)
* shortcut ``Conv2d 1x1 (stride s) + BatchNorm2d`` when the shape changes (``resnet.py:220-224``)
* BasicBlock uses CELU(0.075) (``resnet.py:147-190``)

On MI355X the whole network body runs through ``ops/resnet_fused.py`` (NHWC bf16,
hand-written MFMA implicit-GEMM conv kernels with batch-norm statistics in the epilogue
and normalisation + activation fused into the consumer's operand load); the
``nn.Sequential`` structure below is the CPU/oracle path and defines the state_dict.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..ops import _native
from ..ops.conv_bn import conv_bn_reference


class FusedConvBN(nn.Module):
    """Conv2d (no bias) followed by batch-statistics normalisation without affine.

    Same constructor as the reference (``resnet.py:116-131``); ``exp_avg_factor`` is
    accepted and ignored exactly like the reference (no running statistics, survey Q1).
    Only ``stride == 1`` is supported, as in the reference (``resnet.py:120``).

    ``enable_running_stats`` adds opt-in, non-persistent running statistics (mean and unbiased
    variance of the conv output): updated by train-mode forwards, and used instead of the batch's
    by eval forwards of a model whose ``eval_stats`` is ``"running"`` (``frozen``), so an
    image's output no longer depends on the rest of its batch.
    """
    track_running_stats = False
    momentum = 0.1   # None or < 0: cumulative average (as nn.BatchNorm2d's momentum=None)
    frozen = False   # eval forward normalises with the running statistics

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0,
                 exp_avg_factor=0.1, eps=1e-3, device=None, dtype=None):
        super().__init__()
        assert stride == 1
        factory_kwargs = {"device": device, "dtype": dtype}
        self.conv_weight = nn.Parameter(
            torch.empty(out_channels, in_channels, kernel_size, kernel_size, **factory_kwargs))
        self.num_features = out_channels
        self.in_channels = in_channels
        self.kernel_size = kernel_size
        self.eps = eps
        self.stride = stride
        self.padding = padding
        self.reset_parameters(in_channels, kernel_size)

    def forward(self, X):
        if not self.track_running_stats:
            return conv_bn_reference(X, self.conv_weight, self.stride, self.padding, self.eps)
        y = nn.functional.conv2d(X, self.conv_weight, stride=self.stride, padding=self.padding)
        dims = (0, 2, 3)
        if not self.training and self.frozen:
            mean = self.running_mean.to(y.dtype)[None, :, None, None]
            sd = self.running_var.clamp_min(0).sqrt().to(y.dtype)[None, :, None, None]
            return (y - mean) / (sd + self.eps)
        mean = y.mean(dim=dims, keepdim=True)
        var = y.var(dim=dims, unbiased=True, keepdim=True)
        if self.training:
            with torch.no_grad():
                self.num_batches_tracked += 1
                m = self.momentum
                if m is None or m < 0:
                    m = 1.0 / float(self.num_batches_tracked)
                self.running_mean.mul_(1.0 - m).add_(mean.detach().flatten().float(), alpha=m)
                self.running_var.mul_(1.0 - m).add_(var.detach().flatten().float(), alpha=m)
        return (y - mean) / (var.sqrt() + self.eps)

    def enable_running_stats(self, momentum=0.1):
        if not self.track_running_stats:
            dev = self.conv_weight.device
            # non-persistent: state_dict() keeps the reference checkpoint schema
            self.register_buffer("running_mean", torch.zeros(self.num_features, device=dev), persistent=False)
            self.register_buffer("running_var", torch.ones(self.num_features, device=dev), persistent=False)
            self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long, device=dev),
                                 persistent=False)
            self.track_running_stats = True
        self.momentum = momentum

    def reset_running_stats(self):
        if self.track_running_stats:
            self.running_mean.zero_()
            self.running_var.fill_(1)
            self.num_batches_tracked.zero_()

    def reset_parameters(self, in_channels, kernel_size) -> None:
        n = in_channels * kernel_size * kernel_size
        stdv = 1.0 / math.sqrt(n)
        with torch.no_grad():
            self.conv_weight.uniform_(-stdv, stdv)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.num_features}, kernel_size={self.kernel_size}, "
                f"padding={self.padding}, eps={self.eps}")


class BasicBlock(nn.Module):
    """ResNet-18/34 block (``resnet.py:147-190``): CELU(0.075) activations."""
    expansion = 1

    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        if stride != 1:
            self.residual_function = nn.Sequential(
                nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False),
                nn.BatchNorm2d(out_channels),
                nn.CELU(alpha=0.075, inplace=True),
                FusedConvBN(out_channels, out_channels * BasicBlock.expansion, kernel_size=3, padding=1),
            )
        else:
            self.residual_function = nn.Sequential(
                FusedConvBN(in_channels, out_channels, kernel_size=3, padding=1),
                nn.CELU(alpha=0.075, inplace=True),
                FusedConvBN(out_channels, out_channels * BasicBlock.expansion, kernel_size=3, padding=1),
            )
        self.shortcut = nn.Sequential()
        if stride != 1 or in_channels != BasicBlock.expansion * out_channels:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_channels, out_channels * BasicBlock.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(out_channels * BasicBlock.expansion),
            )
        self.stride = stride

    def forward(self, x):
        return nn.functional.celu(self.residual_function(x) + self.shortcut(x), alpha=0.075)


class BottleNeck(nn.Module):
    """ResNet-50/101/152 block (``resnet.py:193-227``)."""
    expansion = 4

    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        if stride != 1:
            self.residual_function = nn.Sequential(
                FusedConvBN(in_channels, out_channels, kernel_size=1),
                nn.ReLU(inplace=True),
                nn.Conv2d(out_channels, out_channels, stride=stride, kernel_size=3, padding=1, bias=False),
                nn.BatchNorm2d(out_channels),
                nn.ReLU(inplace=True),
                FusedConvBN(out_channels, out_channels * BottleNeck.expansion, kernel_size=1),
            )
        else:
            self.residual_function = nn.Sequential(
                FusedConvBN(in_channels, out_channels, kernel_size=1),
                nn.ReLU(inplace=True),
                FusedConvBN(out_channels, out_channels, kernel_size=3, padding=1),
                nn.ReLU(inplace=True),
                FusedConvBN(out_channels, out_channels * BottleNeck.expansion, kernel_size=1),
            )
        self.shortcut = nn.Sequential()
        if stride != 1 or in_channels != out_channels * BottleNeck.expansion:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_channels, out_channels * BottleNeck.expansion, stride=stride, kernel_size=1, bias=False),
                nn.BatchNorm2d(out_channels * BottleNeck.expansion),
            )
        self.stride = stride

    def forward(self, x):
        return torch.relu(self.residual_function(x) + self.shortcut(x))


class ResNet(nn.Module):
    """CIFAR ResNet (``resnet.py:230-283``).

    ``fast_path``: ``None`` = automatic (HIP engine when the input is on the GPU and the
    native extension is enabled), ``True``/``False`` to force.

    ``eval_stats``: ``"batch"`` (default: FusedConvBN units normalise with the statistics of
    the batch they are given, in eval too, like the reference) or ``"running"`` (eval forwards
    use the tracked running statistics of every unit -- ``enable_running_stats`` -- and so are
    independent of the batch composition; on the GPU they run as the frozen engine forward).
    """

    def __init__(self, block, num_block, num_classes=100):
        super().__init__()
        self.in_channels = 64
        self.conv1 = nn.Sequential(
            FusedConvBN(3, 64, kernel_size=3, padding=1),
            nn.CELU(alpha=0.075, inplace=True))
        self.conv2_x = self._make_layer(block, 64, num_block[0], 1)
        self.conv3_x = self._make_layer(block, 128, num_block[1], 2)
        self.conv4_x = self._make_layer(block, 256, num_block[2], 2)
        self.conv5_x = self._make_layer(block, 512, num_block[3], 2)
        self.avg_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        self.block = block
        self.num_block = list(num_block)
        self.fast_path = None
        self._engine = None
        self._eval_stats = "batch"

    def _make_layer(self, block, out_channels, num_blocks, stride):
        strides = [stride] + [1] * (num_blocks - 1)
        layers = []
        for s in strides:
            layers.append(block(self.in_channels, out_channels, s))
            self.in_channels = out_channels * block.expansion
        return nn.Sequential(*layers)

    @property
    def eval_stats(self):
        return self._eval_stats

    @eval_stats.setter
    def eval_stats(self, mode):
        if mode not in ("batch", "running"):
            raise ValueError(f"eval_stats must be 'batch' or 'running', not {mode!r}")
        units = [m for m in self.modules() if isinstance(m, FusedConvBN)]
        if mode == "running":
            if getattr(self, "_fsdp", None) is not None:
                raise RuntimeError("eval_stats='running' is not supported on an FSDP-sharded model")
            if not all(m.track_running_stats for m in units):
                raise RuntimeError("eval_stats='running' needs tracked statistics: call enable_running_stats(model) "
                                   "first")
        for m in units:
            m.frozen = mode == "running"
        self._eval_stats = mode

    def use_fast_path(self, x: torch.Tensor) -> bool:
        if self.fast_path is None:
            return _native.use_native(x)
        return bool(self.fast_path) and x.is_cuda

    def forward(self, x):
        if self.use_fast_path(x):
            from ..ops.resnet_fused import resnet_engine_forward
            return resnet_engine_forward(self, x)
        return self.forward_reference(x)

    def forward_reference(self, x):
        out = self.conv1(x)
        out = self.conv2_x(out)
        out = self.conv3_x(out)
        out = self.conv4_x(out)
        out = self.conv5_x(out)
        out = self.avg_pool(out)
        out = out.view(out.size(0), -1)
        return self.fc(out)


def resnet18(num_classes=10):
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes=num_classes)


def resnet34(num_classes=10):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes=num_classes)


def resnet50(num_classes=10):
    return ResNet(BottleNeck, [3, 4, 6, 3], num_classes=num_classes)


def resnet101(num_classes=10):
    return ResNet(BottleNeck, [3, 4, 23, 3], num_classes=num_classes)


def resnet152(num_classes=10):
    return ResNet(BottleNeck, [3, 8, 36, 3], num_classes=num_classes)


def _fused_units(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, FusedConvBN)]


def enable_running_stats(model: nn.Module, momentum=0.1):
    """Register ``running_mean`` (0), ``running_var`` (1) and ``num_batches_tracked`` (0) on every
    FusedConvBN of ``model`` (non-persistent buffers: ``state_dict()`` is unchanged) and track
    them in train-mode forwards from now on.  Returns ``model``."""
    for _, m in _fused_units(model):
        m.enable_running_stats(momentum)
    return model


def running_stats_state(model: nn.Module) -> dict:
    """The FusedConvBN running statistics by module name (CPU copies): what a checkpoint stores
    next to the reference-schema ``net`` entry."""
    out = {}
    for n, m in _fused_units(model):
        if m.track_running_stats:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"{n}.{k}"] = getattr(m, k).detach().cpu().clone()
    return out


def load_running_stats(model: nn.Module, state: dict):
    """Import what ``running_stats_state`` exported (enables tracking where it is off; every
    unit keeps its momentum)."""
    units = _fused_units(model)
    want = {f"{n}.{k}" for n, _ in units for k in ("running_mean", "running_var", "num_batches_tracked")}
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
    if set(state) != want:
        missing, extra = sorted(want - set(state)), sorted(set(state) - want)
        raise KeyError(f"running statistics do not match the model: missing {missing[:3]}, unexpected {extra[:3]}")
    with torch.no_grad():
        for n, m in units:
            m.enable_running_stats(m.momentum)
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                getattr(m, k).copy_(state[f"{n}.{k}"])
    return model


@torch.no_grad()
def calibrate_running_stats(model: nn.Module, batches):
    """Replace the running statistics of every FusedConvBN and BatchNorm2d unit by the plain
    average of the batch statistics over ``batches`` (an iterable of image batches, or of (x, y)
    pairs): reset, train-mode forwards without gradients under cumulative averaging, then each
    unit's momentum and the model's train / eval state are restored.  Makes a checkpoint in the
    reference schema (no FusedConvBN statistics) deployable with ``eval_stats='running'``, and
    swaps statistics gathered on mixup-blended inputs for those of clean images.  FusedConvBN
    units that do not track yet start to (as ``enable_running_stats``): later train-mode
    forwards update the statistics too."""
    for _, m in _fused_units(model):
        if not m.track_running_stats:
            m.enable_running_stats()
    units = [m for m in model.modules() if isinstance(m, (FusedConvBN, nn.BatchNorm2d)) and m.track_running_stats]
    saved = [(m, m.momentum) for m in units]
    was_training = model.training
    for m in units:
        m.reset_running_stats()
        m.momentum = None
    n = 0
    try:
        model.train()
        for b in batches:
            x = b[0] if isinstance(b, (tuple, list)) else b
            model(x)
            n += 1
    finally:
        for m, mom in saved:
            m.momentum = mom
        model.train(was_training)
    if n == 0:
        raise ValueError("calibrate_running_stats needs at least one batch")
    return model


def flops_per_image(model: ResNet, hw: int = 32) -> float:
    """Forward FLOPs (2*MACs) of convs + fc for one ``hw x hw`` image (survey: 2.60 GFLOP
    for ResNet-50)."""
    total = 0.0
    h = hw
    hooks = []

    def conv_hook(mod, inp, out):
        nonlocal total
        w = mod.conv_weight if isinstance(mod, FusedConvBN) else mod.weight
        total += 2.0 * w.numel() * out.shape[-1] * out.shape[-2]

    for m in model.modules():
        if isinstance(m, (FusedConvBN, nn.Conv2d)):
            hooks.append(m.register_forward_hook(conv_hook))
    fp = model.fast_path
    model.fast_path = False
    with torch.no_grad():
        model.forward_reference(torch.zeros(1, 3, h, h))
    model.fast_path = fp
    for hk in hooks:
        hk.remove()
    total += 2.0 * model.fc.weight.numel()
    return total
