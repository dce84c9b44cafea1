"""Float64 restatement of the U-Net pieces (rpde/unet.py over csrc/unet.hip) on the CPU, in torch functional calls:
what tests/test_gpu_unet_layers.py and tests/test_gpu_unet_edges.py compare the kernels with, and the restated launch
arithmetic (patches, slices) by which tests/test_unet_edges_ref_cpu.py places the latter's shapes.  Own code."""
from __future__ import annotations

import copy
import functools

import torch
import torch.nn.functional as F

from tests.golden import synth


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / (ref.norm() + 1e-300))


def max_pool(a: torch.Tensor) -> torch.Tensor:
    """MaxPool(kernel_size=2, stride=2) of a's rank, torch's default floor mode"""
    return F.max_pool1d(a, 2, 2) if a.dim() == 3 else F.max_pool2d(a, 2, 2)


def tanh_pool(z: torch.Tensor, scale=None, shift=None):
    """(act, pooled) of tanh(scale z + shift), per-channel scale / shift"""
    shape = (1, -1) + (1,) * (z.dim() - 2)
    y = z if scale is None else z * scale.view(shape) + shift.view(shape)
    act = torch.tanh(y)
    return act, max_pool(act)


def upconv(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """ConvTranspose(kernel_size=2, stride=2) of x's rank"""
    return F.conv_transpose1d(x, w, b, stride=2) if x.dim() == 3 else F.conv_transpose2d(x, w, b, stride=2)


def batchnorm_tanh(z, weight, bias, running_mean, running_var, training: bool, momentum: float = 0.1, eps: float = 1e-5):
    """tanh(BatchNorm(z)); updates the running buffers in place in training mode, as F.batch_norm does"""
    return torch.tanh(F.batch_norm(z, running_mean, running_var, weight, bias, training, momentum, eps))


def groupnorm_tanh(z, num_groups: int, weight, bias, eps: float = 1e-5):
    return torch.tanh(F.group_norm(z, num_groups, weight, bias, eps))


def loss_of(act, pooled, g_act, g_pool):
    """the scalar whose gradient feeds (g_act, g_pool) into the two outputs; either may be None: that output is unused"""
    total = 0.0
    if g_act is not None:
        total = total + (act * g_act).sum()
    if g_pool is not None:
        total = total + (pooled * g_pool).sum()
    return total


# ---- operands on which the kernels' arithmetic is exact ----------------------------------------------------------------
def int_tensor(shape, seed: int, name: str) -> torch.Tensor:
    """integers in [-3, 3] as float32, quantised from synth's seeded normal draw"""
    return (1.6 * synth.rand_tensor(shape, seed, name)).round().clamp(-3.0, 3.0)


def pool_shape(shape):
    return tuple(shape[:2]) + tuple(s // 2 for s in shape[2:])


def _spread(p: torch.Tensor, shape) -> torch.Tensor:
    """a per-window tensor repeated over its window's elements; a trailing odd row / column repeats the last window's"""
    for d in range(2, len(shape)):
        p = p.repeat_interleave(2, dim=d)
        if p.shape[d] < shape[d]:
            p = torch.cat((p, p.narrow(d, p.shape[d] - 1, 1)), dim=d)
    return p


def argmax_operands(shape, seed: int):
    """(act, g_act, g_pool) for the tanh_pool backward: act in {0, +-0.25, +-0.5, +-0.75}, the gradients integers in
    [-3, 3], so that 1 - act^2 and (g_act + g_pool) (1 - act^2) are exact in fp32.  A third of the windows are left as
    drawn (mostly distinct values), a third are raised to a per-window level (several elements share the maximum), a third
    hold one value."""
    ps = pool_shape(shape)
    a = int_tensor(shape, seed, "act") / 4.0
    level = _spread(int_tensor(ps, seed, "level") / 4.0, shape)
    mode = _spread(synth.rand_tensor(ps, seed, "mode"), shape)
    act = torch.where(mode < -0.43, level, torch.where(mode > 0.43, torch.maximum(a, level), a))
    return act, int_tensor(shape, seed, "g_act"), int_tensor(ps, seed, "g_pool")


def windows(a: torch.Tensor) -> torch.Tensor:
    """[..., windows, elements in scan order] of MaxPool(2)'s whole windows"""
    if a.dim() == 3:
        B, C, n = a.shape
        return a[..., :n // 2 * 2].reshape(B, C, n // 2, 2)
    B, C, H, W = a.shape
    w = a[..., :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)
    return w.permute(0, 1, 2, 4, 3, 5).reshape(B, C, -1, 4)


def window_patterns(act: torch.Tensor) -> dict:
    """how many windows have one maximum that is not their first element, a maximum shared by some elements with the
    first of them not the window's first, and one value throughout"""
    w = windows(act)
    at_max = w == w.max(-1, keepdim=True).values
    count, first = at_max.sum(-1), at_max.float().argmax(-1)
    k = w.shape[-1]
    return dict(distinct_late=int(((count == 1) & (first > 0)).sum()), partial=int(((count > 1) & (count < k)).sum()),
                partial_late=int(((count > 1) & (count < k) & (first > 0)).sum()), full=int((count == k).sum()))


def tanh_pool_bwd(act: torch.Tensor, g_act, g_pool) -> torch.Tensor:
    """float64 gy = (g_act + scatter(g_pool)) (1 - act^2), the scatter being torch's CPU max_pool backward on act"""
    a = act.detach().double().requires_grad_(True)
    g = torch.zeros_like(a) if g_act is None else g_act.double().clone()
    if g_pool is not None:
        (max_pool(a) * g_pool.double()).sum().backward()
        g = g + a.grad
    return g * (1.0 - a.detach() * a.detach())


# ---- the launch arithmetic of csrc/unet.hip and csrc/wgrad_sliced.h, restated ------------------------------------------
def tp_items(shape, vec: bool = None):
    """(items, vec) of k_unet_tanh_pool_*: a thread owns ky rows x cw columns, cw = 4 on the 16-byte path (W % 4 == 0
    and aligned pointers: `vec`, by default what a fresh allocation gets) and 2 otherwise; 256 items make a workgroup"""
    B, C = shape[:2]
    H, W, ky = (1, shape[2], 1) if len(shape) == 3 else (shape[2], shape[3], 2)
    vec = W % 4 == 0 if vec is None else vec
    cw = 4 if vec else 2
    return B * C * ((H + ky - 1) // ky) * ((W + cw - 1) // cw), vec


def upconv_slices(B: int, Cin: int, Cout: int, H: int, W: int):
    """(slices, points per slice) of upconv's weight gradient: 4 x 4 channel tiles, 512 workgroups wanted, 256 points
    at least"""
    tiles = ((Cin + 3) // 4) * ((Cout + 3) // 4)
    slices = max(1, min(512 // tiles, B * H * W // 256, 65535))
    return slices, (B * H * W + slices - 1) // slices


def conv_slices(B: int, Cin: int, Cout: int, H: int, W: int):
    """(slices, image rows per slice) of Conv2d(k = 3)'s weight gradient: the same, in whole image rows (b, y)"""
    tiles = ((Cin + 3) // 4) * ((Cout + 3) // 4)
    slices = max(1, min(512 // tiles, B * H, B * H * W // 256, 65535))
    return slices, (B * H + slices - 1) // slices


# ---- whole models -----------------------------------------------------------------------------------------------------
def stock_forward(module, x: torch.Tensor) -> torch.Tensor:
    """the U-Net data flow over the module's own nn.Sequential blocks, poolN, upconvN and conv, which run stock torch
    layers on whatever device and dtype the module lives in; models.unet's forward computes the same with rpde.ops"""
    skips = []
    for i in range(1, 5):
        skips.append(getattr(module, f"encoder{i}")(x))
        x = getattr(module, f"pool{i}")(skips[-1])
    x = module.bottleneck(x)
    for i in range(4, 0, -1):
        x = torch.cat((getattr(module, f"upconv{i}")(x), skips[i - 1]), dim=1)
        x = getattr(module, f"decoder{i}")(x)
    return module.conv(x)


def model_step(forward, module, x: torch.Tensor, g: torch.Tensor) -> dict:
    """one training-mode forward and backward of the loss (y g).sum(): y, dx, grad/<parameter>, buf/<buffer> after it"""
    module.train()
    x = x.clone().requires_grad_(True)
    y = forward(module, x)
    (y * g).sum().backward()
    res = {"y": y.detach(), "dx": x.grad}
    res.update({"grad/" + n: p.grad for n, p in module.named_parameters()})
    res.update({"buf/" + n: b.detach().clone() for n, b in module.named_buffers()})
    return res


def model_errors(got: dict, ref: dict) -> dict:
    """rel-L2 per tensor; a gradient's denominator is max(|ref|, 1e-6 max |ref| over the gradients)"""
    assert set(got) == set(ref)
    grads = [k for k in ref if k == "dx" or k.startswith("grad/")]
    gmax = max(float(ref[k].double().norm()) for k in grads)
    errs = {}
    for k, r in ref.items():
        r = r.detach().double().cpu()
        den = max(float(r.norm()), 1e-6 * gmax) if k in grads else float(r.norm()) + 1e-300
        errs[k] = float((got[k].detach().double().cpu() - r).norm()) / den
    return errs


@functools.lru_cache(maxsize=None)
def model_reference(kind: str, ctor: tuple, x_shape: tuple, seed: int):
    """(module, x, g, ref, floors): a models.unet module of default initialisation under torch.manual_seed(seed) (float32,
    CPU, not yet stepped), synth inputs, the float64 stock_forward step on a copy of it, and per tensor the `floor`: the
    float32 CPU stock_forward step's own distance from the float64 one.  Computed once; callers copy the module."""
    from models import unet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        module = getattr(unet, kind)(**dict(ctor))
    x = synth.smooth_field(x_shape, seed, "x")
    g = synth.rand_tensor((x_shape[0], dict(ctor)["out_channels"]) + tuple(x_shape[2:]), seed, "upstream")
    ref = model_step(stock_forward, copy.deepcopy(module).double(), x.double(), g.double())
    floors = model_errors(model_step(stock_forward, copy.deepcopy(module), x, g), ref)
    return module, x, g, ref, floors
