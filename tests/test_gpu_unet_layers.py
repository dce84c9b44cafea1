"""The U-Net kernels (csrc/unet.hip through rpde.ops tanh_pool, norm_tanh, groupnorm_tanh, upconv1d / upconv2d) on the
GPU against the float64 restatement of tests/unet_ref.py: forward rel-L2 1e-5, gradients 2e-5 (the project's budgets).

tanh_pool runs every shape with and without scale / shift and with the loss on the pooled output only, on the
activation only and on both, which passes a null gradient for the unused output; ties inside windows must scatter as
torch's CPU max_pool backward does, element for element (inputs on which 1 - act^2 is exactly 0 or 1, so that the
comparison is exact); a NaN in a window reaches the pooled output.  upconv checks y, dx, dw, db with and without bias and
a second run bit for bit.

Measured on an MI355X, worst rel-L2 over the cases: tanh_pool act 4.4e-8, pooled 4.4e-8, gy 8.0e-8; upconv y 9.2e-8, dx 2.3e-7,
dw 8.0e-8, db 3.2e-7, the second run bit-equal; norm_tanh (BatchNorm) act 4.4e-8, pooled 4.4e-8, dz 7.9e-8, dgamma 2.4e-7,
dbeta 1.5e-7, running mean 6.3e-8, running variance 5.0e-8; groupnorm_tanh act 3.9e-8, dz 6.2e-8, dgamma 1.7e-7, dbeta
1.2e-7; fused against unfused act 3.5e-8, dz 7.1e-8, dgamma 1.1e-7, the statistics bit-equal; the tie and NaN cases exact.
"""
import pytest
import torch

from tests import unet_ref as R
from tests.golden import synth

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 2e-5

TP_1D = [(1, 1, 2), (3, 5, 33), (2, 4, 64)]
TP_2D = [(1, 2, 2, 2), (2, 3, 5, 7), (2, 4, 8, 16), (2, 1, 33, 4)]


def _pool_shape(shape):
    return tuple(shape[:2]) + tuple(s // 2 for s in shape[2:])


@pytest.mark.parametrize("use", ["pool", "act", "both"])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", TP_1D + TP_2D)
def test_tanh_pool(gpu_device, shape, affine, use):
    from rpde import ops
    seed = 100 + len(shape)
    z = synth.rand_tensor(shape, seed, "z")
    scale = 1.0 + 0.3 * synth.rand_tensor((shape[1],), seed, "scale") if affine else None
    shift = 0.2 * synth.rand_tensor((shape[1],), seed, "shift") if affine else None
    g_act = synth.rand_tensor(shape, seed, "g_act") if use != "pool" else None
    g_pool = synth.rand_tensor(_pool_shape(shape), seed, "g_pool") if use != "act" else None

    z64 = z.double().requires_grad_(True)
    act64, pool64 = R.tanh_pool(z64, None if scale is None else scale.double(), None if shift is None else shift.double())
    R.loss_of(act64, pool64, None if g_act is None else g_act.double(), None if g_pool is None else g_pool.double()).backward()
    # the op returns the gradient with respect to scale z + shift: the caller owns the affine's chain rule
    gy64 = z64.grad if scale is None else z64.grad / scale.double().view((1, -1) + (1,) * (len(shape) - 2))

    dev = gpu_device
    zg = z.to(dev).requires_grad_(True)
    act, pooled = ops.tanh_pool(zg, None if scale is None else scale.to(dev), None if shift is None else shift.to(dev), pool=True)
    R.loss_of(act, pooled, None if g_act is None else g_act.to(dev), None if g_pool is None else g_pool.to(dev)).backward()
    errs = dict(act=R.rel_l2(act, act64), pooled=R.rel_l2(pooled, pool64), gy=R.rel_l2(zg.grad, gy64))
    print(f"tanh_pool {shape} affine={affine} use={use}: {errs}")
    assert tuple(pooled.shape) == _pool_shape(shape)
    assert errs["act"] <= FWD and errs["pooled"] <= FWD and errs["gy"] <= GRAD
    alone = ops.tanh_pool(z.to(dev), None if scale is None else scale.to(dev), None if shift is None else shift.to(dev))
    assert torch.equal(alone, act)                     # without the pool: the same activation, one output


def test_tanh_pool_refuses_an_empty_pooled_tensor(gpu_device):
    from rpde import ops
    with pytest.raises(ValueError, match="nothing left to pool"):
        ops.tanh_pool(torch.zeros(2, 3, 1, device=gpu_device), pool=True)
    with pytest.raises(ValueError, match="nothing left to pool"):
        ops.tanh_pool(torch.zeros(2, 3, 1, 8, device=gpu_device), pool=True)
    assert tuple(ops.tanh_pool(torch.zeros(2, 3, 1, device=gpu_device)).shape) == (2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 3, 64), (2, 3, 31), (2, 2, 16, 32), (1, 2, 9, 14)])
def test_ties_scatter_as_torch_does(gpu_device, shape):
    """z in {0, -20}: act in {0, -1} exactly, every pattern of equal and unequal values occurs inside the windows, and
    1 - act^2 is exactly 1 or 0, so gy must equal torch's CPU result bit for bit"""
    from rpde import ops
    z = torch.where(synth.rand_tensor(shape, 7, "ties") > 0.0, 0.0, -20.0)
    g_act, g_pool = synth.rand_tensor(shape, 7, "g_act"), synth.rand_tensor(_pool_shape(shape), 7, "g_pool")
    zg = z.to(gpu_device).requires_grad_(True)
    act, pooled = ops.tanh_pool(zg, pool=True)
    assert set(act.unique().tolist()) == {-1.0, 0.0}
    R.loss_of(act, pooled, g_act.to(gpu_device), g_pool.to(gpu_device)).backward()
    a = act.detach().cpu().requires_grad_(True)
    (R.max_pool(a) * g_pool).sum().backward()
    want = (g_act + a.grad) * (1.0 - a.detach() * a.detach())
    assert torch.equal(pooled.cpu(), R.max_pool(a.detach()))
    assert torch.equal(zg.grad.cpu(), want)
    only_pool = z.to(gpu_device).requires_grad_(True)
    (ops.tanh_pool(only_pool, pool=True)[1] * g_pool.to(gpu_device)).sum().backward()
    assert torch.equal(only_pool.grad.cpu(), a.grad * (1.0 - a.detach() * a.detach()))


@pytest.mark.parametrize("shape,at", [((1, 2, 8), (0, 1, 3)), ((1, 2, 7), (0, 0, 4)), ((1, 1, 4, 8), (0, 0, 3, 5)), ((1, 1, 4, 6), (0, 0, 0, 2))])
def test_nan_reaches_the_pooled_output(gpu_device, shape, at):
    from rpde import ops
    z = synth.rand_tensor(shape, 9, "z")
    z[at] = float("nan")
    act, pooled = ops.tanh_pool(z.to(gpu_device), pool=True)
    want = R.max_pool(torch.tanh(z))
    assert torch.isnan(pooled.cpu()).equal(torch.isnan(want)) and int(torch.isnan(want).sum()) == 1
    assert torch.isnan(act.cpu()).equal(torch.isnan(z))


UP_1D = [(1, 8, 5, 2), (8, 1, 33, 3), (24, 40, 16, 2), (16, 16, 1, 2)]               # (Cin, Cout, n, B)
UP_2D = [(1, 4, 3, 5, 2), (8, 1, 7, 33, 2), (24, 40, 8, 8, 2), (16, 8, 1, 1, 3)]     # (Cin, Cout, H, W, B)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", UP_1D + UP_2D)
def test_upconv(gpu_device, case, with_bias):
    from rpde import ops
    Cin, Cout, *sizes, B = case
    op = ops.upconv1d if len(sizes) == 1 else ops.upconv2d
    seed = 200 + Cin
    x = synth.rand_tensor((B, Cin, *sizes), seed, "x")
    w = synth.rand_tensor((Cin, Cout) + (2,) * len(sizes), seed, "w", scale=Cin ** -0.5)
    b = 0.1 * synth.rand_tensor((Cout,), seed, "b") if with_bias else None
    up = synth.rand_tensor((B, Cout, *[2 * s for s in sizes]), seed, "upstream")

    leaves64 = [t.double().requires_grad_(True) for t in (x, w)] + ([b.double().requires_grad_(True)] if with_bias else [])
    y64 = R.upconv(*leaves64)
    (y64 * up.double()).sum().backward()

    def run():
        leaves = [t.to(gpu_device).requires_grad_(True) for t in (x, w)] + ([b.to(gpu_device).requires_grad_(True)] if with_bias else [])
        y = op(*leaves)
        (y * up.to(gpu_device)).sum().backward()
        return [y.detach()] + [t.grad for t in leaves]

    got, again = run(), run()
    names = ["y", "dx", "dw"] + (["db"] if with_bias else [])
    errs = {n: R.rel_l2(g, r) for n, g, r in zip(names, got, [y64] + [t.grad for t in leaves64])}
    print(f"upconv {case} bias={with_bias}: {errs}")
    assert tuple(got[0].shape) == tuple(y64.shape)
    assert errs["y"] <= FWD and all(errs[n] <= GRAD for n in names[1:])
    assert all(torch.equal(a, b2) for a, b2 in zip(got, again))                  # fixed order: the same bits again


def test_upconv1d_is_upconv2d_on_a_one_row_plane(gpu_device):
    from rpde import ops
    x = synth.rand_tensor((2, 24, 19), 31, "x").to(gpu_device)
    w2 = synth.rand_tensor((24, 40, 2, 2), 31, "w").to(gpu_device)
    b = synth.rand_tensor((40,), 31, "b").to(gpu_device)
    y1 = ops.upconv1d(x, w2[:, :, 0].contiguous(), b)
    y2 = ops.upconv2d(x.unsqueeze(2), w2, b)
    assert tuple(y2.shape) == (2, 40, 2, 38) and torch.equal(y1, y2[:, :, 0])


def _bn(rank, C, seed, device=None, dtype=torch.float32):
    bn = (torch.nn.BatchNorm1d if rank == 1 else torch.nn.BatchNorm2d)(C)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * synth.rand_tensor((C,), seed, "gamma"))
        bn.bias.copy_(0.1 * synth.rand_tensor((C,), seed, "beta"))
        bn.running_mean.copy_(0.2 * synth.rand_tensor((C,), seed, "rm"))
        bn.running_var.copy_(0.5 + synth.rand_tensor((C,), seed, "rv").abs())
    bn = bn.to(dtype)
    return bn if device is None else bn.to(device)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 33), (4, 8, 64), (2, 3, 6, 10), (2, 4, 8, 16)])
def test_norm_tanh_batchnorm(gpu_device, shape, training):
    from rpde import ops
    rank, C, seed = len(shape) - 2, shape[1], 300 + len(shape)
    z = 0.5 + 1.5 * synth.rand_tensor(shape, seed, "z")
    g_act, g_pool = synth.rand_tensor(shape, seed, "g_act"), synth.rand_tensor(_pool_shape(shape), seed, "g_pool")

    bn64 = _bn(rank, C, seed, dtype=torch.float64).train(training)
    z64 = z.double().requires_grad_(True)
    act64 = R.batchnorm_tanh(z64, bn64.weight, bn64.bias, bn64.running_mean, bn64.running_var, training, bn64.momentum, bn64.eps)
    R.loss_of(act64, R.max_pool(act64), g_act.double(), g_pool.double()).backward()

    bn = _bn(rank, C, seed, gpu_device).train(training)
    zg = z.to(gpu_device).requires_grad_(True)
    act, pooled = ops.norm_tanh(zg, bn, pool=True)
    R.loss_of(act, pooled, g_act.to(gpu_device), g_pool.to(gpu_device)).backward()
    errs = dict(act=R.rel_l2(act, act64), pooled=R.rel_l2(pooled, R.max_pool(act64)), dz=R.rel_l2(zg.grad, z64.grad),
                dgamma=R.rel_l2(bn.weight.grad, bn64.weight.grad), dbeta=R.rel_l2(bn.bias.grad, bn64.bias.grad),
                mean=R.rel_l2(bn.running_mean, bn64.running_mean), var=R.rel_l2(bn.running_var, bn64.running_var))
    print(f"norm_tanh {shape} training={training}: {errs}")
    assert errs["act"] <= FWD and errs["pooled"] <= FWD and errs["mean"] <= FWD and errs["var"] <= FWD
    assert errs["dz"] <= GRAD and errs["dgamma"] <= GRAD and errs["dbeta"] <= GRAD
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    if not training:
        assert errs["mean"] == 0.0 and errs["var"] == 0.0            # eval mode leaves the buffers alone


def test_norm_tanh_refuses_one_value_per_channel(gpu_device):
    from rpde import ops
    bn = torch.nn.BatchNorm1d(3).to(gpu_device).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.norm_tanh(torch.zeros(1, 3, 1, device=gpu_device), bn)


@pytest.mark.parametrize("shape,groups", [((3, 8, 33), 4), ((2, 6, 16), 6), ((2, 8, 4, 6), 2)])
def test_groupnorm_tanh(gpu_device, shape, groups):
    from rpde import ops
    C, seed = shape[1], 400 + groups
    z = 0.5 + 1.5 * synth.rand_tensor(shape, seed, "z")
    gamma, beta = 1.0 + 0.2 * synth.rand_tensor((C,), seed, "gamma"), 0.1 * synth.rand_tensor((C,), seed, "beta")
    g_act, g_pool = synth.rand_tensor(shape, seed, "g_act"), synth.rand_tensor(_pool_shape(shape), seed, "g_pool")
    leaves64 = [t.double().requires_grad_(True) for t in (z, gamma, beta)]
    act64 = R.groupnorm_tanh(leaves64[0], groups, leaves64[1], leaves64[2])
    R.loss_of(act64, R.max_pool(act64), g_act.double(), g_pool.double()).backward()
    leaves = [t.to(gpu_device).requires_grad_(True) for t in (z, gamma, beta)]
    act, pooled = ops.groupnorm_tanh(leaves[0], groups, leaves[1], leaves[2], 1e-5, pool=True)
    R.loss_of(act, pooled, g_act.to(gpu_device), g_pool.to(gpu_device)).backward()
    errs = dict(act=R.rel_l2(act, act64), pooled=R.rel_l2(pooled, R.max_pool(act64)),
                **{n: R.rel_l2(a.grad, b.grad) for n, a, b in zip(("dz", "dgamma", "dbeta"), leaves, leaves64)})
    print(f"groupnorm_tanh {shape} groups={groups}: {errs}")
    assert errs["act"] <= FWD and errs["pooled"] <= FWD
    assert errs["dz"] <= GRAD and errs["dgamma"] <= GRAD and errs["dbeta"] <= GRAD


@pytest.mark.parametrize("shape", [(3, 5, 33), (2, 4, 8, 16)])
def test_fused_norm_tanh_against_the_unfused_ops(gpu_device, shape):
    """norm_tanh against batchnorm -> tanh_pool of the project's own ops, which writes the normalised tensor: the two
    round differently (the fused pass applies an fp32 scale and shift), so they agree to the forward / gradient budgets"""
    from rpde import ops
    rank, C, seed = len(shape) - 2, shape[1], 500
    z = synth.rand_tensor(shape, seed, "z")
    g_act, g_pool = synth.rand_tensor(shape, seed, "g_act").to(gpu_device), synth.rand_tensor(_pool_shape(shape), seed, "g_pool").to(gpu_device)
    out = []
    for fused in (True, False):
        bn = _bn(rank, C, seed, gpu_device).train()
        zg = z.to(gpu_device).requires_grad_(True)
        if fused:
            act, pooled = ops.norm_tanh(zg, bn, pool=True)
        else:
            plain = (ops.batchnorm1d if rank == 1 else ops.batchnorm2d)(zg, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                                                          bn.num_batches_tracked, True, bn.momentum, bn.eps)
            act, pooled = ops.tanh_pool(plain, pool=True)
        R.loss_of(act, pooled, g_act, g_pool).backward()
        out.append((act.detach(), pooled.detach(), zg.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone()))
    errs = [R.rel_l2(a, b) for a, b in zip(*out)]
    print(f"fused against unfused {shape}: {errs}")
    assert errs[0] <= FWD and errs[1] <= FWD and all(e <= GRAD for e in errs[2:5])
    assert errs[5] == 0.0 and errs[6] == 0.0                         # the statistics come from the same kernel
