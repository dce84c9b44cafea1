"""The rest of a CNO block on the GPU against tests/cno_ref.py in float64: rpde.ops.conv1d_k3 (three accumulating GEMMs
on shifted views, a dedicated weight / bias gradient kernel), rpde.ops.batchnorm1d (moments and affine-combine kernels,
torch's buffer semantics), the BatchNorm + activation fusion against the unfused composition of the project's own ops,
and the whole small model against the float64 restatement.

Bounds: forward rel-L2 <= 1e-5, gradients <= 2e-5 (README.md).  conv shapes (C_in, C_out, n, B): one input channel
(K = 1 in the forward GEMMs), one output channel with an odd, misaligned length, 24 -> 40 channels (no multiple of the
GEMM's tiles; ten 4 x 4 gradient tiles by six), and n = 1 where only the centre tap is live.  BatchNorm shapes: odd
sizes, a multiple of 4 (the 16-byte path), and two values per channel, where the backward's three terms cancel to
eps / (var + eps) of their size (what the affine kernel's double coefficients are for).

Measured on an MI355X, worst over each test's cases: conv1d_k3 y 8.4e-8, dx 1.2e-7, dw 9.8e-8, db 2.7e-7; batchnorm1d
y 2.6e-8, dz 3.2e-8, dgamma 3.8e-8, dbeta 3.4e-8, running statistics 7.2e-8; BatchNorm + activation against float64
y 8.5e-8, gradients 1.3e-7, against the unfused composition y 6.3e-8 and gradients bit for bit; the small model y 7.7e-7,
dx 5.4e-7, parameter gradients 4.5e-6 (decoder.1.batch_norm.weight, eval mode).
"""
import pytest
import torch

from tests import cno_ref

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 2e-5


def _rel(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm())


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("Cin,Cout,n,B", [(1, 8, 5, 2), (8, 1, 33, 3), (24, 40, 64, 2), (16, 16, 1, 2)])
def test_conv1d_k3(gpu_device, Cin, Cout, n, B):
    from rpde import ops
    x, w, b, g = _randn(B, Cin, n, seed=1), _randn(Cout, Cin, 3, seed=2) / (3 * Cin) ** 0.5, _randn(Cout, seed=3), _randn(B, Cout, n, seed=4)
    ref_in = [t.double().requires_grad_(True) for t in (x, w, b)]
    ref = cno_ref.conv(*ref_in)
    ref.backward(g.double())
    got_in = [t.to(gpu_device).requires_grad_(True) for t in (x, w, b)]
    out = ops.conv1d_k3(*got_in)
    out.backward(g.to(gpu_device))
    errs = {"y": _rel(out, ref), "dx": _rel(got_in[0].grad, ref_in[0].grad), "dw": _rel(got_in[1].grad, ref_in[1].grad),
            "db": _rel(got_in[2].grad, ref_in[2].grad)}
    print(f"conv1d_k3 Cin={Cin} Cout={Cout} n={n} B={B}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y"] <= FWD_TOL and max(errs["dx"], errs["dw"], errs["db"]) <= GRAD_TOL
    # no bias; the same inputs give the same bits
    nb = ops.conv1d_k3(got_in[0].detach(), got_in[1].detach())
    assert _rel(nb, cno_ref.conv(x, w)) <= FWD_TOL
    w2 = got_in[1].detach().clone().requires_grad_(True)
    ops.conv1d_k3(got_in[0].detach(), w2, got_in[2].detach()).backward(g.to(gpu_device))
    assert torch.equal(w2.grad, got_in[1].grad)
    with pytest.raises(ValueError):
        ops.conv1d_k3(got_in[0].detach(), torch.zeros(Cout, Cin + 1, 3, device=gpu_device))


def _bn_state(C, seed):
    w, b = 1.0 + 0.2 * _randn(C, seed=seed), 0.3 * _randn(C, seed=seed + 1)
    rm, rv = 0.2 * _randn(C, seed=seed + 2), 0.5 + _randn(C, seed=seed + 3).abs()
    return w, b, rm, rv


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,C,n", [(3, 5, 33), (4, 16, 64), (2, 7, 1)])
def test_batchnorm1d(gpu_device, B, C, n, training):
    from rpde import ops
    z, g = 1.5 * _randn(B, C, n, seed=5) + 0.7, _randn(B, C, n, seed=6)
    res = _randn(B, C, n, seed=7)
    w, b, rm, rv = _bn_state(C, 10)
    ref_in = [t.double().requires_grad_(True) for t in (z, w, b, res)]
    ref, rm_ref, rv_ref = cno_ref.batchnorm(ref_in[0], ref_in[1], ref_in[2], rm, rv, training)
    (ref + ref_in[3]).backward(g.double())
    got_in = [t.to(gpu_device).requires_grad_(True) for t in (z, w, b, res)]
    rm_d, rv_d, nbt = rm.to(gpu_device), rv.to(gpu_device), torch.tensor(3, device=gpu_device)
    out = ops.batchnorm1d(got_in[0], got_in[1], got_in[2], rm_d, rv_d, nbt, training, residual=got_in[3])
    out.backward(g.to(gpu_device))
    errs = {"y": _rel(out, ref + ref_in[3]), "dz": _rel(got_in[0].grad, ref_in[0].grad), "dgamma": _rel(got_in[1].grad, ref_in[1].grad),
            "dbeta": _rel(got_in[2].grad, ref_in[2].grad), "mean": _rel(rm_d, rm_ref), "var": _rel(rv_d, rv_ref)}
    print(f"batchnorm1d B={B} C={C} n={n} training={training}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs["y"], errs["mean"], errs["var"]) <= FWD_TOL and max(errs["dz"], errs["dgamma"], errs["dbeta"]) <= GRAD_TOL
    assert torch.equal(got_in[3].grad, g.to(gpu_device))
    assert int(nbt) == (4 if training else 3)
    if not training:
        assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv)


def test_batchnorm1d_refuses_one_value_per_channel(gpu_device):
    from rpde import ops
    w, b, rm, rv = (t.to(gpu_device) for t in _bn_state(4, 20))
    z = torch.zeros(1, 4, 1, device=gpu_device)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.batchnorm1d(z, w, b, rm, rv, None, True)
    assert ops.batchnorm1d(z, w, b, rm, rv, None, False).shape == z.shape      # eval mode takes it
    with pytest.raises(ValueError):
        ops.batchnorm1d(z, w, b, rm, rv, None, False, residual=z, act=(1, 1))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n,in_size,out_size", [(32, 32, 16), (24, 16, 16), (2, 2, 1)])
def test_batchnorm_fused_into_the_activation(gpu_device, n, in_size, out_size, training):
    """act=(in_size, out_size): the BatchNorm's apply step rides in the activation kernel's prologue.  Against the
    unfused composition batchnorm1d -> cno_act1d of the project's own ops (a few ulp: the affine is one fma either way,
    but the unfused path rounds the normalised tensor to fp32 in memory -- the same fp32 value the prologue forms), and
    against float64."""
    from rpde import ops
    B, C = 4, 6
    z, g = 1.3 * _randn(B, C, n, seed=8) - 0.4, _randn(B, C, out_size, seed=9)
    w, b, rm, rv = _bn_state(C, 30)

    def run(fused):
        leaves = [t.to(gpu_device).requires_grad_(True) for t in (z, w, b)]
        bufs = (rm.to(gpu_device), rv.to(gpu_device), torch.tensor(0, device=gpu_device))
        if fused:
            out = ops.batchnorm1d(*leaves, *bufs, training, act=(in_size, out_size))
        else:
            out = ops.cno_act1d(ops.batchnorm1d(*leaves, *bufs, training), in_size, out_size)
        out.backward(g.to(gpu_device))
        return [out] + [t.grad for t in leaves] + list(bufs[:2])

    fused, plain = run(True), run(False)
    ref_in = [t.double().requires_grad_(True) for t in (z, w, b)]
    y64 = cno_ref.act(cno_ref.batchnorm(*ref_in, rm, rv, training)[0], in_size, out_size)
    y64.backward(g.double())
    ref = [y64] + [t.grad for t in ref_in]
    names = ("y", "dz", "dgamma", "dbeta")
    e_plain = {k: _rel(a, c) for k, a, c in zip(names, fused, plain)}
    e_ref = {k: _rel(a, c) for k, a, c in zip(names, fused, ref)}
    print(f"bn+act n={n} {in_size}->{out_size} training={training}: vs unfused " + ", ".join(f"{k} {v:.2e}" for k, v in e_plain.items())
          + "; vs float64 " + ", ".join(f"{k} {v:.2e}" for k, v in e_ref.items()))
    assert e_ref["y"] <= FWD_TOL and max(e_ref[k] for k in names[1:]) <= GRAD_TOL
    assert e_plain["y"] <= FWD_TOL and max(e_plain[k] for k in names[1:]) <= GRAD_TOL
    assert torch.equal(fused[4], plain[4]) and torch.equal(fused[5], plain[5])          # the buffers do not care


@pytest.mark.parametrize("use_bn,training", [(True, True), (True, False), (False, True)], ids=["bn-train", "bn-eval", "nobn"])
def test_small_model_against_float64(gpu_device, use_bn, training):
    """models.CNO1d, small configuration, forward and every gradient against the float64 restatement of the model"""
    from models.CNO1d import CNO1d
    from tests.golden import synth
    from tests.golden.cno_cases import SMALL, state_for
    model = CNO1d(**SMALL, use_bn=use_bn)
    sd = state_for(synth.spec_of(model.state_dict()), 31)
    model.load_state_dict(sd, strict=True)
    model = model.to(gpu_device).train(training)
    x, g = synth.smooth_field((4, 1, 32), 32, "x"), synth.rand_tensor((4, 1, 32), 32, "g")
    xd = x.to(gpu_device).requires_grad_(True)
    y = model(xd)
    y.backward(g.to(gpu_device))

    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    y64, new = cno_ref.cno1d_forward(sd64, x64, 32, 2, 1, 1, use_bn, training)
    y64.backward(g.double())
    e_y, e_dx = _rel(y, y64), _rel(xd.grad, x64.grad)
    gmax = max(float(sd64[k].grad.norm()) for k, _ in model.named_parameters())
    worst, where = 0.0, None
    for k, p in model.named_parameters():
        r = sd64[k].grad
        if float(r.norm()) < 1e-5 * gmax:                   # a bias in front of a training-mode BatchNorm: exactly zero
            assert float(p.grad.norm()) < 1e-4 * gmax, k
            continue
        e = _rel(p.grad, r)
        worst, where = (e, k) if e > worst else (worst, where)
    e_buf = max([_rel(dict(model.named_buffers())[k], v) for k, v in new.items() if "running" in k] or [0.0])
    print(f"CNO1d small use_bn={use_bn} training={training}: y {e_y:.2e}, dx {e_dx:.2e}, worst grad {worst:.2e} ({where}), buffers {e_buf:.2e}")
    assert e_y <= FWD_TOL and e_dx <= GRAD_TOL and worst <= GRAD_TOL and e_buf <= FWD_TOL
    for k, v in new.items():
        if k.endswith("num_batches_tracked"):
            assert int(dict(model.named_buffers())[k]) == int(v)


@pytest.mark.parametrize("B,Cin,Cout,n", [(2, 3, 5, 7), (2, 8, 8, 64)])
def test_conv1d_k3_is_conv2d_k3_on_one_row(gpu_device, B, Cin, Cout, n):
    """Conv1d(k = 3) runs the 2-D tap loop on a plane of one row: against conv2d_k3 on x[:, :, None] with the weight in
    the middle tap row, y and dx are the same GEMMs in the same order, bit for bit.  dw and db come from the 2-D weight
    gradient, which may split the points into slices that the 1-D one adds in one go: GRAD_TOL, not bits."""
    from rpde import ops
    x, w, b, g = _randn(B, Cin, n, seed=11), _randn(Cout, Cin, 3, seed=12) / (3 * Cin) ** 0.5, _randn(Cout, seed=13), _randn(B, Cout, n, seed=14)
    w2 = torch.zeros(Cout, Cin, 3, 3)
    w2[:, :, 1] = w
    one = [t.to(gpu_device).requires_grad_(True) for t in (x, w, b)]
    two = [t.to(gpu_device).requires_grad_(True) for t in (x[:, :, None], w2, b)]
    y1 = ops.conv1d_k3(*one)
    y1.backward(g.to(gpu_device))
    y2 = ops.conv2d_k3(*two)
    y2.backward(g[:, :, None].to(gpu_device))
    e_dw, e_db = _rel(one[1].grad, two[1].grad[:, :, 1]), _rel(one[2].grad, two[2].grad)
    print(f"conv1d_k3 vs conv2d_k3 at H = 1, B={B} Cin={Cin} Cout={Cout} n={n}: y equal {torch.equal(y1, y2[:, :, 0])}, "
          f"dx equal {torch.equal(one[0].grad, two[0].grad[:, :, 0])}, dw {e_dw:.2e}, db {e_db:.2e}")
    assert torch.equal(y1, y2[:, :, 0]) and torch.equal(one[0].grad, two[0].grad[:, :, 0])
    assert e_dw <= GRAD_TOL and e_db <= GRAD_TOL
