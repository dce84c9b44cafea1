"""The rest of a 2-D CNO block on the GPU against tests/cno2d_ref.py in float64: rpde.ops.conv2d_k3 (nine accumulating
GEMMs on shifted views -- flat for the dx = 0 taps, row by row through the two-level batch for the others -- and the
split weight / bias gradient kernel), rpde.ops.batchnorm2d (the rank-agnostic moments and affine-combine kernels,
torch's buffer semantics), its fusion with the 2-D activation, and rpde.ops.skip_add on 4-D.

Bounds: forward rel-L2 <= 1e-5, gradients <= 2e-5 (README.md).  conv planes (H, W): (1,1) where only the centre tap is
live, (1,7) and (6,1) where a whole direction of taps has no valid range, odd (5,7), (16,16), and (33,20) with more
rows than columns; channels (Cin, Cout): (1,64), (3,5), (8,8), (64,3), (18,7) -- no multiples of the 4 x 4 weight-gradient
tile, from 2 to 16 (co, ci) tiles; B = 1 and 3.  The weight gradient splits the B H image rows into
min(512 / tiles, B H, B H W / 256) slices: the planes up to (5,7) run unsplit (one slice), (16,16) runs unsplit at
B = 1 and in 3 slices at B = 3, (33,20) in 2 and 7 slices.  BatchNorm shapes: odd sizes, a multiple of 4 (the 16-byte
path), and two and four values per channel (B = 2 at 1 x 1, B = 1 at 2 x 2), where the backward's three terms cancel to
eps / (var + eps) of their size.

Measured on an MI355X, worst over each test's cases: conv2d_k3 y 1.6e-7, dx 2.0e-7, dw 1.0e-7, db 1.9e-7; batchnorm2d
y 2.6e-8, dz 3.2e-8, dgamma 4.4e-8, dbeta 2.8e-8, running statistics 7.2e-8; BatchNorm + activation against float64
y 1.1e-7, gradients 1.7e-7, against the unfused composition y 6.1e-8 and gradients bit for bit.
"""
import pytest
import torch

from tests import cno2d_ref

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 2e-5
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, (e, where) in sorted(_WORST.items()):
        print(f"\n[cno2d_layers] worst {k} {e:.3e} (at {where})")


def _note(errs, prefix, where):
    for k, e in errs.items():
        if e > _WORST.get(f"{prefix} {k}", (0.0, None))[0]:
            _WORST[f"{prefix} {k}"] = (e, where)


def _rel(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm())


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("Cin,Cout", [(1, 64), (3, 5), (8, 8), (64, 3), (18, 7)])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (6, 1), (5, 7), (16, 16), (33, 20)])
def test_conv2d_k3(gpu_device, H, W, Cin, Cout):
    from rpde import ops
    for B in (1, 3):
        x, w = _randn(B, Cin, H, W, seed=1), _randn(Cout, Cin, 3, 3, seed=2) / (9 * Cin) ** 0.5
        b, g = _randn(Cout, seed=3), _randn(B, Cout, H, W, seed=4)
        ref_in = [t.double().requires_grad_(True) for t in (x, w, b)]
        ref = cno2d_ref.conv(*ref_in)
        ref.backward(g.double())
        got_in = [t.to(gpu_device).requires_grad_(True) for t in (x, w, b)]
        out = ops.conv2d_k3(*got_in)
        out.backward(g.to(gpu_device))
        errs = {"y": _rel(out, ref), "dx": _rel(got_in[0].grad, ref_in[0].grad), "dw": _rel(got_in[1].grad, ref_in[1].grad),
                "db": _rel(got_in[2].grad, ref_in[2].grad)}
        print(f"conv2d_k3 Cin={Cin} Cout={Cout} H={H} W={W} B={B}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        _note(errs, "conv2d_k3", (Cin, Cout, H, W, B))
        assert errs["y"] <= FWD_TOL and max(errs["dx"], errs["dw"], errs["db"]) <= GRAD_TOL
        # no bias; the same inputs give the same bits
        nb = ops.conv2d_k3(got_in[0].detach(), got_in[1].detach())
        assert _rel(nb, cno2d_ref.conv(x, w)) <= FWD_TOL
        w2 = got_in[1].detach().clone().requires_grad_(True)
        b2 = got_in[2].detach().clone().requires_grad_(True)
        ops.conv2d_k3(got_in[0].detach(), w2, b2).backward(g.to(gpu_device))
        assert torch.equal(w2.grad, got_in[1].grad) and torch.equal(b2.grad, got_in[2].grad)
    with pytest.raises(ValueError):
        ops.conv2d_k3(got_in[0].detach(), torch.zeros(Cout, Cin + 1, 3, 3, device=gpu_device))
    with pytest.raises(ValueError):
        ops.conv2d_k3(got_in[0].detach()[0], got_in[1].detach())


def test_conv2d_weight_gradient_slices():
    """the slice counts the docstring states (rpde_conv_k3_bwd_weight_slices at ky = 3; no device needed)"""
    from rpde import _lib
    query = _lib.load().rpde_conv_k3_bwd_weight_slices

    def slices(*dims):
        return query(*dims, 3)

    assert [slices(B, 8, 8, 5, 7) for B in (1, 3)] == [1, 1]
    assert [slices(B, 8, 8, 16, 16) for B in (1, 3)] == [1, 3]
    assert [slices(B, 8, 8, 33, 20) for B in (1, 3)] == [2, 7]
    assert slices(16, 8, 8, 256, 256) == 128                   # level 0 of the shipped yaml: 4 tiles x 128 slices
    assert slices(16, 128, 128, 16, 16) == 1                   # its deepest level: 1024 tiles fill the device unsplit


def _bn_state(C, seed):
    w, b = 1.0 + 0.2 * _randn(C, seed=seed), 0.3 * _randn(C, seed=seed + 1)
    rm, rv = 0.2 * _randn(C, seed=seed + 2), 0.5 + _randn(C, seed=seed + 3).abs()
    return w, b, rm, rv


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,C,H,W", [(3, 5, 5, 7), (2, 16, 8, 8), (2, 7, 1, 1), (1, 7, 2, 2)])
def test_batchnorm2d(gpu_device, B, C, H, W, training):
    from rpde import ops
    z, g = 1.5 * _randn(B, C, H, W, seed=5) + 0.7, _randn(B, C, H, W, seed=6)
    res = _randn(B, C, H, W, seed=7)
    w, b, rm, rv = _bn_state(C, 10)
    ref_in = [t.double().requires_grad_(True) for t in (z, w, b, res)]
    ref, rm_ref, rv_ref = cno2d_ref.batchnorm(ref_in[0], ref_in[1], ref_in[2], rm, rv, training)
    (ref + ref_in[3]).backward(g.double())
    got_in = [t.to(gpu_device).requires_grad_(True) for t in (z, w, b, res)]
    rm_d, rv_d, nbt = rm.to(gpu_device), rv.to(gpu_device), torch.tensor(3, device=gpu_device)
    out = ops.batchnorm2d(got_in[0], got_in[1], got_in[2], rm_d, rv_d, nbt, training, residual=got_in[3])
    out.backward(g.to(gpu_device))
    errs = {"y": _rel(out, ref + ref_in[3]), "dz": _rel(got_in[0].grad, ref_in[0].grad), "dgamma": _rel(got_in[1].grad, ref_in[1].grad),
            "dbeta": _rel(got_in[2].grad, ref_in[2].grad), "mean": _rel(rm_d, rm_ref), "var": _rel(rv_d, rv_ref)}
    print(f"batchnorm2d B={B} C={C} H={H} W={W} training={training}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    _note(errs, "batchnorm2d", (B, C, H, W, training))
    assert max(errs["y"], errs["mean"], errs["var"]) <= FWD_TOL and max(errs["dz"], errs["dgamma"], errs["dbeta"]) <= GRAD_TOL
    assert torch.equal(got_in[3].grad, g.to(gpu_device))
    assert int(nbt) == (4 if training else 3)
    if not training:
        assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv)
    # without the residual
    plain = ops.batchnorm2d(got_in[0].detach(), got_in[1].detach(), got_in[2].detach(), rm.to(gpu_device), rv.to(gpu_device),
                            None, training)
    assert _rel(plain, ref) <= FWD_TOL


def test_batchnorm2d_refuses_one_value_per_channel(gpu_device):
    from rpde import ops
    w, b, rm, rv = (t.to(gpu_device) for t in _bn_state(4, 20))
    z = torch.zeros(1, 4, 1, 1, device=gpu_device)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.batchnorm2d(z, w, b, rm, rv, None, True)
    assert ops.batchnorm2d(z, w, b, rm, rv, None, False).shape == z.shape      # eval mode takes it
    with pytest.raises(ValueError):
        ops.batchnorm2d(z, w, b, rm, rv, None, False, residual=z, act=(1, 1))
    with pytest.raises(ValueError):
        ops.batchnorm2d(z[0], w, b, rm, rv, None, False)
    with pytest.raises(ValueError):
        ops.batchnorm1d(z, w, b, rm, rv, None, False)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("H,W,in_size,out_size", [(16, 16, 16, 8), (12, 10, 8, 8), (2, 2, 2, 1)])
def test_batchnorm_fused_into_the_activation(gpu_device, H, W, in_size, out_size, training):
    """act=(in_size, out_size): the BatchNorm's apply step rides in the 2-D activation kernel's prologue.  Against the
    unfused composition batchnorm2d -> cno_act2d of the project's own ops and against float64."""
    from rpde import ops
    B, C = 3, 5
    z, g = 1.3 * _randn(B, C, H, W, seed=8) - 0.4, _randn(B, C, out_size, out_size, seed=9)
    w, b, rm, rv = _bn_state(C, 30)

    def run(fused):
        leaves = [t.to(gpu_device).requires_grad_(True) for t in (z, w, b)]
        bufs = (rm.to(gpu_device), rv.to(gpu_device), torch.tensor(0, device=gpu_device))
        if fused:
            out = ops.batchnorm2d(*leaves, *bufs, training, act=(in_size, out_size))
        else:
            out = ops.cno_act2d(ops.batchnorm2d(*leaves, *bufs, training), in_size, out_size)
        out.backward(g.to(gpu_device))
        return [out] + [t.grad for t in leaves] + list(bufs[:2])

    fused, plain = run(True), run(False)
    ref_in = [t.double().requires_grad_(True) for t in (z, w, b)]
    y64 = cno2d_ref.act(cno2d_ref.batchnorm(*ref_in, rm, rv, training)[0], in_size, out_size)
    y64.backward(g.double())
    ref = [y64] + [t.grad for t in ref_in]
    names = ("y", "dz", "dgamma", "dbeta")
    e_plain = {k: _rel(a, c) for k, a, c in zip(names, fused, plain)}
    e_ref = {k: _rel(a, c) for k, a, c in zip(names, fused, ref)}
    print(f"bn+act2d {H}x{W} {in_size}->{out_size} training={training}: vs unfused " + ", ".join(f"{k} {v:.2e}" for k, v in e_plain.items())
          + "; vs float64 " + ", ".join(f"{k} {v:.2e}" for k, v in e_ref.items()))
    _note(e_ref, "bn+act2d", (H, W, in_size, out_size, training))
    assert e_ref["y"] <= FWD_TOL and max(e_ref[k] for k in names[1:]) <= GRAD_TOL
    assert e_plain["y"] <= FWD_TOL and max(e_plain[k] for k in names[1:]) <= GRAD_TOL
    assert torch.equal(fused[4], plain[4]) and torch.equal(fused[5], plain[5])          # the buffers do not care


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 4, 8, 8)])
def test_skip_add_4d(gpu_device, shape):
    from rpde import ops
    a, r, g = _randn(*shape, seed=11), _randn(*shape, seed=12), _randn(*shape, seed=13)
    ad, rd = a.to(gpu_device).requires_grad_(True), r.to(gpu_device).requires_grad_(True)
    out = ops.skip_add(ad, rd)
    out.backward(g.to(gpu_device))
    assert _rel(out, a.double() + r.double()) <= 1e-7           # one rounding of the exact sum
    assert torch.equal(ad.grad.cpu(), g) and torch.equal(rd.grad.cpu(), g)
    with pytest.raises(ValueError):
        ops.skip_add(ad[0, 0], rd[0, 0])


def test_conv2d_weight_gradient_refuses_a_short_partial_buffer(gpu_device):
    from rpde import _lib
    lib = _lib.load()
    B, Cin, Cout, H, W = 3, 8, 8, 16, 16                        # 3 slices
    x, g = torch.zeros(B, Cin, H, W, device=gpu_device), torch.zeros(B, Cout, H, W, device=gpu_device)
    gw, gb = torch.zeros(Cout, Cin, 3, 3, device=gpu_device), torch.zeros(Cout, device=gpu_device)
    part = torch.zeros(2, 9 * Cout * Cin + Cout, device=gpu_device)
    args = (_lib.ptr(x), _lib.ptr(g), _lib.ptr(gw), _lib.ptr(gb), B, Cin, Cout, H, W, 3)
    for buf, n in ((None, 0), (_lib.ptr(part), 2)):
        assert lib.rpde_conv_k3_bwd_weight(*args, buf, n, _lib.stream_ptr()) == _lib.ERR_ARG
        assert "3 slices" in lib.rpde_last_error().decode()
    assert lib.rpde_conv_k3_bwd_weight(None, *args[1:], None, 0, _lib.stream_ptr()) == _lib.ERR_ARG
    assert "null" in lib.rpde_last_error().decode()
