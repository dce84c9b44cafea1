"""CPU: oracle/adamw.py (one AdamW step restated in float64) against torch.optim.AdamW on float64 CPU tensors, over
steps in which the learning rate and the weight decay change, with a real and a complex parameter.  The GPU optimizer
tests (tests/test_gpu_optimizer_state.py) check every HIP step against this restatement."""
import pytest
import torch

from oracle.adamw import adamw_step_f64


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-3)])
def test_adamw_step_f64_matches_torch_adamw(betas, eps):
    gen = torch.Generator().manual_seed(5)
    a = torch.nn.Parameter(torch.randn(6, 5, dtype=torch.float64, generator=gen) * 0.1)
    c = torch.nn.Parameter(torch.randn(4, 3, dtype=torch.complex128, generator=gen) * 0.1)
    opt = torch.optim.AdamW([a, c], lr=1e-3, betas=betas, eps=eps, weight_decay=1e-2, foreach=False)
    state = {id(p): (_real(p.detach()).clone(), torch.zeros_like(_real(p.detach())), torch.zeros_like(_real(p.detach())))
             for p in (a, c)}
    for t in range(1, 21):
        lr, wd = 1e-3 * (1.0 + 0.5 * ((t * 7) % 5)), (0.0, 1e-2, 0.3)[t % 3]
        if t == 13:
            lr = 0.0
        opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"] = lr, wd
        # gradients of several magnitudes, one element with a zero gradient every other step
        ga = torch.randn(a.shape, dtype=torch.float64, generator=gen) * 10.0 ** (t % 4 - 2)
        gc = torch.randn(c.shape, dtype=torch.complex128, generator=gen) * 10.0 ** (-(t % 3))
        if t % 2:
            ga[0, 0] = 0.0
        a.grad, c.grad = ga.clone(), gc.clone()
        opt.step()
        for p, g in ((a, ga), (c, gc)):
            p0, m0, v0 = state[id(p)]
            p1, m1, v1 = adamw_step_f64(p0, g, m0, v0, t, lr, wd, betas, eps)
            st = opt.state[p]
            assert int(float(st["step"])) == t
            for got, want in ((_real(p.detach()), p1), (_real(st["exp_avg"]), m1), (_real(st["exp_avg_sq"]), v1)):
                assert got.shape == want.shape
                err = float((got - want).abs().max())
                assert err <= 1e-14 * max(1.0, float(want.abs().max())), (t, err)
            state[id(p)] = (p1, m1, v1)


def test_adamw_step_f64_takes_complex_as_pairs_and_refuses_step_zero():
    p = torch.tensor([0.1 + 0.2j, -0.3 + 0.0j], dtype=torch.complex64)
    g = torch.tensor([1.0 - 1.0j, 0.5 + 2.0j], dtype=torch.complex64)
    z = torch.zeros(2, 2, dtype=torch.float64)
    p1, m1, v1 = adamw_step_f64(p, g, z, z, 1, 1e-3, 0.0)
    assert p1.dtype == torch.float64 and p1.shape == (2, 2)
    # first step from zero moments: the update is lr * g / (|g| + eps * ...) elementwise, i.e. lr * sign(g) for |g| >> eps
    gr = torch.view_as_real(g).double()
    assert torch.allclose(p1, torch.view_as_real(p).double() - 1e-3 * gr.sign(), atol=1e-10)
    assert torch.allclose(m1, 0.1 * gr, atol=1e-15) and torch.allclose(v1, 1e-3 * gr * gr, atol=1e-15)
    with pytest.raises(ValueError):
        adamw_step_f64(p, g, z, z, 0, 1e-3, 0.0)
