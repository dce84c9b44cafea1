"""The vorticity equation-residual loss on the device (csrc/ns_residual.hip through rpde.ops.ns2d_residual and
utils.loss.VorticityResidualLoss) against the float64 restatement tests/ns_residual_ref.py.

The bound of every parity check is ns_solver_ref.FLOOR_FACTOR (4) times the float32 restatement's own error on the same
fp32 inputs (the largest over the case's samples, never below 2^-22), as for the generators and the 1-D residual: rel per
sample, the reductions, and the gradient as a whole tensor in relative L2.

Measured on an MI355X: all 40 parity cases hold every bound.  Noisy p: rel at most 0.10 of its bound, the gradient at
most 0.20.  The exact pairs (rel a remainder of 1e-3 of the field) are the tight ones; the three tightest, per-sample rel:

    case                      device error of rel   bound (4 x floor)   floor of the float32 restatement
    1x48x32 exact, unforced   9.49e-07              1.32e-06            3.3e-07 (another host: the 2^-22 minimum, bound 9.54e-07)
    1x48x32 exact, forced     4.33e-07              9.54e-07            2^-22 (the minimum)
    2x6x10 exact, forced      2.67e-05              7.67e-05            1.9e-05

With d^ on the layer's fp32 transform the first of them had 1.16e-06: inside the bound of that host, outside the smallest
bound the rule can give.  So x^ and d^ both come from the float64 analysis; what is left enters through the products
(DESIGN.md 10.12)."""
import copy
import math

import pytest
import torch

from tests import ns_residual_ref as R
from tests import ns_solver_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = R.FLOOR_FACTOR


def _tables(M, N, f=None, visc=S.VISC, interval=R.INTERVAL):
    from rpde import ops
    return ops.ns2d_residual_tables(M, N, visc, interval), None if f is None else ops.ns2d_residual_forcing(f, visc, interval)


def _run(p, x, tabs, fs=None, affine=None, size_average=True, reduction=True, weights=None):
    """(value, grad_p) on the device; reduction=False: the gradient of sum_b weights_b rel_b (weights default to 1)"""
    from rpde import ops
    p = p.to(DEV).requires_grad_(True)
    v = ops.ns2d_residual(p, x.to(DEV), tabs, fs, affine, size_average, reduction)
    if reduction:
        v.backward()
    else:
        v.backward(torch.ones_like(v) if weights is None else weights.to(DEV))
    torch.cuda.synchronize()
    return v.detach().cpu(), p.grad.detach().cpu()


def _err(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("case", [(2, 4, 6), (1, 12, 6), (3, 16, 24), (2, 64, 64), (1, 48, 160), (16, 1024, 32), (1, 1030, 8),
                                  (1, 4, 1030)], ids=R.case_id)
def test_float64_analysis_against_torch(gpu_device, case):
    """the separable float64 analysis alone: a float64 sum of M N products carries at most M N 2^-53 sum |x| of error
    (the twiddles are correctly rounded to a few ulp: a factor 4 for them), and its fp32 copy is its rounding.  160 columns:
    more than one block of columns; 16 x 1024 x 32: the kernels that own four rows and eight ky per thread (512 blocks
    and more), whose bits are those of the narrow ones a single sample takes; an axis of 1030: the roots of unity stay
    in global memory, and the last group of rows is partial"""
    from rpde import ops
    B, M, N = case
    K = N // 2 + 1
    x = torch.randn(B, M, N, generator=torch.Generator().manual_seed(3 + M + N)) * 3.0 + 0.5
    for affine in (None, (1.75, -0.3125)):                                      # fp32 numbers: the ABI takes floats
        s64, s32 = ops.ns2d_residual_spectrum(x.to(DEV), affine)
        s64, s32 = s64.cpu(), s32.cpu()
        xt = x.double() if affine is None else affine[0] * x.double() + affine[1]
        want = torch.fft.rfft2(xt)
        bound = 4.0 * M * N * 2.0 ** -53 * float(xt.abs().sum((1, 2)).max())
        e = max(float((s64[:, :, 0, :K] - want.real).abs().max()), float((s64[:, :, 1, :K] - want.imag).abs().max()))
        print(f"analysis {case} affine {affine}: max abs error {e:.2e} (bound {bound:.2e})")
        assert e <= bound
        assert not s64[..., K:].any() and not s32[..., K:].any() and torch.equal(s32, s64.float())
        if B == 16:
            alone, _ = ops.ns2d_residual_spectrum(x[5:6].to(DEV), affine)
            assert torch.equal(alone.cpu()[0], s64[5])


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "free"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.CASES + R.EDGE_CASES, ids=R.case_id)
def test_parity_with_float64(gpu_device, case, kind, forced):
    """rel, the mean / sum / vector reductions, the saved per-sample norms and grad_p against float64"""
    B, M, N = case
    ref = R.parity_reference(case, kind, forced)
    tabs, fs = _tables(M, N, ref["f"])
    rel64, grad64 = ref["rel64"], ref["grad64"]
    b_rel, b_grad = F * ref["floor_rel"], F * ref["floor_grad"]
    rel, g_vec = _run(ref["p"], ref["x"], tabs, fs, reduction=False)
    mean, g_mean = _run(ref["p"], ref["x"], tabs, fs, size_average=True)
    total, g_sum = _run(ref["p"], ref["x"], tabs, fs, size_average=False)
    e_rel = float(((rel.double() - rel64).abs() / rel64).max())
    e_mean = abs(float(mean) - float(rel64.mean())) / float(rel64.mean())
    e_sum = abs(float(total) - float(rel64.sum())) / float(rel64.sum())
    e_g = _err(g_vec, grad64)
    print(f"{case} {kind} {'forced' if forced else 'free'}: rel {e_rel:.2e} mean {e_mean:.2e} sum {e_sum:.2e} (bound {b_rel:.2e})  "
          f"grad {e_g:.2e} mean {_err(g_mean, grad64 / B):.2e} sum {_err(g_sum, grad64):.2e} (bound {b_grad:.2e})")
    assert tuple(rel.shape) == (B,) and mean.dim() == 0 and total.dim() == 0
    assert e_rel <= b_rel and e_mean <= b_rel and e_sum <= b_rel
    assert e_g <= b_grad and _err(g_mean, grad64 / B) <= b_grad and _err(g_sum, grad64) <= b_grad
    if case == (3, 8, 8):
        # [B, 1, M, N] is the same call, and per-sample upstream gradients scale the samples' gradients
        rel4, g4 = _run(ref["p"][:, None], ref["x"][:, None], tabs, fs, reduction=False)
        assert tuple(g4.shape) == (B, 1, M, N) and torch.equal(rel4, rel) and torch.equal(g4[:, 0], g_vec)
        w = torch.tensor([0.5, -2.0, 3.0])
        _, gw = _run(ref["p"], ref["x"], tabs, fs, reduction=False, weights=w)
        assert _err(gw, grad64 * w.double()[:, None, None]) <= b_grad


@pytest.mark.parametrize("case", [(2, 4, 6), (2, 32, 48)], ids=R.case_id)
def test_affine_decode_is_folded_in(gpu_device, case):
    """against the restatement on the decoded fields (float64 decode of the same fp32 inputs), two different maps"""
    B, M, N = case
    ref = R.parity_reference(case, "noisy", True)
    tabs, fs = _tables(M, N, ref["f"])
    p, x = ref["p"], ref["x"]
    for aff in ((1.75, 0.3, 1.75, 0.3), (0.6, -0.2, 1.3, 0.1)):
        aff = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in aff)    # the ABI takes floats: decode with those
        rel64, grad64, b_rel, b_grad = R.floors(p, x, M, N, S.VISC, R.INTERVAL, ref["f"], aff)
        rel_a, g_a = _run(p, x, tabs, fs, affine=aff, reduction=False)
        e_rel = float(((rel_a.double() - rel64).abs() / rel64).max())
        print(f"affine {case} {aff}: rel {e_rel:.2e} (bound {b_rel:.2e}) grad {_err(g_a, grad64):.2e} (bound {b_grad:.2e})")
        assert e_rel <= b_rel and _err(g_a, grad64) <= b_grad


@pytest.mark.parametrize("grid", [(4, 6), (8, 8), (64, 64)], ids=str)
def test_bitwise_repeatable_and_independent_of_the_batch(gpu_device, grid):
    M, N = grid
    w = S.initial_vorticity(3, M, N, seed=7)
    gen = torch.Generator().manual_seed(9)
    x = w.float()
    p = (w + 0.1 * torch.randn(3, M, N, generator=gen, dtype=torch.float64)).float()
    tabs, fs = _tables(M, N, S.forcing(M, N))
    first = _run(p, x, tabs, fs, reduction=False)
    again = _run(p, x, tabs, fs, reduction=False)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    m1, m2 = _run(p, x, tabs, fs), _run(p, x, tabs, fs)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    for b in range(3):
        alone = _run(p[b:b + 1], x[b:b + 1], tabs, fs, reduction=False)
        assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b]), b


@pytest.mark.parametrize("grid", [(4, 6), (16, 12)], ids=str)
def test_zero_fields(gpu_device, grid):
    M, N = grid
    tabs, _ = _tables(M, N)
    z = torch.zeros(2, M, N)
    for kw in (dict(reduction=False), dict(size_average=True), dict(size_average=False)):
        v, g = _run(z, z, tabs, None, **kw)
        assert bool(torch.isfinite(v).all()) and not v.any() and bool(torch.isfinite(g).all()) and not g.any()


@pytest.mark.parametrize("grid", [(32, 48), (64, 64)], ids=str)
def test_consecutive_generator_snapshots_satisfy_the_equation(gpu_device, grid):
    """x and p are consecutive snapshots of the device generator at ns_solver_ref's constants: rel < 0.1 rel(p = x) per
    sample (float64 restatement: shares 0.02 .. 0.04).  This pins the signs and the de-aliasing of the loss to the
    generator's, not merely to its own restatement."""
    from rpde import ops
    from utils.loss import VorticityResidualLoss
    M, N = grid
    B = 4
    w0 = S.initial_vorticity(B, M, N, seed=5).float().to(DEV)
    every = int(round(R.INTERVAL / S.DT))
    snaps = ops.ns2d_solve(w0, S.forcing(M, N).float().to(DEV), S.VISC, S.DT, 3 * every, every)
    x, p = snaps[..., 1].contiguous(), snaps[..., 2].contiguous()
    loss = VorticityResidualLoss(S.VISC, R.INTERVAL, forcing="reference", reduction=False)
    true, still = loss(p, None, x).cpu(), loss(x, None, x).cpu()
    print(grid, "true", true.tolist(), "persistence", still.tolist())
    assert tuple(true.shape) == (B,) and bool(torch.isfinite(true).all()) and bool((true < 0.1 * still).all())


def test_forcing_sign(gpu_device):
    """a pair that the forcing carries (tests/test_ns_residual_cpu.py asserts the share on the CPU): the forced tables
    bring the residual below a tenth of what the unforced ones leave; the wrong sign would double it"""
    x, p, f = R.forcing_pair()
    B, M, N = R.FORCING_CASE
    tabs, fs = _tables(M, N, f)
    unforced, _ = _run(p.float(), x.float(), tabs, None, reduction=False)
    forced, _ = _run(p.float(), x.float(), tabs, fs, reduction=False)
    print("unforced", unforced.tolist(), "forced", forced.tolist())
    assert bool((forced < 0.1 * unforced).all())


def _sum_loss():
    from utils.loss import RelativeL2Loss, SumLoss, VorticityResidualLoss
    return SumLoss([(1.0, RelativeL2Loss()), (0.1, VorticityResidualLoss(1e-3, 0.05, forcing="reference"))])


def test_graphed_step_matches_eager(gpu_device):
    """a tiny FNO2d trained on data + residual: three eager steps against three replays of
    rpde.graph.GraphedTrainStep(loss_takes_input=True), after warm(); the bounds of
    tests/test_gpu_etd_residual.py::test_graphed_step_matches_eager"""
    from models.fno import FNO2d
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    torch.manual_seed(3)
    m_e = FNO2d(1, 1, modes1=4, modes2=4, width=8, n_blocks=2).to(gpu_device).train()
    m_g = copy.deepcopy(m_e)
    xs = [torch.randn(4, 1, 16, 24, device=gpu_device) for _ in range(3)]
    ys = [torch.randn(4, 1, 16, 24, device=gpu_device) for _ in range(3)]
    loss_fn = _sum_loss()
    loss_fn.warm((16, 24), gpu_device)
    o_e = FlatAdamW(m_e.parameters(), lr=1e-3, capturable=True)
    o_g = FlatAdamW(m_g.parameters(), lr=1e-3, capturable=True)
    warm = 2
    for _ in range(warm):
        o_e.zero_grad(set_to_none=False)
        loss_fn(m_e(xs[0]), ys[0], xs[0]).backward()
        o_e.step()
    step = GraphedTrainStep(m_g, loss_fn, o_g, xs[0], ys[0], warmup=warm, loss_takes_input=True)
    for x, y in zip(xs, ys):
        o_e.zero_grad(set_to_none=False)
        le = loss_fn(m_e(x), y, x)
        le.backward()
        o_e.step()
        lg = step(x, y)
        assert abs(float(le.detach()) - float(lg)) <= 1e-6 * max(1.0, abs(float(le.detach())))
        del le
    for pe, pg in zip(m_e.parameters(), m_g.parameters()):
        a, b = torch.view_as_real(pe) if pe.is_complex() else pe, torch.view_as_real(pg) if pg.is_complex() else pg
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-6
    # the residual term reached the step: with the data term alone the loss is another number
    with torch.no_grad():
        both = float(loss_fn(m_e(xs[0]), ys[0], xs[0]))
        data = float(loss_fn.terms[0](m_e(xs[0]), ys[0]))
    assert both > data


def test_train_takes_the_loss(gpu_device):
    """train(loss_fn=SumLoss(data + residual)) runs an epoch eagerly and with graph=True and returns finite histories"""
    from models.fno import FNO2d
    from rpde.optim import FlatAdamW
    from train.training import train
    torch.manual_seed(11)
    m0 = FNO2d(1, 1, modes1=4, modes2=4, width=8, n_blocks=2).to(gpu_device)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(1, 16, 16, generator=g), torch.randn(1, 16, 16, generator=g)) for _ in range(16)]
    loader = lambda: torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)   # noqa: E731
    for graph in (False, True):
        m = copy.deepcopy(m0)
        loss_fn = _sum_loss()
        loss_fn.warm((16, 16), gpu_device)
        opt = FlatAdamW(m.parameters(), lr=2e-3, capturable=graph)
        tl, vl = train(m, loader(), loader(), opt, None, epochs=1, device=gpu_device, graph=graph, loss_fn=loss_fn)
        assert len(tl) == 1 and len(vl) == 1 and all(math.isfinite(v) for v in tl + vl)


@pytest.mark.parametrize("graph,use_normalizer", [(False, False), (True, True)])
def test_entry_point_residual_on_generated_ns(gpu_device, tmp_path, capsys, graph, use_normalizer):
    """training.loss=residual trains main_2d on a generated 32 x 32 Navier-Stokes file, eagerly and as a hipGraph, with
    the prediction decoded by the loss (use_normalizer false) or by train() (true); the `equation:` block is overridden
    to the arguments the data was generated with, and the reported scores stay relative L2"""
    import json
    from data_generation import ns_2d
    from rpde.entry import run
    ns_2d.main(["--resolution", "32", "--samples", "16", "--batch", "16", "--viscosity", "1e-3", "--T", "0.4", "--dt", "2e-3",
                "--record-steps", "8", "--out", str(tmp_path / "ns_32.npz")])
    l2 = run(2, ["model=ffno_2d/ffno_2d", "dataset=ns/ns_generated", "dataset.dataset_params.filename=ns_32.npz",
                 f"dataset.dataset_params.saved_folder={tmp_path}", "dataset.original_res=32",
                 "dataset.equation.viscosity=1e-3", "dataset.equation.interval=0.05",
                 "model.width=16", "model.n_layers=2", "model.n_modes=8", "model.factor=2", "training.epochs=1",
                 "training.batch_size=16", "training.loss=residual", "training.loss_lambda=0.2",
                 f"training.graph={str(graph).lower()}", f"training.use_normalizer={str(use_normalizer).lower()}",
                 f"checkpoint_dir={tmp_path}"])
    out = capsys.readouterr().out
    rec = [json.loads(ln) for ln in out.splitlines() if '"test_rel_l2"' in ln]
    assert math.isfinite(l2) and 0 < l2 < 2.0 and rec and rec[0]["test_rel_l2"] == l2
    assert math.isfinite(rec[0]["final_train_loss"]) and rec[0]["final_train_loss"] > 0
    # a 2-D data set without the mapping is refused in words
    with pytest.raises(SystemExit, match="one-dimensional"):
        run(2, ["model=ffno_2d/ffno_2d", "dataset=ns/ns_file", "dataset.dataset_params.filename=ns_32.npz",
                f"dataset.dataset_params.saved_folder={tmp_path}", "training.loss=residual", f"checkpoint_dir={tmp_path}"])
