"""The active-scalar equation-residual loss on the device (csrc/nsc_residual.hip through rpde.ops.nsc2d_residual and
utils.loss.ActiveScalarResidualLoss) against the float64 restatement tests/nsc_residual_ref.py.

The bound of every parity check is nsc_solver_ref.FLOOR_FACTOR (4) times the float32 restatement's own error on the same
fp32 inputs (the largest over the case's samples, never below 2^-22), as for the generators and the other residuals:
rel per sample, the reductions, and the gradient as a whole tensor in relative L2.  The bounds were fixed before any
device run; DESIGN.md 10.15 has the measured device / floor ratios."""
import copy
import json
import math

import pytest
import torch

from tests import ns_solver_ref as S
from tests import nsc_residual_ref as R
from tests import nsc_solver_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = R.FLOOR_FACTOR


def _tables(M, N, f=None, visc=R.VISC, kappa=R.KAPPA, interval=R.INTERVAL):
    from rpde import ops
    return (ops.nsc2d_residual_tables(M, N, visc, kappa, interval),
            None if f is None else ops.ns2d_residual_forcing(f, visc, interval))


def _run(p, x, tabs, fs=None, affine=None, size_average=True, reduction=True, weights=None, beta=R.BETA, scalar_weight=1.0):
    """(value, grad_p) on the device; reduction=False: the gradient of sum_b weights_b rel_b (weights default to 1)"""
    from rpde import ops
    p = p.to(DEV).requires_grad_(True)
    v = ops.nsc2d_residual(p, x.to(DEV), tabs, beta, fs, scalar_weight, affine, size_average, reduction)
    if reduction:
        v.backward()
    else:
        v.backward(torch.ones_like(v) if weights is None else weights.to(DEV))
    torch.cuda.synchronize()
    return v.detach().cpu(), p.grad.detach().cpu()


def _err(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "free"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_parity_with_float64(gpu_device, case, kind, forced):
    """rel, the mean / sum / vector reductions and grad_p -- of the mean, of the sum and of the per-sample vector under
    random upstream weights -- against float64"""
    B, M, N = case
    ref = R.parity_reference(case, kind, forced)
    tabs, fs = _tables(M, N, ref["f"])
    rel64, grad64 = ref["rel64"], ref["grad64"]
    b_rel, b_grad = F * ref["floor_rel"], F * ref["floor_grad"]
    w = torch.rand(B, generator=torch.Generator().manual_seed(B + M + N)) * 2.0 + 0.25
    rel, g_vec = _run(ref["p"], ref["x"], tabs, fs, reduction=False, weights=w)
    mean, g_mean = _run(ref["p"], ref["x"], tabs, fs, size_average=True)
    total, g_sum = _run(ref["p"], ref["x"], tabs, fs, size_average=False)
    e_rel = float(((rel.double() - rel64).abs() / rel64).max())
    e_mean = abs(float(mean) - float(rel64.mean())) / float(rel64.mean())
    e_sum = abs(float(total) - float(rel64.sum())) / float(rel64.sum())
    e_vec = _err(g_vec, grad64 * w.double()[:, None, None, None])
    e_gm, e_gs = _err(g_mean, grad64 / B), _err(g_sum, grad64)
    print(f"{case} {kind} {'forced' if forced else 'free'}: rel {e_rel:.2e} mean {e_mean:.2e} sum {e_sum:.2e} (bound {b_rel:.2e}, "
          f"floor x {e_rel / ref['floor_rel']:.2f})  grad vec {e_vec:.2e} mean {e_gm:.2e} sum {e_gs:.2e} (bound {b_grad:.2e}, "
          f"floor x {e_gs / ref['floor_grad']:.2f})")
    assert tuple(rel.shape) == (B,) and mean.dim() == 0 and total.dim() == 0 and tuple(g_sum.shape) == (B, 3, M, N)
    assert e_rel <= b_rel and e_mean <= b_rel and e_sum <= b_rel
    assert e_vec <= b_grad and e_gm <= b_grad and e_gs <= b_grad


@pytest.mark.parametrize("case", [(2, 4, 6), (2, 32, 48)], ids=R.case_id)
def test_affine_decode_is_folded_in(gpu_device, case):
    """against the restatement on the decoded fields (float64 decode of the same fp32 inputs), two different maps"""
    B, M, N = case
    ref = R.parity_reference(case, "noisy", True)
    tabs, fs = _tables(M, N, ref["f"])
    p, x = ref["p"], ref["x"]
    for aff in ((1.75, 0.3, 1.75, 0.3), (0.6, -0.2, 1.3, 0.1)):
        aff = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in aff)    # the ABI takes floats: decode with those
        rel64, grad64, b_rel, b_grad = R.floors(p, x, M, N, R.VISC, R.KAPPA, R.BETA, R.INTERVAL, ref["f"], aff)
        rel_a, g_a = _run(p, x, tabs, fs, affine=aff, reduction=False)
        e_rel = float(((rel_a.double() - rel64).abs() / rel64).max())
        print(f"affine {case} {aff}: rel {e_rel:.2e} (bound {b_rel:.2e}) grad {_err(g_a, grad64):.2e} (bound {b_grad:.2e})")
        assert e_rel <= b_rel and _err(g_a, grad64) <= b_grad


@pytest.mark.parametrize("lam", [0.25, 4.0])
def test_scalar_weight(gpu_device, lam):
    case = B, M, N = (2, 16, 24)
    ref = R.parity_reference(case, "noisy", True)
    tabs, fs = _tables(M, N, ref["f"])
    rel64, grad64, b_rel, b_grad = R.floors(ref["p"], ref["x"], M, N, R.VISC, R.KAPPA, R.BETA, R.INTERVAL, ref["f"],
                                            scalar_weight=lam)
    rel, g = _run(ref["p"], ref["x"], tabs, fs, reduction=False, scalar_weight=lam)
    e_rel = float(((rel.double() - rel64).abs() / rel64).max())
    print(f"scalar_weight {lam}: rel {e_rel:.2e} (bound {b_rel:.2e}) grad {_err(g, grad64):.2e} (bound {b_grad:.2e})")
    assert e_rel <= b_rel and _err(g, grad64) <= b_grad
    # the weight matters on these inputs
    assert float(((rel64 - ref["rel64"]).abs() / ref["rel64"]).min()) > 100 * b_rel


@pytest.mark.parametrize("grid", [(4, 6), (8, 8), (64, 64)], ids=str)
def test_bitwise_repeatable_and_independent_of_the_batch(gpu_device, grid):
    M, N = grid
    gen = torch.Generator().manual_seed(9)
    w = S.initial_vorticity(3, M, N, seed=7)
    x = G.fields_of(torch.fft.rfft2(w), torch.fft.rfft2(G.initial_scalar(3, M, N, seed=8)), M, N).float()
    p = (x.double() + 0.1 * torch.randn(3, 3, M, N, generator=gen, dtype=torch.float64)).float()
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
    z = torch.zeros(2, 3, M, N)
    for kw in (dict(reduction=False), dict(size_average=True), dict(size_average=False)):
        v, g = _run(z, z, tabs, None, **kw)
        assert bool(torch.isfinite(v).all()) and not v.any() and bool(torch.isfinite(g).all()) and not g.any()


def test_state_is_the_curl_and_the_scalar(gpu_device):
    """the state handed to the generator's fan-out, (X_w, P_w, X_c, P_c), against the float64 restatement's spectra: the
    rounding of a float64 value, a few ulp of the largest entry"""
    from rpde import ops
    case = B, M, N = (2, 6, 10)
    K = N // 2 + 1
    ref = R.parity_reference(case, "noisy", True)
    s = R.spectrum(ref["p"].double(), ref["x"].double(), ref["T64"], R.BETA)
    Xw = R.curl(s["Xq"], s["Xv"], ref["T64"][0])
    st = ops.nsc2d_residual_state(ref["p"].to(DEV), ref["x"].to(DEV)).cpu().double()
    assert tuple(st.shape) == (4, B, M, 2, 8) and not st[..., K:].any()
    for got, want in zip(st, (Xw, s["Pw"], s["Xc"], s["Pc"])):
        e = max(float((got[:, :, 0, :K] - want.real).abs().max()), float((got[:, :, 1, :K] - want.imag).abs().max()))
        assert e <= 4 * 2.0 ** -24 * float(want.abs().max()), e


@pytest.mark.parametrize("grid", [(32, 48), (64, 64)], ids=str)
def test_consecutive_generator_snapshots_satisfy_the_equation(gpu_device, grid):
    """x and p are consecutive snapshots of the device generator at nsc_solver_ref's constants: rel < 0.1 rel(p = x) per
    sample (float64 restatement: at most 0.058).  This pins the signs, the buoyancy's axis and the de-aliasing of the
    loss to the generator's, not merely to its own restatement."""
    from rpde import ops
    from utils.loss import ActiveScalarResidualLoss
    M, N = grid
    B = 4
    w0 = S.initial_vorticity(B, M, N, seed=5).float().to(DEV)
    c0 = G.initial_scalar(B, M, N, seed=6).float().to(DEV)
    every = int(round(R.INTERVAL / G.DT))
    fields, _ = ops.nsc2d_solve(w0, c0, S.forcing(M, N).float().to(DEV), R.VISC, R.KAPPA, R.BETA, G.DT, 3 * every, every)
    x, p = fields[:, 1].contiguous(), fields[:, 2].contiguous()
    loss = ActiveScalarResidualLoss(R.VISC, R.KAPPA, R.BETA, R.INTERVAL, forcing="reference", reduction=False)
    true, still = loss(p, None, x).cpu(), loss(x, None, x).cpu()
    flat = ActiveScalarResidualLoss(R.VISC, R.KAPPA, 0.0, R.INTERVAL, forcing="reference", reduction=False)(p, None, x).cpu()
    print(grid, "true", true.tolist(), "persistence", still.tolist(), "no buoyancy", flat.tolist())
    assert tuple(true.shape) == (B,) and bool(torch.isfinite(true).all()) and bool((true < 0.1 * still).all())
    assert bool((flat > true).all())


def _sum_loss():
    from utils.loss import ActiveScalarResidualLoss, RelativeL2Loss, SumLoss
    return SumLoss([(1.0, RelativeL2Loss()), (0.1, ActiveScalarResidualLoss(1e-3, 2e-3, 5.0, 0.01, forcing="reference"))])


def test_end_to_end_on_generated_files(gpu_device, tmp_path, capsys):
    """the generator CLI writes two files, the loader reads them, FFNO2D(3, 3) AdamW steps under RelativeL2 + 0.1 x the
    residual go through train() eagerly and as a hipGraph to the same weights (the bound of
    tests/test_gpu_ns_residual.py::test_graphed_step_matches_eager), and main_2d runs an epoch with
    training.loss=residual on the loader's min-max normalised fields (the four scalar extrema fold into the loss)"""
    from data_generation import active_scalar_2d as gen
    from dataloaders.active_matter_all_markov import MultiFileActiveMatterMarkovDataset
    from models.ffno import FFNO2D
    from rpde.entry import run
    from rpde.optim import FlatAdamW
    from train.training import train
    gen.main(["--resolution", "32", "--samples", "3", "--batch", "3", "--T", "0.07", "--dt", "1e-3", "--record-steps", "7",
              "--files", "2", "--visc", "1e-3", "--kappa", "2e-3", "--beta", "5", "--out-dir", str(tmp_path)])
    data = MultiFileActiveMatterMarkovDataset("active_scalar_*.npz", str(tmp_path), s=32)
    assert len(data) == 42 and tuple(data[0][0].shape) == (3, 32, 32)

    # four steps of one batch shape: train() runs two eagerly before it captures, so two are replays
    batch = [data[i] for i in range(32)]
    loader = lambda: torch.utils.data.DataLoader(batch, batch_size=8, shuffle=False)   # noqa: E731
    torch.manual_seed(0)
    m0 = FFNO2D(in_channels=3, out_channels=3, width=16, n_layers=2, n_modes=8, factor=2, ff_weight_norm=True,
                n_ff_layers=2, layer_norm=True, dropout=0.0).to(gpu_device)
    trained = []
    for graph in (False, True):
        m = copy.deepcopy(m0)
        loss_fn = _sum_loss()
        loss_fn.warm((32, 32), gpu_device)
        opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, capturable=graph)
        tl, vl = train(m, loader(), loader(), opt, None, epochs=1, device=gpu_device, graph=graph, loss_fn=loss_fn)
        assert len(tl) == 1 and all(math.isfinite(v) for v in tl + vl)
        trained.append((m, tl[0]))
    assert abs(trained[0][1] - trained[1][1]) <= 1e-6 * max(1.0, abs(trained[0][1]))
    moved = 0.0
    for p0, pe, pg in zip(m0.parameters(), trained[0][0].parameters(), trained[1][0].parameters()):
        real = lambda t: torch.view_as_real(t.detach()) if t.is_complex() else t.detach()   # noqa: E731
        assert float((real(pe) - real(pg)).norm() / (real(pe).norm() + 1e-30)) < 1e-6
        moved = max(moved, float((real(pe) - real(p0)).norm()))
    assert moved > 0.0

    capsys.readouterr()
    l2 = run(2, ["model=ffno_2d/ffno_2d_3ch", "dataset=ns/ns_active_generated", f"dataset.dataset_params.saved_folder={tmp_path}",
                 "dataset.dataset_params.s=32", "dataset.original_res=32",
                 "dataset.equation.diffusivity=2e-3", "dataset.equation.buoyancy=5", "dataset.equation.interval=0.01",
                 "model.width=16", "model.n_layers=2", "model.n_modes=8", "model.factor=2", "training.epochs=1",
                 "training.batch_size=8", "training.loss=residual", f"checkpoint_dir={tmp_path}"])
    out = capsys.readouterr().out
    rec = [json.loads(ln) for ln in out.splitlines() if '"test_rel_l2"' in ln]
    assert math.isfinite(l2) and l2 > 0 and rec and rec[0]["test_rel_l2"] == l2
    assert math.isfinite(rec[0]["final_train_loss"]) and rec[0]["final_train_loss"] > 0
