"""The Darcy equation-residual loss on the device (csrc/darcy_residual.hip through rpde.ops.darcy2d_residual and
utils.loss.DarcyResidualLoss) against the float64 restatement tests/darcy_residual_ref.py.

Grids: darcy_ref.CASES up to 100.  8 is the smallest (every 16-byte group touches a wall), 12 has the first group with
no wall, 20 and 36 are no multiples of 8 / 16 / 32 (stencil, halo and GEMM edge tiles), 36 and up take more than one
block per sample (the fixed-order partials).  Inputs: darcy_ref.parity_reference's coefficients at both contrasts, f = 1.

The bound of every parity check is FLOOR_FACTOR (4) times max(floor32, 2^-24): floor32 is the float32 restatement's own
distance from the float64 one on the same fp32 inputs (the largest over the samples for the value, relative L2 for the
gradient), never taken from the device; 2^-24 is half an ulp of the fp32 result itself, and the value's floor falls
below it on some cases.  On the perturbed predictions the floors are at most 1e-5 / 1e-4 (asserted), so the bound
cannot hide a failure.

Measured on an MI355X: all 48 parity cases and all 24 exact pairs hold every bound.  The value is at most 0.77 of its
bound (B2_s12, contrast 1 / 0.1, smooth, L2: 1.84e-07 against 2.38e-07, the 2^-24 minimum), the gradient at most 0.31,
the exact pair at most 0.55 (B2_s20, 1 / 0.1, L2).  With the subtraction f - A u fused into the row's last product (what
the compiler does unasked) two cases were outside: that value 3.25e-07, and the exact pair B1_s100, 1 / 0.1, L2 at
3.54e-05 against 2.54e-05; the kernel now subtracts the rounded A u, as the restatement and the apply entry do
(test_the_residual_is_f_minus_the_apply_entry)."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import darcy_ref as R
from tests import darcy_residual_ref as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tables(s, norm, forcing=1.0):
    from rpde import ops
    return ops.darcy2d_residual_tables(s, forcing, norm)


def _run(p, a, tabs, affine=None, size_average=True, reduction=True, weights=None):
    """(value, grad_p) on the device; reduction=False: the gradient of sum_b weights_b rel_b (weights default to 1)"""
    from rpde import ops
    p = torch.as_tensor(p).to(DEV).requires_grad_(True)
    v = ops.darcy2d_residual(p, torch.as_tensor(a).to(DEV), tabs, affine, size_average, reduction)
    if reduction:
        v.backward()
    else:
        v.backward(torch.ones_like(v) if weights is None else torch.as_tensor(weights, dtype=torch.float32).to(DEV))
    torch.cuda.synchronize()
    return v.detach().cpu().double().numpy(), p.grad.detach().cpu().double().numpy()


def _err(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def _rel_err(x, ref):
    return float(np.max(np.abs(x - ref) / np.abs(ref)))


@pytest.mark.parametrize("norm", Q.NORMS)
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("contrast", Q.CONTRASTS)
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_parity_with_float64(gpu_device, case, contrast, kind, norm):
    """rel per sample with random per-sample upstream weights, the mean and the sum, and grad_p of each, against float64"""
    B, s = case
    ref = Q.parity_reference(case, contrast, kind, norm)
    a, p, rel64, grad64 = ref["a"], ref["p"], ref["rel64"], ref["grad64"]
    assert ref["floor_rel"] <= 1e-5 and ref["floor_grad"] <= 1e-4              # the condition of the bounds
    b_rel, b_grad = Q.bound(ref["floor_rel"]), Q.bound(ref["floor_grad"])
    tabs = _tables(s, norm)
    w = np.random.default_rng(11 + s).uniform(0.5, 2.0, B) * np.where(np.arange(B) % 2, -1.0, 1.0)
    rel, g_vec = _run(p, a, tabs, reduction=False, weights=w)
    mean, g_mean = _run(p, a, tabs, size_average=True)
    total, g_sum = _run(p, a, tabs, size_average=False)
    e_rel, e_mean, e_sum = _rel_err(rel, rel64), _rel_err(mean, rel64.mean()), _rel_err(total, rel64.sum())
    e_vec, e_gm, e_gs = _err(g_vec, grad64 * w[:, None, None]), _err(g_mean, grad64 / B), _err(g_sum, grad64)
    print(f"{case} {contrast} {kind} {norm}: rel {e_rel:.2e} mean {e_mean:.2e} sum {e_sum:.2e} (bound {b_rel:.2e})  "
          f"grad vec {e_vec:.2e} mean {e_gm:.2e} sum {e_gs:.2e} (bound {b_grad:.2e})")
    assert rel.shape == (B,) and mean.ndim == 0 and total.ndim == 0 and g_vec.shape == (B, s, s)
    assert e_rel <= b_rel and e_mean <= b_rel and e_sum <= b_rel
    assert e_vec <= b_grad and e_gm <= b_grad and e_gs <= b_grad
    if case == (3, 8):
        # [B, 1, s, s], what the loader hands, is the same call
        rel4, g4 = _run(p[:, None], a[:, None], tabs, reduction=False, weights=w)
        assert g4.shape == (B, 1, s, s) and np.array_equal(rel4, rel) and np.array_equal(g4[:, 0], g_vec)


@pytest.mark.parametrize("norm", Q.NORMS)
@pytest.mark.parametrize("contrast", Q.CONTRASTS)
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_the_exact_pair(gpu_device, case, contrast, norm):
    """p = u64 rounded to fp32: the value is rounding (float64: 1e-7 .. 1e-6 in the dual norm, 4e-7 .. 6e-5 in L2, the
    s^2 floor), checked under the same rule -- its floor32 is up to 0.09 relative here.  The gradient is not compared:
    its floor is up to 0.25, which proves nothing.  In the dual norm the value is below 1e-4 of the trivial predictor's"""
    B, s = case
    ref = Q.parity_reference(case, contrast, "exact", norm)
    tabs = _tables(s, norm)
    rel, g = _run(ref["p"], ref["a"], tabs, reduction=False)
    zero, _ = _run(np.zeros_like(ref["p"]), ref["a"], tabs, reduction=False)
    e, b = _rel_err(rel, ref["rel64"]), Q.bound(ref["floor_rel"])
    print(f"{case} {contrast} {norm} exact: rel {rel.tolist()} float64 {ref['rel64'].tolist()} error {e:.2e} (bound {b:.2e}, "
          f"floor32 {ref['floor_rel']:.2e}); p = 0: {zero.tolist()}")
    assert np.isfinite(rel).all() and np.isfinite(g).all()
    assert e <= b
    if norm == "dual":
        assert (rel < 1e-4 * zero).all()


@pytest.mark.parametrize("contrast", Q.CONTRASTS)
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_energy_sandwich_and_the_trivial_predictor(gpu_device, case, contrast):
    """on the device's own E = (rel (D + 1e-8))^2: a_min <= E / (e . A e) <= a_max with e = u* - p in float64; and p = 0
    gives rel = 1 to rounding in both norms.  There r = f exactly.  L2: the squares of f = 1 add exactly, what is left is
    the tail's fp32 arithmetic -- sqrt(E), D, D + 1e-8 and the quotient rounded once each: 4 x 2^-24.  Dual norm:
    S f S^T is two fp32 dot products of s terms per coefficient, each within s 2^-24 of its sum of magnitudes (the
    standard worst-case bound; f = 1 and the low sine modes that carry E have one sign, so magnitudes and values
    agree), squared and under a square root: (2 s + 4) 2^-24 with the tail.  The float32 restatement's own floor is 1e-9
    here (numpy adds pairwise), below any fp32 result"""
    B, s = case
    hi, lo = R.CONTRASTS[contrast][:2]
    for kind in Q.KINDS:
        ref = Q.parity_reference(case, contrast, kind, "dual")
        tabs = _tables(s, "dual")
        rel, _ = _run(ref["p"], ref["a"], tabs, reduction=False)
        e = ref["u64"] - ref["p"].astype(np.float64)
        ratio = (rel * (tabs[3] + 1e-8)) ** 2 / np.sum(e * R.apply(ref["a"].astype(np.float64), e), axis=(1, 2))
        print(case, contrast, kind, "E / e.Ae", ratio.tolist())
        assert (ratio >= lo).all() and (ratio <= hi).all()
    for norm in Q.NORMS:
        ref = Q.parity_reference(case, contrast, "smooth", norm)
        zero = np.zeros_like(ref["p"])
        rel, g = _run(zero, ref["a"], _tables(s, norm), reduction=False)
        bound = (4 if norm == "l2" else 2 * s + 4) * Q.HALF_ULP
        print(case, contrast, norm, "p = 0:", rel.tolist(), "bound", bound)
        assert np.abs(ref["zero64"] - 1.0).max() < 1e-7 and np.abs(rel - 1.0).max() <= bound and np.isfinite(g).all() and g.any()


@pytest.mark.parametrize("case", [(2, 64), (1, 100)], ids=Q.case_id)
def test_the_residual_is_f_minus_the_apply_entry(gpu_device, case):
    """r = f - A u with A u rounded as rpde_darcy2d_apply rounds it (no fusion of the subtraction into the row's last
    product): on the exact pair, where the value is rounding and a fused r gives another number in the fifth digit, the
    L2 value is |f - darcy2d_apply(a, p)| / D to the tail's own rounding (4 x 2^-24)"""
    from rpde import ops
    B, s = case
    ref = Q.parity_reference(case, "1_0.1", "exact", "l2")
    a, p = torch.from_numpy(ref["a"]).to(DEV), torch.from_numpy(ref["p"]).to(DEV)
    r = torch.from_numpy(ref["f"]) - ops.darcy2d_apply(a, p).cpu()              # fp32, one rounding per element
    want = np.sqrt((r.double() ** 2).sum((1, 2)).numpy()) / (float(s) + 1e-8)
    rel, _ = _run(ref["p"], ref["a"], _tables(s, "l2"), reduction=False)
    print(case, "rel", rel.tolist(), "from the apply entry", want.tolist())
    assert _rel_err(rel, want) <= 4 * Q.HALF_ULP


@pytest.mark.parametrize("norm", Q.NORMS)
@pytest.mark.parametrize("case", [(3, 8), (2, 36)], ids=Q.case_id)
def test_affine_decode_is_folded_in(gpu_device, case, norm):
    """the fields as a SimpleNormalizer encodes them plus `affine` give the loss of the decoded fields, and a_p times its
    gradient: against the restatement, which decodes the same fp32 inputs in float64.  The encoded coefficient is
    negative wherever a < mean: without the map the operator would mean nothing"""
    B, s = case
    ref = Q.parity_reference(case, "12_3", "white", norm)
    a, p = ref["a"], ref["p"]
    f32 = lambda v: float(np.float32(v))                                        # noqa: E731  the ABI takes floats
    aff = (f32(p.std() + 1e-5), f32(p.mean()), f32(a.std() + 1e-5), f32(a.mean()))
    p_enc, a_enc = ((p - aff[1]) / aff[0]).astype(np.float32), ((a - aff[3]) / aff[2]).astype(np.float32)
    assert (a_enc < 0).any() and (a_enc > 0).any()
    w = np.array([0.7, -1.3, 2.0][:B])
    rel64, grad64, fv, fg = Q.floors(a_enc, p_enc, ref["f"], norm, aff, w)
    assert fv <= 1e-5 and fg <= 1e-4
    rel, g = _run(p_enc, a_enc, _tables(s, norm), affine=aff, reduction=False, weights=w)
    print(f"affine {case} {norm}: rel {_rel_err(rel, rel64):.2e} (bound {Q.bound(fv):.2e}) grad {_err(g, grad64):.2e} (bound {Q.bound(fg):.2e})")
    assert _rel_err(rel, rel64) <= Q.bound(fv) and _err(g, grad64) <= Q.bound(fg)
    # the decoded fields themselves: the same loss to the decode's rounding, and the gradient a_p times theirs
    plain, g_plain = _run(p, a, _tables(s, norm), reduction=False, weights=w)
    assert _rel_err(rel, plain) < 1e-3 and _err(g, aff[0] * g_plain) < 1e-3


@pytest.mark.parametrize("norm", Q.NORMS)
@pytest.mark.parametrize("s", [8, 36, 64])
def test_bitwise_repeatable_and_independent_of_the_batch(gpu_device, s, norm):
    ref = R.parity_reference((3, 8) if s == 8 else (2, s), "12_3")
    a = ref["a"]
    p = (ref["u64"] * (1.0 + 0.02 * np.random.default_rng(s).standard_normal(a.shape))).astype(np.float32)
    tabs = _tables(s, norm)
    aff = (1.25, 0.001, 0.5, 1.0)
    first, again = _run(p, a, tabs, aff, reduction=False), _run(p, a, tabs, aff, reduction=False)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    m1, m2 = _run(p, a, tabs, aff), _run(p, a, tabs, aff)
    assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])
    for b in range(a.shape[0]):
        alone = _run(p[b:b + 1], a[b:b + 1], tabs, aff, reduction=False)
        assert np.array_equal(alone[0][0], first[0][b]) and np.array_equal(alone[1][0], first[1][b]), b


def test_forward_without_gradient_gives_the_same_value(gpu_device):
    """validation: a forward under no_grad (one sep2d, no backward), then a separate forward + backward"""
    from utils.loss import DarcyResidualLoss
    ref = Q.parity_reference((2, 36), "12_3", "smooth", "dual")
    a, p = torch.from_numpy(ref["a"]).to(DEV), torch.from_numpy(ref["p"]).to(DEV)
    for norm in Q.NORMS:
        loss = DarcyResidualLoss(norm=norm)
        with torch.no_grad():
            quiet = loss(p, None, a)
        assert not quiet.requires_grad
        q = p.clone().requires_grad_(True)
        loud = loss(q, None, a)
        loud.backward()
        assert torch.equal(quiet, loud.detach()) and bool(torch.isfinite(q.grad).all()) and bool(q.grad.any())


@pytest.mark.parametrize("s", [32, 64])
def test_the_generators_own_solution_satisfies_the_equation(gpu_device, s):
    """darcy2d_solve at 24 iterations, coefficients 12 / 3: below 1e-4 of the trivial predictor (rel = 1) per sample in
    the dual norm.  This pins the loss to the generator's operator, not merely to its own restatement"""
    from rpde import ops
    from utils.loss import DarcyResidualLoss
    a = torch.from_numpy(R.threshold(R.neumann_field(4, s, seed=77 + s), 12.0, 3.0).astype(np.float32)).to(DEV)
    u, res, _ = ops.darcy2d_solve(a, torch.ones(s, s, device=DEV), iterations=24)
    loss = DarcyResidualLoss(reduction=False)
    true, zero = loss(u, None, a).cpu(), loss(torch.zeros_like(u), None, a).cpu()
    l2 = DarcyResidualLoss(norm="l2", reduction=False)(u, None, a).cpu()
    print(s, "dual", true.tolist(), "p = 0", zero.tolist(), "l2", l2.tolist(), "the solver's own residual", res.cpu().tolist())
    assert bool(torch.isfinite(true).all()) and bool((true < 1e-4 * zero).all())
    assert torch.allclose(l2, res.cpu(), rtol=1e-3, atol=1e-7)                  # the L2 form is the solver's true residual


def test_op_refuses_a_bad_grid_on_the_device(gpu_device):
    from rpde import ops
    z = torch.ones(2, 12, 16, device=DEV)
    with pytest.raises(ValueError, match="8 .. 512"):
        ops.darcy2d_residual(z, z, _tables(16, "dual"))
    z = torch.ones(2, 20, 20, device=DEV)
    with pytest.raises(ValueError, match="tables"):
        ops.darcy2d_residual(z, z, _tables(16, "dual"))


def _sum_loss():
    from utils.loss import DarcyResidualLoss, RelativeL2Loss, SumLoss
    return SumLoss([(1.0, RelativeL2Loss()), (0.1, DarcyResidualLoss())])


def _coefficients(n, s, seed):
    g = torch.from_numpy(R.neumann_field(n, s, seed=seed)).float()
    return torch.where(g >= 0, torch.full_like(g, 12.0), torch.full_like(g, 3.0))[:, None]


def test_graphed_step_matches_eager(gpu_device):
    """a tiny FNO2d trained on data + residual: three eager steps against three replays of
    rpde.graph.GraphedTrainStep(loss_takes_input=True), after warm(); the pattern and bounds of
    tests/test_gpu_ns_residual.py::test_graphed_step_matches_eager"""
    from models.fno import FNO2d
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    torch.manual_seed(3)
    m_e = FNO2d(1, 1, modes1=4, modes2=4, width=8, n_blocks=2).to(gpu_device).train()
    m_g = copy.deepcopy(m_e)
    xs = [_coefficients(4, 16, 20 + i).to(gpu_device) for i in range(3)]
    ys = [torch.randn(4, 1, 16, 16, device=gpu_device) * 0.01 for _ in range(3)]
    loss_fn = _sum_loss()
    loss_fn.warm((16, 16), gpu_device)
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
        pe, pg = pe.detach(), pg.detach()
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
    xs = _coefficients(16, 16, 5)
    g = torch.Generator().manual_seed(5)
    data = [(xs[i], torch.randn(1, 16, 16, generator=g) * 0.01) for i in range(16)]
    loader = lambda: torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)   # noqa: E731
    for graph in (False, True):
        m = copy.deepcopy(m0)
        loss_fn = _sum_loss()
        loss_fn.warm((16, 16), gpu_device)
        opt = FlatAdamW(m.parameters(), lr=2e-3, capturable=graph)
        tl, vl = train(m, loader(), loader(), opt, None, epochs=1, device=gpu_device, graph=graph, loss_fn=loss_fn)
        assert len(tl) == 1 and len(vl) == 1 and all(math.isfinite(v) for v in tl + vl)


@pytest.mark.parametrize("use_normalizer", [False, True])
def test_entry_point_residual_on_generated_darcy(gpu_device, tmp_path, capsys, use_normalizer):
    """training.loss=residual trains main_2d on a 16 x 16 Darcy file generated here, with the prediction decoded by the
    loss (use_normalizer false) or by train() (true); the coefficient is decoded by the loss either way, and the
    reported scores stay relative L2"""
    from data_generation import darcy_2d
    from rpde.entry import run
    darcy_2d.main(["--resolution", "16", "--samples", "40", "--batch", "20", "--seed", "3", "--out", os.path.join(tmp_path, "darcy_16.mat")])
    capsys.readouterr()
    common = ["dataset=darcy_flow/darcy_generated", "model=fno_2d/fno_2d", "dataset.dataset_params.filename=darcy_16.mat",
              f"dataset.dataset_params.saved_folder={tmp_path}", "dataset.original_res=16", "model.modes1=4", "model.modes2=4",
              "model.width=8", "model.n_blocks=2", "training.epochs=1", "training.batch_size=8", f"checkpoint_dir={tmp_path}"]
    l2 = run(2, common + ["training.loss=residual", "training.loss_lambda=0.2", f"training.use_normalizer={str(use_normalizer).lower()}"])
    rec = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if '"test_rel_l2"' in ln]
    assert math.isfinite(l2) and l2 > 0 and rec and rec[0]["test_rel_l2"] == l2
    assert math.isfinite(rec[0]["final_train_loss"]) and rec[0]["final_train_loss"] > 0
    # strided samples are refused in words
    with pytest.raises(SystemExit, match="reduced_resolution"):
        run(2, common + ["training.loss=residual", "dataset.dataset_params.reduced_resolution=2"])
