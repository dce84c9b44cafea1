"""The on-device Darcy generator (csrc/darcy.hip, rpde.ops.darcy2d_solve / darcy2d_apply / sep2d,
data_generation/darcy_2d.py, random_fields.GaussianRFNeumann, dataloaders/darcy_loader.py) against the float64
restatement tests/darcy_ref.py.

The bound everywhere is FLOOR_FACTOR = 4 times the restatement's own float32 error on the same inputs (`floor32`, here
7e-8 .. 1.8e-7: close to fp32 representation error), fixed before any device run, not a measured device number.
Measured on the MI355X (device error / floor32 per sample; DESIGN.md 10.7 has the table with the errors):

    (B, s)      12 / 3 (24 iterations)          1 / 0.1 (32 iterations)
    (3, 8)      0.41 0.78 0.80   frozen 11-13   0.86 0.87 0.36   frozen 14-20
    (2, 12)     0.71 0.50        frozen 13      0.66 0.46        frozen 19-20
    (2, 20)     0.31 0.32        frozen 14      0.56 0.47        frozen 21
    (2, 36)     0.28 0.31        frozen 14      0.51 0.47        frozen 21-22
    (2, 64)     0.26 0.27        frozen 16      0.32 0.35        frozen 25
    (1, 100)    0.26             frozen 15      0.43             frozen 24
    (1, 128)    0.27             frozen 16      0.43             frozen 25

device errors 2.3e-8 .. 1.6e-7; every frozen_at equals the float32 restatement's.  The ratios are below 1 because the
device carries the iterate as a two-float sum and the restatement, as the bound's definition asks, a
plain float32 one.  Freeze / independence batch at s = 20: frozen_at [2, 13, 2, 14], errors 0.79, 0.30, 0.66, 0.33 of
floor32, batch against B = 1 bit-equal.  Reported against float64-recomputed residual: 6.386e-6 / 6.383e-6 and
7.084e-6 / 7.084e-6 (24 iterations), 0.4893 / 0.4893 (3 iterations).  Apply 0.81 .. 1.00 of floor32, symmetry defect at
most 0.19 eps |Ap| |q| (bound 64); closed form 1.31; u(4 a) 4 against u(a): equal bits; sep2d 1.00 and 1.00 at s = 12,
100; cosine-series field 0.96.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import darcy_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _dev(x, gpu_device):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(gpu_device)


def _solve(ref, gpu_device, a=None):
    from rpde import ops
    a = ref["a"] if a is None else a
    return ops.darcy2d_solve(_dev(a, gpu_device), _dev(ref["f"], gpu_device), ref["iterations"], R.TOL)


# ---- 1. solver parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
@pytest.mark.parametrize("contrast", list(R.CONTRASTS))
def test_solver_matches_float64(gpu_device, contrast, case):
    ref = R.parity_reference(case, contrast)
    B, s = case
    # conditions on the inputs, from the restatement alone: the coefficient's structure matters, and the float32
    # restatement converges within the budget
    assert min(ref["gap"]) >= 0.2, ref["gap"]
    assert int(ref["frozen32"].max()) <= ref["within"], ref["frozen32"]
    u, rel_res, frozen_at = _solve(ref, gpu_device)
    assert tuple(u.shape) == (B, s, s) and u.dtype == torch.float32 and u.is_contiguous()
    assert tuple(rel_res.shape) == (B,) and tuple(frozen_at.shape) == (B,) and frozen_at.dtype == torch.int32
    assert bool(torch.isfinite(u).all())
    errs = [R.rel(u[b], ref["u64"][b]) for b in range(B)]
    print(f"[darcy parity] {contrast} {R.case_id(case)}: device rel-L2 {['%.2e' % e for e in errs]}, floor32 "
          f"{['%.2e' % v for v in ref['floor32']]}, ratio {['%.2f' % (e / v) for e, v in zip(errs, ref['floor32'])]}, "
          f"frozen_at {frozen_at.tolist()} (float32 restatement {ref['frozen32'].tolist()}), "
          f"rel_residual {['%.1e' % v for v in rel_res.tolist()]}")
    for b in range(B):
        assert errs[b] <= R.FLOOR_FACTOR * ref["floor32"][b], (b, errs[b], ref["floor32"][b])
    assert int(frozen_at.max()) < ref["iterations"], frozen_at.tolist()


# ---- 2. freeze and independence --------------------------------------------------------------------------------------
def test_freeze_and_independence(gpu_device):
    from rpde import ops
    s, iters = 20, 24
    th = R.threshold(R.neumann_field(2, s, seed=77), 12.0, 3.0)
    a = np.stack([np.ones((s, s)), th[0], np.full((s, s), 7.0), th[1]]).astype(np.float32)
    f = np.ones((s, s), dtype=np.float32)
    u64 = R.direct(a, f)
    u32, frozen32 = R.pcg(a, f, iters, R.TOL, np.float32)
    floor32 = [R.rel(u32[b], u64[b]) for b in range(4)]
    da, df = _dev(a, gpu_device), _dev(f, gpu_device)
    u, rel_res, frozen_at = ops.darcy2d_solve(da, df, iters, R.TOL)
    fz = frozen_at.tolist()
    errs = [R.rel(u[b], u64[b]) for b in range(4)]
    print(f"[darcy freeze] frozen_at {fz} (restatement {frozen32.tolist()}), device rel-L2 {['%.2e' % e for e in errs]}, "
          f"floor32 {['%.2e' % v for v in floor32]}")
    assert fz[0] <= 2 and fz[2] <= 2, fz                       # the preconditioner is the inverse up to the constant
    assert 2 < fz[1] < iters and 2 < fz[3] < iters, fz         # ... beside samples that keep iterating
    assert bool(torch.isfinite(u).all())
    for b in range(4):
        assert errs[b] <= R.FLOOR_FACTOR * floor32[b], (b, errs[b], floor32[b])
    for b in range(4):                                         # a sample does not see the batch around it
        alone, _, fa = ops.darcy2d_solve(da[b:b + 1].contiguous(), df, iters, R.TOL)
        d = R.rel(alone[0], u[b].double().cpu().numpy())
        print(f"[darcy freeze] sample {b}: batch vs alone {d:.2e} ({d / floor32[b]:.2f} floor32), frozen_at {fa.tolist()}")
        assert d <= 2 * floor32[b], (b, d, floor32[b])
    u2, rel2, fz2 = ops.darcy2d_solve(da, df, iters, R.TOL)     # identical calls, identical bits
    assert torch.equal(u, u2) and torch.equal(rel_res, rel2) and torch.equal(frozen_at, fz2)
    # batched right-hand sides: the same f repeated gives the same bits as the shared one
    u3, _, fz3 = ops.darcy2d_solve(da, df.expand(4, s, s).contiguous(), iters, R.TOL)
    assert torch.equal(u, u3) and torch.equal(frozen_at, fz3)


# ---- 3. the reported residual and freeze iteration are true -------------------------------------------------------------
@pytest.mark.parametrize("iterations", [3, 24])
def test_reported_residual_is_the_true_one(gpu_device, iterations):
    from rpde import ops
    ref = R.parity_reference((2, 36), "12_3")
    u, rel_res, frozen_at = ops.darcy2d_solve(_dev(ref["a"], gpu_device), _dev(ref["f"], gpu_device), iterations, R.TOL)
    a64, f64 = ref["a"].astype(np.float64), np.broadcast_to(ref["f"].astype(np.float64), ref["a"].shape)
    res = f64 - R.apply(a64, u.double().cpu().numpy())
    true = np.sqrt((res ** 2).sum(axis=(1, 2)) / (f64 ** 2).sum(axis=(1, 2)))
    print(f"[darcy residual] iterations {iterations}: reported {rel_res.tolist()}, float64 {true.tolist()}, "
          f"frozen_at {frozen_at.tolist()}")
    for b in range(2):
        got = float(rel_res[b])
        assert (0.5 * true[b] <= got <= 2 * true[b]) or (got < 1e-6 and true[b] < 1e-6), (b, got, true[b])
    if iterations == 3:                                         # not converged: `iterations` means "not frozen"
        assert frozen_at.tolist() == [3, 3] and float(rel_res.min()) > 1e-4
    else:
        assert int(frozen_at.max()) < iterations, frozen_at.tolist()


# ---- 4. the apply ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 8), (2, 12), (2, 36), (1, 100), (1, 128)], ids=R.case_id)
def test_apply_matches_float64_and_is_symmetric(gpu_device, case):
    from rpde import ops
    B, s = case
    rng = np.random.default_rng(200 + s)
    a = R.threshold(R.neumann_field(B, s, seed=300 + s), 12.0, 3.0).astype(np.float32)
    a[0] = np.exp(rng.standard_normal((s, s))).astype(np.float32)                       # one smooth-less, many-valued a
    smooth = R.neumann_field(B, s, seed=400 + s).astype(np.float32)
    rough = rng.standard_normal((B, s, s)).astype(np.float32)
    da = _dev(a, gpu_device)
    for name, p in (("smooth", smooth), ("rough", rough)):
        want = R.apply(a.astype(np.float64), p.astype(np.float64))
        floor32 = R.rel(R.apply(a, p), want)
        got = ops.darcy2d_apply(da, _dev(p, gpu_device))
        err = R.rel(got, want)
        print(f"[darcy apply] {R.case_id(case)} {name}: device rel-L2 {err:.2e}, floor32 {floor32:.2e}, ratio {err / floor32:.2f}")
        assert err <= R.FLOOR_FACTOR * floor32, (name, err, floor32)
    q = rng.standard_normal((B, s, s)).astype(np.float32)
    Ap = ops.darcy2d_apply(da, _dev(rough, gpu_device)).double().cpu().numpy()
    Aq = ops.darcy2d_apply(da, _dev(q, gpu_device)).double().cpu().numpy()
    for b in range(B):
        lhs, rhs = float((Ap[b] * q[b]).sum()), float((rough[b].astype(np.float64) * Aq[b]).sum())
        scale = np.linalg.norm(Ap[b]) * np.linalg.norm(q[b])
        print(f"[darcy apply] {R.case_id(case)} sample {b}: |<Ap,q> - <p,Aq>| / (eps |Ap| |q|) = {abs(lhs - rhs) / (EPS * scale):.2f}")
        assert abs(lhs - rhs) <= 64 * EPS * scale, (b, lhs, rhs)


# ---- 5. closed forms -------------------------------------------------------------------------------------------------
def test_closed_forms(gpu_device):
    from rpde import ops
    s, c, k1, k2 = 20, 2.5, 1, 2
    S, lam = R.tables(s)
    f64 = np.outer(S[k1], S[k2])[None]                           # one discrete eigenvector of the constant operator
    exact = f64 / (c * (lam[k1] + lam[k2]))
    a = np.full((1, s, s), c)
    assert R.rel(R.direct(a, f64), exact) < 1e-12
    u32, _ = R.pcg(a, f64, 24, R.TOL, np.float32)
    floor32 = R.rel(u32, exact)
    u, rel_res, frozen_at = ops.darcy2d_solve(_dev(a, gpu_device), _dev(f64, gpu_device), 24, R.TOL)
    err = R.rel(u, exact)
    print(f"[darcy closed form] device rel-L2 {err:.2e}, floor32 {floor32:.2e}, ratio {err / floor32:.2f}, frozen_at {frozen_at.tolist()}")
    assert err <= R.FLOOR_FACTOR * floor32, (err, floor32)
    # scaling a by 4 scales u by 1/4
    ref = R.parity_reference((2, 20), "12_3")
    u1, _, _ = _solve(ref, gpu_device)
    u4, _, _ = _solve(ref, gpu_device, a=4.0 * ref["a"])
    d = R.rel(4.0 * u4.double().cpu().numpy(), u1.double().cpu().numpy())
    print(f"[darcy closed form] u(4 a) 4 vs u(a): {d / EPS:.2f} eps")
    assert d <= 8 * EPS, d


# ---- 6. sep2d and the cosine-series field ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 12), (2, 100)], ids=R.case_id)
def test_sep2d_matches_float64(gpu_device, case):
    from rpde import ops
    B, s = case
    rng = np.random.default_rng(s)
    x, L, Rt = (rng.standard_normal(sh).astype(np.float32) for sh in ((B, s, s), (s, s), (s, s)))
    want = L.astype(np.float64) @ x.astype(np.float64) @ Rt.astype(np.float64).T
    floor32 = R.rel(L @ x @ Rt.T, want)
    got = ops.sep2d(_dev(x, gpu_device), _dev(L, gpu_device), _dev(Rt, gpu_device))
    err = R.rel(got, want)
    print(f"[sep2d] {R.case_id(case)}: device rel-L2 {err:.2e}, floor32 {floor32:.2e}, ratio {err / floor32:.2f}")
    assert tuple(got.shape) == (B, s, s) and err <= R.FLOOR_FACTOR * floor32, (err, floor32)


def test_neumann_field(gpu_device):
    from data_generation.random_fields import GaussianRFNeumann
    s, n = 20, 6
    grf = GaussianRFNeumann(s, alpha=2, tau=3, device=gpu_device)
    noise = torch.randn(n, s, s, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(5))
    g = grf.sample(n, noise=noise)
    want = R.neumann_field(n, s, seed=None, noise=noise.double().cpu().numpy())
    coef32 = R.neumann_coef(s).astype(np.float32)
    C32 = R.cosine_table(s).astype(np.float32)
    floor32 = R.rel(C32 @ (coef32 * noise.cpu().numpy()) @ C32.T, want)
    err = R.rel(g, want)
    print(f"[neumann field] device rel-L2 {err:.2e}, floor32 {floor32:.2e}, ratio {err / floor32:.2f}")
    assert err <= R.FLOOR_FACTOR * floor32, (err, floor32)
    # the mean mode's coefficient is 0: the sample mean is what the products round
    rms = float(g.double().pow(2).mean().sqrt())
    assert float(g.double().mean(dim=(1, 2)).abs().max()) <= 64 * EPS * rms
    # equal seeds, equal fields
    g1 = grf.sample(3, generator=torch.Generator(device=gpu_device).manual_seed(11))
    g2 = grf.sample(3, generator=torch.Generator(device=gpu_device).manual_seed(11))
    g3 = grf.sample(3, generator=torch.Generator(device=gpu_device).manual_seed(12))
    assert torch.equal(g1, g2) and not torch.equal(g1, g3)
    # zero flux: the same cosine series evaluated (float64) at the centres beyond the walls x = 1 and y = 1 is the
    # device's sample mirrored.  Bound: two length-s fp32 products and once-rounded tables lose at most a few s eps of
    # the largest value per entry; 64 s eps leaves a margin and is four orders below a wrong mirror's O(1)
    i = (np.arange(2 * s) + 0.5)[:, None]
    C2 = np.cos(np.pi * np.arange(s)[None, :] * i / s)
    ext = C2 @ (R.neumann_coef(s) * noise.double().cpu().numpy()) @ C2.T
    gd = g.double().cpu().numpy()
    assert np.abs(ext[:, s:, :s] - gd[:, ::-1, :]).max() <= 64 * EPS * np.abs(gd).max() * s
    assert np.abs(ext[:, :s, s:] - gd[:, :, ::-1]).max() <= 64 * EPS * np.abs(gd).max() * s
    with pytest.raises(ValueError):
        grf.sample(2, noise=noise)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_device_usable(gpu_device):
    from rpde import _lib, ops
    ok = torch.ones(1, 16, 16, device=gpu_device)
    for s in (10, 6, 516):
        bad = torch.ones(1, s, s, device=gpu_device)
        with pytest.raises(ValueError):
            ops.darcy2d_solve(bad, bad[0])
        with pytest.raises(ValueError):
            ops.darcy2d_apply(bad, bad)
        with pytest.raises(ValueError):
            ops.sep2d(bad, bad[0], bad[0])
    with pytest.raises(ValueError):
        ops.darcy2d_solve(ok, torch.ones(16, 12, device=gpu_device))                   # wrong f shape
    with pytest.raises(ValueError):
        ops.darcy2d_solve(ok, torch.ones(2, 16, 16, device=gpu_device))
    with pytest.raises(ValueError):
        ops.darcy2d_solve(torch.ones(1, 16, 12, device=gpu_device), ok[0])
    for v in (0.0, -1.0, float("nan"), float("inf")):
        a = ok.clone()
        a[0, 3, 5] = v
        with pytest.raises(ValueError):
            ops.darcy2d_solve(a, ok[0])
    with pytest.raises(ValueError):
        ops.darcy2d_solve(ok, ok[0], iterations=-1)
    with pytest.raises(_lib.RpdeError):
        ops.darcy2d_solve(ok.cpu(), ok[0].cpu())                                         # no CPU fallback
    # a short workspace, through the C ABI
    lib = _lib.load()
    S, il = (t.to(gpu_device) for t in ops.darcy2d_tables(16))
    u, rel = torch.empty_like(ok), torch.empty(1, device=gpu_device)
    fz = torch.empty(1, dtype=torch.int32, device=gpu_device)
    need = lib.rpde_darcy2d_ws_bytes(1, 16)
    ws = _lib.workspace(need, gpu_device)
    args = (ok.data_ptr(), ok.data_ptr(), 0, S.data_ptr(), il.data_ptr(), u.data_ptr(), rel.data_ptr(), fz.data_ptr(), 1, 16, 4, 1e-6)
    assert lib.rpde_darcy2d_solve(*args, ws.data_ptr(), need - 256, _lib.stream_ptr()) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.rpde_last_error()
    assert lib.rpde_sep2d(ok.data_ptr(), S.data_ptr(), S.data_ptr(), u.data_ptr(), 1, 16, ws.data_ptr(), 512, _lib.stream_ptr()) \
        == _lib.ERR_WORKSPACE
    assert lib.rpde_darcy2d_solve(*args, ws.data_ptr() + 16, need, _lib.stream_ptr()) == _lib.ERR_ARG
    # ... and the device still works
    u, rel, fz = ops.darcy2d_solve(ok, ok[0])
    torch.cuda.synchronize()
    assert float(rel[0]) < 1e-5 and int(fz[0]) <= 2


# ---- 8. end to end -----------------------------------------------------------------------------------------------------
def test_script_loader_and_training_end_to_end(gpu_device, tmp_path, capsys):
    from scipy.io import loadmat
    from data_generation import darcy_2d
    from dataloaders.darcy_loader import darcy_dataset
    from rpde import entry
    out = os.path.join(tmp_path, "darcy_32.mat")
    darcy_2d.main(["--resolution", "32", "--samples", "40", "--batch", "20", "--seed", "3", "--out", out])
    blob = loadmat(out)
    coeff, sol = blob["coeff"], blob["sol"]
    assert coeff.shape == (40, 32, 32) and sol.shape == (40, 32, 32) and coeff.dtype == np.float32
    assert set(np.unique(coeff).tolist()) == {3.0, 12.0} and np.isfinite(sol).all() and (sol > 0).all()
    assert not np.array_equal(coeff[:20], coeff[20:])                                  # the generator advances
    # the file's pairs solve the discrete problem (float64, from the file alone)
    res = 1.0 - R.apply(coeff[:4].astype(np.float64), sol[:4].astype(np.float64))
    assert float(np.sqrt((res ** 2).mean())) < 1e-5
    tr, va, te, xn, yn = darcy_dataset("darcy_32.mat", str(tmp_path))
    assert (len(tr), len(va), len(te)) == (32, 4, 4) and tuple(tr[0][0].shape) == (1, 32, 32)
    # the script refuses to write an unconverged archive
    bad = os.path.join(tmp_path, "bad.npz")
    with pytest.raises(RuntimeError):
        darcy_2d.main(["--resolution", "32", "--samples", "4", "--batch", "4", "--iterations", "2", "--out", bad])
    assert not os.path.exists(bad)
    capsys.readouterr()
    entry.run(2, ["dataset=darcy_flow/darcy_generated", "model=fno_2d/fno_2d", "training.epochs=2", "training.batch_size=8",
                  "dataset.dataset_params.filename=darcy_32.mat", f"dataset.dataset_params.saved_folder={tmp_path}",
                  "dataset.original_res=32", f"checkpoint_dir={tmp_path}"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    scores = next(d for d in lines if "test_rel_l2" in d)
    sweep = next(d for d in lines if "resolution_rel_l2" in d)
    assert all(np.isfinite(scores[k]) for k in ("final_train_loss", "final_val_loss", "test_rel_l2")), scores
    assert sweep["evaluation_type"] == "naive_downsample" and "32" in sweep["resolution_rel_l2"]
    assert all(np.isfinite(v) for v in sweep["resolution_rel_l2"].values()), sweep
