"""The on-device active-scalar Navier-Stokes generator (csrc/ns_solver.hip, rpde.ops.nsc2d_solve / nsc2d_fields,
data_generation/active_scalar_2d.py) against the float64 restatement tests/nsc_solver_ref.py, and the active-matter data
path from the generator's files to a training run.

The bound everywhere is FLOOR_FACTOR = 4 times the restatement's own float32 error on the same inputs, per channel
(c, q, v, w) and snapshot: the project's standing margin for its generators, not a measured device number.  Measured on
the MI355X (device error / float32 floor) -- see DESIGN.md "Active-scalar NS generator"."""
import math

import numpy as np
import pytest
import torch

from tests import ns_solver_ref as R
from tests import nsc_solver_ref as C

pytestmark = pytest.mark.gpu


def _dev(t, gpu_device):
    return t.to(torch.float32).to(gpu_device)


def _solve(gpu_device, w0, c0, f, visc=C.VISC, kappa=C.KAPPA, beta=C.BETA, T=C.T_FINAL, dt=C.DT, rec=C.RECORD_STEPS):
    from data_generation.active_scalar_2d import active_scalar_2d
    return active_scalar_2d(_dev(w0, gpu_device), _dev(c0, gpu_device), _dev(f, gpu_device), visc, kappa, beta, T, dt, rec)


def _check(tag, fields, vort, f64, v64, floor):
    """every channel and snapshot within FLOOR_FACTOR x floor; prints the ratios first"""
    errs = C.floors(fields, vort, f64, v64)
    for ch, name in enumerate(C.CHANNELS):
        print(f"[{tag}] {name}: device rel-L2 {['%.2e' % e for e in errs[ch]]}, floor32 {['%.2e' % v for v in floor[ch]]}, "
              f"ratio {['%.2f' % (e / v) for e, v in zip(errs[ch], floor[ch])]}")
    for ch in range(4):
        for n, (e, fl) in enumerate(zip(errs[ch], floor[ch])):
            assert e <= C.FLOOR_FACTOR * fl, (tag, C.CHANNELS[ch], n, e, fl)


# ---- 1. solver parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_solver_matches_float64(gpu_device, case):
    ref = C.parity_reference(case)
    # conditions on the inputs: without buoyancy, and without advection, the answer is visibly different
    assert ref["buoyancy_share"] >= 0.1 and ref["advection_share"] >= 0.1, (ref["buoyancy_share"], ref["advection_share"])
    fields, vort, sol_t = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"])
    B, M, N = case
    assert tuple(fields.shape) == (B, C.RECORD_STEPS, 3, M, N) and tuple(vort.shape) == (B, C.RECORD_STEPS, M, N)
    assert fields.dtype == vort.dtype == torch.float32 and fields.is_contiguous() and vort.is_contiguous()
    assert torch.equal(sol_t.cpu(), ref["t64"].float())
    _check(f"nsc parity {C.case_id(case)}", fields, vort, ref["fields64"], ref["vort64"], ref["floor32"])


# ---- 2. the closed form ----------------------------------------------------------------------------------------------
def test_closed_form(gpu_device):
    """functions of theta = 2 pi (3x + 2y) advect nothing: the coefficients of e^{i theta} obey a 2 x 2 recurrence.
    Independent of the restatement's nonlinear code (the restatement only supplies the float32 floor)."""
    w0, c0, f, theta, par = C.closed_form_inputs()
    w, c = C.closed_form(theta, **par)
    args = (par["visc"], par["kappa"], par["beta"], par["steps"] * par["dt"], par["dt"], 1)
    f32, v32, _ = C.solve(w0.float(), c0.float(), f.float(), *args, dtype=torch.float32)
    fields, vort, _ = _solve(gpu_device, w0, c0, f, *args)
    for name, got, flo, want in (("w", vort[0, 0], v32[0, 0], w), ("c", fields[0, 0, 0], f32[0, 0, 0], c)):
        err, floor32 = C.rel(got, want), C.rel(flo, want)
        print(f"[nsc closed form] {name}: device rel-L2 {err:.2e}, floor32 {floor32:.2e}, ratio {err / floor32:.2f}")
        assert err <= C.FLOOR_FACTOR * floor32, (name, err, floor32)


# ---- 3. forcing shapes -----------------------------------------------------------------------------------------------
def test_forcing_shapes(gpu_device):
    B, M, N = case = (2, 16, 24)
    ref = C.parity_reference(case)
    one = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"])
    rep = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"].expand(B, M, N))
    assert torch.equal(one[0], rep[0]) and torch.equal(one[1], rep[1])
    # a forcing of its own for every sample
    scale = torch.tensor([1.0, -2.5], dtype=torch.float64).view(B, 1, 1)
    fb = scale * ref["f"] + 0.05 * R.forcing(M, N).roll(3, dims=1)
    args = (C.VISC, C.KAPPA, C.BETA, C.T_FINAL, C.DT, C.RECORD_STEPS)
    f64, v64, _ = C.solve(ref["w0"], ref["c0"], fb, *args)
    f32, v32, _ = C.solve(ref["w0"].float(), ref["c0"].float(), fb.float(), *args, dtype=torch.float32)
    assert C.rel(v64[:, -1], ref["vort64"][:, -1]) > 1e-2             # the forcings do differ
    fields, vort, _ = _solve(gpu_device, ref["w0"], ref["c0"], fb)
    _check("nsc batch forcing", fields, vort, f64, v64, C.floors(f32, v32, f64, v64))


# ---- 4. beta = 0 is the vorticity solver -----------------------------------------------------------------------------
def test_beta_zero_matches_the_vorticity_solver(gpu_device):
    """without buoyancy the vorticity does not see the scalar: it is ops.ns2d_solve's, up to the rounding of two launch
    shapes (not bit for bit: the transforms see 6 B and 4 B images).  Both against float64 and against each other within
    FLOOR_FACTOR x the NS restatement's float32 floor."""
    from rpde import ops
    case = (2, 32, 48)
    ns, ref = R.parity_reference(case), C.parity_reference(case)
    assert torch.equal(ns["w0"], ref["w0"]) and (C.VISC, C.DT, C.T_FINAL, C.RECORD_STEPS) == (R.VISC, R.DT, R.T_FINAL, R.RECORD_STEPS)
    _, vort, _ = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"], beta=0.0)
    record_time = R.STEPS // R.RECORD_STEPS
    plain = ops.ns2d_solve(_dev(ns["w0"], gpu_device), _dev(ns["f"], gpu_device), R.VISC, R.DT, R.STEPS, record_time)
    for n in range(C.RECORD_STEPS):
        e64, gap, fl = R.rel(vort[:, n], ns["sol64"][..., n]), R.rel(vort[:, n], plain[..., n]), ns["floor32"][n]
        print(f"[nsc beta 0] snapshot {n}: against float64 {e64:.2e}, against ns2d_solve {gap:.2e}, floor32 {fl:.2e}, "
              f"ratios {e64 / fl:.2f} {gap / fl:.2f}")
        assert e64 <= C.FLOOR_FACTOR * fl and gap <= C.FLOOR_FACTOR * fl, (n, e64, gap, fl)
    assert R.rel(vort[:, -1], ref["vort64"][:, -1]) > 0.1              # and beta = 5 is another flow


# ---- 5. repeatability and record bookkeeping -------------------------------------------------------------------------
def test_identical_calls_give_identical_bits(gpu_device):
    ref = C.parity_reference((2, 32, 48))
    a = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"], T=0.04, rec=2)            # 20 steps
    b = _solve(gpu_device, ref["w0"], ref["c0"], ref["f"], T=0.04, rec=2)
    assert tuple(a[0].shape) == (2, 2, 3, 32, 48) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert R.rel(a[1][:, 1], ref["w0"]) > 1e-3 and R.rel(a[0][:, 1, 0], ref["c0"]) > 1e-3      # something was computed


def test_record_bookkeeping(gpu_device):
    """5 snapshots of 10 steps: each equals, bit for bit, a solve that stops there in one device call -- so k calls of n
    steps are one call of k n steps, through the first-, middle- and last-step variants of the update kernel"""
    from rpde import ops
    B, M, N, T, dt, rec = 2, 16, 16, 0.05, 1e-3, 5
    w0 = _dev(R.initial_vorticity(B, M, N, seed=21), gpu_device)
    c0 = _dev(C.initial_scalar(B, M, N, seed=22), gpu_device)
    f = _dev(R.forcing(M, N), gpu_device)
    fields, vort, sol_t = _solve(gpu_device, w0, c0, f, T=T, dt=dt, rec=rec)
    assert tuple(fields.shape) == (B, 5, 3, 16, 16) and tuple(vort.shape) == (B, 5, 16, 16) and tuple(sol_t.shape) == (5,)
    steps, record_time, times = R.schedule(T, dt, rec)
    assert (steps, record_time) == (50, 10)
    assert torch.equal(sol_t.cpu(), torch.tensor(times, dtype=torch.float64).float())
    assert tuple(ops.nsc2d_solve(w0, c0, f, C.VISC, C.KAPPA, C.BETA, dt, 7, 10)[0].shape) == (B, 0, 3, 16, 16)
    for n in range(rec):
        k = (n + 1) * record_time
        af, av = ops.nsc2d_solve(w0, c0, f, C.VISC, C.KAPPA, C.BETA, dt, k, k)
        assert tuple(af.shape) == (B, 1, 3, 16, 16) and tuple(av.shape) == (B, 1, 16, 16)
        assert torch.equal(af[:, 0], fields[:, n]) and torch.equal(av[:, 0], vort[:, n]), n
    one = ops.nsc2d_solve(w0, c0, f, C.VISC, C.KAPPA, C.BETA, dt, 3, 1)                # single-step calls: first = last
    assert torch.equal(one[0][:, 2], ops.nsc2d_solve(w0, c0, f, C.VISC, C.KAPPA, C.BETA, dt, 3, 3)[0][:, 0])


# ---- 6. the fields call alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 16, 24), (3, 6, 10)], ids=C.case_id)
def test_fields_of_a_state(gpu_device, case):
    from rpde import ops
    B, M, N = case
    w, c = R.initial_vorticity(B, M, N, seed=31), C.initial_scalar(B, M, N, seed=32)
    want = C.fields_of(torch.fft.rfft2(w), torch.fft.rfft2(c), M, N)
    flo = C.fields_of(torch.fft.rfft2(w.float()), torch.fft.rfft2(c.float()), M, N, dtype=torch.float32)
    got = ops.nsc2d_fields(_dev(w, gpu_device), _dev(c, gpu_device))
    assert tuple(got.shape) == (B, 3, M, N) and got.is_contiguous()
    for ch in range(3):
        err, fl = C.rel(got[:, ch], want[:, ch]), C.rel(flo[:, ch], want[:, ch])
        print(f"[nsc fields {C.case_id(case)}] {C.CHANNELS[ch]}: device rel-L2 {err:.2e}, floor32 {fl:.2e}, ratio {err / fl:.2f}")
        assert err <= C.FLOOR_FACTOR * fl, (ch, err, fl)
    assert torch.equal(got, ops.nsc2d_fields(_dev(w, gpu_device), _dev(c, gpu_device)))


# ---- 7. end to end: generate, load at three sizes, train -------------------------------------------------------------
def test_cli_to_training(gpu_device, tmp_path, capsys):
    import json
    from data_generation import active_scalar_2d as gen
    from dataloaders.active_matter_all_markov import MultiFileActiveMatterMarkovDataset, multi_file_active_matter_markov_dataset
    from models.ffno import FFNO2D
    from oracle.reference_path import resize_2d
    from rpde.entry import run
    from tests.resize_ref import FWD_TOL
    from utils.loss import RelativeL2Loss
    from utils.res_utils import downsample
    paths = gen.main(["--resolution", "32", "--samples", "3", "--batch", "2", "--T", "0.07", "--dt", "1e-3", "--record-steps", "7",
                      "--files", "2", "--visc", "1e-3", "--kappa", "2e-3", "--beta", "5", "--out-dir", str(tmp_path)])
    assert [p.split("/")[-1] for p in paths] == [gen.file_name(1e-3, 2e-3, 5.0, i) for i in (0, 1)]
    blobs = []
    for p in paths:
        with np.load(p) as z:
            conc, vel, vort = z["t0_fields/concentration"], z["t1_fields/velocity"], z["t0_fields/vorticity"]
            assert conc.shape == (3, 8, 32, 32) and vel.shape == (3, 8, 32, 32, 2) and vort.shape == (3, 8, 32, 32)
            assert conc.dtype == vel.dtype == np.float32 and np.isfinite(conc).all() and np.isfinite(vel).all()
            assert z["t"].shape == (8,) and z["t"][0] == 0 and abs(float(z["t"][-1]) - 0.07) < 1e-6
            assert abs(float(z["scalars/kappa"]) - 2e-3) < 1e-9 and float(z["scalars/beta"]) == 5.0
            assert not np.array_equal(conc[0, 0], conc[2, 0])                  # the second batch drew new fields
            # frame 0 is the velocity of the vorticity's frame 0
            w0 = torch.from_numpy(vort[:, 0])
            want = C.fields_of(torch.fft.rfft2(w0.double()), torch.fft.rfft2(w0.double()), 32, 32)
            flo = C.fields_of(torch.fft.rfft2(w0), torch.fft.rfft2(w0), 32, 32, dtype=torch.float32)
            for ch in (1, 2):
                err, fl = C.rel(torch.from_numpy(vel[:, 0, :, :, ch - 1]), want[:, ch]), C.rel(flo[:, ch], want[:, ch])
                assert err <= C.FLOOR_FACTOR * fl, (ch, err, fl)
            blobs.append((conc, vel))
    assert not np.array_equal(blobs[0][0], blobs[1][0])
    conc, vel = np.concatenate([b[0] for b in blobs]), np.concatenate([b[1] for b in blobs])
    frames = np.concatenate([conc[:, :, None], np.moveaxis(vel, -1, 2)], axis=2)          # [6, 8, 3, 32, 32]

    same = MultiFileActiveMatterMarkovDataset("active_scalar_*.npz", str(tmp_path), s=32)
    assert len(same) == 6 * 7 and np.array_equal(same.x.numpy(), frames[:, :-1].reshape(-1, 3, 32, 32))
    assert np.array_equal(same.y.numpy(), frames[:, 1:].reshape(-1, 3, 32, 32))
    assert same.file_parameters[4]["beta"] == 5.0 and same.parameter_stats["total_files"] == 2
    down = MultiFileActiveMatterMarkovDataset("active_scalar_*.npz", str(tmp_path), s=16)
    want = downsample(frames[:, :-1].reshape(-1, 1, 32, 32), 16).reshape(-1, 3, 16, 16)
    assert np.allclose(down.x.numpy(), want, rtol=0, atol=1e-6 * np.abs(want).max())
    up = MultiFileActiveMatterMarkovDataset("active_scalar_*.npz", str(tmp_path), s=48)
    want = resize_2d(torch.from_numpy(frames[:, 1:].reshape(-1, 3, 32, 32)).double(), (48, 48))    # float64 irfft2 of the padded spectrum
    err = C.rel(up.y, want)
    with capsys.disabled():
        print(f"[nsc e2e] resize 32 -> 48 against float64: rel {err:.2e}")
    assert tuple(up.y.shape) == (42, 3, 48, 48) and err <= FWD_TOL, err

    train, val, test, min_data, max_data, min_model, max_model = multi_file_active_matter_markov_dataset(
        "active_scalar_*.npz", str(tmp_path), s=32)
    assert (len(train), len(val), len(test)) == (33, 4, 5) and min_data < 0 < max_data and min_model < max_model
    xb = torch.stack([train[i][0] for i in range(8)]).to(gpu_device)
    yb = torch.stack([train[i][1] for i in range(8)]).to(gpu_device)
    assert tuple(xb.shape) == (8, 3, 32, 32)
    torch.manual_seed(0)
    model = FFNO2D(in_channels=3, out_channels=3, width=64, n_layers=2, n_modes=12, factor=4, ff_weight_norm=True,
                   n_ff_layers=3, layer_norm=True, dropout=0.0).to(gpu_device).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    loss = RelativeL2Loss()(model(xb), yb)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach()))

    capsys.readouterr()
    l2 = run(2, ["model=ffno_2d/ffno_2d_3ch", "dataset=ns/ns_active_generated", f"dataset.dataset_params.saved_folder={tmp_path}",
                 "dataset.dataset_params.s=32", "dataset.original_res=32", "model.width=16", "model.n_layers=2", "model.n_modes=8",
                 "model.factor=2", "training.epochs=1", "training.batch_size=8", f"checkpoint_dir={tmp_path}"])
    out = capsys.readouterr().out
    assert math.isfinite(l2) and l2 > 0
    rec = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and "resolution_rel_l2" in ln]
    assert rec and sorted(rec[0]["resolution_rel_l2"]) == ["32"] and math.isfinite(rec[0]["resolution_rel_l2"]["32"])
    assert run.last["test_rel_l2"] == l2 and sorted(run.last["resolution_rel_l2"]) == [32]
