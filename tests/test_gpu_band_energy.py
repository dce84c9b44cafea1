"""GPU: the per-sample band energies (csrc/band_energy.hip rpde_band_energy_* -> rpde.ops.band_energy), the two losses on
them (utils.loss.BandRelativeL2Loss, SpectrumMatchingLoss) and the rollout statistic, against the float64 restatement
of tests/band_energy_ref.py.

Bound of every compared quantity: max(project budget, 4 x floor32) with the budgets of tests/test_gpu_spectral_loss.py
(1e-5 on loss-like quantities, 2e-5 on gradients, rel-L2) and floor32 the same restatement in float32 on the same
inputs, which must itself stay within the budget.  The parity test prints both numbers per case and quantity."""
import copy
import functools
import json
import math

import pytest
import torch

from tests import band_energy_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bands_arg(case):
    """what the public interfaces take as `bands` / num_bands for a case"""
    B, C, M, N, (kind, nb) = case
    if kind == "one":
        return torch.zeros((N // 2 + 1,) if M == 1 else (M, N // 2 + 1), dtype=torch.int64), None
    return kind, nb


@functools.lru_cache(maxsize=None)
def _reference(case):
    """float64 quantities and the float32 floor of each: computed once per case"""
    r64, r32 = R.reference(case), R.reference(case, torch.float32)
    floor = {k: R.rel_l2(r32[k], r64[k]) for k in R.QUANTITIES}
    floor["strong"] = R.strong_band_error(r32["E"], r64["E"])
    return r64, floor


@functools.lru_cache(maxsize=None)
def _device(case):
    """the same quantities through the public interfaces, on the device"""
    from rpde import ops
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss
    B, C, M, N, _ = case
    dims = R.dims_of(case)
    bands, nb = _bands_arg(case)
    x, y = R.make_inputs(B, C, M, N)
    yd = y.to(DEV)
    T = ops.resolve_bands(bands if nb is None else (bands, nb), x.shape[2:], DEV)
    gE = R.upstream(B, T.J).to(DEV)
    out = {}
    for key, gkey, other in (("E", "gE_grad", None), ("E_diff", "E_diff_grad", yd)):
        xd = x.to(DEV).requires_grad_(True)
        E = ops.band_energy(xd, T, dims, y=other)
        (E * gE).sum().backward()
        out[key], out[gkey] = E.detach().cpu(), xd.grad.cpu()
    for key, cls in (("band", BandRelativeL2Loss), ("spectrum", SpectrumMatchingLoss)):
        xd = x.to(DEV).requires_grad_(True)
        out[key] = cls(dims, bands, nb, reduction=False)(xd, yd).detach().cpu()
        cls(dims, bands, nb)(xd, yd).backward()
        out[key + "_grad"] = xd.grad.cpu()
    return out


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_parity_with_the_float64_restatement(gpu_device, case):
    r64, floor = _reference(case)
    got = _device(case)
    errs = {k: R.rel_l2(got[k], r64[k]) for k in R.QUANTITIES}
    errs["strong"] = R.strong_band_error(got["E"], r64["E"])
    for k, e in errs.items():
        print(f"{R.case_id(case)}: {k:14s} device vs float64 {e:.2e}   floor32 {floor[k]:.2e}   "
              f"bound {max(R.budget(k), R.FLOOR_FACTOR * floor[k]):.1e}")
    assert got["E"].dtype == torch.float32 and got["E"].shape == r64["E"].shape
    assert got["band"].shape == (case[0],) and got["band_grad"].shape == r64["band_grad"].shape
    for k, e in errs.items():
        assert e <= R.bound(R.budget(k), floor[k]), (k, e, floor[k])


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_comparison_sees_a_wrong_answer(gpu_device, case):
    """Restatements with multiplicity 2 at DC / Nyquist, and (2-D octave) with an unsigned ky in the band table, miss the
    device by at least 1e-2 on a loss-like quantity and on a gradient.  Both losses are ratios band by band and so blind
    to a factor on a WHOLE band: in 1-D octave bands DC and Nyquist are bands of their own.  So the multiplicity shows in
    E and its gradient on every case, and in the spectrum loss where the kx = 0 column shares its bands (2-D); the
    unsigned ky moves entries between bands and shows in both losses."""
    B, C, M, N, (kind, nb) = case
    got = _device(case)
    wrong = R.reference(case, edge_weight=2.0)
    keys = ("E", "gE_grad") + (("spectrum", "spectrum_grad") if M > 1 else ())
    miss = {k: R.rel_l2(wrong[k], got[k]) for k in keys}
    print(f"{R.case_id(case)}: multiplicity 2 on DC and Nyquist misses the device by", {k: round(v, 3) for k, v in miss.items()})
    assert all(v >= 1e-2 for v in miss.values()), miss
    if M > 1 and kind == "octave":
        wrong = R.reference(case, unsigned_ky=True)
        miss = {k: R.rel_l2(wrong[k], got[k]) for k in ("band", "band_grad", "spectrum", "spectrum_grad")}
        print(f"{R.case_id(case)}: unsigned ky misses the device by", {k: round(v, 3) for k, v in miss.items()})
        assert all(v >= 1e-2 for v in miss.values()), miss


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4][0] in ("octave", "one")], ids=R.case_id)
def test_parseval_on_the_device(gpu_device, case):
    """every entry has a band: the band energies of a sample add up to sum x^2"""
    B, C, M, N, _ = case
    x, _ = R.make_inputs(B, C, M, N)
    want = (x.double() ** 2).flatten(1).sum(1)
    e = R.rel_l2(_device(case)["E"].double().sum(1), want)
    print(f"{R.case_id(case)}: sum_j E_j vs sum x^2 {e:.2e}")
    assert e <= R.bound(R.LOSS_TOL, _reference(case)[1]["E"])


@pytest.mark.parametrize("shape", [(3, 2, 48), (2, 1, 16, 12), (2, 2, 9, 15)], ids=str)
def test_one_band_zero_floor_is_relative_l2(gpu_device, shape):
    """one band that owns every entry, band_floor = 0: RelativeL2Loss -- the device's own, value and gradient"""
    from utils.loss import BandRelativeL2Loss, RelativeL2Loss
    dims = len(shape) - 2
    M, N = (1, shape[2]) if dims == 1 else shape[2:]
    x, y = R.make_inputs(shape[0], shape[1], M, N)
    one = torch.zeros((N // 2 + 1,) if dims == 1 else (M, N // 2 + 1), dtype=torch.int32)
    res = []
    for fn in (BandRelativeL2Loss(dims, one, band_floor=0.0, reduction=False), RelativeL2Loss(reduction=False)):
        xd = x.to(DEV).requires_grad_(True)
        r = fn(xd, y.to(DEV))
        r.mean().backward()
        res.append((r.detach().cpu(), xd.grad.cpu()))
    e = (R.rel_l2(res[0][0], res[1][0]), R.rel_l2(res[0][1], res[1][1]))
    print(f"{shape}: one band, zero floor vs device RelativeL2Loss {e[0]:.2e} (value) {e[1]:.2e} (gradient)")
    assert e[0] <= R.LOSS_TOL and e[1] <= R.GRAD_TOL, e


def test_identical_calls_give_identical_bits(gpu_device):
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss
    for dims, (B, C, M, N), bands, nb in ((1, (3, 2, 1, 200), "octave", None), (2, (2, 1, 64, 64), "radial", 16)):
        x, y = R.make_inputs(B, C, M, N)
        for cls in (BandRelativeL2Loss, SpectrumMatchingLoss):
            outs = []
            for _ in range(2):
                xd = x.to(DEV).requires_grad_(True)
                v = cls(dims, bands, nb, reduction=False)(xd, y.to(DEV))
                v.sum().backward()
                outs.append((v.detach().cpu(), xd.grad.cpu()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (dims, cls.__name__)


@pytest.mark.parametrize("shape,bands", [((3, 1, 16), "octave"), ((3, 2, 200), "octave"), ((3, 1, 8, 8), "octave"),
                                         ((3, 1, 64, 72), ("radial", 16))], ids=str)
def test_a_sample_does_not_depend_on_its_batch(gpu_device, shape, bands):
    """E of a batch of 3 equals E of three batches of 1, bit for bit (64 x 72: more than one partial sum per band)"""
    from rpde import ops
    dims = len(shape) - 2
    M, N = (1, shape[2]) if dims == 1 else shape[2:]
    x, y = R.make_inputs(shape[0], shape[1], M, N)
    xd, yd = x.to(DEV), y.to(DEV)
    for other in (None, yd):
        whole = ops.band_energy(xd, bands, dims, y=other)
        single = torch.cat([ops.band_energy(xd[b:b + 1], bands, dims, y=None if other is None else other[b:b + 1])
                            for b in range(shape[0])])
        assert torch.equal(whole, single)


def test_zeros_and_floors(gpu_device):
    from rpde import ops
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss
    x, y = R.make_inputs(3, 1, 1, 64)
    # a sample with x == y: band loss 0 for it, gradient 0 and finite everywhere
    x2 = x.clone()
    x2[1] = y[1]
    xd = x2.to(DEV).requires_grad_(True)
    r = BandRelativeL2Loss(1, reduction=False)(xd, y.to(DEV))
    r.sum().backward()
    r = r.detach()
    assert float(r[1]) == 0.0 and bool((xd.grad[1] == 0).all()) and bool(torch.isfinite(xd.grad).all())
    assert float(r[0]) > 0 and bool((xd.grad[0] != 0).any())
    # bands empty in x up to the rounding of the input (modes 8 .. 15 of sample 0 removed, one band per mode): a finite
    # spectrum loss, larger than a complete sample's, and a finite gradient
    X = torch.fft.rfft(x.double(), dim=-1)
    X[0, :, 8:16] = 0
    x3 = torch.fft.irfft(X, n=64, dim=-1).float()
    xd = x3.to(DEV).requires_grad_(True)
    v = SpectrumMatchingLoss(1, "modes", 16, reduction=False)(xd, y.to(DEV))
    v.sum().backward()
    v = v.detach()
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(xd.grad).all()) and float(v[0]) > float(v[2])
    # exactly zero energy: a zero field, every band empty
    zd = torch.zeros(2, 1, 64, device=DEV, requires_grad=True)
    v = SpectrumMatchingLoss(1, reduction=False)(zd, y[:2].to(DEV))
    v.sum().backward()
    assert bool(torch.isfinite(v).all()) and bool((zd.grad == 0).all())
    # a -1 entry carries no energy and no gradient.  Only DC has a band ("modes" with one band): its table row is cos 0 = 1
    # and sin 0 = 0, so on inputs that are small multiples of 2^-8 the device's DC coefficient is an exact sum, and
    # perturbing only the Nyquist mode (band -1) by 0.25 (-1)^t -- also exact in fp32 -- must leave E unchanged to the bit;
    # the gradient of E is then the constant 2 Z_0 / n, with no component along any other mode
    xq = (x * 256).round() / 256
    nyq = 0.25 * (1 - 2 * (torch.arange(64) % 2)).float().view(1, 1, 64)
    E0 = ops.band_energy(xq.to(DEV), ("modes", 1), 1)
    E1 = ops.band_energy((xq + nyq).to(DEV), ("modes", 1), 1)
    assert torch.equal(E0, E1) and torch.equal(E0.cpu()[:, 0], (xq.double().sum(2)[:, 0] ** 2 / 64).float())
    xd = (xq + nyq).to(DEV).requires_grad_(True)
    ops.band_energy(xd, ("modes", 1), 1).sum().backward()
    g = xd.grad.cpu()
    assert torch.equal(g, g[..., :1].expand_as(g)) and torch.equal(g[:, 0, 0].double(), 2 * (xq + nyq).double().sum(2)[:, 0] / 64)
    # and on the rounded inputs of the parity cases, where the transform's own rounding moves every coefficient: the
    # energies of the banded modes move by rounding only when mode 20 (band -1 under "modes" 16) grows by 0.25 cos
    t = torch.arange(64, dtype=torch.float64)
    bump = (0.25 * torch.cos(2 * math.pi * 20 * t / 64)).float().view(1, 1, 64)
    E0 = ops.band_energy(x.to(DEV), ("modes", 16), 1).cpu()
    E1 = ops.band_energy((x + bump).to(DEV), ("modes", 16), 1).cpu()
    assert R.rel_l2(E1, E0) <= R.LOSS_TOL          # the bump itself carries 0.25^2 / 2 x 64 = 2, several times E_tot's tail


def test_spec_is_kept_only_for_a_gradient(gpu_device):
    from rpde import ops
    x, _ = R.make_inputs(2, 1, 1, 64)
    E = ops.band_energy(x.to(DEV), "octave", 1)
    assert not E.requires_grad and E.grad_fn is None
    xd = x.to(DEV).requires_grad_(True)
    with torch.no_grad():
        assert ops.band_energy(xd, "octave", 1).grad_fn is None
    E2 = ops.band_energy(xd, "octave", 1)
    assert torch.equal(E2.detach(), E) and len(E2.grad_fn.saved_tensors) == 1
    yd = torch.ones_like(xd).requires_grad_(True)
    ops.band_energy(xd, "octave", 1, y=yd).sum().backward()
    assert yd.grad is None and xd.grad is not None


def test_one_object_serves_several_grids(gpu_device):
    """one loss object called at 32^2, 64^2 and 32^2 again gives what fresh objects give; an explicit table serves one
    grid and raises on another"""
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss
    for cls in (BandRelativeL2Loss, SpectrumMatchingLoss):
        shared = cls(2, reduction=False)
        for n in (32, 64, 32):
            x, y = R.make_inputs(2, 1, n, n)
            res = []
            for fn in (shared, cls(2, reduction=False)):
                xd = x.to(DEV).requires_grad_(True)
                r = fn(xd, y.to(DEV))
                r.sum().backward()
                res.append((r.detach().cpu(), xd.grad.cpu()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert len(shared._tables) == 2
    fixed = BandRelativeL2Loss(2, torch.zeros(32, 17, dtype=torch.int64))
    x, y = R.make_inputs(2, 1, 32, 32)
    fixed(x.to(DEV), y.to(DEV))
    with pytest.raises(ValueError):
        fixed(torch.zeros(2, 1, 16, 16, device=DEV), torch.ones(2, 1, 16, 16, device=DEV))


def test_reductions_and_sum_loss(gpu_device):
    from utils.loss import BandRelativeL2Loss, RelativeL2Loss, SpectrumMatchingLoss, SumLoss
    x, y = R.make_inputs(3, 2, 1, 48)
    xd, yd = x.to(DEV), y.to(DEV)
    for cls in (BandRelativeL2Loss, SpectrumMatchingLoss):
        v = cls(1, reduction=False)(xd, yd)
        assert torch.allclose(cls(1)(xd, yd), v.mean(), rtol=1e-6) and torch.allclose(cls(1, size_average=False)(xd, yd), v.sum(), rtol=1e-6)
    both = SumLoss([(1.0, RelativeL2Loss()), (0.25, SpectrumMatchingLoss(1))])
    want = RelativeL2Loss()(xd, yd) + 0.25 * SpectrumMatchingLoss(1)(xd, yd)
    assert torch.allclose(both(xd, yd), want, rtol=1e-6)


def test_rollout_band_energy(gpu_device):
    from utils.autoregressive_step import rollout_band_energy
    B, T, n = 3, 4, 64
    _, traj = R.make_inputs(B * (T + 1), 1, 1, n)
    traj = traj.reshape(B, T + 1, n)
    pred = traj[:, 1:] * torch.tensor([1.0, 1.0, 0.5, 1.0]).view(1, T, 1)      # step 2 has a quarter of the energy
    st = rollout_band_energy(pred.to(DEV), traj.to(DEV), spectrum_floor=0.0)
    table, J = R.table_of(1, n, "octave", None)
    E_true = R.band_energies(traj[:, 1:].reshape(B * T, 1, n).double(), table, J).view(B, T, J).mean(0)
    assert st["energy_pred"].shape == (T, J) and st["energy_true"].shape == (T, J) and st["log_ratio_rms"].shape == (T,)
    assert R.rel_l2(st["energy_true"], E_true) <= R.LOSS_TOL
    assert R.rel_l2(st["energy_pred"][2], 0.25 * E_true[2]) <= R.LOSS_TOL
    rms = st["log_ratio_rms"]
    assert float(rms[0]) == 0.0 and float(rms[3]) == 0.0 and abs(float(rms[2]) - math.log(4.0)) <= 1e-5


def test_train_takes_a_band_loss_under_a_graph(gpu_device):
    """train(..., loss_fn=BandRelativeL2Loss(1), graph=True) after warm() follows the eager loop, losses and weights, within
    the bounds of test_graphed_step_matches_eager (tests/test_gpu_spectral_loss.py)"""
    from models.fno import FNO1d
    from rpde.optim import FlatAdamW
    from train.training import train
    from utils.loss import BandRelativeL2Loss
    torch.manual_seed(11)
    m0 = FNO1d(1, 1, modes=8, width=16).to(gpu_device)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(1, 64, generator=g), torch.randn(1, 64, generator=g)) for _ in range(16)]
    loader = lambda: torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)   # noqa: E731
    loss_fn = BandRelativeL2Loss(1)
    loss_fn.warm((64,), gpu_device)

    def run(graph):
        m = copy.deepcopy(m0)
        opt = FlatAdamW(m.parameters(), lr=2e-3, capturable=True)
        return m, train(m, loader(), loader(), opt, None, epochs=2, device=gpu_device, graph=graph, loss_fn=loss_fn)

    m_g, (tl_g, vl_g) = run(True)
    m_e, (tl_e, vl_e) = run(False)
    assert len(tl_g) == 2 and all(math.isfinite(v) for v in tl_g + vl_g)
    for a, b in zip(tl_g + vl_g, tl_e + vl_e):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (tl_g, tl_e, vl_g, vl_e)
    for pe, pg in zip(m_e.parameters(), m_g.parameters()):
        a, b = (torch.view_as_real(p.detach()) if p.is_complex() else p.detach() for p in (pe, pg))
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-6
    assert any(not torch.equal(a, b) for a, b in zip(m0.parameters(), m_g.parameters()))


def test_entry_point_spectrum(gpu_device, tmp_path, capsys):
    """training.loss=spectrum trains main_1d on relative L2 + lambda x spectrum matching; the reported scores stay relative
    L2 and the rollout record carries the band energies"""
    from rpde.entry import run
    base = ["model=fno_1d/fno_1d", "dataset=synthetic/ks_512", "dataset.resolutions={64: 16}", "dataset.n_val=8",
            "dataset.n_test=8", "training.epochs=2", "training.batch_size=8", "model.width=16", "model.modes=8",
            f"checkpoint_dir={tmp_path}"]
    l2 = run(1, base + ["training.loss=spectrum"])
    out = capsys.readouterr().out
    rec = [json.loads(ln) for ln in out.splitlines() if '"test_rel_l2"' in ln]
    assert math.isfinite(l2) and 0 < l2 < 2.0 and rec and rec[0]["test_rel_l2"] == l2
    assert math.isfinite(rec[0]["final_train_loss"]) and rec[0]["final_train_loss"] > 0
    bands = [json.loads(ln) for ln in out.splitlines() if '"rollout_band_energy"' in ln]
    assert bands and '"rollout_rel_l2"' in out
    for res, st in bands[0]["rollout_band_energy"].items():
        J = R.table_of(1, int(res), "octave", None)[1]
        assert set(st) == {"energy_pred", "energy_true", "log_ratio_rms"}
        T = len(st["log_ratio_rms"])
        assert T >= 1 and len(st["energy_pred"]) == T and len(st["energy_pred"][0]) == J == len(st["energy_true"][0])
        assert all(math.isfinite(v) for v in st["log_ratio_rms"]) and all(math.isfinite(v) for row in st["energy_pred"] for v in row)
    assert run.last["rollout_band_energy"].keys() == run.last["rollout_rel_l2"].keys()
