"""CPU (no GPU needed): the Darcy restatement tests/darcy_ref.py checks itself (matrix-free apply against the sparse
matrix, the sine table diagonalises the constant-coefficient operator, float64 PCG against the direct solve), the
library exports the new entry points and refuses bad grids without a device, the host tables equal the restatement's,
dataloaders/darcy_loader.py follows the reference's rules (synthetic archives, and the fixture
tests/golden/darcy_loader.npz recorded from the reference's load_darcy_data_from_mat), and the script
data_generation/darcy_2d.py refuses bad arguments before any device work."""
import json
import os

import numpy as np
import pytest
import torch

from tests import darcy_ref as R
from tests.conftest import REPO


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 12, 20])
def test_matrix_free_apply_equals_the_sparse_matrix(s):
    rng = np.random.default_rng(s)
    for a in (R.threshold(R.neumann_field(1, s, seed=s), 12.0, 3.0)[0], np.exp(rng.standard_normal((s, s)))):
        u = rng.standard_normal((s, s))
        mat = (R.matrix(a) @ u.ravel()).reshape(s, s)
        assert R.rel(R.apply(a, u), mat) < 1e-12
        m = R.matrix(a)
        assert abs(m - m.T).max() == 0.0                                   # symmetric bit for bit, boundary faces included
    # a boundary face weighs 2 a_c: the corner cell of a = 1 has diagonal s^2 (1 + 1 + 2 + 2)
    assert R.matrix(np.ones((s, s)))[0, 0] == 6.0 * s * s


@pytest.mark.parametrize("s", [8, 12, 36])
def test_sine_table_is_orthogonal_and_diagonalises_the_constant_operator(s):
    S, lam = R.tables(s)
    assert np.abs(S @ S.T - np.eye(s)).max() < 1e-13
    K = np.kron(S, S)
    D = K @ R.matrix(np.ones((s, s))).toarray() @ K.T
    want = np.diag((lam[:, None] + lam[None, :]).ravel())
    assert np.abs(D - want).max() < 1e-12 * lam.max()


@pytest.mark.parametrize("contrast", ["12_3", "1_0.1"])
def test_float64_pcg_agrees_with_the_direct_solve(contrast):
    hi, lo = R.CONTRASTS[contrast][:2]
    a = R.threshold(R.neumann_field(2, 20, seed=5), hi, lo)
    f = np.ones((20, 20))
    u, frozen_at = R.pcg(a, f, 80, 1e-13, np.float64)
    assert R.rel(u, R.direct(a, f)) < 1e-10
    assert (frozen_at < 80).all()
    # a = const: the preconditioner is the inverse, one iteration
    u1, fz1 = R.pcg(np.full((1, 20, 20), 7.0), f, 10, 1e-12, np.float64)
    assert fz1[0] == 1 and R.rel(u1, R.direct(np.full((1, 20, 20), 7.0), f)) < 1e-12


def test_neumann_field_has_zero_mean_and_mirrors():
    s = 12
    g = R.neumann_field(2, s, seed=3)
    assert np.abs(g.mean(axis=(1, 2))).max() < 1e-13
    # the even extension across the wall x = 1 is the same cosine series evaluated at the mirrored centres
    i = (np.arange(2 * s) + 0.5)[:, None]
    C2 = np.cos(np.pi * np.arange(s)[None, :] * i / s)
    xi = np.random.default_rng(3).standard_normal((2, s, s))
    ext = C2 @ (R.neumann_coef(s) * xi) @ C2.T
    assert np.abs(ext[:, :s, :s] - g).max() < 1e-13
    assert np.abs(ext[:, s:, :s] - g[:, ::-1, :]).max() < 1e-12
    assert np.abs(ext[:, :s, s:] - g[:, :, ::-1]).max() < 1e-12


# ---- the library and the host tables ----------------------------------------------------------------------------------
def test_library_exports_the_darcy_entry_points():
    from rpde import _lib
    lib = _lib.load()
    for name in ("rpde_darcy2d_ws_bytes", "rpde_darcy2d_apply", "rpde_darcy2d_solve", "rpde_sep2d"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES, name
    assert lib.rpde_darcy2d_ws_bytes(2, 20) >= 7 * 2 * 20 * 20 * 4
    for B, s in ((1, 10), (1, 6), (1, 516), (0, 16), (65536, 16), (1, 4)):
        assert lib.rpde_darcy2d_ws_bytes(B, s) == 0, (B, s)
    # argument errors need no device
    assert lib.rpde_darcy2d_apply(None, None, None, 1, 16, None) == _lib.ERR_ARG
    assert b"null" in lib.rpde_last_error()
    assert lib.rpde_sep2d(None, None, None, None, 1, 16, None, 0, None) == _lib.ERR_ARG


@pytest.mark.parametrize("s", [8, 20, 100])
def test_host_tables_are_the_restatement_rounded_once(s):
    from rpde import ops
    S, il = ops.darcy2d_tables(s)
    S64, lam = R.tables(s)
    assert S.dtype == torch.float32 and tuple(S.shape) == (s, s) and tuple(il.shape) == (s, s)
    assert np.array_equal(S.numpy(), S64.astype(np.float32))
    assert np.allclose(il.numpy(), (1.0 / (lam[:, None] + lam[None, :])).astype(np.float32), rtol=2e-7, atol=0)
    for bad in (10, 6, 516):
        with pytest.raises(ValueError):
            ops.darcy2d_tables(bad)


def test_neumann_field_tables_and_argument_errors():
    from data_generation.random_fields import GaussianRF, GaussianRFNeumann, neumann_tables
    C, coef = neumann_tables(12, 2, 3, 3.0)
    assert np.array_equal(C.numpy(), R.cosine_table(12).astype(np.float32))
    assert np.allclose(coef.numpy(), R.neumann_coef(12).astype(np.float32), rtol=2e-7, atol=0) and coef[0, 0] == 0
    g = GaussianRFNeumann(12, device="cpu")                              # construction needs no device
    assert g.sigma == 3.0 and g.size == (12, 12)
    for bad in (10, 4, 516):
        with pytest.raises(ValueError):
            GaussianRFNeumann(bad, device="cpu")
    with pytest.raises(ValueError):
        GaussianRF(2, 16, boundary="neumann", device="cpu")               # the periodic class is as it was


# ---- the loader -------------------------------------------------------------------------------------------------------
def _archive(tmp_path, name, n, s, seed, key="coeff", fmt="npz"):
    rng = np.random.default_rng(seed)
    coeff = np.where(rng.standard_normal((n, s, s)) >= 0, 12.0, 3.0).astype(np.float32)
    sol = rng.standard_normal((n, s, s)).astype(np.float32) + np.arange(n, dtype=np.float32)[:, None, None]
    path = os.path.join(tmp_path, f"{name}.{fmt}")
    if fmt == "npz":
        np.savez(path, **{key: coeff, "sol": sol})
    else:
        from scipy.io import savemat
        savemat(path, {key: coeff, "sol": sol})
    return coeff, sol


def test_loader_rules_on_synthetic_archives(tmp_path):
    from dataloaders.darcy_loader import darcy_dataset
    c1, s1 = _archive(tmp_path, "a", 13, 16, 1)
    c2, s2 = _archive(tmp_path, "b", 10, 16, 2, key="Kcoeff", fmt="mat")
    coeff, sol = np.vstack([c1, c2]), np.vstack([s1, s2])
    tr, va, te, xn, yn = darcy_dataset("a.npz", str(tmp_path), filename2="b.mat", reduced_resolution=2, data_normalizer=False)
    assert (len(tr), len(va), len(te)) == (18, 2, 3) and xn is None and yn is None        # 80 / 10 / 10 of 23
    order = [tr[i] for i in range(18)] + [va[i] for i in range(2)] + [te[i] for i in range(3)]
    for i, (x, y) in enumerate(order):                                                   # file order, stacked, strided
        assert tuple(x.shape) == (1, 8, 8) and tuple(y.shape) == (1, 8, 8)
        assert np.array_equal(x[0].numpy(), coeff[i, ::2, ::2]) and np.array_equal(y[0].numpy(), sol[i, ::2, ::2])
    # statistics from the training split only; the solution's mean grows with the sample index, so a statistic over
    # all 23 samples would differ visibly
    tr, va, te, xn, yn = darcy_dataset("a.npz", str(tmp_path), filename2="b.mat")
    xt, yt = torch.from_numpy(coeff[:18]), torch.from_numpy(sol[:18])
    assert xn.mean == pytest.approx(float(xt.mean()), rel=1e-6) and xn.std == pytest.approx(float(xt.std()), rel=1e-6)
    assert yn.mean == pytest.approx(float(yt.mean()), rel=1e-6) and yn.std == pytest.approx(float(yt.std()), rel=1e-6)
    assert abs(float(yt.mean()) - float(sol.mean())) > 0.1
    x0, y0 = te[0]
    assert torch.allclose(y0[0], (torch.from_numpy(sol[20]) - yn.mean) / (yn.std + yn.eps))
    assert torch.allclose(yn.decode(y0)[0], torch.from_numpy(sol[20]), atol=1e-5)
    # cap, then stride over the samples
    tr, va, te, _, _ = darcy_dataset("a.npz", str(tmp_path), num_samples_max=11, reduced_batch=2, data_normalizer=False)
    assert (len(tr), len(va), len(te)) == (4, 0, 2)
    assert np.array_equal(tr[1][0][0].numpy(), c1[2]) and np.array_equal(te[1][1][0].numpy(), s1[10])
    with pytest.raises(ValueError):
        darcy_dataset("a.npz", str(tmp_path), normalization_type="minmax")
    with pytest.raises(FileNotFoundError):
        darcy_dataset("missing.npz", str(tmp_path))
    np.savez(os.path.join(tmp_path, "bad.npz"), a=c1, u=s1)
    with pytest.raises(KeyError):
        darcy_dataset("bad.npz", str(tmp_path))


def test_loader_reads_the_pdebench_names(tmp_path):
    from dataloaders.darcy_loader import darcy_dataset
    c, s = _archive(tmp_path, "a", 10, 8, 4)
    np.savez(os.path.join(tmp_path, "p.npz"), nu=c, tensor=s[:, None])
    tr, va, te, _, _ = darcy_dataset("p.npz", str(tmp_path), data_normalizer=False)
    assert (len(tr), len(va), len(te)) == (8, 1, 1)
    assert np.array_equal(te[0][0][0].numpy(), c[9]) and np.array_equal(te[0][1][0].numpy(), s[9])


def test_loader_matches_the_reference_fixture(tmp_path):
    """split, stride and point-wise statistics as the reference's load_darcy_data_from_mat produced them
    (tests/golden/make_golden_darcy.py) on the same synthetic files, rebuilt here from the recorded recipe"""
    from scipy.io import savemat
    from dataloaders.darcy_loader import darcy_dataset
    from tests.golden.make_golden_darcy import synthetic_pair
    z = np.load(os.path.join(REPO, "tests", "golden", "darcy_loader.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    for case, (key, scale) in meta["cases"].items():
        names = []
        for i, spec in enumerate(meta["files"]):
            coeff, sol = synthetic_pair(**spec)
            names.append(f"{case}_{i}.mat")
            savemat(os.path.join(tmp_path, names[-1]), {key: coeff, "sol": sol})
        tr, va, te, xn, yn = darcy_dataset(names[0], str(tmp_path), filename2=names[1], reduced_resolution=scale,
                                           normalization_type="unit_gaussian")
        for nm, norm in (("x", xn), ("y", yn)):
            assert float(norm.eps) == float(z[f"{case}|{nm}_eps"])
            assert np.allclose(norm.mean.numpy(), z[f"{case}|{nm}_mean"], rtol=1e-6, atol=1e-7)
            assert np.allclose(norm.std.numpy(), z[f"{case}|{nm}_std"], rtol=1e-6, atol=1e-7)
        for split, ds in (("train", tr), ("val", va), ("test", te)):
            assert len(ds) == int(z[f"{case}|{split}_n"])
            for which, idx in (("first", 0), ("last", len(ds) - 1)):
                x, y = ds[idx]
                assert np.allclose(x.numpy(), z[f"{case}|{split}_x_{which}"], rtol=1e-5, atol=1e-6)
                assert np.allclose(y.numpy(), z[f"{case}|{split}_y_{which}"], rtol=1e-5, atol=1e-6)


# ---- the script -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--resolution", "10", "--out", "x.mat"], ["--resolution", "4", "--out", "x.mat"], ["--resolution", "516", "--out", "x.mat"],
    ["--samples", "0", "--out", "x.mat"], ["--batch", "0", "--out", "x.mat"], ["--lo", "0", "--out", "x.mat"],
    ["--hi", "-1", "--out", "x.mat"], ["--forcing", "0", "--out", "x.mat"], ["--iterations", "0", "--out", "x.mat"],
    ["--out", "x.h5"], [],
])
def test_script_argument_errors_come_before_device_work(argv, tmp_path, monkeypatch):
    from data_generation import darcy_2d
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        darcy_2d.main(argv)
    assert e.value.code == 2
    assert os.listdir(tmp_path) == []


def test_mat_round_trip(tmp_path):
    """what the script writes is what scipy.io.loadmat and the loader read: names, shapes, dtype, values"""
    from scipy.io import loadmat, savemat
    from dataloaders.darcy_loader import read_darcy
    coeff, sol = _archive(tmp_path, "a", 5, 12, 9)
    path = os.path.join(tmp_path, "rt.mat")
    savemat(path, {"coeff": coeff, "sol": sol})
    blob = loadmat(path)
    assert blob["coeff"].shape == (5, 12, 12) and blob["coeff"].dtype == np.float32
    assert np.array_equal(blob["coeff"], coeff) and np.array_equal(blob["sol"], sol)
    x, y = read_darcy(path)
    assert np.array_equal(x, coeff) and np.array_equal(y, sol)


def test_piecewise_constant():
    from data_generation.darcy_2d import piecewise_constant
    g = torch.tensor([[-1.0, 0.0], [2.0, -0.0]])
    assert torch.equal(piecewise_constant(g), torch.tensor([[3.0, 12.0], [12.0, 12.0]]))
    assert torch.equal(piecewise_constant(g, 1.0, 0.1), torch.tensor([[0.1, 1.0], [1.0, 1.0]]))


def test_dataset_config_composes():
    from rpde.config import compose
    args = compose(os.path.join(REPO, "resolution-pde_amd", "conf"), "config", ["dataset=darcy_flow/darcy_generated"])
    assert int(args.dataset.dims) == 2 and args.dataset.pde == "darcy" and args.dataset.evaluation_type == "naive_downsample"
    assert args.dataset.dataset_params["_target_"] == "dataloaders.darcy_loader.darcy_dataset"
    assert args.dataset.dataset_params["filename2"] is None
