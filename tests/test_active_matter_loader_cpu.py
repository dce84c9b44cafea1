"""The active-matter loaders (dataloaders/active_matter_markov.py, active_matter_all_markov.py) on synthetic .npz
archives: every rule is restated here on the arrays the test wrote, independently of the loaders' code."""
import numpy as np
import pytest
import torch

N_FRAMES, H = 6, 8


def _write(folder, name, n, seed, batch_axis=True, scalars=None, members=("c", "v")):
    """one archive with n trajectories of N_FRAMES frames at H x H -> (concentration [n, T, H, W], velocity [n, T, H, W, 2])"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, N_FRAMES, H, H)).astype(np.float32)
    v = rng.standard_normal((n, N_FRAMES, H, H, 2)).astype(np.float32)
    blob = {}
    if "c" in members:
        blob["t0_fields/concentration"] = c if batch_axis else c[0]
    if "v" in members:
        blob["t1_fields/velocity"] = v if batch_axis else v[0]
    for k, val in (scalars or {}).items():
        blob["scalars/" + k] = np.float32(val)
    np.savez(folder / name, **blob)
    return c, v


def _frames(c, v):
    """[n, T, 3, H, W]: the concentration in front of the two velocity components"""
    return np.concatenate([c[:, :, None], np.moveaxis(v, -1, 2)], axis=2)


def _pairs(frames):
    n, T = frames.shape[:2]
    x = np.stack([frames[i, t] for i in range(n) for t in range(T - 1)])
    y = np.stack([frames[i, t + 1] for i in range(n) for t in range(T - 1)])
    return x, y


def test_single_file_pairs_strides_and_cap(tmp_path):
    from dataloaders.active_matter_markov import ActiveMatterMarkovDataset
    c, v = _write(tmp_path, "one.npz", 7, seed=1, scalars={"alpha": -3.0, "zeta": 9.0})
    ds = ActiveMatterMarkovDataset("one.npz", str(tmp_path))
    x, y = _pairs(_frames(c, v))
    assert len(ds) == 7 * (N_FRAMES - 1) and tuple(ds.x.shape) == (35, 3, H, H)
    assert np.array_equal(ds.x.numpy(), x) and np.array_equal(ds.y.numpy(), y)
    assert np.array_equal(ds.x[:, 0].numpy(), x[:, 0]) and np.array_equal(ds[3][1].numpy(), y[3])   # channel 0: concentration
    assert tuple(ds.data.shape) == (7, N_FRAMES, H, H, 3) and tuple(ds.grid.shape) == (H, H, 2)
    assert (ds.alpha, ds.zeta) == (-3.0, 9.0)
    # strides on samples and time first, then the cap
    ds = ActiveMatterMarkovDataset("one.npz", str(tmp_path), reduced_batch=2, reduced_resolution_t=2, num_samples_max=3)
    x, y = _pairs(_frames(c[::2, ::2], v[::2, ::2])[:3])
    assert len(ds) == 3 * 2 and np.array_equal(ds.x.numpy(), x) and np.array_equal(ds.y.numpy(), y)
    with pytest.raises(AssertionError, match="reduced_resolution"):
        ActiveMatterMarkovDataset("one.npz", str(tmp_path), reduced_resolution=2)


def test_missing_member_and_missing_files(tmp_path):
    from dataloaders.active_matter_all_markov import MultiFileActiveMatterMarkovDataset
    from dataloaders.active_matter_markov import ActiveMatterMarkovDataset
    _write(tmp_path, "no_velocity.npz", 2, seed=2, members=("c",))
    with pytest.raises(KeyError, match="t1_fields/velocity"):
        ActiveMatterMarkovDataset("no_velocity.npz", str(tmp_path))
    with pytest.raises(KeyError, match="t1_fields/velocity"):
        MultiFileActiveMatterMarkovDataset("no_velocity.npz", str(tmp_path))
    with pytest.raises(ValueError, match="No files found"):
        MultiFileActiveMatterMarkovDataset("absent_*.npz", str(tmp_path))
    with pytest.raises(AssertionError, match="reduced_resolution"):
        MultiFileActiveMatterMarkovDataset("no_velocity.npz", str(tmp_path), reduced_resolution=2)
    with pytest.raises(FileNotFoundError):
        ActiveMatterMarkovDataset("absent.npz", str(tmp_path))


def test_multi_file_order_parameters_and_batch_axis(tmp_path):
    from dataloaders.active_matter_all_markov import MultiFileActiveMatterMarkovDataset, parameters_from_filename
    # written out of order: the loader sorts the names
    cb, vb = _write(tmp_path, "active_matter_L_10.0_zeta_17.0_alpha_-5.0.npz", 1, seed=4, batch_axis=False)
    cc, vc = _write(tmp_path, "active_scalar_visc_0.001_kappa_0.002_beta_5_0.npz", 2, seed=5,
                    scalars={"visc": 1e-3, "kappa": 2e-3, "beta": 5.0})
    ca, va = _write(tmp_path, "active_matter_L_10.0_zeta_1.0_alpha_-1.0.npz", 3, seed=3, scalars={"alpha": -2.0})
    assert parameters_from_filename("active_matter_L_10.0_zeta_17.0_alpha_-5.0.hdf5") == (10.0, 17.0, -5.0)
    assert parameters_from_filename("active_scalar_visc_0.001_kappa_0.002_beta_5_0.npz") == (None, None, None)
    ds = MultiFileActiveMatterMarkovDataset("active_*.npz", str(tmp_path))
    # sorted: ..zeta_1.0.. < ..zeta_17.0.. < active_scalar..; the [T, H, W] members of the second count as one trajectory
    x, y = _pairs(_frames(np.concatenate([ca, cb, cc]), np.concatenate([va, vb, vc])))
    assert len(ds) == 6 * (N_FRAMES - 1)
    assert np.array_equal(ds.x.numpy(), x) and np.array_equal(ds.y.numpy(), y)
    p = ds.file_parameters
    assert len(p) == 6 and [q["filename"][:16] for q in p] == ["active_matter_L_"] * 4 + ["active_scalar_vi"] * 2
    assert (p[0]["L"], p[0]["zeta"], p[0]["alpha"]) == (10.0, 1.0, -2.0)          # scalars/alpha in front of the name's
    assert (p[3]["L"], p[3]["zeta"], p[3]["alpha"]) == (10.0, 17.0, -5.0)
    assert (p[5]["L"], p[5]["zeta"], p[5]["alpha"]) == (None, None, None)
    assert p[5]["beta"] == 5.0 and abs(p[5]["kappa"] - 2e-3) < 1e-9 and "beta" not in p[0]
    st = ds.parameter_stats
    assert st["total_trajectories"] == 6 and st["total_files"] == 3
    assert st["alpha"] == {"min": -5.0, "max": -2.0, "unique": [-5.0, -2.0]} and st["L"]["unique"] == [10.0]
    # max_files keeps a prefix of the sorted names; the cap applies after concatenation
    ds = MultiFileActiveMatterMarkovDataset("active_*.npz", str(tmp_path), max_files=2, num_samples_max=4)
    x, y = _pairs(_frames(np.concatenate([ca, cb]), np.concatenate([va, vb])))
    assert len(ds.file_paths) == 2 and len(ds) == 4 * (N_FRAMES - 1) and len(ds.file_parameters) == 4
    assert np.array_equal(ds.x.numpy(), x) and np.array_equal(ds.y.numpy(), y)
    assert ds.parameter_stats["total_trajectories"] == 4
    ds = MultiFileActiveMatterMarkovDataset("active_*.npz", str(tmp_path), reduced_batch=2, reduced_resolution_t=3)
    x, y = _pairs(_frames(np.concatenate([ca[::2, ::3], cb[::2, ::3], cc[::2, ::3]]),
                          np.concatenate([va[::2, ::3], vb[::2, ::3], vc[::2, ::3]])))
    assert len(ds) == 4 * 1 and np.array_equal(ds.x.numpy(), x) and np.array_equal(ds.y.numpy(), y)


def test_split_statistics_and_normalisation(tmp_path):
    from dataloaders.active_matter_all_markov import multi_file_active_matter_markov_dataset
    from dataloaders.active_matter_markov import active_matter_markov_dataset
    c, v = _write(tmp_path, "active_scalar_a.npz", 5, seed=6)
    x, y = _pairs(_frames(c, v))
    n = len(x)                                                                 # 25 pairs: 20 / 2 / 3
    order = torch.randperm(n, generator=torch.Generator().manual_seed(42)).tolist()
    parts = order[:20], order[20:22], order[22:]
    for out in (active_matter_markov_dataset("active_scalar_a.npz", str(tmp_path), data_normalizer=False),
                multi_file_active_matter_markov_dataset("active_scalar_*.npz", str(tmp_path), data_normalizer=False)):
        assert len(out) == 7 and out[3:] == (None, None, None, None)
        for split, idx in zip(out[:3], parts):
            assert len(split) == len(idx)
            for j, i in enumerate(idx):
                assert np.array_equal(split[j][0].numpy(), x[i]) and np.array_equal(split[j][1].numpy(), y[i])
    lo_x, hi_x = float(x[parts[0]].min()), float(x[parts[0]].max())
    lo_y, hi_y = float(y[parts[0]].min()), float(y[parts[0]].max())
    assert (lo_x, hi_x) != (float(x.min()), float(x.max())) or (lo_y, hi_y) != (float(y.min()), float(y.max()))
    for out in (active_matter_markov_dataset("active_scalar_a.npz", str(tmp_path)),
                multi_file_active_matter_markov_dataset("active_scalar_*.npz", str(tmp_path))):
        assert out[3:] == (lo_x, hi_x, lo_y, hi_y)                             # the training split only
        for split, idx in zip(out[:3], parts):
            xs, ys = split[len(idx) - 1]
            i = idx[-1]
            assert np.allclose(xs.numpy(), (x[i] - lo_x) / (hi_x - lo_x), rtol=0, atol=1e-6)
            assert np.allclose(ys.numpy(), (y[i] - lo_y) / (hi_y - lo_y), rtol=0, atol=1e-6)
        xs = torch.stack([out[0][j][0] for j in range(20)])
        assert float(xs.min()) == 0.0 and abs(float(xs.max()) - 1.0) < 1e-6


def test_downsample_leg_and_resize_leg(tmp_path):
    from dataloaders.active_matter_all_markov import MultiFileActiveMatterMarkovDataset
    from dataloaders.active_matter_markov import ActiveMatterMarkovDataset
    from rpde._lib import RpdeError
    from utils.res_utils import downsample
    c, v = _write(tmp_path, "active_scalar_a.npz", 2, seed=7)
    frames = _frames(c, v)                                                     # [n, T, 3, H, W]
    small = np.stack([[[downsample(frames[i, t, ch][None, None], 4)[0, 0] for ch in range(3)]
                       for t in range(N_FRAMES)] for i in range(2)])
    x, y = _pairs(small)
    for ds in (ActiveMatterMarkovDataset("active_scalar_a.npz", str(tmp_path), s=4),
               MultiFileActiveMatterMarkovDataset("active_scalar_*.npz", str(tmp_path), s=4)):
        assert tuple(ds.x.shape) == (10, 3, 4, 4) and tuple(ds.grid.shape) == (4, 4, 2)
        assert np.allclose(ds.x.numpy(), x, rtol=0, atol=1e-6) and np.allclose(ds.y.numpy(), y, rtol=0, atol=1e-6)
    same = ActiveMatterMarkovDataset("active_scalar_a.npz", str(tmp_path), s=H)
    assert np.array_equal(same.x.numpy(), _pairs(frames)[0])                   # s == H: untouched
    if not torch.cuda.is_available():
        with pytest.raises(RpdeError, match="GPU"):                            # the resize leg is a device op
            ActiveMatterMarkovDataset("active_scalar_a.npz", str(tmp_path), s=12)
