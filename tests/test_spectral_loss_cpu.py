"""CPU (no GPU needed): the float64 restatement of the mode-weighted relative L2 loss (tests/spectral_loss_ref.py) is
consistent with itself -- autograd against the closed-form gradient, omega == 1 against relative L2 -- the weight presets
and the host-side validation of utils/loss.py, and the argument checks of the C ABI."""
import math

import numpy as np
import pytest
import torch

from tests import spectral_loss_ref as S

SMALL = [c for c in S.CASES if c[1][-1] <= 96]


@pytest.mark.parametrize("case", SMALL, ids=S.case_id)
def test_autograd_gradient_equals_the_closed_form(case):
    dims, shape, s = case
    x, y = S.make_inputs(shape, 1e-2, S.SEED)
    omega = S.sobolev(shape[2:], s)
    B = shape[0]
    up = torch.linspace(0.5, 2.0, B, dtype=torch.float64)
    for kw, g_b in ((dict(size_average=True), torch.full((B,), 1.0 / B, dtype=torch.float64)),
                    (dict(size_average=False), torch.ones(B, dtype=torch.float64)),
                    (dict(reduction=False, upstream=up), up)):
        _, g = S.loss_and_grad(x, y, omega, dims, **kw)
        assert S.rel_l2(g, S.closed_form_grad(x, y, omega, dims, g_b)) < 1e-12


@pytest.mark.parametrize("case", SMALL, ids=S.case_id)
def test_unit_weights_are_relative_l2(case):
    dims, shape, _ = case
    x, y = S.make_inputs(shape, 1e-2, S.SEED)
    ones = np.ones(shape[-1] // 2 + 1 if dims == 1 else (shape[-2], shape[-1] // 2 + 1))
    assert S.rel_l2(S.rel(x, y, ones, dims), S.relative_l2(x, y)) < 1e-12


def test_wrong_variants_are_wrong_in_float64():
    """the switches of the restatement move the answer by far more than the tolerances (the GPU tests rely on it)"""
    for dims, shape, s in SMALL:
        if s != 1.0:
            continue
        x, y = S.make_inputs(shape, 1e-2, S.SEED)
        good = S.rel(x, y, S.sobolev(shape[2:], s), dims)
        for label, (kw_w, kw_r) in S.wrong_variants(dims).items():
            wrong = S.rel(x, y, S.sobolev(shape[2:], s, **kw_w), dims, **kw_r)
            assert S.rel_l2(wrong, good) >= 1e-2, (shape, label)


def _independent_sobolev(shape, s, L):
    """integer wavenumbers from numpy's fftfreq, |k| at the Nyquist bin"""
    ks = [np.abs(np.fft.fftfreq(n, 1.0 / n)) for n in shape]
    ks[-1] = ks[-1][:shape[-1] // 2 + 1]
    q = sum(np.expand_dims((2 * np.pi * k / l) ** 2, tuple(a for a in range(len(shape)) if a != i))
            for i, (k, l) in enumerate(zip(ks, L)))
    return (1.0 + q) ** s


@pytest.mark.parametrize("shape,s,length", [((64,), 1.0, 1.0), ((63,), 2.0, 1.0), ((96,), 0.5, 2.0 * math.pi),
                                            ((32, 32), 1.0, 1.0), ((31, 33), 1.0, 1.0), ((24, 40), 2.0, (2.0, 0.5)),
                                            ((8, 6), 1.5, (1.0, 3.0))])
def test_sobolev_weights(shape, s, length):
    from utils.loss import check_mode_weights, sobolev_weights
    w = sobolev_weights(shape, s, length)
    L = [length] * len(shape) if isinstance(length, float) else list(length)
    want = _independent_sobolev(shape, s, L)
    assert w.dtype == torch.float64 and tuple(w.shape) == want.shape
    assert np.allclose(w.numpy(), want, rtol=1e-13, atol=0)
    assert np.allclose(w.numpy(), S.sobolev(shape, s, length), rtol=1e-13, atol=0)
    assert float(w.reshape(-1)[0]) == 1.0                                     # DC
    if shape[-1] % 2 == 0:                                                    # the Nyquist bin counts with |k| = n/2
        last = w[-1] if len(shape) == 1 else w[0, -1]
        assert abs(float(last) - (1.0 + (2 * math.pi * (shape[-1] // 2) / L[-1]) ** 2) ** s) <= 1e-12 * float(last)
    if len(shape) == 2 and shape[0] % 2 == 0:
        assert abs(float(w[shape[0] // 2, 0]) - (1.0 + (2 * math.pi * (shape[0] // 2) / L[0]) ** 2) ** s) <= 1e-9
    check_mode_weights(w, shape)                                               # a preset passes its own validation


def test_sobolev_weights_refuses_bad_arguments():
    from utils.loss import sobolev_weights
    for bad in (dict(spatial_shape=(4, 4, 4)), dict(spatial_shape=(1,)), dict(spatial_shape=(8, 8), length=(1.0,)),
                dict(spatial_shape=(8,), length=0.0)):
        with pytest.raises(ValueError):
            sobolev_weights(**bad)


def test_explicit_tables_are_validated_on_the_host():
    from utils.loss import SpectralRelativeL2Loss, check_mode_weights
    good = S.symmetric_random_table((8, 6), 1)
    check_mode_weights(good, (8, 6))
    check_mode_weights(S.symmetric_random_table((7, 5), 1), (7, 5))
    check_mode_weights(S.symmetric_random_table((16,), 1), (16,))
    neg, nan, inf = good.clone(), good.clone(), good.clone()
    neg[2, 1], nan[0, 0], inf[3, 2] = -1e-3, float("nan"), float("inf")
    asym0, asymn, interior = good.clone(), good.clone(), good.clone()
    asym0[1, 0] += 0.25                   # kx = 0: omega[1] != omega[7]
    asymn[2, 3] += 0.25                   # kx = W/2 (W = 6)
    interior[2, 1] += 0.25                # an interior column carries no constraint
    check_mode_weights(interior, (8, 6))
    for bad in (neg, nan, inf, asym0, asymn, good[:, :3], good[:7], good[0]):
        with pytest.raises(ValueError):
            check_mode_weights(bad, (8, 6))
    odd = S.symmetric_random_table((8, 5), 2)
    odd[3, 2] += 0.25                     # odd W: no Nyquist column, kx = 2 is interior
    check_mode_weights(odd, (8, 5))
    with pytest.raises(ValueError):
        check_mode_weights(torch.tensor([1.0, -1.0, 1.0]), (4,))
    # the loss object validates before it touches a device: bad tables raise ValueError even with CPU inputs
    x, y = torch.randn(2, 1, 8, 6), torch.randn(2, 1, 8, 6)
    for bad in (neg, nan, asym0, good[:, :3]):
        with pytest.raises(ValueError):
            SpectralRelativeL2Loss(2, weights=bad)(x, y)
    with pytest.raises(ValueError):
        SpectralRelativeL2Loss(1, weights=good)                                # a 2-D table for dims=1
    with pytest.raises(ValueError):
        SpectralRelativeL2Loss(3)
    with pytest.raises(ValueError):
        SpectralRelativeL2Loss(2, weights="h1")


def test_cpu_tensors_raise():
    from rpde import RpdeError
    from utils.loss import SpectralRelativeL2Loss
    with pytest.raises(RpdeError):
        SpectralRelativeL2Loss(1)(torch.randn(2, 1, 16), torch.randn(2, 1, 16))
    with pytest.raises(RpdeError):
        SpectralRelativeL2Loss(2, weights=S.symmetric_random_table((8, 6), 1))(torch.randn(2, 1, 8, 6), torch.randn(2, 1, 8, 6))
    with pytest.raises(ValueError):
        SpectralRelativeL2Loss(2)(torch.randn(2, 1, 16), torch.randn(2, 1, 16))        # a 1-D batch for dims=2


def test_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib
    lib = _lib.load()
    assert lib.rpde_wrel_l2_fwd(None, None, None, None, None, None, None, 0, 0, 0, 0, 1, None, 0, None) == _lib.ERR_ARG
    assert b"null" in lib.rpde_last_error()
    assert lib.rpde_wrel_l2_bwd(None, None, None, None, None, None, 0, 0, 0, 0, 1, None, 0, None) == _lib.ERR_ARG
    assert lib.rpde_wrel_l2_spec_elems(4, 1, 1, 64) == 4 * 2 * 36            # [B C][M][re|im][33 -> 36]
    assert lib.rpde_wrel_l2_spec_elems(2, 3, 24, 40) == 2 * 3 * 24 * 2 * 24  # 21 -> 24
    assert lib.rpde_wrel_l2_spec_elems(2, 1, 1, 8192) == 0 and lib.rpde_wrel_l2_ws_bytes(0, 1, 1, 64) == 0
    assert lib.rpde_wrel_l2_ws_bytes(2, 3, 24, 40) >= 4 * (2 * 3 * 24 * 40 + 2 * lib.rpde_wrel_l2_spec_elems(2, 3, 24, 40))
