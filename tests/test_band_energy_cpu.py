"""CPU: the restatement of tests/band_energy_ref.py against itself (Parseval, closed-form gradient, the relative-L2
limit), the host side of the band energies (rpde.ops.band_table / check_band_table / band_tables), the ABI's four
symbols in the header and the binding, the CPU refusal and the entry options."""
import os
import re

import pytest
import torch

from tests import band_energy_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rpde_band_energy_ws_bytes", "rpde_band_energy_spec_elems", "rpde_band_energy_fwd", "rpde_band_energy_bwd")
BANDED_ALL = [c for c in R.CASES if c[4][0] in ("octave", "one")]          # every entry has a band


@pytest.mark.parametrize("case", BANDED_ALL, ids=R.case_id)
def test_restatement_parseval(case):
    B, C, M, N, (kind, nb) = case
    table, J = R.table_of(M, N, kind, nb)
    x, _ = R.make_inputs(B, C, M, N)
    E = R.band_energies(x.double(), table, J)
    assert R.rel_l2(E.sum(1), (x.double() ** 2).flatten(1).sum(1)) <= 1e-13


@pytest.mark.parametrize("case", R.CASES + [(2, 2, 1, 15, ("octave", None)), (2, 1, 9, 7, ("octave", None))], ids=R.case_id)
def test_closed_form_gradient_is_autograd(case):
    """2 irfft2(gE[band] Z) against float64 autograd of the definition: 1-D and 2-D, even and odd N, tables with -1"""
    B, C, M, N, (kind, nb) = case
    table, J = R.table_of(M, N, kind, nb)
    x, _ = R.make_inputs(B, C, M, N)
    gE = R.upstream(B, J)
    xx = x.double().requires_grad_(True)
    g, = torch.autograd.grad((R.band_energies(xx, table, J) * gE.double()).sum(), xx)
    assert R.rel_l2(R.closed_form_grad(x, table, J, gE), g) <= 1e-12


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4][0] == "one"] + [(3, 2, 1, 48, ("one", None))], ids=R.case_id)
def test_one_band_zero_floor_is_relative_l2(case):
    B, C, M, N, (kind, nb) = case
    table, J = R.table_of(M, N, kind, nb)
    x, y = R.make_inputs(B, C, M, N)
    r, g = R.value_and_grad(lambda t: R.band_rel(t, y.double(), table, J, band_floor=0.0), x)
    r2, g2 = R.value_and_grad(lambda t: R.relative_l2(t, y), x)
    assert R.rel_l2(r, r2) <= 1e-12 and R.rel_l2(g, g2) <= 1e-12


def test_octave_edges():
    """band 1 + floor(log2 |k|): a new band starts at |k|^2 = 1, 4, 16, 64 and the value below each still has the
    previous band; in 2-D |k|^2 = k1^2 + k2^2 with signed k1"""
    from rpde import ops
    t1, J1 = ops.band_table((64,), "octave")
    assert t1.dtype == torch.int32 and tuple(t1.shape) == (1, 33) and J1 == 7
    assert [int(t1[0, k]) for k in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32)] == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    t2, J2 = ops.band_table((32, 32), "octave")
    by_q = {}
    for r in range(32):
        for k in range(17):
            by_q.setdefault(R.signed(32)[r] ** 2 + k ** 2, set()).add(int(t2[r, k]))
    for q, band in ((0, 0), (1, 1), (3, None), (4, 2), (15, None), (16, 3), (63, None), (64, 4), (65, 4)):
        if band is not None:
            assert by_q[q] == {band}, (q, by_q[q])
    assert by_q[2] == {1} and by_q[13] == {2} and by_q[61] == {3}          # one below 4, 16 (15 = no k), 64 (63 = no k)
    assert by_q[5] == {2} and by_q[17] == {3}
    assert torch.equal(t2.to(torch.int64), R.octave_table(32, 32)[0]) and J2 == R.octave_table(32, 32)[1]
    assert int(t2.min()) == 0                                     # every entry has a band
    assert int(t2[31, 1]) == int(t2[1, 1]) == 1                   # ky = 31 is k1 = -1
    assert ops.band_table((32, 32), "octave") is ops.band_table((32, 32), "octave")        # cached


def test_radial_and_modes_tables():
    from rpde import ops
    t, J = ops.band_table((32, 32), "radial", 64)
    assert J == 64 and torch.equal(t, ops.radial_bins(32, 32, 64)[0])
    assert ops.band_table((16, 12), "radial")[1] == 64
    tabs = ops.band_tables(t, J, (32, 32), "cpu")
    # 32^2 with 64 bins of width 1/128 in r = |k| / 32, i.e. 1/4 in |k|: a bin owns an entry iff some k1^2 + k2^2 with
    # |k| < 16 falls into it
    qs = {a * a + b * b for a in range(-16, 16) for b in range(17)}
    want = len({int(4 * q ** 0.5 + 1e-9) for q in qs if q < 256})
    assert tabs.J_e == want and tabs.J_e < 64
    m, Jm = ops.band_table((64,), "modes", 16)
    assert Jm == 16 and m[0, :16].tolist() == list(range(16)) and bool((m[0, 16:] == -1).all())
    for bad in (dict(spatial_shape=(64,), kind="radial"), dict(spatial_shape=(8, 8), kind="modes", num_bands=4),
                dict(spatial_shape=(64,), kind="modes"), dict(spatial_shape=(64,), kind="thirds"),
                dict(spatial_shape=(64,), kind="octave", num_bands=3), dict(spatial_shape=(64,), kind="modes", num_bands=5000)):
        with pytest.raises(ValueError):
            ops.band_table(**bad)


def test_device_tables_list_every_band():
    """band_tables on the host: the padded table, and entries / start naming each band's entries exactly once with the
    Hermitian multiplicity in the low bit"""
    from rpde import ops
    for M, N, kind, nb in ((1, 200, "octave", None), (16, 12, "radial", 6), (8, 9, "octave", None)):
        grid = (N,) if M == 1 else (M, N)
        table, J = ops.band_table(grid, kind, nb)
        T = ops.band_tables(table, J, grid, "cpu")
        K, kp = N // 2 + 1, (N // 2 + 1 + 3) // 4 * 4
        assert tuple(T.band.shape) == (M, kp) and torch.equal(T.band[:, :K], table) and bool((T.band[:, K:] == -1).all())
        assert T.start.tolist()[0] == 0 and T.start.tolist()[-1] == T.n_entries == int((table >= 0).sum())
        seen = torch.zeros(M, K, dtype=torch.int64)
        for j in range(J):
            for en in T.entries[T.start[j]:T.start[j + 1]].tolist():
                off, twice = en >> 1, en & 1
                ky, rest = divmod(off, 2 * kp)
                assert rest < K and int(table[ky, rest]) == j
                assert twice == (0 if rest == 0 or (N % 2 == 0 and rest == N // 2) else 1)
                seen[ky, rest] += 1
        assert torch.equal(seen, (table >= 0).to(torch.int64))
        assert T.J_e == R.owned_bands(table.to(torch.int64), J)


def test_check_band_table_refuses():
    from rpde import ops
    good = ops.band_table((16, 12), "radial", 6)[0]
    ops.check_band_table(good, (16, 12), 6)
    ops.check_band_table(torch.zeros(33, dtype=torch.int64), (64,), 1)          # a 1-D table may be [K]
    asym = good.clone()
    asym[3, 0] = (int(asym[3, 0]) + 1) % 6                                       # band[3] != band[13] in column kx = 0
    with pytest.raises(ValueError, match="kx=0"):
        ops.check_band_table(asym, (16, 12), 6)
    nyq = good.clone()
    nyq[2, 6] = 0 if int(nyq[2, 6]) != 0 else 1
    with pytest.raises(ValueError, match="kx=6"):
        ops.check_band_table(nyq, (16, 12), 6)
    inner = good.clone()
    inner[3, 2] = (int(inner[3, 2]) + 1) % 6                                     # an inner column may be anything
    ops.check_band_table(inner, (16, 12), 6)
    for bad in (torch.full_like(good, 6), torch.full_like(good, -2)):
        with pytest.raises(ValueError, match="values"):
            ops.check_band_table(bad, (16, 12), 6)
    with pytest.raises(ValueError, match="integer"):
        ops.check_band_table(good.float(), (16, 12), 6)
    with pytest.raises(ValueError, match="shape"):
        ops.check_band_table(good, (16, 16), 6)


def test_header_declares_and_lib_binds():
    from rpde import _lib
    header = open(os.path.join(REPO, "include", "rpde.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
        assert name in _lib._SIGNATURES
    lib = _lib.load()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    # the queries need no device; refused sizes give 0
    assert lib.rpde_band_energy_spec_elems(2, 3, 1, 200) == 2 * 3 * 2 * 104
    assert lib.rpde_band_energy_spec_elems(2, 1, 16, 12) == 2 * 16 * 2 * 8
    assert lib.rpde_band_energy_ws_bytes(2, 1, 16, 12, 6) >= 2 * 4 * 2 * 16 * 2 * 8
    for args in ((0, 1, 1, 16, 4), (1, 1, 1, 5000, 4), (1, 1, 1, 16, 0), (1, 1, 1, 16, 4097)):
        assert lib.rpde_band_energy_ws_bytes(*args) == 0
    assert lib.rpde_band_energy_spec_elems(1, 1, 8, 1) == 0


def test_argument_errors_come_before_device_work():
    """null pointers, a refused size and a short workspace are reported by the entry points themselves: no device is
    needed to get the answer"""
    from rpde import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32)
    p = buf.data_ptr() + (-buf.data_ptr()) % 256
    assert lib.rpde_band_energy_fwd(None, None, p, p, 1, p, None, 1, 1, 1, 16, 4, p, 4096, None) == _lib.ERR_ARG
    assert lib.rpde_band_energy_fwd(p, None, p, p, 1, p, None, 1, 1, 1, 16, 0, p, 4096, None) == _lib.ERR_ARG
    assert lib.rpde_band_energy_fwd(p, None, p, p, 100, p, None, 1, 1, 1, 16, 4, p, 4096, None) == _lib.ERR_ARG
    assert lib.rpde_band_energy_fwd(p, None, p, p, 1, p, None, 1, 1, 1, 16, 4, p, 16, None) == _lib.ERR_WORKSPACE
    assert lib.rpde_band_energy_bwd(p, p, None, p, 1, 1, 1, 16, 4, p, 4096, None) == _lib.ERR_ARG
    assert lib.rpde_band_energy_bwd(p, p, p, p, 1, 1, 1, 16, 4, p, 16, None) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.rpde_last_error()


def test_cpu_tensors_raise():
    from rpde import ops
    from rpde._lib import RpdeError
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss, SumLoss, RelativeL2Loss
    x, y = R.make_inputs(2, 1, 1, 64)
    with pytest.raises(RpdeError):
        ops.band_energy(x, "octave", 1)
    with pytest.raises(RpdeError):
        ops.band_energy(x, "octave", 1, y=y)
    for fn in (BandRelativeL2Loss(1), SpectrumMatchingLoss(1), SumLoss([(1.0, RelativeL2Loss()), (0.1, SpectrumMatchingLoss(1))])):
        with pytest.raises(RpdeError):
            fn(x, y)
    with pytest.raises(ValueError):
        ops.band_energy(x, "octave", 2)


def test_loss_constructors():
    from utils.loss import BandRelativeL2Loss, SpectrumMatchingLoss, SumLoss
    with pytest.raises(ValueError):
        BandRelativeL2Loss(3)
    with pytest.raises(ValueError):
        BandRelativeL2Loss(1, "radial")
    with pytest.raises(ValueError):
        SpectrumMatchingLoss(2, "modes", 4)
    with pytest.raises(ValueError):
        BandRelativeL2Loss(1, band_floor=-1.0)
    with pytest.raises(ValueError):
        SpectrumMatchingLoss(1, torch.zeros(33))                  # a float table
    with pytest.raises(ValueError):
        SumLoss([])
    assert BandRelativeL2Loss(1, torch.zeros(33, dtype=torch.int64)).num_bands == 1


def test_entry_options():
    from rpde.entry import training_loss
    from utils.loss import BandRelativeL2Loss, RelativeL2Loss, SpectralRelativeL2Loss, SpectrumMatchingLoss, SumLoss
    assert training_loss({}, 1) == ("l2", None) and training_loss({"loss": "l2"}, 2) == ("l2", None)
    assert isinstance(training_loss({"loss": "sobolev", "loss_s": 0.5}, 1)[1], SpectralRelativeL2Loss)
    name, fn = training_loss({"loss": "band", "loss_bands": "radial", "loss_num_bands": 16, "loss_band_floor": 0.01}, 2)
    assert name == "band" and isinstance(fn, BandRelativeL2Loss) and (fn.bands, fn.num_bands, fn.band_floor) == ("radial", 16, 0.01)
    name, fn = training_loss({"loss": "band"}, 1)
    assert (fn.bands, fn.num_bands, fn.band_floor, fn.dims) == ("octave", None, 1e-3, 1)
    name, fn = training_loss({"loss": "spectrum", "loss_lambda": 0.25, "loss_spectrum_floor": 1e-4}, 1)
    assert name == "spectrum" and isinstance(fn, SumLoss) and fn.weights == [1.0, 0.25]
    assert isinstance(fn.terms[0], RelativeL2Loss) and isinstance(fn.terms[1], SpectrumMatchingLoss)
    assert fn.terms[1].spectrum_floor == 1e-4 and fn.terms[1].bands == "octave"
    assert training_loss({"loss": "spectrum"}, 2)[1].weights == [1.0, 0.1]
    for bad in ({"loss": "h7"}, {"loss": "band", "loss_bands": "radial"}, {"loss": "spectrum", "loss_bands": "modes"}):
        with pytest.raises(SystemExit):
            training_loss(bad, 1)
