"""models.CNO1d on the GPU against the fixtures that tests/golden/make_golden_cno.py wrote from the reference's CNO1d
(CPU, float32): the activation alone, the small model in training mode (outputs, every gradient, the BatchNorm buffers
after the step), in eval mode, without BatchNorm, fed another length than it was built for, and the shipped yaml at
size 64.  The fixture's state loads with strict=True.

Budgets: synth.check_results with the project's forward 1e-5 and gradient 2e-5, each widened to 3 x the fixture's
`floor` where the reference's own float32 run sits further than that from its float64 run (the LeakyReLU kink, as for
the ReLU fixtures).

Measured on an MI355X, worst rel-L2 per fixture (the fixture's worst floor): cno_lrelu_* 0 (bit for bit; 7.4e-8),
cno1d_small_train 1.6e-6 (1.2e-6), cno1d_small_eval 9.1e-7 (9.8e-7), cno1d_small_nobn 1.4e-6 (2.4e-6), cno1d_offsize 9.4e-7
(5.6e-7), cno1d_yaml_64 4.6e-7 (3.8e-7).
"""
import pytest

from tests.conftest import load_fixture
from tests.golden import synth
from tests.golden.cno_cases import CASES, run_case, state_for

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_fixture(gpu_device, name):
    from models import CNO1d as M
    case, spec, digests = load_fixture(name)
    module = getattr(M, case["kind"])(**case["ctor"])
    assert synth.spec_of(module.state_dict()) == spec
    missing, unexpected = module.load_state_dict(state_for(spec, case["seed"]), strict=True)
    assert not missing and not unexpected
    res = run_case(module.to(gpu_device), case, device=gpu_device)
    errs = synth.check_results(res, digests, tol=1e-5, grad_tol=2e-5, label=name)
    worst = max(errs, key=errs.get)
    floors = [float(d["floor"]) for d in digests.values() if float(d["floor"]) < 1.0]      # (>= 1: a gradient that is zero in float64)
    print(f"{name}: {len(errs)} tensors, worst rel-L2 {errs[worst]:.3e} ({worst}), worst floor {max(floors):.2e}")
