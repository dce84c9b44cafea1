"""models.CNO2d on the GPU against the fixtures that tests/golden/make_golden_cno2d.py wrote from the reference's CNO2d
(CPU, float32): the activation alone at three ratios, the small model (in_dim = out_dim = 1, size 16, two levels, one
residual block per level, channel_multiplier 8) in training mode (outputs, every gradient, the BatchNorm buffers after
the step), in eval mode, without BatchNorm, a size = 16 model fed 24 x 24, and the shipped yaml at size 32, whose neck
is 2 x 2 (gradient dx only).  The fixture's state loads with strict=True.

Budgets: synth.check_results with the project's forward 1e-5 and gradient 2e-5, each widened to 3 x the fixture's
`floor` where the reference's own float32 run sits further than that from its float64 run (the LeakyReLU kink), as
tests/test_gpu_cno_golden.py does.

Measured on an MI355X, worst rel-L2 per fixture (the fixture's worst floor): cno2d_lrelu_16_16 1.4e-7 (1.2e-7),
cno2d_lrelu_16_8 1.5e-7 (1.4e-7), cno2d_lrelu_8_16 1.4e-7 (1.3e-7), cno2d_small_train 1.8e-6 (2.1e-6), cno2d_small_eval
1.0e-6 (9.7e-7), cno2d_small_nobn 6.5e-7 (5.5e-7), cno2d_offsize 1.2e-6 (1.2e-6), cno2d_yaml_32 6.2e-7 (5.4e-7).
"""
import pytest

from tests.conftest import load_fixture
from tests.golden import synth
from tests.golden.cno2d_cases import CASES, run_case, state_for

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_fixture(gpu_device, name):
    from models import CNO2d as M
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
