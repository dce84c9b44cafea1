"""models.unet on the GPU against the fixtures that tests/golden/make_golden_unet.py wrote from the reference's UNet1d /
UNet2d (CPU, float32): the small models in training mode (outputs, every gradient, the BatchNorm buffers after the
step) and in eval mode, a 32-point input whose bottleneck has two points, GroupNorm with several channels and with one
channel per group, a rectangular 2-D input with three channels, and the shipped 1-D yaml at width 64.  The fixture's
state loads with strict=True.

Budgets: synth.check_results with the project's forward 1e-5 and gradient 2e-5, each widened to 3 x the fixture's
`floor` where the reference's own float32 run sits further than that from its float64 run (BatchNorm's cancellation);
the generator writes no fixture with a floor above 3.3e-5.

Measured on an MI355X, worst rel-L2 per fixture (the fixture's worst floor): unet1d_small_train 9.0e-6 (7.3e-6),
unet1d_small_eval 1.3e-6 (1.9e-6), unet1d_short_train 7.9e-6 (4.7e-6), unet1d_gn_train 6.6e-6 (4.1e-6), unet1d_gn_3ch 3.4e-6
(3.9e-6), unet1d_yaml_64 4.9e-7 (3.5e-7), unet2d_small_train 3.9e-6 (3.4e-6), unet2d_small_eval 1.9e-6 (1.3e-6),
unet2d_rect_train 1.04e-5 (7.6e-6).
"""
import pytest

from tests.golden import synth
from tests.golden.unet_cases import CASES, load_case, run_case, state_for

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_fixture(gpu_device, name):
    from models import unet as M
    case, spec, digests = load_case(name)
    module = getattr(M, case["kind"])(**case["ctor"])
    assert synth.spec_of(module.state_dict()) == spec
    missing, unexpected = module.load_state_dict(state_for(spec, case["seed"]), strict=True)
    assert not missing and not unexpected
    res = run_case(module.to(gpu_device), case, device=gpu_device)
    errs = synth.check_results(res, digests, tol=1e-5, grad_tol=2e-5, label=name)
    worst = max(errs, key=errs.get)
    floors = [float(d["floor"]) for d in digests.values() if float(d["floor"]) < 1.0]      # (>= 1: a gradient that is zero in float64)
    print(f"{name}: {len(errs)} tensors, worst rel-L2 {errs[worst]:.3e} ({worst}), worst floor {max(floors):.2e}")
