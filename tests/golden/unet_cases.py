"""The U-Net fixtures: cases and the seeded weights / buffers / inputs of tests/golden/cno_cases.py, whose run_case runs a
case on a module -- the reference's when tests/golden/make_golden_unet.py writes the fixtures, the project's when the
GPU tests read them.  Own code; no reference content."""
from __future__ import annotations

import os

from tests.golden.cno_cases import run_case, state_for  # noqa: F401  (the U-Net fixtures are run as the CNO ones are)

SMALL_1D = dict(in_channels=1, out_channels=1, width=8)
SMALL_2D = dict(in_channels=1, out_channels=1, width=4)
# conf/model/unet/unet_1d.yaml over base_model
YAML_1D = dict(in_channels=1, out_channels=1, width=64)

# mode: the module's train / eval flag; grads: "all" (dx and every parameter) or "dx"
CASES = [
    dict(name="unet1d_small_train", kind="UNet1d", ctor=dict(SMALL_1D), x=(4, 1, 64), seed=61, mode="train", grads="all"),
    dict(name="unet1d_small_eval", kind="UNet1d", ctor=dict(SMALL_1D), x=(4, 1, 64), seed=62, mode="eval", grads="all"),
    # 32 points: the bottleneck has 2 points per sample, 8 values per channel
    dict(name="unet1d_short_train", kind="UNet1d", ctor=dict(SMALL_1D), x=(4, 1, 32), seed=63, mode="train", grads="all"),
    dict(name="unet1d_gn_train", kind="UNet1d", ctor=dict(SMALL_1D, use_groupnorm=True), x=(4, 1, 64), seed=64, mode="train", grads="all"),
    # width 4: GroupNorm(4) with one channel per group in the first level, three input and two output channels
    dict(name="unet1d_gn_3ch", kind="UNet1d", ctor=dict(in_channels=3, out_channels=2, width=4, use_groupnorm=True), x=(2, 3, 48),
         seed=65, mode="train", grads="all"),
    dict(name="unet1d_yaml_64", kind="UNet1d", ctor=dict(YAML_1D), x=(2, 1, 64), seed=66, mode="eval", grads="dx"),
    dict(name="unet2d_small_train", kind="UNet2d", ctor=dict(SMALL_2D), x=(2, 1, 32, 32), seed=71, mode="train", grads="all"),
    dict(name="unet2d_small_eval", kind="UNet2d", ctor=dict(SMALL_2D), x=(2, 1, 32, 32), seed=72, mode="eval", grads="all"),
    dict(name="unet2d_rect_train", kind="UNet2d", ctor=dict(in_channels=3, out_channels=2, width=4), x=(2, 3, 32, 48), seed=73,
         mode="train", grads="all"),
]
BY_NAME = {c["name"]: c for c in CASES}


def part_name(name: str, i: int) -> str:
    """fixture file i of a case: a case whose digests exceed one file's size limit is spread over several"""
    return name if i == 0 else f"{name}.part{i + 1}"


def load_case(name: str):
    """-> (case, spec, digests) of all the case's fixture files, through tests.conftest.load_fixture"""
    from tests.conftest import load_fixture
    case, spec, digests = load_fixture(name)
    i = 1
    while os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), part_name(name, i) + ".npz")):
        more = load_fixture(part_name(name, i))
        assert more[0] == case and more[1] == spec and not set(more[2]) & set(digests)
        digests.update(more[2])
        i += 1
    return case, spec, digests


def fixture_files(name: str):
    here = os.path.dirname(os.path.abspath(__file__))
    return [f for f in sorted(os.listdir(here)) if f == name + ".npz" or (f.startswith(name + ".part") and f.endswith(".npz"))]
