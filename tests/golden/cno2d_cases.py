"""The CNO2d fixtures: cases and the seeded weights / buffers / inputs of tests/golden/cno_cases.py, whose run_case runs a
case on a module -- the reference's when tests/golden/make_golden_cno2d.py writes the fixtures, the project's when the
GPU tests read them.  Own code; no reference content."""
from __future__ import annotations

from tests.golden.cno_cases import run_case, state_for  # noqa: F401  (the 2-D fixtures are run as the 1-D ones are)

SMALL = dict(in_dim=1, out_dim=1, size=16, N_layers=2, N_res=1, N_res_neck=1, channel_multiplier=8)
# conf/model/cno_2d/cno_2d.yaml
YAML = dict(in_dim=3, out_dim=3, N_layers=4, N_res=4, N_res_neck=4, channel_multiplier=16, use_bn=False)

# mode: the module's train / eval flag; grads: "all" (dx and every parameter) or "dx"
CASES = [
    dict(name="cno2d_lrelu_16_16", kind="CNO_LReLu", ctor=dict(in_size=16, out_size=16), x=(2, 3, 16, 16), seed=41, mode="train", grads="dx"),
    dict(name="cno2d_lrelu_16_8", kind="CNO_LReLu", ctor=dict(in_size=16, out_size=8), x=(2, 3, 16, 16), seed=42, mode="train", grads="dx"),
    dict(name="cno2d_lrelu_8_16", kind="CNO_LReLu", ctor=dict(in_size=8, out_size=16), x=(2, 3, 8, 8), seed=43, mode="train", grads="dx"),
    dict(name="cno2d_small_train", kind="CNO2d", ctor=dict(SMALL, use_bn=True), x=(4, 1, 16, 16), seed=51, mode="train", grads="all"),
    dict(name="cno2d_small_eval", kind="CNO2d", ctor=dict(SMALL, use_bn=True), x=(4, 1, 16, 16), seed=52, mode="eval", grads="all"),
    dict(name="cno2d_small_nobn", kind="CNO2d", ctor=dict(SMALL, use_bn=False), x=(4, 1, 16, 16), seed=53, mode="train", grads="all"),
    # a size = 16 model fed 24 x 24: the first activation resamples 24 -> 32 -> 16 along both axes
    dict(name="cno2d_offsize", kind="CNO2d", ctor=dict(SMALL, use_bn=True), x=(2, 1, 24, 24), seed=54, mode="eval", grads="all"),
    # the shipped yaml at size 32: its neck is 2 x 2, its deepest activations run on 4 x 4 and 2 x 2 planes
    dict(name="cno2d_yaml_32", kind="CNO2d", ctor=dict(YAML, size=32), x=(2, 3, 32, 32), seed=55, mode="eval", grads="dx"),
]
BY_NAME = {c["name"]: c for c in CASES}
