"""The CNO fixtures: cases, seeded weights / buffers / inputs, and the one routine that runs a case on a module --
the reference's when tests/golden/make_golden_cno.py writes the fixtures, the project's when the GPU tests read them.
Own code; no reference content."""
from __future__ import annotations

from typing import Dict

import torch

from tests.golden import synth

SMALL = dict(in_dim=1, out_dim=1, size=32, N_layers=2, N_res=1, N_res_neck=1, channel_multiplier=8)
# conf/model/cno_1d/cno_1d.yaml
YAML = dict(in_dim=1, out_dim=1, N_layers=5, N_res=4, N_res_neck=4, channel_multiplier=32, use_bn=True)

# mode: the module's train / eval flag; grads: "all" (dx and every parameter) or "dx"
CASES = [
    dict(name="cno_lrelu_16_16", kind="CNO_LReLu", ctor=dict(in_size=16, out_size=16), x=(2, 3, 16), seed=11, mode="train", grads="dx"),
    dict(name="cno_lrelu_16_8", kind="CNO_LReLu", ctor=dict(in_size=16, out_size=8), x=(2, 3, 16), seed=12, mode="train", grads="dx"),
    dict(name="cno_lrelu_8_16", kind="CNO_LReLu", ctor=dict(in_size=8, out_size=16), x=(2, 3, 8), seed=13, mode="train", grads="dx"),
    dict(name="cno1d_small_train", kind="CNO1d", ctor=dict(SMALL, use_bn=True), x=(4, 1, 32), seed=21, mode="train", grads="all"),
    dict(name="cno1d_small_eval", kind="CNO1d", ctor=dict(SMALL, use_bn=True), x=(4, 1, 32), seed=22, mode="eval", grads="all"),
    dict(name="cno1d_small_nobn", kind="CNO1d", ctor=dict(SMALL, use_bn=False), x=(4, 1, 32), seed=23, mode="train", grads="all"),
    # a size = 32 model fed 48 points: the first activation resamples 48 -> 64 -> 32
    dict(name="cno1d_offsize", kind="CNO1d", ctor=dict(SMALL, use_bn=True), x=(4, 1, 48), seed=24, mode="eval", grads="all"),
    # the shipped yaml at size 64 (its neck has 2 points): eval mode only -- training-mode statistics over the 4 values
    # per channel there are ill-conditioned in the reference itself
    dict(name="cno1d_yaml_64", kind="CNO1d", ctor=dict(YAML, size=64), x=(2, 1, 64), seed=25, mode="eval", grads="dx"),
]
BY_NAME = {c["name"]: c for c in CASES}


def state_for(spec, seed: int) -> Dict[str, torch.Tensor]:
    """synth.fill_state_dict plus what BatchNorm's buffers need: positive running variances, an int64 step count"""
    sd = synth.fill_state_dict({k: v for k, v in spec.items() if not k.endswith("num_batches_tracked")}, seed)
    for name, (shape, dt) in spec.items():
        if name.endswith("running_var"):
            sd[name] = 0.5 + synth.rand_tensor(shape, seed, name).abs()
        elif name.endswith("running_mean"):
            sd[name] = 0.2 * synth.rand_tensor(shape, seed, name)
        elif name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(3, dtype=torch.int64)
    return sd


def run_case(module, case, device="cpu", dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """One forward and backward of `module` (already holding the case's state) on the case's seeded input:
    y, dx, grad/<parameter> (grads == "all"), buf/<buffer> after the step (training mode)."""
    seed = case["seed"]
    make = synth.rand_tensor if case["kind"] == "CNO_LReLu" else synth.smooth_field
    x = make(tuple(case["x"]), seed, "x").to(device=device, dtype=dtype).requires_grad_(True)
    module.train(case["mode"] == "train")
    y = module(x)
    upstream = synth.rand_tensor(tuple(y.shape), seed, "upstream").to(device=device, dtype=dtype)
    (y * upstream).sum().backward()
    res = {"y": y.detach(), "dx": x.grad.detach()}
    if case["grads"] == "all":
        for name, p in module.named_parameters():
            res["grad/" + name] = p.grad.detach()
    if case["mode"] == "train":
        for name, b in module.named_buffers():
            res["buf/" + name] = b.detach().clone()
    return res
