"""UNet1d / UNet2d end to end on the GPU: five AdamW steps on one fixed batch lower the relative-L2 loss and repeat bit
for bit from one seed; main_1d / main_2d train the new yamls (width 8, the smallest synthetic data the entry accepts),
run the all-resolution sweep at the model's native resolutions and write a checkpoint; a saved state_dict reloads and
reproduces the eval-mode output bit for bit."""
import math

import pytest
import torch

from tests.golden import synth

pytestmark = pytest.mark.gpu

MODELS = [("UNet1d", dict(in_channels=1, out_channels=1, width=8), (4, 1, 64)),
          ("UNet1d", dict(in_channels=1, out_channels=1, width=8, use_groupnorm=True), (4, 1, 64)),
          ("UNet2d", dict(in_channels=1, out_channels=1, width=4), (2, 1, 32, 32))]


def _five_steps(kind, ctor, shape, device):
    from models import unet
    from rpde.optim import FlatAdamW
    from utils.loss import RelativeL2Loss
    torch.manual_seed(0)
    model = getattr(unet, kind)(**ctor).to(device).train()
    x, y = synth.smooth_field(shape, 5, "x").to(device), synth.smooth_field(shape, 5, "y").to(device)
    opt = FlatAdamW(model.parameters(), lr=2e-3)
    loss_fn, losses = RelativeL2Loss(), []
    for _ in range(5):
        opt.zero_grad()
        loss = loss_fn(model(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("kind,ctor,shape", MODELS)
def test_five_steps_lower_the_loss_and_repeat(gpu_device, kind, ctor, shape):
    losses, params = _five_steps(kind, ctor, shape, gpu_device)
    again, params2 = _five_steps(kind, ctor, shape, gpu_device)
    print(f"{kind} {ctor}: losses {losses}")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert losses == again and all(torch.equal(a, b) for a, b in zip(params, params2))


def test_main_1d_trains_sweeps_and_checkpoints(gpu_device, tmp_path):
    from rpde.entry import run
    l2 = run(1, ["model=unet/unet_1d", "dataset=synthetic/burgers_1024", "dataset.resolutions={64: 32}", "dataset.n_val=8",
                 "dataset.n_test=8", "model.width=8", "training.epochs=1", "training.batch_size=8", f"checkpoint_dir={tmp_path}"])
    assert math.isfinite(l2)
    last = run.last
    assert sorted(last["resolution_rel_l2"]) == [32, 64] and all(math.isfinite(v) and v > 0 for v in last["resolution_rel_l2"].values())
    ck = torch.load(tmp_path / "rpde_mi355x_1d.pt", weights_only=True)
    assert "encoder1.enc1conv1.weight" in ck["model_state_dict"] and "upconv4.weight" in ck["model_state_dict"]


def test_main_2d_trains_sweeps_and_checkpoints(gpu_device, tmp_path):
    from rpde.entry import run
    l2 = run(2, ["model=unet/unet_2d", "dataset=synthetic/ns_256", "dataset.resolutions={32: 16}", "dataset.n_val=8",
                 "dataset.n_test=8", "model.width=8", "training.epochs=1", "training.batch_size=8", f"checkpoint_dir={tmp_path}"])
    assert math.isfinite(l2)
    last = run.last
    assert sorted(last["resolution_rel_l2"]) == [32] and all(math.isfinite(v) and v > 0 for v in last["resolution_rel_l2"].values())
    ck = torch.load(tmp_path / "rpde_mi355x_2d.pt", weights_only=True)
    assert "bottleneck.bottleneckconv2.weight" in ck["model_state_dict"] and "conv.bias" in ck["model_state_dict"]


@pytest.mark.parametrize("kind,ctor,shape", MODELS)
def test_saved_state_reloads_bit_for_bit(gpu_device, tmp_path, kind, ctor, shape):
    from models import unet
    torch.manual_seed(1)
    model = getattr(unet, kind)(**ctor).to(gpu_device)
    x = synth.smooth_field(shape, 6, "x").to(gpu_device)
    model.train()
    model(x)                                           # moves the running statistics off their initial values
    model.eval()
    with torch.no_grad():
        want = model(x)
    torch.save(model.state_dict(), tmp_path / "unet.pt")
    fresh = getattr(unet, kind)(**ctor)
    fresh.load_state_dict(torch.load(tmp_path / "unet.pt", weights_only=True), strict=True)
    with torch.no_grad():
        got = fresh.to(gpu_device).eval()(x)
    assert torch.equal(got, want)
