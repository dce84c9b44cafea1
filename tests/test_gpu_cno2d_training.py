"""CNO2d end to end on the GPU: train() on synthetic 2-D Markov pairs lowers the loss and moves the BatchNorm statistics,
evaluate() and the all-resolution sweep run, and the sweep's model_resolution path (resize to the model's resolution,
run, resize back) equals the plain path bit for bit where no resize is needed -- and the default path is untouched."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(in_dim=1, out_dim=1, size=16, N_layers=2, N_res=1, N_res_neck=1, channel_multiplier=8)


def _loaders(res, n_train, n_val, bs):
    from train.mres_training import ResolutionGroupedDataLoader
    from utils.synthetic import markov_pairs
    mk = lambda ds, shuffle: ResolutionGroupedDataLoader(ds, bs, shuffle=shuffle, seed=0, verbose=False, drop_last=shuffle)   # noqa: E731
    return mk(markov_pairs({res: n_train}, 2, 0), True), mk(markov_pairs({res: n_val}, 2, 50000), False)


def test_two_epochs_lower_the_loss_and_move_the_statistics(gpu_device):
    from models.CNO2d import CNO2d
    from rpde.optim import FlatAdamW
    from train.training import evaluate, train
    torch.manual_seed(0)
    model = CNO2d(**SMALL).to(gpu_device)
    bn = model.encoder[0].batch_norm
    mean0, var0 = bn.running_mean.clone(), bn.running_var.clone()
    train_loader, val_loader = _loaders(16, 64, 16, 16)
    opt = FlatAdamW(model.parameters(), lr=2e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=30, gamma=0.5)
    records = []
    hist, val = train(model, train_loader, val_loader, opt, sched, epochs=2, device=gpu_device, log=records.append)
    print(f"CNO2d small, 2 epochs: train {hist}, val {val}")
    assert len(hist) == 2 and all(math.isfinite(v) for v in hist + val)
    assert hist[1] < hist[0]
    assert int(bn.num_batches_tracked) == 2 * len(train_loader)
    assert not torch.equal(bn.running_mean, mean0) and not torch.equal(bn.running_var, var0)
    score = evaluate(model, val_loader, normalization_type="simple", device=gpu_device)
    assert math.isfinite(score)


def test_sweep_at_the_models_resolution(gpu_device):
    from models.CNO2d import CNO2d
    from utils.resize_utils import evaluate_all_resolutions
    from utils.synthetic import markov_pairs
    torch.manual_seed(1)
    model = CNO2d(**SMALL).to(gpu_device).eval()
    pairs = markov_pairs({32: 6}, 2, 60000)
    tx, ty = torch.stack([x for x, _ in pairs]), torch.stack([y for _, y in pairs])
    # (a CNO2d returns size x size points whatever it is fed, so the plain sweep can only score it at its own resolution)
    plain = evaluate_all_resolutions(model, tx, ty, max_resolution=16, min_resolution=16, batch_size=4, device=gpu_device)
    sized = evaluate_all_resolutions(model, tx, ty, max_resolution=32, min_resolution=16, batch_size=4, device=gpu_device,
                                     model_resolution=16)
    print(f"sweep plain {plain}, through resolution 16 {sized}")
    assert list(plain) == [16] and list(sized) == [16, 32]
    assert all(math.isfinite(v) for v in list(plain.values()) + list(sized.values()))
    assert sized[16] == plain[16]                       # no resize at the model's own resolution: the same calls
    with pytest.raises(RuntimeError):                   # 32 x 32 in, 16 x 16 out: only the resized path scores 32
        evaluate_all_resolutions(model, tx, ty, max_resolution=32, min_resolution=32, batch_size=4, device=gpu_device)


def test_default_sweep_makes_the_same_calls(gpu_device):
    """without model_resolution the model sees exactly the strided fields, once per batch, as before"""
    from utils.resize_utils import evaluate_all_resolutions, to_resolution
    from utils.synthetic import markov_pairs
    pairs = markov_pairs({32: 6}, 2, 60001)
    tx, ty = torch.stack([x for x, _ in pairs]), torch.stack([y for _, y in pairs])
    seen = []

    class Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x.clone())
            return 0.5 * x

    out = evaluate_all_resolutions(Stub(), tx, ty, max_resolution=32, min_resolution=16, batch_size=4, device=gpu_device)
    assert list(out) == [16, 32]
    assert [tuple(s.shape) for s in seen] == [(4, 1, 16, 16), (2, 1, 16, 16), (4, 1, 32, 32), (2, 1, 32, 32)]
    assert torch.equal(seen[0], to_resolution(tx[:4].to(gpu_device), 16)) and torch.equal(seen[3], tx[4:].to(gpu_device))
    from utils.loss import RelativeL2Loss
    want = float(RelativeL2Loss()(0.5 * tx.to(gpu_device), ty.to(gpu_device)))
    assert abs(out[32] - want) <= 1e-6 * abs(want)
