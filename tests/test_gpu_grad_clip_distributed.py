"""Two ranks sharing cuda:0 over gloo (the pattern of tests/test_gpu_distributed.py): each rank on its half of the
batch, gradients averaged through the flat bucket, then FlatAdamW(max_grad_norm=...).  The norm is taken after the
average, so both ranks form the same number from the same bytes -- no collective of its own -- and two clipped steps
leave the weights of a single process on the concatenated batch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import DROPIN, REPO
from tests.test_gpu_grad_clip import LR, SMALL, WD, _batch, _loss_fn, _model, _plain_grad_norm, _real

pytestmark = pytest.mark.gpu


def _two_steps(model, opt, batches, exchange):
    """two steps whose scales differ (the second target is SMALL): after the first alone Adam's m / sqrt(v) would hide
    the scale from the weights.  -> the record's (norm, scale) after each step"""
    recs = []
    for k, (x, y) in enumerate(batches):
        opt.zero_grad()
        _loss_fn()(model(x), y * (SMALL if k else 1.0)).backward()
        exchange(opt.bucket)
        opt.step()
        recs.append(opt.grad_stats()[0:2].cpu())
    return torch.stack(recs)


def _setup(dev, bound):
    from rpde.optim import FlatAdamW
    model = _model(dev, seed=3)
    opt = FlatAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=bound)
    return model, opt, [_batch(dev, 4, 40), _batch(dev, 4, 41)]


def _worker(rank, world, port, bound, out):
    for p in (REPO, DROPIN):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, opt, batches = _setup("cuda:0", bound)
    mine = [(x[rank * 2:(rank + 1) * 2], y[rank * 2:(rank + 1) * 2]) for x, y in batches]

    def exchange(bucket):
        bucket.gather()
        flat_cpu = bucket.flat.cpu()                   # gloo reduces host tensors
        dist.all_reduce(flat_cpu)
        bucket.flat.copy_(flat_cpu / world)
    recs = _two_steps(model, opt, mine, exchange)
    weights = torch.cat([_real(p.detach()).reshape(-1) for p in model.parameters()]).cpu()
    torch.save({"recs": recs, "weights": weights}, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_norm_and_match_one_process(gpu_device, tmp_path):
    from rpde.launch import free_port
    model, opt, batches = _setup(gpu_device, 1.0)
    bound = float(np.float32(3.0 * _plain_grad_norm(model, *batches[0])))
    mp.spawn(_worker, args=(2, free_port(), bound, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(str(tmp_path / f"rank{r}.pt"), weights_only=True) for r in (0, 1))
    assert torch.equal(r0["recs"].view(torch.int32), r1["recs"].view(torch.int32))       # the same bytes, the same bits
    assert torch.equal(r0["weights"], r1["weights"])
    model, opt, batches = _setup(gpu_device, bound)
    recs = _two_steps(model, opt, batches, lambda bucket: bucket.gather())
    ref = torch.cat([_real(p.detach()).reshape(-1) for p in model.parameters()]).cpu()
    assert float(recs[0, 1]) == 1.0 and float(recs[1, 1]) < 0.5, recs                  # one unclipped step, one clipped
    # the gradients of the two layouts agree to 1e-5 of their norm (tests/test_gpu_distributed.py); so do norm and scale
    assert bool(((r0["recs"] - recs).abs() <= 1e-5 * recs.abs()).all()), (r0["recs"], recs)
    rel = float((r0["weights"] - ref).norm() / ref.norm())
    assert rel < 1e-5, rel
