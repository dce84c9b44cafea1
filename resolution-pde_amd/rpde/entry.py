"""Shared body of main_1d.py / main_2d.py: compose config, build data, model,
optimiser and scheduler, train, test, checkpoint -- the sequence of the
reference's entry points (main_1d.py:34-309, main_2d.py:38-324) minus wandb and
plotting.  Datasets: synthetic Markov pairs (default), or a file through the
reference's `dataset_params` convention (conf/dataset/ns/ns_file.yaml ->
dataloaders/ns_naive_markov.py)."""
from __future__ import annotations

import json
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.optim as optim

from rpde.config import compose, instantiate


def _init_distributed():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # RPDE_FORCE_DIST=1: join the process group even as a single rank, so that a 1-GPU box exercises the RCCL path
    # (librccl load, communicator init, the gradient all-reduce on the launch stream): tests/test_gpu_rccl.py
    force = os.environ.get("RPDE_FORCE_DIST") == "1"
    if (world > 1 or force) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this driver
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=rank, world_size=world)
    return world, rank, local


def _cno_name(args):
    """CNO1d / CNO2d when the model is one of them, else None"""
    target = str(args.model["_target_"])
    return next((name for name in ("CNO1d", "CNO2d") if target.endswith(name)), None)


def build_model(args):
    """instantiate(args.model); a CNO1d / CNO2d is built for size = dataset.cno_train_size, the resolution it is trained
    at (reference main_1d.py:100-104, main_2d.py:119-124): its levels are sized from it"""
    cno = _cno_name(args)
    if cno is not None:
        size = args.dataset.get("cno_train_size")
        if size is None:
            raise SystemExit(f"model {cno}: the dataset config has no `cno_train_size` (the training resolution, "
                             "which the model's `size` is set to)")
        return instantiate(args.model, size=int(size))
    return instantiate(args.model)


def _model_resolution(args):
    """the resolution the all-resolution sweep resizes to before the model and back after it: CNO's evaluation
    (reference utils/resize_utils.py:527-539 in 1-D, :218-230 in 2-D); None for the models that run at the test
    resolution"""
    return int(args.dataset["cno_train_size"]) if _cno_name(args) is not None else None


def _at_own_resolution(args, model):
    """the model as the rollout and the error-by-frequency sweep call it at every resolution: itself, or a CNO behind
    utils.resize_utils.AtResolution (resized in and out)"""
    from utils.resize_utils import AtResolution
    res = _model_resolution(args)
    return model if res is None else AtResolution(model, res)


def _sweep_fields(args, test_set, x_normalizer, y_normalizer, min_model, max_model, device):
    """What the post-training sweeps (every resolution, error by frequency) evaluate on: (test inputs as the model takes
    them, test targets in physical units, decoder of the model's output or None, evaluation_type, top resolution)."""
    dp = args.dataset.get("dataset_params") or {}
    raw_eval = None
    if dp.get("eval_dataset_target") and args.dataset.get("train_mres"):
        # multi-resolution training evaluates on ONE single-resolution file through another loader (reference
        # utils/naive_utils.py:322-350): un-normalised pairs, encoded here with the training statistics
        keep = ("reduced_batch", "reduced_resolution_t", "use_low_pass_filter", "lowpass_cutoff_ratio", "num_samples_max")
        node = {"_target_": dp["eval_dataset_target"], "filename": dp["eval_filename"],
                "saved_folder": dp.get("eval_saved_folder", dp.get("saved_folder")), "data_normalizer": False,
                **{k: dp[k] for k in keep if k in dp}}
        raw_eval = instantiate(node)[2]
    pairs = [(raw_eval or test_set)[i] for i in range(len(raw_eval or test_set))]
    top_res = max(int(x.shape[-1]) for x, _ in pairs)
    pairs = [(torch.as_tensor(x), torch.as_tensor(y)) for x, y in pairs if int(x.shape[-1]) == top_res]   # a mixed test
    tx, ty = torch.stack([x for x, _ in pairs]), torch.stack([y for _, y in pairs])        # split: highest resolution only
    if raw_eval is not None and x_normalizer is not None:
        tx, ty = x_normalizer.encode(tx), y_normalizer.encode(ty)
    how = str(args.dataset.get("evaluation_type", "naive_downsample"))
    if y_normalizer is not None:
        dec = lambda t: y_normalizer.decode(t, device=device)                                    # noqa: E731
    elif min_model is not None:
        dec = lambda t: t * (max_model - min_model) + min_model                                  # noqa: E731
    else:
        dec = None
    ty_phys = dec(ty.to(device)).cpu() if dec else ty
    return tx, ty_phys, dec, how, top_res


def _etd_residual(eq):
    from utils.loss import EquationResidualLoss
    return EquationResidualLoss(**{k: float(v) for k, v in eq.items()})


def _vorticity_residual(eq):
    from utils.loss import VorticityResidualLoss
    forcing = eq.get("forcing")
    forcing = None if forcing is None or str(forcing).lower() in ("none", "null") else str(forcing)
    return VorticityResidualLoss(float(eq["viscosity"]), float(eq["interval"]), forcing=forcing)


def _darcy_residual(eq):
    from utils.loss import DarcyResidualLoss
    return DarcyResidualLoss(forcing=float(eq.get("forcing", 1.0)), norm=str(eq.get("norm", "dual")))


def _active_scalar_residual(eq):
    from utils.loss import ActiveScalarResidualLoss
    forcing = eq.get("forcing")
    forcing = None if forcing is None or str(forcing).lower() in ("none", "null") else str(forcing)
    return ActiveScalarResidualLoss(float(eq["viscosity"]), float(eq["diffusivity"]), float(eq["buoyancy"]),
                                    float(eq["interval"]), forcing=forcing)


# training.loss=residual, the `equation:` mapping by kind -- None: the 1-D ETD family, which names none --: the rank of
# its grids, the keys it may hold, those it must, the loss it builds and the refusal of any other mapping
_RESIDUALS = {
    None: (1, {"c1", "c2", "c3", "c4", "advect", "length", "interval"}, {"length", "interval"}, _etd_residual,
           "equation needs length and interval and takes c1, c2, c3, c4, advect"),
    "ns_vorticity": (2, {"kind", "viscosity", "interval", "forcing"}, {"viscosity", "interval"}, _vorticity_residual,
                     "a ns_vorticity equation needs viscosity and interval and takes forcing (reference, or none)"),
    "darcy": (2, {"kind", "forcing", "norm"}, {"kind"}, _darcy_residual,
              "a darcy equation takes forcing (a number, default 1.0) and norm (dual, or l2)"),
    "active_scalar": (2, {"kind", "viscosity", "diffusivity", "buoyancy", "interval", "forcing"},
                      {"kind", "viscosity", "diffusivity", "buoyancy", "interval"}, _active_scalar_residual,
                      "an active_scalar equation needs viscosity, diffusivity, buoyancy and interval and takes forcing "
                      "(reference, or none)"),
}


def training_loss(training, dims: int, dataset=None):
    """(name, loss_fn or None) of the optional training objective, from the overrides under `training` (a mapping; no
    device work here); `dataset`: the data set's config, read by training.loss=residual alone.  Absent or "l2": (l2, None), train() then takes RelativeL2Loss.
      training.loss=sobolev   the H^s relative loss (utils.loss.SpectralRelativeL2Loss) with training.loss_s (default
                              1.0) and training.loss_length (a float or one per axis, default 1.0)
      training.loss=band      the relative error band by band (BandRelativeL2Loss) with training.loss_band_floor (1e-3)
      training.loss=spectrum  relative L2 + training.loss_lambda (0.1) x the mismatch of the energy per band
                              (SpectrumMatchingLoss) with training.loss_spectrum_floor (1e-6)
      training.loss=residual  relative L2 + training.loss_lambda (0.1) x the equation residual of the one-step map
                              (EquationResidualLoss in 1-D), built from the data set's `equation:` mapping
                              {c1, c2, c3, c4, advect, length, interval} (length and interval required, the rest
                              default to 0 and advect to 1); in 2-D the mapping {kind: ns_vorticity, viscosity,
                              interval, forcing} (forcing: reference, or none) builds VorticityResidualLoss and
                              {kind: darcy, forcing, norm} (forcing a number, default 1.0; norm dual or l2; only the
                              kind is required; reduced_resolution must be 1) builds DarcyResidualLoss and
                              {kind: active_scalar, viscosity, diffusivity, buoyancy, interval, forcing} (forcing:
                              reference, or none; the rest required) builds ActiveScalarResidualLoss for the
                              three-channel (c, q, v) data; a 2-D mapping without a known kind is refused; run() sets
                              the decode maps (residual_affine)
    band and spectrum take training.loss_bands (octave; radial in 2-D, modes in 1-D) and training.loss_num_bands, and
    the 1-D rollout record then also carries the octave band energies along the rollout.  Anything else: SystemExit.
    Validation, the test score and the sweeps stay relative L2."""
    name = str(training.get("loss", "l2"))
    if name == "l2":
        return name, None
    if name == "sobolev":
        from utils.loss import SpectralRelativeL2Loss
        length = training.get("loss_length", 1.0)
        length = [float(v) for v in length] if isinstance(length, (list, tuple)) else float(length)
        return name, SpectralRelativeL2Loss(dims, "sobolev", s=float(training.get("loss_s", 1.0)), length=length)
    if name == "residual":
        from utils.loss import RelativeL2Loss, SumLoss
        eq = dict((None if dataset is None else dataset.get("equation")) or {})
        kind = eq.get("kind") if dims != 1 else None             # a 1-D mapping names no kind: the key is refused below
        row = _RESIDUALS.get(kind if kind is None else str(kind))
        if dims != 1 and (row is None or row[0] != dims):
            raise SystemExit(f"training.loss=residual: the equation residual is one-dimensional, got dims={dims} (a 2-D data "
                             "set names the vorticity equation: `equation: {kind: ns_vorticity, viscosity, interval, forcing}`"
                             ", the Darcy equation: `equation: {kind: darcy, forcing, norm}`, or the active-scalar system: "
                             "`equation: {kind: active_scalar, viscosity, diffusivity, buoyancy, interval, forcing}`)")
        if not eq:
            raise SystemExit("training.loss=residual: the dataset config has no `equation:` mapping "
                             "({c1, c2, c3, c4, advect, length, interval})")
        _, allowed, required, make, refusal = row
        if set(eq) - allowed or not required <= set(eq):
            raise SystemExit(f"training.loss=residual: {refusal}; got {sorted(eq)}")
        if kind == "darcy":
            # strided samples of the cell centres (i + 1/2) / s are not the cell centres of the coarse grid: the coarse
            # discrete equation does not hold for them (DESIGN.md 10.14 has the figure)
            params = dataset.get("dataset_params") or {}
            if int(params.get("reduced_resolution", 1)) != 1:
                raise SystemExit("training.loss=residual: the Darcy residual needs the generator's own grid, got "
                                 f"dataset_params.reduced_resolution={params.get('reduced_resolution')} (strided cell centres "
                                 "are not the cell centres of the coarse grid)")
        try:
            res = make(eq)
        except ValueError as e:
            raise SystemExit(f"training.loss=residual: {e}")
        return name, SumLoss([(1.0, RelativeL2Loss()), (float(training.get("loss_lambda", 0.1)), res)])
    if name not in ("band", "spectrum"):
        raise SystemExit(f"training.loss={name}: expected l2, sobolev, band, spectrum or residual")
    from utils.loss import BandRelativeL2Loss, RelativeL2Loss, SpectrumMatchingLoss, SumLoss
    bands = str(training.get("loss_bands", "octave"))
    nb = training.get("loss_num_bands", None)
    nb = None if nb is None else int(nb)
    try:
        if name == "band":
            return name, BandRelativeL2Loss(dims, bands, nb, band_floor=float(training.get("loss_band_floor", 1e-3)))
        match = SpectrumMatchingLoss(dims, bands, nb, spectrum_floor=float(training.get("loss_spectrum_floor", 1e-6)))
        return name, SumLoss([(1.0, RelativeL2Loss()), (float(training.get("loss_lambda", 0.1)), match)])
    except ValueError as e:
        raise SystemExit(f"training.loss={name}: {e}")


def residual_affine(loss_fn, x_normalizer, y_normalizer, use_normalizer: bool, minmax: bool = False, ranges=None) -> None:
    """The decode maps of a training.loss=residual objective from the data set's normalisers, so that the equation is
    asked in physical units: the input is decoded with the x-statistics; the prediction with the y-statistics, unless
    training.use_normalizer is true -- train() has decoded it by then and its map is the identity.  Only one global
    affine map folds into the loss: SimpleNormalizer, or min-max normalisation with the loader's four scalar extrema
    `ranges` = (min_data, max_data, min_model, max_model), field * (max - min) + min (four None: the loader did not
    normalise, the identity).  Point-wise normalisers, and min-max without scalar ranges, are a SystemExit."""
    from utils.loss import _ResidualLoss
    from utils.normalizers import scalar_stats
    terms = [t for t in getattr(loss_fn, "terms", [loss_fn]) if isinstance(t, _ResidualLoss)]
    if not terms:
        return
    if minmax and ranges is not None and all(r is None for r in ranges):
        for t in terms:
            t.set_affine()
        return
    if minmax and ranges is not None and len(ranges) == 4 and all(isinstance(r, (int, float)) for r in ranges):
        lo_x, hi_x, lo_y, hi_y = (float(r) for r in ranges)
        for t in terms:
            t.set_affine(pred=(hi_y - lo_y, lo_y), inp=(hi_x - lo_x, lo_x))
        return
    if minmax:
        raise SystemExit("training.loss=residual: min-max normalised data is not supported (normalization_type: simple, "
                         "one global mean and std, is)")
    maps = []
    for norm in (x_normalizer, y_normalizer):
        st = (0.0, 1.0) if norm is None else scalar_stats(norm)
        if st is None:
            raise SystemExit("training.loss=residual: a point-wise normaliser does not fold into the loss "
                             "(normalization_type: simple, one global mean and std, does)")
        maps.append((st[1], st[0]))                              # decode: field * (std + eps) + mean
    for t in terms:
        t.set_affine(pred=(1.0, 0.0) if use_normalizer and y_normalizer is not None else maps[1], inp=maps[0])


def run(dims: int, argv=None):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = compose(os.path.join(here, "conf"), "config", list(sys.argv[1:] if argv is None else argv))
    if int(args.dataset.dims) != dims:
        raise SystemExit(f"main_{dims}d.py needs a {dims}-D dataset config, got dims={args.dataset.dims}")
    world, rank, local = _init_distributed()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    from rpde.launch import limit_host_threads
    limit_host_threads(world)                  # host ops (batch stacking, pinned copies) on the cores this rank may use

    from train.mres_training import ResolutionGroupedDataLoader
    from train.training import evaluate, train
    from utils.synthetic import markov_pairs

    seed = int(args.training.get("seed", 0))
    bs = int(args.training.batch_size)
    x_normalizer = y_normalizer = min_data = max_data = min_model = max_model = rollout_set = None
    normalization_type = "simple"
    if args.dataset.get("dataset_params"):
        # reference main_2d.py:72-82: (train, val, test, *stats); main_1d.py:69-80: (train, val, test, rollout, *stats).
        # stats are (x_normalizer, y_normalizer) or, for Burgers' "minmax", (min_data, max_data, min_model, max_model)
        data_ = instantiate(args.dataset.dataset_params)
        train_set, val_set, test_set = data_[:3]
        if dims == 1:
            rollout_set = data_[3]
        stats = data_[4 if dims == 1 else 3:]
        if len(stats) == 4:
            normalization_type = "minmax"
            min_data, max_data, min_model, max_model = stats
        elif len(stats) == 2:
            x_normalizer, y_normalizer = stats
    else:
        train_set = markov_pairs(args.dataset.resolutions, dims, seed)
        top = max(int(r) for r in dict(args.dataset.resolutions))
        val_set = markov_pairs({top: int(args.dataset.n_val)}, dims, seed + 50000)
        test_set = markov_pairs({top: int(args.dataset.n_test)}, dims, seed + 60000)
    # training: equal rank slices of whole global batches; validation / test: every sample once (ragged rank shares)
    mk = lambda ds, shuffle: ResolutionGroupedDataLoader(ds, bs, shuffle=shuffle, seed=seed, rank=rank,  # noqa: E731
                                                         world_size=world, verbose=rank == 0, drop_last=shuffle)
    train_loader, val_loader, test_loader = mk(train_set, True), mk(val_set, False), mk(test_set, False)

    torch.manual_seed(seed)                                   # same initial weights on every rank
    model = build_model(args).to(device)
    torch.manual_seed(seed + 1 + rank)                        # dropout seeds are drawn from this stream: one per rank
    ckpt = args.dataset.get("saved_checkpoint_path")
    if ckpt:
        state = torch.load(ckpt, map_location=device, weights_only=True)
        model.load_state_dict(state["model_state_dict"])

    # plans for every grid the run will meet -- the training / validation / test groups and the post-training sweep
    # [32 .. max] -- before the first step (no hipMalloc / stream sync inside the training loop)
    from rpde.ops import warm_plans
    from utils.resize_utils import get_lower_resolutions
    seen = {r for ld in (train_loader, val_loader, test_loader) for r in ld.resolution_groups}
    if seen:
        seen |= set(get_lower_resolutions(max(seen), min(32, max(seen))))
        warm_plans(model, seen, dims, in_channels=int(train_set[0][0].shape[0]), device=device)

    lr = float(args.training.learning_rate)
    # torch.optim.AdamW's update rule and state_dict format, one kernel per step (rpde/optim.py)
    from rpde.optim import FlatAdamW
    # training.graph=true (or RPDE_TRAIN_GRAPH=1): train() replays each batch shape's step as one hipGraph -- the optimizer's
    # step state (count, learning rate, weight decay) then lives on the device
    use_graph = bool(args.training.get("graph", False)) or os.environ.get("RPDE_TRAIN_GRAPH") == "1"
    # optional guards of the step (no yaml carries them by default): training.max_grad_norm clips the gradient norm,
    # training.skip_nonfinite drops a step whose norm is NaN / inf; the latter needs the device-side step counter
    max_grad_norm = args.training.get("max_grad_norm", None)
    skip_nonfinite = bool(args.training.get("skip_nonfinite", False))
    guard = dict(max_grad_norm=None if max_grad_norm is None else float(max_grad_norm), skip_nonfinite=skip_nonfinite,
                 capturable=use_graph or skip_nonfinite)
    if dims == 2:     # reference main_2d.py:173-174
        optimizer = FlatAdamW(model.parameters(), lr=lr, **guard)
        scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=30, gamma=0.5)
    else:             # reference main_1d.py:144-145
        optimizer = FlatAdamW(model.parameters(), lr=lr, weight_decay=1e-4, **guard)
        scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=100, eta_min=1e-5)

    # optional training objective (no yaml carries it): training_loss() below
    loss_name, loss_fn = training_loss(args.training, dims, args.dataset)
    if loss_fn is not None:
        residual_affine(loss_fn, x_normalizer, y_normalizer, bool(args.training.use_normalizer), normalization_type == "minmax",
                        ranges=(min_data, max_data, min_model, max_model))
        for r in train_loader.resolution_groups:
            loss_fn.warm((int(r),) * dims, device)

    n_params = sum(p.numel() for p in model.parameters())
    if rank == 0:
        print(json.dumps({"model": args.model["_target_"], "params": n_params, "world": world,
                          "train_batches": len(train_loader), "choices": args["_choices_"]}), flush=True)
    from rpde.launch import freeze_setup_garbage
    freeze_setup_garbage()                     # model, optimizer, datasets are long-lived: keep full collections off them
    t0 = time.time()
    loss_hist, val_hist = train(model, train_loader, val_loader, optimizer, scheduler, y_normalizer=y_normalizer,
                                use_normalizer=bool(args.training.use_normalizer), epochs=int(args.training.epochs),
                                device=device, graph=use_graph, loss_fn=loss_fn)
    torch.cuda.synchronize()
    test_l2 = evaluate(model, test_loader, normalization_type=normalization_type, min_data=min_data, max_data=max_data,
                       min_model=min_model, max_model=max_model, y_normalizer=y_normalizer, device=device)
    if rank == 0:
        print(json.dumps({"train_seconds": round(time.time() - t0, 3), "final_train_loss": loss_hist[-1],
                          "final_val_loss": val_hist[-1], "test_rel_l2": test_l2}), flush=True)

    # ---- the reference's post-training sequence: every resolution [32, .., max] (main_2d.py:287, main_1d.py:250),
    # ---- and in 1-D the autoregressive rollout (main_1d.py:272; utils/autoregressive_step.py:284-309)
    from utils.resize_utils import evaluate_all_resolutions, to_resolution
    tx, ty_phys, dec, how, top_res = _sweep_fields(args, test_set, x_normalizer, y_normalizer, min_model, max_model, device)
    resolution_results = evaluate_all_resolutions(model, tx, ty_phys, max_resolution=top_res, min_resolution=min(32, top_res),
                                                  how=how, batch_size=bs, y_decode=dec, device=device,
                                                  model_resolution=_model_resolution(args))
    rollout_results = rollout_bands = None
    if dims == 1:
        from utils.autoregressive_step import perform_rollout_1d, rollout_loss
        steps = int(args.dataset.get("rollout_steps", 4))
        if rollout_set is not None and len(rollout_set):
            # whole test trajectories of the file [T, X], physical units: encode the start, roll in normalised space
            # (decode with y-statistics, re-encode with x-statistics between steps), compare in physical units
            steps = min(steps, int(rollout_set[0].shape[0]) - 1)
            # (a multi-resolution loader hands over test trajectories of every file resolution: like the mixed test
            #  split above, the rollout is evaluated on the highest one)
            full = [rollout_set[i] for i in range(len(rollout_set)) if int(rollout_set[i].shape[-1]) == top_res]
            mine = full[rank::world]                                                             # this rank's trajectories
            phys = (torch.stack(mine)[:, :steps + 1] if mine else torch.zeros(0, steps + 1, top_res)).to(device)
            if min_data is not None:
                enc = lambda t: (t - min_data) / (max_data - min_data)                           # noqa: E731
                from types import SimpleNamespace
                xn = SimpleNamespace(encode=enc)
                yn = SimpleNamespace(decode=lambda t, device=None: t * (max_model - min_model) + min_model)
            else:
                xn, yn = x_normalizer, y_normalizer
                enc = xn.encode if xn is not None else (lambda t: t)                             # noqa: E731
            traj, decode_pred = phys, (lambda t: yn.decode(t, device=device)) if yn is not None else (lambda t: t)
        else:
            from utils.synthetic import advance
            frames = [tx[rank::world, 0]]
            for _ in range(steps):
                frames.append(advance(frames[-1], 1))
            traj = torch.stack(frames, dim=1).to(device)                       # [n, steps+1, res]
            xn = yn = None
            enc = decode_pred = lambda t: t                                      # noqa: E731
        roller = _at_own_resolution(args, model.eval())
        acc = torch.zeros(len(resolution_results), 2, dtype=torch.float64, device=device)
        # with a banded objective: sums over this rank's trajectories of (E_pred [J], E_true [J], log-ratio mean square)
        # per step, by resolution
        band_acc = {} if loss_name in ("band", "spectrum") else None
        for k, res in enumerate(resolution_results):
            tr = to_resolution(traj, res, "naive_downsample")
            if tr.shape[0]:
                pred = perform_rollout_1d(roller, enc(tr[:, 0]), steps, device=device, x_normalizer=xn, y_normalizer=yn)
                pred = decode_pred(pred)
                acc[k, 0] += rollout_loss(pred, tr) * tr.shape[0]
                acc[k, 1] += tr.shape[0]
            if band_acc is not None:
                from rpde.ops import band_table
                from utils.autoregressive_step import rollout_band_energy
                J = band_table((int(res),), "octave")[1]
                band_acc[res] = torch.zeros(steps, 2 * J + 1, dtype=torch.float64, device=device)
                if tr.shape[0]:
                    st = rollout_band_energy(pred, tr, "octave")
                    band_acc[res] += tr.shape[0] * torch.cat([st["energy_pred"], st["energy_true"],
                                                              st["log_ratio_rms"].view(-1, 1) ** 2], dim=1).to(device)
        if world > 1:
            dist.all_reduce(acc)
            for t in (band_acc or {}).values():
                dist.all_reduce(t)
        rollout_results = {res: (float(acc[k, 0] / acc[k, 1]) if float(acc[k, 1]) > 0 else float("nan"))
                           for k, res in enumerate(resolution_results)}
        if band_acc is not None:
            rollout_bands = {}
            for k, res in enumerate(resolution_results):
                n, t = float(acc[k, 1]), band_acc[res].cpu()
                if n > 0:
                    J = (t.shape[1] - 1) // 2
                    rollout_bands[res] = {"energy_pred": (t[:, :J] / n).tolist(), "energy_true": (t[:, J:2 * J] / n).tolist(),
                                          "log_ratio_rms": (t[:, 2 * J] / n).sqrt().tolist()}
    if rank == 0:
        print(json.dumps({"evaluation_type": how, "resolution_rel_l2": {str(k): v for k, v in resolution_results.items()}}),
              flush=True)
        if rollout_results is not None:
            print(json.dumps({"rollout_rel_l2": {str(k): v for k, v in rollout_results.items()}}), flush=True)
        if rollout_bands is not None:
            print(json.dumps({"rollout_band_energy": {str(k): v for k, v in rollout_bands.items()}}), flush=True)
    run.last = {"test_rel_l2": test_l2, "resolution_rel_l2": resolution_results, "rollout_rel_l2": rollout_results}
    if rollout_bands is not None:
        run.last["rollout_band_energy"] = rollout_bands
    if rank == 0:
        os.makedirs(args.checkpoint_dir, exist_ok=True)
        path = os.path.join(args.checkpoint_dir, f"{args.project_name}_{dims}d.pt")
        torch.save({"model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                    "loss_history": loss_hist, "val_loss_history": val_hist, "l2_loss": test_l2,
                    "resolution_rel_l2": resolution_results}, path)
        print(json.dumps({"checkpoint": path}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return test_l2


def run_frequency(argv=None):
    """Body of frequency_evaluation.py (reference: frequency_evaluation.py / utils/multiresolution_analysis.py, minus the
    plots): load the checkpoint(s) the training entry points write, take the test split through
    utils.frequency_error.evaluate_frequency_error at every resolution [32, .., max] and print ONE JSON document.

    Overrides as in main_1d.py / main_2d.py, plus ``checkpoints=[a.pt,b.pt]`` (default: the reference's
    dataset.model_checkpoints {name: path}, else dataset.saved_checkpoint_path, else
    <checkpoint_dir>/<project_name>_<dims>d.pt), ``num_modes=K`` (1-D) and ``num_radial_bins=N`` (2-D, default 64)."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = compose(os.path.join(here, "conf"), "config", list(sys.argv[1:] if argv is None else argv))
    dims = int(args.dataset.dims)
    world, rank, local = _init_distributed()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    from utils.frequency_error import evaluate_frequency_error
    from utils.resize_utils import get_lower_resolutions
    from utils.synthetic import markov_pairs

    seed = int(args.training.get("seed", 0))
    x_normalizer = y_normalizer = min_model = max_model = None
    if args.dataset.get("dataset_params"):
        data_ = instantiate(args.dataset.dataset_params)
        test_set = data_[2]
        stats = data_[4 if dims == 1 else 3:]
        if len(stats) == 4:
            min_model, max_model = stats[2], stats[3]
        elif len(stats) == 2:
            x_normalizer, y_normalizer = stats
    else:
        top = max(int(r) for r in dict(args.dataset.resolutions))
        test_set = markov_pairs({top: int(args.dataset.n_test)}, dims, seed + 60000)
    tx, ty_phys, dec, how, top_res = _sweep_fields(args, test_set, x_normalizer, y_normalizer, min_model, max_model, device)

    ckpts = args.get("checkpoints") or args.dataset.get("model_checkpoints") or args.dataset.get("saved_checkpoint_path") or \
        os.path.join(args.checkpoint_dir, f"{args.project_name}_{dims}d.pt")
    if isinstance(ckpts, dict):                 # the reference's dataset.model_checkpoints: {name: path}
        ckpts = {str(k): str(v) for k, v in ckpts.items()}
    else:
        ckpts = {str(c): str(c) for c in (ckpts if isinstance(ckpts, (list, tuple)) else [ckpts])}
    resolutions = get_lower_resolutions(top_res, min(32, top_res))
    doc = {"dims": dims, "evaluation_type": how,
           "n_test": int(tx.shape[0]), "resolutions": resolutions, "models": {}}
    for name, path in ckpts.items():
        model = build_model(args).to(device)
        state = torch.load(path, map_location=device, weights_only=True)
        model.load_state_dict(state["model_state_dict"])
        res = evaluate_frequency_error(_at_own_resolution(args, model), tx, ty_phys, resolutions=resolutions, how=doc["evaluation_type"],
                                       batch_size=int(args.training.batch_size), num_modes=args.get("num_modes"),
                                       num_radial_bins=int(args.get("num_radial_bins", 64)), y_decode=dec, device=device)
        doc["models"][name] = {str(r): {"error": e.tolist(), "solution": s.tolist(), "frequencies": f.tolist()}
                               for r, (e, s, f) in res.items()}
    if rank == 0:
        print(json.dumps(doc), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return doc
