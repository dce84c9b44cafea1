"""CPU: models.CNO1d keeps the reference's state_dict layout (names, shapes, dtypes as recorded in the fixtures that
tests/golden/make_golden_cno.py wrote from the reference), conf/model/cno_1d/cno_1d.yaml composes, and the entry point
builds the model for the data set's cno_train_size or refuses, naming the key.  (evaluate_all_resolutions' default path
ends in the relative-L2 kernel, which has no CPU form: tests/test_gpu_cno_training.py checks it.)"""
import os

import pytest
import torch

from tests.conftest import DROPIN, load_fixture
from tests.golden import synth
from tests.golden.cno_cases import BY_NAME, CASES, state_for


@pytest.mark.parametrize("name", ["cno1d_small_train", "cno1d_small_nobn", "cno1d_yaml_64"])
def test_state_dict_layout_matches_reference(name):
    from models.CNO1d import CNO1d
    case, spec, _ = load_fixture(name)
    assert case["ctor"] == BY_NAME[name]["ctor"]
    model = CNO1d(**case["ctor"])
    sd = model.state_dict()
    assert synth.spec_of(sd) == spec
    assert list(sd.keys()) == list(spec.keys())
    bn = [k for k in sd if k.endswith("num_batches_tracked")]
    assert (len(bn) > 0) == bool(case["ctor"]["use_bn"]) and all(sd[k].dtype == torch.int64 for k in bn)
    missing, unexpected = model.load_state_dict(state_for(spec, case["seed"]), strict=True)
    assert not missing and not unexpected


def test_fixture_cases_are_the_committed_files():
    for case in CASES:
        stored, _, digests = load_fixture(case["name"])
        assert stored == dict(case, x=tuple(case["x"])), case["name"]
        assert "y" in digests and "dx" in digests and all("floor" in d for d in digests.values())


def test_attribute_names_and_sizes():
    from models.CNO1d import CNO1d, CNO_LReLu, CNOBlock, LiftProjectBlock, ResidualBlock, ResNet
    m = CNO1d(in_dim=2, out_dim=3, size=64, N_layers=3, channel_multiplier=8)
    assert (m.N_layers, m.lift_dim, m.N_res, m.N_res_neck) == (3, 4, 4, 4)
    assert m.encoder_features == [4, 8, 16, 32] and m.decoder_features_in == [32, 32, 16] and m.decoder_features_out == [16, 8, 4]
    assert m.encoder_sizes == [64, 32, 16, 8] and m.decoder_sizes == [8, 16, 32, 64]
    assert isinstance(m.lift, LiftProjectBlock) and isinstance(m.encoder[0], CNOBlock) and isinstance(m.res_net_neck, ResNet)
    blk = m.res_nets[1].res_nets[0]
    assert isinstance(blk, ResidualBlock) and isinstance(blk.act, CNO_LReLu) and (blk.act.in_size, blk.act.out_size) == (32, 32)
    assert (m.ED_expansion[3].in_size, m.ED_expansion[3].out_size) == (8, 8)
    assert isinstance(CNOBlock(2, 2, 8, 8, use_bn=False).batch_norm, torch.nn.Identity)


def test_yaml_composes_and_the_entry_builds_for_cno_train_size():
    from models.CNO1d import CNO1d
    from rpde.config import compose
    from rpde.entry import build_model
    conf = os.path.join(DROPIN, "conf")
    args = compose(conf, "config", ["model=cno_1d/cno_1d", "dataset=synthetic/burgers_1024", "model.N_layers=2", "model.N_res=1"])
    assert args.model["_target_"] == "models.CNO1d.CNO1d" and args.dataset.cno_train_size == 1024
    full = compose(conf, "config", ["model=cno_1d/cno_1d"]).model
    assert {k: v for k, v in full.items() if not k.startswith("_")} == dict(
        in_dim=1, out_dim=1, N_layers=5, N_res=4, N_res_neck=4, channel_multiplier=32, use_bn=True)
    model = build_model(args)
    assert isinstance(model, CNO1d) and model.encoder_sizes == [1024, 512, 256] and model.N_res == 1 and model.N_res_neck == 4


def test_missing_cno_train_size_is_refused_by_name():
    from rpde.config import compose
    from rpde.entry import build_model
    args = compose(os.path.join(DROPIN, "conf"), "config", ["model=cno_1d/cno_1d", "dataset=synthetic/burgers_1024"])
    del args.dataset["cno_train_size"]
    with pytest.raises(SystemExit, match="cno_train_size"):
        build_model(args)
    # the other model families never look at the key
    other = compose(os.path.join(DROPIN, "conf"), "config", ["model=fno_1d/fno_1d", "dataset=synthetic/burgers_1024"])
    del other.dataset["cno_train_size"]
    assert type(build_model(other)).__name__ == "FNO1d"


@pytest.mark.parametrize("name,res", [("burger/burger_generated", 1024), ("ks/ks_generated", 256), ("kdv/kdv_generated", 256)])
def test_generated_dataset_yamls_carry_their_training_resolution(name, res):
    from rpde.config import compose
    ds = compose(os.path.join(DROPIN, "conf"), "config", ["dataset=" + name]).dataset
    assert ds.cno_train_size == res == ds.original_res


_EXPORTED = ("CNO_LReLu", "CNOBlock", "LiftProjectBlock", "ResidualBlock", "ResNet")


@pytest.mark.parametrize("rank", [1, 2])
def test_each_rank_exports_its_own_picklable_classes(rank):
    """both ranks bind one shared module tree; every class still lives under its own module and name, so pickle (and
    with it torch.save(model)) resolves it there"""
    import importlib
    import pickle
    name = f"CNO{rank}d"
    mod = importlib.import_module("models." + name)
    for cls_name in _EXPORTED + (name,):
        cls = getattr(mod, cls_name)
        assert (cls.__module__, cls.__qualname__, cls.__name__) == ("models." + name, cls_name, cls_name)
        assert pickle.loads(pickle.dumps(cls)) is cls


def test_the_ranks_stay_distinct_classes():
    import models.CNO1d
    import models.CNO2d
    assert models.CNO1d.CNOBlock is not models.CNO2d.CNOBlock
    for cls_name in _EXPORTED:
        a, b = getattr(models.CNO1d, cls_name), getattr(models.CNO2d, cls_name)
        assert a is not b and not issubclass(a, b) and not issubclass(b, a)


@pytest.mark.parametrize("rank", [1, 2])
def test_a_model_owns_only_layers_and_classes_of_its_rank(rank):
    import importlib
    nn = torch.nn
    mod = importlib.import_module(f"models.CNO{rank}d")
    own = {1: (nn.Conv1d, nn.BatchNorm1d), 2: (nn.Conv2d, nn.BatchNorm2d)}
    model = getattr(mod, f"CNO{rank}d")(in_dim=1, out_dim=1, size=16, N_layers=2, N_res=1, N_res_neck=1, channel_multiplier=4)
    convs = [m for m in model.modules() if isinstance(m, nn.modules.conv._ConvNd)]
    norms = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert convs and norms
    assert all(type(m) is own[rank][0] for m in convs) and all(type(m) is own[rank][1] for m in norms)
    other = tuple(own[3 - rank])
    assert not any(isinstance(m, other) for m in model.modules())
    # every container in the tree is this module's class, none the other rank's or the shared base itself
    for m in model.modules():
        if type(m).__name__ in _EXPORTED:
            assert type(m).__module__ == mod.__name__ and type(m) is getattr(mod, type(m).__name__)
    # torch.save(model) pickles the classes by module and name
    import io
    buf = io.BytesIO()
    torch.save(model, buf)
    back = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    assert type(back) is type(model) and list(back.state_dict()) == list(model.state_dict())
