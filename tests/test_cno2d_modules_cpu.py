"""CPU: models.CNO2d keeps the reference's state_dict layout (names, shapes, dtypes as recorded in the fixtures that
tests/golden/make_golden_cno2d.py wrote from the reference), the two conf/model/cno_2d yamls compose, the entry point
builds the model for the data set's cno_train_size or refuses, naming the key, and utils.resize_utils.AtResolution
resizes 4-D fields in and out.  (evaluate_all_resolutions ends in the relative-L2 kernel, which has no CPU form:
tests/test_gpu_cno2d_training.py checks the sweep.)"""
import os

import pytest
import torch

from tests.conftest import DROPIN, load_fixture
from tests.golden import synth
from tests.golden.cno2d_cases import BY_NAME, CASES, state_for

CONF = os.path.join(DROPIN, "conf")


@pytest.mark.parametrize("name", ["cno2d_small_train", "cno2d_small_nobn", "cno2d_yaml_32"])
def test_state_dict_layout_matches_reference(name):
    from models.CNO2d import CNO2d
    case, spec, _ = load_fixture(name)
    assert case["ctor"] == BY_NAME[name]["ctor"]
    model = CNO2d(**case["ctor"])
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
        assert os.path.getsize(os.path.join(os.path.dirname(DROPIN), "tests", "golden", case["name"] + ".npz")) < 256 * 1024


def test_attribute_names_and_sizes():
    from models.CNO2d import CNO2d, CNO_LReLu, CNOBlock, LiftProjectBlock, ResidualBlock, ResNet
    m = CNO2d(in_dim=2, out_dim=3, size=64, N_layers=3, channel_multiplier=8)
    assert (m.N_layers, m.lift_dim, m.N_res, m.N_res_neck) == (3, 4, 4, 4)
    assert m.encoder_features == [4, 8, 16, 32] and m.decoder_features_in == [32, 32, 16] and m.decoder_features_out == [16, 8, 4]
    assert m.encoder_sizes == [64, 32, 16, 8] and m.decoder_sizes == [8, 16, 32, 64]
    assert isinstance(m.lift, LiftProjectBlock) and isinstance(m.encoder[0], CNOBlock) and isinstance(m.res_net_neck, ResNet)
    assert isinstance(m.lift.convolution, torch.nn.Conv2d) and isinstance(m.encoder[0].batch_norm, torch.nn.BatchNorm2d)
    assert tuple(m.encoder[0].convolution.weight.shape) == (8, 4, 3, 3)
    blk = m.res_nets[1].res_nets[0]
    assert isinstance(blk, ResidualBlock) and isinstance(blk.act, CNO_LReLu) and (blk.act.in_size, blk.act.out_size) == (32, 32)
    assert (m.ED_expansion[3].in_size, m.ED_expansion[3].out_size) == (8, 8)
    assert isinstance(CNOBlock(2, 2, 8, 8, use_bn=False).batch_norm, torch.nn.Identity)


@pytest.mark.parametrize("yaml,channels,dataset,size", [("cno_2d/cno_2d", 3, "ns/ns_active_generated", 64),
                                                        ("cno_2d/cno_2d_1ch", 1, "synthetic/ns_256", 256),
                                                        ("cno_2d/cno_2d_1ch", 1, "darcy_flow/darcy_generated", 32),
                                                        ("cno_2d/cno_2d_1ch", 1, "ns/ns_generated", 64)])
def test_yamls_compose_and_the_entry_builds_for_cno_train_size(yaml, channels, dataset, size):
    from models.CNO2d import CNO2d
    from rpde.config import compose
    from rpde.entry import _model_resolution, build_model
    full = compose(CONF, "config", ["model=" + yaml]).model
    assert {k: v for k, v in full.items() if not k.startswith("_")} == dict(
        in_dim=channels, out_dim=channels, N_layers=4, N_res=4, N_res_neck=4, channel_multiplier=16, use_bn=False)
    args = compose(CONF, "config", ["model=" + yaml, "dataset=" + dataset, "model.N_layers=2", "model.N_res=1"])
    assert args.model["_target_"] == "models.CNO2d.CNO2d" and args.dataset.cno_train_size == size
    model = build_model(args)
    assert isinstance(model, CNO2d) and model.encoder_sizes == [size, size // 2, size // 4]
    assert (model.in_dim, model.out_dim, model.N_res, model.N_res_neck) == (channels, channels, 1, 4)
    assert _model_resolution(args) == size


def test_missing_cno_train_size_is_refused_by_name():
    from rpde.config import compose
    from rpde.entry import _model_resolution, build_model
    args = compose(CONF, "config", ["model=cno_2d/cno_2d_1ch", "dataset=synthetic/ns_256"])
    del args.dataset["cno_train_size"]
    with pytest.raises(SystemExit, match="CNO2d.*cno_train_size"):
        build_model(args)
    # the other model families never look at the key
    other = compose(CONF, "config", ["model=fno_2d/fno_2d", "dataset=synthetic/ns_256"])
    del other.dataset["cno_train_size"]
    assert type(build_model(other)).__name__ == "FNO2d" and _model_resolution(other) is None


@pytest.mark.parametrize("name,res", [("ns/ns_generated", 64), ("ns/ns_active_generated", 64), ("darcy_flow/darcy_generated", 32)])
def test_generated_dataset_yamls_carry_their_training_resolution(name, res):
    from rpde.config import compose
    ds = compose(CONF, "config", ["dataset=" + name]).dataset
    assert ds.cno_train_size == res == ds.original_res


def test_at_resolution_resizes_4d_fields_in_and_out(monkeypatch):
    """a 4-D field of another size goes through resize(x, (r, r)) on the way in and resize(., its own size) on the way
    out; one already r x r is passed untouched (resize itself is a GPU kernel: stubbed here, its calls recorded)"""
    from utils import resize_utils
    calls, seen = [], []

    def fake_resize(x, size):
        calls.append((tuple(x.shape), tuple(size)))
        return torch.zeros(*x.shape[:2], *size) + float(x.mean())

    def fake_resize_1d(x, n):
        calls.append((tuple(x.shape), n))
        return torch.zeros(*x.shape[:2], n)

    monkeypatch.setattr(resize_utils, "resize", fake_resize)
    monkeypatch.setattr(resize_utils, "resize_1d", fake_resize_1d)

    class Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x)
            return 2.0 * x

    run = resize_utils.AtResolution(Stub(), 16)
    x = torch.ones(2, 3, 32, 32)
    out = run(x)
    assert calls == [((2, 3, 32, 32), (16, 16)), ((2, 3, 16, 16), (32, 32))]
    assert tuple(seen[0].shape) == (2, 3, 16, 16) and tuple(out.shape) == (2, 3, 32, 32) and float(out[0, 0, 0, 0]) == 2.0
    calls.clear()
    own = torch.randn(2, 3, 16, 16)
    assert torch.equal(run(own), 2.0 * own) and seen[-1] is own and calls == []
    rect = run(torch.ones(1, 1, 16, 24))                        # only an exact r x r plane is the model's own
    assert calls == [((1, 1, 16, 24), (16, 16)), ((1, 1, 16, 16), (16, 24))] and tuple(rect.shape) == (1, 1, 16, 24)
    calls.clear()
    run(torch.ones(2, 1, 32))                                   # 1-D fields keep their path
    assert calls == [((2, 1, 32), 16), ((2, 1, 16), 32)]
