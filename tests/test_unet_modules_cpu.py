"""CPU: models.unet keeps the reference's state_dict layout (names, order, shapes, dtypes as recorded in the fixtures
that tests/golden/make_golden_unet.py wrote from the reference) and loads it with strict=True, the committed fixture
files are the declared cases, both conf/model/unet yamls compose and build, an input whose size is no multiple of 16 is
refused by name, every C entry of csrc/unet.hip reports bad arguments as RPDE_ERR_ARG without a GPU, and the classes
pickle under models.unet."""
import ctypes
import os
import pickle

import pytest
import torch

from tests.conftest import DROPIN
from tests.golden import synth
from tests.golden.unet_cases import BY_NAME, CASES, fixture_files, load_case, state_for

CONF = os.path.join(DROPIN, "conf")
GOLDEN = os.path.join(os.path.dirname(DROPIN), "tests", "golden")


@pytest.mark.parametrize("name", ["unet1d_small_train", "unet1d_gn_3ch", "unet1d_yaml_64", "unet2d_small_train", "unet2d_rect_train"])
def test_state_dict_layout_matches_reference(name):
    from models import unet
    case, spec, _ = load_case(name)
    assert case["ctor"] == BY_NAME[name]["ctor"]
    model = getattr(unet, case["kind"])(**case["ctor"])
    sd = model.state_dict()
    assert synth.spec_of(sd) == spec
    assert list(sd.keys()) == list(spec.keys())
    for key in ("encoder1.enc1conv1.weight", "bottleneck.bottleneckconv2.weight", "upconv4.weight", "upconv1.bias", "conv.bias"):
        assert key in sd
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert (len(tracked) == 0) == bool(case["ctor"].get("use_groupnorm")) and all(sd[k].dtype == torch.int64 for k in tracked)
    assert ("encoder1.enc1norm1.running_mean" in sd) == (not case["ctor"].get("use_groupnorm"))
    missing, unexpected = model.load_state_dict(state_for(spec, case["seed"]), strict=True)
    assert not missing and not unexpected


def test_fixture_cases_are_the_committed_files():
    committed = sorted(f for f in os.listdir(GOLDEN) if f.startswith("unet") and f.endswith(".npz"))
    assert committed == sorted(f for case in CASES for f in fixture_files(case["name"]))
    for case in CASES:
        stored, _, digests = load_case(case["name"])
        assert stored == dict(case, x=tuple(case["x"])), case["name"]
        assert "y" in digests and "dx" in digests and all("floor" in d for d in digests.values())
        assert ("grad/conv.bias" in digests) == (case["grads"] == "all")
        assert any(k.startswith("buf/") for k in digests) == (case["mode"] == "train" and not case["ctor"].get("use_groupnorm"))
        floors = [float(d["floor"]) for d in digests.values() if float(d["floor"]) < 1.0]
        assert max(floors) <= 3.3e-5                     # 3 x floor stays below 1e-4
        for f in fixture_files(case["name"]):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 256 * 1024, f


@pytest.mark.parametrize("yaml,kind,dataset", [("unet/unet_1d", "UNet1d", "synthetic/burgers_1024"),
                                               ("unet/unet_2d", "UNet2d", "synthetic/ns_256")])
def test_yamls_compose_and_build(yaml, kind, dataset):
    from models import unet
    from rpde.config import compose
    from rpde.entry import _model_resolution, build_model
    full = compose(CONF, "config", ["model=" + yaml]).model
    assert {k: v for k, v in full.items() if not k.startswith("_")} == dict(in_channels=1, out_channels=1, width=64)
    assert full["_target_"] == "models.unet." + kind
    args = compose(CONF, "config", ["model=" + yaml, "dataset=" + dataset, "model.width=4"])
    model = build_model(args)
    assert type(model) is getattr(unet, kind) and model.conv.in_channels == 4 and model.upconv4.in_channels == 64
    assert _model_resolution(args) is None           # no resize wrapper: the sweep runs at the model's native resolutions


@pytest.mark.parametrize("kind,shape,size", [("UNet1d", (2, 1, 40), 40), ("UNet2d", (2, 1, 32, 24), 24), ("UNet2d", (2, 1, 8, 32), 8)])
def test_sizes_that_are_no_multiple_of_16_are_refused_by_name(kind, shape, size):
    from models import unet
    model = getattr(unet, kind)(1, 1, 4)
    with pytest.raises(ValueError, match=rf"multiples of 16.*got {size} "):
        model(torch.zeros(shape))


def test_classes_pickle_under_models_unet():
    from models import unet
    for model in (unet.UNet1d(1, 1, 4), unet.UNet1d(3, 2, 4, use_groupnorm=True), unet.UNet2d(2, 1, 4)):
        assert type(model).__module__ == "models.unet"
        again = pickle.loads(pickle.dumps(model))
        assert type(again) is type(model) and list(again.state_dict()) == list(model.state_dict())
    m = unet.UNet1d(1, 1, 4, use_groupnorm=True)
    assert isinstance(m.encoder1.enc1norm1, torch.nn.GroupNorm) and m.encoder1.enc1norm1.num_groups == 4
    assert isinstance(m.pool1, torch.nn.MaxPool1d) and isinstance(m.upconv4, torch.nn.ConvTranspose1d)
    assert isinstance(m.encoder1.enc1tanh1, torch.nn.Tanh) and m.encoder1.enc1conv1.bias is None
    m2 = unet.UNet2d(1, 1, 4)
    assert isinstance(m2.decoder1.dec1norm2, torch.nn.BatchNorm2d) and tuple(m2.upconv1.weight.shape) == (8, 4, 2, 2)


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from rpde import _lib
    lib = _lib.load()
    ERR = _lib.ERR_ARG
    buf = (ctypes.c_float * 64)()                      # host memory: never dereferenced, the checks come first
    p = ctypes.addressof(buf)
    # tanh_pool_fwd(z, scale, shift, act, pooled, B, C, H, W, ky, stream)
    fwd = lib.rpde_unet_tanh_pool_fwd
    assert fwd(None, None, None, p, None, 1, 1, 1, 4, 1, None) == ERR
    assert fwd(p, None, None, None, None, 1, 1, 1, 4, 1, None) == ERR
    assert fwd(p, p, None, p, None, 1, 1, 1, 4, 1, None) == ERR              # scale without shift
    assert fwd(p, None, None, p, None, 0, 1, 1, 4, 1, None) == ERR
    assert fwd(p, None, None, p, None, 1, 1, 1, -4, 1, None) == ERR
    assert fwd(p, None, None, p, None, 1, 1, 1, 4, 3, None) == ERR             # ky is 1 or 2
    assert fwd(p, None, None, p, None, 1, 1, 2, 4, 1, None) == ERR             # the 1-D entry is a plane of one row
    assert fwd(p, None, None, p, None, 1, 1, 1, 1 << 24, 1, None) == ERR
    assert fwd(p, None, None, p, p, 1, 1, 1, 1, 1, None) == ERR                # pooled size 0
    assert fwd(p, None, None, p, p, 1, 1, 1, 8, 2, None) == ERR                # pooled size 0 along H
    assert b"pool" in lib.rpde_last_error()
    # tanh_pool_bwd(act, g_act, g_pool, gy, B, C, H, W, ky, stream)
    bwd = lib.rpde_unet_tanh_pool_bwd
    assert bwd(None, p, p, p, 1, 1, 1, 4, 1, None) == ERR
    assert bwd(p, p, p, None, 1, 1, 1, 4, 1, None) == ERR
    assert bwd(p, None, None, p, 1, 1, 1, 4, 1, None) == ERR                   # both gradients null
    assert b"g_act and g_pool" in lib.rpde_last_error()
    assert bwd(p, p, None, p, 1, 0, 1, 4, 1, None) == ERR
    assert bwd(p, None, p, p, 1, 1, 1, 1, 1, None) == ERR
    # upconv_fwd(x, w, bias, out, B, Cin, Cout, H, W, ky, stream); bwd_data(g, w, gx, ...)
    up = lib.rpde_unet_upconv_fwd
    assert up(None, p, None, p, 1, 1, 1, 1, 4, 1, None) == ERR
    assert up(p, None, None, p, 1, 1, 1, 1, 4, 1, None) == ERR
    assert up(p, p, None, None, 1, 1, 1, 1, 4, 1, None) == ERR
    assert up(p, p, None, p, 1, 0, 1, 1, 4, 1, None) == ERR
    assert up(p, p, None, p, 1, 1, 1, 2, 4, 1, None) == ERR
    assert up(p, p, None, p, 1, 1, 1, 1, 4, 0, None) == ERR
    assert up(p, p, None, p, 1, 1, 1 << 24, 1, 4, 1, None) == ERR
    data = lib.rpde_unet_upconv_bwd_data
    assert data(None, p, p, 1, 1, 1, 1, 4, 1, None) == ERR
    assert data(p, p, None, 1, 1, 1, 1, 4, 1, None) == ERR
    assert data(p, p, p, 1, 1, -1, 1, 4, 1, None) == ERR
    # upconv_bwd_weight(x, g, gw, gb, B, Cin, Cout, H, W, ky, partial, partial_slices, stream)
    wg = lib.rpde_unet_upconv_bwd_weight
    assert wg(None, p, p, None, 1, 1, 1, 1, 4, 1, None, 0, None) == ERR
    assert wg(p, p, None, None, 1, 1, 1, 1, 4, 1, None, 0, None) == ERR
    assert wg(p, p, p, None, 1, 1, 1, 1, 0, 1, None, 0, None) == ERR
    B, Cin, Cout, H, W = 8, 4, 4, 64, 64                                         # few tiles, many points: several slices
    slices = lib.rpde_unet_upconv_bwd_weight_slices(B, Cin, Cout, H, W)
    assert slices > 1 and lib.rpde_unet_upconv_bwd_weight_slices(1, 1024, 512, 4, 4) == 1
    assert lib.rpde_unet_upconv_bwd_weight_slices(0, 4, 4, 4, 4) == 0
    assert wg(p, p, p, None, B, Cin, Cout, H, W, 2, None, 0, None) == ERR        # partial sums needed, none given
    assert wg(p, p, p, None, B, Cin, Cout, H, W, 2, p, slices - 1, None) == ERR
    assert b"slices" in lib.rpde_last_error()
